"""Device-side episode resets (mjb_episode_*, csrc/mjb_episode.hip) through the Python face: against the host reset (mjb_reset, bit for bit), against the
numpy reference tests/episode_ref.py (EXACT_TOL = 1e-11 in |got - want| / (1 + |want|): the compiler may contract lo + (hi - lo) u, so bit equality with
numpy is not demanded there), against a host-driven loop (bit for bit) and between the lane = env kernel and the generic one (reset states bit for bit,
rollouts 1e-9 as tests/test_gpu_lane_env.py).  Every test prints its figures (pytest -s)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import episode_ref as er
import jacobian_models as jm
from mujoco_ros_pkgs_amd import refdyn

pytestmark = pytest.mark.gpu

EXACT_TOL = 1e-11
ROLLOUT_TOL = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE = ("qpos", "qvel", "act", "ctrl", "qacc_warmstart", "qfrc_applied", "xfrc_applied", "time", "sensordata", "qacc", "ctrlnoise", "mocap_pos", "mocap_quat",
         "energy")
MODELS = ("two_roots", "franka_like", "act_arm", "mocap_world", "empty_world", "franka_table")


@functools.lru_cache(maxsize=None)
def model(name):
    from mujoco_ros_pkgs_amd import mjcf
    if name == "two_roots":
        return jm.model(name)
    if name == "act_arm":
        from test_activation_states import arm
        return arm()
    if name in ("mocap_world", "empty_world"):
        return mjcf.compile_xml_file(os.path.join(GOLDEN, name + ".xml"))
    return mjcf.load_asset(name)     # franka_like; franka_table (PGS, contacts)


@functools.lru_cache(maxsize=None)
def compiled(name):
    from mujoco_ros_pkgs_amd import engine
    return engine.CompiledModel(model(name))


def batch(name, nenv):
    from mujoco_ros_pkgs_amd import engine
    return engine.Batch(compiled(name), nenv)


def start_state(name, n, seed=3, scale=0.05):
    """(qpos, qvel) a little off qpos0 on the manifold, seeded per env"""
    m = model(name)
    q0 = np.asarray(m["qpos0"], float).reshape(int(m["nq"]))
    qpos, qvel = np.zeros((n, int(m["nq"]))), np.zeros((n, int(m["nv"])))
    for e in range(n):
        rng = np.random.default_rng([seed, e])
        qpos[e] = refdyn.integrate_pos(m, q0, scale * rng.normal(size=int(m["nv"])), 1.0)
        qvel[e] = 0.2 * rng.normal(size=int(m["nv"]))
    return qpos, qvel


def stir(b, name, n, seed=3):
    """a state in which every field the reset touches is non-zero, then three steps"""
    m = model(name)
    rng = np.random.default_rng(seed + 100)
    qpos, qvel = start_state(name, n, seed)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if int(m["nu"]):
        b.set("ctrl", rng.uniform(-0.5, 0.5, (n, int(m["nu"]))))
        b.set_ctrl_noise(0.3, 0.1, 77, 0)
    if int(m.get("na", 0)):
        b.set("act", rng.uniform(-0.02, 0.02, (n, int(m["na"]))))
    if int(m["nv"]):
        b.set("qfrc_applied", rng.uniform(-0.1, 0.1, (n, int(m["nv"]))))
    b.set("xfrc_applied", rng.uniform(-0.05, 0.05, (n, 6 * int(m["nbody"]))))
    if int(m.get("nmocap", 0)):
        b.set("mocap_pos", b.get("mocap_pos") + rng.uniform(-0.05, 0.05, (n, 3 * int(m["nmocap"]))))
        w = rng.normal(size=(n, int(m["nmocap"]), 4))
        b.set("mocap_quat", (w / np.linalg.norm(w, axis=-1, keepdims=True)).reshape(n, -1))
    b.step(3)


def snapshot(b):
    return {f: b.get(f) for f in STATE}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_same_state(A, B, what, rows=None):
    for f in STATE:
        a, b = (A[f], B[f]) if rows is None else (A[f][rows], B[f][rows])
        assert same_bits(a, b), f"{what}: {f} differs in {int(np.sum(np.any(bits(a) != bits(b), axis=1)))} envs"


def device_mask(mask):
    """a torch uint8 tensor on the device, complete before its address is used on another stream"""
    import torch
    t = torch.tensor(np.asarray(mask, dtype=np.uint8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def corner_mask(n):
    """envs 0, 63, 64 and the last -- the edges of the kernel's 64-env groups -- and none of their neighbours"""
    mask = np.zeros(n, dtype=np.uint8)
    mask[[e for e in (0, 63, 64, n - 1) if e < n]] = 1
    return mask


SIZES = [(name, n) for name in MODELS for n in ((1, 63, 64, 65, 131) if name in ("two_roots", "franka_like") else (65, 131))]


@pytest.mark.parametrize("name,n", SIZES, ids=[f"{a}-{b}" for a, b in SIZES])
def test_equals_the_host_reset(name, n):
    """No bank, no noise, no rule: episode_reset(device mask) after three steps leaves every state field of every env -- reset or not -- with the bits
    mjb_reset(host mask) leaves in a twin batch.  The mask is a torch tensor, or (131 envs) the done buffer of a third batch.
    Measured on the MI355X: 0 differing words in every case; ndone = the mask's population."""
    A, B = batch(name, n), batch(name, n)
    try:
        stir(A, name, n)
        stir(B, name, n)
        before = snapshot(A)
        assert_same_state(before, snapshot(B), "twins before the reset")
        mask = corner_mask(n)
        if n == 131:     # the mask is what another batch's launch wrote
            third = batch(name, n)
            third.episode_reset(mask)
            assert np.array_equal(third.episode_done(), mask)
            A.episode_reset(third.episode_device_ptr("done"))
            A.synchronize()
            third.close()
        else:
            t = device_mask(mask)
            A.episode_reset(t.data_ptr())
            A.synchronize()
        B.reset(mask)
        after = snapshot(A)
        assert_same_state(after, snapshot(B), "episode_reset against mjb_reset")
        assert_same_state(after, before, "envs outside the mask", rows=mask == 0)
        assert np.array_equal(A.episode_done(), mask) and A.episode_ndone() == int(mask.sum())
        assert np.array_equal(A.episode_counts(), mask.astype(np.uint32))
        m = model(name)
        if int(m["nq"]):
            assert same_bits(after["qpos"][mask == 1], np.tile(np.asarray(m["qpos0"], float), (int(mask.sum()), 1)))
        changed = sum(int(np.any(bits(after[f][mask == 1]) != bits(before[f][mask == 1]))) for f in STATE)
        print(f"{name}, {n} envs: {int(mask.sum())} reset, {changed} of {len(STATE)} fields changed by it, 0 words differ from mjb_reset")
        assert changed >= (5 if name in ("two_roots", "franka_like") else 2)
    finally:
        A.close()
        B.close()


def noise_ranges(name):
    m = model(name)
    nv = int(m["nv"])
    d = np.arange(nv)
    return (-0.3 - 0.01 * d, 0.2 + 0.02 * d), (-1.0 + 0.03 * d, 0.5 + 0.01 * d)


def bank(name, ninit=5):
    """(qpos, qvel, act or None) of an initial-state bank: jacobian_models' seeded states; the activation arm (limited joints, na > 0) gets its own"""
    if name != "act_arm":
        return tuple(np.array(x) for x in jm.states(name, ninit)) + (None,)
    q, v = start_state(name, ninit, seed=31, scale=0.3)
    return q, v, np.random.default_rng(32).uniform(-0.02, 0.02, (ninit, int(model(name)["na"])))


@pytest.mark.parametrize("name", ["two_roots", "franka_like", "act_arm"])
def test_bank_noise_and_clamp_against_the_reference(name):
    """A bank of five rows, ranges non-zero on every dof (rotations included), clamp on: the reset envs' qpos, qvel and act against episode_ref, the picked
    rows, a second reset at episode 1, the counters.
    Measured on the MI355X (65 envs, 33 reset), worst error at episode 0 / 1: two_roots 1.43e-16 / 1.42e-16, franka_like 1.10e-16 / 1.08e-16, act_arm
    1.33e-16 / 1.22e-16 with 30 / 32 coordinates on a limit (the other two models have no limited joint); quaternion norms off 1 by at most 2.22e-16;
    every picked row the reference's."""
    m = model(name)
    n, seed, offset = 65, 0x5EED0123456789, 1000
    nq, nv = int(m["nq"]), int(m["nv"])
    bq, bv, ba = bank(name)     # (two_roots and franka_like have no limited joint: the arm is where the clamp bites)
    qr, vr = noise_ranges(name)
    mask = np.zeros(n, dtype=np.uint8)
    mask[::2] = 1
    A, X = batch(name, n), batch(name, n)
    try:
        for b in (A, X):
            stir(b, name, n)
            b.set_episode_init(bq, bv, ba)
        A.set_episode_noise(seed, qpos_range=qr, qvel_range=vr, clamp=True, env_offset=offset)
        X.set_episode_noise(seed, env_offset=offset)      # the rows alone: qvel comes back as the bank has it
        X.episode_reset(mask)
        xv = X.get("qvel")
        rows = [int(np.flatnonzero([same_bits(xv[e], bv[k]) for k in range(5)])[0]) for e in np.flatnonzero(mask)]
        want_rows = [er.pick(seed, offset + e, 0, nv, 5) for e in np.flatnonzero(mask)]
        assert rows == want_rows and len(set(rows)) == 5
        assert same_bits(X.get("qpos")[mask == 1], bq[rows]) and (ba is None or same_bits(X.get("act")[mask == 1], ba[rows]))
        before = snapshot(A)
        first = None
        for episode in (0, 1):
            A.episode_reset(mask)      # (a host mask: uploaded by the Python face)
            got = snapshot(A)
            worst, qn, clamped = 0.0, 0.0, 0
            for e in np.flatnonzero(mask):
                q, v, a, k = er.reset_state(m, seed, offset + e, episode, bank=(bq, bv, ba), qpos_range=qr, qvel_range=vr, do_clamp=True)
                worst = max(worst, er.rel_err(got["qpos"][e], q), er.rel_err(got["qvel"][e], v), er.rel_err(got["act"][e], a))
                for j in range(int(m["njnt"])):
                    ty, qa = int(m["jnt_type"][j]), int(m["jnt_qposadr"][j])
                    if ty in (refdyn.JNT_FREE, refdyn.JNT_BALL):
                        o = qa + (3 if ty == refdyn.JNT_FREE else 0)
                        qn = max(qn, abs(np.linalg.norm(got["qpos"][e][o:o + 4]) - 1))
                    elif int(m["jnt_limited"][j]):
                        lo, hi = (float(x) for x in m["jnt_range"][j])
                        assert lo <= got["qpos"][e][qa] <= hi
                        clamped += got["qpos"][e][qa] in (lo, hi)
            print(f"{name}, episode {episode}: worst error {worst:.2e} (bound {EXACT_TOL:.0e}), |quat| - 1 up to {qn:.2e}, {clamped} coordinates on a limit")
            assert worst <= EXACT_TOL and qn <= EXACT_TOL
            assert clamped > 0 or name != "act_arm"
            for f in ("ctrl", "ctrlnoise", "qacc_warmstart", "qfrc_applied", "xfrc_applied", "qacc", "sensordata", "time", "energy"):
                assert not got[f][mask == 1].any(), f
            assert_same_state(got, before, "envs outside the mask", rows=mask == 0)
            if first is not None:
                assert np.all(np.any(bits(got["qpos"][mask == 1]) != bits(first["qpos"][mask == 1]), axis=1)), "episode 1 repeats episode 0"
                assert np.all(np.any(bits(got["qvel"][mask == 1]) != bits(first["qvel"][mask == 1]), axis=1))
            first = got
        assert np.array_equal(A.episode_counts(), 2 * mask.astype(np.uint32))
    finally:
        A.close()
        X.close()


def test_keyed_by_global_env_not_by_batch_shape():
    """One seed: the first 131 envs of a 300-env batch equal a 131-env batch, and a 131-env batch at env_offset 7 equals envs 7.. of the 300-env batch, to
    the bit (two_roots, bank of five rows, noise on every dof, two episodes).  Measured on the MI355X: 0 differing words."""
    name = "two_roots"
    bq, bv = (np.array(x) for x in jm.states(name, 5))
    qr, vr = noise_ranges(name)
    out = {}
    for key, n, off in (("big", 300, 0), ("small", 131, 0), ("shifted", 131, 7)):
        b = batch(name, n)
        try:
            b.set_episode_init(bq, bv)
            b.set_episode_noise(42, qpos_range=qr, qvel_range=vr, env_offset=off)
            res = []
            for _ in range(2):
                b.episode_reset()
                res.append((b.get("qpos"), b.get("qvel")))
            assert b.episode_ndone() == n and np.all(b.episode_counts() == 2)
            out[key] = res
        finally:
            b.close()
    for ep in range(2):
        for k in range(2):
            assert same_bits(out["big"][ep][k][:131], out["small"][ep][k])
            assert same_bits(out["big"][ep][k][7:138], out["shifted"][ep][k])
    assert not same_bits(out["big"][0][0], out["big"][1][0])
    print("two_roots: 300 / 131 / 131 @ 7 envs, two episodes: 0 words differ")


def test_done_rule():
    """two_roots, 131 envs, K = 3: per-env starting times with the limit halfway between two step times; a box on a hinge coordinate and on the free
    joint's z, violated from either side; one coordinate set to NaN between the launches; an extra mask.  done equals the reference's decisions from the
    time and qpos read back before the call, ndone their sum, the envs that are not done keep their bits, the done ones start over.
    Measured on the MI355X: 131 decisions equal, 72 done (time 52, box 8, NaN 1, extra 22, with overlaps)."""
    name, n, K = "two_roots", 131, 3
    m = model(name)
    nq, dt = int(m["nq"]), float(m["timestep"][0])
    hinge = int(m["jnt_qposadr"][list(m["names"]["joint"]).index("a1j")])
    z = int(m["jnt_qposadr"][list(m["names"]["joint"]).index("fj")]) + 2
    lo, hi = np.full(nq, -np.inf), np.full(nq, np.inf)
    lo[hinge], hi[hinge], lo[z], hi[z] = -0.5, 0.5, 0.5, 1.5
    b = batch(name, n)
    try:
        qpos, qvel = start_state(name, n)
        qpos[[3, 64], hinge] = 0.9
        qpos[[40, 130], hinge] = -0.9
        qpos[[5, 63], z] = 1.9
        qpos[[66, 100], z] = 0.1
        b.set("qpos", qpos)
        b.set("qvel", 0.1 * qvel)
        b.set("time", ((np.arange(n) % 10) * dt)[:, None])
        b.set_episode_rule(time_limit=8.5 * dt, qpos_box=(lo, hi))
        b.step(K)
        q = b.get("qpos")
        q[77, hinge + 1] = np.nan
        b.set("qpos", q)
        extra = (np.arange(n) % 6 == 1).astype(np.uint8)
        before = snapshot(b)
        want = er.done_rule(before["time"], before["qpos"], 8.5 * dt, (lo, hi), extra)
        parts = [int(er.done_rule(before["time"], before["qpos"], 8.5 * dt).sum()), int(er.done_rule(before["time"], np.where(np.isnan(q), 0.0, q), 0.0, (lo, hi)).sum()),
                 int(np.isnan(before["qpos"]).any(axis=1).sum()), int(extra.sum())]
        t = device_mask(extra)
        b.episode_step(t.data_ptr())
        done = b.episode_done()
        after = snapshot(b)
        print(f"two_roots, {n} envs: {int(done.sum())} done (time {parts[0]}, box {parts[1]}, NaN {parts[2]}, extra {parts[3]}, with overlaps)")
        assert np.array_equal(done, want)
        assert b.episode_ndone() == int(want.sum()) and 0 < want.sum() < n
        assert parts[0] and parts[1] == 8 and parts[2] == 1 and want[77] and want[[3, 64, 40, 130, 5, 63, 66, 100]].all()
        assert_same_state(after, before, "envs that are not done", rows=want == 0)
        assert same_bits(after["qpos"][want == 1], np.tile(np.asarray(m["qpos0"], float), (int(want.sum()), 1)))
        assert not after["time"][want == 1].any() and not after["qvel"][want == 1].any()
        assert np.array_equal(b.episode_counts(), want.astype(np.uint32))
        # no rule at all: nothing is done, nothing changes
        b.set_episode_rule()
        b.episode_step()
        assert b.episode_ndone() == 0 and not b.episode_done().any()
        assert_same_state(snapshot(b), after, "a launch without a done env")
    finally:
        b.close()


@pytest.mark.parametrize("name,n", [("franka_table", 67), ("franka_like", 131)])
def test_closed_loop_equals_the_host_driven_loop(name, n):
    """40 launches of K = 5 with episode_step between them (one-row bank, no noise, the time rule) against a twin driven from the host: get("time"),
    reset(mask), set("qpos" / "qvel").  All state equal to the bit after every launch and after every reset, warmstart of the reset envs zero, everything
    finite.  Measured on the MI355X: franka_table (PGS) 67 envs 385 resets, franka_like 131 envs 754 resets, 0 differing words."""
    m = model(name)
    K, launches, dt = 5, 40, float(m["timestep"][0])
    q0, v0 = start_state(name, 1, seed=9, scale=0.03)
    limit = 32.5 * dt
    rng = np.random.default_rng(21)
    A, B = batch(name, n), batch(name, n)
    try:
        qpos, qvel = start_state(name, n, seed=5, scale=0.03)
        for b in (A, B):
            b.set("qpos", qpos)
            b.set("qvel", qvel)
            b.set("time", ((np.arange(n) % 33) * dt)[:, None])
        A.set_episode_init(q0, v0)
        A.set_episode_rule(time_limit=limit)
        resets = 0
        for it in range(launches):
            ctrl = rng.uniform(-0.3, 0.3, (n, int(m["nu"])))
            for b in (A, B):
                b.set("ctrl", ctrl)
                b.step(K)
            assert_same_state(snapshot(A), snapshot(B), f"launch {it}")
            A.episode_step()
            mask = (B.get("time")[:, 0] >= limit).astype(np.uint8)
            B.reset(mask)
            q, v = B.get("qpos"), B.get("qvel")
            q[mask == 1], v[mask == 1] = q0[0], v0[0]
            B.set("qpos", q)
            B.set("qvel", v)
            sa = snapshot(A)
            assert_same_state(sa, snapshot(B), f"reset after launch {it}")
            assert np.array_equal(A.episode_done(), mask) and A.episode_ndone() == int(mask.sum())
            assert not sa["qacc_warmstart"][mask == 1].any()
            assert all(np.all(np.isfinite(sa[f])) for f in STATE)
            resets += int(mask.sum())
        assert resets > 2 * n and int(A.episode_counts().sum()) == resets
        print(f"{name}, {n} envs, {launches} launches of {K}: {resets} resets, 0 words differ from the host-driven loop")
    finally:
        A.close()
        B.close()


def test_lane_env_kernel_between_episode_steps():
    """franka_like, 4096 envs, set_lane_env(1) against a set_lane_env(0) twin: launches of K = 5 alternate with episode_step (bank, noise on, the time
    rule).  The lane = env kernel ran; the done sets are equal and the states of the reset envs right after each reset equal to the bit; the rollouts
    agree within 1e-9.  Measured on the MI355X: 8 launches, 4014 resets, rollouts apart by at most 1.36e-15."""
    name, n, K = "franka_like", 4096, 5
    m = model(name)
    dt = float(m["timestep"][0])
    bq, bv = (np.array(x) for x in jm.states(name, 5))
    d = np.arange(int(m["nv"]))
    qr, vr = (-0.05 - 0.001 * d, 0.04 + 0.002 * d), (-0.3, 0.2)
    qpos, qvel = start_state(name, n, seed=13, scale=0.03)
    A, B = batch(name, n), batch(name, n)
    try:
        for b, mode in ((A, 1), (B, 0)):
            b.set_lane_env(mode)
            b.set("qpos", qpos)
            b.set("qvel", qvel)
            b.set("time", ((np.arange(n) % 50) * dt)[:, None])
            b.set_episode_init(bq, bv)
            b.set_episode_noise(2024, qpos_range=qr, qvel_range=vr, clamp=True)
            b.set_episode_rule(time_limit=40.5 * dt)
        worst, resets = 0.0, 0
        for it in range(8):
            A.step(K)
            B.step(K)
            assert A.lane_env_info()[1] and not B.lane_env_info()[1]
            for f in ("qpos", "qvel"):
                worst = max(worst, er.rel_err(A.get(f), B.get(f)))
            A.episode_step()
            B.episode_step()
            done = A.episode_done()
            assert np.array_equal(done, B.episode_done())
            for f in ("qpos", "qvel", "time", "qacc_warmstart", "ctrl"):
                assert same_bits(A.get(f)[done == 1], B.get(f)[done == 1]), (it, f)
            resets += int(done.sum())
        print(f"franka_like, {n} envs, lane = env against generic: {resets} resets, rollouts apart by at most {worst:.2e} (bound {ROLLOUT_TOL:.0e})")
        assert worst <= ROLLOUT_TOL and resets > n // 2
    finally:
        A.close()
        B.close()


def test_contract():
    """MJB_EINVAL for a NaN bank entry, a zero quaternion, lo > hi, a negative ninit and an env range outside the batch; derived fields, cast_rays and
    jacobians refuse after an episode call until forward(); the live-resource count returns to its start after close(); an unknown `which` gives NULL
    with a message."""
    from mujoco_ros_pkgs_amd import engine
    name = "two_roots"
    m = model(name)
    nq, nv = int(m["nq"]), int(m["nv"])
    cm = compiled(name)
    lib = cm.lib
    live0 = lib.mjb_debug_live_resources()
    b = batch(name, 70)
    pd = C.POINTER(C.c_double)
    EINVAL = -1
    try:
        good = np.array(jm.states(name, 2)[0])
        bad = good.copy()
        bad[1, 0] = np.nan
        assert lib.mjb_episode_set_init(b.ptr, 2, bad.ctypes.data_as(pd), None, None) == EINVAL and b"non-finite" in lib.mjb_last_error()
        bad = good.copy()
        bad[0, 3:7] = 0     # the free joint's quaternion
        assert lib.mjb_episode_set_init(b.ptr, 2, bad.ctypes.data_as(pd), None, None) == EINVAL and b"zero quaternion" in lib.mjb_last_error()
        assert lib.mjb_episode_set_init(b.ptr, -1, good.ctypes.data_as(pd), None, None) == EINVAL
        lo, hi = np.zeros(nv), np.zeros(nv)
        lo[4] = 1e-3
        assert lib.mjb_episode_set_noise(b.ptr, 1, 0, lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), None, None, 0) == EINVAL
        hi[4] = np.inf
        assert lib.mjb_episode_set_noise(b.ptr, 1, 0, None, None, lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), 0) == EINVAL
        assert lib.mjb_episode_get(b.ptr, 0, 71, None, None, None) == EINVAL and lib.mjb_episode_get(b.ptr, -1, 3, None, None, None) == EINVAL
        with pytest.raises(engine.EngineError):
            b.set_episode_noise(1, qpos_range=(0.1, -0.1))
        assert lib.mjb_episode_device_ptr(b.ptr, 3) is None and b"which" in lib.mjb_last_error()
        with pytest.raises(engine.EngineError):
            b.episode_device_ptr(7)
        assert b.episode_device_ptr("done") and b.episode_device_ptr("episode") and b.episode_device_ptr("ndone")
        # a refused configuration leaves the one before it in place: no bank, no noise
        b.set_rays("s_world", [[0.0, 0.0, -1.0]])
        b.set_jac_points([("site", "s_a2")])
        for call in (b.episode_reset, b.episode_step):
            b.forward()
            assert b.get("xpos").shape[0] == 70 and b.cast_rays()[0].shape == (70, 1) and b.jacobians()["J"].shape == (70, 1, 6, nv)
            call()
            for refused in (lambda: b.get("xpos"), b.cast_rays, b.jacobians):
                with pytest.raises(engine.EngineError):
                    refused()
        assert same_bits(b.get("qpos"), np.tile(np.asarray(m["qpos0"], float), (70, 1)))
        b.forward()
        assert np.all(np.isfinite(b.get("xpos")))
        assert lib.mjb_debug_live_resources() > live0
    finally:
        b.close()
    assert lib.mjb_debug_live_resources() == live0
