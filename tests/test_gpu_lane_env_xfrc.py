"""Batch.set_lane_env_xfrc: the lane = env kernel on a batch whose xfrc_applied has been written (csrc/mjb_lane_env_kernel.h, template flag XF) --
mj_xfrcAccumulate folded into the root -> leaf sweep, the wrenches read from a transposed table (DevState::le_xfrc) -- against the CPU oracle
and against the generic 16-lanes-per-env kernel running the same batch.

Bounds, those the sibling files hold the same comparisons to: one step against the oracle 1e-11 (1 + |x|); rollouts of 60 steps or fewer, and the
lane = env kernel against the generic one, 1e-9 (1 + |x|); energy rtol 1e-7; bit equality where a test says so.  Wrenches: one-step tests draw
f ~ U(-30, 30) N and t ~ U(-5, 5) N m on every body, the world included; rollouts U(-5, 5) and U(-1, 1).  70 envs = one full wavefront and a
6-lane tail; envs 0, 63, 64, 69 go against the oracle where not every env does."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_franka_state
from mujoco_ros_pkgs_amd import mjcf
from test_gpu_lane_env import JIT_ARM, tree_state, two_arm_xml  # noqa: F401  (JIT_ARM: the siblings' other hiprtc model)
from test_gpu_lane_env_params import apply, batch, draw, load, ran_per_env_kernel, states, twin_model

pytestmark = pytest.mark.gpu

NENV = 70
CHECK = (0, 63, 64, 69)
FIELDS = ("qpos", "qvel", "qacc", "sensordata")
NOISE = (20.0, 0.1, 5, 0)


def _err(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if want.size else 0.0


def _close(got, want, tol, what):
    err = _err(got, want)
    print(f"{what}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e}"


def wrenches(nenv, nb, seed, fs, ts):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-fs, fs, (nenv, nb, 3)), rng.uniform(-ts, ts, (nenv, nb, 3))], axis=2).reshape(nenv, 6 * nb)


def moving(model, b):
    """A joint on the body's path to the world."""
    while b > 0:
        if int(model["body_jntnum"][b]) > 0:
            return True
        b = int(model["body_parentid"][b])
    return False


def only(model, X, bodies):
    """X with every body's wrench but those of `bodies` cleared."""
    Y = np.zeros_like(X).reshape(X.shape[0], -1, 6)
    Y[:, list(bodies)] = X.reshape(X.shape[0], -1, 6)[:, list(bodies)]
    return Y.reshape(X.shape)


def make(engine, cm, qpos, qvel, ctrl, xfrc, mode=1, switch=True, noise=None):
    b = batch(engine, cm, mode, qpos, qvel, ctrl)
    if switch is not None:
        b.set_lane_env_xfrc(switch)
    if xfrc is not None:
        b.set("xfrc_applied", xfrc)
    if noise:
        b.set_ctrl_noise(*noise)
    return b


def ran(b, lane):
    assert bool(b.lane_env_info()[1]) == lane, f"lane = env kernel used: {b.lane_env_info()[1]}, expected {lane}"
    if lane:
        assert b.lane_env_last_form() == 0


def oracle(po, model, qpos, qvel, ctrl, xfrc, K, noise=None, env=0):
    d = po.OracleData(model)
    d.reset()
    d.qpos[:] = qpos
    d.qvel[:] = qvel
    if ctrl is not None:
        d.ctrl[:] = ctrl
    if xfrc is not None:
        d.xfrc_applied[:] = xfrc
    for k in range(K):
        if noise:
            d.ctrl_noise(noise[0], noise[1], noise[2], noise[3] + env, k)
        d.step()
    return d


def against_oracle(po, model, b, qpos, qvel, ctrl, X, K, tol, envs, what, noise=None, full=True):
    got = {f: b.get(f) for f in FIELDS + ("energy",)}
    worst = 0.0
    for e in envs:
        d = oracle(po, model, qpos[e], qvel[e], None if ctrl is None else ctrl[e], X[e], K, noise, e)
        for f in (FIELDS if full else ("qpos", "qvel")):
            err = _err(got[f][e], d.field(f))
            worst = max(worst, err)
            assert err <= tol, f"{what} env {e}, {K} steps: {f} {err:.2e} > {tol:.0e}"
        if full and int(model["enableflags"]) & 2:
            assert np.allclose(got["energy"][e], d.energy, rtol=1e-7, atol=1e-8), f"{what} env {e}: energy {got['energy'][e]} vs {d.energy}"
    print(f"{what} K={K}: worst error against the oracle over {len(list(envs))} envs {worst:.2e} (bound {tol:.0e})")
    return got


def against_generic(got, ref, tol, what, fields=FIELDS):
    for f in fields:
        _close(got[f], ref[f], tol, f"{what}: {f} against the generic kernel")


# ------------------------------------------------------------------------------------------------------ 1. the switch and the kernel choice
def test_switch_and_kernel_choice(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    qpos, qvel, ctrl = states("franka_like", base, NENV, 3)
    X = wrenches(NENV, base["nbody"], 5, 30, 5)
    every = FIELDS + ("energy", "time")

    on = make(engine, cm, qpos, qvel, ctrl, X)
    on.step(3)
    ran(on, True)
    # switch off: the generic kernel, bit-equal to a batch that never heard of the switch
    off, never = make(engine, cm, qpos, qvel, ctrl, X, switch=False), make(engine, cm, qpos, qvel, ctrl, X, switch=None)
    for b in (off, never):
        b.step(3)
        ran(b, False)
    for f in every:
        assert np.array_equal(off.get(f), never.get(f)), f
        _close(on.get(f), never.get(f), 1e-9, f"switch on against off, {f}")
    # mode 0 with the switch on: never
    m0 = make(engine, cm, qpos, qvel, ctrl, X, mode=0)
    m0.step(3)
    ran(m0, False)
    for f in every:
        assert np.array_equal(m0.get(f), never.get(f)), f
    for b in (on, off, never, m0):
        b.close()
    # switch on, xfrc_applied never written: the launches of mode 1 without the switch -- the plain build, any form
    lib = engine.binding.load_library()
    for form in (0, 3):
        lib.mjb_lane_env_set_form(form)
        try:
            pair = [make(engine, cm, qpos, qvel, ctrl, None, switch=sw) for sw in (True, None)]
            for b in pair:
                b.step(7)
                assert b.lane_env_info()[1]
            assert pair[0].lane_env_last_form() == pair[1].lane_env_last_form()
            for f in every:
                assert np.array_equal(pair[0].get(f), pair[1].get(f)), (form, f)
            for b in pair:
                b.close()
        finally:
            lib.mjb_lane_env_set_form(-1)


# --------------------------------------------------------------------------------------- 2. one step against the oracle and the generic kernel
@pytest.mark.parametrize("asset,nenv,case", [("franka_like", 70, "every_body"), ("lane_env_tree", 77, "every_body"), ("lane_env_tree", 77, "jointless_body"),
                                             ("franka_like", 70, "bodies_at_rest"), ("lane_env_tree", 77, "bodies_at_rest")])
def test_one_step(oracle_built, asset, nenv, case):
    """every_body: a wrench on every body, the world included.  jointless_body: on lane_env_tree's bracket alone, welded to the moving base -- it has no
    joint of its own and must pass its wrench up.  bodies_at_rest: on the world and on the bodies welded to it alone (franka_like's base; lane_env_tree
    has none but the world) -- nothing moves, and the step equals, bit for bit, the same build's step with a zero wrench written."""
    from mujoco_ros_pkgs_amd import engine
    po = oracle_built
    base = load(asset)
    cm = engine.CompiledModel(base)
    nb = int(base["nbody"])
    qpos, qvel, ctrl = states(asset, base, nenv, 3)
    X = wrenches(nenv, nb, 6, 30, 5)
    if case == "jointless_body":
        weld = [b for b in range(1, nb) if moving(base, b) and int(base["body_jntnum"][b]) == 0]
        assert weld == [base.name2id("body", "bracket")]
        X = only(base, X, weld)
    elif case == "bodies_at_rest":
        rest = [b for b in range(nb) if not moving(base, b)]
        assert rest[0] == 0 and (len(rest) > 1) == (asset == "franka_like")
        X = only(base, X, rest)
    b = make(engine, cm, qpos, qvel, ctrl, X)
    b.step(1)
    ran(b, True)
    got = against_oracle(po, base, b, qpos, qvel, ctrl, X, 1, 1e-11, range(nenv), f"{asset} {case}")
    assert np.array_equal(b.get("xfrc_applied"), X)
    b.close()
    g = make(engine, cm, qpos, qvel, ctrl, X, mode=0)
    g.step(1)
    ran(g, False)
    against_generic(got, {f: g.get(f) for f in FIELDS}, 1e-9, f"{asset} {case}")
    g.close()
    free = make(engine, cm, qpos, qvel, ctrl, np.zeros_like(X))
    free.step(1)
    ran(free, True)
    if case == "bodies_at_rest":
        for f in FIELDS + ("energy",):
            assert np.array_equal(got[f], free.get(f)), f"a wrench on bodies at rest changed {f}"
    else:
        assert _err(got["qacc"], free.get("qacc")) > 1e-3  # (the wrench does act)
    free.close()


# ------------------------------------------------------------------------------------------------------------------- 3. the LDS budgets
@pytest.mark.parametrize("nenv", [16384 + 37, 40000], ids=["80KB", "40KB"])
def test_lds_budgets(oracle_built, nenv):
    """More than one / two wavefronts per CU: the 80 KB and the 40 KB-per-wavefront builds (on a 256-CU device 16 384 < 16 421 <= 32 768 < 40 000)."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    qpos, qvel, ctrl = states("franka_like", base, nenv, 21)
    X = wrenches(nenv, base["nbody"], 22, 5, 1)
    b = make(engine, cm, qpos, qvel, ctrl, X)
    b.step(10)
    ran(b, True)
    got = against_oracle(oracle_built, base, b, qpos, qvel, ctrl, X, 10, 1e-9, (0, 63, 64, nenv // 2 + 5, nenv - 1), f"{nenv} envs")
    for f in FIELDS:
        assert np.all(np.isfinite(got[f])), f
    b.close()


# -------------------------------------------------------------------------------------------------------------------------- 4. rollouts
@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_rollout(oracle_built, asset):
    """60 steps under ctrl noise and a constant wrench: against the oracle on sampled envs and the generic kernel on all; 20 + 20 + 20 is the one
    launch bit for bit; a generic launch in the middle stays within the bound."""
    from mujoco_ros_pkgs_amd import engine
    base = load(asset)
    cm = engine.CompiledModel(base)
    qpos, qvel, _ = states(asset, base, NENV, 9)
    X = wrenches(NENV, base["nbody"], 10, 5, 1)
    every = FIELDS + ("energy", "time", "ctrl")
    res = []
    for plan in ([(1, 60)], [(1, 20), (1, 20), (1, 20)], [(1, 20), (0, 20), (1, 20)], [(0, 60)]):
        b = make(engine, cm, qpos, qvel, None, X, noise=NOISE)
        for mode, k in plan:
            b.set_lane_env(mode)
            b.step(k)
            ran(b, mode == 1)
        if len(res) == 0:
            against_oracle(oracle_built, base, b, qpos, qvel, None, X, 60, 1e-9, CHECK, asset, noise=NOISE)
        res.append({f: b.get(f) for f in every})
        b.close()
    for f in every:
        assert np.array_equal(res[0][f], res[1][f]), f"splitting an XF launch changed {f}"
    against_generic(res[0], res[2], 1e-9, f"{asset} with a generic launch in the middle", every)
    against_generic(res[0], res[3], 1e-9, f"{asset} 60 steps", every)


def test_wrench_changes_between_launches(oracle_built):
    """A new wrench, and then zeros, written between launches act from the next launch on: the generic kernel given the same sequence agrees."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nb = int(base["nbody"])
    qpos, qvel, _ = states("franka_like", base, NENV, 13)
    seq = [wrenches(NENV, nb, 14, 5, 1), wrenches(NENV, nb, 15, 5, 1), np.zeros((NENV, 6 * nb))]
    out = {}
    for mode in (1, 0):
        b = make(engine, cm, qpos, qvel, None, None, mode=mode, noise=NOISE)
        trail = []
        for X in seq:
            b.set("xfrc_applied", X)
            b.step(20)
            ran(b, mode == 1)
            trail.append({f: b.get(f) for f in FIELDS})
        out[mode] = trail
        b.close()
    for k in range(3):
        against_generic(out[1][k], out[0][k], 1e-9, f"leg {k}")
    still = make(engine, cm, qpos, qvel, None, seq[0], noise=NOISE)  # (and the wrench did change something: leg 2 under the first wrench ends elsewhere)
    still.step(40)
    assert _err(still.get("qvel"), out[1][1]["qvel"]) > 1e-6
    still.close()


# ------------------------------------------------------------------------------------------------------------------------ 5. with mode 2
def test_with_per_env_parameters(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    po = oracle_built
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    qpos, qvel, ctrl = states("franka_like", base, NENV, 4)
    R = draw(base, NENV, 7)
    for K, tol, X in ((1, 1e-11, wrenches(NENV, base["nbody"], 8, 30, 5)), (20, 1e-9, wrenches(NENV, base["nbody"], 8, 5, 1))):
        b = make(engine, cm, qpos, qvel, ctrl, X, mode=2)
        apply(b, R)
        b.step(K)
        assert ran_per_env_kernel(b)
        got = {f: b.get(f) for f in FIELDS + ("energy",)}
        worst = 0.0
        for e in range(NENV):
            d = oracle(po, twin_model(base, R, e), qpos[e], qvel[e], ctrl[e], X[e], K)
            for f in FIELDS:
                err = _err(got[f][e], d.field(f))
                worst = max(worst, err)
                assert err <= tol, f"env {e}, {K} steps: {f} {err:.2e} > {tol:.0e}"
            assert np.allclose(got["energy"][e], d.energy, rtol=1e-7, atol=1e-8)
        print(f"mode 2 with wrenches, K={K}: worst error against the twins {worst:.2e} (bound {tol:.0e})")
        b.close()
        # (the overlay matters: the same batch without it ends elsewhere)
    plain = make(engine, cm, qpos, qvel, ctrl, X, mode=2)
    plain.step(20)
    assert _err(plain.get("qvel"), got["qvel"]) > 1e-6
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------------- 6. resets
def test_resets_inside_a_launch(oracle_built):
    """mj_checkPos / mj_checkVel / mj_checkAcc with wrenches set: the NaN qpos and huge qvel cases of test_bad_state_resets_like_mj_step, and env 70
    whose wrench itself is the fault -- f = 1e14 N on the last body drives qacc beyond mjMAXVAL, mj_checkAcc resets the env and the retry runs without
    the wrench.  mj_resetData zeroes xfrc_applied: the reset envs run on without a wrench and find their rows zero after the launch."""
    from mujoco_ros_pkgs_amd import engine
    po = oracle_built
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv, nb = 128, int(base["nbody"])
    qpos, qvel = random_franka_state(base, nenv, 11)
    qpos[5, 2] = np.nan
    qvel[17, 0] = 1e12
    qvel[17, 1] = np.nan
    qpos[40, 0] = np.inf
    qvel[90, 3] = 9e9  # (fine for mj_checkVel, and its qacc stays below mjMAXVAL: no reset)
    ctrl = np.random.default_rng(1).uniform(-5, 5, (nenv, base["nu"]))
    X = wrenches(nenv, nb, 12, 5, 1)
    X[70, 6 * (nb - 1)] = 1e14
    sampled = (5, 17, 40, 70, 90, 0, 127)
    state = ("qpos", "qvel", "ctrl", "time")
    lanes = [make(engine, cm, qpos, qvel, ctrl, X) for _ in range(2)]
    gen = make(engine, cm, qpos, qvel, ctrl, X, mode=0)
    for b in lanes + [gen]:
        b.step(3)
    ran(lanes[0], True)
    ran(gen, False)
    warn = [[b.warning(w) for w in range(8)] for b in (lanes[0], gen)]
    assert warn[0] == warn[1], f"warning counters differ: {warn[0]} vs {warn[1]}"
    assert warn[0][4] == 2 and warn[0][5] == 1 and warn[0][6] >= 1
    got = {f: lanes[0].get(f) for f in state}
    assert np.all(np.isfinite(got["qpos"])) and np.all(np.isfinite(got["qvel"]))
    for f in state:
        _close(got[f], gen.get(f), 1e-9, f"state after the resets, {f}, against the generic kernel")
    twins = {e: oracle(po, base, qpos[e], qvel[e], ctrl[e], X[e], 3) for e in sampled}
    for e, d in twins.items():
        for f in ("qpos", "qvel"):
            _close(got[f][e], d.field(f), 1e-9, f"env {e} {f} against the oracle")
    xf = lanes[0].get("xfrc_applied")
    reset_envs = [e for e in sampled if np.all(twins[e].xfrc_applied == 0)]  # (the oracle's mj_resetData zeroed the env's wrench)
    assert {5, 17, 40, 70} <= set(reset_envs) and 0 not in reset_envs and 127 not in reset_envs
    keep = np.ones(nenv, dtype=bool)
    keep[list(reset_envs)] = False
    assert np.all(xf[list(reset_envs)] == 0), "mj_resetData zeroes xfrc_applied"
    assert np.array_equal(xf[keep], X[keep]), "the other envs' wrenches are untouched"
    # one more step, on this kernel and on the generic one (switched off: it reads the zeroed rows), against the oracle continued
    lanes[1].set_lane_env_xfrc(False)
    for b, lane in zip(lanes, (True, False)):
        b.step(1)
        ran(b, lane)
    for d in twins.values():
        d.step()
    for b, name in zip(lanes, ("lane = env", "generic")):
        q, v = b.get("qpos"), b.get("qvel")
        for e, d in twins.items():
            _close(q[e], d.field("qpos"), 1e-9, f"one more step on the {name} kernel, env {e} qpos")
            _close(v[e], d.field("qvel"), 1e-9, f"one more step on the {name} kernel, env {e} qvel")
    for b in lanes + [gen]:
        b.close()


# ------------------------------------------------------------------------------------------------------------- 7. a topology built by hiprtc
def test_topology_built_by_hiprtc(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    po = oracle_built
    model = mjcf.compile_xml_string(two_arm_xml())
    cm = engine.CompiledModel(model)
    rng = np.random.default_rng(3)
    qpos = rng.uniform(-0.8, 0.8, (NENV, model["nq"]))
    qvel = rng.uniform(-1, 1, (NENV, model["nv"]))
    ctrl = rng.uniform(-2, 2, (NENV, model["nu"]))
    X = wrenches(NENV, model["nbody"], 4, 30, 5)

    def builds(b):
        comp, hits = C.c_int(0), C.c_int(0)
        b.lib.mjb_lane_env_jit_counts(C.byref(comp), C.byref(hits))
        return comp.value + hits.value

    plain = make(engine, cm, qpos, qvel, ctrl, None)
    assert plain.lane_env_info()[0] == -2
    plain.step(1)
    if plain.lane_env_info()[0] == -3 and ("not found" in plain.lane_env_error() or "disabled" in plain.lane_env_error()):
        pytest.skip("hiprtc not available: " + plain.lane_env_error())
    assert plain.lane_env_info()[1], plain.lane_env_error()
    before = builds(plain)
    plain.close()
    b = make(engine, cm, qpos, qvel, ctrl, X)
    b.step(1)
    assert b.lane_env_info()[1], "the XF build of the hiprtc topology did not run: " + b.lane_env_error()
    assert b.lane_env_last_form() == 0
    built = builds(b)
    assert built > before, "the XF build must be a code object of its own in the JIT cache"
    got = against_oracle(po, model, b, qpos, qvel, ctrl, X, 1, 1e-11, range(NENV), "two-arm model")
    b.close()
    again = make(engine, cm, qpos, qvel, ctrl, X)  # a second batch in this process reuses the build
    again.step(1)
    assert again.lane_env_info()[1] and builds(again) == built
    for f in FIELDS:
        assert np.array_equal(again.get(f), got[f]), f
    again.close()


# ---------------------------------------------------------------------------------------------------------------------- 8. range writes
def test_range_writes(oracle_built):
    """The table follows writes of a sub-range of envs: as the very first write of the field, and over a full write."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nb = int(base["nbody"])
    qpos, qvel, ctrl = states("franka_like", base, NENV, 17)
    X1, X2, X3 = (wrenches(NENV, nb, s, 30, 5) for s in (18, 19, 20))
    out = {}
    for mode in (1, 0):
        b = make(engine, cm, qpos, qvel, ctrl, None, mode=mode)
        trail = []
        for X, lo, hi in ((X1, 20, 40), (X2, 0, NENV), (X3, 60, 66), (np.zeros_like(X1), 0, 10)):
            b.set("xfrc_applied", X[lo:hi], lo, hi)
            b.step(1)
            ran(b, mode == 1)
            trail.append({f: b.get(f) for f in FIELDS + ("xfrc_applied",)})
        out[mode] = trail
        b.close()
    want = np.zeros_like(X1)
    for k, (X, lo, hi) in enumerate(((X1, 20, 40), (X2, 0, NENV), (X3, 60, 66), (np.zeros_like(X1), 0, 10))):
        want[lo:hi] = X[lo:hi]
        assert np.array_equal(out[1][k]["xfrc_applied"], want)
        against_generic(out[1][k], out[0][k], 1e-9, f"after write {k}")
    # (each write did act on its range: the first launch moved envs 20 .. 39 away from the wrench-free step and no other env)
    free = make(engine, cm, qpos, qvel, ctrl, None)
    free.step(1)
    d = np.abs(out[1][0]["qacc"] - free.get("qacc")).max(axis=1)
    assert np.all(d[20:40] > 1e-3) and np.all(d[:20] < 1e-9) and np.all(d[40:] < 1e-9)
    free.close()
