"""Batch.set_lane_env(2): the lane = env kernel on a batch that carries per-env gravity, masses, joint and actuator parameters -- every env
reads its own values from the per-env table (DevState::le_overlay).  Method of tests/test_gpu_env_joint_params.py and tests/test_gpu_env_params.py:
each env against the oracle on its own twin model from the same state.  Tolerances are those the sibling tests hold the same comparisons to:
one step 1e-11 (1 + |x|), 100 steps 1e-8, five steps 1e-10 and unrandomised neighbours 1e-9 (test_large_batch_kernel_choice),
the generic kernel over 60 noisy steps 1e-9 (tests/test_gpu_lane_env.py), energy rtol 1e-7."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import random_franka_state
from mujoco_ros_pkgs_amd import mjcf
from test_gpu_env_joint_params import KEYS, FIELDS, _err, _oracle_steps, randomised, twin
from test_gpu_lane_env import JIT_ARM, tree_state

pytestmark = pytest.mark.gpu

ALL = ("gravity", "mass", "joint", "actuator")
JOINT_KEYS, ACT_KEYS = ("damping", "armature", "stiffness"), ("gainprm", "biasprm")


def load(asset):
    m = mjcf.load_asset(asset)
    m["enableflags"] = int(m["enableflags"]) | 2  # mjENBL_ENERGY
    return m


def states(asset, model, nenv, seed):
    qpos, qvel = (random_franka_state if asset == "franka_like" else tree_state)(model, nenv, seed)
    ctrl = np.random.default_rng(seed + 1).uniform(-3, 3, (nenv, model["nu"]))
    return qpos, qvel, ctrl


def draw(base, nenv, seed, which=ALL, keep0=True):
    """Per-env values of the four families; a family not in `which` keeps the model's.  Env 0 keeps the model's unless keep0 is False."""
    n = nenv + (0 if keep0 else 1)
    rng = np.random.default_rng(seed + 100)
    P = randomised(base, n, seed)
    for k in KEYS:
        if (k in JOINT_KEYS and "joint" not in which) or (k in ACT_KEYS and "actuator" not in which):
            P[k][:] = np.asarray(base[FIELDS[k]], dtype=np.float64)[None]
    scale = rng.uniform(0.5, 2.0, (n, base["nbody"]))
    grav = np.tile(np.asarray(base["gravity"], dtype=np.float64), (n, 1))
    g = rng.uniform(-1, 1, (n, 3)) * [2.0, 2.0, 3.0] + [0, 0, -7.0]
    if "mass" not in which:
        scale[:] = 1.0
    if "gravity" in which:
        grav[1:] = g[1:]
    scale[0] = 1.0
    mass = np.asarray(base["body_mass"], dtype=np.float64)[None] * scale
    inertia = np.asarray(base["body_inertia"], dtype=np.float64).reshape(1, -1, 3) * scale[:, :, None]  # (uniform density change)
    cut = slice(0 if keep0 else 1, None)
    return SimpleNamespace(P={k: P[k][cut] for k in KEYS}, mass=mass[cut], inertia=inertia[cut], grav=grav[cut], which=which)


def apply(b, R, lo=1, hi=None):
    """Only the setters of the families drawn: a gravity-only batch has no parameter block and the other way round."""
    hi = b.nenv if hi is None else hi
    P = R.P
    if "gravity" in R.which:
        b.set_env_gravity(R.grav[lo:hi], lo, hi)
    if "mass" in R.which:
        b.set_env_body_mass(R.mass[lo:hi], R.inertia[lo:hi], lo=lo, hi=hi)
    if "joint" in R.which:
        b.set_env_dof_params(P["damping"][lo:hi], P["armature"][lo:hi], None, lo=lo, hi=hi)
        b.set_env_joint_stiffness(P["stiffness"][lo:hi], lo=lo, hi=hi)
    if "actuator" in R.which:
        b.set_env_actuator_params(P["gainprm"][lo:hi], P["biasprm"][lo:hi], lo=lo, hi=hi)


def twin_model(base, R, e):
    m = mjcf.Model(dict(twin(mjcf.with_body_mass(base, R.mass[e], R.inertia[e]), R.P, e)))
    m["gravity"] = R.grav[e].copy()
    return m


def batch(engine, cm, mode, qpos, qvel, ctrl=None):
    b = engine.Batch(cm, qpos.shape[0])
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if ctrl is not None:
        b.set("ctrl", ctrl)
    return b


def ran_per_env_kernel(b):
    return bool(b.lane_env_info()[1]) and b.lane_env_last_form() == 0


def against_twins(po, base, R, b, qpos, qvel, ctrl, K, tol, envs, full=False, what=""):
    got = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata", "energy")}
    worst = 0.0
    for e in envs:
        d = _oracle_steps(po, twin_model(base, R, e), qpos[e], qvel[e], None if ctrl is None else ctrl[e], K)
        fields = [("qpos", d.qpos), ("qvel", d.qvel)]
        if full:
            fields += [("qacc", d.field("qacc")), ("sensordata", d.field("sensordata")), ("energy", d.energy)]
        for f, want in fields:
            err = _err(got[f][e], want)
            worst = max(worst, err)
            assert err <= tol, f"{what} env {e}, {K} steps: {f} {err:.2e} > {tol:.0e}"
        assert np.allclose(got["energy"][e], d.energy, rtol=1e-7, atol=1e-8), f"{what} env {e}: energy {got['energy'][e]} vs {d.energy}"
    print(f"{what} K={K}: worst error over {len(list(envs))} envs {worst:.2e} (bound {tol:.0e})")
    return got


# ---------------------------------------------------------------------------------------------------- 1. the mode
def test_mode_2_is_accepted_and_used(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv = 70  # one full wavefront and a 6-lane tail
    qpos, qvel, ctrl = states("franka_like", base, nenv, 3)
    R = draw(base, nenv, 5)
    b = batch(engine, cm, 2, qpos, qvel, ctrl)
    apply(b, R)
    b.step(1)
    assert b.lane_env_info()[1], "mode 2: a batch with per-env overrides runs the lane = env kernel"
    assert b.lane_env_last_form() == 0
    for mode in (1, -1):
        b.set_lane_env(mode)
        b.step(1)
        assert not b.lane_env_info()[1], f"mode {mode}: a batch with overrides runs the generic kernel"
    with pytest.raises(engine.EngineError):
        b.set_lane_env(3)
    b.close()
    # without overrides mode 2 is mode 1, bit for bit
    plain = [batch(engine, cm, mode, qpos, qvel, ctrl) for mode in (1, 2)]
    for p in plain:
        p.step(7)
        assert p.lane_env_info()[1]
    for f in ("qpos", "qvel", "qacc", "sensordata", "energy"):
        assert np.array_equal(plain[0].get(f), plain[1].get(f)), f
    for p in plain:
        p.close()


# ---------------------------------------------------------------------------------------------------- 2. every env against its twin
@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_every_env_matches_its_twin(oracle_built, asset):
    from mujoco_ros_pkgs_amd import engine
    base = load(asset)
    cm = engine.CompiledModel(base)
    nenv = 70
    qpos, qvel, ctrl = states(asset, base, nenv, 4)
    R = draw(base, nenv, 7)
    for K, tol in ((1, 1e-11), (100, 1e-8)):
        b = batch(engine, cm, 2, qpos, qvel, ctrl)
        apply(b, R)
        b.step(K)
        assert ran_per_env_kernel(b)
        against_twins(oracle_built, base, R, b, qpos, qvel, ctrl, K, tol, range(nenv), full=K == 1, what=asset)
        b.close()


# ---------------------------------------------------------------------------------------------------- 3. one family at a time
@pytest.fixture(scope="module")
def franka5(oracle_built):
    """franka_like, 70 envs, five steps without overrides (mode 1): what a family's overrides must move the batch away from."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    qpos, qvel, ctrl = states("franka_like", base, 70, 6)
    b = batch(engine, cm, 1, qpos, qvel, ctrl)
    b.step(5)
    assert b.lane_env_info()[1]
    plain = (b.get("qpos"), b.get("qvel"))
    b.close()
    return SimpleNamespace(engine=engine, base=base, cm=cm, qpos=qpos, qvel=qvel, ctrl=ctrl, plain=plain)


@pytest.mark.parametrize("family", ALL)
def test_one_family_at_a_time(oracle_built, franka5, family):
    f5 = franka5
    R = draw(f5.base, 70, 11, which=(family,))
    b = batch(f5.engine, f5.cm, 2, f5.qpos, f5.qvel, f5.ctrl)
    apply(b, R)
    b.step(5)
    assert ran_per_env_kernel(b)
    got = against_twins(oracle_built, f5.base, R, b, f5.qpos, f5.qvel, f5.ctrl, 5, 1e-10, range(70), what=family)
    moved = max(np.abs(got["qpos"][1:] - f5.plain[0][1:]).max(), np.abs(got["qvel"][1:] - f5.plain[1][1:]).max())
    print(f"{family}: moves the batch by {moved:.2e}")
    assert moved > 1e-6, f"{family}: the override does not reach the kernel ({moved:.2e})"
    np.testing.assert_allclose(got["qpos"][0], f5.plain[0][0], rtol=0, atol=1e-9)  # (env 0 keeps the model's values)
    b.close()


# ---------------------------------------------------------------------------------------------------- 4. lane placement
def test_lane_placement(oracle_built):
    """Overrides on the first and last lane of a wavefront, the first lane of the next and the last live lane of a tail; their neighbours keep the model's."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv, K = 130, 5
    qpos, qvel, ctrl = states("franka_like", base, nenv, 8)
    R = draw(base, nenv, 13, keep0=False)
    own, others = (0, 63, 64, 129), (1, 62, 65, 128)
    for e in range(nenv):
        if e not in own:
            for k in KEYS:
                R.P[k][e] = np.asarray(base[FIELDS[k]], dtype=np.float64)
            R.mass[e], R.inertia[e] = base["body_mass"], np.asarray(base["body_inertia"], dtype=np.float64).reshape(-1, 3)
            R.grav[e] = base["gravity"]
    b = batch(engine, cm, 2, qpos, qvel, ctrl)
    for e in own:
        apply(b, R, lo=e, hi=e + 1)
    b.step(K)
    assert ran_per_env_kernel(b)
    got = against_twins(oracle_built, base, R, b, qpos, qvel, ctrl, K, 1e-10, own, what="lane placement")
    p = batch(engine, cm, 1, qpos, qvel, ctrl)
    p.step(K)
    assert p.lane_env_info()[1]
    pq, pv = p.get("qpos"), p.get("qvel")
    for e in others:
        assert _err(got["qpos"][e], pq[e]) <= 1e-9 and _err(got["qvel"][e], pv[e]) <= 1e-9, f"env {e} (no overrides) vs the mode-1 batch"
    for e in own:
        assert max(np.abs(got["qpos"][e] - pq[e]).max(), np.abs(got["qvel"][e] - pv[e]).max()) > 1e-6, f"env {e}: overrides not seen"
    b.close()
    p.close()


# ---------------------------------------------------------------------------------------------------- 5. against the generic kernel
def test_against_the_generic_kernel(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv, K = 70, 60
    qpos, qvel, _ = states("franka_like", base, nenv, 9)
    R = draw(base, nenv, 17)
    out = {}
    for mode in (0, 2):
        b = batch(engine, cm, mode, qpos, qvel)
        apply(b, R)
        b.set_ctrl_noise(5.0, 0.1, 777, 1000)
        b.step(K)
        assert b.lane_env_info()[1] == (mode == 2)
        out[mode] = (b.get("qpos"), b.get("qvel"))
        b.close()
    eq, ev = _err(out[2][0], out[0][0]), _err(out[2][1], out[0][1])
    print(f"mode 2 vs the generic kernel, {K} noisy steps: qpos {eq:.2e} qvel {ev:.2e}")
    assert eq <= 1e-9 and ev <= 1e-9


# ---------------------------------------------------------------------------------------------------- 6. launch splits
def test_launch_splits(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv = 70
    qpos, qvel, _ = states("franka_like", base, nenv, 10)
    R = draw(base, nenv, 19)

    def fresh():
        b = batch(engine, cm, 2, qpos, qvel)
        apply(b, R)
        b.set_ctrl_noise(5.0, 0.1, 99, 0)
        return b
    fields = ("qpos", "qvel", "qacc", "sensordata", "time", "ctrl")
    whole = fresh()
    whole.step(6)
    assert ran_per_env_kernel(whole)
    ref = {f: whole.get(f) for f in fields}
    two = fresh()
    two.step(2)
    two.step(4)
    assert ran_per_env_kernel(two)
    for f in fields:
        assert np.array_equal(two.get(f), ref[f]), f"step(2); step(4) vs step(6): {f}"
    for ncb in (0, 5):  # the host runtime's split step: envs [0, ncb) in two halves on the generic kernels, the rest fused
        s = fresh()
        for _ in range(6):
            assert s.lib.mjb_step1_prefix(s.ptr, ncb) == 0
            assert s.lib.mjb_step_rest(s.ptr, ncb) == 0
            assert ran_per_env_kernel(s)
            assert s.lib.mjb_step2_prefix(s.ptr, ncb) == 0
        for f in fields:
            x = s.get(f)
            assert np.array_equal(x[ncb:], ref[f][ncb:]), f"prefix {ncb} + rest vs whole-batch steps: {f}"
            assert np.allclose(x[:ncb], ref[f][:ncb], rtol=0, atol=1e-9 * (1 + np.abs(ref[f]).max())), f"prefix envs (generic kernels): {f}"
        s.close()
    whole.close()
    two.close()


# ---------------------------------------------------------------------------------------------------- 7. a setter between two launches
def test_setter_between_launches(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv = 70
    qpos, qvel, ctrl = states("franka_like", base, nenv, 12)
    R = draw(base, nenv, 23)
    b, same = (batch(engine, cm, 2, qpos, qvel, ctrl) for _ in range(2))
    for x in (b, same):
        apply(x, R)
        x.step(3)
    R2 = draw(base, nenv, 23)
    R2.P["damping"][5] = R.P["damping"][5] * 2.5 + 0.3
    R2.grav[5] = [1.5, -0.5, -3.7]
    b.set_env_dof_params(R2.P["damping"][5:6], lo=5, hi=6)
    b.set_env_gravity(R2.grav[5:6], 5, 6)
    for x in (b, same):
        x.step(3)
        assert ran_per_env_kernel(x)
    d = _oracle_steps(oracle_built, twin_model(base, R, 5), qpos[5], qvel[5], ctrl[5], 3)
    d = _oracle_steps(oracle_built, twin_model(base, R2, 5), np.array(d.qpos), np.array(d.qvel), ctrl[5], 3)
    eq, ev = _err(b.get("qpos")[5], d.qpos), _err(b.get("qvel")[5], d.qvel)
    print(f"env 5, model changed after step 3: qpos {eq:.2e} qvel {ev:.2e}")
    assert eq <= 1e-10 and ev <= 1e-10
    assert np.abs(b.get("qvel")[5] - same.get("qvel")[5]).max() > 1e-6, "the setter call is not visible in the next launch"
    for f in ("qpos", "qvel"):
        assert np.array_equal(np.delete(b.get(f), 5, axis=0), np.delete(same.get(f), 5, axis=0)), f"{f}: another env changed"
    b.close()
    same.close()


# ---------------------------------------------------------------------------------------------------- 8. resets
def test_reset_keeps_the_overrides(oracle_built):
    """As test_bad_state_resets_like_mj_step: bad qpos / qvel reset the env (mj_checkPos / mj_checkVel); it then steps with its own parameters."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    nenv = 70
    qpos, qvel, ctrl = states("franka_like", base, nenv, 14)
    R = draw(base, nenv, 29)
    qpos[5, 2] = np.nan
    qvel[17, 0] = 1e12
    qvel[17, 1] = np.nan
    qpos[40, 0] = np.inf
    got = {}
    for mode in (2, 0):
        b = batch(engine, cm, mode, qpos, qvel, ctrl)
        apply(b, R)
        b.step(3)
        assert b.lane_env_info()[1] == (mode == 2)
        got[mode] = (b.get("qpos"), b.get("qvel"), b.get("ctrl"), b.get("time"), [b.warning(w) for w in range(8)])
        b.close()
    assert got[2][4] == got[0][4], f"warning counters differ: {got[2][4]} vs {got[0][4]}"
    assert got[2][4][4] == 2 and got[2][4][5] == 1
    for a, c in zip(got[2][:4], got[0][:4]):
        assert np.all(np.isfinite(a)) and _err(a, c) <= 1e-9, "state after resets, mode 2 vs the generic kernel"
    for e in (5, 17, 40, 6):
        d = _oracle_steps(oracle_built, twin_model(base, R, e), qpos[e], qvel[e], ctrl[e], 3)
        assert _err(got[2][0][e], d.qpos) <= 1e-9 and _err(got[2][1][e], d.qvel) <= 1e-9, f"env {e} vs its twin"
    plain = _oracle_steps(oracle_built, base, qpos[5], qvel[5], ctrl[5], 3)
    assert _err(got[2][1][5], plain.qvel) > 1e-6  # (after the reset env 5 falls under ITS gravity, not the model's)


# ---------------------------------------------------------------------------------------------------- 9. the leaner LDS budgets
@pytest.mark.parametrize("nenv", [20000, 40000], ids=["80KB", "40KB"])
def test_lean_lds_variants(oracle_built, nenv):
    """More than one / two wavefronts per CU: the 80 KB and the 40 KB-per-wavefront builds (test_lean_lds_variant_at_full_occupancy; on a 256-CU device
    16 384 < 20 000 <= 32 768 < 40 000).  Case 2 on sampled envs, at one step and at a hundred.  Gravity, damping, stiffness and gains differ in every env;
    masses and armature (a mj_setConst derivation per env on the host) in the sampled ones."""
    from mujoco_ros_pkgs_amd import engine
    base = load("franka_like")
    cm = engine.CompiledModel(base)
    qpos, qvel, ctrl = states("franka_like", base, nenv, 21)
    R = draw(base, nenv, 31)
    sampled = (63, 64, 12345, nenv - 1)
    keep = np.ones(nenv, dtype=bool)
    keep[list(sampled)] = False
    R.mass[keep], R.inertia[keep] = base["body_mass"], np.asarray(base["body_inertia"], dtype=np.float64).reshape(-1, 3)
    R.P["armature"][keep] = np.asarray(base["dof_armature"], dtype=np.float64)
    for K, tol in ((1, 1e-11), (100, 1e-8)):
        b = batch(engine, cm, 2, qpos, qvel, ctrl)
        b.set_env_gravity(R.grav[1:], 1, nenv)
        b.set_env_dof_params(R.P["damping"][1:], lo=1, hi=nenv)
        b.set_env_joint_stiffness(R.P["stiffness"][1:], lo=1, hi=nenv)
        b.set_env_actuator_params(R.P["gainprm"][1:], R.P["biasprm"][1:], lo=1, hi=nenv)
        for e in sampled:
            b.set_env_body_mass(R.mass[e:e + 1], R.inertia[e:e + 1], lo=e, hi=e + 1)
            b.set_env_dof_params(armature=R.P["armature"][e:e + 1], lo=e, hi=e + 1)
        b.step(K)
        assert ran_per_env_kernel(b)
        got = against_twins(oracle_built, base, R, b, qpos, qvel, ctrl, K, tol, (0,) + sampled, full=K == 1, what=f"{nenv} envs")
        assert np.all(np.isfinite(got["qpos"])) and np.all(np.isfinite(got["qvel"]))
        b.close()


# ---------------------------------------------------------------------------------------------------- 10. a topology built by hiprtc
def test_topology_built_by_hiprtc(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    xml = JIT_ARM.replace('actuator="3"', 'actuator="act3"').replace('<motor joint="j4" forcelimited', '<motor name="act3" joint="j4" forcelimited')
    base = mjcf.compile_xml_string(xml)
    base["enableflags"] = int(base["enableflags"]) | 2
    cm = engine.CompiledModel(base)
    nenv = 70
    rng = np.random.default_rng(8)
    qpos = np.tile(np.asarray(base["qpos0"], dtype=np.float64), (nenv, 1)) + rng.uniform(-0.7, 0.7, (nenv, base["nq"])) * np.where(np.asarray(base["jnt_type"]) == 3, 1.0, 0.05)
    qvel = rng.uniform(-1, 1, (nenv, base["nv"]))
    ctrl = rng.uniform(-2, 2, (nenv, base["nu"]))
    R = draw(base, nenv, 37)
    b = batch(engine, cm, 2, qpos, qvel, ctrl)
    assert b.lane_env_info()[0] == -2
    apply(b, R)
    b.step(1)
    topo, used = b.lane_env_info()
    if topo == -3:
        why = b.lane_env_error()
        assert "compile failed" not in why, why  # (a kernel that does not compile is a failure, a box without hiprtc is not)
        pytest.skip("hiprtc build not available on this box: " + why)
    assert used and b.lane_env_last_form() == 0
    against_twins(oracle_built, base, R, b, qpos, qvel, ctrl, 1, 1e-11, range(nenv), full=True, what="hiprtc arm")
    comp, hits = C.c_int(0), C.c_int(0)
    b.lib.mjb_lane_env_jit_counts(C.byref(comp), C.byref(hits))
    built = comp.value + hits.value
    assert built >= 1
    again = batch(engine, cm, 2, qpos, qvel, ctrl)  # a second batch in this process reuses the build
    apply(again, R)
    again.step(1)
    assert again.lane_env_info()[1]
    again.lib.mjb_lane_env_jit_counts(C.byref(comp), C.byref(hits))
    assert comp.value + hits.value == built
    for f in ("qpos", "qvel", "qacc"):
        assert np.array_equal(again.get(f), b.get(f)), f
    b.close()
    again.close()
