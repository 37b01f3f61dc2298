"""Form 3 on four wavefronts with the frame wavefront X taken off the sweep's pacing path (csrc/mjb_lane_env_kernel.h, roles 8 - 11): X no longer
computes cdof -- it reads the six doubles C publishes for V from the two-deep ring, one phase after C wrote them and one before C overwrites them --
and whether a joint's anchor is off centre (jnt_pos != 0) is a flag of the topology (jnt_offc), not a run-time test.

What that could break: the ring's parities (lane_env_tree: two trees, a jointless body in mid-chain, slides whose angular half V and X zero), the
flag's true branch (lane_env_tree, and a franka_like with a moved anchor, which hiprtc builds), X's qM -- so qacc, mj_checkAcc's verdicts, the retry
trip, energy --, and nothing else: sensors, the force block and the OU state are checked because the same launch produces them.  "Three wavefronts" =
the same inputs under mjb_lane_env_set_sweep_waves(3), whose code is untouched.

Bounds are the project's own (tests/test_gpu_lane_env.py, tests/test_gpu_lane_env_qacc_split.py): one step <= 1e-11 (relative + absolute) against the
oracle, rollouts <= 1e-9 against the oracle and the generic kernel, two instantiations of the kernel on the same inputs <= 1e-12, launch splits and
untouched lanes bit for bit, warning counters exactly.
"""
import numpy as np
import pytest

from conftest import random_franka_state
from test_gpu_lane_env import _close, make, tree_state

pytestmark = pytest.mark.gpu

DSBL_PASSIVE = 1 << 5
DSBL_ACTUATION = 1 << 10
DSBL_EULERDAMP = 1 << 14
ENBL_ENERGY = 2
ALL = ("qpos", "qvel", "qacc", "sensordata", "energy")
STATE = ("qpos", "qvel", "ctrl", "time")
# qvel[3] of a franka_like env: mj_checkAcc passes the first step (|qacc| ~ 1e9) and trips in the SECOND (the oracle: anywhere in 1e4 .. 1e5)
TRIPS_AT_STEP_2 = 3e4


@pytest.fixture(scope="module")
def eng(oracle_built):
    from mujoco_ros_pkgs_amd import engine, mjcf
    return engine, mjcf, oracle_built


@pytest.fixture
def lib(eng):
    """Form 3 requested for the test; the rule again afterwards."""
    lib = eng[0].binding.load_library()
    lib.mjb_lane_env_set_form(3)
    yield lib
    lib.mjb_lane_env_set_form(-1)
    lib.mjb_lane_env_set_sweep_waves(0)


def _ran(lib, waves):
    assert lib.mjb_lane_env_last_form() == 3 and lib.mjb_lane_env_last_sweep_waves() == waves, (
        lib.mjb_lane_env_last_form(), lib.mjb_lane_env_last_sweep_waves(), waves)


def _run(eng, lib, cm, qpos, qvel, ctrl, plan, waves, fields, noise=None, every=False):
    """Launches of plan[0], plan[1], ... steps: waves = 3 / 4 -> form 3 on that many wavefronts, 0 -> the generic kernel.  Returns the fields and the
    eight warning counters."""
    nenv = qpos.shape[0]
    if waves:
        lib.mjb_lane_env_set_sweep_waves(waves)
    b = make(eng[0], cm, nenv, qpos, qvel, 1 if waves else 0, ctrl)
    if every:
        b.set_sensors_every_step(True)
    if noise:
        b.set_ctrl_noise(*noise)
    for k in ([plan] if isinstance(plan, int) else plan):
        b.step(k)
        if waves:
            assert b.lane_env_info()[1]
            _ran(lib, waves)
    out = {f: b.get(f) for f in fields}
    out["warn"] = [b.warning(w) for w in range(8)]
    b.close()
    return out


def _state(model, asset, nenv, seed):
    return (random_franka_state if asset == "franka_like" else tree_state)(model, nenv, seed)


def _model(eng, asset, disable=0):
    engine, mjcf, _ = eng
    model = mjcf.load_asset(asset)
    model["enableflags"] = int(model["enableflags"]) | ENBL_ENERGY
    model["disableflags"] = int(model["disableflags"]) | disable
    return model, engine.CompiledModel(model)


def _four_vs_three(eng, lib, cm, qpos, qvel, K, noise, what):
    got = {w: _run(eng, lib, cm, qpos, qvel, None, K, w, ALL, noise) for w in (3, 4)}
    for f in ALL:
        print(f"{what}, {K} noise steps, {f}: max |four - three wavefronts| = {np.abs(got[4][f] - got[3][f]).max():.3e}")
    for f in ALL:
        assert np.all(np.isfinite(got[4][f])), f
        if f == "qacc":   # (|qacc| reaches 1e3 under this noise: relative + absolute, as tests/test_gpu_lane_env_qacc_split.py holds it)
            _close(got[4][f], got[3][f], 1e-12, f"{what} {f} after {K} noise steps, four wavefronts vs three")
        else:
            assert np.abs(got[4][f] - got[3][f]).max() <= 1e-12, f"{what} {f} after {K} noise steps, four wavefronts vs three"
    assert got[4]["warn"] == got[3]["warn"]


@pytest.mark.parametrize("asset,nenv,K,std", [("franka_like", 64, 200, 43.5), ("lane_env_tree", 33, 300, 1.5)])
def test_four_against_three_wavefronts(eng, lib, asset, nenv, K, std):
    """The same inputs through both instantiations.  lane_env_tree: off-centre anchors (the flag's true branch), a jointless mid-chain body and two trees
    (the cdof ring's parities do not follow the body ids)."""
    model, cm = _model(eng, asset)
    qpos, qvel = _state(model, asset, nenv, 3)
    _four_vs_three(eng, lib, cm, qpos, qvel, K, (std, 0.1, 777, 1000), asset)


@pytest.fixture(scope="module")
def oracle_33(eng):
    """Both topologies, 33 envs: the oracle after one step (constant ctrl) and after 50 noise steps, computed once."""
    _, mjcf, po = eng
    ref = {}
    for asset, std in (("franka_like", 43.5), ("lane_env_tree", 1.5)):
        model = mjcf.load_asset(asset)
        model["enableflags"] = int(model["enableflags"]) | ENBL_ENERGY
        nenv = 33
        qpos, qvel = _state(model, asset, nenv, 3)
        ctrl = np.random.default_rng(4).uniform(-3, 3, (nenv, model["nu"]))
        one = {f: [] for f in ALL}
        for e in range(nenv):
            d = po.OracleData(model)
            d.reset()
            d.qpos[:] = qpos[e]
            d.qvel[:] = qvel[e] * 3
            d.ctrl[:] = ctrl[e]
            d.step(1)
            for f in ALL:
                one[f].append(np.array(d.field(f), dtype=np.float64).copy())
        noise = (std, 0.1, 777, 1000)
        roll = po.rollout(model, qpos, qvel, 50, noise_std=std, noise_rate=0.1, seed=777, env_offset=1000, nthreads=8)
        ref[asset] = dict(model=model, qpos=qpos, qvel=qvel, ctrl=ctrl, noise=noise, one={f: np.array(v) for f, v in one.items()}, roll=roll)
    return ref


@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_one_step_against_the_oracle(eng, lib, oracle_33, asset):
    r = oracle_33[asset]
    cm = eng[0].CompiledModel(r["model"])
    got = _run(eng, lib, cm, r["qpos"], r["qvel"] * 3, r["ctrl"], 1, 4, ALL)
    for f in ALL:
        print(f"{asset}, one step, {f}: max |four wavefronts - oracle| = {np.abs(got[f] - r['one'][f].reshape(got[f].shape)).max():.3e}")
    for f in ALL:
        _close(got[f], r["one"][f].reshape(got[f].shape), 1e-11, f"{asset} {f} after one step vs the oracle")


@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_fifty_noise_steps_against_the_oracle(eng, lib, oracle_33, asset):
    r = oracle_33[asset]
    cm = eng[0].CompiledModel(r["model"])
    got = _run(eng, lib, cm, r["qpos"], r["qvel"], None, 50, 4, ("qpos", "qvel", "sensordata"), r["noise"])
    oq, ov, osd = r["roll"]
    for f, o in (("qpos", oq), ("qvel", ov), ("sensordata", osd)):
        print(f"{asset}, 50 noise steps, {f}: max |four wavefronts - oracle| = {np.abs(got[f] - o).max():.3e}")
    for f, o in (("qpos", oq), ("qvel", ov), ("sensordata", osd)):
        _close(got[f], o, 1e-9, f"{asset} {f} after 50 noise steps vs the oracle")


@pytest.mark.parametrize("with_reset", [False, True], ids=["plain", "with_reset"])
def test_launch_splits_agree_bit_for_bit(eng, lib, with_reset):
    """70 envs: the second block has 6 live lanes.  K = 50 at once, as 25 + 25 and as 50 launches of one step."""
    model, cm = _model(eng, "franka_like")
    nenv = 70
    qpos, qvel = random_franka_state(model, nenv, 9)
    if with_reset:
        qvel[66, 3] = 9e9   # (a lane of the tail block: mj_checkAcc in the first step)
    fields = STATE + ("qacc", "sensordata", "energy")
    res = [_run(eng, lib, cm, qpos, qvel, None, plan, 4, fields, (20.0, 0.1, 5, 0)) for plan in ([50], [25, 25], [1] * 50)]
    assert res[0]["warn"][6] == (1 if with_reset else 0)
    assert np.all(np.isfinite(res[0]["qpos"]))
    for r in res[1:]:
        assert r["warn"] == res[0]["warn"]
        for f in fields:
            assert np.array_equal(r[f], res[0][f]), f"splitting a launch changed {f}"


@pytest.mark.parametrize("K,noise", [(3, None), (50, None), (2, None), (3, (20.0, 0.1, 5, 0))], ids=["K3", "K50", "last_step", "K3_noise"])
def test_reset_in_the_second_step(eng, lib, K, noise):
    """Run A: one env trips mj_checkAcc in the launch's SECOND step (K = 2: its last).  Run B: the same batch with an ordinary value there.  Every other
    env ends bit-equal in both; the reset env and the counters are the generic kernel's.  With OU noise on, ctrl shows that the retry trip did not
    advance the OU state a second time (bit-equal in the untouched lanes, the generic kernel's value in the reset one)."""
    model, cm = _model(eng, "franka_like")
    nenv, bad = 128, 20
    qpos, qvel = random_franka_state(model, nenv, 11)
    ctrl = None if noise else np.random.default_rng(1).uniform(-5, 5, (nenv, model["nu"]))
    qa = qvel.copy()
    qa[bad, 3] = TRIPS_AT_STEP_2
    others = np.arange(nenv) != bad
    fields = STATE + ("qacc",)
    gen1 = _run(eng, lib, cm, qpos, qa, ctrl, 1, 0, fields, noise)
    assert gen1["warn"][6] == 0, "the first step was meant to pass"
    gen = _run(eng, lib, cm, qpos, qa, ctrl, K, 0, fields, noise)
    assert gen["warn"][6] == 1, gen["warn"]
    A = _run(eng, lib, cm, qpos, qa, ctrl, K, 4, fields, noise)
    B = _run(eng, lib, cm, qpos, qvel, ctrl, K, 4, fields, noise)
    for f in fields:
        print(f"K = {K}, {f}: max |A - B| over the untouched envs = {np.nanmax(np.abs(A[f][others] - B[f][others])):.3e}, "
              f"reset env |four wavefronts - generic| = {np.abs(A[f][bad] - gen[f][bad]).max():.3e}")
    for f in fields:
        assert np.array_equal(A[f][others], B[f][others]), f"K = {K}: {f} of an untouched env differs between the runs"
    assert A["warn"] == gen["warn"], f"warning counters {A['warn']} vs the generic kernel's {gen['warn']}"
    assert B["warn"][6] == 0
    for f in fields:
        _close(A[f][bad], gen[f][bad], 1e-9, f"K = {K}: the reset env's {f} vs the generic kernel")
    assert np.all(np.isfinite(A["qpos"])) and np.all(np.isfinite(A["qacc"]))
    if noise:
        assert np.any(A["ctrl"][others] != 0)
    if K == 2:
        assert np.all(A["ctrl"][bad] == 0)   # mj_resetData in the last step: the step's ctrl reads zero


@pytest.mark.parametrize("flag", [DSBL_ACTUATION, DSBL_PASSIVE, DSBL_EULERDAMP], ids=["actuation", "passive", "eulerdamp"])
def test_disable_flags(eng, lib, flag):
    model, cm = _model(eng, "franka_like", flag)
    qpos, qvel = random_franka_state(model, 64, 6)
    _four_vs_three(eng, lib, cm, qpos, qvel, 50, (43.5, 0.1, 777, 1000), f"franka_like, disableflags {flag}")


@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_sensors_at_every_step(eng, lib, oracle_33, asset, K):
    """mjb_set_sensors_every_step: the launch's sensordata is still its last step's, against the oracle."""
    _, _, po = eng
    r = oracle_33[asset]
    cm = eng[0].CompiledModel(r["model"])
    got = _run(eng, lib, cm, r["qpos"], r["qvel"], None, K, 4, ("qpos", "sensordata"), r["noise"], every=True)
    oq, _, osd = po.rollout(r["model"], r["qpos"], r["qvel"], K, noise_std=r["noise"][0], noise_rate=0.1, seed=777, env_offset=1000, nthreads=8)
    print(f"{asset}, K = {K}, sensors at every step: max |sensordata - oracle| = {np.abs(got['sensordata'] - osd).max():.3e}")
    _close(got["sensordata"], osd, 1e-9, f"{asset} sensordata after {K} steps, sensors at every step")
    _close(got["qpos"], oq, 1e-9, f"{asset} qpos after {K} steps, sensors at every step")


def test_moved_anchor_is_built_by_hiprtc(eng, lib):
    """franka_like with one jnt_pos off centre: not the compiled-in topology any more (its kernel has no off-centre code), hiprtc builds one whose flag is
    set, and a step agrees with the oracle."""
    engine, mjcf, po = eng
    model = mjcf.load_asset("franka_like")
    model["enableflags"] = int(model["enableflags"]) | ENBL_ENERGY
    model["jnt_pos"] = np.array(model["jnt_pos"], dtype=np.float64)
    model["jnt_pos"][3] = (0.03, -0.02, 0.05)
    cm = engine.CompiledModel(model)
    nenv = 33
    qpos, qvel = random_franka_state(model, nenv, 3)
    ctrl = np.random.default_rng(4).uniform(-3, 3, (nenv, model["nu"]))
    lib.mjb_lane_env_set_sweep_waves(4)
    b = make(engine, cm, nenv, qpos, qvel * 3, 1, ctrl)
    assert b.lane_env_info()[0] == -2
    b.step(1)
    topo, used = b.lane_env_info()
    if topo == -3:
        pytest.fail("hiprtc build of the lane = env kernel not available on this box: " + b.lane_env_error())
    assert used
    _ran(lib, 4)
    got = {f: b.get(f) for f in ALL}
    b.close()
    for e in range(nenv):
        d = po.OracleData(model)
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e] * 3
        d.ctrl[:] = ctrl[e]
        d.step(1)
        for f in ALL:
            _close(got[f][e], d.field(f), 1e-11, f"moved anchor, {f} env {e} after one step vs the oracle")
    # (the anchor matters: the centred model's qacc is somewhere else entirely)
    base, cmb = _model(eng, "franka_like")
    ref = _run(eng, lib, cmb, qpos, qvel * 3, ctrl, 1, 4, ("qacc",))
    moved = np.abs(ref["qacc"] - got["qacc"]).max()
    print(f"moved anchor: max |qacc - the centred model's| = {moved:.3e}")
    assert moved > 1e-6
