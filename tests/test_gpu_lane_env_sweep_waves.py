"""Form 3 of the lane = env kernel with its root -> leaf sweep on three and on four wavefronts (mjb_lane_env_set_sweep_waves): the four-wavefront
variant cuts the pose wavefront's chain into an orientation chain and a frame follower (csrc/mjb_lane_env_kernel.h, roles 8 - 11).

Bounds are those of tests/test_gpu_lane_env.py and no others: one step <= 1e-11 (relative + absolute) against the oracle and the generic kernel,
rollouts <= 1e-9 against the oracle, two instantiations of the kernel on the same inputs <= 1e-12 (they agree to rounding, not bit for bit), launch
splits within one variant bit for bit.
"""
import numpy as np
import pytest

from conftest import random_franka_state
from test_gpu_lane_env import JIT_ARM, _close, make, tree_state, two_arm_xml

pytestmark = pytest.mark.gpu


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


@pytest.fixture(params=[3, 4], ids=["three_waves", "four_waves"])
def waves(request, lib):
    lib.mjb_lane_env_set_sweep_waves(request.param)
    return request.param


def _ran(lib, waves):
    assert lib.mjb_lane_env_last_form() == 3 and lib.mjb_lane_env_last_sweep_waves() == waves, (
        lib.mjb_lane_env_last_form(), lib.mjb_lane_env_last_sweep_waves(), waves)


def test_setter_and_getter(eng, lib):
    assert lib.mjb_lane_env_set_sweep_waves(4) == 0
    assert lib.mjb_lane_env_set_sweep_waves(3) == 4
    assert lib.mjb_lane_env_set_sweep_waves(7) == 3  # (anything else = the rule)
    assert lib.mjb_lane_env_set_sweep_waves(0) == 0
    engine, mjcf, _ = eng
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    qpos, qvel = random_franka_state(model, 64, 1)
    # the rule: four wavefronts where form 3 runs and the two extra rings fit; no sweep wavefronts to speak of in any other form
    b = make(engine, cm, 64, qpos, qvel, 1)
    b.step(2)
    _ran(lib, 4)
    assert b.set_lane_env_sweep_waves(0) == 0 and b.lane_env_last_sweep_waves() == 4
    lib.mjb_lane_env_set_form(0)
    b.step(2)
    assert lib.mjb_lane_env_last_form() == 0 and lib.mjb_lane_env_last_sweep_waves() == 0
    b.close()


@pytest.mark.parametrize("asset,nenv", [("franka_like", 200), ("lane_env_tree", 77)])
def test_one_step_matches_oracle_and_generic_kernel(eng, lib, waves, asset, nenv):
    engine, mjcf, po = eng
    model = mjcf.load_asset(asset)
    model["enableflags"] = int(model["enableflags"]) | 2
    cm = engine.CompiledModel(model)
    qpos, qvel = (random_franka_state if asset == "franka_like" else tree_state)(model, nenv, 3)
    qvel = qvel * 3
    ctrl = np.random.default_rng(4).uniform(-3, 3, (nenv, model["nu"]))
    out = {}
    for mode in (1, 0):
        b = make(engine, cm, nenv, qpos, qvel, mode, ctrl)
        b.step(1)
        assert b.lane_env_info()[1] == (mode == 1)
        if mode == 1:
            _ran(lib, waves)
        out[mode] = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "qacc_warmstart", "sensordata", "time", "energy", "ctrl")}
        b.close()
    d = po.OracleData(model)
    for e in range(nenv):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.ctrl[:] = ctrl[e]
        d.step(1)
        for f in ("qpos", "qvel", "qacc", "sensordata", "energy"):
            _close(out[1][f][e], d.field(f), 1e-11, f"{asset} {f} env {e} vs oracle")
    for f in out[1]:
        _close(out[1][f], out[0][f], 1e-11, f"{asset} {f} vs the generic kernel")


@pytest.mark.parametrize("asset,nenv,K,std", [("franka_like", 64, 200, 43.5), ("lane_env_tree", 33, 300, 1.5)])
def test_noise_rollouts_match_oracle_and_each_other(eng, lib, asset, nenv, K, std):
    engine, mjcf, po = eng
    model = mjcf.load_asset(asset)
    cm = engine.CompiledModel(model)
    qpos, qvel = (random_franka_state if asset == "franka_like" else tree_state)(model, nenv, 5)
    oq, ov, osd = po.rollout(model, qpos, qvel, K, noise_std=std, noise_rate=0.1, seed=777, env_offset=1000, nthreads=8)
    got = {}
    for w in (3, 4):
        lib.mjb_lane_env_set_sweep_waves(w)
        b = make(engine, cm, nenv, qpos, qvel, 1)
        b.set_ctrl_noise(std, 0.1, 777, 1000)
        b.step(K)
        assert b.lane_env_info()[1]
        _ran(lib, w)
        got[w] = (b.get("qpos"), b.get("qvel"), b.get("sensordata"))
        assert np.allclose(b.get("time"), K * float(np.ravel(model["timestep"])[0]), atol=1e-12)
        b.close()
        for a, o, what in zip(got[w], (oq, ov, osd), ("qpos", "qvel", "sensordata")):
            print(f"{asset} {w} wavefronts, {what} after {K} steps: max |gpu - oracle| = {np.abs(a - o).max():.3e}")
    for a, c, what in zip(got[3], got[4], ("qpos", "qvel", "sensordata")):
        print(f"{asset} {what} after {K} steps: max |three - four wavefronts| = {np.abs(a - c).max():.3e}")
    for w in (3, 4):
        for a, o, what in zip(got[w], (oq, ov, osd), ("qpos", "qvel", "sensordata")):
            _close(a, o, 1e-9, f"{asset} {what} after {K} steps, {w} wavefronts")
    for a, c, what in zip(got[3], got[4], ("qpos", "qvel", "sensordata")):
        _close(a, c, 1e-12, f"{asset} {what} after {K} steps, three vs four wavefronts")


def test_launch_splits_agree_bit_for_bit(eng, lib, waves):
    engine, mjcf, _ = eng
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    nenv = 70
    qpos, qvel = random_franka_state(model, nenv, 9)
    res = []
    for plan in ([120], [40, 40, 40], [1, 119]):
        b = make(engine, cm, nenv, qpos, qvel, 1)
        b.set_ctrl_noise(20.0, 0.1, 5, 0)
        for k in plan:
            b.step(k)
            _ran(lib, waves)
        res.append((b.get("qpos"), b.get("qvel"), b.get("ctrl"), b.get("time")))
        b.close()
    for i in (1, 2):
        for a, c in zip(res[0], res[i]):
            assert np.array_equal(a, c), "splitting a launch changed the result"


@pytest.mark.parametrize("nenv", [4097, 4100])
def test_tail_blocks(eng, lib, waves, nenv):
    """A last block with one / four live lanes: the lanes without an env run along and store nothing."""
    engine, mjcf, po = eng
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    K = 20
    qpos, qvel = random_franka_state(model, nenv, 2)
    b = make(engine, cm, nenv, qpos, qvel, 1)
    b.set_ctrl_noise(10.0, 0.1, 3, 0)
    b.step(K)
    assert b.lane_env_info()[1]
    _ran(lib, waves)
    q, v, sd = b.get("qpos"), b.get("qvel"), b.get("sensordata")
    b.close()
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(v)) and np.all(np.isfinite(sd))
    for e in (0, 4095, 4096, nenv - 1):
        oq, ov, osd = po.rollout(model, qpos[e:e + 1], qvel[e:e + 1], K, noise_std=10.0, noise_rate=0.1, seed=3, env_offset=int(e))
        _close(q[e], oq[0], 1e-9, f"env {e} of {nenv} qpos")
        _close(v[e], ov[0], 1e-9, f"env {e} of {nenv} qvel")
        _close(sd[e], osd[0], 1e-9, f"env {e} of {nenv} sensordata")


def test_bad_state_resets_like_mj_step(eng, lib, waves):
    engine, mjcf, po = eng
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    nenv = 128
    qpos, qvel = random_franka_state(model, nenv, 11)
    qpos[5, 2] = np.nan
    qvel[17, 0] = 1e12
    qvel[17, 1] = np.nan
    qpos[40, 0] = np.inf
    qvel[90, 3] = 9e9  # fine for mj_checkVel; the damping force makes qacc huge: mj_checkAcc's second trip through the forward pass
    ctrl = np.random.default_rng(1).uniform(-5, 5, (nenv, model["nu"]))
    got = {}
    for mode in (1, 0):
        b = make(engine, cm, nenv, qpos, qvel, mode, ctrl)
        b.step(3)
        if mode == 1:
            _ran(lib, waves)
        got[mode] = (b.get("qpos"), b.get("qvel"), b.get("ctrl"), b.get("time"), [b.warning(w) for w in range(8)])
        b.close()
    assert got[1][4] == got[0][4], f"warning counters differ: {got[1][4]} vs {got[0][4]}"
    assert got[1][4][4] == 2 and got[1][4][5] == 1 and got[1][4][6] >= 1
    for a, c in zip(got[1][:4], got[0][:4]):
        _close(a, c, 1e-9, "state after resets, lane = env vs generic")
    assert np.all(np.isfinite(got[1][0])) and np.all(got[1][2][5] == 0) and np.all(got[1][2][17] == 0)
    d = po.OracleData(model)
    for e in (5, 17, 40, 90):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.ctrl[:] = ctrl[e]
        d.step(3)
        _close(got[1][0][e], d.field("qpos"), 1e-9, f"env {e} qpos vs oracle")
        _close(got[1][1][e], d.field("qvel"), 1e-9, f"env {e} qvel vs oracle")


def test_sensors_every_step_is_the_same_launch(eng, lib, waves):
    engine, mjcf, _ = eng
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    nenv = 192
    qpos, qvel = random_franka_state(model, nenv, 21)
    out = []
    for every in (False, True):
        b = make(engine, cm, nenv, qpos, qvel, 1)
        b.set_sensors_every_step(every)
        b.set_ctrl_noise(3.0, 0.1, 5, 0)
        b.step(40)
        assert b.lane_env_info()[1]
        _ran(lib, waves)
        out.append((b.get("qpos"), b.get("sensordata")))
        b.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-13


def _jit_arm_model(mjcf):
    xml = JIT_ARM.replace('actuator="3"', 'actuator="act3"').replace('<motor joint="j4" forcelimited', '<motor name="act3" joint="j4" forcelimited')
    return mjcf.compile_xml_string(xml)


def test_hiprtc_built_topology(eng, lib, waves):
    """The hiprtc-built arm (an off-centre hinge, a slide, a branch, site sensors): one step against the oracle, a noise rollout, the reset paths."""
    engine, mjcf, po = eng
    model = _jit_arm_model(mjcf)
    model["enableflags"] = int(model["enableflags"]) | 2
    cm = engine.CompiledModel(model)
    nenv = 100
    rng = np.random.default_rng(8)
    qpos = np.tile(np.asarray(model["qpos0"], dtype=np.float64), (nenv, 1)) + rng.uniform(-0.7, 0.7, (nenv, model["nq"])) * np.where(np.asarray(model["jnt_type"]) == 3, 1.0, 0.05)
    qvel = rng.uniform(-1, 1, (nenv, model["nv"]))
    ctrl = rng.uniform(-2, 2, (nenv, model["nu"]))
    b = make(engine, cm, nenv, qpos, qvel, 1, ctrl)
    assert b.lane_env_info()[0] == -2
    b.step(1)
    topo, used = b.lane_env_info()
    if topo == -3:
        pytest.fail("hiprtc build of the lane = env kernel not available on this box: " + b.lane_env_error())
    assert used
    _ran(lib, waves)
    out = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata", "energy")}
    b.close()
    d = po.OracleData(model)
    for e in range(nenv):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.ctrl[:] = ctrl[e]
        d.step(1)
        for f in out:
            _close(out[f][e], d.field(f), 1e-11, f"jit arm {f} env {e}")
    b = make(engine, cm, nenv, qpos, qvel, 1)
    b.set_ctrl_noise(1.5, 0.1, 31, 500)
    b.step(150)
    _ran(lib, waves)
    oq, ov, osd = po.rollout(model, qpos, qvel, 150, noise_std=1.5, noise_rate=0.1, seed=31, env_offset=500, nthreads=8)
    _close(b.get("qpos"), oq, 1e-9, "jit arm qpos after 150 steps")
    _close(b.get("sensordata"), osd, 1e-9, "jit arm sensordata after 150 steps")
    b.close()
    qb, vb = qpos.copy(), qvel.copy()
    qb[3, 1] = np.nan
    vb[70, 2] = 2e11
    res = {}
    for mode in (1, 0):
        b = make(engine, cm, nenv, qb, vb, mode, ctrl)
        b.step(4)
        res[mode] = (b.get("qpos"), b.get("qvel"), [b.warning(w) for w in range(8)])
        b.close()
    assert res[1][2] == res[0][2] and res[1][2][4] == 1 and res[1][2][5] == 1
    _close(res[1][0], res[0][0], 1e-9, "jit arm, state after resets vs the generic kernel")


def test_layout_beyond_the_lds_falls_back(eng, lib):
    """two_arm_xml(): 14 dofs, 15 moving bodies -- the three-wavefront layout already exceeds a CU's 160 KB, so a request for form 3 with four
    wavefronts runs a two-wavefront form, and the getter says so."""
    engine, mjcf, po = eng
    model = mjcf.compile_xml_string(two_arm_xml())
    cm = engine.CompiledModel(model)
    lib.mjb_lane_env_set_sweep_waves(4)
    nenv, K = 200, 60
    rng = np.random.default_rng(3)
    qpos = rng.uniform(-0.8, 0.8, (nenv, model["nq"]))
    qvel = rng.uniform(-1, 1, (nenv, model["nv"]))
    b = make(engine, cm, nenv, qpos, qvel, 1)
    b.set_ctrl_noise(1.0, 0.1, 17, 0)
    b.step(K)
    topo, used = b.lane_env_info()
    assert used, f"lane = env kernel not used (info {topo}): {b.lane_env_error()}"
    assert lib.mjb_lane_env_last_form() in (1, 2) and lib.mjb_lane_env_last_sweep_waves() == 0
    q = b.get("qpos")
    b.close()
    for e in (0, nenv // 2, nenv - 1):
        oq, _, _ = po.rollout(model, qpos[e:e + 1], qvel[e:e + 1], K, noise_std=1.0, noise_rate=0.1, seed=17, env_offset=int(e))
        _close(q[e], oq[0], 1e-9, f"two-arm env {e} qpos")


def test_four_wavefront_hiprtc_build_is_cached_on_disk(tmp_path):
    """A second process loads the four-wavefront hiprtc build from $MJB_JIT_CACHE without compiling; the three-wavefront build of the same model is
    another cache entry."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import ctypes as C, json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from mujoco_ros_pkgs_amd import engine, mjcf
from test_gpu_lane_env import JIT_ARM
xml = JIT_ARM.replace('actuator="3"', 'actuator="act3"').replace('<motor joint="j4" forcelimited', '<motor name="act3" joint="j4" forcelimited')
model = mjcf.compile_xml_string(xml)
cm = engine.CompiledModel(model)
b = engine.Batch(cm, 64)
b.set_lane_env(1)
b.lib.mjb_lane_env_set_form(3)
b.lib.mjb_lane_env_set_sweep_waves(int(sys.argv[1]))
rng = np.random.default_rng(2)
b.set("qvel", rng.uniform(-1, 1, (64, model["nv"])))
b.step(3)
q = b.get("qpos")
comp, hits = C.c_int(0), C.c_int(0)
b.lib.mjb_lane_env_jit_counts(C.byref(comp), C.byref(hits))
print(json.dumps(dict(used=b.lane_env_info()[1], compiled=comp.value, hits=hits.value, qsum=float(np.abs(q).sum()), err=b.lane_env_error(),
                      form=b.lib.mjb_lane_env_last_form(), waves=b.lib.mjb_lane_env_last_sweep_waves())))
''' % (root, os.path.join(root, "tests"))
    env = dict(os.environ, MJB_JIT_CACHE=str(tmp_path / "jit"))
    runs = []
    for w in (4, 4, 3):
        out = subprocess.run([sys.executable, "-c", script, str(w)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    first, second, three = runs
    assert first["used"], "hiprtc build not available on this box: " + first["err"]
    assert first["form"] == 3 and first["waves"] == 4 and first["compiled"] == 1 and first["hits"] == 0, first
    assert second["used"] and second["waves"] == 4 and second["compiled"] == 0 and second["hits"] == 1, second
    assert second["qsum"] == first["qsum"]
    assert three["used"] and three["form"] == 3 and three["waves"] == 3 and three["compiled"] == 1 and three["hits"] == 0, three
    assert len(list((tmp_path / "jit").glob("le_*.hsaco"))) == 2
