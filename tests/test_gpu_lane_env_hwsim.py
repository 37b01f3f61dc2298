"""The device-side ros_control stage (DefaultRobotHWSim::writeSim, mjb_hwsim_*) inside the lane = env kernel (Batch.set_lane_env_hwsim;
csrc/mjb_lane_env_kernel.h, template flag HW), against the CPU oracle's restatement (oracle/mjo_hwsim.c) and against the generic
16-lanes-per-env kernel running the same batch.

Bounds.  One step: 1e-11 relative + absolute on qpos / qvel / qacc / sensordata, the bound tests/test_gpu_lane_env.py holds this kernel to, and
1e-11 max(1, |value|) on qfrc_applied.  Rollouts: the bounds of tests/test_hwsim.py::test_gpu_matches_oracle on the same inputs (200 steps: qpos 1e-8,
qvel 1e-6, qfrc_applied 1e-6; after the e-stop leg qpos 1e-7).  Against the generic kernel over tens of steps: 1e-9 relative + absolute, the
interleaving bound of tests/test_gpu_lane_env.py.  70 envs = one full wavefront and a 6-lane tail; envs 0, 63, 64, 69 go against the oracle."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_franka_state
from test_gpu_lane_env import JIT_ARM, tree_state
from test_hwsim import _cadence_rollout, _cfg, _commands, _oracle_cfg, _oracle_rollout

pytestmark = pytest.mark.gpu

NENV = 70
CHECK = (0, 63, 64, 69)
STATE = ("qpos", "qvel", "qfrc_applied", "time")


def _close(a, b, tol, what):
    a, b = np.asarray(a), np.asarray(b)
    err = np.abs(a - b)
    bound = tol * (1.0 + np.abs(b))
    assert np.all(err <= bound), f"{what}: max err {np.nanmax(err):.3e} (ref scale {np.nanmax(np.abs(b)):.3e})"


def _close_frc(a, b, tol, what):
    a, b = np.asarray(a), np.asarray(b)
    err = np.abs(a - b)
    assert np.all(err <= tol * np.maximum(1.0, np.abs(b))), f"{what}: max err {err.max():.3e} (ref scale {np.abs(b).max():.3e})"


@pytest.fixture(scope="module")
def eng(oracle_built):
    from mujoco_ros_pkgs_amd import engine, mjcf
    return engine, mjcf, oracle_built


def _tree_cfg(model):
    """lane_env_tree: every control method, on hinges and on both slides; a revolute joint with and one without limits."""
    j = {n: model.name2id("joint", n) for n in model["names"]["joint"]}
    return [
        dict(joint=j["j_base"], method="position_pid", kind="revolute", p=60, i=4, d=3, i_max=2, i_min=-2, effort_limit=20, lower=-1.0, upper=1.2),
        dict(joint=j["jA1"], method="position_pid", kind="continuous", p=40, d=2),
        dict(joint=j["jA2"], method="position_pid", kind="prismatic", p=300, d=8, effort_limit=15),
        dict(joint=j["jB1"], method="velocity_pid", p=5, i=1, i_max=1, i_min=-1, antiwindup=1, effort_limit=6),
        dict(joint=j["jB2"], method="effort"),
        dict(joint=j["jB3"], method="velocity"),
        dict(joint=j["jP1"], method="position"),
        dict(joint=j["jP2"], method="position_pid", kind="revolute", p=20, i=3, d=1, i_max=0.5, i_min=-0.5),
    ]


def _setup(eng, asset="franka_like", nenv=NENV, seed=3, override=None):
    engine, mjcf, po = eng
    model = mjcf.load_asset(asset, override=override) if override else mjcf.load_asset(asset)
    spec = _cfg(model) if asset == "franka_like" else _tree_cfg(model)
    qpos, qvel = (random_franka_state if asset == "franka_like" else tree_state)(model, nenv, seed)
    cmds = _commands(len(spec), nenv, seed + 100)
    return model, engine.CompiledModel(model), spec, _oracle_cfg(spec), qpos, qvel, cmds


def _batch(engine, cm, spec, qpos, qvel, cmds, mode=1, switch=True, period=None, ctrl=None, applied=None):
    b = engine.Batch(cm, len(qpos))
    b.set_lane_env(mode)
    if switch:
        b.set_lane_env_hwsim(True)
    if spec is not None:
        b.hwsim_configure(spec)
        if period is not None:
            b.hwsim_set_period(period)
        for which, c in zip(("position", "velocity", "effort"), cmds):
            b.hwsim_set_command(which, c)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if ctrl is not None:
        b.set("ctrl", ctrl)
    if applied is not None:
        b.set("qfrc_applied", applied)
    return b


def _ran(b, lane):
    assert b.lane_env_info()[1] == lane, f"lane = env kernel used: {b.lane_env_info()[1]}, expected {lane}"
    if lane:
        assert b.lane_env_last_form() == 0


class Twin:
    """One env in the oracle with the ros_control stage between step1 and step2: writeSim at every step, or under the controller cadence."""

    def __init__(self, po, model, cfg, qpos, qvel, cmds, ctrl=None, applied=None, time=0.0):
        self.d = po.OracleData(model)
        self.d.qpos[:] = qpos
        self.d.qvel[:] = qvel
        if ctrl is not None:
            self.d.ctrl[:] = ctrl
        if applied is not None:
            self.d.qfrc_applied[:] = applied
        self.d.time[:] = time
        n = len(cfg["joint"])
        self.cfg, self.cmds, self.pid, self.hold, self.estop = cfg, [np.array(c, dtype=np.float64) for c in cmds], np.zeros((n, 2)), np.zeros(n), False
        self.set_period(0.0)

    def set_period(self, period):
        n = len(self.cfg["joint"])
        self.period, self.cad = period, np.r_[0.0, 0.0, np.ones(n), np.zeros(n)]

    def step(self, k=1):
        cp, cv, ce = self.cmds
        for _ in range(k):
            self.d.call("step1")
            if self.period > 0:
                self.d.hwsim_control_callback(self.cfg, cp, cv, ce, self.hold, self.pid, self.estop, self.cad, self.period)
            else:
                self.d.hwsim_write(self.cfg, cp, cv, ce, self.hold, self.pid, self.estop)
            self.d.call("step2")
        return self


def _worst(b, twins, fields=("qpos", "qvel", "qfrc_applied")):
    got = {f: b.get(f) for f in fields}
    return {f: max(float(np.abs(got[f][e] - t.d.field(f)).max()) for e, t in twins.items()) for f in fields}


# ------------------------------------------------------------------------------------------------------------------- 1. the switch
def test_switch(eng):
    engine = eng[0]
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng)
    on = _batch(engine, cm, spec, qpos, qvel, cmds, mode=1, switch=True)
    on.step(1)
    _ran(on, True)
    off = _batch(engine, cm, spec, qpos, qvel, cmds, mode=1, switch=False)
    off.step(1)
    _ran(off, False)
    never = _batch(engine, cm, spec, qpos, qvel, cmds, mode=0, switch=True)
    never.step(1)
    _ran(never, False)
    for b in (on, off, never):
        b.close()
    # no stage left: a switched-on batch is a batch that never had the switch
    out = []
    for switch in (True, False):
        b = _batch(engine, cm, spec if switch else None, qpos, qvel, cmds, mode=1, switch=switch)
        if switch:
            b.hwsim_configure([])
        b.set_ctrl_noise(5.0, 0.1, 3, 0)
        b.step(20)
        assert b.lane_env_info()[1]
        out.append([b.get(f) for f in STATE + ("sensordata", "ctrl")])
        b.close()
    for a, c in zip(*out):
        assert np.array_equal(a, c)


# ------------------------------------------------------------------------------- 2. one step against the oracle and the generic kernel
@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_one_step_matches_oracle_and_generic_kernel(eng, asset):
    engine, _, po = eng
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, asset)
    qvel = qvel * 3
    rng = np.random.default_rng(4)
    ctrl = rng.uniform(-3, 3, (NENV, model["nu"]))
    applied = rng.uniform(-2, 2, (NENV, model["nv"]))  # (the user's qfrc_applied: stays on the dofs no controller writes)
    out = {}
    for mode in (1, 0):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=mode, ctrl=ctrl, applied=applied)
        b.step(1)
        _ran(b, mode == 1)
        out[mode] = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata", "qfrc_applied", "time")}
        b.close()
    for e in range(NENV):
        t = Twin(po, model, cfg, qpos[e], qvel[e], [c[e] for c in cmds], ctrl[e], applied[e]).step(1)
        for f in ("qpos", "qvel", "qacc", "sensordata"):
            _close(out[1][f][e], t.d.field(f), 1e-11, f"{asset} {f} env {e} vs oracle")
        _close_frc(out[1]["qfrc_applied"][e], t.d.field("qfrc_applied"), 1e-11, f"{asset} qfrc_applied env {e} vs oracle")
    for f in ("qpos", "qvel", "qacc", "sensordata", "time"):
        _close(out[1][f], out[0][f], 1e-11, f"{asset} {f} vs the generic kernel")
    _close_frc(out[1]["qfrc_applied"], out[0]["qfrc_applied"], 1e-11, f"{asset} qfrc_applied vs the generic kernel")


# ------------------------------------------------------------------------------------------------------ 3. rollouts against the oracle
def test_rollout_matches_oracle(eng):
    """The sequence and inputs of tests/test_hwsim.py::test_gpu_matches_oracle, at 70 envs on the lane = env kernel (and, for the printed figures, on
    the generic one)."""
    engine, mjcf, po = eng
    model = mjcf.load_asset("franka_like")
    spec = _cfg(model)
    cfg = _oracle_cfg(spec)
    cp, cv, ce = _commands(len(spec), NENV, 1)
    qpos = np.tile(np.asarray(model["qpos0"], dtype=np.float64), (NENV, 1))
    cm = engine.CompiledModel(model)
    bs = {mode: _batch(engine, cm, spec, qpos, 0 * qpos, (cp, cv, ce), mode=mode) for mode in (1, 0)}
    for mode, b in bs.items():
        b.step(150)
        _ran(b, mode == 1)
        b.step(1)
        b.step(49)
    ref = {e: _oracle_rollout(po, model, cfg, qpos[e], cp[e], cv[e], ce[e], 200)[0] for e in CHECK}
    for mode, b in bs.items():
        w = {f: max(float(np.abs(b.get(f)[e] - ref[e].field(f)).max()) for e in CHECK) for f in ("qpos", "qvel", "qfrc_applied")}
        print(f"200 steps, {'lane = env' if mode else 'generic'} kernel, worst |gpu - oracle|: " + ", ".join(f"{f} {v:.3e}" for f, v in w.items()))
    b = bs[1]
    for e in CHECK:
        np.testing.assert_allclose(b.get("qpos")[e], ref[e].qpos, rtol=0, atol=1e-8)
        np.testing.assert_allclose(b.get("qvel")[e], ref[e].qvel, rtol=0, atol=1e-6)
        np.testing.assert_allclose(b.get("qfrc_applied")[e], ref[e].qfrc_applied, rtol=0, atol=1e-6)
    for mode, b in bs.items():
        b.hwsim_estop(True)
        b.hwsim_set_command("position", cp + 1.0)  # ignored while the e-stop holds the old commands
        b.step(100)
        _ran(b, mode == 1)
    ref = {e: _oracle_rollout(po, model, cfg, qpos[e], cp[e], cv[e], ce[e], 300, estop_at=200)[0] for e in CHECK}
    for mode, b in bs.items():
        w = max(float(np.abs(b.get("qpos")[e] - ref[e].qpos).max()) for e in CHECK)
        print(f"e-stop leg, {'lane = env' if mode else 'generic'} kernel, worst |gpu - oracle|: qpos {w:.3e}")
    for e in CHECK:
        np.testing.assert_allclose(bs[1].get("qpos")[e], ref[e].qpos, rtol=0, atol=1e-7)
    for b in bs.values():
        b.close()


# ----------------------------------------------------------------------------------------------------- 4. cadence, lanes disagreeing
@pytest.mark.parametrize("factor", [4.0, 0.5])
def test_cadence_with_lanes_disagreeing(eng, factor):
    """Every env starts at its own time -- whole steps apart (the update every 4 dt falls on different steps) and a fraction of a step apart (the
    nanosecond stamps differ) -- so the lanes of a wavefront update and write at different steps; two envs are set back between launches and re-arm."""
    engine, _, po = eng
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=5)
    dt = float(np.ravel(model["timestep"])[0])
    period = factor * dt
    idx = np.arange(NENV)
    t0 = (idx % 5) * dt + (idx % 3) * 0.37 * dt
    t0[0] = 0.0  # (nothing happens at t = 0)
    back = {63: 1.5 * dt, 69: 0.0}
    bs = {}
    for mode in (1, 0):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=mode, period=period)
        b.set("time", t0.reshape(b.get("time").shape))
        b.step(7)
        _ran(b, mode == 1)
        b.step(1)
        t = b.get("time")
        for e, v in back.items():
            t[e] = v
        b.set("time", t)
        b.step(12)
        _ran(b, mode == 1)
        bs[mode] = b
    twins = {}
    for e in CHECK:
        t = Twin(po, model, cfg, qpos[e], qvel[e], [c[e] for c in cmds], time=t0[e])
        t.set_period(period)
        t.step(8)
        if e in back:
            t.d.time[:] = back[e]
        twins[e] = t.step(12)
    for mode, b in bs.items():
        w = _worst(b, twins)
        print(f"cadence {factor} dt, {'lane = env' if mode else 'generic'} kernel, worst |gpu - oracle|: " + ", ".join(f"{f} {v:.3e}" for f, v in w.items()))
    w = _worst(bs[1], twins)
    assert w["qpos"] <= 1e-8 and w["qvel"] <= 1e-6 and w["qfrc_applied"] <= 1e-6, w
    for f in STATE:
        _close(bs[1].get(f), bs[0].get(f), 1e-9, f"cadence {factor} dt, {f} vs the generic kernel")
    # back to a write at every step on the step's own state
    for mode, b in bs.items():
        b.hwsim_set_period(0)
        b.step(3)
        _ran(b, mode == 1)
    for t in twins.values():
        t.set_period(0.0)
        t.step(3)
    w = _worst(bs[1], twins)
    assert w["qpos"] <= 1e-8 and w["qvel"] <= 1e-6 and w["qfrc_applied"] <= 1e-6, w
    for f in STATE:
        _close(bs[1].get(f), bs[0].get(f), 1e-9, f"period 0 after cadence {factor} dt, {f} vs the generic kernel")
    for b in bs.values():
        b.close()


def test_cadence_from_time_zero_matches_shared_rollout(eng):
    """The cadence rollout of tests/test_hwsim.py (qvel = 0, t = 0) on the lane = env kernel: nothing at t = 0, first update and write one step later."""
    engine, mjcf, po = eng
    model = mjcf.load_asset("franka_like")
    spec = _cfg(model)
    cfg = _oracle_cfg(spec)
    cmds = _commands(len(spec), NENV, 2)
    qpos = np.tile(np.asarray(model["qpos0"], dtype=np.float64), (NENV, 1))
    dt = float(np.ravel(model["timestep"])[0])
    b = _batch(engine, engine.CompiledModel(model), spec, qpos, 0 * qpos, cmds, period=4 * dt)
    b.step(1)
    _ran(b, True)
    da3 = model["jnt_dofadr"][spec[3]["joint"]]
    assert np.all(b.get("qfrc_applied")[:, da3] == 0)  # nothing written at t = 0
    b.step(60)
    b.step(1)
    b.step(38)
    for e in CHECK:
        d, *_ = _cadence_rollout(po, model, cfg, qpos[e], *[c[e] for c in cmds], 100, 4 * dt)
        np.testing.assert_allclose(b.get("qpos")[e], d.qpos, rtol=0, atol=1e-8)
        np.testing.assert_allclose(b.get("qvel")[e], d.qvel, rtol=0, atol=1e-6)
        np.testing.assert_allclose(b.get("qfrc_applied")[e], d.qfrc_applied, rtol=0, atol=1e-6)
    b.close()


# --------------------------------------------------------------------------------------------------- 5. launch splits and hand-over
def test_launch_splits_and_handover(eng):
    engine = eng[0]
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=9)
    dt = float(np.ravel(model["timestep"])[0])
    res = []
    for plan in ([40], [1] * 40, [13, 27]):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, period=4 * dt)
        for k in plan:
            b.step(k)
            _ran(b, True)
        res.append([b.get(f) for f in STATE])
        b.close()
    for other in res[1:]:
        for f, a, c in zip(STATE, res[0], other):
            assert np.array_equal(a, c), f"splitting a launch changed {f}: PID state or cadence stamps did not survive HBM"
    # the two kernels hand the same batch back and forth
    out = {}
    for alternate in (True, False):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=1, switch=False, period=4 * dt)
        for i in range(6):
            lane = alternate and i % 2 == 0
            b.set_lane_env_hwsim(lane)
            b.step(10)
            _ran(b, lane)
        out[alternate] = [b.get(f) for f in STATE]
        b.close()
    for f, a, c in zip(STATE, out[True], out[False]):
        _close(a, c, 1e-9, f"lane = env / generic interleaved, {f}")


# ------------------------------------------------------------------------------------------------------------------------ 6. resets
@pytest.mark.parametrize("factor", [4.0, 0.0])
def test_bad_state_resets_like_mj_step(eng, factor):
    """mj_checkPos / mj_checkVel / mj_checkAcc with the stage on: a NaN qpos, a huge qvel, and -- in the tail wavefront -- an effort command that
    drives qacc beyond mjMAXVAL, so that the step's retry runs the stage a second time for that lane and for no other."""
    engine, _, po = eng
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=11)
    dt = float(np.ravel(model["timestep"])[0])
    period = factor * dt
    qpos, qvel = qpos.copy(), qvel.copy()
    qpos[5, 2] = np.nan
    qvel[20, 0] = 1e12
    cmds2 = [c.copy() for c in cmds]
    cmds2[2][66, 3] = 1e13  # (entry 3 of the controller set: the EFFORT joint)
    got = {}
    for mode in (1, 0):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=mode, period=period if period > 0 else None)
        b.step(2)
        b.hwsim_set_command("effort", cmds2[2])
        b.step(5)
        _ran(b, mode == 1)
        got[mode] = [b.get(f) for f in STATE] + [[b.warning(w) for w in range(8)]]
        b.close()
    assert got[1][4] == got[0][4], f"warning counters differ: {got[1][4]} vs {got[0][4]}"
    assert got[1][4][4] == 1 and got[1][4][5] >= 1 and got[1][4][6] >= 1
    for f, a, c in zip(STATE, got[1][:4], got[0][:4]):
        assert np.all(np.isfinite(a)), f
        _close(a, c, 1e-9, f"{f} after resets, lane = env vs generic")
    # the neighbours of the reset lanes never noticed
    for e in (4, 6, 19, 21, 65, 67):
        t = Twin(po, model, cfg, qpos[e], qvel[e], [c[e] for c in cmds])
        t.set_period(period)
        t.step(7)
        for f, tol in (("qpos", 1e-8), ("qvel", 1e-6), ("qfrc_applied", 1e-6)):
            np.testing.assert_allclose(got[1][STATE.index(f)][e], t.d.field(f), rtol=0, atol=tol, err_msg=f"env {e} {f} vs oracle")


@pytest.mark.parametrize("factor", [0.0, 4.0])
def test_reset_beside_a_retry_in_one_wavefront(eng, factor):
    """At one and the same step, in one wavefront: env 5 gets a NaN qpos, env 20 a huge qvel (mj_checkPos / mj_checkVel reset them in front of the
    stage), and env 10 an effort command that drives qacc beyond mjMAXVAL (mj_checkAcc resets it; the wavefront takes the retry trip).  The retry
    concerns env 10 alone: envs 5 and 20 keep the force the stage gave them on the first trip, as in the generic kernel, which reruns the stage for
    the reset env only.  Compared after that step alone (qacc and qfrc_applied of the step itself), and four steps on."""
    engine = eng[0]
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=23)
    dt = float(np.ravel(model["timestep"])[0])
    eff = cmds[2].copy()
    eff[10, 3] = 1e13  # (entry 3 of the controller set: the EFFORT joint)
    fields = STATE + ("qacc",)
    got = {}
    for mode in (1, 0):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=mode, period=factor * dt if factor > 0 else None)
        b.step(2)
        q, v = b.get("qpos"), b.get("qvel")
        q[5, 2] = np.nan
        v[20, 0] = 1e12
        b.set("qpos", q)
        b.set("qvel", v)
        b.hwsim_set_command("effort", eff)
        res = []
        for k in (1, 4):
            b.step(k)
            _ran(b, mode == 1)
            res.append([b.get(f) for f in fields] + [[b.warning(w) for w in range(8)]])
        got[mode] = res
        b.close()
    for leg, (lane, gen) in enumerate(zip(got[1], got[0])):
        assert lane[-1] == gen[-1], f"warning counters differ: {lane[-1]} vs {gen[-1]}"
        assert lane[-1][4] == 1 and lane[-1][5] >= 1 and lane[-1][6] >= 1  # bad qpos (once), bad qvel, bad qacc
        for f, a, c in zip(fields, lane, gen):
            assert np.all(np.isfinite(a)), f
            _close(a, c, 1e-9, f"{f} {'of the step with the resets' if leg == 0 else 'four steps on'}, lane = env vs generic")


# --------------------------------------------------------------------------------------------------- 7. ctrl noise with the stage
def test_ctrl_noise_with_the_stage(eng):
    engine = eng[0]
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=13)
    for plan in ([100], [10] * 10):  # the launch's pre-generated normals / generated inside the kernel (K < 16)
        out = {}
        for mode in (1, 0):
            b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=mode)
            b.set_ctrl_noise(5.0, 0.1, 777, 1000)
            for k in plan:
                b.step(k)
                _ran(b, mode == 1)
            out[mode] = [b.get(f) for f in STATE + ("ctrl",)]
            b.close()
        for f, a, c in zip(STATE + ("ctrl",), out[1], out[0]):
            _close(a, c, 1e-9, f"ctrl noise + stage, launches of {plan[0]}, {f}")


# --------------------------------------------------------------------------------------------------------------- 8. lean LDS builds
@pytest.mark.parametrize("nenv", [20000, 40000])
def test_lean_lds_variants(eng, nenv):
    engine, _, po = eng
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, nenv=nenv, seed=21)
    sampled = (0, 63, 64, 12345, nenv - 1)
    for K in (1, 100):
        b = _batch(engine, cm, spec, qpos, qvel, cmds)
        b.step(K)
        _ran(b, True)
        got = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata", "qfrc_applied")}
        b.close()
        assert all(np.all(np.isfinite(got[f])) for f in ("qpos", "qvel", "qfrc_applied"))
        for e in sampled:
            t = Twin(po, model, cfg, qpos[e], qvel[e], [c[e] for c in cmds]).step(K)
            if K == 1:
                for f in ("qpos", "qvel", "qacc", "sensordata"):
                    _close(got[f][e], t.d.field(f), 1e-11, f"{nenv} envs, {f} env {e} after one step")
                _close_frc(got["qfrc_applied"][e], t.d.field("qfrc_applied"), 1e-11, f"{nenv} envs, qfrc_applied env {e} after one step")
            else:
                for f in ("qpos", "qvel"):
                    _close(got[f][e], t.d.field(f), 1e-8, f"{nenv} envs, {f} env {e} after {K} steps")


# --------------------------------------------------------------------------------------------------------------- 9. hiprtc topology
def test_topology_built_by_hiprtc(eng):
    engine, mjcf, po = eng
    xml = JIT_ARM.replace('actuator="3"', 'actuator="act3"').replace('<motor joint="j4" forcelimited', '<motor name="act3" joint="j4" forcelimited')
    model = mjcf.compile_xml_string(xml)
    cm = engine.CompiledModel(model)
    j = {n: model.name2id("joint", n) for n in model["names"]["joint"]}
    spec = [dict(joint=j["j2"], method="position_pid", kind="revolute", p=50, i=5, d=2, i_max=1, i_min=-1, effort_limit=30, lower=-1.2, upper=1.0),
            dict(joint=j["j4"], method="velocity_pid", p=20, i=2, i_max=1, i_min=-1, antiwindup=1),
            dict(joint=j["j5"], method="position")]
    cfg = _oracle_cfg(spec)
    rng = np.random.default_rng(8)
    qpos = np.tile(np.asarray(model["qpos0"], dtype=np.float64), (NENV, 1)) + rng.uniform(-0.7, 0.7, (NENV, model["nq"])) * np.where(np.asarray(model["jnt_type"]) == 3, 1.0, 0.05)
    qvel = rng.uniform(-1, 1, (NENV, model["nv"]))
    ctrl = rng.uniform(-2, 2, (NENV, model["nu"]))
    cmds = _commands(len(spec), NENV, 9)

    def builds(b):
        comp, hits = C.c_int(0), C.c_int(0)
        b.lib.mjb_lane_env_jit_counts(C.byref(comp), C.byref(hits))
        return comp.value + hits.value

    plain = _batch(engine, cm, None, qpos, qvel, cmds, ctrl=ctrl)
    assert plain.lane_env_info()[0] == -2
    plain.step(1)
    if plain.lane_env_info()[0] == -3 and ("not found" in plain.lane_env_error() or "disabled" in plain.lane_env_error()):
        pytest.skip("hiprtc not available: " + plain.lane_env_error())
    assert plain.lane_env_info()[1], plain.lane_env_error()
    before = builds(plain)
    plain.close()
    b = _batch(engine, cm, spec, qpos, qvel, cmds, ctrl=ctrl)
    b.step(1)
    assert b.lane_env_info()[1], "the HW build of the hiprtc topology did not run: " + b.lane_env_error()
    assert b.lane_env_last_form() == 0
    assert builds(b) > before, "the HW build must be a code object of its own in the JIT cache"
    got = {f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata", "qfrc_applied")}
    b.close()
    for e in range(NENV):
        t = Twin(po, model, cfg, qpos[e], qvel[e], [c[e] for c in cmds], ctrl[e]).step(1)
        for f in ("qpos", "qvel", "qacc", "sensordata"):
            _close(got[f][e], t.d.field(f), 1e-11, f"jit arm {f} env {e}")
        _close_frc(got["qfrc_applied"][e], t.d.field("qfrc_applied"), 1e-11, f"jit arm qfrc_applied env {e}")


# ------------------------------------------------------------------------------------------------------------------ 10. stand-downs
@pytest.mark.parametrize("what", ["env_gravity", "xfrc_applied", "stats", "rk4", "joint_controlled_twice"])
def test_stand_downs(eng, what):
    """With the switch on these batches still run the generic kernels, and compute what a switched-off batch computes, bit for bit."""
    engine = eng[0]
    model, cm, spec, cfg, qpos, qvel, cmds = _setup(eng, seed=17, override={"integrator": "RK4"} if what == "rk4" else None)
    if what == "joint_controlled_twice":  # (the kernel's table is by dof: one entry per joint. The generic stage runs the entries in order, the later one wins)
        spec = spec + [dict(joint=spec[0]["joint"], method="effort")]
        cmds = _commands(len(spec), NENV, 117)
    rng = np.random.default_rng(2)
    out = []
    for switch in (True, False):
        b = _batch(engine, cm, spec, qpos, qvel, cmds, mode=2 if what == "env_gravity" else 1, switch=switch)
        if what == "env_gravity":
            b.set_env_gravity(np.asarray(model["gravity"], dtype=np.float64)[None] + np.random.default_rng(1).uniform(-0.5, 0.5, (NENV, 3)))
        elif what == "xfrc_applied":
            b.set("xfrc_applied", rng.uniform(-1, 1, (NENV, model["nbody"], 6)) if switch else out[0][-1])
        elif what == "stats":
            b.set_stats(True)
        b.step(10)
        _ran(b, False)
        out.append([b.get(f) for f in STATE] + [b.get("xfrc_applied")])
        b.close()
    for f, a, c in zip(STATE, out[0], out[1]):
        assert np.array_equal(a, c), f"{what}: {f} differs from the switched-off batch"
