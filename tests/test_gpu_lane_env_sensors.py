"""Frame-axis, velocity- and acceleration-stage sensors in the lane = env kernel (csrc/mjb_lane_env_kernel.h, LeSens): velocity sensors in the
root -> leaf sweep, the acceleration stage in a pass behind the qacc solve -- against the CPU oracle, against the generic 16-lanes-per-env kernel
running the same batch, and against closed forms on a one-hinge model.

Bounds, max |got - want| / (1 + |want|), those of the sibling lane = env tests: one step against the oracle 1e-11; rollouts of 60 steps or fewer, and the
lane = env kernel against the generic one, 1e-9; bit equality where a test says so.  70 envs = one full wavefront and a 6-lane tail; envs 0, 63, 64, 69
go against the oracle where not every env does.  Models and states: tests/lane_env_sensor_models.py.  Every test checks that the kernel ran, built by
hiprtc, in its one-wavefront form: a silent fall-back to the generic kernel would pass every comparison."""
import functools

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import mjcf
import lane_env_sensor_models as sm
from lane_env_sensor_models import CHECK, NENV
from test_gpu_lane_env_params import apply, draw, twin_model
from test_lane_env_act import oracle_env

pytestmark = pytest.mark.gpu

FIELDS = ("qpos", "qvel", "qacc", "sensordata")
EVERY = FIELDS + ("time", "ctrl")
NOISE = (20.0, 0.1, 5, 0)
ROLLOUT = 60
DSBL_SENSOR = 1 << 12
VEL_TYPES, ACC_TYPES = {2, 3, 28, 29}, {1, 4, 5, 30, 31}


def _engine():
    from mujoco_ros_pkgs_amd import engine
    return engine


def _err(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if want.size else 0.0


def _close(got, want, tol, what):
    err = _err(got, want)
    print(f"{what}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e}"


@functools.lru_cache(maxsize=None)
def case(which, **kw):
    """(model, compiled model, states): compiled once per module and shared; callers do not write into the states."""
    model = sm.model_P(**kw) if which == "P" else sm.model_S(**kw)
    return model, _engine().CompiledModel(model), sm.states(which, model)


def make(cm, S, mode=1, noise=None, ctrl=True, n=None):
    qpos, qvel, c, act = S
    b = _engine().Batch(cm, qpos.shape[0] if n is None else n)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if act.shape[1]:
        b.set("act", act)
    if ctrl:
        b.set("ctrl", c)
    if noise:
        b.set_ctrl_noise(*noise)
    return b


def ran(b, lane=True):
    """The lane = env kernel ran (or, lane False, did not), built by hiprtc, one wavefront per 64 envs."""
    topo, used = b.lane_env_info()
    if lane and topo == -3:
        pytest.fail("hiprtc build of the lane = env kernel not available on this box: " + b.lane_env_error())
    assert (topo, bool(used)) == (-2, lane), f"lane_env_info() = {(topo, used)}, expected {(-2, lane)}: {b.lane_env_error()}"
    if lane:
        assert b.lane_env_last_form() == 0, b.lane_env_error()


def snapshot(b, fields=EVERY):
    return {f: b.get(f) for f in fields}


def against_oracle(po, model, got, S, K, tol, envs, what, noise=None, xfrc=None, models=None):
    qpos, qvel, ctrl, act = S
    worst = {f: 0.0 for f in FIELDS}
    for e in envs:
        d = oracle_env(po, models[e] if models else model, qpos[e], qvel[e], None if noise else ctrl[e], act[e], K, noise, e, None if xfrc is None else xfrc[e])
        for f in FIELDS:
            worst[f] = max(worst[f], _err(got[f][e], d.field(f)))
    print(f"{what}, {K} step(s), {len(list(envs))} envs against the oracle: " + ", ".join(f"{f} {v:.2e}" for f, v in worst.items()) + f" (bound {tol:.0e})")
    for f in FIELDS:
        assert worst[f] <= tol, f"{what}: {f} {worst[f]:.2e} > {tol:.0e}"


def against_generic(got, ref, tol, what, fields=EVERY):
    for f in fields:
        _close(got[f], ref[f], tol, f"{what}: {f} against the generic kernel")


def run(cm, S, K, mode=1, lane=None, setup=None, **kw):
    b = make(cm, S, mode=mode, **kw)
    if setup:
        setup(b)
    b.step(K)
    ran(b, (mode != 0) if lane is None else lane)
    out = snapshot(b)
    b.close()
    return out


# ------------------------------------------------------------------------------------------------------- 1. one step against the oracle
@pytest.mark.parametrize("which", ["S", "P"])
def test_one_step(oracle_built, which):
    model, cm, S = case(which)
    got = run(cm, S, 1)
    # (per stage, for the record: the acceleration stage adds a second evaluation order on top of the sweep's)
    ref = np.array([sm.oracle_field(oracle_env(oracle_built, model, S[0][e], S[1][e], S[2][e], S[3][e], 1), "sensordata") for e in range(NENV)])
    for name, types in (("velocity stage", VEL_TYPES), ("acceleration stage", ACC_TYPES)):
        w = max(_err(got["sensordata"][:, sm.sensor_slice(model, i)], ref[:, sm.sensor_slice(model, i)]) for i in sm.sensors_of(model, types))
        print(f"model {which}, {name} sensors, one step against the oracle: {w:.3e}")
    against_oracle(oracle_built, model, got, S, 1, 1e-11, range(NENV), f"model {which}")
    against_generic(got, run(cm, S, 1, mode=0), 1e-9, f"model {which}, one step")
    # the cutoffs are met by the drawn states (S): some envs sit on the bound, in both stages
    if which == "S":
        for i in (k for k in range(model["nsensor"]) if model["sensor_cutoff"][k] > 0):
            v, c = got["sensordata"][:, sm.sensor_slice(model, i)], float(model["sensor_cutoff"][i])
            assert np.all(np.abs(v) <= c) and np.sum(np.abs(v) == c) >= 4, (i, c)


# ------------------------------------------------------------------------------------- 2. closed forms, independent of the oracle
def test_closed_forms_on_a_pendulum():
    """Model P after one step against sm.pendulum_closed_forms: the sensors belong to the state the step started from and to the qacc it computed."""
    model, cm, S = case("P")
    got = run(cm, S, 1)
    sl = [sm.sensor_slice(model, i) for i in range(6)]
    worst = np.zeros(6)
    for e in range(NENV):
        want = sm.pendulum_closed_forms(model, S[0][e, 0], S[1][e, 0], got["qacc"][e, 0])
        for k in range(6):
            worst[k] = max(worst[k], _err(got["sensordata"][e][sl[k]], want[k]))
    names = ("gyro", "velocimeter", "accelerometer", "framelinacc", "force", "torque")
    print("model P against the closed forms: " + ", ".join(f"{n} {x:.2e}" for n, x in zip(names, worst)))
    assert np.all(worst <= 1e-11), dict(zip(names, worst))


def test_rest_without_gravity_reads_zero_and_the_base_reads_minus_gravity():
    """S at rest (qvel = 0, ctrl = 0, the slide at its spring's reference) without gravity: qacc = 0 and every velocity- and acceleration-stage sensor
    reads exactly zero.  With gravity on, whatever the arm does, the accelerometer on the base's site reads -R' g (R: the site's frame, from the model
    alone) and framelinacc of the second tree's root -g: bodies at rest."""
    model, cm, S = case("S", gravity="0 0 0")
    qpos = S[0].copy()
    qpos[:, 1] = float(model["qpos_spring"][1])
    still = (qpos, np.zeros_like(S[1]), np.zeros_like(S[2]), S[3])
    got = run(cm, still, 1)
    assert np.all(got["qacc"] == 0)
    for i in sm.sensors_of(model, VEL_TYPES | ACC_TYPES):
        assert np.all(got["sensordata"][:, sm.sensor_slice(model, i)] == 0), (i, int(model["sensor_type"][i]))
    for i in sm.sensors_of(model, {25, 26, 27}):   # (the frame axes are unit vectors)
        assert np.allclose(np.linalg.norm(got["sensordata"][:, sm.sensor_slice(model, i)], axis=1), 1, rtol=0, atol=1e-12)
    model, cm, S = case("S")
    got = run(cm, S, 1)
    g = np.asarray(model["gravity"], float)
    R = sm.quat_mat(model["body_quat"][1]) @ sm.quat_mat(model["site_quat"][0])
    acc = [i for i in sm.sensors_of(model, {1}) if int(model["sensor_objid"][i]) == 0][0]
    lin = [i for i in sm.sensors_of(model, {30}) if int(model["sensor_objtype"][i]) == 1 and int(model["sensor_objid"][i]) == 6][0]
    _close(got["sensordata"][:, sm.sensor_slice(model, acc)], np.tile(-R.T @ g, (NENV, 1)), 1e-11, "the base's accelerometer against -R' g")
    _close(got["sensordata"][:, sm.sensor_slice(model, lin)], np.tile(-g, (NENV, 1)), 1e-11, "framelinacc of the second root against -g")
    rest = [i for i in sm.sensors_of(model, VEL_TYPES) if (int(model["sensor_objtype"][i]), int(model["sensor_objid"][i])) in ((6, 0), (2, 6))]
    assert len(rest) == 2   # the gyro on the base's site, framelinvel of the second tree's root: velocities of bodies at rest
    for i in rest:
        assert np.all(got["sensordata"][:, sm.sensor_slice(model, i)] == 0), i


# ----------------------------------------------------------------------------------------------------------------------------- 3. rollout
@pytest.mark.parametrize("noisy", [True, False], ids=["ctrl_noise", "drawn_ctrl"])
def test_rollout(oracle_built, noisy):
    model, cm, S = case("S")
    kw = dict(noise=NOISE, ctrl=False) if noisy else {}
    got = run(cm, S, ROLLOUT, **kw)
    assert np.all(np.isfinite(got["sensordata"]))
    against_oracle(oracle_built, model, got, S, ROLLOUT, 1e-9, CHECK, "model S", noise=NOISE if noisy else None)
    against_generic(got, run(cm, S, ROLLOUT, mode=0, **kw), 1e-9, f"model S, {ROLLOUT} steps")


# --------------------------------------------------------------------------------------------------------------------- 4. launch handling
def test_launch_handling():
    model, cm, S = case("S")
    res = {}
    for name, parts in (("whole", [(1, 20)]), ("split", [(1, 7), (1, 13)]), ("mixed", [(1, 10), (0, 10), (1, 10)]), ("generic", [(0, 30)])):
        b = make(cm, S, noise=NOISE, ctrl=False)
        for mode, k in parts:
            b.set_lane_env(mode)
            b.step(k)
            ran(b, mode == 1)
        res[name] = snapshot(b)
        b.close()
    for f in EVERY:
        assert np.array_equal(res["whole"][f], res["split"][f]), f"splitting a launch changed {f}"
    against_generic(res["mixed"], res["generic"], 1e-9, "a generic launch in the middle")
    # sensors at every step: the launch ends with the same sensordata and state, bit for bit
    every = run(cm, S, 20, noise=NOISE, ctrl=False, setup=lambda b: b.set_sensors_every_step(True))
    for f in EVERY:
        assert np.array_equal(res["whole"][f], every[f]), f"set_sensors_every_step changed {f}"
    # mjDSBL_SENSOR: sensordata stays what it was set to
    off = sm.model_S()
    off["disableflags"] = int(off["disableflags"]) | DSBL_SENSOR
    marks = np.random.default_rng(2).uniform(-1, 1, (NENV, int(off["nsensordata"])))
    quiet = run(_engine().CompiledModel(off), S, 5, setup=lambda b: b.set("sensordata", marks))
    assert np.array_equal(quiet["sensordata"], marks)
    assert np.array_equal(quiet["qpos"], run(cm, S, 5)["qpos"])


# ---------------------------------------------------------------------------------------------------------------------------- 5. resets
def test_resets_inside_a_launch(oracle_built):
    """Env 5's qvel trips mj_checkVel at the first step; env 20's ctrl on the unlimited motor of the slide trips mj_checkAcc there.  The pass sits ahead
    of mj_checkAcc's verdict: the reset lane's sensordata of that step comes from the retry on the reset state."""
    po = oracle_built
    model, cm, S0 = case("S")
    qpos, qvel, ctrl, act = (a.copy() for a in S0)
    qvel[5, 0] = 1e12
    ctrl[20, 1] = 1e14
    S = (qpos, qvel, ctrl, act)
    for K in (1, 3):
        lane, gen, tidy = make(cm, S), make(cm, S, mode=0), make(cm, S0)
        for b in (lane, gen, tidy):
            b.step(K)
        ran(lane)
        ran(gen, False)
        ran(tidy)
        warn = [[b.warning(w) for w in range(8)] for b in (lane, gen)]
        assert warn[0] == warn[1], f"warning counters differ: {warn[0]} vs {warn[1]}"
        assert warn[0][4] == 0 and warn[0][5] == 1 and warn[0][6] == 1
        got, ref = snapshot(lane), snapshot(tidy)
        assert np.all(np.isfinite(got["sensordata"]))
        against_generic(got, snapshot(gen), 1e-9, f"after the resets, {K} step(s)")
        for e in (5, 20, 0, 21, 69):
            d = oracle_env(po, model, qpos[e], qvel[e], ctrl[e], act[e], K)
            for f in FIELDS:
                _close(got[f][e], d.field(f), 1e-9, f"{K} step(s), env {e} {f} against the oracle")
        others = np.ones(NENV, dtype=bool)
        others[[5, 20]] = False
        for f in EVERY:
            assert np.array_equal(got[f][others], ref[f][others]), f"a reset in the wavefront changed {f} of another lane"
        for b in (lane, gen, tidy):
            b.close()


# ---------------------------------------------------------------------------------------------------------------------------- 6. builds
def test_mode_2_per_env_parameters(oracle_built):
    """The overlay build: per-env mass and inertia (the pass reads the sweep's cinert), gravity (the bodies at rest read the env's) and joint parameters."""
    base, cm, S = case("S")
    R = draw(base, NENV, 7, which=("gravity", "mass", "joint"))
    twins = {e: twin_model(base, R, e) for e in CHECK}
    for K, tol in ((1, 1e-11), (20, 1e-9)):
        got = run(cm, S, K, mode=2, setup=lambda b: apply(b, R))
        against_oracle(oracle_built, base, got, S, K, tol, CHECK, "model S, mode 2", models=twins)
    plain = run(cm, S, 20, mode=2)
    assert _err(plain["sensordata"][1:], got["sensordata"][1:]) > 1e-6   # (the overlay reaches the sensors)


def test_xfrc_build(oracle_built):
    """The xfrc build on S without the base's wrench sensors, a wrench on every body: cfrc_ext enters the moving link's force / torque."""
    model, cm, S = case("S", base_wrench=False)
    nb = int(model["nbody"])
    rng = np.random.default_rng(6)
    wr = sm.sensors_of(model, {4, 5})
    assert len(wr) == 2
    for K, tol, fs, ts in ((1, 1e-11, 30, 5), (20, 1e-9, 5, 1)):
        X = np.concatenate([rng.uniform(-fs, fs, (NENV, nb, 3)), rng.uniform(-ts, ts, (NENV, nb, 3))], axis=2).reshape(NENV, 6 * nb)

        def setup(b):
            b.set_lane_env_xfrc(True)
            b.set("xfrc_applied", X)
        got = run(cm, S, K, setup=setup)
        against_oracle(oracle_built, model, got, S, K, tol, range(NENV) if K == 1 else CHECK, "model S with wrenches", xfrc=X)
        against_generic(got, run(cm, S, K, mode=0, setup=setup), 1e-9, f"model S with wrenches, {K} steps")
        if K == 1:
            free = run(cm, S, 1)
            for i in wr:
                assert np.abs(got["sensordata"][:, sm.sensor_slice(model, i)] - free["sensordata"][:, sm.sensor_slice(model, i)]).max() > 1e-6, i


def test_xfrc_with_a_wrench_sensor_on_the_base_runs_the_generic_kernel():
    """No xfrc build has a force / torque sensor on a body at rest: the batch runs the generic kernel, bit-equal to a mode-0 batch, and the model is not
    marked unavailable -- without the wrenches it runs the kernel."""
    model, cm, S = case("S")
    X = np.random.default_rng(9).uniform(-3, 3, (NENV, 6 * int(model["nbody"])))

    def setup(b):
        b.set_lane_env_xfrc(True)
        b.set("xfrc_applied", X)
    a = run(cm, S, 5, mode=1, lane=False, setup=setup)
    g = run(cm, S, 5, mode=0, setup=setup)
    for f in EVERY:
        assert np.array_equal(a[f], g[f]), f
    run(cm, S, 2)   # (asserts that the kernel ran)


def test_hwsim_build():
    model, cm, S = case("S")
    eff = np.random.default_rng(8).uniform(-2, 2, (NENV, 1))

    def setup(b):
        b.set_lane_env_hwsim(True)
        b.hwsim_configure([dict(joint=2, method="effort")])
        b.hwsim_set_command("effort", eff)
    got = run(cm, S, 20, setup=setup)
    against_generic(got, run(cm, S, 20, mode=0, setup=setup), 1e-9, "model S with a hwsim effort joint")
    assert _err(got["sensordata"], run(cm, S, 20)["sensordata"]) > 1e-6   # (the stage does act)
    # a velocity and a position joint below a moving parent: the stage writes their qvel ahead of the pass, which forms cdof_dot qvel with it as the generic
    # kernels' rne_post does
    rng = np.random.default_rng(9)
    vel, pos = rng.uniform(-1, 1, (NENV, 3)), rng.uniform(-0.02, 0.02, (NENV, 3))

    def setup3(b):
        b.set_lane_env_hwsim(True)
        b.hwsim_configure([dict(joint=0, method="effort"), dict(joint=1, method="position", kind="prismatic"), dict(joint=2, method="velocity")])
        b.hwsim_set_command("effort", eff.repeat(3, axis=1))
        b.hwsim_set_command("velocity", vel)
        b.hwsim_set_command("position", pos)
    for K in (1, 20):
        against_generic(run(cm, S, K, setup=setup3), run(cm, S, K, mode=0, setup=setup3), 1e-9, f"model S with hwsim position / velocity joints, {K} step(s)")


@pytest.mark.parametrize("variant", ["stateful", "gravcomp"])
def test_activation_states_and_gravity_compensation(oracle_built, variant):
    """The oracle has no gravity compensation of its own: its twin is the compensation-free model driven step by step with the compensation's joint
    forces in qfrc_applied (gravcomp_models.expected_step) -- which, as in MuJoCo, are no part of cfrc_int."""
    model, cm, S = case("S", **{variant: True})
    for K, tol in ((1, 1e-11), (20, 1e-9)):
        got = run(cm, S, K)
        envs = list(range(NENV) if K == 1 else CHECK)
        if variant == "gravcomp":
            import gravcomp_models as gm
            want = gm.expected_step(oracle_built, model, S[0][envs], S[1][envs], S[2][envs], K)
            for f in FIELDS:
                _close(got[f][envs], want[f], tol, f"model S, gravcomp, {K} step(s), {len(envs)} envs against the oracle: {f}")
        else:
            against_oracle(oracle_built, model, got, S, K, tol, envs, f"model S, {variant}")
        against_generic(got, run(cm, S, K, mode=0), 1e-9, f"model S, {variant}, {K} steps")
    if variant == "gravcomp":   # (compensation moves the arm, and is no part of cfrc_int: it reaches the base's force sensor through qacc alone)
        one, plain = run(cm, S, 1), run(case("S")[1], S, 1)
        assert _err(one["qacc"], plain["qacc"]) > 1e-3


# ------------------------------------------------------------------------------------------------------------------- 7. unchanged ground
def test_model_without_such_sensors_still_runs():
    """franka_like (the compiled-in kernel), 70 envs, 20 steps in mode 1 against mode 0."""
    from conftest import random_franka_state
    engine = _engine()
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    qpos, qvel = random_franka_state(model, NENV, 3)
    ctrl = np.random.default_rng(4).uniform(-3, 3, (NENV, model["nu"]))
    res = []
    for mode in (1, 0):
        b = engine.Batch(cm, NENV)
        b.set_lane_env(mode)
        b.set("qpos", qpos)
        b.set("qvel", qvel)
        b.set("ctrl", ctrl)
        b.step(20)
        assert b.lane_env_info() == (0, mode == 1), b.lane_env_error()
        res.append({f: b.get(f) for f in FIELDS})
        b.close()
    for f in res[0]:
        _close(res[0][f], res[1][f], 1e-9, f"franka_like {f}, lane = env against the generic kernel")
