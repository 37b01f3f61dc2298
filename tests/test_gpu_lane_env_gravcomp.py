"""GPU: body gravity compensation in the lane = env kernel (one env per lane; a model with gravcomp is built by hiprtc and runs the
one-wavefront form).  70 envs: one wavefront plus a 6-lane tail."""
import numpy as np
import pytest

import gravcomp_models as gm

pytestmark = pytest.mark.gpu

NENV = 70


def _engine():
    from mujoco_ros_pkgs_amd import engine
    return engine


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / (1 + np.abs(b).max()))


def _batch(cm, mode, st, n=NENV):
    b = _engine().Batch(cm, n)
    b.set_lane_env(mode)
    b.set("qpos", st[0][:n])
    b.set("qvel", st[1][:n])
    b.set("ctrl", st[2][:n])
    return b


@pytest.fixture(scope="module")
def case():
    m = gm.model_T()
    return m, _engine().CompiledModel(m), gm.states(m, NENV, 43, "T")


def test_runs_the_kernel_in_form_0(case):
    m, cm, st = case
    b = _batch(cm, 1, st)
    b.step(2)
    assert b.lane_env_info() == (-2, True), b.lane_env_error()   # no compiled-in topology: hiprtc's; the kernel ran
    assert b.lane_env_last_form() == 0
    prev = b.set_lane_env_form(3)
    try:
        b.step(2)
        assert b.lane_env_info()[1] and b.lane_env_last_form() == 0   # whatever form is asked for
    finally:
        b.set_lane_env_form(prev)
    b.close()


def test_one_step_definition(oracle_built, case):
    m, cm, st = case
    want = gm.expected_step(oracle_built, m, *st)
    b = _batch(cm, 1, st)
    b.step(1)
    assert b.lane_env_info()[1]
    for k in ("qacc", "qvel", "qpos", "sensordata"):
        err = _rel(b.get(k), want[k])
        print(f"lane = env, one step, {k}: {err:.3e}")
        assert err <= 1e-11, (k, err)
    b.close()


def test_rollout_against_the_generic_kernel(case):
    m, cm, st = case
    out = {}
    for mode in (0, 1):
        b = _batch(cm, mode, st)
        b.set_ctrl_noise(5.0, 0.1, 777, 1000)
        b.step(60)
        assert b.lane_env_info()[1] == (mode == 1)
        out[mode] = {k: b.get(k) for k in ("qpos", "qvel", "qacc", "sensordata")}
        b.close()
    for k in out[0]:
        err = max(_rel(out[1][k][e], out[0][k][e]) for e in range(NENV))
        print(f"lane = env vs generic, 60 noisy steps, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)
    # the term matters over this rollout: without the coefficients the same launch ends elsewhere
    b = _batch(_engine().CompiledModel(gm.without_gravcomp(m)), 1, st)
    b.set_ctrl_noise(5.0, 0.1, 777, 1000)
    b.step(60)
    assert np.abs(b.get("qpos") - out[1]["qpos"]).max() > 1e-3
    b.close()


def test_launch_split(case):
    m, cm, st = case
    fields = ("qpos", "qvel", "qacc", "sensordata", "time", "ctrl")
    res = []
    for parts in ((60,), (17, 43)):
        b = _batch(cm, 1, st)
        b.set_ctrl_noise(5.0, 0.1, 99, 0)
        for k in parts:
            b.step(k)
            assert b.lane_env_info()[1]
        res.append({f: b.get(f) for f in fields})
        b.close()
    for f in fields:
        assert np.array_equal(res[0][f], res[1][f]), f


def test_mode_2_per_env_mass_and_gravity(case):
    m, cm, st = case
    rng = np.random.default_rng(47)
    mass = m["body_mass"] * rng.uniform(0.6, 1.5, (NENV, m["nbody"]))
    grav = np.asarray(m["gravity"]) * rng.uniform(0.5, 1.5, (NENV, 3))
    out = {}
    for mode in (0, 2):
        b = _batch(cm, mode, st)
        b.set_env_body_mass(mass)
        b.set_env_gravity(grav)
        b.set_ctrl_noise(5.0, 0.1, 5, 0)
        b.step(60)
        assert b.lane_env_info()[1] == (mode == 2), b.lane_env_error()
        out[mode] = {k: b.get(k) for k in ("qpos", "qvel", "qacc", "sensordata")}
        b.close()
    for k in out[0]:
        err = max(_rel(out[2][k][e], out[0][k][e]) for e in range(NENV))
        print(f"mode 2 vs generic, per-env mass and gravity, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)
    # (the overrides reach the term: the model's own mass and gravity end elsewhere)
    b = _batch(cm, 1, st)
    b.set_ctrl_noise(5.0, 0.1, 5, 0)
    b.step(60)
    assert np.abs(b.get("qpos") - out[2]["qpos"]).max() > 1e-3
    b.close()


def test_automatic_mode_keeps_the_generic_kernel(case):
    m, cm, st = case
    b = _batch(cm, -1, st)
    b.step(3)
    assert not b.lane_env_info()[1]
    b.close()
