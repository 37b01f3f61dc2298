"""GPU: joint limits under PGS in the lane = env kernel (one env per lane; a model with limit rows is built by hiprtc and runs the plain build of the
one-wavefront form).  70 envs: one wavefront plus a 6-lane tail; the states are constructed (tests/lane_env_limit_models.py): every count of active
rows from 0 to 4, both sides of every limit, neighbouring lanes with different active sets."""
import numpy as np
import pytest

import lane_env_limit_models as lm

pytestmark = pytest.mark.gpu

NENV = lm.NENV
NOISE = (5.0, 0.1, 777, 1000)
STATE = ("qpos", "qvel", "qacc", "sensordata")


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


def _against_oracle(b, want, what):
    """One step's results of every env against the oracle's: 1e-11 in the project's relative measure, the two counts as integers."""
    for k in lm.FIELDS:
        err = _rel(b.get(k), want[k])
        print(f"{what}, {k}: {err:.3e}")
        assert err <= 1e-11, (what, k, err)
    assert np.array_equal(b.get("nefc").ravel(), want["nefc"]), what
    assert np.array_equal(b.get("solver_iter").ravel(), want["solver_iter"]), what


@pytest.fixture(scope="module")
def case():
    m = lm.model_L()
    return m, _engine().CompiledModel(m), lm.states_L(m)


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
    b = _batch(cm, -1, st)   # the automatic mode keeps the generic kernels for a model with limits
    b.step(2)
    assert not b.lane_env_info()[1]
    b.close()


def test_one_step_against_the_oracle(oracle_built, case):
    m, cm, st = case
    want = lm.reference_L()
    b = _batch(cm, 1, st)
    b.step(1)
    assert b.lane_env_info()[1], b.lane_env_error()
    _against_oracle(b, want, "lane = env, one step")
    assert sorted(set(b.get("nefc").ravel())) == [0, 1, 2, 3, 4]
    b.close()


def test_one_row_closed_form():
    """Model P: one slide, one row, no warmstart.  f = max(0, -b / AR) from the model's numbers -- mass + armature, the default solref / solimp with the
    joint past solimp's width (the impedance is its end value) --, reached in the first sweep; the second finds nothing to improve: solver_iter == 2."""
    m = lm.model_P()
    cm = _engine().CompiledModel(m)
    qpos, qvel, ctrl = lm.states_P(m)
    b = _batch(cm, 1, (qpos, qvel, ctrl))
    b.step(1)
    assert b.lane_env_info() == (-2, True), b.lane_env_error()
    M = 1.7 + 0.05
    lo, hi = -0.1, 0.15
    q, v = qpos[:, 0], qvel[:, 0]
    smooth = (-9.81 * 1.7 + 2 * ctrl[:, 0]) / M
    side = np.where(q < lo, 1.0, np.where(q > hi, -1.0, 0.0))   # J
    pos = np.where(side > 0, q - lo, hi - q)
    imp, dmax, tc, dr = 0.95, 0.95, 0.02, 1.0
    R = (1 - imp) * float(m["dof_invweight0"][0]) / imp
    K, B = 1 / (dmax * dmax * tc * tc * dr * dr), 2 / (dmax * tc)
    aref = -B * side * v - K * imp * pos
    AR = 1 / M + R
    f = np.where(side != 0, np.maximum(0.0, -(side * smooth - aref) / AR), 0.0)
    assert np.count_nonzero(f > 0) >= 40 and np.count_nonzero(side > 0) >= 20 and np.count_nonzero(side < 0) >= 20
    qacc = smooth + side * f / M
    want = {"qacc": qacc[:, None], "qfrc_constraint": (side * f)[:, None], "qvel": (v + 0.002 * qacc)[:, None],
            "qpos": (q + 0.002 * (v + 0.002 * qacc))[:, None]}
    for k, w in want.items():
        err = _rel(b.get(k), w)
        print(f"model P against the closed form, {k}: {err:.3e}")
        assert err <= 1e-11, (k, err)
    assert np.array_equal(b.get("nefc").ravel(), (side != 0).astype(int))
    assert np.array_equal(b.get("solver_iter").ravel(), np.where(side == 0, 0, np.where(f > 0, 2, 1)))
    b.close()
    cm.close()


def test_iteration_cap(oracle_built, case):
    st = case[2]
    m = lm.model_L(iterations=3)
    cm = _engine().CompiledModel(m)
    want = lm.reference_L(iterations=3)
    assert np.count_nonzero(want["solver_iter"] == 3) >= 8
    b = _batch(cm, 1, st)
    b.step(1)
    assert b.lane_env_info()[1], b.lane_env_error()
    _against_oracle(b, want, "iterations = 3")
    b.close()
    cm.close()


@pytest.fixture(scope="module")
def generic_rollout(case):
    """60 steps under ctrl noise on the generic kernels: shared by the rollout, launch-split and hand-over tests (not written into)."""
    m, cm, st = case
    b = _batch(cm, 0, st)
    b.set_ctrl_noise(*NOISE)
    b.step(60)
    assert not b.lane_env_info()[1]
    out = {k: b.get(k) for k in STATE}
    b.close()
    return out


def test_rollout_against_the_generic_kernels(case, generic_rollout):
    m, cm, st = case
    b = _batch(cm, 1, st)
    b.set_ctrl_noise(*NOISE)
    b.step(60)
    assert b.lane_env_info()[1], b.lane_env_error()
    got = {k: b.get(k) for k in STATE}
    b.close()
    for k in STATE:
        err = max(_rel(got[k][e], generic_rollout[k][e]) for e in range(NENV))
        print(f"lane = env vs generic, 60 noisy steps, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)
    # the rows act: the same launch on the tree without its limits ends elsewhere
    free = _engine().CompiledModel(lm.model_L(limits=False))
    b = _batch(free, 1, st)
    b.set_ctrl_noise(*NOISE)
    b.step(60)
    assert b.lane_env_info()[1]
    assert np.abs(b.get("qpos") - got["qpos"]).max() > 1e-3
    b.close()
    free.close()


def test_launch_split(case):
    """The warmstart crosses the launch boundary: (60,) and (17, 43) are the same rollout bit for bit."""
    m, cm, st = case
    fields = STATE + ("time", "ctrl")
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


def test_hand_over_between_the_kernels(case, generic_rollout):
    m, cm, st = case
    b = _batch(cm, 0, st)
    b.set_ctrl_noise(*NOISE)
    for mode in (0, 1, 0):
        b.set_lane_env(mode)
        b.step(20)
        assert b.lane_env_info()[1] == (mode == 1)
    for k in STATE:
        err = max(_rel(b.get(k)[e], generic_rollout[k][e]) for e in range(NENV))
        print(f"20 generic + 20 lane = env + 20 generic vs 60 generic, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)
    b.close()


def test_resets_with_active_rows(oracle_built, case):
    """An env whose qvel trips mj_checkVel and one whose ctrl on the unlimited motor trips mj_checkAcc, both with active rows (the retry runs the
    constraint stage again on the reset state): state, qacc, sensordata and the warning counters against the oracle and the generic kernels."""
    m, cm, st = case
    qpos, qvel, ctrl = (a.copy() for a in st)
    sides = lm.sides_L()
    ev, ea = 2, 64
    assert np.any(sides[ev]) and np.any(sides[ea])
    qvel[ev, 1] = 3e10       # beyond mjMAXVAL
    ctrl[ea, 1] = 1e12       # the motor on j2 has no ctrlrange: qacc beyond mjMAXVAL
    want = lm.oracle_steps(oracle_built, m, qpos, qvel, ctrl)
    assert want["warning"][5] == 1 and want["warning"][6] == 1 and want["warning"][4] == 0
    out = {}
    for mode in (0, 1):
        b = _batch(cm, mode, (qpos, qvel, ctrl))
        b.step(1)
        assert b.lane_env_info()[1] == (mode == 1)
        for k in STATE:
            err = _rel(b.get(k), want[k])
            print(f"resets, mode {mode}, one step vs oracle, {k}: {err:.3e}")
            assert err <= 1e-11, (mode, k, err)
        assert [b.warning(w) for w in (4, 5, 6)] == [0, 1, 1], mode
        b.step(9)
        out[mode] = {k: b.get(k) for k in STATE}
        assert [b.warning(w) for w in (4, 5, 6)] == [0, 1, 1], mode
        b.close()
    for k in STATE:
        err = max(_rel(out[1][k][e], out[0][k][e]) for e in range(NENV))
        print(f"resets, 10 steps, lane = env vs generic, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)


@pytest.mark.parametrize("flag", ["warmstart", "refsafe"])
def test_disable_flags(oracle_built, case, flag):
    """mjDSBL_WARMSTART / mjDSBL_REFSAFE on the model (refsafe: with j1's time constant below two timesteps, so the flag changes the row): one step and a
    10-step rollout against the oracle."""
    st = case[2]
    m = lm.model_L(flags=f' {flag}="disable"')
    if flag == "refsafe":
        m["jnt_solref"] = np.array(m["jnt_solref"], float)
        m["jnt_solref"][0] = (0.003, 1.0)
    cm = _engine().CompiledModel(m)
    b = _batch(cm, 1, st)
    b.step(1)
    assert b.lane_env_info()[1], b.lane_env_error()
    _against_oracle(b, lm.oracle_steps(oracle_built, m, *st), f"{flag} disabled, one step")
    b.step(9)
    want = lm.oracle_steps(oracle_built, m, *st, nsteps=10)
    for k in STATE:
        err = max(_rel(b.get(k)[e], want[k][e]) for e in range(NENV))
        print(f"{flag} disabled, 10 steps vs oracle, {k}: {err:.3e}")
        assert err <= 1e-9, (k, err)
    b.close()
    cm.close()


def test_overrides_keep_the_generic_kernels(case):
    """No overlay and no xfrc build has the constraint stage: a mode-2 batch with a per-env mass override, and a batch with set_lane_env_xfrc and a
    written wrench, run the generic kernels, bit-equal to a mode-0 batch."""
    m, cm, st = case
    rng = np.random.default_rng(47)
    mass = m["body_mass"] * rng.uniform(0.6, 1.5, (NENV, m["nbody"]))
    xfrc = rng.uniform(-1, 1, (NENV, 6 * m["nbody"]))

    def run(mode, what):
        b = _batch(cm, mode, st)
        if what == "mass":
            b.set_env_body_mass(mass)
        else:
            b.set_lane_env_xfrc(mode != 0)
            b.set("xfrc_applied", xfrc)
        b.set_ctrl_noise(5.0, 0.1, 5, 0)
        b.step(20)
        assert not b.lane_env_info()[1] and b.lane_env_info()[0] == -2, b.lane_env_error()
        out = {k: b.get(k) for k in STATE}
        b.close()
        return out
    for what, mode in (("mass", 2), ("xfrc", 1)):
        ref, got = run(0, what), run(mode, what)
        for k in STATE:
            assert np.array_equal(ref[k], got[k]), (what, k)
