"""GPU: body gravity compensation in the generic step kernels.  Expected values never come from the kernels: the oracle on the gravcomp-free
model with refdyn.gravcomp_force (the definition, tests/test_gravcomp.py ties it to two independent routes) in qfrc_applied, and -- for a
uniform coefficient alpha -- the oracle on the gravcomp-free model under gravity (1 - alpha) g."""
import numpy as np
import pytest

import gravcomp_models as gm

pytestmark = pytest.mark.gpu

ONE_STEP = 1e-11   # the project's one-step bound, relative to 1 + |x|
ROLLOUT = 1e-9     # the project's rollout bound

# Model C (contacts): |engine - oracle| / (1 + |oracle|) over qpos, qvel, qacc after 20 steps of the comparison the engine could already run
# before it knew gravcomp -- the gravcomp-free model under gravity (1 - alpha) g on both sides, same states -- measured on an MI355X
# (profiles/gravcomp.txt).  The gravcomp run differs from it only in where the gravity term is summed, so its bound is 10 x that figure.
# (States and kernels are deterministic: the figures reproduce to the digit from run to run.)  Key: (solver, integrator, alpha).
C_PARENT_ERR = {
    ("PGS", "Euler", 1.0): 6.291e-16,
    ("PGS", "Euler", 0.5): 1.339e-14,
    ("PGS", "Euler", 2.0): 8.904e-16,
    ("PGS", "RK4", 1.0): 8.282e-16,
    ("PGS", "RK4", 0.5): 6.146e-12,
    ("PGS", "RK4", 2.0): 5.792e-16,
    ("PGS", "implicitfast", 1.0): 6.291e-16,
    ("PGS", "implicitfast", 0.5): 1.339e-14,
    ("PGS", "implicitfast", 2.0): 8.904e-16,
    ("Newton", "Euler", 1.0): 6.218e-16,
    ("Newton", "Euler", 0.5): 1.174e-14,
    ("Newton", "Euler", 2.0): 6.828e-16,
    ("Newton", "RK4", 1.0): 6.626e-16,
    ("Newton", "RK4", 0.5): 9.263e-15,
    ("Newton", "RK4", 2.0): 5.639e-16,
    ("Newton", "implicitfast", 1.0): 6.218e-16,
    ("Newton", "implicitfast", 0.5): 1.174e-14,
    ("Newton", "implicitfast", 2.0): 6.828e-16,
}


def _engine():
    from mujoco_ros_pkgs_amd import engine
    return engine


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / (1 + np.abs(b).max())) if a.size else 0.0


def _batch(model, qpos, qvel, ctrl, lanes=0, keep=False):
    engine = _engine()
    b = engine.Batch(engine.CompiledModel(model), qpos.shape[0])
    b.set_lane_env(0)   # the generic kernels (the lane = env kernel: test_gpu_lane_env_gravcomp.py)
    if lanes:
        b.set_launch(lanes, 0)
    if keep:
        b.set_keep_frame(True)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if model["nu"]:
        b.set("ctrl", ctrl)
    return b


def _model(name, **kw):
    return gm.model_T(**kw) if name == "T" else gm.model_X(**kw)


_cache = {}


def _one_step_case(oracle, name):
    """(model, states, expectation of one step) -- computed once, shared, never written to."""
    if name not in _cache:
        m = _model(name)
        st = gm.states(m, 8, 11, name)
        _cache[name] = (m, st, gm.expected_step(oracle, m, *st))
    return _cache[name]


# ---- 1. one step, against the definition
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
@pytest.mark.parametrize("name", ["T", "X"])
def test_one_step_definition(oracle_built, name, lanes):
    m, (qpos, qvel, ctrl), want = _one_step_case(oracle_built, name)
    b = _batch(m, qpos, qvel, ctrl, lanes, keep=True)
    b.step(1)
    assert not b.lane_env_info()[1]
    got = {k: b.get(k) for k in want}
    b.close()
    gc = want["qfrc_passive"] - gm.expected_step(oracle_built, gm.without_gravcomp(m), qpos, qvel, ctrl)["qfrc_passive"] if lanes == 8 else None
    if gc is not None:
        assert np.abs(gc).max() > 0.5   # the term is there to be missed
    for k in ("qfrc_passive", "qacc", "qvel", "qpos", "sensordata"):
        err = _rel(got[k], want[k])
        print(f"{name} lanes {lanes} {k}: {err:.3e}")
        assert err <= ONE_STEP, (k, err)


# ---- 2. production frames: the fused launch on its compact / lean / wide / row-slot frame against the full frame (mjb_step1 + mjb_step2)
def _fused_vs_full(model, st, K, tol, what):
    qpos, qvel, ctrl = st
    b = _batch(model, qpos, qvel, ctrl)
    b.step(K)
    fused = {k: b.get(k) for k in ("qpos", "qvel", "qacc")}
    b.close()
    b = _batch(model, qpos, qvel, ctrl)
    for _ in range(K):
        b.step1()
        b.step2()
    full = {k: b.get(k) for k in fused}
    b.close()
    for k in fused:
        err = _rel(fused[k], full[k])
        print(f"{what} {k}: fused vs full {err:.3e}")
        assert err <= tol, (what, k, err)
    return fused


@pytest.mark.parametrize("integrator", ["Euler", "RK4", "implicitfast"])
@pytest.mark.parametrize("name", ["T", "X"])
def test_production_frames_unconstrained(name, integrator):
    m = _model(name, integrator=integrator)
    _fused_vs_full(m, gm.states(m, 8, 13, name), 5, ONE_STEP, f"{name} {integrator}")


@pytest.mark.parametrize("solver", ["PGS", "Newton", "CG"])
def test_production_frames_contacts(solver):
    m = gm.model_C(0.5, solver)
    st = gm.states(m, 8, 13, "C")
    _fused_vs_full(m, st, 5, ONE_STEP, f"C {solver}")
    b = _batch(m, *st, keep=True)   # (the scene is in contact: the rows are built, the lean frame's overlays are in use)
    b.step(5)
    assert (b.get("ncon") > 0).sum() >= 4
    b.close()


def test_production_frames_wide_and_row_slot():
    """Newton, capacities beyond the register-row kernels: the wide fused frame (more than 128 rows), the row-slot solver with its frame in LDS and in
    HBM (more than 256) -- each fused frame against its full frame at the one-step bound, like every other frame, and (a check of its own, at the rollout
    bound: another solver path) against the 60-row model."""
    from mujoco_ros_pkgs_amd import mjcf
    engine = _engine()
    base = gm.model_C(0.5, "Newton")
    st = gm.states(base, 8, 17, "C")
    ref = _fused_vs_full(base, st, 10, ONE_STEP, "C Newton")
    slot = set()
    for njmax in (200, 300, 1024):
        m = mjcf.Model(dict(base))
        m["nefcmax"] = njmax   # (the loader caps njmax at the scene's worst case)
        info = engine.CompiledModel(m).frame_info()
        slot.add(info)
        got = _fused_vs_full(m, st, 10, ONE_STEP, f"C Newton njmax {njmax}")
        for k in ref:
            err = _rel(got[k], ref[k])
            print(f"njmax {njmax} {k}: vs njmax 60 {err:.3e}")
            assert err <= ROLLOUT, (njmax, k, err)
    assert any(not s[0] for s in slot) and any(s[0] for s in slot) and any(s[0] and (s[1] or s[2]) for s in slot), slot


# ---- 3. rollouts, Euler: the oracle driven step by step with the definition in qfrc_applied
def _c_bound(solver, integrator, alpha):
    return 10 * C_PARENT_ERR[(solver, integrator, alpha)]


def _rollout_err(oracle, model, expect_fn, st, K=20, ne=4):
    qpos, qvel, ctrl = (a[:ne] for a in st)
    b = _batch(model, qpos, qvel, ctrl)
    b.step(K)
    got = {k: b.get(k) for k in ("qpos", "qvel", "qacc")}
    b.close()
    want = expect_fn(qpos, qvel, ctrl)
    return {k: _rel(got[k], want[k]) for k in got}


@pytest.mark.parametrize("case", ["T", "X", "C-PGS", "C-Newton"])
def test_rollout_against_the_definition(oracle_built, case):
    if case in ("T", "X"):
        m, name, tol = _model(case), case, ROLLOUT
    else:
        m, name, tol = gm.model_C(0.5, case[2:]), "C", _c_bound(case[2:], "Euler", 0.5)
    # (C: the states C_PARENT_ERR was measured on)
    err = _rollout_err(oracle_built, m, lambda q, v, c: gm.expected_step(oracle_built, m, q, v, c, nsteps=20), gm.states(m, 4, 29 if name == "C" else 19, name))
    print(f"{case}: 20 steps vs the oracle with the definition in qfrc_applied {err}, bound {tol:.3e}")
    assert max(err.values()) <= tol, err


# ---- 4. a uniform coefficient alpha is gravity (1 - alpha) g, under every integrator
def _oracle_rollout(oracle, model, qpos, qvel, ctrl, K):
    d = oracle.OracleData(model)
    out = {k: [] for k in ("qpos", "qvel", "qacc")}
    for e in range(qpos.shape[0]):
        d.reset()
        d.qpos[:], d.qvel[:] = qpos[e], qvel[e]
        d.ctrl[:] = ctrl[e]
        d.step(K)
        for k in out:
            out[k].append(np.array(getattr(d, k)))
    return {k: np.array(v) for k, v in out.items()}


ALPHAS = [1.0, 0.5, 2.0]
INTEGRATORS = ["Euler", "RK4", "implicitfast"]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_uniform_alpha_T(oracle_built, integrator, alpha):
    gc = np.r_[0.0, np.full(7, alpha)]
    m = gm.model_T(gc=gc, integrator=integrator)
    free = gm.scaled_gravity(gm.without_gravcomp(m), 1 - alpha)
    err = _rollout_err(oracle_built, m, lambda q, v, c: _oracle_rollout(oracle_built, free, q, v, c, 20), gm.states(m, 4, 23, "T"))
    print(f"T {integrator} alpha {alpha}: {err}")
    assert max(err.values()) <= ROLLOUT, err


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_uniform_alpha_C(oracle_built, solver, integrator, alpha):
    m = gm.model_C(alpha, solver, integrator)
    free = gm.model_C(0.0, solver, integrator, gravity_scale=1 - alpha)
    st = gm.states(m, 4, 29, "C")
    want = lambda q, v, c: _oracle_rollout(oracle_built, free, q, v, c, 20)
    parent = _rollout_err(oracle_built, free, want, st)   # what C_PARENT_ERR records (printed: the measurement run reads it)
    err = _rollout_err(oracle_built, m, want, st)
    print(f"C_PARENT_ERR ({solver!r}, {integrator!r}, {alpha}): {max(parent.values()):.3e},   with gravcomp: {max(err.values()):.3e}")
    assert max(err.values()) <= _c_bound(solver, integrator, alpha), (err, parent)


# ---- 5. the switches: with passive forces or gravity off, or zero gravity, the coefficients change no bit of any field
def _every_field(model, st):
    """Every data field the model has, after three fused steps.  (The model carries an accelerometer and a force sensor: mj_rnePostConstraint
    runs, so cfrc_int / cfrc_ext are computed like every other field.)"""
    from mujoco_ros_pkgs_amd.binding import Field
    b = _batch(model, *st, keep=True)
    b.step(3)
    out = {k: b.get(k) for k in Field.names if b.cm.field_size(k) > 0}
    b.close()
    return out


@pytest.mark.parametrize("how", ["passive", "gravity", "zero"])
def test_switches(how):
    kw = dict(gravity="0 0 0") if how == "zero" else dict(flags=f' {how}="disable"')
    m = gm.model_T(sensors=gm.POST_SENSORS, **kw)
    st = gm.states(m, 8, 31, "T")
    a, b = _every_field(m, st), _every_field(gm.without_gravcomp(m), st)
    assert "cfrc_int" in a and "cfrc_ext" in a and "qfrc_passive" in a and len(a) > 40
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_switches_on():
    """The counterpart: the same two batches without any switch differ, and by the term -- qfrc_passive of the first step by the definition."""
    from mujoco_ros_pkgs_amd import refdyn
    m = gm.model_T(sensors=gm.POST_SENSORS)
    st = gm.states(m, 8, 31, "T")
    out = []
    for model in (m, gm.without_gravcomp(m)):
        b = _batch(model, *st, keep=True)
        b.step(1)
        out.append(b.get("qfrc_passive"))
        b.close()
    want = np.array([refdyn.gravcomp_force(m, q) for q in st[0]])
    assert np.abs(want).max() > 0.5
    assert _rel(out[0] - out[1], want) <= ONE_STEP


def test_per_env_mass_and_gravity(oracle_built):
    """The force takes the env's mass and the env's gravity (mjb_set_env_body_mass / mjb_set_env_gravity): every env against the oracle on ITS model."""
    from mujoco_ros_pkgs_amd import mjcf
    m = gm.model_T()
    n = 8
    qpos, qvel, ctrl = gm.states(m, n, 37, "T")
    rng = np.random.default_rng(41)
    mass = m["body_mass"] * rng.uniform(0.6, 1.5, (n, m["nbody"]))
    grav = np.asarray(m["gravity"]) * rng.uniform(0.5, 1.5, (n, 3))
    b = _batch(m, qpos, qvel, ctrl, keep=True)
    b.set_env_body_mass(mass)
    b.set_env_gravity(grav)
    b.step(1)
    got = {k: b.get(k) for k in ("qfrc_passive", "qacc", "qvel", "qpos")}
    b.close()
    for e in range(n):
        me = mjcf.with_body_mass(m, mass[e])
        me["gravity"] = grav[e]
        want = gm.expected_step(oracle_built, me, qpos[e:e + 1], qvel[e:e + 1], ctrl[e:e + 1])
        for k in got:
            err = _rel(got[k][e], want[k][0])
            assert err <= ONE_STEP, (e, k, err)
