"""Batched joint-space dynamics on the device (Batch.set_dynamics / dynamics, csrc/mjb_dyn.hip) against the references of dynamics_models.py
(refdyn.mass_matrix, numpy solves, a Richardson-extrapolated difference of refdyn.jac_point: plain numpy that shares nothing with the kernel), through
round trips that run through the engine's forward pass, the acceleration sensors, across launch shapes bit for bit, under per-env parameters, and the
interface's contract.  The references and their teeth are those test_dynamics_reference.py checks without a device.

Measure: the worst |got - want| / (1 + |want|) over the entries of an output (jacobian_models.rel_err).  Bounds: M, MV and the sensor identity EXACT_TOL =
1e-11 (no finite difference, no solve in the reference); MinvV max(1e-11, 100 x the difference between np.linalg.solve and a Cholesky solve); the round
trips max(1e-11, 100 x the distance of solve(M, M V) to V); Jdotv max(1e-11, 100 x the distance between the Richardson extrapolations from steps
1e-4 / 2e-4 and 2e-4 / 4e-4) -- the ACC_TOL rule of the sensor tests, and no bound may exceed 1e-8.  ID is compared bit for bit with the sum formed in
numpy.  Every test prints its figures and bounds (pytest -s).  No bound is taken from the kernel's distance to the reference."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import dynamics_models as dm
import jacobian_models as jm
from mujoco_ros_pkgs_amd import mjcf, refdyn

pytestmark = pytest.mark.gpu

ALL = dm.OUTPUTS
NVEC = dm.NVEC
MANY = 4096


@contextlib.contextmanager
def compiled(m):
    from mujoco_ros_pkgs_amd import engine
    cm = engine.CompiledModel(m)
    try:
        yield cm
    finally:
        cm.close()


@contextlib.contextmanager
def batch(cm, qpos, qvel=None):
    from mujoco_ros_pkgs_amd import engine
    b = engine.Batch(cm, len(qpos))
    try:
        b.set("qpos", qpos)
        if qvel is not None:
            b.set("qvel", qvel)
        yield b
    finally:
        b.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def all_zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint64).any()


def states(name, n):
    """(qpos, qvel) of envs 0 .. n - 1: env e has the same state for every n"""
    qpos, qvel = jm.states(name, n=jm.NENV_MANY if n <= jm.NENV_MANY else MANY)
    return qpos[:n], qvel[:n]


@functools.lru_cache(maxsize=None)
def ref_mass(name, e, nvec=NVEC):
    qpos, _ = states(name, e + 1)
    return dm.ref_mass(jm.model(name), qpos[e], dm.vectors(name, e + 1, nvec)[e])


@functools.lru_cache(maxsize=None)
def ref_jdotv(name, e):
    pts, pnt = jm.points(name)
    qpos, qvel = states(name, e + 1)
    return dm.ref_jdotv(jm.model(name), qpos[e], qvel[e], pts, pnt)


def id_in_numpy(b, out, envs=None):
    """(MV + qfrc_bias) - qfrc_passive formed in numpy, in that order, from the same launch's MV and the frame's fields"""
    bias, passive = b.get("qfrc_bias"), b.get("qfrc_passive")
    if envs is not None:
        bias, passive = bias[envs], passive[envs]
    return (out["MV"] + bias[:, None, :]) - passive[:, None, :]


def check(m, out, mass, jd, what):
    """out: the five outputs of len(mass) envs; mass: dm.ref_mass per env; jd: dm.ref_jdotv per env (or None).  Asserts the bounds, returns the figures."""
    own_s = max(r["own"]["solve"] for r in mass)
    tol = {"M": jm.EXACT_TOL, "MV": jm.EXACT_TOL, "MinvV": dm.bound(own_s, what)}
    err = {k: max(jm.rel_err(out[k][e], r[k]) for e, r in enumerate(mass)) for k in tol if k in out}
    line = f"{what}: " + "  ".join(f"{k} {err[k]:.1e} (bound {tol[k]:.1e}" + (f", own {own_s:.1e})" if k == "MinvV" else ")") for k in err)
    if jd is not None and "Jdotv" in out:
        own_j = max(o for _, o in jd)
        tol["Jdotv"] = dm.bound(own_j, what)
        err["Jdotv"] = max(jm.rel_err(out["Jdotv"][e], r) for e, (r, _) in enumerate(jd))
        line += f"  Jdotv {err['Jdotv']:.1e} (bound {tol['Jdotv']:.1e}, own {own_j:.1e})"
    print(line)
    if "M" in out:
        rel = dm.related(m)
        for e in range(len(mass)):
            assert same_bits(out["M"][e], out["M"][e].T), (what, e, "M equals its transpose to the bit")
            assert all_zero_bits(out["M"][e][~rel]), (what, e, "a structural zero of M is +0.0 to the bit")
    for k in err:
        assert err[k] <= tol[k], (what, k, err[k], tol[k])
    return err, tol


def formula_on_device_fields(m, b, pts, pnt, envs, qvel):
    """Jdot qvel by dynamics_models.jdotv_formula on the DEVICE's cvel, cdof_dot, subtree_com and the points' positions from refdyn: no finite
    difference in it, for the models whose Richardson reference is not tabulated"""
    cvel, cdd, com, qpos = b.get("cvel"), b.get("cdof_dot"), b.get("subtree_com"), b.get("qpos")
    out = []
    for e in envs:
        kin = refdyn.kinematics(m, qpos[e])
        row = []
        for k, (kind, oid) in enumerate(jm.resolve(m, pts)):
            body, p = jm.point_world(m, kin, kind, oid, pnt[k])
            row.append(dm.jdotv_formula(m, qvel[e], cvel[e].reshape(-1, 6), cdd[e].reshape(-1, 6), com[e].reshape(-1, 3)[int(m["body_rootid"][body])], p, body))
        out.append(row)
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------------ 1. after forward()
@pytest.mark.parametrize("name", ["two_roots", "wide", "franka_like"])
def test_against_the_reference_after_forward(name):
    """Measured on an MI355X (7 envs, nvec = 3; own error of the reference and bound for the two that have one):
    two_roots    M 9.8e-17  MV 2.1e-16  MinvV 9.5e-14 (own 2.1e-14, bound 1.0e-11)  Jdotv 2.5e-12 (own 3.1e-12, bound 3.1e-10)
    wide         M 5.3e-16  MV 6.6e-16  MinvV 1.6e-12 (own 7.0e-13, bound 7.0e-11)  Jdotv 6.0e-12 (own 7.2e-12, bound 7.2e-10)
    franka_like  M 1.1e-15  MV 1.1e-15  MinvV 2.0e-15 (own 1.5e-15, bound 1.0e-11)  Jdotv 2.5e-12 (own 3.3e-12, bound 3.3e-10)
    ID equals the sum formed in numpy to the bit on all three."""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    n, nv = jm.NENV, int(m["nv"])
    qpos, qvel = states(name, n)
    V = dm.vectors(name, n)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
        b.set_dyn_vectors(V)
        out = b.dynamics()
        want_id = id_in_numpy(b, out)
    assert sorted(out) == sorted(ALL) and out["M"].shape == (n, nv, nv) and out["Jdotv"].shape == (n, len(pts), 6)
    assert all(out[k].shape == (n, NVEC, nv) for k in ("MV", "MinvV", "ID")) and all(a.dtype == np.float64 for a in out.values())
    check(m, out, [ref_mass(name, e) for e in range(n)], [ref_jdotv(name, e) for e in range(n)], name + " after forward()")
    assert same_bits(out["ID"], want_id), "ID = (MV + qfrc_bias) - qfrc_passive, rounded in that order"
    assert np.abs(out["ID"] - out["MV"]).max() > 0.01, "the bias is not small"
    assert np.ptp(out["M"], axis=0).max() > 0.01, "the envs have different mass matrices"


# ------------------------------------------------------------------------------------------------------------------ 2. round trip through the engine
@pytest.mark.parametrize("name", ["franka_like", "wide", "two_roots"])
def test_round_trip_through_the_forward_pass(name):
    """Inverse, then forward dynamics: with qfrc_applied = ID[:, 0] - qfrc_actuator, forward() gives qacc_smooth = V[:, 0]; and MinvV of the vectors
    ID - qfrc_bias + qfrc_passive gives V back.  Bound: max(1e-11, 100 x the distance of np.linalg.solve(M, M V) to V).
    Measured on an MI355X (7 envs; qacc_smooth against V / MinvV against V; the reference's own round trip; bound):
    franka_like  3.6e-14 / 5.0e-14  (own 1.0e-15, bound 1.0e-11)
    wide         1.0e-13 / 1.2e-13  (own 3.8e-14, bound 1.0e-11)
    two_roots    8.9e-15 / 1.2e-14  (own 3.2e-15, bound 1.0e-11)"""
    m = jm.model(name)
    n = jm.NENV
    qpos, qvel = states(name, n)
    V = dm.vectors(name, n)
    tol = dm.bound(max(ref_mass(name, e)["own"]["round"] for e in range(n)), name)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_dynamics(nvec=NVEC, outputs=("ID", "MinvV"))
        b.set_dyn_vectors(V)
        out = b.dynamics()
        bias, passive = b.get("qfrc_bias"), b.get("qfrc_passive")
        b.set("qfrc_applied", out["ID"][:, 0] - b.get("qfrc_actuator"))
        b.forward()
        e1 = jm.rel_err(b.get("qacc_smooth"), V[:, 0])
        b.set_dyn_vectors(out["ID"] - bias[:, None, :] + passive[:, None, :])
        e2 = jm.rel_err(b.dynamics()["MinvV"], V)
    print(f"{name}: qacc_smooth under qfrc_applied = ID - qfrc_actuator against V {e1:.1e}, MinvV of ID - bias + passive against V {e2:.1e} (bound {tol:.1e})")
    assert e1 <= tol and e2 <= tol


# ------------------------------------------------------------------------------------------------------------------ 3. the sensor identity
def test_sensor_identity_on_the_device():
    """two_roots with <framelinacc> / <frameangacc> on s_a2 and s_paddle, its gravity on: sensordata = J qacc + Jdotv (angular) and J qacc + Jdotv -
    gravity (linear), J from set_jac_points and Jdotv from this interface on the same sites, within EXACT_TOL.
    Measured on an MI355X (7 envs): 1.0e-15, the largest reading 3.7 (bound 1.0e-11)."""
    m = dm.sensor_model()
    sites = list(dm.SENSOR_SITES)
    sl = dm.sensor_slices(m)
    g = np.asarray(m["gravity"], float)
    n = jm.NENV
    qpos, qvel = states("two_roots", n)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_jac_points(sites, outputs=("J",))
        b.set_dynamics(outputs=("Jdotv",), points=sites)
        J, jd = b.jacobians()["J"], b.dynamics()["Jdotv"]
        qacc, sens = b.get("qacc"), b.get("sensordata")
    acc = np.einsum("ekrd,ed->ekr", J, qacc) + jd
    worst = 0.0
    for k, s in enumerate(sites):
        worst = max(worst, jm.rel_err(acc[:, k, :3] - g, sens[:, sl[s][0]]), jm.rel_err(acc[:, k, 3:], sens[:, sl[s][1]]))
    print(f"sensor identity on the device: {worst:.1e} (bound {jm.EXACT_TOL:.0e}); the largest reading {np.abs(sens).max():.2g}")
    assert worst <= jm.EXACT_TOL and np.abs(sens).max() > 1


# ------------------------------------------------------------------------------------------------------------------ 4. after step(2) with keep_frame
@pytest.mark.parametrize("name,nenv,sample", [("franka_like", MANY, (0, 1, 63, 64, 1000, 2047, 4032, 4095)), ("two_roots", jm.NENV, tuple(range(jm.NENV)))])
def test_after_a_fused_step_with_keep_frame(name, nenv, sample):
    """After step(2) the frame holds the forward pass of the second step: the poses AND the velocities after ONE step (a twin batch stepped once
    supplies both), as mjData after mj_step.  M belongs to that qpos; ID to that frame's qfrc_bias / qfrc_passive; Jdotv to that frame's velocities,
    not to qvel after both steps -- the kernel takes the second step's velocity update back.  xpos of the frame is checked first against the
    reference's kinematics at that qpos.
    Measured on an MI355X:
    franka_like (8 of 4096)  M 8.3e-16  MV 1.1e-15  MinvV 3.1e-15 (own 7.5e-16, bound 1.0e-11)  Jdotv 4.5e-12 (own 4.1e-12, bound 4.1e-10)  xpos 2.2e-16
    two_roots (7)            M 1.3e-16  MV 1.5e-16  MinvV 2.6e-14 (own 6.3e-15, bound 1.0e-11)  Jdotv 3.2e-12 (own 3.1e-12, bound 3.1e-10)  xpos 1.1e-16
    qvel moves by 0.46 (franka_like) and 0.02 (two_roots) in the second step."""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = states(name, nenv)
    sample = list(sample)
    V = dm.vectors(name, nenv)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b, batch(cm, qpos, qvel) as twin:
        twin.step(1)
        q1, v1 = twin.get("qpos")[sample], twin.get("qvel")[sample]
        b.set_keep_frame(True)
        b.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
        b.set_dyn_vectors(V)
        b.step(2)
        out = {k: a[sample] for k, a in b.dynamics().items()}
        v2, xpos = b.get("qvel")[sample], b.get("xpos")[sample]
        want_id = id_in_numpy(b, out, sample)
    ex = max(jm.rel_err(xpos[i].reshape(-1, 3), refdyn.kinematics(m, q1[i])["xpos"]) for i in range(len(sample)))
    print(f"{name}: frame after step(2): xpos against kinematics(qpos after one step) {ex:.1e}; qvel moved by {np.abs(v2 - v1).max():.1e} in the second step")
    assert ex <= jm.EXACT_TOL and np.abs(v2 - v1).max() > 1e-4
    mass = [dm.ref_mass(m, q1[i], V[sample[i]]) for i in range(len(sample))]
    jd = [dm.ref_jdotv(m, q1[i], v1[i], pts, pnt) for i in range(len(sample))]
    check(m, out, mass, jd, f"{name} after step(2) with keep_frame, {len(sample)} of {nenv} envs")
    assert same_bits(out["ID"], want_id)
    wrong = max(jm.rel_err(dm.ref_jdotv(m, q1[i], v2[i], pts, pnt)[0], jd[i][0]) for i in range(2))
    assert wrong > 1e-6, "Jdot qvel at the velocities after both steps is another number"


# ------------------------------------------------------------------------------------------------------------------ 5. launch shapes
@pytest.mark.parametrize("name", ["two_roots", "wide"])
def test_equal_bits_across_launch_shapes(name):
    """Envs 0 - 6 inside batches of 1, 7, 70 and 4096 envs; vector 0 configured alone against nvec = 3; one point against the full point set (and, on
    two_roots, the set repeated to 48 points: more than a block takes of one env, so they go in tiles of 42); each output configured alone against
    all five together.  Every value has the same bits everywhere."""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    n = jm.NENV
    qpos, qvel = states(name, MANY)
    V = dm.vectors(name, n)
    with compiled(m) as cm:
        with batch(cm, qpos[:n], qvel[:n]) as b7:
            b7.forward()
            b7.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
            b7.set_dyn_vectors(V)
            base = b7.dynamics()
            with batch(cm, qpos, qvel) as bmany, batch(cm, qpos[:jm.NENV_MANY], qvel[:jm.NENV_MANY]) as b70, batch(cm, qpos[:1], qvel[:1]) as b1:
                for b, envs in ((bmany, n), (b70, n), (b7, n), (b1, 1)):
                    b.forward()
                    b.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
                    b.set_dyn_vectors(V[:envs], 0, envs)
                    got = b.dynamics(0, envs)
                    for key in ALL:
                        assert same_bits(got[key], base[key][:envs]), (name, b.nenv, key)
                for b, envs in ((b70, n), (b1, 1)):
                    b.set_dynamics(nvec=1, outputs=ALL, points=pts[:1], pnt=pnt[:1])   # vector 0 alone, one point
                    b.set_dyn_vectors(V[:envs, :1], 0, envs)
                    got = b.dynamics(0, envs)
                    for key in ("MV", "MinvV", "ID"):
                        assert same_bits(got[key], base[key][:envs, :1]), (name, b.nenv, "vector 0 alone", key)
                    assert same_bits(got["Jdotv"], base["Jdotv"][:envs, :1]) and same_bits(got["M"], base["M"][:envs])
                    for key in ALL:   # each output alone
                        b.set_dynamics(nvec=NVEC, outputs=(key,), points=pts, pnt=pnt)
                        if key in ("MV", "MinvV", "ID"):
                            b.set_dyn_vectors(V[:envs], 0, envs)
                        got = b.dynamics(0, envs)
                        assert sorted(got) == [key] and same_bits(got[key], base[key][:envs]), (name, b.nenv, "alone", key)
                if name == "two_roots":
                    rep = 6
                    b70.set_dynamics(outputs=("Jdotv",), points=list(pts) * rep, pnt=np.tile(pnt, (rep, 1)))
                    got = b70.dynamics(0, n)["Jdotv"]
                    for r in range(rep):
                        assert same_bits(got[:, r * len(pts):(r + 1) * len(pts)], base["Jdotv"]), (name, "48 points", r)


# ------------------------------------------------------------------------------------------------------------------ 6. per-env parameters
def test_per_env_masses_inertias_and_armature():
    """Each env against the reference on its own copy of the model (set_env_body_mass, set_env_dof_params): M, MV and MinvV follow the env's twin model;
    with every env in env 0's state two envs still differ by more than 1e-3.
    Measured on an MI355X (7 envs): M 2.3e-16, MV 1.7e-16, MinvV 4.9e-15 (own 5.2e-15), bounds 1.0e-11; in one state two envs differ by 0.088 .. 0.90 in M
    and 0.88 .. 7.6 in MinvV (the tests' measure)."""
    name = "two_roots"
    m = jm.model(name)
    n, nv, nb = jm.NENV, int(m["nv"]), int(m["nbody"])
    qpos, qvel = states(name, n)
    V = dm.vectors(name, n)
    rng = np.random.default_rng(9)
    mass = np.asarray(m["body_mass"], float) * rng.uniform(0.5, 2.0, (n, nb))
    inertia = np.asarray(m["body_inertia"], float) * rng.uniform(0.5, 2.0, (n, nb, 1))
    arm = rng.uniform(0.0, 0.05, (n, nv))
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.set_env_body_mass(mass, inertia)
        b.set_env_dof_params(armature=arm)
        b.forward()
        b.set_dynamics(nvec=NVEC, outputs=("M", "MV", "MinvV"))
        b.set_dyn_vectors(V)
        out = b.dynamics()
        b.set("qpos", np.tile(qpos[0], (n, 1)))
        b.set("qvel", np.tile(qvel[0], (n, 1)))
        b.forward()
        b.set_dyn_vectors(np.tile(V[0], (n, 1, 1)))
        shared = b.dynamics()
    pairs = [(e, f) for e in range(n) for f in range(e + 1, n)]
    d_m = sorted(jm.rel_err(shared["M"][e], shared["M"][f]) for e, f in pairs)
    d_s = sorted(jm.rel_err(shared["MinvV"][e], shared["MinvV"][f]) for e, f in pairs)
    print(f"envs in one state: M differs between two envs by {d_m[0]:.1e} .. {d_m[-1]:.1e}, MinvV by {d_s[0]:.1e} .. {d_s[-1]:.1e}")
    assert d_m[-1] > 1e-3 and d_s[-1] > 1e-3
    refs = [dm.ref_mass(mjcf.with_joint_params(mjcf.with_body_mass(m, mass[e], inertia[e]), armature=arm[e]), qpos[e], V[e]) for e in range(n)]
    check(m, out, refs, None, "two_roots with per-env masses, inertias and armature")
    assert max(jm.rel_err(refs[e]["M"], ref_mass(name, e)["M"]) for e in range(n)) > 1e-3, "M follows the env's parameters"
    assert max(jm.rel_err(refs[e]["MinvV"], ref_mass(name, e)["MinvV"]) for e in range(n)) > 1e-3


# ------------------------------------------------------------------------------------------------------------------ 7. the hand and the largest model
def test_the_hand_with_its_fingertips():
    """shadow_hand_like, five fingertip sites, 64 envs, nvec = 2, 3 sampled envs against the references.  Measured on an MI355X: M 3.9e-18, MV 2.6e-18,
    MinvV 3.9e-14 (own 8.9e-15, bound 1.0e-11), Jdotv 1.3e-12 (own 1.5e-12, bound 1.5e-10); Jdotv against the formula in numpy on the device's own
    cvel, cdof_dot and subtree_com 1.3e-16 (bound 1.0e-11)."""
    name, nenv, sample, nvec = "shadow_hand_like", 64, [0, 31, 63], 2
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = states(name, nenv)
    V = dm.vectors(name, nenv, nvec)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_dynamics(nvec=nvec, outputs=ALL, points=[p[1] for p in pts])   # (sites by name, no pnt)
        b.set_dyn_vectors(V)
        out = {k: a[sample] for k, a in b.dynamics().items()}
        want_id = id_in_numpy(b, out, sample)
        direct = formula_on_device_fields(m, b, pts, pnt, sample, qvel)
    check(m, out, [ref_mass(name, e, nvec) for e in sample], [ref_jdotv(name, e) for e in sample], "shadow_hand_like, 5 fingertips, 3 of 64 envs")
    assert same_bits(out["ID"], want_id)
    ef = jm.rel_err(out["Jdotv"], direct)
    print(f"shadow_hand_like: Jdotv against the formula in numpy on the device's cvel, cdof_dot, subtree_com {ef:.1e} (bound {jm.EXACT_TOL:.0e})")
    assert ef <= jm.EXACT_TOL


def test_the_largest_model():
    """deep: one chain of nv = 64 dofs (nM = 2080), the most mjb_compile takes, 3 envs, nvec = 5 and the five DEEP_POINTS against the references; then
    40 vectors (the first five the same) and the points repeated to 50, so that both vectors and points go in tiles, and env 0 alone in a 1-env batch:
    the same bits.  (One env per block; 40 vectors go in tiles of 29, 50 points in tiles of 42.)
    Measured on an MI355X: M 8.5e-16, MV 1.9e-15, MinvV 3.7e-12 (own 2.8e-12, bound 2.8e-10), Jdotv 2.3e-12 (own 5.2e-12, bound 5.2e-10); Jdotv against the
    formula in numpy on the device's own cvel, cdof_dot and subtree_com 4.2e-15 (bound 1.0e-11)."""
    name, nenv, nvec = "deep", 3, 5
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = states(name, nenv)
    V = dm.vectors(name, nenv, nvec)
    with compiled(m) as cm:
        with batch(cm, qpos, qvel) as b:
            b.forward()
            b.set_dynamics(nvec=nvec, outputs=ALL, points=pts, pnt=pnt)
            b.set_dyn_vectors(V)
            out = b.dynamics()
            want_id = id_in_numpy(b, out)
            direct = formula_on_device_fields(m, b, pts, pnt, range(nenv), qvel)
            rep, many = 10, 40
            b.set_dynamics(nvec=many, outputs=ALL, points=list(pts) * rep, pnt=np.tile(pnt, (rep, 1)))
            b.set_dyn_vectors(dm.vectors(name, nenv, many))
            tiled = b.dynamics()
        check(m, out, [ref_mass(name, e, nvec) for e in range(nenv)], [ref_jdotv(name, e) for e in range(nenv)], "deep (nv = 64), 5 vectors, 5 points, 3 envs")
        assert same_bits(out["ID"], want_id)
        ef = jm.rel_err(out["Jdotv"], direct)
        print(f"deep: Jdotv against the formula in numpy on the device's cvel, cdof_dot, subtree_com {ef:.1e} (bound {jm.EXACT_TOL:.0e})")
        assert ef <= jm.EXACT_TOL
        assert same_bits(tiled["M"], out["M"]) and all(same_bits(tiled[k][:, :nvec], out[k]) for k in ("MV", "MinvV", "ID")), "vectors in tiles"
        assert all(same_bits(tiled["Jdotv"][:, r * len(pts):(r + 1) * len(pts)], out["Jdotv"]) for r in range(rep)), "points in tiles"
        with batch(cm, qpos[:1], qvel[:1]) as b1:
            b1.forward()
            b1.set_dynamics(nvec=2, outputs=("MinvV", "Jdotv"), points=pts[:2], pnt=pnt[:2])
            b1.set_dyn_vectors(V[:1, :2])
            one = b1.dynamics()
            assert same_bits(one["MinvV"], out["MinvV"][:1, :2]) and same_bits(one["Jdotv"], out["Jdotv"][:1, :2])


# ------------------------------------------------------------------------------------------------------------------ 8. the contract
def test_contract():
    from mujoco_ros_pkgs_amd import binding, engine
    lib = binding.load_library()
    live0 = lib.mjb_debug_live_resources()
    name = "two_roots"
    m = jm.model(name)
    pts, pnt = jm.points(name)
    n, nv = jm.NENV, int(m["nv"])
    qpos, qvel = states(name, n)
    V = dm.vectors(name, n)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    M, MV, MINVV, ID, JDOTV, IN_V = 1, 2, 4, 8, 16, 256

    def configure(b, outputs, nvec=1, ty=(0,), oid=(0,), p=None, npoint=None, null_points=False):
        ty, oid = np.asarray(ty, np.int32), np.asarray(oid, np.int32)
        p = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
        return lib.mjb_dyn_configure(b.ptr, nvec, len(ty) if npoint is None else npoint, None if null_points else ty.ctypes.data_as(pi),
                                     None if null_points else oid.ctypes.data_as(pi), None if p is None else p.ctypes.data_as(pd), outputs)

    def refused(rc, rule):
        assert rc == -1 and rule.encode() in lib.mjb_last_error(), (rule, lib.mjb_last_error())   # MJB_EINVAL

    with compiled(m) as cm:
        with batch(cm, qpos, qvel) as b:
            with pytest.raises(engine.EngineError, match="before mjb_dyn_configure"):
                b.eval_dynamics_async()
            assert not lib.mjb_dyn_device_ptr(b.ptr, M) and not lib.mjb_dyn_device_ptr(b.ptr, IN_V)
            buf = np.zeros(n * max(nv * nv, NVEC * nv, len(pts) * 6))
            refused(lib.mjb_dyn_get(b.ptr, M, 0, n, buf.ctypes.data_as(pd)), "before mjb_dyn_configure")
            refused(lib.mjb_dyn_set_vectors(b.ptr, 0, n, buf.ctypes.data_as(pd)), "before mjb_dyn_configure")
            # every MJB_EINVAL of mjb_dyn_configure, each with the rule in its message
            refused(configure(b, 0), "at least one of the MJB_DYN_OUT_*")
            refused(configure(b, 32 | M), "at least one of the MJB_DYN_OUT_*")
            refused(configure(b, IN_V | M), "MJB_DYN_IN_V names the input")
            for bit in (MV, MINVV, ID):
                refused(configure(b, bit, nvec=0), "at least 1 for MV, MINVV or ID")
            refused(configure(b, M, nvec=-1), "never negative")
            refused(configure(b, JDOTV, npoint=0), "npoint must be at least 1")
            refused(configure(b, JDOTV, null_points=True), "npoint must be at least 1")
            refused(configure(b, JDOTV, ty=[4]), "unknown object type")
            refused(configure(b, JDOTV, ty=[0], oid=[int(m["nsite"])]), "outside [0,")
            refused(configure(b, JDOTV, ty=[1], oid=[-1]), "outside [0,")
            refused(configure(b, JDOTV, p=[[0.0, np.nan, 0.0]]), "non-finite pnt")
            nvec_c, np_c = C.c_int(-1), C.c_int(-1)
            assert lib.mjb_dyn_count(b.ptr, C.byref(nvec_c), C.byref(np_c)) == 0 and (nvec_c.value, np_c.value) == (0, 0), "a refused configuration leaves none"
            with pytest.raises(ValueError):
                b.set_dynamics(outputs=("M", "Lambda"))
            with pytest.raises(ValueError):
                b.set_dynamics(outputs=("Jdotv",), points=["no such site"])

            # a freshly configured V is zero: MV all +0.0 bits, ID = qfrc_bias - qfrc_passive to the bit; eval needs current frames first
            b.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):
                b.dynamics()
            b.forward()
            zero = b.dynamics()
            assert all_zero_bits(zero["MV"]) and all_zero_bits(zero["MinvV"])
            bias, passive = b.get("qfrc_bias"), b.get("qfrc_passive")
            assert same_bits(zero["ID"], np.repeat((bias - passive)[:, None, :], NVEC, axis=1)) and np.abs(zero["ID"]).max() > 0.01
            world = [k for k, p in enumerate(pts) if p == ("site", "s_world")]
            assert world and all_zero_bits(zero["Jdotv"][:, world]), "a point on the world body gives +0.0"
            assert np.abs(zero["Jdotv"][:, [k for k in range(len(pts)) if k not in world]]).max() > 0.1
            b.set_dyn_vectors(V)
            first = b.dynamics()

            # staleness: qvel written -> M / MV / MinvV still evaluate, ID and Jdotv refuse until the next forward()
            b.set("qvel", qvel[::-1].copy())
            with pytest.raises(engine.EngineError, match="qvel has been written"):
                b.dynamics()
            b.set_dynamics(nvec=NVEC, outputs=("M", "MV", "MinvV"))
            b.set_dyn_vectors(V)
            still = b.dynamics()
            assert all(same_bits(still[k], first[k]) for k in still), "M, MV and MinvV do not care about qvel"
            for key in ("ID", "Jdotv"):
                b.set_dynamics(nvec=NVEC, outputs=(key,), points=pts, pnt=pnt)
                with pytest.raises(engine.EngineError, match="qvel has been written"):
                    b.dynamics()
            b.set_dynamics(nvec=NVEC, outputs=ALL, points=pts, pnt=pnt)
            b.set_dyn_vectors(V)
            b.forward()
            moved = b.dynamics()
            assert same_bits(moved["M"], first["M"]) and not same_bits(moved["Jdotv"], first["Jdotv"]) and not same_bits(moved["ID"], first["ID"])
            # ... through set_many and set_packed too
            fid = (C.c_int * 1)(binding.Field.ids["qvel"])
            host = np.ascontiguousarray(qvel, dtype=np.float64)
            ptrs = (pd * 1)(host.ctypes.data_as(pd))
            assert lib.mjb_set_many(b.ptr, 1, fid, 0, n, ptrs) == 0 and lib.mjb_synchronize(b.ptr) == 0
            with pytest.raises(engine.EngineError, match="qvel has been written"):
                b.dynamics()
            b.forward()
            assert sorted(b.dynamics()) == sorted(ALL)
            assert lib.mjb_set_packed(b.ptr, 1, fid, 0, n, host.ctypes.data_as(pd)) == 0 and lib.mjb_synchronize(b.ptr) == 0
            with pytest.raises(engine.EngineError, match="qvel has been written"):
                b.dynamics()
            b.forward()
            # qpos written -> everything refuses
            b.set("qpos", qpos[::-1].copy())
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):
                b.dynamics()
            b.step()
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):   # after step() without keep_frame
                b.dynamics()
            b.forward()
            assert not same_bits(b.dynamics()["M"], first["M"]), "the evaluation followed the frames"
            b.step1()
            between = b.dynamics()   # between step1 and step2
            b.step2()
            after = b.dynamics()     # the frame of the step's forward pass, qvel integrated behind it
            assert same_bits(between["M"], after["M"]) and same_bits(between["ID"], after["ID"])
            assert jm.rel_err(after["Jdotv"], between["Jdotv"]) <= jm.EXACT_TOL, "Jdotv behind step2 belongs to the frame's velocities"

            # an output that was not configured
            b.forward()
            b.set_dynamics(nvec=NVEC, outputs=("M", "MV"))
            for bit in (MINVV, ID, JDOTV, M | MV, IN_V):
                refused(lib.mjb_dyn_get(b.ptr, bit, 0, n, buf.ctypes.data_as(pd)), "is not one MJB_DYN_OUT_* bit of the configuration")
            assert not lib.mjb_dyn_device_ptr(b.ptr, MINVV) and not lib.mjb_dyn_device_ptr(b.ptr, JDOTV) and lib.mjb_dyn_device_ptr(b.ptr, IN_V)
            with pytest.raises(engine.EngineError):
                b.dyn_device_ptr("ID")
            assert lib.mjb_dyn_get(b.ptr, M, 0, n + 1, buf.ctypes.data_as(pd)) != 0, "env range"
            b.set_dynamics(outputs=("M",))
            assert not lib.mjb_dyn_device_ptr(b.ptr, IN_V), "no vectors without an output of theirs"
            refused(lib.mjb_dyn_set_vectors(b.ptr, 0, n, buf.ctypes.data_as(pd)), "no vectors")

            # reconfiguration replaces the shapes; the device pointers serve the same numbers, V included
            b.set_dynamics(nvec=2, outputs=ALL, points=pts[:3], pnt=pnt[:3])
            b.set_dyn_vectors(V[:, :2])
            out = b.dynamics()
            assert lib.mjb_dyn_count(b.ptr, C.byref(nvec_c), C.byref(np_c)) == 0 and (nvec_c.value, np_c.value) == (2, 3)
            assert out["MV"].shape == (n, 2, nv) and out["Jdotv"].shape == (n, 3, 6)
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for key in ALL + ("V",):
                p = b.dyn_device_ptr(key)
                want = np.ascontiguousarray(V[:, :2]) if key == "V" else out[key]
                back = np.empty_like(want)
                assert p and hip.hipMemcpy(back.ctypes.data, p, back.nbytes, 2) == 0 and same_bits(back, want), key
            part = b.dynamics(2, 5)
            assert all(same_bits(part[k], out[k][2:5]) for k in ALL)
            # V written on the device through its pointer
            newV = np.ascontiguousarray(V[:, 1:3])
            assert hip.hipMemcpy(b.dyn_device_ptr("V"), newV.ctypes.data, newV.nbytes, 1) == 0
            assert same_bits(b.dynamics()["MV"][:, 0], out["MV"][:, 1])
        # reconfiguring frees and reallocates cleanly: batch after batch, configuration after configuration, nothing left behind
        for rounds in range(3):
            with batch(cm, qpos, qvel) as b:
                b.forward()
                for outs, nvec in ((ALL, 3), (("M",), 0), (("MinvV", "Jdotv"), 1), (ALL, 5)):
                    b.set_dynamics(nvec=nvec, outputs=outs, points=pts, pnt=pnt)
                    assert sorted(b.dynamics()) == sorted(outs)
    with compiled(mjcf.compile_xml_string("<mujoco><worldbody><geom name='g' type='sphere' size='0.1'/><site name='s'/></worldbody></mujoco>")) as cm0:
        with batch(cm0, np.zeros((1, 0))) as b0:
            refused(configure(b0, M), "no dofs")
    assert lib.mjb_debug_live_resources() == live0
