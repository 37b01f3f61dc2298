"""Batched Jacobians on the device (Batch.set_jac_points / jacobians, csrc/mjb_jac.hip) against the reference of jacobian_models.py (refdyn.kinematics,
jac_point, mass_matrix: plain numpy that shares nothing with the kernel), through physical identities that run through the engine's forward pass,
across launch shapes bit for bit, under per-env parameters, and the interface's contract.  The models, states, point sets and their teeth are those
test_jacobian_reference.py checks without a device.

Measure: the worst |got - want| / (1 + |want|) over the entries of an output.  Bounds: J and vel EXACT_TOL = 1e-11 (test_sensor_reference.py's bound for
a reference without a finite difference); MinvJT and Ainv go through M^-1, where the reference carries an error of its own -- the difference between
np.linalg.solve and a Cholesky solve of the same system, in the same measure -- and their bound is max(EXACT_TOL, 100 x that difference), the ACC_TOL
rule of the sensor tests.  Every test prints its figures and bounds (pytest -s) and records in its docstring what it measured on an MI355X: the worst
over its envs and points, `own` = the reference's own error, bound = max(1e-11, 100 own).  No bound is taken from the kernel's distance to the reference."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import jacobian_models as jm
from mujoco_ros_pkgs_amd import mjcf, refdyn

pytestmark = pytest.mark.gpu

ALL = jm.OUTPUTS


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


def check(out, refs, what):
    """out: Batch.jacobians() of len(refs) envs; refs: jm.ref_outputs per env.  Returns the figures."""
    own = {k: max(r["own"][k] for r in refs) for k in ("MinvJT", "Ainv")}
    tol = {"J": jm.EXACT_TOL, "vel": jm.EXACT_TOL, "MinvJT": jm.acc_tol(own["MinvJT"]), "Ainv": jm.acc_tol(own["Ainv"])}
    err = {k: max(jm.rel_err(out[k][e], r[k]) for e, r in enumerate(refs)) for k in out}
    print(f"{what}: " + "  ".join(f"{k} {err[k]:.1e} (bound {tol[k]:.1e}" + (f", own {own[k]:.1e})" if k in own else ")") for k in out))
    for e, r in enumerate(refs):
        for k in range(len(r["bodies"])):
            if "J" in out:
                assert all_zero_bits(out["J"][e, k][:, r["zero"][k]]), (what, e, k, "a column of a dof that does not move the body is 0.0 to the bit")
            if "Ainv" in out:
                assert same_bits(out["Ainv"][e, k], out["Ainv"][e, k].T), (what, e, k, "Ainv equals its transpose to the bit")
            if r["bodies"][k] == 0:
                assert all(all_zero_bits(out[key][e, k]) for key in out), (what, e, k, "every output of a point on the world body is zero")
    for k in out:
        assert err[k] <= tol[k], (what, k, err[k], tol[k])
    return err, tol


def reference(m, qpos, qvel, pts, pnt, envs):
    return [jm.ref_outputs(m, qpos[e], qvel[e], pts, pnt) for e in envs]


# ------------------------------------------------------------------------------------------------------------------ 1. after forward()
@pytest.mark.parametrize("name", ["two_roots", "wide", "franka_like"])
def test_against_the_reference_after_forward(name):
    """Measured on an MI355X (7 envs; J / MinvJT / Ainv / vel, own error of the reference and bound for the two that go through M^-1):
    two_roots    J 3.7e-16  MinvJT 2.8e-14 (own 6.6e-15, bound 1.0e-11)  Ainv 1.8e-14 (own 6.1e-15, bound 1.0e-11)  vel 4.6e-16
    wide         J 4.4e-16  MinvJT 1.5e-12 (own 2.9e-13, bound 2.9e-11)  Ainv 2.3e-13 (own 1.2e-14, bound 1.0e-11)  vel 6.1e-16
    franka_like  J 6.8e-16  MinvJT 3.4e-15 (own 8.4e-16, bound 1.0e-11)  Ainv 3.0e-15 (own 4.6e-16, bound 1.0e-11)  vel 7.5e-16"""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:jm.NENV] for a in jm.states(name))
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_jac_points(pts, outputs=ALL, pnt=pnt)
        out = b.jacobians()
        nv = int(m["nv"])
        assert sorted(out) == sorted(ALL) and out["J"].shape == (jm.NENV, len(pts), 6, nv) and out["MinvJT"].shape == out["J"].shape
        assert out["Ainv"].shape == (jm.NENV, len(pts), 6, 6) and out["vel"].shape == (jm.NENV, len(pts), 6) and all(a.dtype == np.float64 for a in out.values())
        check(out, reference(m, qpos, qvel, pts, pnt, range(jm.NENV)), name + " after forward()")
        assert np.ptp(out["J"], axis=0).max() > 0.01, "the envs have different Jacobians"


# ------------------------------------------------------------------------------------------------------------------ 2. after step(2) with keep_frame
@pytest.mark.parametrize("name,nenv,sample", [("franka_like", 4096, (0, 1, 63, 64, 1000, 2047, 4032, 4095)), ("two_roots", jm.NENV, tuple(range(jm.NENV)))])
def test_after_a_fused_step_with_keep_frame(name, nenv, sample):
    """After step(2) the frame holds the forward pass of the second step: the poses at qpos after ONE step (a twin batch stepped once supplies it), as
    mjData after mj_step; vel multiplies that J with the batch's qvel, the state after both steps.  Both are checked first: xpos of the frame against
    the reference's kinematics at that qpos, and qpos after two steps = integrate_pos(qpos after one, qvel after two, h), the semi-implicit Euler rule.
    (A batch of 4096 envs of franka_like runs the lane = env kernel for plain fused steps; with keep_frame the launcher keeps the generic kernels, which
    dump the frame -- the test is about what the frame then holds, whichever kernel wrote it.)
    Measured on an MI355X:
    franka_like (8 of 4096)  J 5.5e-16  MinvJT 3.1e-15 (own 1.0e-15)  Ainv 3.6e-15 (own 5.3e-16)  vel 5.3e-16   xpos 2.2e-16  Euler rule 1.7e-18
    two_roots (7)            J 7.0e-16  MinvJT 3.1e-14 (own 7.2e-15)  Ainv 2.3e-14 (own 8.6e-15)  vel 5.4e-16   xpos 1.1e-16  Euler rule 7.1e-17
    (every bound 1.0e-11)"""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:nenv] for a in jm.states(name, n=max(nenv, jm.NENV_MANY)))
    sample = list(sample)
    with compiled(m) as cm, batch(cm, qpos, qvel) as b, batch(cm, qpos, qvel) as twin:
        twin.step(1)
        q1 = twin.get("qpos")[sample]
        b.set_keep_frame(True)
        b.set_jac_points(pts, outputs=ALL, pnt=pnt)
        b.step(2)
        out = b.jacobians()
        q2, v2, xpos = b.get("qpos")[sample], b.get("qvel")[sample], b.get("xpos")[sample]
        h = float(np.asarray(m["timestep"]).ravel()[0])
        ex = max(jm.rel_err(xpos[i].reshape(-1, 3), refdyn.kinematics(m, q1[i])["xpos"]) for i in range(len(sample)))
        ee = max(jm.rel_err(q2[i], refdyn.integrate_pos(m, q1[i], v2[i], h)) for i in range(len(sample)))
        print(f"{name}: frame after step(2): xpos against kinematics(qpos after one step) {ex:.1e}, qpos2 = integrate(qpos1, qvel2, h) {ee:.1e}")
        assert ex <= jm.EXACT_TOL and ee <= jm.EXACT_TOL
        assert np.abs(q2 - qpos[sample]).max() > 1e-4, "the envs moved"
        refs = [jm.ref_outputs(m, q1[i], v2[i], pts, pnt) for i in range(len(sample))]
        check({k: a[sample] for k, a in out.items()}, refs, f"{name} after step(2) with keep_frame, {len(sample)} of {nenv} envs")
        # J of EVERY env is the same bits when it is asked for alone: then no solve follows the output in the kernel, whose in-place substitution
        # must wait for the block's last read of the rows
        for outs in (("J",), ("J", "Ainv")):
            b.set_jac_points(pts, outputs=outs, pnt=pnt)
            assert same_bits(b.jacobians()["J"], out["J"]), (name, outs)


# ------------------------------------------------------------------------------------------------------------------ 3. physical identities
def test_identities_through_the_forward_pass():
    """Through engine code the Jacobian kernel shares nothing with (xfrc_applied's projection, the forward dynamics), on two_roots, contacts off.
    a. Wrench at the centre of mass: forward() with xfrc_applied[body] = w and forward() with qfrc_applied = J' w (J of the bodycom point) give the same qacc.
    b. Response to a wrench at any point: with dqacc = qacc(qfrc_applied = J' w) - qacc(qfrc_applied = 0), dqacc = MinvJT' w and J dqacc = Ainv w.  For b
       the envs are at rest in zero gravity (set_env_gravity), where qacc(0) is zero: at the states' own velocities |qacc| is some hundred times |dqacc|
       and the difference would carry the rounding of two large accelerations, not of the quantity under test.
    Bounds: those of test 1 for MinvJT (a, and b's first identity) and for Ainv (b's second).
    Measured on an MI355X (7 envs): a 7.1e-15   b dqacc 1.1e-14, J dqacc 5.4e-15   (bounds 1.0e-11): every identity meets the bound of test 1."""
    name = "two_roots"
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:jm.NENV] for a in jm.states(name))
    n, nv, nb = jm.NENV, int(m["nv"]), int(m["nbody"])
    refs = reference(m, qpos, qvel, pts, pnt, range(n))
    tol_m = jm.acc_tol(max(r["own"]["MinvJT"] for r in refs))
    tol_a = jm.acc_tol(max(r["own"]["Ainv"] for r in refs))
    rng = np.random.default_rng(5)
    with compiled(m) as cm:
        # a
        com_pts = [("bodycom", "paddle"), ("bodycom", "a2"), ("bodycom", "base")]
        with batch(cm, qpos, qvel) as b:
            b.set_jac_points(com_pts, outputs=("J",))
            worst = 0.0
            for kind, body in com_pts:
                k, bid = com_pts.index((kind, body)), m["names"]["body"].index(body)
                w = rng.uniform(-2, 2, (n, 6))
                xf = np.zeros((n, nb, 6))
                xf[:, bid] = w
                b.set("xfrc_applied", xf.reshape(n, -1))
                b.set("qfrc_applied", np.zeros((n, nv)))
                b.forward()
                qacc_x = b.get("qacc")
                J = b.jacobians()["J"][:, k]
                b.set("xfrc_applied", np.zeros((n, nb * 6)))
                b.set("qfrc_applied", np.einsum("erd,er->ed", J, w))
                b.forward()
                qacc_q = b.get("qacc")
                assert np.abs(qacc_x).max() > 1
                worst = max(worst, jm.rel_err(qacc_q, qacc_x))
            print(f"identity a, wrench at the centre of mass: qacc(xfrc_applied) against qacc(J' w) {worst:.1e} (bound {tol_m:.1e})")
            assert worst <= tol_m
        # b
        with batch(cm, qpos, np.zeros_like(qvel)) as b:
            b.set_env_gravity(np.zeros((n, 3)))
            b.set_jac_points(pts, outputs=ALL, pnt=pnt)
            b.forward()
            out = b.jacobians()
            qacc0 = b.get("qacc")
            assert np.abs(qacc0).max() <= 1e-13, "at rest without gravity"
            e1 = e2 = 0.0
            for k in range(len(pts)):
                w = rng.uniform(-2, 2, (n, 6))
                b.set("qfrc_applied", np.einsum("erd,er->ed", out["J"][:, k], w))
                b.forward()
                dq = b.get("qacc") - qacc0
                e1 = max(e1, jm.rel_err(dq, np.einsum("erd,er->ed", out["MinvJT"][:, k], w)))
                e2 = max(e2, jm.rel_err(np.einsum("erd,ed->er", out["J"][:, k], dq), np.einsum("erc,ec->er", out["Ainv"][:, k], w)))
            print(f"identity b, response to a wrench: dqacc against MinvJT' w {e1:.1e} (bound {tol_m:.1e}), J dqacc against Ainv w {e2:.1e} (bound {tol_a:.1e})")
            assert e1 <= tol_m and e2 <= tol_a


# ------------------------------------------------------------------------------------------------------------------ 4. launch shapes
@pytest.mark.parametrize("name", ["two_roots", "wide"])
def test_equal_bits_across_launch_shapes(name):
    """Envs 0 - 6 of a 70-env batch, a 7-env batch and a 1-env batch hold the same states; the point set is cut to 1, 3 and all of its points (and
    repeated to 48 points on two_roots: more than a block takes of one env, so its points go in tiles of 42), each output is asked for alone and with
    the others -- the launch's envs per block, points per block and LDS plan follow all of these.  Every (env, point) gives the same bits everywhere."""
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = jm.states(name)
    cuts = sorted({1, min(3, len(pts)), len(pts)})
    with compiled(m) as cm:
        with batch(cm, qpos[:jm.NENV], qvel[:jm.NENV]) as b7:
            b7.forward()
            b7.set_jac_points(pts, outputs=ALL, pnt=pnt)
            base = b7.jacobians()
            with batch(cm, qpos, qvel) as b70, batch(cm, qpos[:1], qvel[:1]) as b1:
                b70.forward()
                b1.forward()
                for b, envs in ((b70, jm.NENV), (b7, jm.NENV), (b1, 1)):
                    for npt in cuts:
                        for outs in [ALL] + [(o,) for o in ALL] + [("J", "Ainv"), ("MinvJT", "vel")]:
                            b.set_jac_points(pts[:npt], outputs=outs, pnt=pnt[:npt])
                            got = b.jacobians(0, envs)
                            assert sorted(got) == sorted(outs)
                            for key in outs:
                                assert same_bits(got[key], base[key][:envs, :npt]), (name, b.nenv, npt, outs, key)
                if name == "two_roots":
                    rep = 6
                    b70.set_jac_points(list(pts) * rep, outputs=ALL, pnt=np.tile(pnt, (rep, 1)))
                    got = b70.jacobians(0, jm.NENV)
                    for key in ALL:
                        for r in range(rep):
                            assert same_bits(got[key][:, r * len(pts):(r + 1) * len(pts)], base[key]), (name, "48 points", key, r)


# ------------------------------------------------------------------------------------------------------------------ 5. per-env parameters
def test_per_env_masses_inertias_and_armature():
    """Measured on an MI355X (7 envs, each against the reference on its own copy of the model): J 3.7e-16, MinvJT 5.7e-15 (own 3.9e-15), Ainv 5.8e-15
    (own 2.8e-15), vel 4.6e-16, bounds 1.0e-11; J against the UNCHANGED model's reference 3.7e-16.
    With every env in env 0's state, two envs differ by 1.4 .. 26 in Ainv and 0.76 .. 6.1 in MinvJT (the tests' measure), and by at most 5.4e-17 in J."""
    name = "two_roots"
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:jm.NENV] for a in jm.states(name))
    n, nv, nb = jm.NENV, int(m["nv"]), int(m["nbody"])
    rng = np.random.default_rng(9)
    mass = np.asarray(m["body_mass"], float) * rng.uniform(0.5, 2.0, (n, nb))
    inertia = np.asarray(m["body_inertia"], float) * rng.uniform(0.5, 2.0, (n, nb, 1))
    arm = rng.uniform(0.0, 0.05, (n, nv))
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.set_env_body_mass(mass, inertia)
        b.set_env_dof_params(armature=arm)
        b.forward()
        b.set_jac_points(pts, outputs=ALL, pnt=pnt)
        out = b.jacobians()
        # every env in env 0's state: what still differs between two envs is their parameters' doing
        b.set("qpos", np.tile(qpos[0], (n, 1)))
        b.set("qvel", np.tile(qvel[0], (n, 1)))
        b.forward()
        shared = b.jacobians()
    pairs = [(e, f) for e in range(n) for f in range(e + 1, n)]
    da = sorted(jm.rel_err(shared["Ainv"][e], shared["Ainv"][f]) for e, f in pairs)
    dm = sorted(jm.rel_err(shared["MinvJT"][e], shared["MinvJT"][f]) for e, f in pairs)
    dj = max(jm.rel_err(shared["J"][e], shared["J"][f]) for e, f in pairs)
    print(f"envs in one state: Ainv differs between two envs by {da[0]:.1e} .. {da[-1]:.1e}, MinvJT by {dm[0]:.1e} .. {dm[-1]:.1e}, J by at most {dj:.1e}")
    assert da[-1] > 1e-3 and dm[-1] > 1e-3, "at least two envs differ from each other by more than 1e-3"
    assert dj <= jm.EXACT_TOL, "... in what goes through M^-1 only"
    refs = [jm.ref_outputs(mjcf.with_joint_params(mjcf.with_body_mass(m, mass[e], inertia[e]), armature=arm[e]), qpos[e], qvel[e], pts, pnt) for e in range(n)]
    check(out, refs, "two_roots with per-env masses, inertias and armature")
    plain = reference(m, qpos, qvel, pts, pnt, range(n))
    ej = max(jm.rel_err(out["J"][e], plain[e]["J"]) for e in range(n))
    print(f"J against the unchanged model's reference {ej:.1e}")
    assert ej <= jm.EXACT_TOL, "J does not depend on the masses"
    d = max(jm.rel_err(refs[e]["Ainv"], plain[e]["Ainv"]) for e in range(n))
    assert d > 1e-3, "Ainv follows the env's parameters"
    assert max(jm.rel_err(refs[e]["MinvJT"], plain[e]["MinvJT"]) for e in range(n)) > 1e-3


# ------------------------------------------------------------------------------------------------------------------ 6. the hand
def test_the_hand_with_its_fingertips():
    """shadow_hand_like, five fingertip sites, 3 sampled envs of 64.  Measured on an MI355X: J 3.3e-16, MinvJT 4.5e-14 (own 3.1e-15, bound 1.0e-11),
    Ainv 2.4e-13 (own 1.9e-13, bound 1.9e-11), vel 3.3e-16."""
    name, nenv, sample = "shadow_hand_like", 64, [0, 31, 63]
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:nenv] for a in jm.states(name))
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.forward()
        b.set_jac_points([p[1] for p in pts], outputs=ALL)   # (sites by name, no pnt)
        out = b.jacobians()
    check({k: a[sample] for k, a in out.items()}, reference(m, qpos, qvel, pts, pnt, sample), "shadow_hand_like, 5 fingertips, 3 of 64 envs")


def test_the_largest_model():
    """deep: one chain of nv = 64 dofs (nM = 2080), the most mjb_compile takes -- one env per block, the five points in tiles of three, a 64-deep solve.
    3 envs against the reference, and env 0 alone in a 1-env batch bit for bit.  Measured on an MI355X: J 8.4e-16, MinvJT 4.9e-12 (own 3.9e-12, bound 3.9e-10), Ainv 8.7e-13
    (own 5.9e-13, bound 5.9e-11), vel 1.4e-15."""
    name, nenv = "deep", 3
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:nenv] for a in jm.states(name))
    with compiled(m) as cm:
        with batch(cm, qpos, qvel) as b:
            b.forward()
            b.set_jac_points(pts, outputs=ALL, pnt=pnt)
            out = b.jacobians()
        check(out, reference(m, qpos, qvel, pts, pnt, range(nenv)), "deep (nv = 64), 5 points, 3 envs")
        with batch(cm, qpos[:1], qvel[:1]) as b1:
            b1.forward()
            b1.set_jac_points(pts[:2], outputs=("MinvJT", "Ainv"), pnt=pnt[:2])
            one = b1.jacobians()
            assert all(same_bits(one[k], out[k][:1, :2]) for k in one)


# ------------------------------------------------------------------------------------------------------------------ 7. the contract
def test_contract():
    from mujoco_ros_pkgs_amd import binding, engine
    lib = binding.load_library()
    live0 = lib.mjb_debug_live_resources()
    name = "two_roots"
    m = jm.model(name)
    pts, pnt = jm.points(name)
    qpos, qvel = (a[:jm.NENV] for a in jm.states(name))
    nv = int(m["nv"])
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def configure(b, ty, oid, p=None, outputs=1, npoint=None):
        ty, oid = np.asarray(ty, np.int32), np.asarray(oid, np.int32)
        p = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
        return lib.mjb_jac_configure(b.ptr, len(ty) if npoint is None else npoint, ty.ctypes.data_as(pi), oid.ctypes.data_as(pi), None if p is None else p.ctypes.data_as(pd), outputs)

    with compiled(m) as cm:
        with batch(cm, qpos, qvel) as b:
            with pytest.raises(engine.EngineError, match="before mjb_jac_configure"):
                b.eval_jacobians_async()
            assert lib.mjb_jac_count(b.ptr) == 0 and not lib.mjb_jac_device_ptr(b.ptr, 1)
            # every MJB_EINVAL of mjb_jac_configure
            for why, rc in (("npoint < 1", configure(b, [0], [0], npoint=0)), ("an unknown object type", configure(b, [4], [0])), ("a negative type", configure(b, [-1], [0])),
                            ("a site id out of range", configure(b, [0], [int(m["nsite"])])), ("a body id out of range", configure(b, [1], [int(m["nbody"])])),
                            ("a bodycom id out of range", configure(b, [2], [-1])), ("a geom id out of range", configure(b, [3], [int(m["ngeom"])])),
                            ("a non-finite pnt", configure(b, [0], [0], p=[[0.0, np.nan, 0.0]])), ("an infinite pnt", configure(b, [0, 0], [0, 1], p=[[0.0] * 3, [np.inf, 0, 0]])),
                            ("outputs 0", configure(b, [0], [0], outputs=0)), ("unknown output bits", configure(b, [0], [0], outputs=16 | 1))):
                assert rc == -1 and b"mjb_jac_configure" in lib.mjb_last_error(), why   # MJB_EINVAL
            assert lib.mjb_jac_count(b.ptr) == 0, "a refused configuration leaves none"
            with pytest.raises(ValueError):
                b.set_jac_points(["no such site"])
            with pytest.raises(ValueError):
                b.set_jac_points([("body", "no such body")])
            with pytest.raises(ValueError):
                b.set_jac_points([("joint", 0)])
            with pytest.raises(ValueError):
                b.set_jac_points([0], outputs=("J", "Lambda"))

            # eval needs current frames, as get() of a derived field does
            b.set_jac_points(pts, outputs=("J", "vel"), pnt=pnt)
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):
                b.jacobians()
            b.forward()
            first = b.jacobians()
            assert sorted(first) == ["J", "vel"]
            b.set("qpos", qpos[::-1].copy())
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):   # stale after set("qpos") without forward()
                b.jacobians()
            b.step()
            with pytest.raises(engine.EngineError, match="only after mjb_forward"):   # after step() without keep_frame
                b.jacobians()
            b.forward()
            assert not same_bits(b.jacobians()["J"], first["J"]), "the evaluation followed the frames"
            b.step1()
            between = b.jacobians()   # between step1 and step2
            b.step2()
            assert np.isfinite(between["J"]).all()

            # an output that was not configured
            buf = np.zeros(jm.NENV * len(pts) * 6 * nv)
            assert lib.mjb_jac_get(b.ptr, 2, 0, jm.NENV, buf.ctypes.data_as(pd)) == -1 and lib.mjb_jac_get(b.ptr, 4, 0, jm.NENV, buf.ctypes.data_as(pd)) == -1
            assert lib.mjb_jac_get(b.ptr, 3, 0, jm.NENV, buf.ctypes.data_as(pd)) == -1, "which is one bit"
            assert not lib.mjb_jac_device_ptr(b.ptr, 2) and not lib.mjb_jac_device_ptr(b.ptr, 4)
            with pytest.raises(engine.EngineError):
                b.jac_device_ptr("Ainv")
            assert lib.mjb_jac_get(b.ptr, 1, 0, jm.NENV + 1, buf.ctypes.data_as(pd)) != 0, "env range"

            # reconfiguration replaces the shapes; the device pointers serve the same numbers
            b.forward()
            b.set_jac_points(pts[:3], outputs=ALL, pnt=pnt[:3])
            out = b.jacobians()
            assert lib.mjb_jac_count(b.ptr) == 3 and out["J"].shape == (jm.NENV, 3, 6, nv) and out["Ainv"].shape == (jm.NENV, 3, 6, 6)
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for key in ALL:
                p = b.jac_device_ptr(key)
                assert p
                back = np.empty_like(out[key])
                assert hip.hipMemcpy(back.ctypes.data, p, back.nbytes, 2) == 0 and same_bits(back, out[key]), key
            part = b.jacobians(2, 5)
            assert all(same_bits(part[k], out[k][2:5]) for k in ALL)
            b.set_jac_points(["s_a2"], outputs="vel")   # one site by name, one output by name
            assert sorted(b.jacobians()) == ["vel"] and lib.mjb_jac_count(b.ptr) == 1
    with compiled(mjcf.compile_xml_string("<mujoco><worldbody><geom name='g' type='sphere' size='0.1'/><site name='s'/></worldbody></mujoco>")) as cm0:
        with batch(cm0, np.zeros((1, 0))) as b0:
            assert configure(b0, [0], [0]) == -1 and b"no dofs" in lib.mjb_last_error()
    assert lib.mjb_debug_live_resources() == live0
