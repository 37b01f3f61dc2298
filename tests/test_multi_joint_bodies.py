"""Bodies with several joints (CPU): the oracle against the independent numpy dynamics of mujoco_ros_pkgs_amd/refdyn.py on the models of
multi_joint_models.py -- kinematics, qM, qfrc_bias (refdyn.bias_newton_euler: every joint type, any number of joints per body), qacc_smooth
and one Euler step -- plus mj_setConst's C++ mirror, what the loader and mjb_compile refuse, and the random multi-joint generator's sanity.
The GPU side of the same models is test_gpu_multi_joint_bodies.py; the bounds BIAS_TOL / STEP_* fixed here are the ones it uses."""
import ctypes as C
import os

import numpy as np
import pytest

import multi_joint_models as MJ
from mujoco_ros_pkgs_amd import binding, engine, mjcf, refdyn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Finite-difference checks: the error is the central difference's (truncation ~ eps^2, roundoff ~ 1e-16 / eps), about ten apart between
# states.  Measured on these tests' own states, oracle against refdyn (worst over every model and state below):
#     qfrc_bias        6.2e-11  relative to 1 + max|c|   (MJ_CON; |c| up to 40)
#     qacc_smooth      1.9e-11  relative to 1 + max|a|   (MJ_FREE; cond(M) ~ 1e4, |a| up to 2e3)
#     qvel after step  2.1e-11  absolute,     qpos after step  2.2e-14  absolute
# The bounds are 100 x the measured worst; all are far below the 2e-6 of the Lagrangian check in test_oracle_smooth.py.
BIAS_TOL = 6.2e-9
QACC_TOL = 1.9e-9
STEP_QVEL_TOL = 2.1e-9
STEP_QPOS_TOL = 2.2e-12
NSTATE = 8


@pytest.fixture(scope="module")
def free_model():
    return mjcf.compile_xml_string(MJ.MJ_FREE)


@pytest.fixture(scope="module")
def con_model():
    return mjcf.compile_xml_string(MJ.mj_con_xml())


def test_models_are_what_the_tests_need(free_model, con_model):
    assert free_model["nv"] <= 16 and free_model["nbody"] <= 16 and free_model["nefcmax"] == 0
    assert MJ.joint_list_shapes(free_model) == {("slide", "slide", "hinge"), ("hinge", "hinge", "hinge"), ("ball", "slide"), ("slide", "ball")}
    assert MJ.joint_list_shapes(con_model) == MJ.joint_list_shapes(free_model) | {("free",), ("ball",)}
    assert np.all(np.linalg.norm(np.asarray(free_model["jnt_pos"]), axis=1) > 0)
    for m in (free_model, con_model):
        qpos, _ = MJ.states(m, NSTATE, 1)
        for e in range(NSTATE):
            assert np.linalg.cond(refdyn.mass_matrix(m, qpos[e])) <= 1e6


@pytest.mark.parametrize("which", ["free", "con"])
def test_oracle_kinematics_and_qM_match_refdyn(oracle_built, free_model, con_model, which):
    m = free_model if which == "free" else con_model
    d = oracle_built.OracleData(m)
    qpos, qvel = MJ.states(m, NSTATE, 1)
    for e in range(NSTATE):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.forward()
        kin = refdyn.kinematics(m, qpos[e])
        for f, shape in (("xpos", (-1, 3)), ("xmat", (-1, 3, 3)), ("xipos", (-1, 3)), ("ximat", (-1, 3, 3)), ("xanchor", (-1, 3)), ("xaxis", (-1, 3))):
            np.testing.assert_allclose(np.asarray(d.field(f)).reshape(shape), kin[f], rtol=0, atol=1e-14, err_msg=f)
        np.testing.assert_allclose(MJ.dense_M(m, d.qM), refdyn.mass_matrix(m, qpos[e]), rtol=0, atol=1e-13)


def _bias_models(free_model):
    pend = mjcf.compile_xml_file(os.path.join(GOLDEN, "pendulum_world.xml"), disable=("contact",))
    return {"MJ_FREE": free_model, "MJ_CON": mjcf.compile_xml_string(MJ.mj_con_xml(contact=False)), "split_step_tree": mjcf.load_asset("split_step_tree"),
            "pendulum_world": pend, "franka_like": mjcf.load_asset("franka_like")}


@pytest.mark.parametrize("name", ["MJ_FREE", "MJ_CON", "split_step_tree", "pendulum_world", "franka_like"])
def test_oracle_bias_matches_newton_euler_projection(oracle_built, free_model, name):
    """qfrc_bias (mj_rne) against refdyn.bias_newton_euler, 8 states per model.  Measured worst |oracle - refdyn| / (1 + max|c|) = 6.2e-11
    (MJ_CON; 4.0e-11 on MJ_FREE); bound BIAS_TOL = 6.2e-9 = 100 x that, below the Lagrangian check's 2e-6.  On franka_like the Lagrangian bias, a third
    derivation, agrees too."""
    m = _bias_models(free_model)[name]
    d = oracle_built.OracleData(m)
    qpos, qvel = MJ.states(m, NSTATE, 2)
    worst = 0.0
    for e in range(NSTATE):
        assert np.linalg.cond(refdyn.mass_matrix(m, qpos[e])) <= 1e6
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.forward()
        got = np.array(d.qfrc_bias)
        c = refdyn.bias_newton_euler(m, qpos[e], qvel[e])
        worst = max(worst, float(np.abs(got - c).max() / (1 + np.abs(c).max())))
        if name == "franka_like":
            cl = refdyn.bias_lagrange(m, qpos[e], qvel[e])
            np.testing.assert_allclose(c, cl, rtol=1e-6, atol=2e-6)
            np.testing.assert_allclose(got, cl, rtol=1e-6, atol=2e-6)
    print(f"{name}: worst bias error {worst:.3e}")
    assert worst <= BIAS_TOL, worst


def test_oracle_qacc_smooth_and_step_match_step_euler(oracle_built, free_model):
    """MJ_FREE under random ctrl: qacc_smooth and one step() against refdyn.step_euler (springs and actuators from the model's constants).
    Measured worst: qacc_smooth 1.9e-11 relative to 1 + max|a|, qvel 2.1e-11, qpos 2.2e-14; bounds (100 x) QACC_TOL = 1.9e-9,
    STEP_QVEL_TOL = 2.1e-9, STEP_QPOS_TOL = 2.2e-12."""
    m = free_model
    d = oracle_built.OracleData(m)
    qpos, qvel = MJ.states(m, NSTATE, 3)
    ctrl = np.random.default_rng(4).uniform(-2, 2, (NSTATE, m["nu"]))
    wa = wv = wq = 0.0
    for e in range(NSTATE):
        assert np.linalg.cond(refdyn.mass_matrix(m, qpos[e])) <= 1e6
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.ctrl[:] = ctrl[e]
        d.forward()
        qn, vn, a = refdyn.step_euler(m, qpos[e], qvel[e], MJ.applied_force(m, qpos[e], qvel[e], ctrl[e]))
        wa = max(wa, float(np.abs(np.array(d.qacc_smooth) - a).max() / (1 + np.abs(a).max())))
        d.step()
        wv = max(wv, float(np.abs(np.array(d.qvel) - vn).max()))
        wq = max(wq, float(np.abs(np.array(d.qpos) - qn).max()))
    print(f"worst qacc_smooth {wa:.3e} qvel {wv:.3e} qpos {wq:.3e}")
    assert wa <= QACC_TOL and wv <= STEP_QVEL_TOL and wq <= STEP_QPOS_TOL, (wa, wv, wq)


def test_bias_newton_euler_refuses_a_rotation_after_a_ball():
    m = mjcf.compile_xml_string(MJ.BALL_THEN_HINGE)
    with pytest.raises(ValueError, match="last rotational joint"):
        refdyn.bias_newton_euler(m, m["qpos0"], np.zeros(m["nv"]))
    with pytest.raises(ValueError):
        refdyn.bias_lagrange(m, m["qpos0"], np.zeros(m["nv"]))


@pytest.mark.parametrize("which", ["free", "con"])
def test_setconst_mirror_on_multi_joint_bodies(free_model, con_model, which):
    """CompiledModel.derive_mass_params (the C++ mj_setConst mirror: per-body joint loop, point Jacobians) against mjcf.mass_params."""
    m = free_model if which == "free" else con_model
    cm = engine.CompiledModel(m)
    got, want = cm.derive_mass_params(m["body_mass"]), mjcf.mass_params(m)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12), np.abs(got - want).max()
    rng = np.random.default_rng(3)
    mass = np.asarray(m["body_mass"]) * rng.uniform(0.5, 2.0, m["nbody"])
    inert = np.asarray(m["body_inertia"]).reshape(-1, 3) * rng.uniform(0.5, 2.0, (m["nbody"], 1))
    got, want = cm.derive_mass_params(mass, inert), mjcf.mass_params(mjcf.with_body_mass(m, mass, inert))
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12), np.abs(got - want).max()


FREE_SHARED = """<mujoco><worldbody><body pos="0 0 1"><freejoint/><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>"""
FREE_BELOW = """<mujoco><worldbody><body pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.1"/>
<body pos="0.2 0 0"><freejoint/><geom type="sphere" size="0.1"/></body></body></worldbody></mujoco>"""


def _compile_rc(model):
    lib = binding.load_library()
    desc, keep = binding.make_desc(model)
    ptr = lib.mjb_compile(C.byref(desc))
    err = lib.mjb_last_error().decode()
    if ptr:
        lib.mjb_free_model(ptr)
    return bool(ptr), err


def test_free_joint_refusals():
    """A free joint is the only joint of a top-level body: the kinematics of every kernel takes `jntnum == 1 && FREE` as the only free-joint
    case.  The loader refuses anything else, and so does mjb_compile on a descriptor edited by hand."""
    for xml in (FREE_SHARED, FREE_BELOW):
        with pytest.raises(mjcf.MjcfError, match="free joint must be the only joint of a top-level body"):
            mjcf.compile_xml_string(xml)
    # a free body and a hinged body, both top level
    m = mjcf.compile_xml_string("""<mujoco><worldbody><body name="f" pos="0 0 1"><freejoint/><geom type="sphere" size="0.1"/></body>
        <body name="h" pos="1 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>""")
    assert _compile_rc(m)[0]
    shared = mjcf.Model(dict(m))        # the free body claims the hinge as its second joint
    shared["body_jntnum"] = np.array([0, 2, 0], np.int32)
    shared["body_jntadr"] = np.array([-1, 0, -1], np.int32)
    ok, err = _compile_rc(shared)
    assert not ok and "free joint" in err and "only joint of a top-level body" in err, err
    below = mjcf.Model(dict(m))         # the free body hangs below the hinged one
    below["body_parentid"] = np.array([0, 2, 0], np.int32)
    ok, err = _compile_rc(below)
    assert not ok and "free joint" in err and "only joint of a top-level body" in err, err


MULTI_SEEDS = list(range(int(os.environ.get("MJB_RANDOM_MULTIJOINT", "16"))))


def test_random_multijoint_models_load_and_step_on_the_oracle(oracle_built):
    """Every generated model compiles, M is well conditioned on the states the GPU test draws, the oracle takes 20 finite steps, and every
    joint-list shape of the generator occurred."""
    shapes = set()
    for seed in MULTI_SEEDS:
        m = mjcf.compile_xml_string(MJ.random_multijoint_model(seed))
        assert int(m["solver"]) == [2, 0, 1][seed % 3]
        shapes |= MJ.joint_list_shapes(m)
        qpos, qvel = MJ.harness_states(m, seed)
        for e in range(qpos.shape[0]):
            assert np.linalg.cond(refdyn.mass_matrix(m, qpos[e])) <= 1e8, seed
        for j in range(m["njnt"]):      # axes of one body pairwise at least 30 degrees apart
            for k in range(j):
                if m["jnt_bodyid"][j] == m["jnt_bodyid"][k] and min(m["jnt_type"][j], m["jnt_type"][k]) >= 2:
                    assert abs(np.dot(m["jnt_axis"][j], m["jnt_axis"][k])) <= np.cos(np.pi / 6) + 1e-3, seed
        d = oracle_built.OracleData(m)
        d.reset()
        rng = np.random.default_rng(1000 + seed)
        d.qvel[:] = rng.uniform(-0.5, 0.5, m["nv"])
        d.ctrl[:] = rng.uniform(-1, 1, m["nu"])
        d.step(20)
        assert np.isfinite(np.array(d.qpos)).all() and np.isfinite(np.array(d.qvel)).all(), seed
    assert shapes == set(MJ.JOINT_LISTS), set(MJ.JOINT_LISTS) - shapes


def test_mj_con_states_reach_every_row_type(oracle_built):
    """The states the GPU harness draws for MJ_CON (seed 0): at least 3 of 16 in contact, and equality, dof friction, joint limit (slide, hinge
    and ball) and tendon limit rows each active in at least one."""
    m = mjcf.compile_xml_string(MJ.mj_con_xml())
    qpos, qvel = MJ.harness_states(m, 0)
    d = oracle_built.OracleData(m)
    in_contact, types, limited = 0, set(), set()
    for e in range(16):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.forward()
        n = int(d.nefc[0])
        t, i = np.array(d.efc_type)[:n], np.array(d.efc_id)[:n]
        in_contact += int(d.ncon[0]) > 0
        types |= set(int(x) for x in t)
        limited |= set(int(x) for x in i[t == 3])
    assert in_contact >= 3, in_contact
    assert {0, 1, 3, 4} <= types and types & {5, 6, 7}, types      # equality, dof friction, joint limit, tendon limit, contact
    names = m["names"]["joint"]
    assert limited == {names.index("sy"), names.index("g3"), names.index("b")}, limited
