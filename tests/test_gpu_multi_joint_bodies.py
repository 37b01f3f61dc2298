"""Bodies with several joints on the GPU: the step kernels' per-body joint loop past the first joint (the lane-cached and the uncached
load paths of the kinematics), com_vel's walk over the velocity groups of a body's earlier joints, and everything downstream of cdof_dot,
against the oracle AND against refdyn (numpy, independent of both: test_multi_joint_bodies.py pins the oracle to it and fixes the bounds)."""
import numpy as np
import pytest

import multi_joint_models as MJ
from mujoco_ros_pkgs_amd import mjcf, refdyn
from test_gpu_parity import FWD_FIELDS, _close
from test_gpu_random_models import _random_model_matches_oracle
from test_multi_joint_bodies import BIAS_TOL, MULTI_SEEDS, NSTATE, QACC_TOL, STEP_QPOS_TOL, STEP_QVEL_TOL

pytestmark = pytest.mark.gpu

NENV = 37   # ragged against every group size


@pytest.fixture(scope="module")
def free_setup(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.MJ_FREE)
    return m, engine.CompiledModel(m), engine, oracle_built


@pytest.fixture(scope="module")
def free_forward_reference(free_setup):
    """37 states of MJ_FREE and the oracle's forward fields on them, computed once"""
    m, cm, engine, po = free_setup
    qpos, qvel = MJ.states(m, NENV, 5)
    ctrl = np.random.default_rng(6).uniform(-2, 2, (NENV, m["nu"]))
    d = po.OracleData(m)
    ref = []
    for e in range(NENV):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.ctrl[:] = ctrl[e]
        d.forward()
        ref.append({f: np.array(d.field(f)) for f in FWD_FIELDS})
    return qpos, qvel, ctrl, ref


def _forward_matches_oracle(model, cm, engine, po, qpos, qvel, ctrl, fields, tol, what):
    n = qpos.shape[0]
    b = engine.Batch(cm, n)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if model["nu"]:
        b.set("ctrl", ctrl)
    b.forward()
    got = {f: b.get(f) for f in fields}
    b.close()
    d = po.OracleData(model)
    for e in range(n):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        if model["nu"]:
            d.ctrl[:] = ctrl[e]
        d.forward()
        for f in fields:
            _close(got[f][e], d.field(f), tol, f"{what}: {f} env {e}")


@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_forward_fields_match_oracle_on_every_group_size(free_setup, free_forward_reference, lanes):
    """16 lanes: the dense kernel with the lane cache (a body's first joint in registers, the later ones loaded); the others: uncached builds"""
    m, cm, engine, po = free_setup
    qpos, qvel, ctrl, ref = free_forward_reference
    b = engine.Batch(cm, NENV)
    b.set_launch(lanes, 0)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set("ctrl", ctrl)
    b.forward()
    got = {f: b.get(f) for f in FWD_FIELDS}
    b.close()
    for e in range(NENV):
        for f in FWD_FIELDS:
            _close(got[f][e], ref[e][f], 1e-11, f"{f} env {e} lanes {lanes}")


@pytest.mark.parametrize("lanes", [16, 64])
def test_forward_and_step_match_refdyn(free_setup, lanes):
    """The leg that shares no author with the kernels: qM, qfrc_bias, qacc_smooth and one step of MJ_FREE against refdyn.mass_matrix /
    bias_newton_euler / step_euler, on the states and at the bounds of test_multi_joint_bodies.py (100 x the oracle's measured distance
    from refdyn; the kernels sit within 1e-11 of the oracle)."""
    m, cm, engine, po = free_setup
    qpos, qvel = MJ.states(m, NSTATE, 3)
    ctrl = np.random.default_rng(4).uniform(-2, 2, (NSTATE, m["nu"]))
    b = engine.Batch(cm, NSTATE)
    b.set_launch(lanes, 0)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set("ctrl", ctrl)
    b.forward()
    qM, bias, qacc = b.get("qM"), b.get("qfrc_bias"), b.get("qacc_smooth")
    b.step(1)
    q1, v1 = b.get("qpos"), b.get("qvel")
    b.close()
    for e in range(NSTATE):
        np.testing.assert_allclose(MJ.dense_M(m, qM[e]), refdyn.mass_matrix(m, qpos[e]), rtol=0, atol=1e-13)
        c = refdyn.bias_newton_euler(m, qpos[e], qvel[e])
        qn, vn, a = refdyn.step_euler(m, qpos[e], qvel[e], MJ.applied_force(m, qpos[e], qvel[e], ctrl[e]))
        eb = np.abs(bias[e] - c).max() / (1 + np.abs(c).max())
        ea = np.abs(qacc[e] - a).max() / (1 + np.abs(a).max())
        ev, eq = np.abs(v1[e] - vn).max(), np.abs(q1[e] - qn).max()
        print(f"env {e}: bias {eb:.2e} qacc_smooth {ea:.2e} qvel {ev:.2e} qpos {eq:.2e}")
        assert eb <= BIAS_TOL and ea <= QACC_TOL and ev <= STEP_QVEL_TOL and eq <= STEP_QPOS_TOL, (e, eb, ea, ev, eq)


def test_rollout_matches_oracle_and_every_way_of_cutting_it(free_setup):
    """100 steps against the oracle at the 1e-8 of test_gpu_parity.test_step_matches_oracle; K fused steps == K single launches ==
    K (step1 + step2) pairs, bit for bit."""
    m, cm, engine, po = free_setup
    n = 32
    rng = np.random.default_rng(7)
    qpos = np.array([refdyn.integrate_pos(m, np.asarray(m["qpos0"], float), rng.normal(size=m["nv"]), 0.5) for _ in range(n)])
    qvel = rng.uniform(-0.5, 0.5, (n, m["nv"]))
    ctrl = rng.uniform(-1, 1, (n, m["nu"]))
    outs = []
    for mode in range(3):
        b = engine.Batch(cm, n)
        b.set("qpos", qpos)
        b.set("qvel", qvel)
        b.set("ctrl", ctrl)
        if mode == 0:
            b.step(7)
        elif mode == 1:
            for _ in range(7):
                b.step(1)
        else:
            for _ in range(7):
                b.step1()
                b.step2()
        outs.append((b.get("qpos"), b.get("qvel"), b.get("time"), b.get("sensordata")))
        if mode == 0:
            b.step(93)
            q100, v100, s100 = b.get("qpos"), b.get("qvel"), b.get("sensordata")
        b.close()
    for k in range(4):
        assert np.array_equal(outs[0][k], outs[1][k]) and np.array_equal(outs[0][k], outs[2][k]), k
    oq, ov, os_ = po.rollout(m, qpos, qvel, 100, ctrl=ctrl)
    _close(q100, oq, 1e-8, "qpos after 100 steps")
    _close(v100, ov, 1e-8, "qvel after 100 steps")
    _close(s100, os_, 1e-8, "sensordata after 100 steps")


# {hinge, hinge}, {slide, hinge}, {slide, ball} on every body, second joints limited.  wide: nbody 22 > 16 and nv 56 > 32 -- the serial pose walk, the
# flat subtree sums, the sparse factor; mid: nv 26 -- the level-scheduled factor; each with several dofs and two joints per body
TREES = {"wide-21": (21, 1), "mid-10": (10, 2)}


@pytest.mark.parametrize("case", sorted(TREES))
def test_two_joint_tree_matches_oracle(oracle_built, case):
    """field list and tolerances of test_gpu_tree_shapes.test_tree_shape_matches_oracle"""
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.two_joint_tree(*TREES[case]))
    if case == "wide-21":
        assert m["nv"] > 32 and m["nbody"] > 16 and int(np.min(np.asarray(m["body_jntnum"])[1:])) == 2
    else:
        assert 16 < m["nv"] <= 32
    cm = engine.CompiledModel(m)
    nenv = 6
    rng = np.random.default_rng(11)
    qpos = np.array([refdyn.integrate_pos(m, np.asarray(m["qpos0"], float), rng.uniform(-1, 1, m["nv"]), 0.7) for _ in range(nenv)])   # some beyond their limits
    qvel = rng.uniform(-0.5, 0.5, (nenv, m["nv"]))
    b = engine.Batch(cm, nenv)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.forward()
    d = oracle_built.OracleData(m)
    rows = 0
    for e in range(nenv):
        d.reset()
        d.qpos[:] = qpos[e]
        d.qvel[:] = qvel[e]
        d.forward()
        rows += int(d.nefc[0])
        for f in ("xpos", "subtree_com", "cinert", "crb", "qM", "qLD", "qLDiagInv", "cvel", "qfrc_bias", "qacc_smooth", "qacc"):
            ref = np.asarray(d.field(f))
            np.testing.assert_allclose(b.get(f)[e], ref, rtol=0, atol=1e-9 * (1 + np.abs(ref).max()), err_msg=f"{case}: {f}")
    assert rows > 0
    b.step(25)
    oq, ov, _ = oracle_built.rollout(m, qpos, qvel, 25)
    np.testing.assert_allclose(b.get("qpos"), oq, rtol=0, atol=1e-7, err_msg=case)
    np.testing.assert_allclose(b.get("qvel"), ov, rtol=0, atol=1e-5, err_msg=case)
    b.close()


CON_CASES = [("PGS", "pyramidal", "Euler"), ("PGS", "elliptic", "Euler"), ("Newton", "pyramidal", "Euler"), ("Newton", "elliptic", "Euler"),
             ("CG", "pyramidal", "Euler"), ("Newton", "pyramidal", "implicitfast"), ("Newton", "elliptic", "RK4")]


@pytest.mark.parametrize("solver,cone,integrator", CON_CASES)
def test_mj_con_matches_oracle_under_every_solver(oracle_built, solver, cone, integrator):
    """MJ_CON through the random-model harness: 1 and 15 steps, step1 / step2, chained halves, RK4 cuts, hwsim, sensor packing, ctrl noise and
    the per-env parameters.  (test_multi_joint_bodies.test_mj_con_states_reach_every_row_type: its states are in contact and at their limits.)"""
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.mj_con_xml(solver, cone, integrator))
    _random_model_matches_oracle(oracle_built, engine, m, engine.CompiledModel(m), 0)


@pytest.mark.parametrize("solver", ["Newton", "CG"])
def test_mj_con_matches_oracle_on_the_row_slot_kernels(oracle_built, solver):
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.mj_con_xml(solver, "pyramidal", extra_geoms=4))
    assert m["nefcmax"] > 256, m["nefcmax"]
    cm = engine.CompiledModel(m)
    assert cm.frame_info()[0]
    _random_model_matches_oracle(oracle_built, engine, m, cm, 0)


def test_ball_then_hinge_matches_oracle(oracle_built):
    """A ball FOLLOWED by a hinge on one body, GPU against the oracle only.  refdyn is not applied: MuJoCo writes the ball's cdof with the body's
    final xmat, so this pair's Jacobian is not the derivative of its kinematics along mj_integratePos and no independent derivation of "the"
    dynamics exists -- what is checked is that the kernels make the oracle's (MuJoCo's) choice."""
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.BALL_THEN_HINGE)
    cm = engine.CompiledModel(m)
    n = 24
    qpos, qvel = MJ.states(m, n, 9)
    qvel *= 0.5
    ctrl = np.random.default_rng(10).uniform(-1, 1, (n, m["nu"]))
    _forward_matches_oracle(m, cm, engine, oracle_built, qpos, qvel, ctrl, FWD_FIELDS, 1e-11, "ball then hinge")
    b = engine.Batch(cm, n)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set("ctrl", ctrl)
    b.step(25)
    oq, ov, os_ = oracle_built.rollout(m, qpos, qvel, 25, ctrl=ctrl)
    _close(b.get("qpos"), oq, 1e-8, "ball then hinge: qpos after 25 steps")
    _close(b.get("qvel"), ov, 1e-8, "ball then hinge: qvel after 25 steps")
    _close(b.get("sensordata"), os_, 1e-8, "ball then hinge: sensordata after 25 steps")
    b.close()


@pytest.mark.parametrize("which", ["hinge-slide-tree", "MJ_CON"])
def test_lane_env_and_split_step_kernels_refuse_multi_joint_bodies(oracle_built, which):
    """Plain PGS, 64 envs: asked for, neither the lane = env nor the split-step kernel runs (their sweeps assume one joint per body); the generic
    kernels do, and the result is the oracle's."""
    from mujoco_ros_pkgs_amd import engine
    n = 64
    for ask in ("lane_env", "split_step"):
        if which == "MJ_CON":
            xml = MJ.mj_con_xml("PGS", "pyramidal")
        else:       # (the lane = env kernel takes no constraint rows: asked on the tree without limits, so that the joint count is ITS reason to refuse)
            xml = MJ.hinge_slide_two_joint_tree("PGS", limited=ask == "split_step")
        m = mjcf.compile_xml_string(xml)
        assert int(m["solver"]) == 0 and int(np.max(m["body_jntnum"])) > 1
        cm = engine.CompiledModel(m)
        qpos, qvel = MJ.harness_states(m, 3, n)
        oq, ov, _ = oracle_built.rollout(m, qpos, qvel, 5)
        b = engine.Batch(cm, n)
        if ask == "lane_env":
            b.set_lane_env(1)
        else:
            b.set_split_step(1)
        b.set("qpos", qpos)
        b.set("qvel", qvel)
        b.step(5)
        if ask == "lane_env":
            assert b.lane_env_info() == (-1, False)
        else:
            assert b.split_step_info()[1] is False
        _close(b.get("qpos"), oq, 1e-8, f"{which} {ask}: qpos")       # (the harness's bounds for 5 steps: its per-env parameter leg)
        _close(b.get("qvel"), ov, 1e-6, f"{which} {ask}: qvel")
        b.close()


@pytest.mark.parametrize("seed", MULTI_SEEDS)
def test_gpu_random_multijoint_model_matches_oracle(oracle_built, seed):
    from mujoco_ros_pkgs_amd import engine
    m = mjcf.compile_xml_string(MJ.random_multijoint_model(seed))
    _random_model_matches_oracle(oracle_built, engine, m, engine.CompiledModel(m), seed)
