"""Actuators on sites (mjTRN_SITE, include/mjb.h): what the loader and mjb_compile take and refuse, that the lane = env and split-step
kernels leave such models to the generic kernels, and that models without site actuators keep their frames.  Host side only: mjb_compile
needs no GPU.  The scenes are shared with tests/test_gpu_site_transmission.py."""
import ctypes as C
import os

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import binding, engine, mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a free body with four rotors at (+-a, +-a, 0): thrust along the body's z axis and a reaction torque of +-c per unit thrust
QUAD_MASS, QUAD_I, QUAD_A, QUAD_C = 1.2, (0.011, 0.013, 0.021), 0.17, 0.02
QUAD = """
<mujoco model="quad">
  <option timestep="0.002" integrator="{integrator}" solver="{solver}" cone="{cone}" iterations="400" tolerance="1e-14"/>
  <size nconmax="{ncon}" njmax="{njmax}"/>
  <worldbody>
    {floor}
    <body name="quad" pos="0 0 {z}">
      <freejoint/>
      <inertial pos="0 0 0" mass="1.2" diaginertia="0.011 0.013 0.021"/>
      <geom type="box" size="0.12 0.12 0.02" mass="0" contype="{con}" conaffinity="{con}"/>
      <site name="r0" pos="0.17 0.17 0"/>
      <site name="r1" pos="-0.17 0.17 0"/>
      <site name="r2" pos="-0.17 -0.17 0"/>
      <site name="r3" pos="0.17 -0.17 0"/>
    </body>
  </worldbody>
  <actuator>
    <motor site="r0" gear="0 0 1 0 0 0.02"/>
    <motor site="r1" gear="0 0 1 0 0 -0.02"/>
    <motor site="r2" gear="0 0 1 0 0 0.02"/>
    <motor site="r3" gear="0 0 1 0 0 -0.02"/>
  </actuator>
</mujoco>
"""
QUAD_SIGN = np.array([1.0, -1.0, 1.0, -1.0])
QUAD_POS = np.array([[0.17, 0.17], [-0.17, 0.17], [-0.17, -0.17], [0.17, -0.17]])


def quad_model(integrator="Euler", solver="Newton", cone="pyramidal", floor=False, z=1.0):
    f = '<geom name="floor" type="plane" size="3 3 0.1"/>' if floor else ""
    return mjcf.compile_xml_string(QUAD.format(integrator=integrator, solver=solver, cone=cone, ncon=8 if floor else 0, njmax=40 if floor else 0,
                                               floor=f, z=z, con=1 if floor else 0))


# an arm of three hinges and a slide; sites on the hand, the forearm, the base and the world.  {acts} are the actuators; joint limits give
# constraint rows, and with floor="1" the hand's sphere meets a floor
ARM = """
<mujoco model="site_arm">
  <compiler angle="radian"/>
  <option timestep="0.002" integrator="{integrator}" solver="{solver}" cone="{cone}" iterations="80" tolerance="1e-12"/>
  <size nconmax="{ncon}" njmax="{njmax}"/>
  <default><joint damping="{damping}" armature="0.01"/></default>
  <worldbody>
    {floor}
    <site name="world_ref" pos="0.1 -0.2 0.3" quat="0.9 0.1 0.3 -0.2"/>
    <body name="base" pos="0 0 0.6">
      <joint name="j0" type="hinge" axis="0 0 1" limited="true" range="-2.5 2.5"/>
      <geom type="capsule" fromto="0 0 0 0 0 0.2" size="0.04" mass="1.0"/>
      <body name="upper" pos="0 0 0.2">
        <joint name="j1" type="hinge" axis="0 1 0" limited="true" range="-1.5 1.5"/>
        <geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.035" mass="0.8"/>
        <body name="fore" pos="0.3 0 0">
          <joint name="j2" type="hinge" axis="0 1 0" limited="true" range="-2 2"/>
          <geom type="capsule" fromto="0 0 0 0.25 0 0" size="0.03" mass="0.5"/>
          <body name="hand" pos="0.25 0 0" quat="0.96 0.1 0.2 0.15">
            <joint name="j3" type="slide" axis="1 0 0" limited="true" range="-0.05 0.05"/>
            <geom type="sphere" size="0.05" mass="0.3"/>
            <site name="hand" pos="0.03 0.01 -0.02" quat="0.8 0.2 -0.3 0.48"/>
          </body>
          <site name="fore_ref" pos="0.1 0.02 0" quat="0.95 0 0.31 0"/>
        </body>
      </body>
      <site name="base_ref" pos="0 0 0.2"/>
    </body>
  </worldbody>
  <actuator>
    {acts}
  </actuator>
  {sensors}
</mujoco>
"""
ARM_6D = '<motor name="wrench" site="hand" gear="0.8 -0.4 1.2 0.05 -0.03 0.07" ctrllimited="true" ctrlrange="-3 3"/>'
ARM_VEL = '<velocity name="damp" site="hand" gear="0.3 1 -0.5 0 0 0" kv="4"/>'


def arm_model(acts=ARM_6D, integrator="Euler", solver="Newton", cone="pyramidal", floor=False, njmax=24, damping=0.1, sensors=""):
    f = '<geom name="floor" type="plane" size="3 3 0.1" pos="0 0 0.05"/>' if floor else ""
    return mjcf.compile_xml_string(ARM.format(acts=acts, integrator=integrator, solver=solver, cone=cone, ncon=8 if floor else 0, njmax=njmax,
                                              floor=f, damping=damping, sensors=sensors))


def _compile_rc(model):
    """(model pointer or None, last error) of mjb_compile on the model's descriptor."""
    lib = binding.load_library()
    desc, keep = binding.make_desc(model)
    ptr = lib.mjb_compile(C.byref(desc))
    err = lib.mjb_last_error().decode()
    if ptr:
        lib.mjb_free_model(ptr)
    return bool(ptr), err


def test_loader_fields():
    m = arm_model(ARM_6D + ARM_VEL + '<position name="pos" site="hand" refsite="fore_ref" kp="2" gear="1 0 0 0 0 1"/>'
                  '<motor name="jm" jointinparent="j1"/><motor name="ws" site="hand" refsite="world_ref"/>')
    # sites sorted by body: world_ref (world), base_ref (base), fore_ref (fore), hand (hand) -- not the document order
    assert m["names"]["site"] == ["world_ref", "base_ref", "fore_ref", "hand"]
    assert list(m["actuator_trntype"]) == [4, 4, 4, 0, 4]
    assert m["actuator_trnid"].tolist() == [[3, -1], [3, -1], [3, 2], [1, -1], [3, 0]]
    np.testing.assert_array_equal(m["actuator_gear"][0], [0.8, -0.4, 1.2, 0.05, -0.03, 0.07])
    np.testing.assert_array_equal(m["actuator_gear"][2], [1, 0, 0, 0, 0, 1])
    np.testing.assert_array_equal(m["actuator_gear"][4], [1, 0, 0, 0, 0, 0])    # MuJoCo's default gear
    np.testing.assert_array_equal(m["actuator_biasprm"][1], [0, 0, -4])          # <velocity> on a site: kv as for a joint
    q = quad_model()
    assert list(q["actuator_trntype"]) == [4] * 4 and q["actuator_trnid"].tolist() == [[0, -1], [1, -1], [2, -1], [3, -1]]


@pytest.mark.parametrize("act,msg", [
    ('<motor site="hand" joint="j1"/>', "exactly one of"),
    ('<motor site="nope"/>', "unknown site 'nope'"),
    ('<motor site="hand" refsite="nope"/>', "unknown refsite 'nope'"),
    ('<motor site="hand" refsite="hand"/>', "refsite must be another site"),
    ('<motor joint="j1" refsite="hand"/>', "refsite= only goes with site="),
    ('<general site="hand" cranksite="fore_ref" slidersite="hand"/>', "slider-crank"),
    ('<general cranksite="fore_ref" slidersite="hand"/>', "slider-crank"),
    ('<general body="hand"/>', "body (adhesion)"),
])
def test_loader_refusals(act, msg):
    with pytest.raises(mjcf.MjcfError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        arm_model(act)


def test_implicitfast_refuses_velocity_terms_on_sites():
    with pytest.raises(mjcf.MjcfError, match="velocity-dependent actuator on a site"):
        arm_model(ARM_VEL, integrator="implicitfast")
    assert arm_model(ARM_6D, integrator="implicitfast")["integrator"] == 3   # a plain motor has no velocity term
    m = arm_model(ARM_6D, integrator="implicitfast")
    m["actuator_biastype"] = np.array([1], np.int32)
    m["actuator_biasprm"] = np.array([[0, 0, -2.0]])
    ok, err = _compile_rc(m)
    assert not ok and "velocity-dependent actuator on a site" in err


def test_compile_accepts_and_refuses_descriptors():
    m = arm_model(ARM_6D + '<position site="hand" refsite="fore_ref" kp="2"/>')
    assert _compile_rc(m)[0]
    for trnid, typ in (([9, -1], 4), ([-1, -1], 4), ([3, 3], 4), ([3, 7], 4), ([3, -2], 4), ([3, -1], 2), ([3, -1], 5)):
        bad = mjcf.Model(dict(m))
        t = np.array(m["actuator_trnid"])
        t[0] = trnid
        ty = np.array(m["actuator_trntype"])
        ty[0] = typ
        bad["actuator_trnid"], bad["actuator_trntype"] = t, ty
        ok, err = _compile_rc(bad)
        assert not ok and "site transmissions" in err, (trnid, typ, err)


def test_lane_env_and_split_step_refuse_site_actuators():
    """Both kernels test trntype != JOINT: a model that would qualify is -1 once one actuator sits on a site."""
    def classify(model):
        cm = engine.CompiledModel(model)
        v = int(cm.lib.mjb_model_lane_env(cm.ptr)), int(cm.lib.mjb_model_split_step(cm.ptr))
        cm.close()
        return v
    xml = open(os.path.join(mjcf.ASSET_DIR, "lane_env_tree.xml")).read()
    assert classify(mjcf.compile_xml_string(xml))[0] == 1
    assert classify(mjcf.compile_xml_string(xml.replace('<motor name="mB2" joint="jB2"/>', '<motor name="mB2" site="tipB" gear="0 0 0 0 0 1"/>'))) == (-1, -1)
    xml = open(os.path.join(mjcf.ASSET_DIR, "split_step_tree.xml")).read()
    assert classify(mjcf.compile_xml_string(xml))[1] == 1
    assert classify(mjcf.compile_xml_string(xml.replace('joint="joint1" ctrlrange', 'site="ee" ctrlrange'))) == (-1, -1)


# mjb_frame_bytes(m, 0 / 1 / 2) of the parent commit: a model without site actuators keeps every frame
FRAME_BYTES = {
    "franka_like": (12848, 9520, 9520), "franka_table": (49424, 20448, 20448), "shadow_hand_like": (139568, 37984, 53520),
    "shadow_hand_grasp": (139680, 38032, 53568), "lane_env_tree": (10400, 8336, 8336), "split_step_tree": (36512, 17104, 17104),
    "empty_world": (1072, 832, 832), "pendulum_world": (30176, 14576, 14576), "sensors_world": (30400, 14752, 14752),
    "mocap_world": (19312, 8976, 8976), "equality_world": (59792, 21648, 32672),
}


@pytest.mark.parametrize("name", sorted(FRAME_BYTES))
def test_frames_without_site_actuators_unchanged(name):
    path = os.path.join(ROOT, "tests", "golden", name + ".xml")
    model = mjcf.compile_xml_file(path) if os.path.exists(path) else mjcf.load_asset(name)
    cm = engine.CompiledModel(model)
    assert tuple(cm.lib.mjb_frame_bytes(cm.ptr, k) for k in range(3)) == FRAME_BYTES[name]
    cm.close()


def test_site_actuators_add_their_moment_rows():
    """The frames of a site-actuated model hold nsite_act x nv moment doubles more than its joint-actuated twin."""
    def fb(model):
        cm = engine.CompiledModel(model)
        v = [cm.lib.mjb_frame_bytes(cm.ptr, k) for k in range(2)]
        cm.close()
        return v
    two = ARM_6D + '<position site="hand" refsite="fore_ref" kp="2"/>'
    a, b = fb(arm_model(two)), fb(arm_model('<motor joint="j1"/><motor joint="j2"/>'))
    assert [x - y for x, y in zip(a, b)] == [2 * 4 * 8, 2 * 4 * 8], (a, b)
