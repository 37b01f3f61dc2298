"""Per-env joint and actuator parameters, the parts that need no GPU: mjcf.with_joint_params (the twin model the oracle runs for an env
that carries its own damping / armature / frictionloss / stiffness / gains) against the MJCF compiler on an edited XML, the device-free
C++ derivation of mj_setConst's constants with a caller's armature (mjb_derive_mass_params_armature) against the numpy one, the exported
entry points, and the frame layouts of the shipped models, which the feature must not move."""
import os
import re

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import binding, engine, mjcf

ASSETS = ["franka_like", "franka_table", "lane_env_tree", "shadow_hand_grasp", "shadow_hand_like", "split_step_tree"]

# a two-link arm with a fixed tendon over both joints, a spring, dry friction and a position / velocity servo pair
TENDON_XML = """
<mujoco model="tendon_arm"><compiler angle="radian"/><option timestep="0.002" gravity="0 0 -9.81"/>
<worldbody><body pos="0 0 1"><joint name="j1" type="hinge" axis="0 1 0" damping="{d1}" armature="{a1}" frictionloss="{f1}" stiffness="{s1}"/>
<geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.02" mass="1"/>
<body pos="0.3 0 0"><joint name="j2" type="hinge" axis="0 1 0" damping="{d2}" armature="{a2}" frictionloss="{f2}" stiffness="{s2}" springref="0.3"/>
<geom type="capsule" fromto="0 0 0 0.25 0 0" size="0.02" mass="0.7"/></body></body></worldbody>
<tendon><fixed name="t" limited="true" range="-1 1" frictionloss="0.05"><joint joint="j1" coef="1"/><joint joint="j2" coef="-0.5"/></fixed></tendon>
<actuator><position name="p1" joint="j1" kp="{kp}"/><velocity name="v2" joint="j2" kv="{kv}"/></actuator></mujoco>
"""
TENDON_BASE = dict(d1=0.4, d2=0.2, a1=0.01, a2=0.02, f1=0.03, f2=0.01, s1=2.0, s2=5.0, kp=30.0, kv=1.5)


def _same_model(a, b, what):
    assert set(a.keys()) == set(b.keys()), what
    for k in a:
        if isinstance(a[k], np.ndarray) or isinstance(b[k], np.ndarray):
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: field {k}"
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{what}: field {k}"  # (NaN marks "not stated" in a few tables)
        else:
            assert a[k] == b[k], f"{what}: field {k}"


def _own_values(m):
    return dict(damping=m["dof_damping"], armature=m["dof_armature"], frictionloss=m["dof_frictionloss"], stiffness=m["jnt_stiffness"],
                gainprm=m["actuator_gainprm"], biasprm=m["actuator_biasprm"])


@pytest.mark.parametrize("asset", ["franka_like", "franka_table", "shadow_hand_like"])
def test_own_values_return_the_compiled_model(asset):
    m = mjcf.load_asset(asset)
    _same_model(mjcf.with_joint_params(m, **_own_values(m)), m, asset)
    _same_model(mjcf.with_joint_params(m), m, asset)


def test_own_values_return_the_compiled_tendon_model():
    m = mjcf.compile_xml_string(TENDON_XML.format(**TENDON_BASE))
    assert m["ntendon"] == 1 and m["tendon_invweight0"][0] > 0
    _same_model(mjcf.with_joint_params(m, **_own_values(m)), m, "tendon_arm")


def test_edited_values_equal_the_edited_xml_tendon_model():
    base = mjcf.compile_xml_string(TENDON_XML.format(**TENDON_BASE))
    ed = dict(d1=0.9, d2=0.05, a1=0.04, a2=0.005, f1=0.01, f2=0.04, s1=0.5, s2=11.0, kp=75.0, kv=0.4)
    want = mjcf.compile_xml_string(TENDON_XML.format(**ed))
    gain, bias = np.array(base["actuator_gainprm"], dtype=np.float64), np.array(base["actuator_biasprm"], dtype=np.float64)
    gain[0, 0], bias[0, 1] = ed["kp"], -ed["kp"]    # <position>: gain kp, bias (0, -kp, 0)
    gain[1, 0], bias[1, 2] = ed["kv"], -ed["kv"]    # <velocity>: gain kv, bias (0, 0, -kv)
    got = mjcf.with_joint_params(base, damping=[ed["d1"], ed["d2"]], armature=[ed["a1"], ed["a2"]], frictionloss=[ed["f1"], ed["f2"]],
                                 stiffness=[ed["s1"], ed["s2"]], gainprm=gain, biasprm=bias)
    _same_model(got, want, "tendon_arm edited")
    assert not np.allclose(got["tendon_invweight0"], base["tendon_invweight0"]) and not np.allclose(got["dof_invweight0"], base["dof_invweight0"])


def test_edited_values_equal_the_edited_xml_franka_like():
    with open(os.path.join(mjcf.ASSET_DIR, "franka_like.xml")) as f:
        xml = f.read()
    base = mjcf.compile_xml_string(xml)
    # the class defaults (every arm joint) and the fingers' own attributes
    assert '<joint armature="0.1" damping="10.0"/>' in xml and xml.count('damping="10" armature="0.01" stiffness="1000"') == 2
    ed = xml.replace('<joint armature="0.1" damping="10.0"/>', '<joint armature="0.23" damping="4.5"/>')
    ed = ed.replace('damping="10" armature="0.01" stiffness="1000"', 'damping="17" armature="0.002" stiffness="650"')
    want = mjcf.compile_xml_string(ed)
    nv = int(base["nv"])
    damping, armature = np.full(nv, 4.5), np.full(nv, 0.23)
    damping[7:], armature[7:] = 17.0, 0.002
    stiffness = np.array(base["jnt_stiffness"], dtype=np.float64)
    stiffness[7:] = 650.0
    got = mjcf.with_joint_params(base, damping=damping, armature=armature, stiffness=stiffness)
    _same_model(got, want, "franka_like edited")
    assert not np.allclose(got["body_invweight0"], base["body_invweight0"]) and got["meaninertia"][0] != base["meaninertia"][0]


def test_bad_values_are_refused():
    m = mjcf.load_asset("franka_like")
    nv = int(m["nv"])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(mjcf.MjcfError, match="finite and non-negative"):
            mjcf.with_joint_params(m, damping=np.full(nv, bad))


# ---- the C++ derivation with a caller's armature (tolerance: tests/test_setconst_cpp.py's for masses) ----
def _tendon_model():
    return mjcf.compile_xml_string(TENDON_XML.format(**TENDON_BASE))


@pytest.mark.parametrize("name", ["franka_like", "franka_table", "shadow_hand_like", "tendon_arm"])
def test_cpp_derivation_with_armature_matches_numpy(name):
    m = _tendon_model() if name == "tendon_arm" else mjcf.load_asset(name)
    cm = engine.CompiledModel(m)
    # the model's own armature, handed over explicitly and as NULL, reproduces the model's constants
    for arm in (None, m["dof_armature"]):
        got = cm.derive_mass_params_armature(armature=arm)
        assert np.allclose(got, mjcf.mass_params(m), rtol=1e-9, atol=1e-12), np.abs(got - mjcf.mass_params(m)).max()
    rng = np.random.default_rng(5)
    arm = np.asarray(m["dof_armature"]) * rng.uniform(0.25, 4.0, m["nv"]) + rng.uniform(0, 1e-3, m["nv"])
    want = mjcf.mass_params(mjcf.with_joint_params(m, armature=arm))
    got = cm.derive_mass_params_armature(armature=arm)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12), np.abs(got - want).max()
    assert not np.allclose(got, mjcf.mass_params(m), rtol=1e-6, atol=0)
    # ... and together with new masses and inertias
    mass = np.asarray(m["body_mass"]) * rng.uniform(0.5, 2.0, m["nbody"])
    inert = np.asarray(m["body_inertia"]).reshape(-1, 3) * rng.uniform(0.5, 2.0, (m["nbody"], 1))
    want = mjcf.mass_params(mjcf.with_joint_params(mjcf.with_body_mass(m, mass, inert), armature=arm))
    got = cm.derive_mass_params_armature(mass, inert, arm)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12), np.abs(got - want).max()
    # the order of the two edits does not matter
    other = mjcf.mass_params(mjcf.with_body_mass(mjcf.with_joint_params(m, armature=arm), mass, inert))
    assert np.array_equal(other, want)


# ---- the public surface ----
NEW_SYMBOLS = ["mjb_set_env_dof_params", "mjb_set_env_joint_stiffness", "mjb_set_env_actuator_params", "mjb_set_env_joint_params",
               "mjb_env_joint_stride", "mjb_derive_mass_params_armature"]


def test_entry_points_declared_and_exported():
    lib = binding.load_library()
    declared = binding.header_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in lib._mjb_symbols and getattr(lib, s) is not None, s


def test_joint_stride():
    lib = binding.load_library()
    for name in ASSETS:
        m = mjcf.load_asset(name)
        cm = engine.CompiledModel(m)
        assert lib.mjb_env_joint_stride(cm.ptr) == 3 * m["nv"] + m["njnt"] + 6 * m["nu"] == mjcf.joint_params(m).size
        # the public mass block keeps its size
        assert lib.mjb_env_mass_stride(cm.ptr) == 7 * m["nbody"] + m["nv"] + m["ntendon"] + 1 == mjcf.mass_params(m).size


# ---- frame sizes and offsets of every shipped model: recorded on the commit before the feature ----
def _frame_record(m):
    lib = binding.load_library()
    cm = engine.CompiledModel(m)
    rec = {"bytes": [int(lib.mjb_frame_bytes(cm.ptr, k)) for k in (0, 1, 2)], "doubles": int(cm.frame_doubles)}
    for name, fid in binding.Field.ids.items():
        rec[name] = [int(lib.mjb_frame_offset(cm.ptr, fid, k)) for k in (0, 1)]
    return rec


def _golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_layouts_before_env_joint_params.json")


def test_frame_layouts_of_shipped_assets_unchanged():
    import json
    with open(_golden_path()) as f:
        want = json.load(f)
    shipped = sorted(re.sub(r"\.xml$", "", n) for n in os.listdir(mjcf.ASSET_DIR) if n.endswith(".xml"))
    assert shipped == sorted(want), "a shipped model has no recorded frame layout"
    for name in shipped:
        got = _frame_record(mjcf.load_asset(name))
        assert got == want[name], name
