"""Body gravity compensation (mjModel.body_gravcomp, MuJoCo >= 2.3.1): loader, model description, what mjb_compile derives, and the
expected values the GPU tests use -- refdyn.gravcomp_force against a finite difference of its potential and, through the oracle's
qfrc_bias of a re-massed twin, against an independent route.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gravcomp_models as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mujoco_ros_pkgs_amd import binding
    return binding.load_library()


@pytest.fixture(scope="module")
def mjcf():
    from mujoco_ros_pkgs_amd import mjcf
    return mjcf


def _compile(lib, model):
    from mujoco_ros_pkgs_amd import binding
    desc, keep = binding.make_desc(model)
    return lib.mjb_compile(C.byref(desc))


def test_loader_values_and_default(mjcf):
    T = gm.model_T()
    assert np.array_equal(T["body_gravcomp"], gm.T_GC) and T["body_gravcomp"].dtype == np.float64
    assert T["names"]["body"][4] == "w4" and T["body_jntnum"][4] == 0 and T["body_gravcomp"][4] == 1.5   # the welded body, non-zero
    assert np.array_equal(gm.model_X()["body_gravcomp"], gm.X_GC)
    for name in ("franka_like", "lane_env_tree", "franka_table"):   # no attribute anywhere: zeros, one per body
        m = mjcf.load_asset(name)
        assert m["body_gravcomp"].shape == (m["nbody"],) and not m["body_gravcomp"].any()
    with pytest.raises(mjcf.MjcfError):
        mjcf.compile_xml_string('<mujoco><worldbody><body gravcomp="nan"><geom size="0.1"/><joint/></body></worldbody></mujoco>')


def test_with_gravcomp(mjcf):
    T = gm.model_T()
    vals = np.arange(8) * 0.25 - 0.5
    m = mjcf.with_gravcomp(T, vals)
    assert np.array_equal(m["body_gravcomp"], vals) and np.array_equal(T["body_gravcomp"], gm.T_GC)   # a copy
    for k in T:
        if k != "body_gravcomp" and isinstance(T[k], np.ndarray):
            assert np.array_equal(m[k], T[k]), k
    with pytest.raises(mjcf.MjcfError):
        mjcf.with_gravcomp(T, np.full(8, np.inf))
    with pytest.raises(ValueError):
        mjcf.with_gravcomp(T, np.zeros(7))


def test_make_desc_without_the_key(lib, mjcf):
    from mujoco_ros_pkgs_amd import binding
    old = dict(mjcf.load_asset("franka_like"))
    del old["body_gravcomp"]   # a model dict built by hand before the field existed
    desc, keep = binding.make_desc(old)
    assert [desc.body_gravcomp[b] for b in range(old["nbody"])] == [0.0] * old["nbody"]
    p = lib.mjb_compile(C.byref(desc))
    assert p and lib.mjb_model_lane_env(p) == 0
    lib.mjb_free_model(p)


def test_compile_refuses_non_finite(lib, mjcf):
    T = gm.model_T()
    for bad in (np.nan, np.inf, -np.inf):
        m = mjcf.Model(dict(T))
        g = gm.T_GC.copy()
        g[3] = bad
        m["body_gravcomp"] = g
        assert not _compile(lib, m)
        assert b"body_gravcomp[3]" in lib.mjb_last_error()
    for ok in (5.0, -3.0):   # any finite value, above 1 and below 0
        p = _compile(lib, mjcf.with_gravcomp(T, np.full(8, ok)))
        assert p
        lib.mjb_free_model(p)


def test_kernel_choice(lib, mjcf):
    T = gm.model_T()
    p = _compile(lib, T)
    assert lib.mjb_model_lane_env(p) == -2 and lib.mjb_model_split_step(p) == -1
    lib.mjb_free_model(p)
    p = _compile(lib, gm.without_gravcomp(T))   # gravcomp all zero: what the model had (T is nobody's compiled-in topology)
    assert lib.mjb_model_lane_env(p) == -2
    lib.mjb_free_model(p)
    fr = mjcf.load_asset("franka_like")
    p = _compile(lib, fr)
    assert lib.mjb_model_lane_env(p) == 0
    lib.mjb_free_model(p)
    p = _compile(lib, mjcf.with_gravcomp(fr, np.r_[0.0, np.ones(fr["nbody"] - 1)]))   # no compiled-in topology has gravcomp: hiprtc's
    assert lib.mjb_model_lane_env(p) == -2
    lib.mjb_free_model(p)
    # the generic kernels only: X (free / ball joints), C (contacts); and the split step stands down for a model it otherwise takes
    for m in (gm.model_X(), gm.model_C(0.5)):
        p = _compile(lib, m)
        assert lib.mjb_model_lane_env(p) == -1 and lib.mjb_model_split_step(p) == -1
        lib.mjb_free_model(p)
    ft = mjcf.load_asset("franka_table")
    p = _compile(lib, ft)
    assert lib.mjb_model_split_step(p) >= 0
    lib.mjb_free_model(p)
    p = _compile(lib, mjcf.with_gravcomp(ft, np.r_[0.0, np.ones(ft["nbody"] - 1)]))
    assert lib.mjb_model_split_step(p) == -1
    lib.mjb_free_model(p)


def test_plan_answers_form_0(lib):
    p = _compile(lib, gm.model_T())
    out = [C.c_int(-7) for _ in range(3)]
    for build in range(5):
        for form in (-1, 0, 1, 2, 3):
            for nenv in (70, 4096, 65536):
                assert lib.mjb_lane_env_plan(p, 256, nenv, build, form, 0, 0, *[C.byref(o) for o in out]) == 0
                assert (out[0].value, out[1].value) == (0, 0), (build, form, nenv)
                got = tuple(o.value for o in out)   # ... and the plan of "form 0 asked for" in full: the same LDS budget
                assert lib.mjb_lane_env_plan(p, 256, nenv, build, 0, 0, 0, *[C.byref(o) for o in out]) == 0
                assert got == tuple(o.value for o in out), (build, form, nenv, got)
    assert lib.mjb_lane_env_plan(p, 256, 65536, 0, 3, 0, 0, *[C.byref(o) for o in out]) == 0
    assert tuple(o.value for o in out) == (0, 0, 40)   # four wavefronts per CU, not the two of a forced multi-wavefront form
    lib.mjb_free_model(p)
    p = _compile(lib, gm.without_gravcomp(gm.model_T()))   # the same tree without gravcomp keeps the other forms
    assert lib.mjb_lane_env_plan(p, 256, 70, 0, 3, 0, 0, *[C.byref(o) for o in out]) == 0 and out[0].value == 3
    lib.mjb_free_model(p)


def test_generator_agrees_with_the_library(lib, mjcf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_lane_env_topo as gen
    fr = mjcf.load_asset("franka_like")
    for m in (gm.model_T(), gm.without_gravcomp(gm.model_T()), gm.model_X(), gm.model_C(1.0), fr, mjcf.with_gravcomp(fr, np.ones(fr["nbody"]))):
        p = _compile(lib, m)
        assert (gen.eligible(m) is None) == (lib.mjb_model_lane_env(p) != -1)
        lib.mjb_free_model(p)
    with pytest.raises(SystemExit):   # a compiled-in topology has no gravcomp
        gen.emit("T", gm.model_T())
    assert "body_gc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }" in gen.emit("T0", gm.without_gravcomp(gm.model_T()))
    old = dict(gm.without_gravcomp(gm.model_T()))
    del old["body_gravcomp"]   # a model dict from before the field
    assert "body_gc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }" in gen.emit("T1", old)


def test_tape_slot_29(lib):
    from mujoco_ros_pkgs_amd import engine
    T = gm.model_T()
    a = engine.CompiledModel(T).lane_env_tape()
    b = engine.CompiledModel(gm.without_gravcomp(T)).lane_env_tape()
    nb = T["nbody"]
    ra, rb = a[8:8 + 32 * nb].reshape(nb, 32), b[8:8 + 32 * nb].reshape(nb, 32)   # LeTapeHdr is 8 doubles, LeTapeBody 32
    assert np.array_equal(ra[:, 29], gm.T_GC) and not rb[:, 29].any()
    keep = np.arange(32) != 29
    assert np.array_equal(ra[:, keep], rb[:, keep])
    assert np.array_equal(a[:8], b[:8]) and np.array_equal(a[8 + 32 * nb:], b[8 + 32 * nb:]) and a.size == b.size


# mjb_frame_bytes(model, full) / (model, fused) of the shipped models on the commit before the field: no frame storage was added
PARENT_FRAME_BYTES = {
    "franka_like": (12848, 9520),
    "lane_env_tree": (10400, 8336),
    "franka_table": (49424, 20448),
    "split_step_tree": (36512, 17104),
    "shadow_hand_like": (139568, 37984),
    "shadow_hand_grasp": (139680, 38032),
}


@pytest.mark.parametrize("name", sorted(PARENT_FRAME_BYTES))
def test_frame_bytes_unchanged(lib, mjcf, name):
    m = mjcf.load_asset(name)
    p = _compile(lib, m)
    got = (lib.mjb_frame_bytes(p, 0), lib.mjb_frame_bytes(p, 1))
    lib.mjb_free_model(p)
    assert got == PARENT_FRAME_BYTES[name]
    # ... and gravcomp on every body costs none either
    p = _compile(lib, mjcf.with_gravcomp(m, np.r_[0.0, np.ones(m["nbody"] - 1)]))
    assert (lib.mjb_frame_bytes(p, 0), lib.mjb_frame_bytes(p, 1)) == got
    lib.mjb_free_model(p)


def _potential(m, q):
    """sum_b gc_b m_b g . xipos_b: gravcomp_force is minus its gradient."""
    from mujoco_ros_pkgs_amd import refdyn
    kin = refdyn.kinematics(m, q)
    g = np.asarray(m["gravity"], dtype=np.float64)
    return sum(m["body_gravcomp"][b] * m["body_mass"][b] * (g @ kin["xipos"][b]) for b in range(1, m["nbody"]))


@pytest.mark.parametrize("name", ["T", "X"])
def test_force_is_minus_the_gradient(name):
    from mujoco_ros_pkgs_amd import refdyn
    m = gm.model_T() if name == "T" else gm.model_X()
    qpos, qvel, _ = gm.states(m, 4, 3, name)
    eps = 1e-6
    zero = np.zeros(m["nv"])
    for q in qpos:
        f = refdyn.gravcomp_force(m, q)
        fd = np.zeros(m["nv"])
        for k in range(m["nv"]):   # (along the dof: integrate_pos moves a quaternion on its manifold)
            e = zero.copy()
            e[k] = 1.0
            fd[k] = -(_potential(m, refdyn.integrate_pos(m, q, e, eps)) - _potential(m, refdyn.integrate_pos(m, q, e, -eps))) / (2 * eps)
        assert np.abs(f).max() > 0.1
        assert np.abs(f - fd).max() <= 1e-6, np.abs(f - fd).max()


@pytest.mark.parametrize("name", ["T", "X"])
def test_twin_with_scaled_masses(oracle_built, mjcf, name):
    """Gravity acts on body b as m_b g at xipos_b, so the compensating force is what the gravity term of qfrc_bias loses when the masses go from
    m to m (1 + gc): at qvel = 0 (no Coriolis terms) bias(twin) - bias(model) == gravcomp_force.  The oracle's RNE and refdyn's Jacobians share
    nothing."""
    from mujoco_ros_pkgs_amd import refdyn
    m = gm.model_T() if name == "T" else gm.model_X()
    twin = mjcf.with_body_mass(m, m["body_mass"] * (1 + m["body_gravcomp"]))
    qpos, _, _ = gm.states(m, 4, 5, name)
    d0, d1 = oracle_built.OracleData(gm.without_gravcomp(m)), oracle_built.OracleData(gm.without_gravcomp(twin))
    for q in qpos:
        for d in (d0, d1):
            d.reset()
            d.qpos[:] = q
            d.qvel[:] = 0
            d.forward()
        want = refdyn.gravcomp_force(m, q)
        got = np.array(d1.qfrc_bias) - np.array(d0.qfrc_bias)
        assert np.abs(got - want).max() <= 1e-11, np.abs(got - want).max()


def test_switches_in_the_definition():
    """A body welded to the world, a mocap body and the world itself contribute nothing; zero gravity gives zero."""
    from mujoco_ros_pkgs_amd import mjcf, refdyn
    xml = """<mujoco><option gravity="0 0 -9.81"/><worldbody>
      <body name="fixed" pos="0 0 1" gravcomp="1"><inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/></body>
      <body name="mc" mocap="true" pos="1 0 1" gravcomp="1"><inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/></body>
      <body name="arm" pos="0 1 1"><inertial pos="0.2 0 0" mass="1" diaginertia="1 1 1"/><joint axis="0 1 0"/></body>
    </worldbody></mujoco>"""
    m = mjcf.compile_xml_string(xml)
    assert np.array_equal(m["body_gravcomp"], [0, 1, 1, 0])
    assert not refdyn.gravcomp_force(m, m["qpos0"]).any()
    T = gm.scaled_gravity(gm.model_T(), 0.0)
    assert not refdyn.gravcomp_force(T, gm.states(T, 1, 0, "T")[0][0]).any()
