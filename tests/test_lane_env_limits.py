"""Joint limits under PGS in the lane = env kernel, host side, no GPU: which models the kernel takes (every constraint row a hinge / slide joint-limit
row, PGS, one row per limited joint at most, full capacity), that such a model is hiprtc's and never a compiled-in topology, what the launcher's plan
answers for it (form 0 of the plain build; no overlay, hwsim or xfrc build), the limit records behind the constant tape, and -- in the oracle alone --
that the constructed states of tests/lane_env_limit_models.py hold every count of active rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import binding, mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lane_env_limit_models as lm  # noqa: E402

HDR, BODY, ACT, LIMHDR, LIM = 8, 32, 16, 8, 16  # doubles per tape record (csrc/mjb_dev.h)
PLAIN, OVERLAY, HWSIM, XFRC, OVERLAY_XFRC = range(5)


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g
    from mujoco_ros_pkgs_amd import engine as e
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    binding.load_library()
    return e


def classify(engine, model):
    cm = engine.CompiledModel(model)
    v = int(cm.lib.mjb_model_lane_env(cm.ptr))
    cm.close()
    return v


def plan(lib, model, nenv, ncu=256, build=PLAIN, form=-1, sweep=0, kb=0):
    out = [C.c_int(-9) for _ in range(3)]
    rc = lib.mjb_lane_env_plan(model, ncu, nenv, build, form, sweep, kb, *[C.byref(o) for o in out])
    return None if rc != 0 else tuple(o.value for o in out)


def test_the_models_are_what_the_tests_need():
    m = lm.model_L()
    assert (m["nbody"], m["nv"], m["nq"], m["njnt"], m["nu"]) == (8, 6, 6, 6, 3)
    assert [int(v) for v in m["jnt_limited"]] == [1, 0, 1, 1, 0, 1] and m["nefcmax"] == 4 and m["nconmax"] <= 0
    assert [j for j in range(6) if m["jnt_limited"][j]] == list(lm.LIMITED)
    assert [int(t) for t in m["jnt_type"]] == [3, 3, 2, 3, 3, 3]           # one slide
    assert int(m["body_jntnum"][4]) == 0 and int(m["body_parentid"][5]) == 4   # the jointless body in mid-chain
    assert int(m["dof_parentid"][2]) == 1 and int(m["dof_parentid"][1]) == 0   # the unlimited j2 between the limited j1 and j3
    assert np.any(np.asarray(m["jnt_pos"])[0] != 0)
    assert m["jnt_margin"][2] == 0.05 and m["jnt_solimp"][2][4] == 1 and m["jnt_solref"][3][0] < 0 and m["jnt_solimp"][5][2] == 0
    assert int(m["solver"]) == 0 and int(m["iterations"]) == 100 and float(np.ravel(m["tolerance"])[0]) == 1e-8
    assert np.count_nonzero(np.asarray(m["gravity"])) == 3 and np.all(np.asarray(m["dof_damping"]) > 0)
    p = lm.model_P()
    assert (p["nv"], p["nefcmax"]) == (1, 1) and int(p["jnt_type"][0]) == 2 and int(p["disableflags"]) & (1 << 8)
    # the constructed active sets
    s = lm.sides_L()
    assert sorted(set(np.count_nonzero(s, axis=1))) == [0, 1, 2, 3, 4]
    assert all(np.any((s[e] != 0) != (s[e + 1] != 0)) for e in range(lm.NENV - 1))   # neighbouring lanes differ in their active set
    assert all({-1, 1} <= set(s[:, r]) for r in range(4))                              # both sides of every limit
    assert np.any(s[63]) and np.any(s[64]) and not np.any(s[69])
    assert s[lm.DEEP_ENV, lm.DEEP_ROW] != 0


def test_which_models_the_kernel_takes(engine):
    import gen_lane_env_topo as gen
    assert classify(engine, lm.model_L()) == -2 and gen.eligible(lm.model_L()) is None
    assert classify(engine, lm.model_P()) == -2 and gen.eligible(lm.model_P()) is None
    for name, kw in lm.VARIANTS.items():
        m = lm.model_L(**kw)
        assert classify(engine, m) == -1, name
        assert gen.eligible(m) is not None, name
    # limits switched off by flag: no rows, the unconstrained model the kernel took before
    assert classify(engine, lm.model_L(flags=' limit="disable"')) == -2
    # what was classified before stays what it was
    assert classify(engine, mjcf.load_asset("franka_like")) == 0
    assert classify(engine, mjcf.load_asset("lane_env_tree")) == 1
    assert classify(engine, mjcf.load_asset("franka_table")) == -1


def test_a_limited_model_is_never_a_compiled_in_topology(engine):
    """franka_like with limited="true" on its nine joints has the compiled-in topology's structure in every array mjb_lane_env_match compares: it is
    refused there (-2: hiprtc's), and the generator refuses to emit it."""
    import gen_lane_env_topo as gen
    xml = open(os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", "franka_like.xml")).read()
    lim = mjcf.compile_xml_string(xml.replace("<joint ", '<joint limited="true" '))
    assert np.all(np.asarray(lim["jnt_limited"]) != 0) and lim["nefcmax"] == 9
    assert classify(engine, lim) == -2
    with pytest.raises(SystemExit, match="joint limits"):
        gen.emit("limited", lim)
    with pytest.raises(SystemExit, match="joint limits"):
        gen.emit("L", lm.model_L())


def test_topology_text_carries_the_limit_set():
    """The limit set is a compile-time fact: it is part of the text hiprtc is handed, which keys the kernel cache.  A model without rows has no such line."""
    import gen_lane_env_topo as gen
    text = gen.rt_struct(lm.model_L())
    assert "jnt_limited[6] = { 1, 0, 1, 1, 0, 1 }" in text
    free = gen.rt_struct(lm.model_L(limits=False))
    assert "jnt_limited" not in free
    assert text.replace("\tstatic constexpr int jnt_limited[6] = { 1, 0, 1, 1, 0, 1 };\n", "") == free
    other = lm.model_L_xml().replace('<joint name="j2" type="hinge" axis="0 1 0"', '<joint name="j2" type="hinge" axis="0 1 0" limited="true" range="-1 1"')
    assert "jnt_limited[6] = { 1, 1, 1, 1, 0, 1 }" in gen.rt_struct(mjcf.compile_xml_string(other))


def test_plan_is_form_0_of_the_plain_build(engine):
    lib = binding.load_library()
    for m in (lm.model_L(), lm.model_P()):
        cm = engine.CompiledModel(m)
        for form in (-1, 0, 1, 2, 3):
            for nenv in (70, 4096, 16385, 65536):
                got = plan(lib, cm.ptr, nenv, form=form)
                assert got is not None and got[0] == 0 and got[1] == 0, (form, nenv, got)
        for build in (OVERLAY, HWSIM, XFRC, OVERLAY_XFRC):
            for form in (-1, 0, 3):
                assert plan(lib, cm.ptr, 4096, build=build, form=form) is None, (build, form)
        cm.close()
    # the same tree without limits keeps its forms and its builds
    cm = engine.CompiledModel(lm.model_L(limits=False))
    assert plan(lib, cm.ptr, 4096, build=XFRC) is not None and plan(lib, cm.ptr, 4096, build=OVERLAY) is not None
    cm.close()


def _getsolparam(m, j):
    sr = [float(v) for v in m["jnt_solref"][j]]
    if (sr[0] > 0) != (sr[1] > 0):
        sr = [0.02, 1.0]
    if not (int(m["disableflags"]) & (1 << 11)) and sr[0] > 0:
        sr[0] = max(sr[0], 2 * float(np.ravel(m["timestep"])[0]))
    si = [float(v) for v in m["jnt_solimp"][j]]
    imp = [min(0.9999, max(0.0001, si[0])), min(0.9999, max(0.0001, si[1])), max(0.0, si[2]), min(0.9999, max(0.0001, si[3])), max(1.0, si[4])]
    return sr, imp


def test_tape_keeps_its_offsets_and_carries_the_limit_records(engine):
    m = lm.model_L()
    free = lm.model_L(limits=False)
    cm, cf = engine.CompiledModel(m), engine.CompiledModel(free)
    tape, tfree = cm.lane_env_tape(), cf.lane_env_tape()
    nb, nu, nl = int(m["nbody"]), int(m["nu"]), 4
    base = HDR + BODY * nb + ACT * nu
    assert tfree.size == base and tape.size == base + LIMHDR + LIM * nl
    assert np.array_equal(tape[:base], tfree)   # header, body and actuator records where they were
    h = tape[base:base + LIMHDR]
    mi = float(np.ravel(m["meaninertia"])[0])
    assert h[0] == mi and h[1] == 1e-8 and h[2] == 100 and h[3] == 1.0 / (mi * 6) and h[4] == 0 and h[5] == 0
    for r, j in enumerate(lm.LIMITED):
        rec = tape[base + LIMHDR + LIM * r:base + LIMHDR + LIM * (r + 1)]
        sr, imp = _getsolparam(m, j)
        assert np.array_equal(rec[0:2], np.asarray(m["jnt_range"], float).reshape(-1, 2)[j]) and rec[2] == m["jnt_margin"][j]
        assert list(rec[3:5]) == sr and list(rec[5:10]) == imp
        assert rec[10] == m["dof_invweight0"][j]
    cm.close()
    cf.close()
    # the clamps: a mixed-sign solref becomes the default, refsafe lifts a short time constant, solimp is cut to its legal ranges; the disable bits
    x = lm.model_L(flags=' warmstart="disable"')
    x["jnt_solref"] = np.array(x["jnt_solref"], float)
    x["jnt_solimp"] = np.array(x["jnt_solimp"], float)
    x["jnt_solref"][0] = (0.03, -1.0)
    x["jnt_solref"][2] = (0.001, 0.7)
    x["jnt_solimp"][5] = (-0.5, 1.5, -1.0, 2.0, 0.5)
    cx = engine.CompiledModel(x)
    t = cx.lane_env_tape()
    recs = [t[base + LIMHDR + LIM * r:base + LIMHDR + LIM * (r + 1)] for r in range(nl)]
    assert list(recs[0][3:5]) == [0.02, 1.0]
    assert list(recs[1][3:5]) == [2 * 0.002, 0.7]
    assert list(recs[3][5:10]) == [0.0001, 0.9999, 0.0, 0.9999, 1.0]
    assert t[base + 4] == 1 and t[base + 5] == 0
    cx.close()
    y = lm.model_L(flags=' refsafe="disable"')
    y["jnt_solref"] = np.array(y["jnt_solref"], float)
    y["jnt_solref"][2] = (0.001, 0.7)
    cy = engine.CompiledModel(y)
    t = cy.lane_env_tape()
    assert list(t[base + LIMHDR + LIM + 3:base + LIMHDR + LIM + 5]) == [0.001, 0.7] and t[base + 4] == 0 and t[base + 5] == 1
    cy.close()


def test_oracle_sees_every_count_of_active_rows(oracle_built):
    """The oracle alone on L's states: nefc of every env is what sides_L constructs -- each count from 0 to 4 --, lanes 63 and 64 have rows, the tail's last
    env has none, and the forces act."""
    ref = lm.reference_L()
    want = np.count_nonzero(lm.sides_L(), axis=1)
    assert np.array_equal(ref["nefc"], want)
    assert sorted(set(ref["nefc"])) == [0, 1, 2, 3, 4]
    assert ref["nefc"][63] > 0 and ref["nefc"][64] > 0 and ref["nefc"][69] == 0
    assert np.all(ref["solver_iter"][ref["nefc"] == 0] == 0) and np.all(ref["solver_iter"][ref["nefc"] > 0] >= 1)
    assert ref["solver_iter"].max() < 100   # every env converges ahead of the cap
    assert np.abs(ref["qfrc_constraint"]).max() > 1 and np.all(np.isfinite(ref["qacc"]))
    print("solver_iter over the envs:", sorted(set(int(v) for v in ref["solver_iter"])))
    capped = lm.reference_L(iterations=3)
    assert np.any(capped["solver_iter"] == 3) and capped["solver_iter"].max() == 3
