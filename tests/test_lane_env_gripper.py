"""Fixed-tendon actuators and joint equalities under PGS in the lane = env kernel, host side, no GPU: which models the kernel takes (fixed tendons that
only carry actuators, joint equalities in both forms, equality and limit rows together at exact capacity), that such a model is hiprtc's and never a
compiled-in topology, that the models taken before keep their classification and their tape byte for byte, what the launcher's plan answers (form 0 of
the plain build; no overlay, hwsim or xfrc build), the equality and wrap records behind the limit records of the tape, the topology text, and -- in the
oracle alone -- that the constructed states of tests/lane_env_gripper_models.py hold what the GPU tests rely on."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mujoco_ros_pkgs_amd import binding, mjcf  # noqa: E402
import lane_env_gripper_models as gm  # noqa: E402
import lane_env_limit_models as lm  # noqa: E402

HDR, BODY, ACT, LIMHDR, LIM, EQ, WRAP = 8, 32, 16, 8, 16, 24, 8  # doubles per tape record (csrc/mjb_dev.h)
PLAIN, OVERLAY, HWSIM, XFRC, OVERLAY_XFRC = range(5)
GOLDEN = os.path.join(ROOT, "tests", "golden", "lane_env_gripper_digest.json")

# classification, tape doubles and sha256 of the tape's bytes, recorded from the build of the commit before fixed tendons and joint equalities
BEFORE = {
    "franka_like": (0, 536, "4eff63f02eb1cda82680693e5c505f79103b867825cb0795499278ad8db3ca34"),
    "lane_env_tree": (1, 440, "551315e72ad49c7d1de8d13c04264fe8b8bda45efb432c7789c8a70d1e22f114"),
    "model_L": (-2, 384, "d67821bc9cca31bff5e923162f4c9ca2d3756e8bac557de0c0832c9504106924"),
    "model_P": (-2, 112, "d8ae85efeefdb12cf2e925eeda1717e746b86938562f5f5868ff22b119fcf3a7"),
}


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
    rows = cm.lane_env_rows()
    cm.close()
    return v, rows


def plan(lib, model, nenv, ncu=256, build=PLAIN, form=-1, sweep=0, kb=0):
    out = [C.c_int(-9) for _ in range(3)]
    rc = lib.mjb_lane_env_plan(model, ncu, nenv, build, form, sweep, kb, *[C.byref(o) for o in out])
    return None if rc != 0 else tuple(o.value for o in out)


def _models():
    return {"G": gm.model_G(), "Q": gm.model_Q(), "franka_gripper": mjcf.load_asset("gripper/franka_gripper")}


def test_the_models_are_what_the_tests_need():
    m = gm.model_G()
    assert (m["nbody"], m["nv"], m["nq"], m["njnt"], m["nu"], m["na"]) == (8, 6, 6, 6, 3, 1) and m["nv"] <= 8
    assert [int(t) for t in m["jnt_type"]] == [3, 3, 2, 3, 3, 3]                          # hinges and one slide
    assert len({int(m["body_rootid"][b]) for b in range(1, 8)}) == 2                      # two trees
    assert int(m["body_jntnum"][3]) == 0 and int(m["body_parentid"][4]) == 3              # the jointless body in mid-chain
    assert [int(v) for v in m["eq_type"]] == [2, 2, 2, 2] and [int(v) for v in m["eq_active"]] == [1, 1, 1, 0]
    pairs = [(int(a), int(b)) for a, b in zip(m["eq_obj1id"], m["eq_obj2id"])]
    assert tuple(pairs[:3]) == gm.EQ_PAIRS
    assert int(m["dof_parentid"][1]) == 0                                                  # E0: g2 is g1's child -- ancestor / descendant
    assert int(m["body_rootid"][m["jnt_bodyid"][3]]) != int(m["body_rootid"][m["jnt_bodyid"][5]])   # E1: across the two trees
    assert pairs[2][1] < 0                                                                 # E2: the one-joint form
    data = np.asarray(m["eq_data"], float).reshape(4, 11)
    assert tuple(data[0][:5]) == gm.POLY and data[0][2] != 0                               # E0 is non-linear: poly' differs per env
    assert m["eq_solref"][1][0] < 0 and m["eq_solimp"][2][4] == 1
    assert [j for j in range(6) if m["jnt_limited"][j]] == list(gm.LIMITED) and 2 in (p[0] for p in pairs[:3])   # g3: limited AND in an equality
    assert m["nefcmax"] == gm.NE + gm.NL and m["nconmax"] <= 0 and int(m["solver"]) == 0
    assert (m["ntendon"], m["nwrap"]) == (2, 4) and [int(t) for t in m["actuator_trntype"]] == [3, 3, 0]
    assert min(float(v) for v in m["wrap_prm"]) < 0                                        # one coefficient negative
    assert int(m["actuator_forcelimited"][0]) and int(m["actuator_dyntype"][1]) == 2      # forcelimited motor; the filtered general
    st = [int(t) for t in m["sensor_type"]]
    assert st.count(8) == 6 and st.count(9) == 6 and st.count(12) == 2 and st.count(13) == 2 and st.count(14) == 2
    q = gm.model_Q()
    assert (q["nv"], q["neq"], q["nefcmax"]) == (2, 1, 1) and int(q["disableflags"]) & (1 << 8) and not np.any(q["jnt_limited"])
    assert int(q["body_rootid"][1]) != int(q["body_rootid"][2])
    g = mjcf.load_asset("gripper/franka_gripper")
    assert (g["nv"], g["nu"], g["neq"], g["ntendon"], g["nefcmax"]) == (9, 8, 1, 1, 10) and np.all(np.asarray(g["jnt_limited"]) != 0)
    assert int(g["actuator_trntype"][7]) == 3 and [float(v) for v in g["wrap_prm"]] == [0.5, 0.5] and not np.any(g["jnt_stiffness"])
    # the constructed states
    s = gm.sides_G()
    assert sorted(set(np.count_nonzero(s, axis=1))) == [0, 1, 2, 3]
    assert all(np.any((s[e] != 0) != (s[e + 1] != 0)) for e in range(gm.NENV - 1))   # neighbouring lanes differ in their active set
    assert all({-1, 1} <= set(s[:, r]) for r in range(gm.NL))                         # both sides of every limit
    assert np.any(s[63]) and np.any(s[64]) and np.any(s[69])
    x = gm.states_G(m)[0][:, 0] - float(m["qpos0"][0])
    assert np.count_nonzero(x > 0.1) >= 15 and np.count_nonzero(x < -0.1) >= 15       # x of the non-linear equality over both signs


def test_which_models_the_kernel_takes(engine):
    """Fails on the commit before: G, Q and franka_gripper were refused (-1) for their tendons and equalities."""
    import gen_lane_env_topo as gen
    want = {"G": (6, 3, 3), "Q": (1, 1, 0), "franka_gripper": (10, 1, 9)}
    for name, m in _models().items():
        assert classify(engine, m) == (-2, want[name]), name
        assert gen.eligible(m) is None, name
    for name, kw in gm.VARIANTS.items():
        m = gm.model_G(**kw)
        assert classify(engine, m) == (-1, (0, 0, 0)), name
        assert gen.eligible(m) is not None, name
    # row kinds switched off by flag have no rows (njmax follows); G under mjDSBL_CONSTRAINT is a tendon model without a constraint stage
    assert classify(engine, gm.model_G(flags=' equality="disable"', njmax=gm.NL)) == (-2, (3, 0, 3))
    assert classify(engine, gm.model_G(flags=' limit="disable"', njmax=gm.NE)) == (-2, (3, 3, 0))
    assert classify(engine, gm.model_G(rows=False)) == (-2, (0, 0, 0))
    # room for the inactive equality's row: an env could switch it on (set_env_equality) -- the generic kernels
    roomy = gm.model_G(njmax=gm.NE + gm.NL + 1)
    assert roomy["nefcmax"] == gm.NE + gm.NL + 1 and classify(engine, roomy)[0] == -1 and gen.eligible(roomy) is not None
    # an equality of a joint with itself
    same = mjcf.compile_xml_string(gm.model_G_xml().replace('joint1="g4" joint2="g6"', 'joint1="g4" joint2="g4"'))
    assert classify(engine, same)[0] == -1 and gen.eligible(same) is not None


def test_models_taken_before_are_unchanged(engine):
    """franka_like, lane_env_tree, and the limit models L and P: the classification, the tape's size and its bytes of the commit before."""
    models = {"franka_like": mjcf.load_asset("franka_like"), "lane_env_tree": mjcf.load_asset("lane_env_tree"), "model_L": lm.model_L(), "model_P": lm.model_P()}
    for name, m in models.items():
        cm = engine.CompiledModel(m)
        tape = cm.lane_env_tape()
        got = (int(cm.lib.mjb_model_lane_env(cm.ptr)), int(tape.size), hashlib.sha256(np.ascontiguousarray(tape, dtype=np.float64).tobytes()).hexdigest())
        assert got == BEFORE[name], name
        assert cm.lane_env_rows() == {"model_L": (4, 0, 4), "model_P": (1, 0, 1)}.get(name, (0, 0, 0)), name
        cm.close()


def test_topology_text_gains_only_what_the_model_has():
    """The tendon wiring and the equality rows' joint pairs are compile-time facts: part of the text hiprtc is handed, which keys the kernel cache.  A model
    without tendons or equalities has none of the lines -- its text, and so its cache key, is what it was."""
    import gen_lane_env_topo as gen
    text = gen.rt_struct(gm.model_G())
    for line in ("act_trntype[3] = { 3, 3, 0 }", "act_tendon[3] = { 0, 1, -1 }", "tendon_adr[2] = { 0, 2 }", "tendon_num[2] = { 2, 2 }",
                 "wrap_jnt[4] = { 1, 3, 4, 5 }", "eq_jnt1[3] = { 1, 3, 2 }", "eq_jnt2[3] = { 0, 5, -1 }", "jnt_limited[6] = { 1, 0, 1, 0, 1, 0 }"):
        assert line in text, line
    for m in (lm.model_L(), lm.model_L(limits=False), mjcf.load_asset("franka_like")):
        t = gen.rt_struct(m)
        assert not any(k in t for k in ("act_trntype", "act_tendon", "tendon_adr", "tendon_num", "wrap_jnt", "eq_jnt"))
    assert hashlib.sha256(gen.rt_struct(lm.model_L()).encode()).hexdigest() == "ada7f3191195f1ca7e26efc14867f85235fddb2c883a8544236a7d650ee44a6d"
    # rows a flag switches off are not in the text; the tendon lines stay
    t = gen.rt_struct(gm.model_G(flags=' equality="disable"', njmax=gm.NL))
    assert "eq_jnt" not in t and "wrap_jnt" in t and "jnt_limited[6] = { 1, 0, 1, 0, 1, 0 }" in t
    t = gen.rt_struct(gm.model_G(flags=' limit="disable"', njmax=gm.NE))
    assert "eq_jnt1[3]" in t and "jnt_limited[6] = { 0, 0, 0, 0, 0, 0 }" in t
    t = gen.rt_struct(gm.model_G(rows=False))
    assert "eq_jnt" not in t and "jnt_limited" not in t and "act_tendon[3] = { 0, 1, -1 }" in t
    with pytest.raises(SystemExit, match="joint limits|tendons or equalities"):
        gen.emit("G", gm.model_G())


def test_plan_is_form_0_of_the_plain_build(engine):
    lib = binding.load_library()
    for name, m in list(_models().items()) + [("G without rows", gm.model_G(rows=False))]:
        cm = engine.CompiledModel(m)
        for form in (-1, 0, 1, 2, 3):
            for nenv in (70, 4096, 16385, 65536):
                got = plan(lib, cm.ptr, nenv, form=form)
                assert got is not None and got[0] == 0 and got[1] == 0, (name, form, nenv, got)
        for build in (OVERLAY, HWSIM, XFRC, OVERLAY_XFRC):
            for form in (-1, 0, 3):
                assert plan(lib, cm.ptr, 4096, build=build, form=form) is None, (name, build, form)
        cm.close()
    # the packed AR beside the state sets the smallest budget: G (21 + 6 doubles) and the gripper arm (55 + 9) need 80 KB where 40 is asked for
    for m in (gm.model_G(), mjcf.load_asset("gripper/franka_gripper")):
        cm = engine.CompiledModel(m)
        assert plan(lib, cm.ptr, 65536, kb=40)[2] == 80
        cm.close()


def _getsolparam(m, sr, si):
    sr = [float(v) for v in sr]
    if (sr[0] > 0) != (sr[1] > 0):
        sr = [0.02, 1.0]
    if not (int(m["disableflags"]) & (1 << 11)) and sr[0] > 0:
        sr[0] = max(sr[0], 2 * float(np.ravel(m["timestep"])[0]))
    si = [float(v) for v in si]
    imp = [min(0.9999, max(0.0001, si[0])), min(0.9999, max(0.0001, si[1])), max(0.0, si[2]), min(0.9999, max(0.0001, si[3])), max(1.0, si[4])]
    return sr, imp


def test_tape_carries_the_equality_and_wrap_records_behind_the_limit_records(engine):
    m = gm.model_G()
    cm = engine.CompiledModel(m)
    tape = cm.lane_env_tape()
    nb, nu = int(m["nbody"]), int(m["nu"])
    base = HDR + BODY * nb + ACT * nu
    assert tape.size == base + LIMHDR + LIM * gm.NL + EQ * gm.NE + WRAP * 4
    # G without rows: the same header, body and actuator records, and the wrap records directly behind them
    cf = engine.CompiledModel(gm.model_G(rows=False))
    tfree = cf.lane_env_tape()
    assert tfree.size == base + WRAP * 4 and np.array_equal(tape[:base], tfree[:base])
    assert list(tfree[base::WRAP]) == [1.0, -0.7, 0.5, 0.5] and not np.any(np.delete(tfree[base:], np.arange(0, 4 * WRAP, WRAP)))
    cf.close()
    h = tape[base:base + LIMHDR]
    mi = float(np.ravel(m["meaninertia"])[0])
    assert h[0] == mi and h[1] == 1e-8 and h[2] == 100 and h[3] == 1.0 / (mi * 6) and h[4] == 0 and h[5] == 0
    for r, j in enumerate(gm.LIMITED):
        rec = tape[base + LIMHDR + LIM * r:base + LIMHDR + LIM * (r + 1)]
        sr, imp = _getsolparam(m, m["jnt_solref"][j], m["jnt_solimp"][j])
        assert np.array_equal(rec[0:2], np.asarray(m["jnt_range"], float).reshape(-1, 2)[j]) and rec[2] == m["jnt_margin"][j]
        assert list(rec[3:5]) == sr and list(rec[5:10]) == imp and rec[10] == m["dof_invweight0"][j]
    e0 = base + LIMHDR + LIM * gm.NL
    data = np.asarray(m["eq_data"], float).reshape(-1, 11)
    iw = np.asarray(m["dof_invweight0"], float)
    for r, (j1, j2) in enumerate(gm.EQ_PAIRS):
        rec = tape[e0 + EQ * r:e0 + EQ * (r + 1)]
        sr, imp = _getsolparam(m, m["eq_solref"][r], m["eq_solimp"][r])
        assert np.array_equal(rec[0:5], data[r][:5])
        assert rec[5] == m["qpos0"][j1] and rec[6] == (m["qpos0"][j2] if j2 >= 0 else 0.0)
        assert list(rec[7:9]) == sr and list(rec[9:14]) == imp
        assert rec[14] == iw[j1] + (iw[j2] if j2 >= 0 else 0.0)
        if sr[0] > 0:
            K, B = 1 / (imp[1] ** 2 * sr[0] ** 2 * sr[1] ** 2), 2 / (imp[1] * sr[0])
        else:
            K, B = -sr[0] / imp[1] ** 2, -sr[1] / imp[1]
        assert abs(rec[15] - K) <= 1e-12 * K and abs(rec[16] - B) <= 1e-12 * B
        assert abs(rec[17] - 1 / imp[3] ** (imp[4] - 1)) <= 1e-15 and abs(rec[18] - 1 / (1 - imp[3]) ** (imp[4] - 1)) <= 1e-15
        assert not np.any(rec[19:])
    assert tape[e0 + EQ + 7] == -400 and tape[e0 + 2 * EQ + 13] == 1          # E1's direct solref, E2's power 1
    w0 = e0 + EQ * gm.NE
    assert list(tape[w0::WRAP]) == [1.0, -0.7, 0.5, 0.5]                       # the PLAIN coefficients, in wrap order; the gear stays in the actuator record
    assert tape[HDR + BODY * nb] == 2.0 and tape[HDR + BODY * nb + ACT] == 1.5
    cm.close()
    # a model with equalities and no limits has the header all the same
    q = gm.model_Q()
    cq = engine.CompiledModel(q)
    t = cq.lane_env_tape()
    assert t.size == HDR + BODY * 3 + ACT * 2 + LIMHDR + EQ and t[HDR + BODY * 3 + ACT * 2 + 4] == 1   # (warmstart disabled)
    cq.close()


def test_digests_of_the_new_models(engine):
    """G, Q, franka_gripper and two refused variants, as compiled: the four digest words (tests/test_model_digest.py) recorded with this change."""
    from test_model_digest import digest
    with open(GOLDEN) as f:
        golden = json.load(f)
    models = dict(_models(), **{"G: " + v: gm.model_G(**gm.VARIANTS[v]) for v in gm.DIGEST_VARIANTS})
    assert sorted(golden) == sorted(models)
    for name, m in models.items():
        assert digest(m) == golden[name], name


def test_oracle_on_the_constructed_states(oracle_built):
    """The oracle alone on G's states: three equality rows in every env and every count of limit rows from 0 to 3 on top, lanes 63, 64 and 69 with limit
    rows; the sweeps end ahead of the cap in at least 90 % of the envs; at most 4 of the 70 envs are marginal (their iteration count moves with the
    tolerance x 0.999 / x 1.001)."""
    ref = gm.reference_G()
    want = gm.NE + np.count_nonzero(gm.sides_G(), axis=1)
    assert np.array_equal(ref["nefc"], want) and sorted(set(ref["nefc"])) == [3, 4, 5, 6]
    assert ref["nefc"][63] > gm.NE and ref["nefc"][64] > gm.NE and ref["nefc"][69] > gm.NE
    assert np.count_nonzero(ref["solver_iter"] < 100) >= 0.9 * gm.NENV and np.all(ref["solver_iter"] >= 1)
    assert np.count_nonzero(ref["marginal"]) <= 4
    print("solver_iter over the envs:", sorted(set(int(v) for v in ref["solver_iter"])), "marginal:", np.flatnonzero(ref["marginal"]))
    assert np.abs(ref["qfrc_constraint"]).max() > 1 and np.all(np.isfinite(ref["qacc"]))
    assert np.all(np.abs(ref["qfrc_constraint"]).max(axis=0) > 0.1)     # every dof is reached by some row
    for kw in (dict(iterations=3), dict(flags=' warmstart="disable"'), dict(flags=' equality="disable"', njmax=gm.NL), dict(flags=' limit="disable"', njmax=gm.NE)):
        r = gm.reference_G(**kw)
        assert np.count_nonzero(r["marginal"]) <= 4, kw
        assert np.count_nonzero(r["solver_iter"] < 100) >= 0.9 * gm.NENV, kw
    assert np.all(gm.reference_G(iterations=3)["solver_iter"] <= 3) and np.count_nonzero(gm.reference_G(iterations=3)["solver_iter"] == 3) >= 8
    assert sorted(set(gm.reference_G(flags=' equality="disable"', njmax=gm.NL)["nefc"])) == [0, 1, 2, 3]
    assert np.all(gm.reference_G(flags=' limit="disable"', njmax=gm.NE)["nefc"] == gm.NE)


if __name__ == "__main__":   # writes the digest fixture from whatever library is built
    from test_model_digest import digest
    rec = dict({name: digest(m) for name, m in _models().items()}, **{"G: " + v: digest(gm.model_G(**gm.VARIANTS[v])) for v in gm.DIGEST_VARIANTS})
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} models -> {GOLDEN}")
