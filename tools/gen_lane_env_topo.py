#!/usr/bin/env python3
"""gen_lane_env_topo.py -- integer structure of the models the lane = env kernel (csrc/mjb_lane_env.hip) is compiled for.

The lane = env kernel keeps one env per LANE with every per-body quantity in registers, so every index into them has to be a
compile-time constant: the kernel is a hand-written template over a `Topo` type that holds the model's INTEGER structure (tree,
joint kinds, dof ancestry, actuator / sensor wiring).  This script writes those tables (csrc/lane_env_topos.h) for a list of
MJCF models; all numeric constants (masses, offsets, axes, gains ...) stay run-time data read from the compiled model by scalar
loads, so editing them needs no rebuild.  `mjb_compile` matches a model against the compiled-in tables by comparing every array
below (mjb_lane_env_match); a model that matches none runs the generic kernels.

    python tools/gen_lane_env_topo.py            # regenerate from the list below (run by csrc/Makefile when this file changes)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mujoco_ros_pkgs_amd import mjcf  # noqa: E402

# (name, path): BASELINE configs[1]'s arm, and a branching two-tree test model with off-centre joints
MODELS = [
    ("franka_like", os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", "franka_like.xml")),
    ("lane_env_tree", os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", "lane_env_tree.xml")),
]

SMOOTH_SENSORS = {8, 9, 14, 23, 24, 35, 12, 13}  # jointpos, jointvel, actuatorfrc, framepos, framequat, clock, actuatorpos, actuatorvel
# ... and what the one-wavefront form of the lane = env kernel alone evaluates (LeSens, csrc/mjb_lane_env_kernel.h): a model with one of them is
# hiprtc's, never a compiled-in topology.  On a frame (body / xbody / site) without a reference frame, or on a site
FRAME_SENSORS = {23, 24, 25, 26, 27, 28, 29, 30, 31}  # framepos, framequat, frame[xyz]axis, framelinvel, frameangvel, framelinacc, frameangacc
SITE_SENSORS = {1, 2, 3, 4, 5}                        # accelerometer, velocimeter, gyro, force, torque
EXTRA_SENSORS = (FRAME_SENSORS - {23, 24}) | SITE_SENSORS
SUPPORTED_SENSORS = SMOOTH_SENSORS | EXTRA_SENSORS


DSBL_EQUALITY, DSBL_LIMIT = 1 << 1, 1 << 3  # mjDSBL_*
LE_MAX_SLOTS = 160                           # a CU's LDS in 1 KB pair slots (csrc/mjb_lane_env_kernel.h)


def limited_joints(m):
    """The joint-limit rows of an eligible model with constraint rows (mjb_lane_env_limits): 0 / 1 per joint -- none under mjDSBL_LIMIT."""
    on = m["nefcmax"] > 0 and not (int(m["disableflags"]) & DSBL_LIMIT)
    return [int(on and m["jnt_limited"][j] != 0) for j in range(m["njnt"])]


def equality_rows(m):
    """The joint-equality rows of such a model (mjb_lane_env_eq_rows): (joint1, joint2 or -1) of every ACTIVE equality, in equality order -- none under
    mjDSBL_EQUALITY."""
    if m["nefcmax"] <= 0 or (int(m["disableflags"]) & DSBL_EQUALITY):
        return []
    return [(int(m["eq_obj1id"][e]), int(m["eq_obj2id"][e]) if int(m["eq_obj2id"][e]) >= 0 else -1) for e in range(m["neq"]) if m["eq_active"][e]]


def limit_rows(m):
    """None if every constraint row the model can ever have is a joint-equality or joint-limit row the lane = env kernel sweeps with PGS (le_limit_rows,
    csrc/mjb_lane_env.hip), else the reason."""
    if int(m["solver"]) != 0:
        return "constraint rows under a solver other than PGS"
    if any(float(v) > 0 for v in m["dof_frictionloss"][:m["nv"]]):
        return "constraint rows: dry friction"
    if not (int(m["disableflags"]) & DSBL_LIMIT):
        for j in range(m["njnt"]):
            if m["jnt_limited"][j]:
                r = m["jnt_range"][j]
                if not (float(r[1]) - float(r[0]) > 2 * float(m["jnt_margin"][j])):
                    return "constraint rows: a range no wider than twice its margin"
    nr = sum(limited_joints(m)) + len(equality_rows(m))
    if nr == 0 or m["nefcmax"] != nr:
        return "constraint rows: other than one per active joint equality and one per limited joint"
    return None


def tendons_equalities(m):
    """None if the model's tendons are fixed tendons that only carry actuators and its equalities are joint equalities (le_bare_tendons,
    le_joint_equalities), else the reason."""
    for t in range(m["ntendon"]):
        if m["tendon_limited"][t] or float(m["tendon_frictionloss"][t]) != 0 or float(m["tendon_stiffness"][t]) != 0 or float(m["tendon_damping"][t]) != 0:
            return "a tendon with a limit, dry friction, a spring or a damper"
    for e in range(m["neq"]):
        j1, j2 = int(m["eq_obj1id"][e]), int(m["eq_obj2id"][e])
        if int(m["eq_type"][e]) != 2 or not (0 <= j1 < m["njnt"]) or j2 >= m["njnt"] or j2 == j1:
            return "an equality other than a joint equality"
    return None


def row_lds_slots(m):
    """Pair slots of the state, the body forces, the packed AR and the rows' qacc_warmstart (le_state_slots): what the smallest build must hold."""
    moving = set()
    for b in range(1, m["nbody"]):
        a, jointed = b, False
        while a > 0:
            jointed = jointed or m["body_jntnum"][a] > 0
            a = int(m["body_parentid"][a])
        if jointed:
            moving.add(b)
    rows = equality_rows(m)
    lim = limited_joints(m)
    nr = len(rows) + sum(lim)
    dofs = {j for j in range(m["njnt"]) if lim[j]} | {j for pair in rows for j in pair if j >= 0}
    return m["nv"] + 3 * len(moving) + (nr * (nr + 1) // 2 + len(dofs) + 1) // 2


def eligible(m):
    """None if the model fits the lane = env kernel, else the reason."""
    if m["nconmax"] > 0:
        return "constraint rows"
    if m["integrator"] != 0:
        return "integrator"
    if m["nmocap"]:
        return "mocap"
    if (m["ntendon"] or m["neq"]) and tendons_equalities(m):
        return tendons_equalities(m)
    if m["nefcmax"] > 0 and limit_rows(m):
        return limit_rows(m)
    if m["nq"] != m["nv"] or m["njnt"] != m["nv"]:
        return "a joint with more than one dof"
    if m["nv"] < 1 or m["nbody"] > 24 or m["nv"] > 20:
        return "size"
    for j in range(m["njnt"]):
        if m["jnt_type"][j] not in (2, 3) or m["jnt_qposadr"][j] != j or m["jnt_dofadr"][j] != j:
            return "joint kind / addressing"
    for b in range(m["nbody"]):
        if m["body_jntnum"][b] > 1:
            return "two joints on a body"
    for i in range(m["nsensor"]):
        if int(m["sensor_type"][i]) not in SUPPORTED_SENSORS:
            return "sensor type %d" % m["sensor_type"][i]
        if int(m["sensor_type"][i]) in FRAME_SENSORS and (m["sensor_refid"][i] >= 0 or int(m["sensor_objtype"][i]) not in (1, 2, 6)):
            return "frame sensor with a reference frame / unsupported object"
        if int(m["sensor_type"][i]) in SITE_SENSORS and int(m["sensor_objtype"][i]) != 6:
            return "site sensor on another object"
    for i in range(m["nu"]):
        if int(m["actuator_trntype"][i]) not in (0, 3) or int(m["actuator_dyntype"][i]) not in (0, 1, 2):  # joint / fixed tendon; none, integrator, filter
            return "actuator transmission / dynamics"
    if sum(int(d) != 0 for d in m["actuator_dyntype"]) != m["na"]:
        return "activation states without an actuator of their own"
    if m["nefcmax"] > 0 and row_lds_slots(m) > LE_MAX_SLOTS:
        return "constraint rows: the packed AR needs more than 160 KB of LDS per wavefront"
    return None


def arr(name, vals):
    vals = [int(v) for v in vals]
    if not vals:
        vals = [0]
    return "\tstatic constexpr int %s[%d] = { %s };\n" % (name, len(vals), ", ".join(str(v) for v in vals))


def emit(name, m):
    why = eligible(m)
    if why:
        raise SystemExit("%s does not fit the lane = env kernel: %s" % (name, why))
    if m["nefcmax"] > 0:
        raise SystemExit("%s has joint limits: mjb_lane_env_match takes no such model for a compiled-in topology" % name)
    if m["ntendon"] or m["neq"]:
        raise SystemExit("%s has tendons or equalities: mjb_lane_env_match takes no such model for a compiled-in topology" % name)
    if "body_gravcomp" in m and any(m["body_gravcomp"][1:] != 0):  # (a hand-built dict from before the field has none)
        raise SystemExit("%s has gravity compensation: mjb_lane_env_match takes no such model for a compiled-in topology" % name)
    if any(int(t) in EXTRA_SENSORS for t in m["sensor_type"][:m["nsensor"]]):
        raise SystemExit("%s has a frame-axis, velocity- or acceleration-stage sensor: mjb_lane_env_match takes no such model for a compiled-in topology" % name)
    return struct_text(name, m, [0] * m["nbody"])


def rt_struct(m):
    """The structure of any eligible model as the library writes it for hiprtc (topo_source, csrc/mjb_lane_env.hip): LeTopo_rt, with the gravity
    compensation flags set.  For tools that build such a model's kernel offline (tools/lane_env_jit_meta.py)."""
    why = eligible(m)
    if why:
        raise SystemExit("the model does not fit the lane = env kernel: %s" % why)
    gc = [int(b > 0 and m["body_gravcomp"][b] != 0) for b in range(m["nbody"])]
    text = struct_text("rt", m, gc).replace('\tstatic constexpr const char *name = "rt";\n', "")
    if m["nefcmax"] > 0:  # (the rows of the constraint stage, LeLim: a model without them has no such line)
        text = text[:text.rindex("};\n")] + arr("jnt_limited", limited_joints(m)) + "};\n"
    if m["ntendon"] > 0:  # (fixed tendons, LeTen: which actuators drive one, and every tendon's wraps)
        ten = [int(m["actuator_trnid"][i][0]) if int(m["actuator_trntype"][i]) == 3 else -1 for i in range(m["nu"])]
        text = (text[:text.rindex("};\n")] + arr("act_trntype", m["actuator_trntype"]) + arr("act_tendon", ten) + arr("tendon_adr", m["tendon_adr"]) +
                arr("tendon_num", m["tendon_num"]) + arr("wrap_jnt", m["wrap_objid"]) + "};\n")
    rows = equality_rows(m)
    if rows:  # (the equality rows, LeEq: the joint pairs of the active joint equalities)
        text = text[:text.rindex("};\n")] + arr("eq_jnt1", [r[0] for r in rows]) + arr("eq_jnt2", [r[1] for r in rows]) + "};\n"
    return text


def struct_text(name, m, body_gc):
    nb = m["nbody"]
    body_jnt = [int(m["body_jntadr"][b]) if m["body_jntnum"][b] == 1 else -1 for b in range(nb)]
    s = "struct LeTopo_%s {\n" % name
    s += '\tstatic constexpr const char *name = "%s";\n' % name
    for k in ("nbody", "nq", "nv", "nu", "na", "njnt", "nsite", "nsensor", "nsensordata", "nM"):
        s += "\tstatic constexpr int %s = %d;\n" % (k.upper() if k != "nM" else "NM", m[k])
    s += arr("body_parentid", m["body_parentid"])
    s += arr("body_rootid", m["body_rootid"])
    s += arr("body_jnt", body_jnt)
    s += arr("body_sameframe", m["body_sameframe"])
    # gravity compensation: a flag per body (the coefficient is run-time data).  Always zeros from emit() -- it refuses a model with gravcomp, which is
    # hiprtc's, whose topology text (mjb_lane_env.hip, topo_source; rt_struct here) sets the flags
    s += arr("body_gc", body_gc)
    s += arr("jnt_type", m["jnt_type"])
    s += arr("jnt_bodyid", m["jnt_bodyid"])
    # off-centre anchors: a flag per joint, 1 where jnt_pos != 0 (the offset itself is run-time data).  mjb_lane_env_match compares it: the kernel has
    # the off-centre code of the flagged joints and of no other
    s += arr("jnt_offc", [any(float(v) != 0 for v in m["jnt_pos"][j]) for j in range(m["njnt"])])
    s += arr("dof_parentid", m["dof_parentid"])
    s += arr("dof_Madr", m["dof_Madr"])
    s += arr("act_jnt", [m["actuator_trnid"][i][0] for i in range(m["nu"])])
    s += arr("act_gaintype", m["actuator_gaintype"])
    s += arr("act_biastype", m["actuator_biastype"])
    s += arr("act_ctrllimited", m["actuator_ctrllimited"])
    s += arr("act_forcelimited", m["actuator_forcelimited"])
    # activation states (mjData.act): the kind of each actuator's dynamics, its slot of act (-1: stateless), whether actrange clamps it
    stateful = m["na"] > 0
    s += arr("act_dyntype", m["actuator_dyntype"])
    s += arr("act_actadr", m["actuator_actadr"] if stateful else [0] * m["nu"])
    s += arr("act_actlimited", m["actuator_actlimited"] if stateful else [0] * m["nu"])
    s += arr("site_bodyid", m["site_bodyid"])
    s += arr("site_sameframe", m["site_sameframe"])
    s += arr("sensor_type", m["sensor_type"])
    s += arr("sensor_objtype", m["sensor_objtype"])
    s += arr("sensor_objid", m["sensor_objid"])
    s += arr("sensor_adr", m["sensor_adr"])
    s += "};\n"
    return s


# ---- the SPLIT step's smooth kernel (csrc/mjb_smooth_kernel.h): models WITH constraint rows -- free / ball joints, geoms -- whose constraint
# half runs one env per wavefront (mjb_cstep_kernel).  BASELINE configs[2]'s arm + table + cube, and a ball / free-joint test tree.
SMOOTH_MODELS = [
    ("franka_table", os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", "franka_table.xml")),
    ("split_step_tree", os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", "split_step_tree.xml")),
]


def smooth_eligible(m):
    """None if the model's smooth stages fit mjb_smooth_kernel.h, else the reason (mirrors mjb_smooth_eligible in csrc/mjb_smooth.hip)."""
    if m["integrator"] != 0:
        return "integrator"
    if m["nmocap"] or m["ntendon"] or m["neq"] or m["na"]:
        return "mocap / tendon / equality / activation"
    for b in range(m["nbody"]):
        if m["body_jntnum"][b] > 1:
            return "two joints on a body"
    if m["nbody"] > 24 or m["nv"] > 20:
        return "size"
    for i in range(m["nsensor"]):
        if int(m["sensor_type"][i]) not in SMOOTH_SENSORS:
            return "sensor type %d" % m["sensor_type"][i]
        if int(m["sensor_type"][i]) in (23, 24) and (m["sensor_refid"][i] >= 0 or int(m["sensor_objtype"][i]) not in (1, 2, 6)):
            return "frame sensor with a reference frame / unsupported object"
    for i in range(m["nu"]):
        if m["actuator_trntype"][i] != 0 or m["actuator_dyntype"][i] != 0:
            return "actuator transmission / dynamics"
        if int(m["jnt_type"][m["actuator_trnid"][i][0]]) not in (2, 3):
            return "actuator on a ball / free joint"
    return None


def handoff_layout(m):
    """csrc/mjb_dev.h: mjb_handoff_layout"""
    o, h = 0, {}
    for name, n in (("GEOM_XPOS", 3 * m["ngeom"]), ("GEOM_XMAT", 9 * m["ngeom"]), ("CDOF", 6 * m["nv"]), ("SUBTREE_COM", 3 * m["nbody"]), ("QLD", m["nM"]),
                    ("QLDIAGINV", m["nv"]), ("QH", m["nM"]), ("QHDI", m["nv"]), ("QFRC_SMOOTH", m["nv"]), ("QACC_SMOOTH", m["nv"])):
        h[name] = o
        o += n
    return h


def emit_smooth(name, m):
    why = smooth_eligible(m)
    if why:
        raise SystemExit("%s does not fit the smooth kernel: %s" % (name, why))
    nb = m["nbody"]
    body_jnt = [int(m["body_jntadr"][b]) if m["body_jntnum"][b] == 1 else -1 for b in range(nb)]
    s = "struct SmTopo_%s {\n" % name
    s += '\tstatic constexpr const char *name = "%s";\n' % name
    for k in ("nbody", "nq", "nv", "nu", "njnt", "ngeom", "nsite", "nsensor", "nsensordata", "nM"):
        s += "\tstatic constexpr int %s = %d;\n" % (k.upper() if k != "nM" else "NM", m[k])
    s += arr("body_parentid", m["body_parentid"])
    s += arr("body_rootid", m["body_rootid"])
    s += arr("body_jnt", body_jnt)
    s += arr("body_sameframe", m["body_sameframe"])
    s += arr("jnt_type", m["jnt_type"])
    s += arr("jnt_bodyid", m["jnt_bodyid"])
    s += arr("jnt_qposadr", m["jnt_qposadr"])
    s += arr("jnt_dofadr", m["jnt_dofadr"])
    s += arr("dof_parentid", m["dof_parentid"])
    s += arr("dof_Madr", m["dof_Madr"])
    s += arr("geom_bodyid", m["geom_bodyid"])
    s += arr("geom_sameframe", m["geom_sameframe"])
    s += arr("act_jnt", [m["actuator_trnid"][i][0] for i in range(m["nu"])])
    s += arr("act_gaintype", m["actuator_gaintype"])
    s += arr("act_biastype", m["actuator_biastype"])
    s += arr("act_ctrllimited", m["actuator_ctrllimited"])
    s += arr("act_forcelimited", m["actuator_forcelimited"])
    s += arr("site_bodyid", m["site_bodyid"])
    s += arr("site_sameframe", m["site_sameframe"])
    s += arr("sensor_type", m["sensor_type"])
    s += arr("sensor_objtype", m["sensor_objtype"])
    s += arr("sensor_objid", m["sensor_objid"])
    s += arr("sensor_adr", m["sensor_adr"])
    for k, v in handoff_layout(m).items():
        s += "\tstatic constexpr int H_%s = %d;\n" % (k, v)
    s += "};\n"
    return s


def main_smooth():
    out = os.path.join(ROOT, "mujoco_ros_pkgs_amd", "csrc", "smooth_topos.h")
    text = ("// smooth_topos.h -- GENERATED by tools/gen_lane_env_topo.py: the integer structure of the models the split step's smooth kernel\n"
            "// (mjb_smooth_kernel.h) is compiled for, and the offsets of the hand-off record (mjb_dev.h: mjb_handoff_layout).\n"
            "#pragma once\n\n")
    names = []
    for name, path in SMOOTH_MODELS:
        m = mjcf.compile_xml_file(path)
        text += emit_smooth(name, m) + "\n"
        names.append(name)
    text += "#define MJB_SM_TOPOS(X) " + " ".join("X(%d, SmTopo_%s)" % (i, n) for i, n in enumerate(names)) + "\n"
    text += "#define MJB_SM_NTOPO %d\n" % len(names)
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out)


def main():
    main_smooth()
    out = os.path.join(ROOT, "mujoco_ros_pkgs_amd", "csrc", "lane_env_topos.h")
    text = ("// lane_env_topos.h -- GENERATED by tools/gen_lane_env_topo.py: the integer structure of the models the lane = env kernel is\n"
            "// compiled for (tree, joint kinds, dof ancestry, actuator / sensor wiring).  Numeric model constants are run-time data.\n"
            "#pragma once\n\n")
    names = []
    for name, path in MODELS:
        m = mjcf.compile_xml_file(path)
        text += emit(name, m) + "\n"
        names.append(name)
    text += "#define MJB_LE_TOPOS(X) " + " ".join("X(%d, LeTopo_%s)" % (i, n) for i, n in enumerate(names)) + "\n"
    text += "#define MJB_LE_NTOPO %d\n" % len(names)
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out)


if __name__ == "__main__":
    main()
