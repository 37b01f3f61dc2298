"""The models mjb_compile is pinned on (tests/test_model_digest.py): name -> a function that returns the compiled model dict.  Together they
reach every branch of the model compiler: every joint type and joint list, the three integrators, the three solvers and both cones,
joint / tendon / site transmissions, stateful actuators, gravity compensation, <contact><pair>, every sensor family, the lane = env and
split-step topologies, the wide-frame search (Newton, 128 < nefcmax <= 256) and the row-slot / HBM frames (nefcmax > 256)."""
import os

import gravcomp_models
import lane_env_limit_models
import lane_env_sensor_models
import multi_joint_models
import test_contact_pairs
import test_large_constraint_sets
import test_site_transmission
import test_slot_scenes
import test_tendon_transmission
from mujoco_ros_pkgs_amd import mjcf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ASSETS = ["franka_like", "franka_table", "lane_env_tree", "shadow_hand_grasp", "shadow_hand_like", "split_step_tree"]
WORLDS = ["empty_world", "equality_world", "mocap_world", "pendulum_world", "sensors_world"]


def _xml(s):
    return lambda: mjcf.compile_xml_string(s)


MODELS = {}
for _n in ASSETS:
    MODELS["asset " + _n] = lambda n=_n: mjcf.load_asset(n)
for _n in WORLDS:
    MODELS["world " + _n] = lambda n=_n: mjcf.compile_xml_file(os.path.join(GOLDEN, n + ".xml"))
MODELS.update({
    # tests/multi_joint_models.py
    "mj_free": _xml(multi_joint_models.MJ_FREE),
    "mj_con newton pyramidal": _xml(multi_joint_models.mj_con_xml("Newton", "pyramidal")),
    "mj_con pgs elliptic": _xml(multi_joint_models.mj_con_xml("PGS", "elliptic")),
    "mj_con cg elliptic rk4": _xml(multi_joint_models.mj_con_xml("CG", "elliptic", "RK4")),
    "mj_con newton implicitfast no contact": _xml(multi_joint_models.mj_con_xml("Newton", "pyramidal", "implicitfast", contact=False)),
    "mj_con newton extra geoms": _xml(multi_joint_models.mj_con_xml("Newton", "elliptic", extra_geoms=1)),
    "ball_then_hinge": _xml(multi_joint_models.BALL_THEN_HINGE),
    "two_joint_tree 7": _xml(multi_joint_models.two_joint_tree(7, 3)),
    "two_joint_tree 20 pgs": _xml(multi_joint_models.two_joint_tree(20, 5, "PGS")),
    "hinge_slide_two_joint_tree": _xml(multi_joint_models.hinge_slide_two_joint_tree()),
    "hinge_slide_two_joint_tree unlimited": _xml(multi_joint_models.hinge_slide_two_joint_tree(limited=False)),
    # tests/lane_env_limit_models.py
    "limits L": lane_env_limit_models.model_L,
    "limits L unlimited": lambda: lane_env_limit_models.model_L(limits=False),
    "limits P": lane_env_limit_models.model_P,
    # tests/lane_env_sensor_models.py
    "sensors S": lane_env_sensor_models.model_S,
    "sensors S stateful": lambda: lane_env_sensor_models.model_S(stateful=True),
    "sensors S gravcomp": lambda: lane_env_sensor_models.model_S(gravcomp=True),
    "sensors S rk4 no base wrench": lambda: lane_env_sensor_models.model_S(integrator="RK4", base_wrench=False),
    "sensors P": lane_env_sensor_models.model_P,
    # tests/gravcomp_models.py
    "gravcomp T": gravcomp_models.model_T,
    "gravcomp T post sensors": lambda: gravcomp_models.model_T(sensors=gravcomp_models.POST_SENSORS),
    "gravcomp X": gravcomp_models.model_X,
    "gravcomp X rk4": lambda: gravcomp_models.model_X(integrator="RK4"),
    "gravcomp C pgs": lambda: gravcomp_models.model_C(0.5),
    "gravcomp C newton implicitfast": lambda: gravcomp_models.model_C(1.0, "Newton", "implicitfast"),
    # the integrators on the flagship model
    "franka_like rk4": lambda: mjcf.load_asset("franka_like", override={"integrator": "RK4"}),
    "franka_like implicitfast": lambda: mjcf.Model(dict(mjcf.load_asset("franka_like"), integrator=3)),  # (mjINT_IMPLICITFAST)
    # site and tendon transmissions
    "site quad": test_site_transmission.quad_model,
    "site quad floor pgs elliptic implicitfast": lambda: test_site_transmission.quad_model("implicitfast", "PGS", "elliptic", floor=True, z=0.15),
    "site arm 6d": test_site_transmission.arm_model,
    "site arm floor cg": lambda: test_site_transmission.arm_model(test_site_transmission.ARM_6D, "Euler", "CG", "pyramidal", floor=True, njmax=40),
    "tendon actuators": test_tendon_transmission.model_of,
    "tendon actuators rk4": lambda: test_tendon_transmission.model_of("RK4"),
    "tendon actuators pgs contacts": lambda: test_tendon_transmission.model_of("Euler", "PGS", "pyramidal", True),
    # <contact><pair>
    "pairs newton elliptic": test_contact_pairs.model_of,
    "pairs pgs pyramidal": lambda: test_contact_pairs.model_of("PGS", "pyramidal"),
    "pairs cg elliptic": lambda: test_contact_pairs.model_of("CG", "elliptic"),
    # Newton, 128 < nefcmax <= 256: the wide-frame search (asset shadow_hand_grasp is one too)
    "grid newton 200": lambda: test_large_constraint_sets.grid_model("Newton", "pyramidal", 3, njmax=200, nconmax=64, n=2),
    "grid newton elliptic 256": lambda: test_large_constraint_sets.grid_model("Newton", "elliptic", 3, njmax=256, nconmax=64, n=2),
    "grid cg 200": lambda: test_large_constraint_sets.grid_model("CG", "pyramidal", 3, njmax=200, nconmax=64, n=2),
    # nefcmax > 256: the row-slot kernels, frames in LDS / the full frame in HBM / both in HBM
    "rows 63 of 300": lambda: test_slot_scenes.rows_model(63, njmax=300),
    "rows 128 of 600 cg": lambda: test_slot_scenes.rows_model(128, "CG", njmax=600),
    "rows 1024": lambda: test_slot_scenes.rows_model(1024),
    "rows 1023 four hinges": lambda: test_slot_scenes.rows_model(1023, nhinge=4, nfric=4),
    "every row newton elliptic": test_slot_scenes.every_row_model,
    "every row cg pyramidal limitfrc": lambda: test_slot_scenes.every_row_model("CG", "pyramidal", limitfrc=True),
    "small grid 300": lambda: test_large_constraint_sets.small_grid_model("Newton", 300),
    "small grid 400 cg": lambda: test_large_constraint_sets.small_grid_model("CG", 400),
    "condim3 grid": lambda: test_slot_scenes.condim3_grid_model("Newton"),
})
for _k, _kw in lane_env_limit_models.VARIANTS.items():
    MODELS["limits L " + _k] = lambda kw=_kw: lane_env_limit_models.model_L(**kw)
for _k, _more in lane_env_sensor_models.REFUSED.items():
    MODELS["sensors S " + _k] = lambda more=_more: lane_env_sensor_models.model_S(more=more)
for _seed in range(18):  # (solver = seed % 3, cone = seed // 3 % 2, integrator = seed // 6 % 3: every combination once)
    MODELS[f"random multijoint {_seed}"] = _xml(multi_joint_models.random_multijoint_model(_seed))
