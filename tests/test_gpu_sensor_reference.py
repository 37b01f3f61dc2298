"""Motion and force sensors on the GPU against tests/sensor_ref.py, the derivation that shares nothing with the oracle or the kernels: the generic
kernels' rne_post (forward()) and the lane = env kernel's LeSens (step(1): the sensors belong to the state the step started from and to the qacc it
computed).  The reference is given the kernel's own qacc.  Models, states, sampled envs and bounds are test_sensor_reference.py's (EXACT_TOL = 1e-11
without a finite difference in the reference, ACC_TOL[model] = 100 x the reference's own error where one enters it; the CPU module pins the oracle
at the same bounds and shows that every term of the reference counts).

Also here: the lane = env kernel's lean LDS budgets on S and L -- the 80 and 40 KB builds, where cinert comes from cin[] instead of LDS and L's AR /
warmstart slots sit in another layout --, reached by the batch sizes of test_gpu_lane_env_xfrc.test_lds_budgets and confirmed through the launcher's
plan (mjb_lane_env_plan, as test_gpu_lane_env_plan.py asks it).

Not here: a split-step run of L.  The split step takes compiled-in topologies with position- and velocity-stage sensors only; L is neither (hiprtc's
topology, an accelerometer and a force sensor), so set_split_step(1) leaves it with the fused kernels.  The contact identity is asked of PGS and
Newton, not of CG (test_sensor_reference.py says why)."""
import ctypes as C
import functools

import numpy as np
import pytest

import sensor_ref as sr
from test_gpu_lane_env_params import apply, draw, twin_model
from test_gpu_lane_env_sensors import NOISE, make, ran
from test_lane_env_act import oracle_env
from test_sensor_reference import (CONTACT_CASES, CONTACT_REST, EXACT_TOL, SAMPLE, against_reference, case, contact_identity_error)

pytestmark = pytest.mark.gpu

assert {0, 63, 64, 69} <= set(SAMPLE) and len(SAMPLE) >= 12
NENV = 70
PLAIN = 0      # the plan's build index of the plain lane = env build (test_gpu_lane_env_plan.py)


def _engine():
    from mujoco_ros_pkgs_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def compiled(name):
    return _engine().CompiledModel(case(name).model)


def _err(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if want.size else 0.0


# ------------------------------------------------------------------------------------------------------------- generic kernels, forward()
def forward(name, setup=None, fields=("sensordata", "qacc")):
    c = case(name)
    b = _engine().Batch(compiled(name), len(c.qpos))
    if setup:
        setup(b)
    b.set("qpos", c.qpos)
    b.set("qvel", c.qvel)
    if c.ctrl is not None and c.model["nu"]:
        b.set("ctrl", c.ctrl)
    if c.act is not None and c.model["na"]:
        b.set("act", c.act)
    if c.xfrc is not None:
        b.set("xfrc_applied", c.xfrc)
    b.forward()
    got = {f: b.get(f) for f in fields}
    b.close()
    return got


@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_generic_multi_joint_tree(lanes):
    """MJ_FREE: slide / hinge / ball joints, several per body (rne_post's cvel_before path), every sensor type, 37 envs on every group size."""
    c = case("MJ_FREE")
    got = forward("MJ_FREE", setup=lambda b: b.set_launch(lanes, 0))
    against_reference(c, got["sensordata"], got["qacc"], f"MJ_FREE, {lanes} lanes per env")


@pytest.mark.parametrize("solver", ["PGS", "Newton", "CG"])
def test_generic_constrained_tree(solver):
    """mj_con_xml without contacts: limits, friction loss, a tendon limit and equalities act -- through qacc alone."""
    name = f"MJ_CON-{solver}"
    c = case(name)
    got = forward(name, fields=("sensordata", "qacc", "nefc"))
    assert np.all(got["nefc"].ravel() > 0)
    against_reference(c, got["sensordata"], got["qacc"], f"MJ_CON, {solver}")


def test_generic_constrained_tree_on_the_row_slot_kernels():
    """The Newton model with the row capacity that selects the row-slot kernels (test_gpu_multi_joint_bodies.py); that capacity comes from its contact
    pairs, so contacts stay enabled.  The reference has no contact forces: the states whose tree touches nothing (at least half) take every sensor, the
    others every sensor but force and torque -- a contact reaches the rest through qacc alone."""
    c = case("MJ_CON-slots")
    assert c.model["nefcmax"] > 256 and compiled("MJ_CON-slots").frame_info()[0]
    got = forward("MJ_CON-slots", fields=("sensordata", "qacc", "nefc", "ncon"))
    clear = [e for e in c.envs if got["ncon"].ravel()[e] == 0]
    assert 2 * len(clear) >= len(c.envs) and np.all(got["nefc"].ravel() > 0)
    against_reference(c, got["sensordata"], got["qacc"], f"MJ_CON, row-slot kernels, {len(clear)} states without contact", envs=clear)
    rest = [i for i in sr.covered(c.model) if int(c.model["sensor_type"][i]) not in (sr.FORCE, sr.TORQUE)]
    against_reference(c, got["sensordata"], got["qacc"], "MJ_CON, row-slot kernels, states in contact, all but force / torque",
                      envs=[e for e in c.envs if e not in clear], sensors=rest)


@pytest.mark.parametrize("name", ["S-xfrc", "S-ref"])
def test_generic_wrenches_and_reference_frames(name):
    c = case(name)
    got = forward(name)
    against_reference(c, got["sensordata"], got["qacc"], f"{name}, generic kernels")


@pytest.mark.parametrize("cone,condim", CONTACT_CASES)
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_generic_contact_identity(solver, cone, condim):
    """The free root's force and torque read zero whatever the contacts do (test_sensor_reference.test_contact_identity shows the oracle's contacts on
    these states to be active, several at once, with torsional and rolling force); the child obeys the full reference."""
    name = f"contact-{solver}-{cone}-{condim}"
    c = case(name)
    got = forward(name, fields=("sensordata", "qacc", "ncon"))
    assert np.count_nonzero(got["ncon"].ravel() >= 3) >= 1 and np.all(got["ncon"].ravel() >= 1)
    w = max(contact_identity_error(c, e, got["sensordata"][e], got["qacc"][e]) for e in c.envs)
    print(f"contact {solver} {cone} condim {condim}: root's wrench / (1 + sum m |a - g|) {w:.2e} (bound 1e-11)")
    assert w <= 1e-11, w
    against_reference(c, got["sensordata"], got["qacc"], f"contact {solver} {cone} condim {condim}: the child", sensors=CONTACT_REST)


def test_generic_cfrc_ext_of_xfrc_applied():
    """The contact model lifted off the floor, a wrench on both bodies: cfrc_ext is the wrench moved to the tree's centre of mass, and the free root
    still reads zero."""
    c = case("contact-lifted")
    got = forward("contact-lifted", fields=("sensordata", "qacc", "ncon", "cfrc_ext"))
    assert not np.any(got["ncon"])
    w = max(sr.measure(got["cfrc_ext"][e], sr.cfrc_ext_of_xfrc(c.model, c.qpos[e], c.xfrc[e]).ravel()) for e in c.envs)
    print(f"cfrc_ext of xfrc_applied against the restated transfer: {w:.2e} (bound {EXACT_TOL:.0e})")
    assert w <= EXACT_TOL, w
    assert max(contact_identity_error(c, e, got["sensordata"][e], got["qacc"][e]) for e in c.envs) <= 1e-11
    against_reference(c, got["sensordata"], got["qacc"], "off the floor under wrenches: the child", sensors=CONTACT_REST)


# --------------------------------------------------------------------------------------------------------------- lane = env kernel, step(1)
def states_of(c, n=None):
    """(qpos, qvel, ctrl, act) as test_gpu_lane_env_sensors.make takes them; n > the case's batch: the case's states repeated."""
    idx = np.arange(len(c.qpos) if n is None else n) % len(c.qpos)
    act = c.act if c.act is not None else np.zeros((len(c.qpos), 0))
    return c.qpos[idx], c.qvel[idx], c.ctrl[idx], act[idx]


def lane_step(name, mode=1, setup=None, n=None, fields=("sensordata", "qacc")):
    b = make(compiled(name), states_of(case(name), n), mode=mode)
    if setup:
        setup(b)
    b.step(1)
    ran(b)     # lane_env_info() == (-2, True), built by hiprtc, the one-wavefront form
    got = {f: b.get(f) for f in fields}
    b.close()
    return got


def _xfrc(name):
    def setup(b):
        b.set_lane_env_xfrc(True)
        b.set("xfrc_applied", case(name).xfrc)
    return setup


def _hwsim_effort(b):      # effort joints only: position / velocity joints overwrite qvel inside the step and stay with the generic-kernel comparison
    b.set_lane_env_hwsim(True)
    b.hwsim_configure([dict(joint=0, method="effort"), dict(joint=2, method="effort")])
    b.hwsim_set_command("effort", np.random.default_rng(8).uniform(-2, 2, (NENV, 2)))


BUILDS = {
    "plain": ("S", None),
    "xfrc": ("S-nobase-xfrc", "xfrc"),
    "hwsim": ("S", _hwsim_effort),
    "sensors_every_step": ("S", lambda b: b.set_sensors_every_step(True)),
    "stateful": ("S-stateful", None),
    "gravcomp": ("S-gravcomp", None),
    "limits": ("L", None),
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_lane_env_builds(build):
    name, setup = BUILDS[build]
    c = case(name)
    got = lane_step(name, setup=_xfrc(name) if setup == "xfrc" else setup, fields=("sensordata", "qacc", "nefc") if name == "L" else ("sensordata", "qacc"))
    if name == "L":
        assert np.count_nonzero(got["nefc"].ravel()[list(SAMPLE)] > 0) >= len(SAMPLE) - 2
    if build == "hwsim":
        assert _err(got["qacc"], lane_step("S")["qacc"]) > 1e-3     # (the stage does act)
    against_reference(c, got["sensordata"], got["qacc"], f"lane = env, {build}")


def test_lane_env_mode_2_per_env_parameters():
    """The overlay build: per-env mass, inertia, gravity and joint parameters; the reference runs on each sampled env's twin model."""
    c = case("S")
    R = draw(c.model, NENV, 7, which=("gravity", "mass", "joint"))
    got = lane_step("S", mode=2, setup=lambda b: apply(b, R))
    refs = {e: sr.SensorRef(twin_model(c.model, R, e), c.qpos[e], c.qvel[e]) for e in SAMPLE}
    against_reference(c, got["sensordata"], got["qacc"], "lane = env, mode 2", refs=refs)
    assert _err(got["sensordata"][1:], lane_step("S")["sensordata"][1:]) > 1e-6     # (the overlay reaches the sensors)


def test_lane_env_after_a_noisy_launch():
    """20 steps under ctrl noise, the state read back, one more step: the reference at the state read."""
    c = case("S")
    b = make(compiled("S"), states_of(c), noise=NOISE, ctrl=False)
    b.step(20)
    ran(b)
    qpos, qvel = b.get("qpos"), b.get("qvel")
    b.step(1)
    ran(b)
    got = {f: b.get(f) for f in ("sensordata", "qacc")}
    b.close()
    assert _err(qpos, c.qpos) > 1e-3
    refs = {e: sr.SensorRef(c.model, qpos[e], qvel[e]) for e in SAMPLE}
    against_reference(c, got["sensordata"], got["qacc"], "lane = env, after 20 noisy steps", refs=refs)


# ------------------------------------------------------------------------------------------------------------------- the lean LDS budgets
def planned_lds_kb(cm, ncu, nenv):
    out = [C.c_int(-9) for _ in range(3)]
    assert cm.lib.mjb_lane_env_plan(cm.ptr, ncu, nenv, PLAIN, -1, 0, 0, *[C.byref(o) for o in out]) == 0
    return out[2].value


@pytest.mark.parametrize("nenv,kb", [(16384 + 37, 80), (40000, 40)], ids=["80KB", "40KB"])
@pytest.mark.parametrize("name", ["S", "L"])
def test_lane_env_lean_lds_budgets(oracle_built, name, nenv, kb):
    """More than one / two wavefronts per CU (on a 256-CU device 16 384 < 16 421 <= 32 768 < 40 000): the launcher's plan answers the 80 / 40 KB build for
    this batch and 160 KB for 70 envs.  The first 70 envs are the case's states: against the reference and the oracle on the sampled ones, against the
    70-env batch on all 70; the whole batch is finite."""
    import torch
    c, cm = case(name), compiled(name)
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert planned_lds_kb(cm, ncu, NENV) == 160
    assert planned_lds_kb(cm, ncu, nenv) == kb, f"{ncu} CUs, {nenv} envs: the plan answers {planned_lds_kb(cm, ncu, nenv)} KB, not {kb}"
    fields = ("sensordata", "qacc", "qpos", "qvel")
    got = lane_step(name, n=nenv, fields=fields)
    for f in fields:
        assert got[f].shape[0] == nenv and np.all(np.isfinite(got[f])), f
    against_reference(c, got["sensordata"], got["qacc"], f"lane = env, {name}, {nenv} envs ({kb} KB)")
    small = lane_step(name, fields=fields)
    S = states_of(c)
    want = {}
    for e in SAMPLE:
        d = oracle_env(oracle_built, c.model, S[0][e], S[1][e], S[2][e], S[3][e], 1)
        want[e] = {f: np.array(d.field(f)) for f in fields}     # (copies: the fields are views into d's memory)
    for f in fields:
        e70 = _err(got[f][:NENV], small[f])
        worst = max(_err(got[f][e], want[e][f]) for e in SAMPLE)
        print(f"{name}, {nenv} envs, {f}: against the 70-env batch {e70:.2e} (bound 1e-9), against the oracle {worst:.2e} (bound 1e-11)")
        assert e70 <= 1e-9 and worst <= 1e-11, (f, e70, worst)
    # (the batch repeats the 70 states: every block computed what the first did)
    assert _err(got["sensordata"][nenv - nenv % NENV - NENV:nenv - nenv % NENV], got["sensordata"][:NENV]) <= 1e-9
