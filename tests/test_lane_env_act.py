"""Activation states (mjData.act: dyntype integrator / filter, <intvelocity>, <cylinder>) in the lane = env kernel, host side, no GPU: which models the
kernel takes, what the launcher's plan answers for them (one wavefront per 64 envs whatever is asked for; no build with the hwsim stage), and the
slots of the constant tape (LeTapeAct, csrc/mjb_dev.h) that hold the filter's time constant and actrange.  Also home of the two models, the states
and the oracle rollouts tests/test_gpu_lane_env_act.py runs: the seeds are chosen here, where the oracle alone says how many envs meet an actrange."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import binding, mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NENV = 70                 # one full wavefront and a 6-lane tail
CHECK = (0, 63, 64, 69)   # the envs that go against the oracle where not every env does
NOISE = (20.0, 0.1, 5, 0)
ROLLOUT = 60
HDR, BODY, ACT = 8, 32, 16  # doubles per tape record (tests/test_lane_env_params.py)
GAIN, BIAS, DYNTAU, ACTLO, ACTHI = 3, 6, 11, 12, 13  # offsets inside a LeTapeAct record
PLAIN, OVERLAY, HWSIM, XFRC, OVERLAY_XFRC = range(5)


def model_a_xml(integrator="Euler", limit=False):
    """ARM of tests/test_activation_states.py without joint limits and without its <size> capacities -- contacts are disabled by flag instead, the
    loader's default capacities are not zero --: no constraint rows, 3 dofs, 5 actuators, na = 4.  A stateless motor shares j1 with a
    filter; <intvelocity> has actrange and forcerange; an integrator with affine gain and bias and a tight actrange; a <cylinder>; actuatorfrc sensors
    on stateful actuators."""
    from test_activation_states import ARM
    xml = ARM.format(integrator=integrator, solver="Newton", cone="pyramidal", ncon=0, njmax=0, floor="", puck="")
    xml = re.sub(r"\s*<size [^>]*/>", "", xml)
    xml = xml.replace('tolerance="1e-10"/>', 'tolerance="1e-10"><flag contact="disable"/></option>')
    if not limit:
        xml = re.sub(r' limited="true" range="[^"]*"', "", xml)
    return xml


def model_a(energy=False, **kw):
    m = mjcf.compile_xml_string(model_a_xml(**kw))
    if energy:
        m["enableflags"] = int(m["enableflags"]) | 2  # mjENBL_ENERGY
    return m


def model_b_xml():
    """Two 3-link trees (two_arm_xml of tests/test_gpu_lane_env.py) with one actuator of each kind, the stateful ones listed first: the slots of act
    run ahead of the actuator order of the stateless ones, and a stateless motor comes last."""
    from test_gpu_lane_env import two_arm_xml
    xml = two_arm_xml(3)
    act = ('<intvelocity name="iv" joint="Lj0" kp="30" actrange="-0.5 0.4" ctrllimited="true" ctrlrange="-2 2"/>'
           '<general name="flt" joint="Rj1" dyntype="filter" dynprm="0.05" gainprm="4" biastype="affine" biasprm="0 -2 -0.1"/>'
           '<cylinder name="cyl" joint="Lj2" timeconst="0.08" area="0.6" bias="0.02 -1 -0.05"/>'
           '<general name="int" joint="Rj0" dyntype="integrator" gainprm="5" actlimited="true" actrange="-0.05 0.04" forcelimited="true" forcerange="-0.15 0.15"/>'
           '<motor name="m0" joint="Lj1" gear="1.5" ctrllimited="true" ctrlrange="-3 3"/>'
           '<position name="p0" joint="Rj2" kp="8" ctrllimited="true" ctrlrange="-1 1"/>'
           '<motor name="m1" joint="Rj0"/>')
    xml = re.sub(r"<actuator>.*</actuator>", "<actuator>" + act + "</actuator>", xml)
    return xml.replace("<sensor>", '<sensor><actuatorfrc actuator="int"/><actuatorfrc actuator="cyl"/><actuatorfrc actuator="m0"/>')


def model_b(energy=False):
    m = mjcf.compile_xml_string(model_b_xml())
    if energy:
        m["enableflags"] = int(m["enableflags"]) | 2
    return m


MODELS = {"A": model_a, "B": model_b}
SEEDS = {"A": 3, "B": 4}


def states(which, model, nenv=NENV, seed=None):
    """qpos, qvel, ctrl (beyond every ctrlrange; every third env commands its integrators a thousand times more gently: its act stays clear of the
    actranges over a rollout under this ctrl, most other envs' act runs into them), act (anywhere inside the actranges)."""
    rng = np.random.default_rng(SEEDS[which] if seed is None else seed)
    if which == "A":
        qpos = np.tile(np.asarray(model["qpos0"], float), (nenv, 1)) + rng.uniform(-0.3, 0.3, (nenv, 3)) * np.array([1, 1, 0.1])
        qvel = rng.uniform(-0.5, 0.5, (nenv, model["nv"]))
        ctrl = rng.uniform(-2.5, 2.5, (nenv, model["nu"]))
    else:
        qpos = rng.uniform(-0.8, 0.8, (nenv, model["nq"]))
        qvel = rng.uniform(-1, 1, (nenv, model["nv"]))
        ctrl = rng.uniform(-3.5, 3.5, (nenv, model["nu"]))
    lim = np.asarray(model["actuator_actlimited"]) != 0
    rngs = np.asarray(model["actuator_actrange"], float).reshape(-1, 2)
    act = rng.uniform(-0.02, 0.02, (nenv, model["na"]))
    for i in np.flatnonzero(lim):
        act[:, int(model["actuator_actadr"][i])] = rng.uniform(0.8 * rngs[i, 0], 0.8 * rngs[i, 1], nenv)
    for i in np.flatnonzero(np.asarray(model["actuator_dyntype"]) == 1):
        ctrl[::3, i] *= 1e-3
    return qpos, qvel, ctrl, act


def oracle_env(po, model, qpos, qvel, ctrl, act, K, noise=None, env=0, xfrc=None, watch=None):
    """K oracle steps of one env; watch(d) after every step."""
    d = po.OracleData(model)
    d.reset()
    d.qpos[:] = qpos
    d.qvel[:] = qvel
    if ctrl is not None:
        d.ctrl[:] = ctrl
    d.act[:] = act
    if xfrc is not None:
        d.xfrc_applied[:] = xfrc
    for k in range(K):
        if noise:
            d.ctrl_noise(noise[0], noise[1], noise[2], noise[3] + env, k)
        d.step()
        if watch:
            watch(d)
    return d


@functools.lru_cache(maxsize=None)
def reference_rollout(which, noisy):
    """The oracle over ROLLOUT steps, every env, under the drawn ctrl or (noisy) under the ctrl-noise injector, which replaces ctrl: the final state of
    each env, and whether its act met an actrange bound on the way.  Computed once per process and shared (callers do not write into it)."""
    from oracle import pyoracle as po
    po.build()
    model = MODELS[which](energy=True)
    qpos, qvel, ctrl, act = states(which, model)
    lim = [i for i in range(model["nu"]) if model["actuator_actlimited"][i]]
    adr = [int(model["actuator_actadr"][i]) for i in lim]
    rngs = np.asarray(model["actuator_actrange"], float).reshape(-1, 2)[lim]
    out, hit = [], np.zeros(NENV, dtype=bool)
    for e in range(NENV):
        met = [False]

        def watch(d):
            a = np.asarray(d.act)[adr]
            met[0] = met[0] or bool(np.any(a == rngs[:, 0]) or np.any(a == rngs[:, 1]))
        d = oracle_env(po, model, qpos[e], qvel[e], None if noisy else ctrl[e], act[e], ROLLOUT, NOISE if noisy else None, e, watch=watch)
        hit[e] = met[0]
        out.append({f: np.array(d.field(f)) for f in ("qpos", "qvel", "qacc", "act", "sensordata")})
    return out, hit


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
    a, b = model_a(), model_b()
    assert (a["nv"], a["nu"], a["na"]) == (3, 5, 4)
    assert list(a["actuator_dyntype"]) == [0, 2, 1, 1, 2] and list(a["actuator_actadr"]) == [-1, 0, 1, 2, 3]
    assert a["actuator_trnid"][0][0] == a["actuator_trnid"][1][0]   # the stateless motor shares j1 with the filter
    assert not np.any(a["jnt_limited"]) and a["nconmax"] <= 0 and a["nefcmax"] <= 0
    assert [int(a["sensor_type"][i]) for i in range(2)] == [14, 14] and [int(a["sensor_objid"][i]) for i in range(2)] == [1, 2]
    assert (b["nv"], b["nu"], b["na"]) == (6, 7, 4) and int(b["body_rootid"][1]) == 1
    assert list(b["actuator_dyntype"]) == [1, 2, 2, 1, 0, 0, 0] and list(b["actuator_actadr"]) == [0, 1, 2, 3, -1, -1, -1]
    assert list(b["actuator_actlimited"]) == [1, 0, 0, 1, 0, 0, 0]


def test_which_models_the_kernel_takes(engine):
    assert classify(engine, model_a()) == -2                      # eligible: built by hiprtc at the first eligible launch
    assert classify(engine, model_b()) == -2
    assert classify(engine, model_a(integrator="RK4")) == -1
    assert classify(engine, model_a(limit=True)) == -1            # a joint limit: constraint rows
    assert classify(engine, mjcf.load_asset("franka_like")) == 0  # the compiled-in topologies, NA = 0, as before
    assert classify(engine, mjcf.load_asset("lane_env_tree")) == 1
    # the generator's eligible() agrees
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_lane_env_topo as gen
    assert gen.eligible(model_a()) is None and gen.eligible(model_b()) is None
    assert gen.eligible(model_a(integrator="RK4")) == "integrator"
    assert gen.smooth_eligible(model_a()) is not None             # the split step keeps refusing activations
    bad = model_a()
    bad["actuator_dyntype"] = np.array([0, 2, 3, 1, 2], dtype=np.asarray(bad["actuator_dyntype"]).dtype)  # (muscle: not a dyntype the kernel runs)
    assert gen.eligible(bad) is not None
    text = gen.emit("a", model_a())
    assert "NA = 4;" in text and "act_dyntype[5] = { 0, 2, 1, 1, 2 }" in text and "act_actadr[5] = { -1, 0, 1, 2, 3 }" in text
    assert "act_actlimited[5] = { 0, 0, 1, 1, 0 }" in text
    franka = gen.emit("f", mjcf.load_asset("franka_like"))
    assert "NA = 0;" in franka and "act_actadr[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }" in franka


def test_plan_runs_one_wavefront_and_no_hwsim_build(engine):
    lib = binding.load_library()
    cm = engine.CompiledModel(model_a())
    for build in (PLAIN, OVERLAY, XFRC, OVERLAY_XFRC):
        for form in (-1, 0, 1, 2, 3):
            for nenv in (70, 4096, 16385, 65536):
                got = plan(lib, cm.ptr, nenv, build=build, form=form)
                assert got is not None and got[0] == 0 and got[1] == 0, (build, form, nenv, got)
    for form in (-1, 0, 3):
        assert plan(lib, cm.ptr, 4096, build=HWSIM, form=form) is None
    cm.close()
    # a model without activation states: the plan of tests/test_lane_env_plan.py, sampled
    fr = engine.CompiledModel(mjcf.load_asset("franka_like"))
    assert plan(lib, fr.ptr, 64) == (3, 4, 160)
    assert plan(lib, fr.ptr, 16385) == (1, 0, 80)
    assert plan(lib, fr.ptr, 32769) == (0, 0, 40)
    assert plan(lib, fr.ptr, 16385, kb=160) == (3, 3, 160)
    assert plan(lib, fr.ptr, 4096, build=HWSIM, form=3) == (0, 0, 160)
    assert plan(lib, fr.ptr, 4096, build=XFRC) == (0, 0, 160)
    fr.close()
    # ... and a hiprtc-built one without them keeps its forms
    from test_gpu_lane_env import two_arm_xml
    two = engine.CompiledModel(mjcf.compile_xml_string(two_arm_xml(3)))
    assert plan(lib, two.ptr, 64)[0] == 3 and plan(lib, two.ptr, 4096, build=HWSIM) is not None
    two.close()


@pytest.mark.parametrize("which", ["A", "B"])
def test_tape_carries_filter_constant_and_actrange(engine, which):
    """LeTapeAct stays 16 doubles with gear .. forcehi where they were; slot 11: max(mjMINVAL, dynprm[0]) of a filter (the value itself, act_dot
    divides by it), slots 12 / 13: actrange.  All three zero for a stateless actuator, slot 11 zero for an integrator."""
    m = MODELS[which]()
    cm = engine.CompiledModel(m)
    tape = cm.lane_env_tape()
    nb, nu = int(m["nbody"]), int(m["nu"])
    assert tape is not None and tape.size == HDR + BODY * nb + ACT * nu
    seen = set()
    for i in range(nu):
        r = tape[HDR + BODY * nb + ACT * i:HDR + BODY * nb + ACT * (i + 1)]
        dyn = int(m["actuator_dyntype"][i])
        seen.add(dyn)
        assert r[0] == m["actuator_gear"][i][0]
        assert np.array_equal(r[1:3], np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2)[i])
        assert np.array_equal(r[GAIN:GAIN + 3], np.asarray(m["actuator_gainprm"], float).reshape(nu, -1)[i, :3])
        assert np.array_equal(r[BIAS:BIAS + 3], np.asarray(m["actuator_biasprm"], float).reshape(nu, -1)[i, :3])
        assert np.array_equal(r[9:11], np.asarray(m["actuator_forcerange"], float).reshape(-1, 2)[i])
        tau = float(np.asarray(m["actuator_dynprm"], float).reshape(nu, -1)[i, 0])
        assert r[DYNTAU] == (max(1e-15, tau) if dyn == 2 else 0.0), i
        want = np.asarray(m["actuator_actrange"], float).reshape(-1, 2)[i] if dyn else np.zeros(2)
        assert np.array_equal(r[ACTLO:ACTHI + 1], want), i
        assert np.all(r[14:] == 0)
    assert seen == {0, 1, 2}
    cm.close()
    # a vanishing time constant is stored as mjMINVAL
    z = MODELS[which]()
    z["actuator_dynprm"] = np.zeros_like(np.asarray(z["actuator_dynprm"], float))
    cz = engine.CompiledModel(z)
    tz = cz.lane_env_tape()
    flt = [i for i in range(nu) if int(z["actuator_dyntype"][i]) == 2]
    assert flt and all(tz[HDR + BODY * nb + ACT * i + DYNTAU] == 1e-15 for i in flt)
    cz.close()


@pytest.mark.parametrize("which", ["A", "B"])
def test_states_meet_the_actrange_in_some_envs_only(oracle_built, which):
    """In the oracle alone: over the rollout under the drawn ctrl at least 8 of the 70 envs meet an actrange bound and at least 8 never do; ctrl is drawn
    beyond the ctrlranges; the drawn act lies inside the actranges.  (Under the ctrl-noise injector at std 20 every env's tight integrator is at a bound
    within a few steps: that rollout exercises the clamp in all 70.)"""
    model = MODELS[which]()
    qpos, qvel, ctrl, act = states(which, model)
    cr = np.asarray(model["actuator_ctrlrange"], float).reshape(-1, 2)
    for i in range(model["nu"]):
        if model["actuator_ctrllimited"][i]:
            assert np.sum((ctrl[:, i] < cr[i, 0]) | (ctrl[:, i] > cr[i, 1])) >= 4, i
        if model["actuator_actlimited"][i]:
            a = act[:, int(model["actuator_actadr"][i])]
            lo, hi = np.asarray(model["actuator_actrange"], float).reshape(-1, 2)[i]
            assert np.all((a > lo) & (a < hi))
    ref, hit = reference_rollout(which, False)
    print(f"model {which}: {int(hit.sum())} of {NENV} envs meet an actrange bound within {ROLLOUT} steps")
    assert hit.sum() >= 8 and (~hit).sum() >= 8
    assert all(np.all(np.isfinite(r["qpos"])) for r in ref)
    noisy, hitn = reference_rollout(which, True)
    print(f"model {which}, ctrl noise: {int(hitn.sum())} of {NENV}")
    assert hitn.sum() >= 8 and all(np.all(np.isfinite(r["qpos"])) for r in noisy)
