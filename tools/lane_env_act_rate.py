#!/usr/bin/env python3
"""Config 2's arm under velocity commands: its seven joint motors replaced by <intvelocity> (an integrator on act behind a position servo, act clamped to
actrange) and one first-order filter actuator added on a finger -- na = 8.  Env-steps/s of (a) the generic kernel (Batch.set_lane_env(0)), which is
what such a batch ran before the lane = env kernel took activation states, (b) the lane = env kernel (built by hiprtc for this model; one wavefront
per 64 envs), (c) for scale, plain franka_like in the lane = env kernel's one-wavefront form (Batch.set_lane_env_form(0)).  K = 200 steps per launch
(mjb_time_steps: device events around the launches), the three batches timed in turn, twice.  Output kept in profiles/lane_env_act.txt."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K = "franka_like", 200
KP = (100, 100, 100, 100, 20, 20, 20)


def act_model():
    xml = open(os.path.join(mjcf.ASSET_DIR, NAME + ".xml")).read()
    for i, kp in enumerate(KP, 1):
        xml, n = re.subn(rf'<motor name="act{i}" joint="joint{i}" ctrlrange="[^"]*"/>',
                         f'<intvelocity name="act{i}" joint="joint{i}" kp="{kp}" actrange="-2.8 2.8" ctrllimited="true" ctrlrange="-2 2"/>', xml)
        assert n == 1
    xml = xml.replace("</actuator>", '<general name="flt" joint="finger_joint1" dyntype="filter" dynprm="0.05" gainprm="1" ctrllimited="true" ctrlrange="-20 20"/></actuator>')
    m = mjcf.compile_xml_string(xml)
    assert m["na"] == 8 and m["nu"] == 10
    return m


def make(model, cm, nenv, mode, std):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    if model["na"]:
        b.set("act", qpos[:, [int(model["actuator_trnid"][i][0]) for i in range(model["nu"]) if model["actuator_actadr"][i] >= 0]])  # (the servos start at rest)
    b.set_ctrl_noise(std, 0.1, 12345, 0)
    b.step(K)  # warm-up: code objects (hiprtc's build of the act model's kernel among them)
    b.synchronize()
    return b


def main():
    plain, act = mjcf.load_asset(NAME), act_model()
    cms = {id(plain): engine.CompiledModel(plain), id(act): engine.CompiledModel(act)}
    for nenv in (4096, 65536):
        kinds = (("(a) act model, generic kernel      ", act, 0, 1.0), ("(b) act model, lane = env kernel   ", act, 1, 1.0),
                 ("(c) franka_like, lane = env form 0 ", plain, 1, WORKLOADS[NAME][1]))
        batches = [make(model, cms[id(model)], nenv, mode, std) for _, model, mode, std in kinds]
        prev = batches[0].set_lane_env_form(0)  # (process-wide; (b) runs form 0 whatever is asked for)
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(2):
            for (label, model, mode, std), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                used, form = b.lane_env_info()[1], b.lane_env_last_form()
                assert used == (mode == 1) and (not used or form == 0), (label, used, form, b.lane_env_error())
                assert np.all(np.isfinite(b.get("qpos", 0, 64))) and (not model["na"] or np.all(np.isfinite(b.get("act", 0, 64))))
                r = nenv * K / (ms * 1e-3)
                rates.setdefault(label[:3], []).append(r)
                print(f"{nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                      f"lane = env used: {used}{', form ' + str(form) if used else ''})", flush=True)
        a, bb, c = (float(np.mean(rates[k])) for k in ("(a)", "(b)", "(c)"))
        print(f"{nenv:6d} envs: (b)/(a) = {bb / a:.2f}, (b)/(c) = {bb / c:.2f}, per env-step (b) - (c) = {1e9 / bb - 1e9 / c:.3f} ns", flush=True)
        batches[0].set_lane_env_form(prev)
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
