#!/usr/bin/env python3
"""Config 2's arm with gravcomp="1" on every link (a torque-controlled arm that compensates gravity inside the robot).  Env-steps/s of (a) the generic
kernel (Batch.set_lane_env(0)), (b) the lane = env kernel (built by hiprtc for this model; one wavefront per 64 envs, whatever form is asked for),
(c) for scale, plain franka_like in the lane = env kernel's one-wavefront form (Batch.set_lane_env_form(0)).  K = 200 steps per launch
(mjb_time_steps: device events around the launches), the three batches timed in turn, twice.  Output kept in profiles/lane_env_gravcomp.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K = "franka_like", 200


def gravcomp_model():
    plain = mjcf.load_asset(NAME)
    m = mjcf.with_gravcomp(plain, np.r_[0.0, np.ones(plain["nbody"] - 1)])  # (what gravcomp="1" on every <body> of the asset compiles to)
    return plain, m


def make(model, cm, nenv, mode, std):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(std, 0.1, 12345, 0)
    b.step(K)  # warm-up: code objects (hiprtc's build of the gravcomp model's kernel among them)
    b.synchronize()
    return b


def main():
    plain, gc = gravcomp_model()
    cms = {id(plain): engine.CompiledModel(plain), id(gc): engine.CompiledModel(gc)}
    std = WORKLOADS[NAME][1]
    for nenv in (4096, 65536):
        kinds = (("(a) gravcomp arm, generic kernel    ", gc, 0), ("(b) gravcomp arm, lane = env kernel ", gc, 1), ("(c) franka_like, lane = env form 0  ", plain, 1))
        batches = [make(model, cms[id(model)], nenv, mode, std) for _, model, mode in kinds]
        prev = batches[0].set_lane_env_form(0)  # (process-wide; (b) runs form 0 whatever is asked for)
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(2):
            for (label, model, mode), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                used, form = b.lane_env_info()[1], b.lane_env_last_form()
                assert used == (mode == 1) and (not used or form == 0), (label, used, form, b.lane_env_error())
                assert np.all(np.isfinite(b.get("qpos", 0, 64)))
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
