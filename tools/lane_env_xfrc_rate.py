#!/usr/bin/env python3
"""Config 2's model with a Cartesian wrench on every body of every env (xfrc_applied: f ~ U(-5, 5) N, t ~ U(-1, 1) N m, each env its own):
env-steps/s of (a) the generic kernel, which is what such a batch runs without the opt-in, (b) the lane = env kernel's XF build
(Batch.set_lane_env_xfrc), (c) the lane = env kernel's one-wavefront form on the same batch without a wrench (Batch.set_lane_env_form(0)).
K = 200 steps per launch (mjb_time_steps: device events around the launches), the three batches timed in turn, twice.  (b) - (c) is what the
wrenches cost on this kernel.  Output kept in profiles/lane_env_xfrc.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K = "franka_like", 200


def make(model, cm, nenv, wrench, switch):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(1)
    b.set_lane_env_xfrc(switch)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(WORKLOADS[NAME][1], 0.1, 12345, 0)
    if wrench:
        rng = np.random.default_rng(7)
        nb = int(model["nbody"])
        b.set("xfrc_applied", np.concatenate([rng.uniform(-5, 5, (nenv, nb, 3)), rng.uniform(-1, 1, (nenv, nb, 3))], axis=2).reshape(nenv, 6 * nb))
    b.step(K)  # warm-up: code objects, the wrench table
    b.synchronize()
    return b


def main():
    model = mjcf.load_asset(NAME)
    cm = engine.CompiledModel(model)
    for nenv in (4096, 65536):
        kinds = (("(a) wrenches, generic kernel       ", True, False), ("(b) wrenches, lane = env XF build  ", True, True),
                 ("(c) no wrench, lane = env form 0   ", False, False))
        batches = [make(model, cm, nenv, wrench, switch) for _, wrench, switch in kinds]
        prev = batches[0].set_lane_env_form(0)  # (process-wide; (b) runs form 0 whatever is asked for)
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(2):
            for (label, wrench, switch), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                used, form = b.lane_env_info()[1], b.lane_env_last_form()
                assert used == (switch or not wrench) and (not used or form == 0) and np.all(np.isfinite(b.get("qpos", 0, 64)))
                r = nenv * K / (ms * 1e-3)
                rates.setdefault(label[:3], []).append(r)
                print(f"{NAME} {nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                      f"lane = env used: {used}{', form ' + str(form) if used else ''})", flush=True)
        a, bb, c = (float(np.mean(rates[k])) for k in ("(a)", "(b)", "(c)"))
        print(f"{NAME} {nenv:6d} envs: (b)/(a) = {bb / a:.2f}, (b)/(c) = {bb / c:.2f}, per env-step (b) - (c) = {1e9 / bb - 1e9 / c:.3f} ns", flush=True)
        batches[0].set_lane_env_form(prev)
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
