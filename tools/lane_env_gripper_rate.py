#!/usr/bin/env python3
"""Config 2's arm with a gripper modelled the usual way (assets/gripper/franka_gripper.xml: limited="true" on the nine joints, the finger slides coupled by a
joint equality, one motor on a fixed tendon over both -- ten constraint rows under PGS, one of them in every env at every step).  Under the
benchmark's ctrl noise, env-steps/s of (a) the generic kernels (Batch.set_lane_env(0)), which is what such a batch ran before the lane = env kernel
took tendon actuators and equality rows and what the automatic mode still runs, (b) the lane = env kernel (Batch.set_lane_env(1): built by hiprtc for
this model, one wavefront per 64 envs), (c) for scale, plain franka_like in the lane = env kernel's one-wavefront form.  K = 200 steps per launch
(mjb_time_steps: device events around the launches), the three batches timed in turn, five times: the median (min - max).  What the rate says depends
on how often the solver has more than the equality row to sweep: the share of env-steps with an active limit row (nefc >= 2) and the mean solver_iter
come from a generic batch with the workload statistics on (mjb_set_stats), over the same steps.  The lines are printed and written to
profiles/lane_env_gripper.txt (--out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

PLAIN, NAME, K, REPS = "franka_like", "gripper/franka_gripper", 200, 5


def make(model, cm, nenv, mode, std, stats=False):
    qpos, qvel = initial_state(PLAIN, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(std, 0.1, 12345, 0)
    if stats:
        b.set_stats(True)
    b.step(K)  # warm-up: code objects (hiprtc's build of the gripper arm's kernel among them)
    b.synchronize()
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane_env_gripper.txt"))
    ap.add_argument("--envs", default="4096,65536")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    plain, grip = mjcf.load_asset(PLAIN), mjcf.load_asset(NAME)
    assert (grip["nv"], grip["nu"], grip["neq"], grip["ntendon"], grip["nefcmax"]) == (9, 8, 1, 1, 10)
    std = WORKLOADS[PLAIN][1]
    cms = {id(plain): engine.CompiledModel(plain), id(grip): engine.CompiledModel(grip)}
    assert cms[id(grip)].lane_env_rows() == (10, 1, 9)
    for nenv in [int(v) for v in a.envs.split(",")]:
        kinds = (("(a) gripper arm, generic kernels    ", grip, 0), ("(b) gripper arm, lane = env kernel  ", grip, 1), ("(c) franka_like, lane = env form 0  ", plain, 1))
        batches = [make(model, cms[id(model)], nenv, mode, std) for _, model, mode in kinds]
        prev = batches[0].set_lane_env_form(0)  # (process-wide; (b) runs form 0 whatever is asked for)
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(REPS):
            for (label, model, mode), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                used, form = b.lane_env_info()[1], b.lane_env_last_form()
                assert used == (mode == 1) and (not used or form == 0), (label, used, form, b.lane_env_error())
                assert np.all(np.isfinite(b.get("qpos", 0, 64)))
                r = nenv * K / (ms * 1e-3)
                rates.setdefault(label[:3], []).append(r)
                say(f"{nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                    f"lane = env used: {used}{', form ' + str(form) if used else ''})")
        med = {}
        for k, v in rates.items():
            med[k] = float(np.median(v))
            say(f"{nenv:6d} envs {k}: median {med[k] / 1e6:.1f} ({min(v) / 1e6:.1f} - {max(v) / 1e6:.1f}) M env-steps/s over {REPS} runs")
        say(f"{nenv:6d} envs: (b)/(a) = {med['(b)'] / med['(a)']:.2f}, (b)/(c) = {med['(b)'] / med['(c)']:.2f}, "
            f"per env-step (b) - (c) = {1e9 / med['(b)'] - 1e9 / med['(c)']:.3f} ns")
        batches[0].set_lane_env_form(prev)
        for b in batches:
            b.close()
        # (the timed batches have no statistics: they would stand the lane = env kernel down)  how often the solver has limit rows to sweep: a generic
        # batch with the statistics on, from the same initial state, over the warm-up and 4 K further steps
        sb = make(grip, cms[id(grip)], nenv, 0, std, stats=True)
        sb.step(4 * K)
        st = sb.stats()
        h, n = st["nefc_hist"], st["evaluations"]
        with_limit = n - int(h[0]) - int(h[1])   # (the equality row is every env-step's: nefc >= 2 means a limit row on top)
        say(f"{nenv:6d} envs, generic kernels with statistics, {n} env-steps: {100.0 * with_limit / n:.2f} % with at least one active limit row, mean nefc "
            f"{st['nefc_mean']:.3f} (max {st['nefc_max']}), mean solver_iter {st['solver_iter_mean']:.3f} over all env-steps")
        sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
