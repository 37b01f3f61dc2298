#!/usr/bin/env python3
"""Config 2's arm with its joint limits switched on: limited="true" on the nine joints of franka_like.xml (text substitution; every joint there already
has a range, the finger springs stay) -- nine joint-limit rows under PGS.  Under the benchmark's ctrl noise, env-steps/s of (a) the generic kernels
(Batch.set_lane_env(0)), which is what such a batch ran before the lane = env kernel took limit rows and what the automatic mode still runs, (b) the
lane = env kernel (Batch.set_lane_env(1): built by hiprtc for this model, one wavefront per 64 envs), (c) for scale, plain franka_like in the lane = env
kernel's one-wavefront form.  K = 200 steps per launch (mjb_time_steps: device events around the launches), the three batches timed in turn, five
times: the median (min - max).  What the rate says depends on how often the solver runs: the share of env-steps with at least one active row and the
mean solver_iter come from a generic batch with the workload statistics on (mjb_set_stats), over the same steps.  Output kept in
profiles/lane_env_limits.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K, REPS = "franka_like", 200, 5


def limited_model():
    xml = open(os.path.join(mjcf.ASSET_DIR, NAME + ".xml")).read()
    m = mjcf.compile_xml_string(xml.replace("<joint ", '<joint limited="true" '))
    assert np.all(np.asarray(m["jnt_limited"]) != 0) and m["nefcmax"] == 9 and m["nv"] == 9
    return m


def make(model, cm, nenv, mode, std, stats=False):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(std, 0.1, 12345, 0)
    if stats:
        b.set_stats(True)
    b.step(K)  # warm-up: code objects (hiprtc's build of the limited arm's kernel among them)
    b.synchronize()
    return b


def main():
    plain, lim = mjcf.load_asset(NAME), limited_model()
    std = WORKLOADS[NAME][1]
    cms = {id(plain): engine.CompiledModel(plain), id(lim): engine.CompiledModel(lim)}
    for nenv in (4096, 65536):
        kinds = (("(a) limited arm, generic kernels    ", lim, 0), ("(b) limited arm, lane = env kernel  ", lim, 1), ("(c) franka_like, lane = env form 0  ", plain, 1))
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
                print(f"{nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                      f"lane = env used: {used}{', form ' + str(form) if used else ''})", flush=True)
        med = {}
        for k, v in rates.items():
            med[k] = float(np.median(v))
            print(f"{nenv:6d} envs {k}: median {med[k] / 1e6:.1f} ({min(v) / 1e6:.1f} - {max(v) / 1e6:.1f}) M env-steps/s over {REPS} runs", flush=True)
        print(f"{nenv:6d} envs: (b)/(a) = {med['(b)'] / med['(a)']:.2f}, (b)/(c) = {med['(b)'] / med['(c)']:.2f}, "
              f"per env-step (b) - (c) = {1e9 / med['(b)'] - 1e9 / med['(c)']:.3f} ns", flush=True)
        batches[0].set_lane_env_form(prev)
        for b in batches:
            b.close()
        # (the timed batches have no statistics: they would stand the lane = env kernel down)  how often the solver runs: a generic batch with the statistics on, from the same initial state, over the warm-up and 4 K further steps
        sb = make(lim, cms[id(lim)], nenv, 0, std, stats=True)
        sb.step(4 * K)
        st = sb.stats()
        h, n = st["nefc_hist"], st["evaluations"]
        with_rows = n - int(h[0])
        print(f"{nenv:6d} envs, generic kernels with statistics, {n} env-steps: {100.0 * with_rows / n:.2f} % with at least one active row, mean nefc {st['nefc_mean']:.3f} "
              f"(max {st['nefc_max']}), mean solver_iter {st['solver_iter_mean']:.3f} over all env-steps, "
              f"{st['solver_iter_mean'] * n / max(1, with_rows):.2f} over those with rows", flush=True)
        sb.close()


if __name__ == "__main__":
    main()
