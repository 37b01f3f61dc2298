#!/usr/bin/env python3
"""What ending and restarting episodes costs a training loop: franka_like at 4096 and 65 536 envs, launches of K fused steps, about 1 % of the envs
reaching their time limit per launch (each env starts at a staggered `time`, and a reset puts it back to 0, so the share is steady).

    (a) device   Batch.episode_step between the launches (csrc/mjb_episode.hip): the done rule, the reset to a bank row with seeded noise, no host
    (b) host     the only route of a checkout without it: get("time"), a host mask, reset(mask), then get / set of qpos and qvel to start the reset
                 envs from the same bank rows
    (c) none     no resets at all: the ceiling

The three loops run alternating in one process on three batches of the same state, after a warm-up; a window is at least `--window` seconds of wall
clock and ends in a synchronise; `--repeats` windows each, reported as median [min .. max] env-steps per second.  The episode kernel's own time
(its launch and the clearing of ndone ahead of it) is the time between two events on the batch's stream around one episode_step behind a step
launch, over `--kernel-samples` launches.  Needs a device."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_ros_pkgs_amd import engine, mjcf
from tools.ray_cast_rate import Events, fmt, stats

NINIT = 16
SHARE = 0.01


def bank_and_state(model, nenv, seed=1000):
    """(bank qpos [NINIT, nq], bank qvel [NINIT, nv], qpos [nenv, nq], qvel [nenv, nv]): inside the joint ranges' middle"""
    rng = np.random.default_rng(seed)

    def poses(n):
        qpos = np.tile(np.asarray(model["qpos0"], float), (n, 1))
        for j in range(int(model["njnt"])):
            lo, hi = (float(x) for x in model["jnt_range"][j]) if int(model["jnt_limited"][j]) else (-0.5, 0.5)
            qpos[:, int(model["jnt_qposadr"][j])] = rng.uniform(0.6 * lo + 0.4 * hi, 0.4 * lo + 0.6 * hi, n)
        return qpos, rng.uniform(-0.5, 0.5, (n, int(model["nv"])))
    return poses(NINIT) + poses(nenv)


class Loop:
    def __init__(self, kind, cm, model, nenv, K, state):
        self.kind, self.K, self.nenv = kind, K, nenv
        self.bq, self.bv, qpos, qvel = state
        dt = float(model["timestep"][0])
        self.limit = K * dt / SHARE   # an episode lasts 1 / SHARE launches
        self.b = b = engine.Batch(cm, nenv)
        b.set("qpos", qpos)
        b.set("qvel", qvel)
        b.set("time", (np.random.default_rng(7).uniform(0, self.limit, nenv))[:, None])
        self.rng = np.random.default_rng(11)
        self.resets = 0
        if kind == "device":
            b.set_episode_init(self.bq, self.bv)
            b.set_episode_noise(2024, qpos_range=(-0.02, 0.02), qvel_range=(-0.1, 0.1), clamp=True)
            b.set_episode_rule(time_limit=self.limit)

    def launch(self):
        b = self.b
        b.step(self.K)
        if self.kind == "device":
            b.episode_step()
        elif self.kind == "host":
            mask = b.get("time")[:, 0] >= self.limit
            b.reset(mask.astype(np.uint8))
            n = int(mask.sum())
            self.resets += n
            rows = self.rng.integers(0, NINIT, n)
            q, v = b.get("qpos"), b.get("qvel")
            q[mask] = self.bq[rows] + self.rng.uniform(-0.02, 0.02, (n, q.shape[1]))
            v[mask] = self.bv[rows] + self.rng.uniform(-0.1, 0.1, (n, v.shape[1]))
            b.set("qpos", q)
            b.set("qvel", v)

    def window(self, launches):
        """env-steps per second over `launches` launches, the synchronise included"""
        self.b.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        self.b.synchronize()
        return self.nenv * self.K * launches / (time.perf_counter() - t0)


def kernel_time(loop, samples):
    """ms of one episode_step behind a step launch (device events), and the share of the envs it found done"""
    b, ev = loop.b, Events(loop.b.stream)
    ms, done = [], []
    for _ in range(samples):
        b.step(loop.K)
        ms.append(ev.time(b.episode_step, 1))
        done.append(b.episode_ndone())
    ev.close()
    return ms, float(np.mean(done)) / loop.nenv


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="K: fused steps per launch")
    ap.add_argument("--window", type=float, default=1.2, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-samples", type=int, default=200)
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 65536])
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("episode_reset_rate.py: no HIP device -- nothing here can be measured without one")
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    K = a.steps
    for nenv in a.envs:
        state = bank_and_state(model, nenv)
        loops = [Loop(kind, cm, model, nenv, K, state) for kind in ("device", "host", "none")]
        launches = {}
        for lp in loops:   # warm-up, and the launches a window needs
            lp.window(20)
            rate = lp.window(20)
            launches[lp.kind] = max(20, int(np.ceil(a.window * rate / (nenv * K))))
        rates = {lp.kind: [] for lp in loops}
        for _ in range(a.repeats):
            for lp in loops:
                rates[lp.kind].append(lp.window(launches[lp.kind]))
        for lp in loops:
            r = np.asarray(rates[lp.kind])
            med = stats(r)[0]
            print(f"loop ({'abc'['device host none'.split().index(lp.kind)]}) {lp.kind:<7s} franka_like {nenv:6d} envs, K = {K}: {fmt(r, 'M env-steps/s', 1e-6)}   "
                  f"{nenv * K / med * 1e6:9.1f} us per launch, {launches[lp.kind]} launches per window", flush=True)
        dev, host, none = (stats(rates[k])[0] for k in ("device", "host", "none"))
        ms, share = kernel_time(loops[0], a.kernel_samples)
        print(f"episode kernel     franka_like {nenv:6d} envs: {fmt(ms)} per episode_step (events on the stream), {100 * share:.2f} % of the envs done per launch", flush=True)
        print(f"ratios             franka_like {nenv:6d} envs: device / host {dev / host:.2f} x, device / none {dev / none:.3f}, host / none {host / none:.3f} (medians); "
              f"host loop reset {loops[1].resets} envs, device loop {int(loops[0].b.episode_counts().sum())}", flush=True)
        for lp in loops:
            lp.b.close()
    cm.close()


if __name__ == "__main__":
    main()
