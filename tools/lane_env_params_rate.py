#!/usr/bin/env python3
"""Config 2's model with EVERY env carrying its own gravity, body masses, joint and actuator parameters: env-steps/s of (a) the generic kernel -- what
such a batch runs in every mode but 2 --, (b) the lane = env kernel reading the per-env table (Batch.set_lane_env(2)), (c) the lane = env kernel on the
same batch without overrides (mode 1).  K = 200 steps per launch (mjb_time_steps: device events around the launches), the three batches timed in turn,
twice.  Output kept as profiles/lane_env_params.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K = "franka_like", 200
JOINT = dict(damping="dof_damping", armature="dof_armature", stiffness="jnt_stiffness", gainprm="actuator_gainprm", biasprm="actuator_biasprm")


def make(model, cm, nenv, mode, overrides):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(WORKLOADS[NAME][1], 0.1, 12345, 0)
    if overrides:
        rng = np.random.default_rng(0)
        P = {}
        for k, f in JOINT.items():
            a = np.asarray(model[f], dtype=np.float64)
            P[k] = np.tile(a[None], (nenv,) + (1,) * a.ndim) * rng.uniform(0.8, 1.2, (nenv,) + a.shape)
        scale = rng.uniform(0.8, 1.2, (nenv, model["nbody"]))
        b.set_env_gravity(np.asarray(model["gravity"], dtype=np.float64)[None] + rng.uniform(-0.5, 0.5, (nenv, 3)))
        b.set_env_body_mass(np.asarray(model["body_mass"], dtype=np.float64)[None] * scale,
                            np.asarray(model["body_inertia"], dtype=np.float64).reshape(1, -1, 3) * scale[:, :, None])
        b.set_env_dof_params(P["damping"], P["armature"], None)
        b.set_env_joint_stiffness(P["stiffness"])
        b.set_env_actuator_params(P["gainprm"], P["biasprm"])
    b.step(K)  # warm-up: code objects, the per-env table
    b.synchronize()
    return b


def main():
    model = mjcf.load_asset(NAME)
    cm = engine.CompiledModel(model)
    print(f"per-env table: {cm.lane_env_overlay().size} doubles per env")
    for nenv in (4096, 65536):
        kinds = (("(a) generic kernel, every env randomised", 0, True), ("(b) mode 2, every env randomised      ", 2, True),
                 ("(c) mode 1, no overrides               ", 1, False))
        batches = [make(model, cm, nenv, mode, ov) for _, mode, ov in kinds]
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(2):
            for (label, mode, ov), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                used, form = b.lane_env_info()[1], b.lane_env_last_form()
                assert used == (mode != 0) and np.all(np.isfinite(b.get("qpos", 0, 64)))
                r = nenv * K / (ms * 1e-3)
                rates.setdefault(label[:3], []).append(r)
                print(f"{NAME} {nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                      f"lane = env used: {used}{', form ' + str(form) if used else ''})", flush=True)
        a, bb, c = (float(np.mean(rates[k])) for k in ("(a)", "(b)", "(c)"))
        print(f"{NAME} {nenv:6d} envs: (b)/(a) = {bb / a:.2f}, (b)/(c) = {bb / c:.2f}", flush=True)
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
