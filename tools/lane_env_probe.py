#!/usr/bin/env python3
"""lane_env_probe.py [envs] -- where a step of the lane = env kernel's multi-wavefront forms spends its cycles: run on the measurement build
(tools/lane_env_probe_build.sh -> csrc/libmjb_xprobe.so, -DMJB_LE_PROBE: s_memtime stamps around the step's phases, summed over the launch and
written over env 0's sensordata).  Per step and wavefront: [sweep root->leaf (own work), rendezvous F, waiting at the per-body barriers (+ V: the
force block), sweep leaf->root, energy / factors, rendezvous A, solves + Euler (V: waiting for them), rendezvous B].
Form 3 on four wavefronts (MJB_LANE_ENV_SWEEP_WAVES=4, or the rule): the first row is O (orientation chain), then C, V, and X (frames and
positions; its eight values lie behind V's, past the end of env 0's 25 sensor values -- in env 1's: take 2 envs or more).  Four more follow X's: a
ninth stamp per role, used by C and V (see the last line printed).
    MJB_LANE_ENV_DUO=2 MJB_LIBRARY=$PWD/mujoco_ros_pkgs_amd/csrc/libmjb_xprobe.so python tools/lane_env_probe.py 4096"""
import os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_ros_pkgs_amd import engine, mjcf
from tests.conftest import random_franka_state
model = mjcf.load_asset("franka_like")
cm = engine.CompiledModel(model)
nenv = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
qpos, qvel = random_franka_state(model, nenv, 0)
b = engine.Batch(cm, nenv)
b.set_lane_env(1)
b.set("qpos", qpos); b.set("qvel", qvel)
b.set_ctrl_noise(5.0, 0.1, 12345, 0)
b.step(1000)
b.step(1000)
lib = engine.binding.load_library()
form, waves = lib.mjb_lane_env_last_form(), lib.mjb_lane_env_last_sweep_waves()
sd = b.get("sensordata").ravel()
print("form", form, "sweep wavefronts", waves)
names = {3: ("P", "C", "V"), 4: ("O", "C", "V", "X")}.get(waves, ("P", "V"))
for k, nm in enumerate(names):
    print(nm + ":", np.round(sd[8 * k:8 * k + 8]).astype(int), int(sd[8 * k:8 * k + 8].sum()))
if waves == 4:
    # (a ninth stamp of C and V, behind the eight of X: the cycles between a sweep barrier and the point where the phase's reads have landed -- C: the pose
    #  ring's; V: cinert, cdof and qvel, with the previous body's force half under them.  The first column above is the rest of the phase.)
    print("of the sweep's own work, from the barrier to the landed reads: C", int(round(sd[32 + 2])), " V", int(round(sd[32 + 3])))
