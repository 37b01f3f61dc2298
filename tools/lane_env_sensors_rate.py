#!/usr/bin/env python3
"""Config 2's arm with the sensors a real one carries: a wrist IMU (accelerometer + gyro on a site of link 7), a wrist force + torque pair, an
end-effector framelinvel, and a base force sensor on a site of the jointless base body.  Env-steps/s of (a) the generic kernel
(Batch.set_lane_env(0)), (b) the lane = env kernel (built by hiprtc for this model; one wavefront per 64 envs, whatever form is asked for) with
sensordata evaluated at the launch's last step, the default, and (b') at every step (Batch.set_sensors_every_step), (c) the same arm with the same
sites and without those sensors, built by hiprtc too, in the same one-wavefront form.  K = 200 steps per launch (mjb_time_steps: device events around
the launches), the batches timed in turn, twice.  Output kept in profiles/lane_env_sensors.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

NAME, K = "franka_like", 200
SITES = {
    '<joint name="joint7" ': '<site name="imu" pos="0.02 0.01 0.03" quat="0.9 0.1 -0.3 0.3"/><site name="ft_wrist" pos="0 0 0.05" quat="0.8 0 0.6 0"/>',
    '<body name="link1" ': '<site name="ft_base" pos="0 0 0.05"/>',   # (ahead of link1: a site of link0, the base)
}
SENSORS = ('<accelerometer site="imu"/><gyro site="imu"/><force site="ft_wrist"/><torque site="ft_wrist"/>'
           '<framelinvel objtype="site" objname="ee_site"/><force site="ft_base"/>')


def models():
    with open(os.path.join(ROOT, "mujoco_ros_pkgs_amd", "assets", NAME + ".xml")) as f:
        xml = f.read()
    for anchor, sites in SITES.items():
        assert xml.count(anchor) == 1
        xml = xml.replace(anchor, sites + anchor)
    bare = mjcf.compile_xml_string(xml)
    full = mjcf.compile_xml_string(xml.replace("</sensor>", SENSORS + "</sensor>"))
    assert full["nsensor"] == bare["nsensor"] + 6 and full["nsite"] == bare["nsite"]
    return bare, full


def sensor_arm():  # (for tools/lane_env_jit_meta.py: the registers and spills of (b)'s and (c)'s kernels)
    return models()[1]


def bare_arm():
    return models()[0]


def make(model, cm, nenv, mode, std, every):
    qpos, qvel = initial_state(NAME, model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set_lane_env(mode)
    if every:
        b.set_sensors_every_step(True)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(std, 0.1, 12345, 0)
    b.step(K)  # warm-up: code objects (hiprtc's builds among them)
    b.synchronize()
    return b


def main():
    bare, full = models()
    cms = {id(bare): engine.CompiledModel(bare), id(full): engine.CompiledModel(full)}
    std = WORKLOADS[NAME][1]
    prev = engine.binding.load_library().mjb_lane_env_set_form(0)  # (process-wide, ahead of the warm-ups; (b) runs form 0 whatever is asked for, (c) is asked to)
    for nenv in (4096, 65536):
        kinds = (("(a) arm with sensors, generic kernel            ", full, 0, False), ("(b) arm with sensors, lane = env, last step     ", full, 1, False),
                 ("(b') arm with sensors, lane = env, every step   ", full, 1, True), ("(c) arm without them, lane = env (hiprtc, form 0)", bare, 1, False))
        batches = [make(model, cms[id(model)], nenv, mode, std, every) for _, model, mode, every in kinds]
        launches = [int(min(400, max(4, 400.0 / b.time_steps(K, 2)))) for b in batches]  # a timed window of ~0.4 s each
        rates = {}
        for rep in range(2):
            for (label, model, mode, every), b, nl in zip(kinds, batches, launches):
                ms = b.time_steps(K, nl)
                (topo, used), form = b.lane_env_info(), b.lane_env_last_form()
                assert used == (mode == 1) and topo == -2 and (not used or form == 0), (label, topo, used, form, b.lane_env_error())
                assert np.all(np.isfinite(b.get("qpos", 0, 64))) and np.all(np.isfinite(b.get("sensordata", 0, 64)))
                r = nenv * K / (ms * 1e-3)
                rates.setdefault(label[:4].strip(), []).append(r)
                print(f"{nenv:6d} envs x {K} steps {label} run {rep + 1}: {r / 1e6:9.1f} M env-steps/s  ({ms:8.3f} ms per launch, {nl} launches, "
                      f"lane = env used: {used}{', form ' + str(form) if used else ''})", flush=True)
        a, bb, be, c = (float(np.mean(rates[k])) for k in ("(a)", "(b)", "(b')", "(c)"))
        print(f"{nenv:6d} envs: (b)/(a) = {bb / a:.2f}, (b)/(c) = {bb / c:.2f}, (b')/(b) = {be / bb:.2f}; per env-step (b) - (c) = {1e9 / bb - 1e9 / c:.3f} ns, "
              f"(b') - (b) = {1e9 / be - 1e9 / bb:.3f} ns", flush=True)
        for b in batches:
            b.close()
    engine.binding.load_library().mjb_lane_env_set_form(prev)


if __name__ == "__main__":
    main()
