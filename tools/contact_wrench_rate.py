#!/usr/bin/env python3
"""Rate of the batched contact-wrench kernel (Batch.eval_contact_wrenches_async, csrc/mjb_contact.hip), and the cost of the only route a checkout without
it has: the nine frame fields to the host (mjb_get_many of contact_frame, contact_pos, contact_dist, contact_friction and efc_force into registered
memory, mjb_get_int of ncon, contact_geom, contact_dim and contact_efc_address), then the numpy decode of tests/contact_wrench_ref.py.

    franka_table       4096 envs   the cube against the fingers, the cube against the table
    shadow_hand_grasp  1024 envs   the five fingertips against the cube, the palm against the cube
    both after the benchmark's own rollout (bench.py: initial state, ctrl noise), from a frame in which contacts exist; all five outputs.

device: the time between two events on the batch's stream around `--launches` back-to-back evaluations, divided by their number, after a warm-up of 3;
`eval + sync` is the wall clock around one evaluation and a synchronize.  host: wall clock of the transfers (they synchronise), and of the decode over
every env; a host sample is their sum.  Five repeats each, reported as median [min .. max].  The launch is also set against the time its own bytes --
what it reads of the live contacts and what it writes -- would take at the HBM rate of bench.py's roofline block.  Exit status 1 when the worst device
sample is not shorter than the best host sample.  Needs a device."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_wrench_ref as ref
from bench import HBM_PEAK_GBS, WORKLOADS, initial_state
from mujoco_ros_pkgs_amd import binding, engine, mjcf
from tools.ray_cast_rate import REPEATS, Events, fmt, stats

OUTPUTS = ("wrench", "normal", "count", "dist", "contacts")
DOUBLE_FIELDS = ("contact_frame", "contact_pos", "contact_dist", "contact_friction", "efc_force")
INT_FIELDS = ("ncon", "contact_geom", "contact_dim", "contact_efc_address")
HAND_TIPS = ("ffdistal", "mfdistal", "rfdistal", "lfdistal", "thdistal")


def queries(name, model):
    if name == "franka_table":
        return [(["cube_geom"], engine.geoms_of_bodies(model, ["left_finger", "right_finger"])), (["cube_geom"], ["table"])]
    return [(engine.geoms_of_bodies(model, b), ["cube_geom"]) for b in HAND_TIPS] + [(engine.geoms_of_bodies(model, "palm"), ["cube_geom"])]


def rolled_out(name, nenv, warm):
    """the benchmark's workload after `warm` steps of its rollout, its last step's frame kept"""
    model = mjcf.load_asset(name)
    cm = engine.CompiledModel(model)
    b = engine.Batch(cm, nenv)
    qpos, qvel = initial_state(name, model, nenv, 1000)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set_ctrl_noise(WORKLOADS[name][1], 0.1, 12345, 0)
    done = 0
    while done < warm:
        k = min(200, warm - done)
        b.step(k)
        done += k
    b.set_keep_frame(True)
    b.step(1)
    b.synchronize()
    return model, cm, b


def wall(fn, n=1):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n   # ms per call


def host_route(b, model, qs):
    """(transfer ms, decode ms) samples, and the fields as transferred"""
    lib, n = b.lib, b.nenv
    dbl = {f: np.zeros((n, b.cm.field_size(f))) for f in DOUBLE_FIELDS}
    ints = {f: np.zeros((n, b.cm.field_size(f)), np.int32) for f in INT_FIELDS}
    for a in dbl.values():
        if lib.mjb_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes) != 0:
            raise RuntimeError("mjb_host_register failed")
    ids = (C.c_int * len(DOUBLE_FIELDS))(*[binding.Field.ids[f] for f in DOUBLE_FIELDS])
    ptrs = (C.POINTER(C.c_double) * len(DOUBLE_FIELDS))(*[dbl[f].ctypes.data_as(C.POINTER(C.c_double)) for f in DOUBLE_FIELDS])

    def pull():
        if lib.mjb_get_many(b.ptr, len(DOUBLE_FIELDS), ids, 0, n, ptrs) != 0:
            raise RuntimeError(lib.mjb_last_error().decode())
        for f in INT_FIELDS:
            if lib.mjb_get_int(b.ptr, binding.Field.ids[f], 0, n, ints[f].ctypes.data_as(C.POINTER(C.c_int))) != 0:
                raise RuntimeError(lib.mjb_last_error().decode())
    for _ in range(3):
        pull()
    pulls = [wall(pull, 10) for _ in range(REPEATS)]
    for a in dbl.values():
        lib.mjb_host_unregister(a.ctypes.data_as(C.c_void_p))
    fields = {**dbl, **ints}
    cone = int(model["cone"])
    geoms = [([model["names"]["geom"].index(g) if isinstance(g, str) else int(g) for g in A], [model["names"]["geom"].index(g) if isinstance(g, str) else int(g) for g in B]) for A, B in qs]

    def decode():
        for e in range(n):
            f = ref.env_fields(fields, e)
            ref.decode(f, cone)
            for A, B in geoms:
                ref.query(f, A, B, None, cone)
    decodes = [wall(decode) for _ in range(REPEATS)]
    return pulls, decodes, fields


def own_bytes(model, fields, nq):
    """what one launch reads of the frames -- ncon, the live contacts' records, their rows of efc_force -- and what it writes"""
    n = fields["ncon"].shape[0]
    cone, read = int(model["cone"]), 0
    for e in range(n):
        nc = int(fields["ncon"][e, 0])
        dim, adr = fields["contact_dim"][e, :nc], fields["contact_efc_address"][e, :nc]
        rows = np.where(dim == 1, 1, dim if cone == ref.ELLIPTIC else 2 * (dim - 1))[adr >= 0].sum()
        read += 4 + nc * (4 * 4 + 18 * 8) + int(rows) * 8
    written = n * (nq * (6 * 8 + 8 + 4 + 8) + int(model["nconmax"]) * 6 * 8)
    return read, written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--launches", type=int, default=100, help="back-to-back evaluations per timed window")
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("contact_wrench_rate.py: no HIP device -- nothing here can be measured without one")
    ok = True
    for name, nenv, warm in (("franka_table", 4096, 1000), ("shadow_hand_grasp", 1024, 600)):
        model, cm, b = rolled_out(name, nenv, warm)
        qs = queries(name, model)
        b.set_contact_queries(qs, outputs=OUTPUTS)
        ev = Events(b.stream)
        for _ in range(3):
            b.eval_contact_wrenches_async()
        b.synchronize()
        dev = [ev.time(b.eval_contact_wrenches_async, a.launches) for _ in range(REPEATS)]

        def eval_sync():
            b.eval_contact_wrenches_async()
            b.synchronize()
        ws = [wall(eval_sync, a.launches) for _ in range(REPEATS)]
        ev.close()
        out = b.contact_wrenches()
        pulls, decodes, fields = host_route(b, model, qs)
        host = [p + d for p, d in zip(pulls, decodes)]
        read, written = own_bytes(model, fields, len(qs))
        floor_ms = (read + written) / (HBM_PEAK_GBS * 1e9) * 1e3
        what = f"{name}, {len(qs)} queries"
        print(f"state    {what:<30s} {nenv:5d} envs after {warm + 1} steps: mean ncon {fields['ncon'].mean():.2f} (max {fields['ncon'].max()}), matching contacts per env "
              f"{out['count'].sum(axis=1).mean():.2f}, largest |force| {np.abs(out['wrench'][:, :, :3]).max():.3g}", flush=True)
        print(f"device   {what:<30s} {nenv:5d} envs, all five outputs: {fmt(dev)} per eval   {stats(dev)[0] * 1e6 / nenv:7.3f} ns per env   eval + sync {fmt(ws)}", flush=True)
        print(f"bytes    {what:<30s} {read / nenv:7.0f} read + {written / nenv:5.0f} written per env: {floor_ms * 1e3:.3f} us at {HBM_PEAK_GBS:.0f} GB/s; "
              f"the launch takes {stats(dev)[0] / floor_ms:.0f} x that", flush=True)
        print(f"host     {what:<30s} {nenv:5d} envs: transfer {fmt(pulls)}   numpy decode {fmt(decodes, 'ms', 1.0)}   sum {fmt(host, 'ms', 1.0)}", flush=True)
        good = max(dev) < min(host)
        ok &= good
        print(f"ratio    {what:<30s} host / device {stats(host)[0] / stats(dev)[0]:.0f} x (medians); transfer alone / device {stats(pulls)[0] / stats(dev)[0]:.1f} x; "
              f"worst device sample {max(dev) * 1e3:.2f} us {'<' if good else '>='} best host sample {min(host) * 1e3:.2f} us", flush=True)
        b.close()
        cm.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
