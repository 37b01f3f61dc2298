#!/usr/bin/env python3
"""Rate of the batched ray kernel (Batch.cast_rays_async, csrc/mjb_ray.hip) on franka_table, and the cost per ray of the only alternative the engine
has: one <site> + <rangefinder> per ray, evaluated by one lane inside mjb_forward.

    cast      a 64 x 48 pinhole image on ee_site at 4096 envs; a 36-ray ring at 4096 and 65 536 envs
    sensors   franka_table with 36 ring sites + rangefinders on the hand: mjb_forward with the sensors minus mjb_forward with sensor="disable",
              4096 envs, the two alternating in one process (--sensor-path-only: this part alone -- it needs nothing the ray interface adds, so
              the same file measures a checkout that lacks it)

Every figure is the time between two events on the batch's stream around `--launches` back-to-back launches, divided by their number, after a warm-up;
five repeats, reported as median [min .. max].  Launches of a few microseconds are bound by the launch path, not the kernel: the figures say what a
caller pays per cast.  Needs a device."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import initial_state
from mujoco_ros_pkgs_amd import engine, mjcf

REPEATS = 5
RING = 36


class Events:
    """Two timing events on a stream (the HIP runtime libmjb.so already loaded)."""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            self._ok(self.hip.hipEventCreate(C.byref(e)))

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def time(self, fn, n):
        """Milliseconds per call of fn over n back-to-back calls."""
        self._ok(self.hip.hipEventRecord(self.e[0], self.stream))
        for _ in range(n):
            fn()
        self._ok(self.hip.hipEventRecord(self.e[1], self.stream))
        self._ok(self.hip.hipEventSynchronize(self.e[1]))
        ms = C.c_float(0)
        self._ok(self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]))
        return ms.value / n

    def close(self):
        for e in self.e:
            self.hip.hipEventDestroy(e)


def stats(v):
    v = np.asarray(v, float)
    return float(np.median(v)), float(v.min()), float(v.max())


def fmt(v, unit="us", scale=1e3, digits=2):
    med, lo, hi = stats(v)
    return f"{med * scale:9.{digits}f} {unit} [{lo * scale:.{digits}f} .. {hi * scale:.{digits}f}]"


def make_batch(model, nenv):
    cm = engine.CompiledModel(model)
    qpos, qvel = initial_state("franka_table", model, nenv, seed=1000)
    b = engine.Batch(cm, nenv)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    return cm, b


def geom_tests_per_env(model, site, exclude=True, visible=None):
    """ray_geom calls of one env's rays: per ray, the geoms that pass the mask (default: alpha != 0) and do not sit on the ray's own body."""
    visible = np.asarray(model["geom_rgba"], float).reshape(-1, 4)[:, 3] != 0 if visible is None else np.asarray(visible) != 0
    gb = np.asarray(model["geom_bodyid"], int)
    n = 0
    for s in np.atleast_1d(site):
        own = int(model["site_bodyid"][s]) if (s >= 0 and exclude) else -1
        n += int((visible & (gb != own)).sum())
    return n


def cast_case(what, nenv, vec, launches):
    model = mjcf.load_asset("franka_table")
    cm, b = make_batch(model, nenv)
    site = model["names"]["site"].index("ee_site")
    b.set_rays(site, vec)
    b.forward()
    ev = Events(b.stream)
    for _ in range(3):
        b.cast_rays_async()
    b.synchronize()
    ms = [ev.time(b.cast_rays_async, launches) for _ in range(REPEATS)]
    dist, gid = b.cast_rays()
    ev.close()
    nray = len(vec)
    tests = geom_tests_per_env(model, [site] * nray) * nenv
    med = stats(ms)[0] * 1e-3
    print(f"cast     {what:<22s} {nenv:6d} envs x {nray:5d} rays, {int(model['ngeom'])} geoms: {fmt(ms)} per cast   {nenv * nray / med / 1e9:8.3f} G rays/s   "
          f"{tests / med / 1e9:8.2f} G ray-geom tests/s   {med * 1e9 / (nenv * nray):8.4f} ns per ray   (hits: {(gid >= 0).mean() * 100:.0f} %)", flush=True)
    b.close()
    cm.close()
    return np.array(ms) * 1e6 / (nenv * nray)   # ns per ray, per repeat


def ring_sensor_xml():
    """franka_table with 36 sites on the hand, their z axes a ring in ee_site's x-y plane, and one rangefinder on each."""
    with open(os.path.join(mjcf.ASSET_DIR, "franka_table.xml")) as f:
        xml = f.read()
    v = engine.lidar_rays(RING) if hasattr(engine, "lidar_rays") else np.stack([np.cos(np.arange(RING) * 2 * np.pi / RING), np.sin(np.arange(RING) * 2 * np.pi / RING), np.zeros(RING)], 1)
    sites = "".join(f'\n                      <site name="ring{k}" pos="0 0 0.1034" zaxis="{float(v[k, 0])!r} {float(v[k, 1])!r} {float(v[k, 2])!r}"/>' for k in range(RING))
    sensors = "".join(f'\n    <rangefinder name="ring{k}" site="ring{k}"/>' for k in range(RING))
    xml, n1 = re.subn(r'(<site name="ee_site"[^>]*/>)', lambda mm: mm.group(1) + sites, xml, count=1)
    xml, n2 = re.subn(r"(<sensor>)", lambda mm: mm.group(1) + sensors, xml, count=1)
    assert n1 == 1 and n2 == 1
    return xml


def sensor_path(nenv, launches):
    xml = ring_sensor_xml()
    variants = {"36 rangefinders": mjcf.compile_xml_string(xml), 'sensor="disable"': mjcf.compile_xml_string(xml, disable=("sensor",)),
                "the asset as shipped": mjcf.load_asset("franka_table")}
    assert int(variants["36 rangefinders"]["nsensor"]) == int(variants["the asset as shipped"]["nsensor"]) + RING
    held = {k: make_batch(m, nenv) for k, m in variants.items()}
    evs = {k: Events(b.stream) for k, (_, b) in held.items()}
    for _, b in held.values():
        for _ in range(3):
            b.forward()
        b.synchronize()
    ms = {k: [] for k in held}
    for _ in range(REPEATS):   # (alternating: a drift of the machine lands on all three)
        for k, (_, b) in held.items():
            ms[k].append(evs[k].time(b.forward, launches))
    sd = held["36 rangefinders"][1].get("sensordata")
    for k in held:
        print(f"sensors  mjb_forward, {k:<22s} {nenv:6d} envs: {fmt(ms[k])} per launch", flush=True)
    rays = nenv * RING
    out = {}
    for name, base in (('minus sensor="disable"', 'sensor="disable"'), ("minus the asset as shipped", "the asset as shipped")):
        d = (np.array(ms["36 rangefinders"]) - np.array(ms[base])) * 1e6 / rays
        out[name] = d
        print(f"sensors  36 rangefinders {name:<28s}: {fmt(d, 'ns per ray', 1.0, 4)}", flush=True)
    adr = [int(variants["36 rangefinders"]["sensor_adr"][variants["36 rangefinders"]["names"]["sensor"].index(f"ring{k}")]) for k in range(RING)]
    print(f"sensors  (rangefinder readings that hit something: {(sd[:, adr] >= 0).mean() * 100:.0f} %)", flush=True)
    for k, (cm, b) in held.items():
        evs[k].close()
        b.close()
        cm.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sensor-path-only", action="store_true")
    ap.add_argument("--launches", type=int, default=200, help="back-to-back launches per timed window")
    ap.add_argument("--parent-ns-per-ray", type=float, nargs=3, metavar=("MEDIAN", "MIN", "MAX"), help="the sensor path's cost per ray measured on the parent commit (this tool, --sensor-path-only)")
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("ray_cast_rate.py: no HIP device -- nothing here can be measured without one")
    sens = sensor_path(4096, max(1, a.launches // 4))
    if a.sensor_path_only:
        return
    pin, _ = engine.pinhole_rays(64, 48, 45.0)
    ring = engine.lidar_rays(RING)
    cast_case("64 x 48 pinhole image", 4096, pin, max(1, a.launches // 10))
    r4k = cast_case("36-ray ring", 4096, ring, a.launches)
    cast_case("36-ray ring", 65536, ring, max(1, a.launches // 4))
    new = stats(r4k)
    ref = stats(sens['minus sensor="disable"']) if a.parent_ns_per_ray is None else tuple(a.parent_ns_per_ray)
    where = "this build" if a.parent_ns_per_ray is None else "the parent commit"
    spread = (new[2] - new[1]) / 2 + (ref[2] - ref[1]) / 2
    print(f'verdict  36-ray ring at 4096 envs: {new[0]:.4f} ns per ray [{new[1]:.4f} .. {new[2]:.4f}] against {ref[0]:.4f} [{ref[1]:.4f} .. {ref[2]:.4f}] of the rangefinder path ({where}); '
          f"run-to-run spread {spread:.4f}: {'not above' if new[0] <= ref[0] + spread else 'ABOVE'} the existing path, {ref[0] / new[0]:.1f} x", flush=True)
    if new[0] > ref[0] + spread:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
