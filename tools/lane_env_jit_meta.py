#!/usr/bin/env python3
"""lane_env_jit_meta.py -- registers, spills and scratch of the lane = env kernel's one-wavefront builds for a model hiprtc would build, compiled
offline with the options the library hands hiprtc (csrc/mjb_lane_env.hip: jit_get), and the ISA lint (tools/check_spill_exec.py) on each.
tools/kernel_meta.py covers the compiled-in topologies; this is its counterpart for any other eligible model.  Needs no GPU.

    python tools/lane_env_jit_meta.py MODEL.xml [--kb 40,80,160] [--builds plain,overlay,hwsim,xfrc,overlay_xfrc] [--keep DIR]
    python tools/lane_env_jit_meta.py tests:lane_env_sensor_models:model_S      # a model function of a module under tests/ or tools/
    python tools/lane_env_jit_meta.py "tests:lane_env_sensor_models:model_S(base_wrench=False)" --builds xfrc,overlay_xfrc
"""
import argparse
import concurrent.futures
import importlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_lane_env_topo as gen  # noqa: E402
from mujoco_ros_pkgs_amd import mjcf  # noqa: E402

CSRC = os.path.join(ROOT, "mujoco_ros_pkgs_amd", "csrc")
# the template arguments behind the budget, as le_rows (csrc/mjb_lane_env.hip) has them
BUILDS = {"plain": "", "overlay": ", 0, true", "hwsim": ", 0, false, true", "xfrc": ", 0, false, false, true", "overlay_xfrc": ", 0, true, false, true"}


def source(topo, build, kb):
    return ('#include "mjb_lane_env_kernel.h"\n' + topo +
            'extern "C" __global__ void __launch_bounds__(64) le_rt(const KernelParams MJB_AS4 *P, int nsteps, unsigned int step0, int lo, int hi)\n{\n'
            "\t__shared__ __attribute__((aligned(16))) unsigned char smem[mjb_le::Lds<LeTopo_rt, %d>::bytes()];\n"
            "\tmjb_le::lane_env_body<LeTopo_rt, %d%s>(P, nsteps, step0, lo, hi, smem);\n}\n" % (kb, kb, BUILDS[build]))


def compile_one(topo, build, kb, outdir):
    src = os.path.join(outdir, "le_%s_%d.hip" % (build, kb))
    asm = src[:-4] + ".s"
    with open(src, "w") as f:
        f.write(source(topo, build, kb))
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-mllvm", "-disable-machine-licm",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return build, kb, None, r.stderr[-3000:]
    txt = open(asm).read()
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", txt).group(1))  # noqa: E731
    lint = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_spill_exec.py"), asm], capture_output=True, text=True)
    row = (get("vgpr_count"), get("agpr_count"), get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size"))
    return build, kb, row, ("" if lint.returncode == 0 else "LINT: " + (lint.stdout + lint.stderr)[-1500:])


def load(spec):
    if spec.startswith("tests:") or spec.startswith("tools:"):
        where, mod, fn = spec.split(":")
        sys.path.insert(0, os.path.join(ROOT, where))
        expr = re.match(r"(\w+)(?:\((.*)\))?$", fn)
        f = getattr(importlib.import_module(mod), expr.group(1))
        kw = eval("dict(%s)" % (expr.group(2) or ""))  # (keyword arguments of the model function, e.g. model_S(gravcomp=True))
        return f(**kw)
    return mjcf.compile_xml_file(spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model")
    ap.add_argument("--kb", default="40,160")
    ap.add_argument("--builds", default=",".join(BUILDS))
    ap.add_argument("--keep", default=None, help="directory for the sources and the ISA (default: a temporary one)")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    m = load(a.model)
    topo = gen.rt_struct(m)
    jobs = [(b, int(k)) for b in a.builds.split(",") for k in a.kb.split(",")]
    tmp = None if a.keep else tempfile.TemporaryDirectory()
    outdir = a.keep or tmp.name
    os.makedirs(outdir, exist_ok=True)
    bad = 0
    print(f"{'lane = env, hiprtc <build, LDS KB>':36s} {'vgpr':>5s} {'agpr':>5s} {'vgpr spills':>11s} {'sgpr spills':>11s} {'private B':>9s} {'LDS B':>7s}")
    with concurrent.futures.ThreadPoolExecutor(a.j) as ex:
        for build, kb, row, msg in ex.map(lambda j: compile_one(topo, j[0], j[1], outdir), jobs):
            if row is None:
                bad += 1
                print(f"<{build}, {kb}>: compile failed\n{msg}")
                continue
            print(f"<{build}, {kb}>".ljust(36) + " %5d %5d %11d %11d %9d %7d" % row)
            if msg:
                bad += 1
                print(msg)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
