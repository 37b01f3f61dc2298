#!/usr/bin/env python3
"""lane_env_phase_table.py [--kernel SUBSTRING] [--all] [file.s] -- the instruction mix of the lane = env kernels between consecutive s_barriers.

Reads csrc/mjb_lane_env.s (make -C mujoco_ros_pkgs_amd/csrc mjb_lane_env.s) and prints, per kernel and per interval between two s_barriers in
program order, the counts of fp64 VALU, other VALU, ds_read, ds_write, s_load, VMEM and s_waitcnt instructions, the waits with their operands in
the order they occur.  A multi-wavefront kernel is one function whose roles follow each other (lane_env_quartet: O, X, C, V), so a role's sweep
phases are a run of consecutive rows; the row "total" counts the whole kernel and its barriers.  Without --kernel the form 3 kernels (three and
four wavefronts) are printed, with --all every kernel of the file.  Two files' tables are compared with diff.
"""
import argparse
import os
import re
import subprocess

COLS = ("fp64", "valu", "ds_rd", "ds_wr", "s_load", "vmem", "wait")


def classify(op):
    if op.startswith("v_"):
        return "fp64" if "f64" in op else "valu"
    if op.startswith(("ds_read", "ds_load")):
        return "ds_rd"
    if op.startswith(("ds_write", "ds_store")):
        return "ds_wr"
    if op.startswith(("s_load_", "s_buffer_load")):
        return "s_load"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_waitcnt":
        return "wait"
    return None


def kernels(path):
    """(mangled name, [instruction lines]) of every function of the file."""
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            body.append(t)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def table(body):
    rows, cur, waits = [], dict.fromkeys(COLS, 0), []
    cur["n"] = 0
    for t in body:
        op = t.split()[0]
        if op == "s_barrier":
            rows.append((cur, waits))
            cur, waits = dict.fromkeys(COLS, 0), []
            cur["n"] = 0
            continue
        cur["n"] += 1
        c = classify(op)
        if c:
            cur[c] += 1
        if c == "wait":
            waits.append(t[len(op):].strip().replace(" ", ""))
    rows.append((cur, waits))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("file", nargs="?", default=os.path.join(here, "..", "mujoco_ros_pkgs_amd", "csrc", "mjb_lane_env.s"))
    ap.add_argument("--kernel", default=None, help="print the kernels whose demangled name contains this text")
    ap.add_argument("--all", action="store_true", help="print every kernel of the file")
    a = ap.parse_args()
    ks = list(kernels(a.file))
    names = demangle([n for n, _ in ks])
    for n, body in ks:
        dn = names[n]
        if a.kernel is not None:
            if a.kernel not in dn:
                continue
        elif not a.all and "trio_kernel" not in dn:
            continue
        rows = table(body)
        print(f"{dn}: {len(rows) - 1} s_barrier, {sum(r['n'] for r, _ in rows)} instructions")
        print(f"  {'interval':>8s} {'instr':>6s} " + " ".join(f"{c:>6s}" for c in COLS) + "  waits")
        tot = dict.fromkeys(COLS, 0)
        for i, (r, w) in enumerate(rows):
            for c in COLS:
                tot[c] += r[c]
            runs = []  # (consecutive equal waits as one entry: "lgkmcnt(0) x3")
            for x in w:
                if runs and runs[-1][0] == x:
                    runs[-1][1] += 1
                else:
                    runs.append([x, 1])
            print(f"  {i:8d} {r['n']:6d} " + " ".join(f"{r[c]:6d}" for c in COLS) + "  " + " ".join(x if k == 1 else f"{x} x{k}" for x, k in runs))
        print(f"  {'total':>8s} {sum(r['n'] for r, _ in rows):6d} " + " ".join(f"{tot[c]:6d}" for c in COLS))
        print()


if __name__ == "__main__":
    main()
