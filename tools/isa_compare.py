#!/usr/bin/env python3
"""isa_compare.py PARENT.s NEW.s [--table] -- did a source change that must not change the arithmetic change it?

For every kernel symbol present in both of hipcc's assembly listings: whether the instruction text is identical; if not, the instruction
counts, the difference of the opcode histograms restricted to mnemonics containing "f64" (the arithmetic: it has to be empty) and the
difference of all other mnemonics (scheduling, copies, waits: reported); and the kernel descriptor's vgpr_count, agpr_count,
vgpr_spill_count, sgpr_spill_count and private_segment_fixed_size on both sides.

Exit status 1 when an f64 histogram differs, or when a kernel's vgpr_spill_count or private_segment_fixed_size grew; 0 otherwise.
--table prints one line per kernel (the form profiles/ keeps) instead of the report.
"""
import collections
import re
import sys

META = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
MUST_NOT_GROW = ("vgpr_spill_count", "private_segment_fixed_size")


def kernels(path):
    """{symbol: (instruction lines, {descriptor field: value})} of the kernels of one listing"""
    txt = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - (?=\.)", txt.split("amdhsa.kernels:", 1)[-1].split("\namdhsa.", 1)[0])[1:]:  # one list item per kernel, whatever its first key
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        found = {k: re.search(r"\." + k + r":\s+(\d+)", blk) for k in META}
        missing = [k for k in META if not found[k]]
        if missing:
            sys.exit(f"{path}: kernel {name.group(1)}: no {', '.join(missing)} in its metadata")
        meta[name.group(1)] = {k: int(found[k].group(1)) for k in META}
    out = {}
    for name, fields in meta.items():
        m = re.search(r"^" + re.escape(name) + r":.*?$(.*?)^\s*\.size\s+" + re.escape(name) + r"\b", txt, re.S | re.M)
        if not m:
            continue
        ins = []
        for line in m.group(1).split("\n"):
            line = line.split(";", 1)[0].strip()
            if not line or line.startswith((".", "//")) or line.endswith(":"):
                continue
            if re.match(r"^[a-z_0-9]+$", line.split()[0]):
                ins.append(" ".join(line.split()))
        out[name] = (ins, fields)
    return out


def hist_diff(a, b, f64):
    ha = collections.Counter(i.split()[0] for i in a)
    hb = collections.Counter(i.split()[0] for i in b)
    return {op: hb[op] - ha[op] for op in sorted(set(ha) | set(hb)) if ("f64" in op) == f64 and ha[op] != hb[op]}


def compare(parent, new, table=False, out=sys.stdout):
    ka, kb = kernels(parent), kernels(new)
    common = [k for k in ka if k in kb]
    bad = 0
    same = 0
    for k in common:
        (ia, ma), (ib, mb) = ka[k], kb[k]
        ident = ia == ib
        same += ident
        d64 = {} if ident else hist_diff(ia, ib, True)
        dother = {} if ident else hist_diff(ia, ib, False)
        grew = [f for f in MUST_NOT_GROW if mb[f] > ma[f]]
        fail = bool(d64) or bool(grew)
        bad += fail
        regs = " ".join(f"{f}={ma[f]}" if ma[f] == mb[f] else f"{f}={ma[f]}->{mb[f]}" for f in META)
        if table:
            print(f"{'FAIL' if fail else 'ok  '} {'identical' if ident else 'differs (f64 same)' if not d64 else 'f64 DIFFERS'} n={len(ia)}" +
                  ("" if ident else f"->{len(ib)}") + f" {regs} {k}", file=out)
            continue
        print(f"{k}\n  {'identical instruction text' if ident else f'instructions {len(ia)} -> {len(ib)}'}\n  {regs}", file=out)
        if not ident:
            print(f"  f64 opcodes: {'same histogram' if not d64 else d64}\n  other opcodes: {dother if dother else 'same histogram'}", file=out)
        if grew:
            print(f"  GREW: {', '.join(grew)}", file=out)
    only = sorted(set(ka) ^ set(kb))
    print(f"{len(common)} kernels in both listings: {same} identical, {len(common) - same} differ, {bad} fail" +
          (f"; {len(only)} in one listing only" if only else ""), file=out)
    return 1 if bad or not common else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--table"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(compare(args[0], args[1], table="--table" in sys.argv))
