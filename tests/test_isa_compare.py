"""tools/isa_compare.py on two short synthetic listings: the same instructions in another order pass, one v_fma_f64 turned into
v_mul_f64 + v_add_f64 fails (the arithmetic of a kernel is its f64 opcode histogram), and so does a kernel that starts to spill.  No device."""
import importlib.util
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
isa_compare = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_compare)

BODY = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_mul_f64 v[0:1], v[2:3], v[4:5]", "v_fma_f64 v[6:7], v[0:1], v[2:3], v[4:5]",
        "ds_write_b64 v8, v[6:7]", "v_accvgpr_write_b32 a0, v6", "s_endpgm"]


def listing(body, vgpr=12, spill=0, private=0, name="_Z6kernelPd"):
    ins = "\n".join("\t" + i + "\t; a comment" for i in body)
    return f"""\t.text
\t.globl\t{name}
{name}:                            ; @{name}
; %bb.0:
{ins}
.Lfunc_end0:
\t.size\t{name}, .Lfunc_end0-{name}
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     1
    .args:
      - .offset:         0
        .size:           8
    .name:           {name}
    .private_segment_fixed_size: {private}
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         {name}.kd
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: {spill}
amdhsa.version:
  - 1
...
\t.end_amdgpu_metadata
"""


def run(tmp_path, a, b):
    pa, pb = tmp_path / "parent.s", tmp_path / "new.s"
    pa.write_text(a)
    pb.write_text(b)
    out = io.StringIO()
    return isa_compare.compare(str(pa), str(pb), out=out), out.getvalue()


def test_identical_and_reordered_pass(tmp_path):
    rc, out = run(tmp_path, listing(BODY), listing(BODY))
    assert rc == 0 and "1 identical" in out
    reordered = [BODY[0], BODY[1], BODY[2], BODY[5], BODY[3], BODY[4], BODY[6]]
    rc, out = run(tmp_path, listing(BODY), listing(reordered, vgpr=10))
    assert rc == 0 and "0 identical, 1 differ, 0 fail" in out and "f64 opcodes: same histogram" in out and "vgpr_count=12->10" in out


def test_split_fma_fails(tmp_path):
    split = BODY[:3] + ["v_mul_f64 v[6:7], v[0:1], v[2:3]", "v_add_f64 v[6:7], v[6:7], v[4:5]"] + BODY[4:]
    rc, out = run(tmp_path, listing(BODY), listing(split))
    assert rc == 1 and "1 fail" in out
    assert "'v_fma_f64': -1" in out and "'v_mul_f64': 1" in out and "'v_add_f64': 1" in out


def test_new_spill_or_scratch_fails(tmp_path):
    assert run(tmp_path, listing(BODY), listing(BODY, spill=2))[0] == 1
    assert run(tmp_path, listing(BODY), listing(BODY, private=16))[0] == 1
    assert run(tmp_path, listing(BODY, spill=2, private=16), listing(BODY))[0] == 0  # (fewer is fine)


def test_other_opcodes_are_reported_not_judged(tmp_path):
    more = BODY[:5] + ["v_accvgpr_write_b32 a0, v7", "s_waitcnt vmcnt(0)"] + BODY[5:]
    rc, out = run(tmp_path, listing(BODY), listing(more))
    assert rc == 0 and "'s_waitcnt': 1" in out and "'v_accvgpr_write_b32': 1" in out


def test_a_missing_descriptor_field_is_reported(tmp_path):
    broken = "\n".join(line for line in listing(BODY).split("\n") if ".vgpr_spill_count" not in line)
    with pytest.raises(SystemExit, match="vgpr_spill_count"):
        run(tmp_path, listing(BODY), broken)
