"""build_model_blob lays the device model blob out as mjb_make_batch did when it held the layout itself, in three hand-kept lists (no GPU).

mjb_debug_blob_digest hashes the blob a batch of the model would upload into three words: [0] the offset of every DevModel pointer member from
the blob's base, in declaration order, [1] the contents of every table, read through those offsets over the table's length, [2] every other
member of the DevModel.  tests/golden/model_blob_digest_before_owner_refactor.json holds the words of every model of tests/compiler_models.py
as the commit before the blob moved into csrc/mjb_model.hip laid it out: made from a copy of that commit in which the blob lines of
mjb_make_batch were lifted as they stood into a host function (the two device calls cut out, the image left on the host) and hashed by a
digest entry written against DevModel's declaration, with `python tests/test_model_blob_digest.py` and MJB_LIBRARY naming that build.

The digest entry of today's builder also checks what it promises about the layout -- every derived int table on a 16-byte boundary, the
lane = env tape on a 64-byte one, no table overlapping the next, the last one ending inside the image -- and fails when one does not hold."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compiler_models import MODELS  # noqa: E402
from mujoco_ros_pkgs_amd import binding, engine  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_blob_digest_before_owner_refactor.json")
KNOBS = ("MJB_DEBUG_JROWS", "MJB_DEBUG_FRAME_ROWS", "MJB_DEBUG_LAYOUT", "MJB_WIDE_ROWS")  # they change the layouts, and with them sens_copy
WORDS = ("table offsets", "table contents", "sizes, options and derived scalars")


def digest(model):
    lib = binding.load_library()
    cm = engine.CompiledModel(model)
    out = (C.c_ulonglong * 3)()
    rc = lib.mjb_debug_blob_digest(cm.ptr, out)
    assert rc == 0, lib.mjb_last_error().decode()
    return [f"{int(w):016x}" for w in out]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_listed_model_is_recorded(golden):
    assert sorted(golden) == sorted(MODELS)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_blob_unchanged(golden, name):
    for k in KNOBS:
        assert k not in os.environ, f"{k} is set: the recorded blobs are the default ones"
    got = digest(MODELS[name]())
    for what, g, w in zip(WORDS, got, golden[name]):
        assert g == w, f"{name}: {what} differ from the blob mjb_make_batch laid out itself"


@pytest.mark.parametrize("name", sorted(MODELS))
def test_blob_layout_promises(name):
    """Alignment, no overlap, all inside the image: mjb_debug_blob_digest answers MJB_EINVAL with the offending table otherwise."""
    lib = binding.load_library()
    cm = engine.CompiledModel(MODELS[name]())
    out = (C.c_ulonglong * 3)()
    assert lib.mjb_debug_blob_digest(cm.ptr, out) == 0, lib.mjb_last_error().decode()


def test_digest_tells_models_apart(golden):
    """The recording has teeth: no two listed models share what the blob holds, and each word varies over the list.  (Contents AND scalars: the list
    has models that differ in an option alone -- the same scene under another solver, integrator or njmax -- whose tables are the same, byte for byte,
    and whose difference lies in word [2]; 75 of the 87 contents words are distinct, and those that repeat do so only within such families.)"""
    assert len({(v[1], v[2]) for v in golden.values()}) == len(golden)
    by_contents = {}
    for name, v in golden.items():
        by_contents.setdefault(v[1], []).append(name)
    assert len(by_contents) >= 75
    for names in by_contents.values():
        assert len({golden[n][0] for n in names}) == 1  # (equal tables sit at equal offsets)
    for k in range(3):
        assert len({v[k] for v in golden.values()}) > 1


if __name__ == "__main__":
    rec = {name: digest(make()) for name, make in sorted(MODELS.items())}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} models -> {GOLDEN}")
