"""mjb_compile builds the same model as it did before the compiler moved into csrc/mjb_model.hip and was cut into stages (no GPU).

mjb_debug_model_digest hashes a compiled model member by member into four words: [0] the copied description, [1] every derived table
and scalar, [2] the frame layouts with what is decided next to them, [3] the lane = env / split-step classification and tape.
tests/golden/model_digest_before_compiler_split.json holds the words of every model of tests/compiler_models.py as the commit before the
split computed them (that commit with the digest function alone added; `python tests/test_model_digest.py` writes the file from
whatever library is built)."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compiler_models import MODELS  # noqa: E402
from mujoco_ros_pkgs_amd import binding, engine  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_digest_before_compiler_split.json")
KNOBS = ("MJB_DEBUG_JROWS", "MJB_DEBUG_FRAME_ROWS", "MJB_DEBUG_LAYOUT", "MJB_WIDE_ROWS")  # they change the layouts: [2] is recorded without them
WORDS = ("description", "derived tables", "layouts", "lane = env / split step")


def digest(model):
    lib = binding.load_library()
    cm = engine.CompiledModel(model)
    out = (C.c_ulonglong * 4)()
    assert lib.mjb_debug_model_digest(cm.ptr, out) == 0
    return [f"{int(w):016x}" for w in out]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_listed_model_is_recorded(golden):
    assert sorted(golden) == sorted(MODELS)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_compiled_model_unchanged(golden, name):
    for k in KNOBS:
        assert k not in os.environ, f"{k} is set: the recorded layouts are the default ones"
    got = digest(MODELS[name]())
    for what, g, w in zip(WORDS, got, golden[name]):
        assert g == w, f"{name}: {what} differ from the compiler before the split"


def test_digest_tells_models_apart(golden):
    """The recording has teeth: no two listed models share a description word, and each word varies over the list."""
    assert len({v[0] for v in golden.values()}) == len(golden)
    for k in range(4):
        assert len({v[k] for v in golden.values()}) > 1


if __name__ == "__main__":
    rec = {name: digest(make()) for name, make in sorted(MODELS.items())}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} models -> {GOLDEN}")
