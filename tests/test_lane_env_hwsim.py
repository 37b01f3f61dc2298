"""mjb_lane_env_set_hwsim (the opt-in that lets a batch with the device hwsim stage run the lane = env kernel): the parts that need no GPU -- the
symbol is exported by libmjb.so, declared in include/mjb.h, bound in binding.py, and rejects a null batch."""
import ctypes as C
import os
import re

from mujoco_ros_pkgs_amd import binding, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_bound():
    lib = binding.load_library()
    raw = C.CDLL(lib._name)
    assert hasattr(raw, "mjb_lane_env_set_hwsim")
    header = open(os.path.join(ROOT, "include", "mjb.h")).read()
    assert re.search(r"^int mjb_lane_env_set_hwsim\(mjb_batch \*b, int on\);", header, re.M)
    fn = lib.mjb_lane_env_set_hwsim
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    assert callable(getattr(engine.Batch, "set_lane_env_hwsim"))


def test_null_batch_is_einval():
    lib = binding.load_library()
    assert lib.mjb_lane_env_set_hwsim(None, 1) == -1  # MJB_EINVAL
    assert b"null batch" in lib.mjb_last_error()

