"""The lane = env launcher's plan (csrc/mjb_lane_env.hip: le_plan) through its introspection entry, mjb_lane_env_plan -- no GPU: which form, how many
sweep wavefronts and which LDS budget a launch gets, as a function of CU count, batch size, build and requests alone ("The lane = env
launcher").  The rows are the launcher's decisions before the plan became a function of its own, derived from that code by hand and confirmed by
comparing both exhaustively (profiles/lane_env_launcher_refactor.txt); tests/test_gpu_lane_env_plan.py holds the launcher to the plan on the device."""
import ctypes as C
import os
import sys

import pytest

from mujoco_ros_pkgs_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAIN, OVERLAY, HWSIM, XFRC, OVERLAY_XFRC = range(5)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load_library()


def plan(lib, nenv, ncu=256, build=PLAIN, form=-1, sweep=0, kb=0, model=None):
    """(form, sweep wavefronts, LDS KB), or None when there is no variant."""
    out = [C.c_int(-9) for _ in range(3)]
    rc = lib.mjb_lane_env_plan(model, ncu, nenv, build, form, sweep, kb, *[C.byref(o) for o in out])
    return None if rc != 0 else tuple(o.value for o in out)


def test_default_rule_on_256_cus(lib):
    """No request: three outcomes only -- four sweep wavefronts while a block has a CU to itself, two halves up to twice that, one wavefront beyond."""
    assert plan(lib, 64) == (3, 4, 160)
    assert plan(lib, 16384) == (3, 4, 160)
    assert plan(lib, 16385) == (1, 0, 80)
    assert plan(lib, 32768) == (1, 0, 80)
    assert plan(lib, 32769) == (0, 0, 40)
    seen = {plan(lib, n) for n in range(1, 70000, 61)}
    assert seen == {(3, 4, 160), (1, 0, 80), (0, 0, 40)}


def test_lds_knob_at_160_reaches_the_other_forms(lib):
    assert plan(lib, 16385, kb=160) == (3, 3, 160)
    assert plan(lib, 21824, kb=160) == (3, 3, 160)   # 341 wavefronts: 3 x 341 <= 4 x 256
    assert plan(lib, 21825, kb=160) == (2, 0, 160)
    assert plan(lib, 32768, kb=160) == (2, 0, 160)
    assert plan(lib, 32769, kb=160) == (0, 0, 160)
    assert plan(lib, 64, kb=80) == (1, 0, 80)
    assert plan(lib, 64, kb=40) == (0, 0, 40)
    assert plan(lib, 64, kb=100) == (3, 4, 160)      # (not a budget: the rule)


def test_requested_forms(lib):
    # a batch at four wavefronts per CU: any form > 0 is the two halves at two per CU
    for form in (1, 2, 3):
        assert plan(lib, 65536, form=form) == (1, 0, 80)
    assert plan(lib, 65536, form=0) == (0, 0, 40)
    # a batch with a CU per block: every form as asked for, at 160 KB
    assert plan(lib, 4096, form=0) == (0, 0, 160)
    assert plan(lib, 4096, form=1) == (1, 0, 160)
    assert plan(lib, 4096, form=2) == (2, 0, 160)
    assert plan(lib, 4096, form=3) == (3, 4, 160)
    assert plan(lib, 4096, form=3, sweep=3) == (3, 3, 160)
    assert plan(lib, 4096, sweep=3) == (3, 3, 160)
    assert plan(lib, 4096, sweep=7) == (3, 4, 160)   # (neither 3 nor 4: the rule)
    assert plan(lib, 4096, form=2, sweep=4) == (2, 0, 160)
    # a request keeps more than one wavefront beyond twice the CUs' worth at an 80 KB budget; forms 2 and 3 need 160
    assert plan(lib, 20000, form=3) == (1, 0, 80)
    assert plan(lib, 40000, form=3, kb=160) == (2, 0, 160)   # 625 wavefronts: 3 x 625 > 4 x 256
    assert plan(lib, 40000, kb=160) == (0, 0, 160)
    assert plan(lib, 4096, form=9) == (3, 4, 160)            # (out of range: the rule, as mjb_lane_env_set_form takes it)


@pytest.mark.parametrize("build", [OVERLAY, HWSIM, XFRC, OVERLAY_XFRC])
def test_opt_in_builds_run_one_wavefront(lib, build):
    for form in (-1, 0, 1, 2, 3):
        for sweep in (0, 3, 4):
            assert plan(lib, 16384, build=build, form=form, sweep=sweep) == (0, 0, 160)   # 256 wavefronts
            assert plan(lib, 32768, build=build, form=form, sweep=sweep) == (0, 0, 80)    # 512
            assert plan(lib, 32769, build=build, form=form, sweep=sweep) == (0, 0, 40)    # 513
    assert plan(lib, 64, build=build, kb=80) == (0, 0, 80)


def test_cu_count(lib):
    for nenv in (64, 4096, 65536):
        assert plan(lib, nenv, ncu=0) == (0, 0, 40)     # unknown device: the leanest variant
    assert plan(lib, 4096, ncu=0, form=3) == (1, 0, 80)
    assert plan(lib, 4096, ncu=64) == (3, 4, 160)
    assert plan(lib, 4097, ncu=64) == (1, 0, 80)
    assert plan(lib, 19456, ncu=304) == (3, 4, 160)     # 304 wavefronts
    assert plan(lib, 19457, ncu=304) == (1, 0, 80)


def test_arguments_out_of_range(lib):
    assert plan(lib, 0) is None
    assert plan(lib, 64, build=5) is None and plan(lib, 64, build=-1) is None
    # outputs may be NULL
    assert lib.mjb_lane_env_plan(None, 256, 64, 0, -1, 0, 0, None, None, None) == 0


def test_fit_limits_of_a_hiprtc_built_model(lib):
    """two_arm_xml(): 14 dofs, 15 moving bodies, 16 bodies.  State and forces take 14 + 3 x 15 = 59 pair slots (so never the 40 KB budget); the trio's
    layout 59 + 5 x 15 + 18 + 8 + 16 = 176 > 160, the pipelined duo's 59 + 75 + 12 + 8 = 154: a request for form 3 on four wavefronts runs form 2 -- what
    tests/test_gpu_lane_env_sweep_waves.py::test_layout_beyond_the_lds_falls_back observes on the device ("form 1 or 2, no sweep wavefronts")."""
    from mujoco_ros_pkgs_amd import engine, mjcf
    from test_gpu_lane_env import JIT_ARM, two_arm_xml
    cm = engine.CompiledModel(mjcf.compile_xml_string(two_arm_xml()))
    try:
        assert int(cm.lib.mjb_model_lane_env(cm.ptr)) == -2
        for form in (3, -1):   # (that test asks for four sweep wavefronts and leaves the form to its fixture, form 3; the rule gives the same)
            got = plan(lib, 200, form=form, sweep=4, model=cm.ptr)
            assert got == (2, 0, 160)
            assert got[0] in (1, 2) and got[1] == 0
        assert plan(lib, 200, model=cm.ptr) == (2, 0, 160)
        assert plan(lib, 200, form=1, model=cm.ptr) == (1, 0, 160)
        assert plan(lib, 20000, model=cm.ptr) == (1, 0, 80)          # 59 + 8 <= 80
        assert plan(lib, 65536, model=cm.ptr) == (0, 0, 80)          # the budget rises to what the state needs
        assert plan(lib, 65536, build=OVERLAY, model=cm.ptr) == (0, 0, 80)
    finally:
        cm.close()
    # a small hiprtc-built model fits every form; a compiled-in topology has no fit test; a model the kernel does not take has no plan
    arm = JIT_ARM.replace('actuator="3"', 'actuator="act3"').replace('<motor joint="j4" forcelimited', '<motor name="act3" joint="j4" forcelimited')
    for model, want in ((mjcf.compile_xml_string(arm), (3, 4, 160)), (mjcf.load_asset("franka_like"), (3, 4, 160)), (mjcf.load_asset("franka_table"), None)):
        cm = engine.CompiledModel(model)
        try:
            assert plan(lib, 64, model=cm.ptr) == want
        finally:
            cm.close()
