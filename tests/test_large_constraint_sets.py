"""Newton / CG models beyond 256 constraint rows (up to nefcmax = 1024) and frames beyond one CU's LDS: mjb_compile takes them and
routes them to the row-slot solver, whose frames live in HBM when they exceed the LDS budget (mjb_model_frame_info).  PGS keeps its caps.
The scenes: a 3 x 3 grid of free boxes on a floor (nv 54), pyramidal condim 3, elliptic condim 6 and pyramidal condim 6 contacts."""
import ctypes as C
import os

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import binding, mjcf

# (cone, condim, rows the oracle must exceed within SETTLE steps)
SCENES = [("pyramidal", 3, 256), ("elliptic", 6, 256), ("pyramidal", 6, 512)]
SETTLE = 100


def grid_xml(solver="Newton", cone="pyramidal", condim=3, njmax=1024, nconmax=256, n=3):
    """An n x n grid of free 10 cm boxes resting on a plane, 1 mm apart, every other one 1 mm up (contacts within the 2 mm margin)."""
    bodies = []
    for i in range(n):
        for j in range(n):
            x, y, z = 0.101 * (i - 1), 0.101 * (j - 1), 0.0505 + 0.001 * ((i + j) % 2)
            bodies.append(f'<body pos="{x:.3f} {y:.3f} {z:.4f}"><freejoint/><geom type="box" size="0.05 0.05 0.05" mass="0.5"/></body>')
    size = f'<size njmax="{njmax}" nconmax="{nconmax}"/>' if njmax is not None else ""
    return (f'<mujoco model="box_grid">{size}<option timestep="0.002" solver="{solver}" cone="{cone}"/>'
            f'<default><geom condim="{condim}" margin="0.002" friction="0.8 0.02 0.002"/></default>'
            f'<worldbody><geom type="plane" size="2 2 0.1"/>{"".join(bodies)}</worldbody></mujoco>')


def grid_model(solver="Newton", cone="pyramidal", condim=3, **kw):
    return mjcf.compile_xml_string(grid_xml(solver, cone, condim, **kw))


# 2 x 2 grids (nv 24), pyramidal condim 6, beyond 256 rows: (njmax, frame_info) -- 300 rows: both frames in LDS (kernel variants 10 / 11);
# 400 rows: the full frame in HBM (mjb_forward, the split step: 12 / 13), the fused frame in LDS (10 / 11)
SMALL = [(300, (1, 0, 0)), (400, (1, 1, 0))]


def small_grid_model(solver, njmax):
    return grid_model(solver, "pyramidal", 6, njmax=njmax, n=2)


def compile_model(lib, model):
    desc, keep = binding.make_desc(model)
    ptr = lib.mjb_compile(C.byref(desc))
    return ptr, lib.mjb_last_error().decode()


def frame_info(lib, ptr):
    full, fused = C.c_int(-1), C.c_int(-1)
    slot = lib.mjb_model_frame_info(ptr, C.byref(full), C.byref(fused))
    return slot, full.value, fused.value


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load_library()


@pytest.mark.parametrize("solver", ["Newton", "CG"])
@pytest.mark.parametrize("cone,condim,_rows", SCENES)
def test_box_grid_compiles(lib, solver, cone, condim, _rows):
    model = grid_model(solver, cone, condim)
    assert model["nv"] == 54 and model["nefcmax"] == 1024
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert frame_info(lib, ptr) == (1, 1, 1)  # (efc_J alone is 1024 x 54 doubles: both frames live in HBM)
        assert lib.mjb_frame_bytes(ptr, 0) > 160 * 1024 and lib.mjb_frame_bytes(ptr, 1) > 160 * 1024
    finally:
        lib.mjb_free_model(ptr)


@pytest.mark.parametrize("njmax", [400, 512, 700])
def test_intermediate_capacities_compile(lib, njmax):
    model = grid_model("Newton", "elliptic", 6, njmax=njmax)
    assert model["nefcmax"] == njmax
    ptr, err = compile_model(lib, model)
    assert ptr, err
    assert frame_info(lib, ptr)[0] == 1
    lib.mjb_free_model(ptr)


def test_large_frame_within_256_rows_compiles(lib):
    # nv 54 with 256 rows of capacity: refused before for its frame alone (beyond one CU's LDS); the row-slot solver runs it from HBM
    model = grid_model("Newton", "elliptic", 6, njmax=256)
    assert model["nefcmax"] == 256
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert lib.mjb_frame_bytes(ptr, 0) > 160 * 1024
        slot, full, _ = frame_info(lib, ptr)
        assert slot == 1 and full == 1
    finally:
        lib.mjb_free_model(ptr)


@pytest.mark.parametrize("solver", ["Newton", "CG"])
def test_above_1024_rows_refused(lib, solver):
    model = grid_model(solver, "pyramidal", 6, njmax=1025)
    assert model["nefcmax"] == 1025
    ptr, err = compile_model(lib, model)
    assert not ptr
    assert "one env per wavefront" in err and "1024" in err and "njmax" in err, err


@pytest.mark.parametrize("cone,condim,cap", [("pyramidal", 3, 128), ("elliptic", 3, 64)])
def test_pgs_caps_unchanged(lib, cone, condim, cap):
    ptr, err = compile_model(lib, grid_model("PGS", cone, condim, njmax=cap + 1))
    assert not ptr and "one env per wavefront" in err, err
    # within the row cap, a frame beyond one CU's LDS is still refused under PGS
    ptr, err = compile_model(lib, grid_model("PGS", cone, condim, njmax=cap))
    assert not ptr and "exceeds one CU" in err, err


@pytest.mark.parametrize("solver", ["Newton", "CG"])
@pytest.mark.parametrize("njmax,info", SMALL)
def test_small_grids_keep_frames_in_lds(lib, solver, njmax, info):
    model = small_grid_model(solver, njmax)
    assert model["nv"] == 24 and model["nefcmax"] == njmax
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert frame_info(lib, ptr) == info
        assert (lib.mjb_frame_bytes(ptr, 0) > 160 * 1024) == bool(info[1]) and lib.mjb_frame_bytes(ptr, 1) <= 160 * 1024
    finally:
        lib.mjb_free_model(ptr)


def test_models_within_the_old_caps_keep_their_path(lib):
    for name, kw in [("franka_table", {}), ("shadow_hand_like", {"nefcmax": 160}), ("shadow_hand_like", {"nefcmax": 128})]:
        ptr, err = compile_model(lib, mjcf.load_asset(name, **kw))
        assert ptr, err
        assert frame_info(lib, ptr) == (0, 0, 0), name
        lib.mjb_free_model(ptr)


@pytest.mark.parametrize("cone,condim,rows", SCENES)
def test_oracle_rows_exceed_old_cap(oracle_built, cone, condim, rows):
    model = grid_model("Newton", cone, condim)
    d = oracle_built.OracleData(model)
    d.reset()
    most = 0
    for _ in range(SETTLE):
        d.step(1)
        most = max(most, int(d.nefc[0]))
    assert most > rows, (cone, condim, most)
    assert d.warning(2) == 0  # (no row dropped at 1024 rows of capacity)
