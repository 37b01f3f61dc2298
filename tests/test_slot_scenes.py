"""Scenes for the row-slot Newton / CG solver (kernel variants 10 - 13) beyond the box grids of test_large_constraint_sets.py, and the KKT
certificate of tests/kkt.py on the oracle's solutions of them (CPU).

  * rows_xml: a hinge chain whose row count is set by its structure, not its state -- dof frictionloss (one row per hinge), welds (6),
    joint equalities (1) are always instantiated -- so that nefc sits exactly on the slot edges 64 k - 1, 64 k, 64 k + 1, at 0 and at
    the 1024-row capacity.  Its capsules give the model contact capacity (nefcmax > 256: the row-slot path) but touch nothing.
  * every_row_xml: one env-step with every row type: equality (connect, weld, joint), dof and tendon frictionloss, joint and tendon limits
    that start violated, and a 3 x 3 box grid with per-box condim 1 / 3 / 4 / 6 -- the non-contact rows cross row 128, cone leaders sit past
    row 255."""

import numpy as np
import pytest

from kkt import assert_certified, kkt_certificate, oracle_certificate
from mujoco_ros_pkgs_amd import mjcf
from test_large_constraint_sets import SCENES, compile_model, frame_info, grid_model, grid_xml, lib  # noqa: F401  (lib: the module fixture)


# both solvers run these scenes to a tight tolerance: at the default one CG's stationarity residual reaches 4e-4 on the welded chains
# (kkt.py), and Newton stops at 1e-9 on the every-row scene
TIGHT_TOL = ' tolerance="1e-12"'


def row_counts(nefc, nfric):
    """(frictionloss hinges, welds, joint equalities) giving exactly nefc rows."""
    f = min(nfric, nefc)
    return f, (nefc - f) // 6, (nefc - f) % 6


def rows_xml(nefc, solver="Newton", nhinge=12, njmax=1024, nfric=12):
    """A horizontal chain of nhinge capsule links 1 m up (hinges about y, the first one to the world), the first min(nfric, nefc) hinges
    with frictionloss, welds between neighbouring links and joint equalities between neighbouring hinges for the rest of the rows.
    Nothing touches anything within a few hundred steps.  Pyramidal condim-6 contacts
    between the links and with the floor give the model its contact capacity (nefcmax = njmax when that is below the worst case)."""
    f, w, j = row_counts(nefc, nfric)
    assert nhinge >= 2 and f <= nhinge and 6 * w + j + f == nefc
    body = ""
    for i in reversed(range(nhinge)):
        fl = ' frictionloss="0.02"' if i < f else ""
        body = (f'<body name="b{i}" pos="{0.0 if i == 0 else 0.1} 0 {1.0 if i == 0 else 0}"><joint name="h{i}" type="hinge" axis="0 1 0"'
                f' damping="0.01"{fl}/><geom type="capsule" fromto="0 0 0 0.1 0 0" size="0.01" mass="0.1"/>{body}</body>')
    eqs = "".join(f'<weld body1="b{k % (nhinge - 1)}" body2="b{k % (nhinge - 1) + 1}"/>' for k in range(w))
    eqs += "".join(f'<joint joint1="h{k % (nhinge - 1)}" joint2="h{k % (nhinge - 1) + 1}"/>' for k in range(j))
    return (f'<mujoco model="rows{nefc}"><size njmax="{njmax}"/><option timestep="0.002" solver="{solver}" cone="pyramidal"{TIGHT_TOL}/>'
            f'<default><geom condim="6" friction="0.8 0.02 0.002"/></default>'
            f'<worldbody><geom type="plane" size="5 5 0.1"/>{body}</worldbody><equality>{eqs}</equality></mujoco>')


def rows_model(nefc, solver="Newton", **kw):
    return mjcf.compile_xml_string(rows_xml(nefc, solver, **kw))


# the slot edges, each with the residency (row-slot solver, full frame in HBM, fused frame in HBM) of its model: with 12 hinges
# (nv 12) nefcmax 300 / 400 keeps both frames in LDS, 600 puts the full frame in HBM, 1024 both; 4 hinges keep the fused frame of 1024 rows in LDS
EDGES = [(0, dict(njmax=300), (1, 0, 0)), (1, dict(njmax=300), (1, 0, 0)), (63, dict(njmax=300), (1, 0, 0)),
         (64, dict(njmax=600), (1, 1, 0)), (65, dict(), (1, 1, 1)),
         (127, dict(njmax=300), (1, 0, 0)), (128, dict(njmax=600), (1, 1, 0)), (129, dict(), (1, 1, 1)),
         (255, dict(njmax=400), (1, 0, 0)), (256, dict(njmax=600), (1, 1, 0)), (257, dict(), (1, 1, 1)),
         (511, dict(njmax=600), (1, 1, 0)), (512, dict(), (1, 1, 1)), (513, dict(njmax=600), (1, 1, 0)),
         (1023, dict(nhinge=4, nfric=4), (1, 1, 0)), (1024, dict(), (1, 1, 1))]


def every_row_xml(solver="Newton", cone="elliptic", warmstart=True, limitfrc=False):
    """3 x 3 grid of free boxes 1 mm apart on a plane (contacts within the 2 mm margin), condim per box 1 / 3 / 4 / 6 (the floor's is 1:
    a contact takes the larger of its two), beside a 10-hinge chain (nv 64 in all) carrying 24 welds, 2 connects, 4 joint equalities,
    frictionloss on every hinge and on a fixed tendon, and lower limits of 0.05 on four hinges and on the tendon (violated at qpos0 = 0)."""
    cds = [1, 3, 4, 6, 1, 6, 4, 3, 1]
    boxes = []
    for i in range(3):
        for j in range(3):
            x, y, z = 0.101 * (i - 1), 0.101 * (j - 1), 0.0505 + 0.001 * ((i + j) % 2)
            boxes.append(f'<body pos="{x:.3f} {y:.3f} {z:.4f}"><freejoint/><geom type="box" size="0.05 0.05 0.05" mass="0.5" condim="{cds[3 * i + j]}"/></body>')
    chain = ""
    for i in reversed(range(10)):
        lim = ' limited="true" range="0.05 0.8"' if i >= 6 else ""
        chain = (f'<body name="c{i}" pos="{0.6 if i == 0 else 0.1} 0 {0.8 if i == 0 else 0}"><joint name="h{i}" type="hinge" axis="0 1 0"'
                 f' damping="0.02" frictionloss="0.01"{lim}/><geom type="capsule" fromto="0 0 0 0.1 0 0" size="0.01" mass="0.1"'
                 f' contype="0" conaffinity="0"/>{chain}</body>')
    eqs = "".join(f'<weld body1="c{k % 5}" body2="c{k % 5 + 1}"/>' for k in range(24))
    eqs += '<connect body1="c2" body2="c3" anchor="0.1 0 0"/><connect body1="c4" body2="c5" anchor="0.1 0 0"/>'
    eqs += '<joint joint1="h1" joint2="h2"/><joint joint1="h3" joint2="h4"/><joint joint1="h6" joint2="h7"/><joint joint1="h8" joint2="h9"/>'
    tendon = ('<tendon><fixed name="t0" limited="true" range="0.05 0.5" frictionloss="0.01"><joint joint="h8" coef="1"/>'
              '<joint joint="h9" coef="1"/></fixed></tendon>')
    flag = '<flag warmstart="disable"/>' if not warmstart else ""
    sensor = '<sensor><jointlimitfrc joint="h6"/><tendonlimitfrc tendon="t0"/></sensor>' if limitfrc else ""
    return (f'<mujoco model="every_row"><size njmax="1024"/><option timestep="0.002" solver="{solver}" cone="{cone}"{TIGHT_TOL}>{flag}</option>'
            f'<default><geom margin="0.002" friction="0.8 0.02 0.002"/></default>'
            f'<worldbody><geom type="plane" size="2 2 0.1" condim="1"/>{"".join(boxes)}{chain}</worldbody>'
            f'<equality>{eqs}</equality>{tendon}{sensor}</mujoco>')


def every_row_model(solver="Newton", cone="elliptic", **kw):
    return mjcf.compile_xml_string(every_row_xml(solver, cone, **kw))


# (solver, cone, warmstart, jointlimitfrc sensor)
EVERY_ROW = [(s, c, True, False) for s in ("Newton", "CG") for c in ("elliptic", "pyramidal")] + \
            [("Newton", "elliptic", False, False), ("CG", "pyramidal", False, False), ("Newton", "elliptic", True, True)]


def every_row_id(p):
    return f"{p[0]}-{p[1]}" + ("" if p[2] else "-nowarm") + ("-limitfrc" if p[3] else "")


def condim3_grid_model(solver):
    """The 3 x 3 box grid of test_large_constraint_sets.py with elliptic condim-3 contacts (hcd = 3): worst case 768 rows, the slot path."""
    return mjcf.compile_xml_string(grid_xml(solver, "elliptic", 3).replace('cone="elliptic"', 'cone="elliptic"' + TIGHT_TOL))


def settle(po, model, steps=20):
    """qpos0 stepped `steps` times on the oracle: the boxes touch the floor and each other."""
    d = po.OracleData(model)
    d.reset()
    d.step(steps)
    return np.array(d.qpos), np.array(d.qvel)


def oracle_forward(po, model, qpos, qvel):
    d = po.OracleData(model)
    d.reset()
    d.qpos[:] = qpos
    d.qvel[:] = qvel
    d.forward()
    return d


def perturbed_certificates(model, d):
    """The certificate of the oracle's solution with one row's force moved by 1e-6 of itself (the row of the largest |R f|), and with qacc
    replaced by qacc_smooth: both must fail."""
    n, ncon = int(d.nefc[0]), int(d.ncon[0])
    f = np.array(d.efc_force[:n])
    r = int(np.argmax(np.abs(np.array(d.efc_R[:n]) * f)))
    f[r] *= 1 + 1e-6
    args = (d.efc_R[:n], d.efc_aref[:n])
    tail = (d.efc_type[:n], d.efc_frictionloss[:n], d.contact_efc_address[:ncon], d.contact_dim[:ncon], d.contact_friction, ncon)
    one = kkt_certificate(model, d.qM, d.efc_J, *args, d.qacc_smooth, d.qacc, f, *tail)
    smooth = kkt_certificate(model, d.qM, d.efc_J, *args, d.qacc_smooth, d.qacc_smooth, d.efc_force[:n], *tail)
    return one, smooth


def _assert_has_teeth(model, d):
    one, smooth = perturbed_certificates(model, d)
    for cert, what in ((one, "one force moved by 1e-6"), (smooth, "qacc = qacc_smooth")):
        with pytest.raises(AssertionError):
            assert_certified(cert, model, what)


@pytest.mark.parametrize("solver", ["Newton", "CG"])
@pytest.mark.parametrize("nefc,kw,info", EDGES, ids=[str(e[0]) for e in EDGES])
def test_row_scene_has_exact_rows_and_residency(lib, oracle_built, solver, nefc, kw, info):  # noqa: F811
    model = rows_model(nefc, solver, **kw)
    assert model["nefcmax"] > 256 and model["nefcmax"] >= nefc
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert frame_info(lib, ptr) == info
    finally:
        lib.mjb_free_model(ptr)
    d = oracle_forward(oracle_built, model, model["qpos0"], np.zeros(model["nv"]))
    assert int(d.nefc[0]) == nefc and int(d.ncon[0]) == 0
    assert_certified(oracle_certificate(model, d), model, f"oracle {solver} nefc {nefc}")
    if nefc:
        d.step(20)        # (the rows stay put as the chain swings)
        d.forward()
        assert int(d.nefc[0]) == nefc and int(d.ncon[0]) == 0
        assert_certified(oracle_certificate(model, d), model, f"oracle {solver} nefc {nefc} after 20 steps")
        _assert_has_teeth(model, d)


def test_row_scene_beyond_capacity(lib, oracle_built):  # noqa: F811
    model = rows_model(1030, "Newton")
    assert model["nefcmax"] == 1024
    ptr, err = compile_model(lib, model)
    assert ptr, err
    lib.mjb_free_model(ptr)
    d = oracle_forward(oracle_built, model, model["qpos0"], np.zeros(model["nv"]))
    assert d.warning(2) > 0


@pytest.mark.parametrize("p", EVERY_ROW, ids=every_row_id)
def test_every_row_scene(lib, oracle_built, p):  # noqa: F811
    solver, cone, warm, limitfrc = p
    model = every_row_model(solver, cone, warmstart=warm, limitfrc=limitfrc)
    assert model["nv"] == 64 and model["nefcmax"] == 1024
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert frame_info(lib, ptr) == (1, 1, 1)
    finally:
        lib.mjb_free_model(ptr)
    qpos, qvel = settle(oracle_built, model)
    d = oracle_forward(oracle_built, model, qpos, qvel)
    n, ncon = int(d.nefc[0]), int(d.ncon[0])
    types = np.array(d.efc_type[:n])
    nc = int(np.count_nonzero(types <= 4))   # (equality, friction and limit rows come first)
    assert set(types[:nc]) == {0, 1, 2, 3, 4} and nc > 128 and not np.isin(types[nc:], [0, 1, 2, 3, 4]).any()
    dims = {int(d.contact_dim[c]) for c in range(ncon)}
    assert dims == {1, 3, 4, 6}, dims
    leaders = [int(d.contact_efc_address[c]) for c in range(ncon) if int(d.contact_dim[c]) > 1]
    assert max(leaders) > 255, (n, max(leaders))
    if cone == "elliptic":
        assert {5, 7} <= set(types)
    assert_certified(oracle_certificate(model, d), model, f"oracle {every_row_id(p)}")
    _assert_has_teeth(model, d)


@pytest.mark.parametrize("solver", ["Newton", "CG"])
def test_elliptic_condim3_grid_takes_the_slot_path(lib, oracle_built, solver):  # noqa: F811
    model = condim3_grid_model(solver)
    assert model["nefcmax"] == 768   # (the grid's worst case: 3 rows a contact)
    ptr, err = compile_model(lib, model)
    assert ptr, err
    try:
        assert frame_info(lib, ptr) == (1, 1, 1)
    finally:
        lib.mjb_free_model(ptr)
    qpos, qvel = settle(oracle_built, model, 100)
    d = oracle_forward(oracle_built, model, qpos, qvel)
    assert int(d.nefc[0]) > 64 and set(np.array(d.efc_type[:int(d.nefc[0])])) == {7}
    assert_certified(oracle_certificate(model, d), model, f"oracle {solver} elliptic condim 3")
    _assert_has_teeth(model, d)


@pytest.mark.parametrize("solver", ["Newton", "CG"])
@pytest.mark.parametrize("cone,condim,_rows", SCENES)
def test_box_grid_certificate(oracle_built, solver, cone, condim, _rows):
    # the 3 x 3 grids of test_large_constraint_sets.py at their default tolerance, settled
    model = grid_model(solver, cone, condim)
    qpos, qvel = settle(oracle_built, model, 100)
    d = oracle_forward(oracle_built, model, qpos, qvel)
    assert int(d.nefc[0]) > 64
    assert_certified(oracle_certificate(model, d), model, f"oracle {solver} {cone} condim {condim}")
    _assert_has_teeth(model, d)


def test_random_slot_seeds_take_the_slot_path(lib):  # noqa: F811
    from test_gpu_random_models import SLOT_PILES, SLOT_SEEDS, random_model, random_pile
    for gen, seeds in ((random_model, SLOT_SEEDS), (random_pile, SLOT_PILES)):
        for seed in seeds:
            model = mjcf.compile_xml_string(gen(seed, large=True))
            assert int(model["solver"]) in (1, 2)
            ptr, err = compile_model(lib, model)
            assert ptr, (gen.__name__, seed, err)
            try:
                assert frame_info(lib, ptr)[0] == 1, (gen.__name__, seed)
            finally:
                lib.mjb_free_model(ptr)
