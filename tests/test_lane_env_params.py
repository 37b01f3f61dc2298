"""The per-env table of the lane = env kernel (Batch.set_lane_env(2); PeSlots in csrc/mjb_lane_env_kernel.h, mjb_lane_env_overlay_row in
csrc/mjb_lane_env.hip), restated in numpy: which values it holds, in which order, and that they are the numbers mjb_compile put on the kernel's
constant tape (LeTapeHdr | LeTapeBody[nbody] | LeTapeAct[nu], csrc/mjb_dev.h) for a model nobody has randomised.  No device needed (mjb_compile and the two
introspection calls run on the host)."""
import os

import numpy as np
import pytest

from mujoco_ros_pkgs_amd import mjcf

HDR, BODY, ACT = 8, 32, 16  # doubles per tape record
# offsets inside a LeTapeBody / LeTapeAct record
STIFFNESS, IBODY, MASS, DAMPING, ARMATURE, HDAMPING = 14, 19, 25, 26, 27, 28
GAIN, BIAS = 3, 6


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g
    from mujoco_ros_pkgs_amd import binding, engine as e
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    binding.load_library()
    return e


def quat2mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def moving(m, b):
    """A joint on the body's path to the world."""
    while b > 0:
        if m["body_jntnum"][b] > 0:
            return True
        b = int(m["body_parentid"][b])
    return False


def overlay_column(m, gravity=None):
    """One env's column, in slot order, from the model dict."""
    nb, nu = int(m["nbody"]), int(m["nu"])
    dt = float(np.ravel(m["timestep"])[0])
    out = list(np.asarray(m["gravity"] if gravity is None else gravity, dtype=np.float64))
    for b in range(1, nb):
        if m["body_jntnum"][b] == 1:
            j = int(m["body_jntadr"][b])
            d = int(m["jnt_dofadr"][j])
            out += [m["jnt_stiffness"][j], m["dof_damping"][d], m["dof_armature"][d], dt * m["dof_damping"][d]]
    for b in range(1, nb):
        if moving(m, b):
            R = quat2mat(np.asarray(m["body_iquat"], dtype=np.float64).reshape(-1, 4)[b])
            Ib = R @ np.diag(np.asarray(m["body_inertia"], dtype=np.float64).reshape(-1, 3)[b]) @ R.T
            out += [m["body_mass"][b], Ib[0, 0], Ib[1, 1], Ib[2, 2], Ib[0, 1], Ib[0, 2], Ib[1, 2]]
    gain = np.asarray(m["actuator_gainprm"], dtype=np.float64).reshape(nu, -1)
    bias = np.asarray(m["actuator_biasprm"], dtype=np.float64).reshape(nu, -1)
    for i in range(nu):
        out += list(gain[i, :3]) + list(bias[i, :3])
    out += [m["body_mass"][b] for b in range(1, nb) if not moving(m, b)]
    return np.asarray(out, dtype=np.float64)


@pytest.mark.parametrize("asset", ["franka_like", "lane_env_tree"])
def test_overlay_layout_matches_the_tape(engine, asset):
    m = mjcf.load_asset(asset)
    cm = engine.CompiledModel(m)
    assert cm.lib.mjb_model_lane_env(cm.ptr) >= 0
    nb, nu = int(m["nbody"]), int(m["nu"])
    tape, col = cm.lane_env_tape(), cm.lane_env_overlay()
    assert tape.size == HDR + BODY * nb + ACT * nu
    jointed = [b for b in range(1, nb) if m["body_jntnum"][b] == 1]
    mov = [b for b in range(1, nb) if moving(m, b)]
    rest = [b for b in range(1, nb) if not moving(m, b)]
    assert len(jointed) == int(m["njnt"])
    # slot count and order: the numpy restatement, value for value (ibody to rounding: R diag R' summed in another order)
    want = overlay_column(m)
    assert col.size == want.size == 3 + 4 * len(jointed) + 7 * len(mov) + 6 * nu + len(rest)
    np.testing.assert_allclose(col, want, rtol=0, atol=1e-15 * (1 + np.abs(want).max()))
    # ... and every slot is the number the kernel reads off the tape today
    body = lambda b, k: tape[HDR + BODY * b + k]  # noqa: E731
    at = 0
    assert np.array_equal(col[:3], tape[1:4])
    at += 3
    dt = tape[0]
    assert dt == float(np.ravel(m["timestep"])[0])
    for b in jointed:
        assert np.array_equal(col[at:at + 4], [body(b, STIFFNESS), body(b, DAMPING), body(b, ARMATURE), body(b, HDAMPING)]), f"body {b}"
        assert col[at + 3] == dt * col[at + 1]  # hdamping = timestep * damping
        at += 4
    for b in mov:
        assert col[at] == body(b, MASS), f"body {b}"
        assert np.array_equal(col[at + 1:at + 7], tape[HDR + BODY * b + IBODY:HDR + BODY * b + IBODY + 6]), f"body {b}"
        at += 7
    for i in range(nu):
        a0 = HDR + BODY * nb + ACT * i
        assert np.array_equal(col[at:at + 3], tape[a0 + GAIN:a0 + GAIN + 3]) and np.array_equal(col[at + 3:at + 6], tape[a0 + BIAS:a0 + BIAS + 3]), f"actuator {i}"
        at += 6
    for b in rest:
        assert col[at] == body(b, MASS)
        at += 1
    assert at == col.size
    assert np.any(np.asarray(m["dof_damping"]) > 0)  # (hdamping is not trivially zero)
    cm.close()


def test_ineligible_model_has_no_overlay(engine):
    cm = engine.CompiledModel(mjcf.load_asset("franka_table"))
    assert cm.lib.mjb_model_lane_env(cm.ptr) == -1
    assert cm.lane_env_overlay() is None and cm.lane_env_tape() is None
    cm.close()
