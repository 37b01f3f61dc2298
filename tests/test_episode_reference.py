"""tests/episode_ref.py, the numpy reference of the device-side episode resets, checked on the CPU: its Philox-4x32-10 against the oracle's
(mjo_philox4x32: the Random123 known-answer vector and random counters, every output word equal), its own invariants (u in (0, 1), the pick covers
0..ninit-1, reset quaternions stay unit, the clamp, the done rule with NaN and infinite bounds), and that the entry points of the feature are declared
in binding.py and exported by libmjb.so."""
import ctypes as C
import os

import numpy as np
import pytest

import episode_ref as er
import jacobian_models as jm
from mujoco_ros_pkgs_amd import binding, refdyn

EPISODE_SYMBOLS = ("mjb_episode_set_init", "mjb_episode_set_noise", "mjb_episode_set_rule", "mjb_episode_reset", "mjb_episode_step", "mjb_episode_get",
                   "mjb_episode_device_ptr")


def test_numpy_philox_equals_the_oracles(oracle_built):
    L = oracle_built.lib()
    assert [hex(int(x)) for x in er.philox4x32([0, 0, 0, 0], [0, 0])] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]   # Random123 kat_vectors
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (200, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (200, 2), dtype=np.uint64)
    ctr[:3] = [[0xFFFFFFFF] * 4, [0, 0, 0, 0x80000000], [1, 0, 0xFFFFFFFF, 0x80000012]]
    got = er.philox4x32(ctr, key)
    for i in range(len(ctr)):
        c = (C.c_uint32 * 4)(*[int(x) for x in ctr[i]])
        k = (C.c_uint32 * 2)(*[int(x) for x in key[i]])
        L.mjo_philox4x32(c, k)
        assert [int(x) for x in got[i]] == list(c), i


def test_uniform_draws_and_pick():
    genv = np.arange(-3, 4000, dtype=np.int64)[:, None] + (1 << 33)
    uu = er.u(0x123456789ABCDEF, genv, 3, np.arange(19)[None, :])
    assert uu.shape == (4003, 19) and np.all(uu > 0) and np.all(uu < 1)
    assert abs(uu.mean() - 0.5) < 0.005 and abs(uu.var() - 1 / 12) < 0.002
    # the counter words: env, episode, idx and the seed each change the draw; the same arguments give the same draw
    base = float(er.u(7, 5, 2, 4))
    assert base == float(er.u(7, 5, 2, 4))
    assert len({base, float(er.u(8, 5, 2, 4)), float(er.u(7, 6, 2, 4)), float(er.u(7, 5, 3, 4)), float(er.u(7, 5, 2, 5)), float(er.u(7 + (1 << 32), 5, 2, 4)),
                float(er.u(7, 5 + (1 << 32), 2, 4))}) == 7
    # extremes of w0: u stays inside (0, 1) and the pick inside the bank
    assert (0 + 0.5) / 4294967296.0 > 0 and (4294967295 + 0.5) / 4294967296.0 < 1
    for ninit in (1, 2, 5, 7):
        ks = [er.pick(11, e, 0, 9, ninit) for e in range(400)]
        assert sorted(set(ks)) == list(range(ninit)), ninit


@pytest.mark.parametrize("name", ["two_roots", "franka_like"])
def test_reset_state_invariants(name):
    m = jm.model(name)
    nv = int(m["nv"])
    bq, bv = jm.states(name, 5)
    qr, vr = (-0.3 - 0.01 * np.arange(nv), 0.2 + 0.02 * np.arange(nv)), (-1.0, 2.0)
    seen = set()
    for e in range(40):
        q, v, a, k = er.reset_state(m, 99, e, 1, bank=(bq, bv, None), qpos_range=qr, qvel_range=vr, do_clamp=True)
        seen.add(k)
        assert np.all(np.isfinite(q)) and a.shape == (int(m.get("na", 0)),)
        assert np.all(v - bv[k] >= -1.0) and np.all(v - bv[k] <= 2.0)
        for j in range(int(m["njnt"])):
            ty, qa = int(m["jnt_type"][j]), int(m["jnt_qposadr"][j])
            if ty in (refdyn.JNT_FREE, refdyn.JNT_BALL):
                o = qa + (3 if ty == refdyn.JNT_FREE else 0)
                assert abs(np.linalg.norm(q[o:o + 4]) - 1) < 1e-14
                assert np.abs(q[o:o + 4] - bq[k][o:o + 4]).max() > 1e-3     # (the rotation draw moved it)
            elif int(m["jnt_limited"][j]):
                assert float(m["jnt_range"][j][0]) <= q[qa] <= float(m["jnt_range"][j][1])
        # without ranges the bank row comes back as it stands; without a bank, qpos0 and zeros
        q0, v0, _, k0 = er.reset_state(m, 99, e, 1, bank=(bq, bv, None))
        assert k0 == k and np.array_equal(q0, bq[k]) and np.array_equal(v0, bv[k])
        q1, v1, _, k1 = er.reset_state(m, 99, e, 1)
        assert k1 == -1 and np.array_equal(q1, np.asarray(m["qpos0"], float)) and not v1.any()
    assert seen == set(range(5))


def test_done_rule():
    time = np.array([0.0, 0.5, 1.0, 1.5, 0.2, 0.2])
    qpos = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [np.nan, 0.0], [0.0, 2.0]])
    assert list(er.done_rule(time, qpos, 1.0)) == [0, 0, 1, 1, 0, 0]
    assert list(er.done_rule(time, qpos, 0.0)) == [0] * 6
    assert list(er.done_rule(time, qpos, 0.0, box=([-1, -np.inf], [1, np.inf]))) == [0, 0, 0, 0, 1, 0]
    assert list(er.done_rule(time, qpos, 0.0, box=(None, [1, 1]))) == [0, 0, 0, 0, 1, 1]
    assert list(er.done_rule(time, qpos, 1.2, box=([-1, -1], None), extra=[1, 0, 0, 0, 0, 0])) == [1, 0, 0, 1, 1, 0]
    assert list(er.done_rule(np.zeros(3), np.zeros((3, 0)), 0.0, box=None, extra=[0, 2, 0])) == [0, 1, 0]


def test_episode_entry_points_are_declared_and_exported():
    """The C-ABI of the feature: each symbol in include/mjb.h, in binding.py's signature table and in libmjb.so."""
    import __graft_entry__ as g
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    lib = binding.load_library()
    declared = binding.header_symbols()
    for name in EPISODE_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mjb.h"
        assert name in lib._mjb_symbols, f"{name} has no signature in binding.py"
        assert hasattr(lib, name), f"libmjb.so does not export {name}"
    assert lib.mjb_episode_device_ptr.restype is C.c_void_p and lib.mjb_episode_set_noise.argtypes[1] is C.c_uint64
