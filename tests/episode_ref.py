"""Numpy reference of the device-side episode resets (mjb_episode_*, include/mjb.h): Philox-4x32-10, the uniform draws, the bank pick, the reset state and
the done rule, written from the header's text.  Nothing is shared with csrc/ or oracle/: the generator is the published algorithm (Salmon et al., SC11)
in numpy integers, the manifold update is refdyn.integrate_pos."""
import numpy as np

from mujoco_ros_pkgs_amd import refdyn

M0, M1 = 0xD2511F53, 0xCD9E8D57   # Philox-4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # Weyl increments of the key
STREAM = 0x80000000               # top bit of the fourth counter word: the episode stream
MASK32 = 0xFFFFFFFF


def philox4x32(ctr, key, rounds=10):
    """ctr [..., 4], key [..., 2] as unsigned integers -> the generator's four output words [..., 4] (uint64 arrays holding 32-bit values)."""
    c = np.array(np.broadcast_arrays(*[np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]), dtype=np.uint64)
    k0 = np.asarray(key, dtype=np.uint64)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint64)[..., 1].copy()
    c0, c1, c2, c3 = (c[i].copy() for i in range(4))
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0     # (32 x 32 bits: fits 64)
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & np.uint64(MASK32), p1 & np.uint64(MASK32), ((p0 >> np.uint64(32)) ^ c3 ^ k1) & np.uint64(MASK32), p0 & np.uint64(MASK32)
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK32)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK32)
    return np.stack([c0, c1, c2, c3], axis=-1)


def u(seed, genv, episode, idx):
    """(w0 + 0.5) / 2^32 of counter (genv lo32, genv hi32, episode, 0x80000000 + idx) under the key (seed lo32, seed hi32); broadcasts over genv / idx."""
    genv = np.asarray(genv, dtype=np.int64).astype(np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    genv, idx = np.broadcast_arrays(genv, idx)
    ctr = np.stack([genv & np.uint64(MASK32), genv >> np.uint64(32), np.full(genv.shape, int(episode), dtype=np.uint64), (np.uint64(STREAM) + idx) & np.uint64(MASK32)], axis=-1)
    key = np.array([int(seed) & MASK32, (int(seed) >> 32) & MASK32], dtype=np.uint64)
    w0 = philox4x32(ctr, key)[..., 0]
    return (w0.astype(np.float64) + 0.5) / 4294967296.0


def pick(seed, genv, episode, nv, ninit):
    """the bank row of the draw: min(ninit - 1, floor(u(2 nv) ninit))"""
    return int(min(ninit - 1, np.floor(float(u(seed, genv, episode, 2 * nv)) * ninit)))


def clamp(m, qpos):
    q = np.array(qpos, dtype=np.float64)
    for j in range(int(m["njnt"])):
        if int(m["jnt_type"][j]) in (refdyn.JNT_SLIDE, refdyn.JNT_HINGE) and int(m["jnt_limited"][j]):
            qa = int(m["jnt_qposadr"][j])
            q[qa] = min(max(q[qa], float(m["jnt_range"][j][0])), float(m["jnt_range"][j][1]))
    return q


def reset_state(m, seed, genv, episode, bank=None, qpos_range=None, qvel_range=None, do_clamp=False):
    """(qpos, qvel, act, picked row) of env `genv` reset at `episode`.  bank = (qpos [ninit, nq], qvel [ninit, nv] or None, act [ninit, na] or None) or None;
    the ranges are (lo [nv], hi [nv]) or None."""
    nq, nv, na = int(m["nq"]), int(m["nv"]), int(m.get("na", 0))
    k = -1
    q, v, a = np.asarray(m["qpos0"], dtype=np.float64).reshape(nq).copy(), np.zeros(nv), np.zeros(na)
    if bank is not None:
        k = pick(seed, genv, episode, nv, len(bank[0]))
        q = np.array(bank[0][k], dtype=np.float64).reshape(nq)
        v = np.zeros(nv) if bank[1] is None else np.array(bank[1][k], dtype=np.float64).reshape(nv)
        a = np.zeros(na) if bank[2] is None else np.array(bank[2][k], dtype=np.float64).reshape(na)
    if qpos_range is not None:
        lo, hi = (np.broadcast_to(np.asarray(x, dtype=np.float64), (nv,)) for x in qpos_range)
        dq = lo + (hi - lo) * u(seed, genv, episode, np.arange(nv))
        for j in range(int(m["njnt"])):   # (quat_integrate normalises the quaternion before it multiplies)
            ty, qa = int(m["jnt_type"][j]), int(m["jnt_qposadr"][j])
            if ty in (refdyn.JNT_FREE, refdyn.JNT_BALL):
                o = qa + (3 if ty == refdyn.JNT_FREE else 0)
                q[o:o + 4] /= np.linalg.norm(q[o:o + 4])
        q = refdyn.integrate_pos(m, q, dq, 1.0)
    if qvel_range is not None:
        lo, hi = (np.broadcast_to(np.asarray(x, dtype=np.float64), (nv,)) for x in qvel_range)
        v = v + (lo + (hi - lo) * u(seed, genv, episode, nv + np.arange(nv)))
    if do_clamp:
        q = clamp(m, q)
    return q, v, a, k


def done_rule(time, qpos, time_limit=0.0, box=None, extra=None):
    """uint8 [nenv]: time >= time_limit (when time_limit > 0), a coordinate with !(lo <= q <= hi), or the extra mask"""
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    n = time.size
    d = np.zeros(n, dtype=bool)
    if time_limit > 0:
        d |= time >= time_limit
    if box is not None and np.asarray(qpos).size:
        q = np.asarray(qpos, dtype=np.float64).reshape(n, -1)
        lo = np.full(q.shape[1], -np.inf) if box[0] is None else np.broadcast_to(np.asarray(box[0], dtype=np.float64), (q.shape[1],))
        hi = np.full(q.shape[1], np.inf) if box[1] is None else np.broadcast_to(np.asarray(box[1], dtype=np.float64), (q.shape[1],))
        with np.errstate(invalid="ignore"):
            d |= np.any(~((q >= lo) & (q <= hi)), axis=1)
    if extra is not None:
        d |= np.asarray(extra).reshape(-1) != 0
    return d.astype(np.uint8)


def rel_err(got, want):
    """the project's measure: max |got - want| / (1 + |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if got.size else 0.0
