"""The reference of the batched contact wrenches (Batch.set_contact_queries / contact_wrenches, csrc/mjb_contact.hip): plain numpy on the nine frame fields
a caller would otherwise copy to the host -- ncon, contact_geom, contact_dim, contact_efc_address, contact_frame, contact_pos, contact_dist,
contact_friction and efc_force of ONE env, as Batch.get or the oracle serve them (flat or shaped).  It shares nothing with the kernel.  No tests here.

decode restates mj_contactForce; world turns a local wrench into the world force and the world torque at contact_pos; query does the sums of one
(A, B) query.  tools/contact_wrench_rate.py times decode + query as the host route."""
import numpy as np

FIELDS = ("ncon", "contact_geom", "contact_dim", "contact_efc_address", "contact_frame", "contact_pos", "contact_dist", "contact_friction", "efc_force")
PYRAMIDAL, ELLIPTIC = 0, 1


def shaped(fields):
    """the nine fields of one env with their shapes: contact_geom [nconmax, 2], contact_frame [nconmax, 3, 3] (row k = axis k, the normal first), ..."""
    f = {k: np.asarray(fields[k]) for k in FIELDS}
    n = f["contact_dim"].size
    return dict(ncon=int(np.ravel(f["ncon"])[0]), geom=f["contact_geom"].reshape(n, 2).astype(int), dim=f["contact_dim"].reshape(n).astype(int),
                adr=f["contact_efc_address"].reshape(n).astype(int), frame=f["contact_frame"].reshape(n, 3, 3).astype(float),
                pos=f["contact_pos"].reshape(n, 3).astype(float), dist=f["contact_dist"].reshape(n).astype(float),
                friction=f["contact_friction"].reshape(n, 5).astype(float), force=f["efc_force"].reshape(-1).astype(float))


def decode(fields, cone):
    """(lf [nconmax, 6], active [nconmax] bool): mj_contactForce of every contact in its own frame, the normal first; zero rows, and active False, for
    c >= ncon and for contacts without constraint rows (contact_efc_address < 0)."""
    s = shaped(fields)
    n = s["dim"].size
    lf, active = np.zeros((n, 6)), np.zeros(n, bool)
    for c in range(s["ncon"]):
        adr, dim = s["adr"][c], s["dim"][c]
        if adr < 0:
            continue
        active[c] = True
        if dim == 1:
            lf[c, 0] = s["force"][adr]
        elif cone == ELLIPTIC:
            lf[c, :dim] = s["force"][adr:adr + dim]
        else:
            edges = s["force"][adr:adr + 2 * (dim - 1)].reshape(dim - 1, 2)   # the two opposing edges of every friction direction
            lf[c, 0] = edges.sum()
            lf[c, 1:dim] = (edges[:, 0] - edges[:, 1]) * s["friction"][c, :dim - 1]
    return lf, active


def world(fields, lf):
    """(F [nconmax, 3], T [nconmax, 3]): the world force and the world torque at contact_pos of every local wrench: sum_k lf[k] axis_k"""
    fr = shaped(fields)["frame"]
    return np.einsum("ck,ckx->cx", lf[:, :3], fr), np.einsum("ck,ckx->cx", lf[:, 3:], fr)


def query(fields, A, B, ref=None, cone=PYRAMIDAL):
    """dict(wrench [6], normal, count, dist, signs [nconmax]) of one query: A, B geom id sets (B None: every geom not in A), ref the point the torque is
    taken about (None: the world origin).  A contact (g1, g2) counts with +1 when g2 is in A and g1 in B, with -1 when g1 is in A and g2 in B; the
    wrench is what the B side exerts on the A side."""
    s = shaped(fields)
    lf, active = decode(fields, cone)
    F, T = world(fields, lf)
    A = set(int(g) for g in A)
    inB = (lambda g: g not in A) if B is None else (lambda g, Bs=set(int(g) for g in B): g in Bs)
    r = np.zeros(3) if ref is None else np.asarray(ref, float)
    wrench, normal, count, dist = np.zeros(6), 0.0, 0, np.inf
    signs = np.zeros(s["dim"].size, int)
    for c in range(s["ncon"]):
        if not active[c]:
            continue
        g1, g2 = s["geom"][c]
        sign = 1 if (g2 in A and inB(g1)) else (-1 if (g1 in A and inB(g2)) else 0)
        if sign == 0:
            continue
        signs[c] = sign
        wrench[:3] += sign * F[c]
        wrench[3:] += sign * (T[c] + np.cross(s["pos"][c] - r, F[c]))
        normal += lf[c, 0]
        count += 1
        dist = min(dist, s["dist"][c])
    return dict(wrench=wrench, normal=normal, count=count, dist=dist, signs=signs)


def env_fields(batch_fields, e):
    """one env's fields out of per-field arrays [nenv, ...]"""
    return {k: batch_fields[k][e] for k in FIELDS}
