"""A certificate of optimality for a solved constraint problem that shares no code with either solver: the KKT conditions of the dual

    min_f  1/2 f' (J M^-1 J' + diag R) f + f' (J qacc_smooth - aref)   over  f in K

(K: equality rows free, friction rows in [-frictionloss, frictionloss], limit / frictionless / pyramidal rows >= 0, elliptic contacts in
their friction cones).  With qacc = qacc_smooth + M^-1 J' f the dual gradient is g = J qacc - aref + R f; because R > 0 the problem is
strictly convex and the conditions below hold at exactly one point:

  * stationarity      M (qacc - qacc_smooth) = J' f
  * equality rows     g = 0
  * friction rows     |f| <= fl;  g <= 0 where f = +fl, g >= 0 where f = -fl, g = 0 strictly inside
  * one-sided rows    f >= 0, g >= 0, f g = 0
  * elliptic cones    y = f / (1, mu_1 ..), z = g (1, mu_1 ..):  |y_t| <= y_n, |z_t| <= z_n, y . z = 0

Every residual is made relative to the rounding scale of the quantity it tests: stationarity to 1 + |J' f|, a row's g to
sum_j |J_ij qacc_j| + |aref_i| + |R_i f_i|, forces to the largest force of the problem (friction rows: to their limit)."""
import numpy as np

from test_oracle_pins import dense_M

TINY = 1e-300
EQUALITY, FRICTION_DOF, FRICTION_TENDON, LIMIT_JOINT, LIMIT_TENDON, FRICTIONLESS, PYRAMIDAL, ELLIPTIC = range(8)


def kkt_certificate(model, M, J, R, aref, qacc_smooth, qacc, efc_force, efc_type, efc_frictionloss, contact_efc_address, contact_dim,
                    contact_friction, ncon):
    """The worst residual of each condition (a dict; 0 where the problem has no row of that kind).  M: nv x nv dense (or the packed qM),
    J: nefc x nv (or flat), the row arrays: nefc long; the contact arrays as mjData keeps them (contact_friction: 5 per contact)."""
    nv = int(model["nv"])
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = dense_M(model, M)
    f = np.asarray(efc_force, dtype=np.float64)
    n = len(f)
    J = np.asarray(J, dtype=np.float64)[:n * nv].reshape(n, nv).astype(np.longdouble)
    R, aref = np.asarray(R, dtype=np.float64)[:n], np.asarray(aref, dtype=np.float64)[:n]
    qacc, qacc_smooth = np.asarray(qacc, dtype=np.float64), np.asarray(qacc_smooth, dtype=np.float64)
    types = np.asarray(efc_type)[:n]
    fl = np.asarray(efc_frictionloss, dtype=np.float64)[:n]
    fL = f.astype(np.longdouble)
    jtf = J.T @ fL
    lhs = M.astype(np.longdouble) @ (qacc.astype(np.longdouble) - qacc_smooth)
    out = dict(stationarity=float(np.abs(lhs - jtf).max() / (1 + np.abs(jtf).max())) if nv else 0.0,
               equality=0.0, friction_box=0.0, friction_comp=0.0, sign=0.0, comp=0.0, cone_y=0.0, cone_z=0.0, cone_comp=0.0)
    if n == 0:
        return out
    jq = J @ qacc.astype(np.longdouble)
    g = jq - aref + R * fL
    sg = (np.abs(J) @ np.abs(qacc).astype(np.longdouble)) + np.abs(aref) + np.abs(R * f) + TINY
    rg = np.asarray(g / sg, dtype=np.float64)                  # g of each row relative to its rounding scale
    sf = max(float(np.abs(f).max()), TINY)

    def worst(x):
        return float(np.max(x)) if np.size(x) else 0.0

    eq = types == EQUALITY
    out["equality"] = worst(np.abs(rg[eq]))
    fr = (types == FRICTION_DOF) | (types == FRICTION_TENDON)
    if fr.any():
        lim = np.maximum(fl[fr], TINY)
        ff = f[fr]
        out["friction_box"] = worst(np.maximum(np.abs(ff) - lim, 0) / lim)
        # g > 0 only at the lower bound (f = -fl), g < 0 only at the upper one (f = +fl)
        out["friction_comp"] = worst(np.maximum(np.minimum(np.maximum(rg[fr], 0), (ff + lim) / lim),
                                                np.minimum(np.maximum(-rg[fr], 0), (lim - ff) / lim)))
    one = (types >= LIMIT_JOINT) & (types <= PYRAMIDAL)
    if one.any():
        out["sign"] = worst(np.maximum(np.maximum(-f[one] / sf, 0), np.maximum(-rg[one], 0)))
        out["comp"] = worst(np.minimum(np.abs(f[one]) / sf, np.abs(rg[one])))
    seen = np.zeros(n, dtype=bool)
    fric = np.asarray(contact_friction, dtype=np.float64)
    for c in range(int(ncon)):
        adr, dim = int(contact_efc_address[c]), int(contact_dim[c])
        if adr < 0 or dim <= 1 or types[adr] != ELLIPTIC:
            continue
        sl = slice(adr, adr + dim)
        assert np.all(types[sl] == ELLIPTIC) and not seen[sl].any(), f"contact {c}: rows {adr}..{adr + dim - 1} are not one elliptic cone"
        seen[sl] = True
        mu = np.concatenate([[1.0], fric[5 * c:5 * c + dim - 1]])
        y = f[sl] / mu
        z = np.asarray(g[sl], dtype=np.float64) * mu
        zs = float(np.linalg.norm(np.asarray(sg[sl], dtype=np.float64) * mu))
        ys = max(float(np.linalg.norm(y)), TINY)
        out["cone_y"] = max(out["cone_y"], max(float(np.linalg.norm(y[1:]) - y[0]), 0.0) / ys)
        out["cone_z"] = max(out["cone_z"], max(float(np.linalg.norm(z[1:]) - z[0]), 0.0) / zs)
        out["cone_comp"] = max(out["cone_comp"], abs(float(y @ z)) / (ys * zs))
    assert seen.sum() == np.count_nonzero(types == ELLIPTIC), "an elliptic row outside every contact's cone"
    return out


def oracle_certificate(model, d):
    """kkt_certificate of the oracle's solution in OracleData d (after forward())."""
    n, ncon = int(d.nefc[0]), int(d.ncon[0])
    return kkt_certificate(model, d.qM, d.efc_J, d.efc_R[:n], d.efc_aref[:n], d.qacc_smooth, d.qacc, d.efc_force[:n], d.efc_type[:n],
                           d.efc_frictionloss[:n], d.contact_efc_address[:ncon], d.contact_dim[:ncon], d.contact_friction, ncon)


def batch_certificate(model, got, e):
    """kkt_certificate of env e's solution as the engine dumped it: got[name] = Batch.get(name) for the fields of CERT_FIELDS."""
    n, ncon = int(got["nefc"][e, 0]), int(got["ncon"][e, 0])
    return kkt_certificate(model, got["qM"][e], got["efc_J"][e], got["efc_R"][e][:n], got["efc_aref"][e][:n], got["qacc_smooth"][e], got["qacc"][e],
                           got["efc_force"][e][:n], got["efc_type"][e][:n], got["efc_frictionloss"][e][:n], got["contact_efc_address"][e][:ncon],
                           got["contact_dim"][e][:ncon], got["contact_friction"][e], ncon)


CERT_FIELDS = ["qM", "efc_J", "efc_R", "efc_aref", "qacc_smooth", "qacc", "efc_force", "efc_type", "efc_frictionloss", "contact_efc_address",
               "contact_dim", "contact_friction", "nefc", "ncon"]

# bounds: stationarity by solver -- Newton converges to rounding (<= 1e-10 on the oracle); CG stops on its tolerance, and its residual in
# J' f is as large as the problem is stiff: on the oracle, 1e-5 - 1e-4 on the box grids at the default tolerance, up to 4e-4 on the welded
# chains of test_slot_scenes.py, which therefore run CG at tolerance 1e-12 (<= 2e-5 there).  Every other condition to rounding in both
# solvers: the forces are the primal's formulas of the final qacc, so they sit exactly on their zones (<= 3e-15 on the oracle).
STATIONARITY = {2: 1e-9, 1: 1e-4}   # (mjtSolver: 2 Newton, 1 CG)
ROUNDING = 1e-9


def assert_certified(cert, model, what=""):
    bound = STATIONARITY[int(model["solver"])]
    bad = {k: v for k, v in cert.items() if v > (bound if k == "stationarity" else ROUNDING)}
    assert not bad, f"{what}: KKT residuals beyond their bounds {bad} (all: {cert})"
