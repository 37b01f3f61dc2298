"""An independent reference of the parameters of a constraint row: K, B, imp, imp', R, D and aref, in 50-digit decimal arithmetic.

It restates the documented definitions (MuJoCo's computation chapter, "Solver parameters", 2.3.7) and shares no code with oracle/ or csrc/:

  getsolparam   a solref with exactly one positive number is replaced by (0.02, 1); with refsafe, a positive solref[0] is at least
                2 timestep; solimp's d0, dwidth and midpoint are clamped to [1e-4, 0.9999], its width to >= 0, its power to >= 1
  impedance     x = |pos - margin| / width;  d(x) = d0 + y(x) (dwidth - d0),  y = x^p / mid^(p-1) for x <= mid and
                1 - (1-x)^p / (1-mid)^(p-1) above;  d0 at x <= 0, dwidth at x >= 1;  the mean of the two where d0 == dwidth or width <= 1e-15
  gains         solref > 0: K = 1 / (dmax^2 timeconst^2 dampratio^2), B = 2 / (dmax timeconst);  solref <= 0: K = -solref0 / dmax^2, B = -solref1 / dmax
  R             max(1e-15, (1 - imp) diagApprox / imp),  D = 1 / R,  aref = -B vel - K imp (pos - margin)
  contact mix   the higher priority wins; else mix = s1 / (s1 + s2) (0.5 / 0 / 1 where a solmix is < 1e-15); solref mixed where both
                first numbers are positive, else the element-wise minimum; solimp always mixed

expected_rows() derives every row's parameters from what the row is (its type, id, position, margin, velocity and its contact), not from
how some engine built it.  `mut` names a deliberate mistake (MUTATIONS): tests use it to show that their inputs tell right from wrong."""
from decimal import Decimal, getcontext

import numpy as np

getcontext().prec = 50

EQUALITY, FRICTION_DOF, FRICTION_TENDON, LIMIT_JOINT, LIMIT_TENDON, FRICTIONLESS, PYRAMIDAL, ELLIPTIC = range(8)
EQ_CONNECT, EQ_WELD, EQ_JOINT, EQ_TENDON = range(4)
REFSAFE_BIT = 1 << 11   # mjDSBL_REFSAFE
MINVAL = Decimal("1e-15")
MINIMP, MAXIMP = Decimal("0.0001"), Decimal("0.9999")

MUTATIONS = ("power2", "swap_sides", "no_refsafe", "no_clamps", "no_fallback", "mix_half", "mix_not_min", "impratio1", "diag_no_friction",
             "friction_at_dist", "eq_per_row")

# impedance branches, as the coverage counters name them
BRANCHES = ("flat", "x<=0", "x>=1", "below", "above", "power1", "power2", "power_other")


def D(x):
    """Exact decimal value of a binary double."""
    return Decimal(float(x))


def _clip(x, lo, hi):
    return min(hi, max(lo, x))


def solparam(solref, solimp, timestep, refsafe, mut=()):
    r0, r1 = D(solref[0]), D(solref[1])
    if (r0 > 0) != (r1 > 0) and "no_fallback" not in mut:
        r0, r1 = Decimal("0.02"), Decimal(1)
    if refsafe and r0 > 0 and "no_refsafe" not in mut:
        r0 = max(r0, 2 * D(timestep))
    s = [D(v) for v in solimp]
    if "no_clamps" not in mut:
        s = [_clip(s[0], MINIMP, MAXIMP), _clip(s[1], MINIMP, MAXIMP), max(Decimal(0), s[2]), _clip(s[3], MINIMP, MAXIMP), max(Decimal(1), s[4])]
    if "power2" in mut:
        s[4] = Decimal(2)
    return (r0, r1), s


def impedance(solimp, pos, margin, mut=(), branch=None):
    """(imp, imp') of clamped solimp at pos, margin.  `branch`: a list that receives the names of the branches taken."""
    d0, dw, width, mid, power = solimp
    note = branch.append if branch is not None else (lambda b: None)
    if d0 == dw or width <= MINVAL:
        note("flat")
        return (d0 + dw) / 2, Decimal(0)
    s = D(pos) - D(margin)
    x = abs(s) / width
    if x <= 0:
        note("x<=0")
        return d0, Decimal(0)
    if x >= 1:
        note("x>=1")
        return dw, Decimal(0)
    note("power1" if power == 1 else ("power2" if power == 2 else "power_other"))
    if power == 1:
        y, yp = x, Decimal(1)
    else:
        below = x <= mid
        note("below" if below else "above")
        if "swap_sides" in mut:
            below = not below
        if below:
            a = 1 / mid ** (power - 1)
            y, yp = a * x ** power, power * a * x ** (power - 1)
        else:
            b = 1 / (1 - mid) ** (power - 1)
            y, yp = 1 - b * (1 - x) ** power, power * b * (1 - x) ** (power - 1)
    sign = 1 if s > 0 else -1
    return d0 + y * (dw - d0), yp * sign * (dw - d0) / width


def gains(solref, dmax):
    r0, r1 = solref
    if r0 > 0:
        return 1 / max(MINVAL, dmax * dmax * r0 * r0 * r1 * r1), 2 / max(MINVAL, dmax * r0)
    return -r0 / max(MINVAL, dmax * dmax), -r1 / max(MINVAL, dmax)


def R(imp, diag_approx):
    return max(MINVAL, (1 - imp) * D(diag_approx) / imp)


def contact_param(model, g1, g2, mut=()):
    """(solref[2], solimp[5]) of a contact between geoms g1 and g2 as the two geoms give it, in decimals."""
    ref = [[D(v) for v in np.asarray(model["geom_solref"]).reshape(-1, 2)[g]] for g in (g1, g2)]
    imp = [[D(v) for v in np.asarray(model["geom_solimp"]).reshape(-1, 5)[g]] for g in (g1, g2)]
    p1, p2 = int(model["geom_priority"][g1]), int(model["geom_priority"][g2])
    if p1 != p2:
        k = 0 if p1 > p2 else 1
        return ref[k], imp[k]
    s1, s2 = D(model["geom_solmix"][g1]), D(model["geom_solmix"][g2])
    if s1 >= MINVAL and s2 >= MINVAL:
        mix = s1 / (s1 + s2)
    elif s1 < MINVAL and s2 < MINVAL:
        mix = Decimal("0.5")
    else:
        mix = Decimal(0) if s1 < MINVAL else Decimal(1)
    if "mix_half" in mut:
        mix = Decimal("0.5")
    if (ref[0][0] > 0 and ref[1][0] > 0) or "mix_not_min" in mut:
        solref = [mix * a + (1 - mix) * b for a, b in zip(*ref)]
    else:
        solref = [min(a, b) for a, b in zip(*ref)]
    return solref, [mix * a + (1 - mix) * b for a, b in zip(*imp)]


def pair_param(model, g1, g2, mut=()):
    """contact_param with what a <contact><pair> of the two geoms states on top (collpair_param: friction[5] solref[2] solimp[5] margin gap,
    NaN where the pair does not state it)."""
    solref, solimp = contact_param(model, g1, g2, mut)
    pairs = np.asarray(model["collpair_geom"]).reshape(-1, 2)
    for p in range(len(pairs)):
        if model["collpair_explicit"][p] and {int(pairs[p, 0]), int(pairs[p, 1])} == {int(g1), int(g2)}:
            pp = np.asarray(model["collpair_param"]).reshape(-1, 14)[p]
            if not np.isnan(pp[5]):
                solref = [D(pp[5]), D(pp[6])]
            if not np.isnan(pp[7]):
                solimp = [D(v) for v in pp[7:12]]
    return solref, solimp


def _row(model, solref, solimp, pos, margin, vel, diag, mut, branch, ipos=None, imargin=None):
    """[K, B, imp, imp', R, D, aref] of one row; the impedance is evaluated at (ipos, imargin) where that differs from the row's own."""
    refsafe = not (int(model["disableflags"]) & REFSAFE_BIT)
    sr, si = solparam(solref, solimp, float(np.asarray(model["timestep"]).ravel()[0]), refsafe, mut)
    imp, impP = impedance(si, pos if ipos is None else ipos, margin if imargin is None else imargin, mut, branch)
    K, B = gains(sr, si[1])
    r = R(imp, diag)
    return [K, B, imp, impP, r, 1 / r, -B * D(vel) - K * imp * (D(pos) - D(margin))]


def expected_rows(model, fields, mut=(), branches=None):
    """Expected parameters of every row of one env.  fields: nefc, efc_type, efc_id, efc_pos, efc_margin, efc_vel, contact_geom, contact_dim,
    contact_friction, contact_dist, contact_includemargin (flat arrays as the frame keeps them).  Returns a dict of float64 arrays
    efc_KBIP [nefc, 4], efc_R, efc_D, efc_aref [nefc], contact_solref [ncon_used, 2], contact_solimp [ncon_used, 5] (NaN for a contact no
    row refers to) -- and fills `branches` (a list, one list of branch names per row) when given."""
    mut = frozenset(mut)
    assert mut <= set(MUTATIONS), mut
    n = int(np.asarray(fields["nefc"]).ravel()[0])
    typ, ids = np.asarray(fields["efc_type"])[:n], np.asarray(fields["efc_id"])[:n]
    pos, margin, vel = (np.asarray(fields[k], dtype=np.float64)[:n] for k in ("efc_pos", "efc_margin", "efc_vel"))
    dofw, tenw = np.asarray(model["dof_invweight0"]), np.asarray(model.get("tendon_invweight0", np.zeros(0)))
    bodyw = np.asarray(model["body_invweight0"]).reshape(-1, 2)
    arr = lambda name, w: np.asarray(model[name]).reshape(-1, w)
    impratio = Decimal(1) if "impratio1" in mut else max(MINVAL, D(np.asarray(model["impratio"]).ravel()[0]))
    out = [None] * n
    ncon = 1 + int(max([ids[i] for i in range(n) if typ[i] >= FRICTIONLESS], default=-1))
    csolref, csolimp = np.full((ncon, 2), np.nan), np.full((ncon, 5), np.nan)
    notes = [[] for _ in range(n)]
    i = 0
    while i < n:
        t, k = int(typ[i]), int(ids[i])
        j = i
        while j < n and typ[j] == t and ids[j] == k and (t == EQUALITY or t >= FRICTIONLESS):
            j += 1   # the rows of one equality or one contact
        j = max(j, i + 1)
        rows = range(i, j)
        if t == EQUALITY:
            et, o1, o2 = int(model["eq_type"][k]), int(model["eq_obj1id"][k]), int(model["eq_obj2id"][k])
            nrm = sum(D(pos[r]) ** 2 for r in rows).sqrt()
            for q, r in enumerate(rows):
                if et in (EQ_CONNECT, EQ_WELD):
                    diag = D(bodyw[o1, q // 3]) + D(bodyw[o2, q // 3])
                elif et == EQ_JOINT:
                    diag = D(dofw[model["jnt_dofadr"][o1]]) + (D(dofw[model["jnt_dofadr"][o2]]) if o2 >= 0 else 0)
                else:
                    diag = D(tenw[o1]) + (D(tenw[o2]) if o2 >= 0 else 0)
                shared = len(rows) > 1 and "eq_per_row" not in mut
                out[r] = _row(model, arr("eq_solref", 2)[k], arr("eq_solimp", 5)[k], pos[r], 0.0, vel[r], diag, mut, notes[r],
                              ipos=nrm if shared else None)
        elif t in (FRICTION_DOF, FRICTION_TENDON):
            sr, si, w = (("dof_solref", "dof_solimp", dofw) if t == FRICTION_DOF else ("tendon_solref_fri", "tendon_solimp_fri", tenw))
            out[i] = _row(model, arr(sr, 2)[k], arr(si, 5)[k], 0.0, 0.0, vel[i], w[k], mut, notes[i])
        elif t == LIMIT_JOINT:
            out[i] = _row(model, arr("jnt_solref", 2)[k], arr("jnt_solimp", 5)[k], pos[i], margin[i], vel[i], dofw[model["jnt_dofadr"][k]], mut, notes[i])
        elif t == LIMIT_TENDON:
            out[i] = _row(model, arr("tendon_solref_lim", 2)[k], arr("tendon_solimp_lim", 5)[k], pos[i], margin[i], vel[i], tenw[k], mut, notes[i])
        else:
            g1, g2 = (int(g) for g in np.asarray(fields["contact_geom"])[2 * k:2 * k + 2])
            solref, solimp = pair_param(model, g1, g2, mut)
            csolref[k], csolimp[k] = [float(v) for v in solref], [float(v) for v in solimp]
            fri = [D(v) for v in np.asarray(fields["contact_friction"])[5 * k:5 * k + 5]]
            dist, inc = fields["contact_dist"][k], fields["contact_includemargin"][k]
            b1, b2 = int(model["geom_bodyid"][g1]), int(model["geom_bodyid"][g2])
            tran = D(bodyw[b1, 0]) + D(bodyw[b2, 0])
            mu2 = fri[0] * fri[0] / impratio
            if t == FRICTIONLESS:
                out[i] = _row(model, solref, solimp, dist, inc, vel[i], tran, mut, notes[i])
            elif t == PYRAMIDAL:
                diag = tran if "diag_no_friction" in mut else tran * (1 + fri[0] * fri[0])
                for r in rows:
                    out[r] = _row(model, solref, solimp, dist, inc, vel[r], diag, mut, notes[r])
                    out[r][4] = max(MINVAL, 2 * mu2 * out[r][4])
                    out[r][5] = 1 / out[r][4]
            else:
                out[i] = _row(model, solref, solimp, dist, inc, vel[i], tran, mut, notes[i])
                for q, r in enumerate(rows):
                    if q == 0:
                        continue
                    at = (dist, inc) if "friction_at_dist" in mut else (0.0, 0.0)
                    out[r] = _row(model, solref, solimp, 0.0, 0.0, vel[r], tran, mut, notes[r], ipos=at[0], imargin=at[1])
                    out[r][4] = max(MINVAL, out[i][4] * mu2 / (fri[q - 1] * fri[q - 1]))
                    out[r][5] = 1 / out[r][4]
        i = j
    if branches is not None:
        branches.extend(notes)
    f = np.array([[float(v) for v in row] for row in out], dtype=np.float64).reshape(n, 7)
    return dict(efc_KBIP=f[:, :4].copy(), efc_R=f[:, 4].copy(), efc_D=f[:, 5].copy(), efc_aref=f[:, 6].copy(),
                contact_solref=csolref, contact_solimp=csolimp)
