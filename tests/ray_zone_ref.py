"""An independent reference for the two sensors that intersect a ray with a shape, rangefinder and touch (test_ray_zone_sensors.py,
test_gpu_ray_zone_sensors.py): no tests here.

numpy longdouble only.  Nothing is shared with oracle/ or csrc/, and the derivation differs from theirs: no per-primitive quadratic, no slab
formula.  A shape is its exact signed distance, written from its definition in the shape's own frame:

    sphere   |q| - r
    capsule  |q - clamp(q_z, -h, h) e_z| - r                        (a segment plus a radius)
    box      |max(d, 0)| + min(max(d_x, d_y, d_z), 0),  d = |q| - s

All three are convex, so  t -> sdf(p + t v)  is convex along a ray: a golden-section search finds its minimiser t* on [0, tmax]; the ray meets
the shape iff it starts inside or sdf(p + t* v) <= 0, and the surface crossing is bracketed -- by [0, tmax] for a start inside (the exit), by
[0, t*] otherwise (the entry) -- and bisected.  min sdf is returned with every answer: where |min sdf| is at the rounding level the decision is a
tie that the tests exclude.

The plane is stated from its contract: it is hit from the front only (local z >= 0 and v_z < 0) and only where the crossing point lies inside
|x| <= size0, |y| <= size1, a size of 0 meaning unbounded.

Every function takes one ray (p, v of shape [3]) or N rays ([N, 3]) and answers in kind."""
import numpy as np

LD = np.longdouble
PLANE, SPHERE, CAPSULE, BOX = 0, 2, 3, 6
CONTACT_FRICTIONLESS, CONTACT_PYRAMIDAL, CONTACT_ELLIPTIC = 5, 6, 7
GOLD = (np.sqrt(LD(5)) - 1) / 2
N_GOLD = 64       # 0.618^64 = 4e-14 of the bracket: beyond sqrt(eps) = 3e-10 the minimum's VALUE no longer moves (it is flat to second order)
N_BISECT = 72     # 2^-72 of the bracket: below longdouble's 1.1e-19

# What a wrong implementation would compute: the tests show that their inputs tell each of these from the contract.
MUTATIONS = {
    "flip_body2": "touch: the contact normal is not negated when the sensor's body is geom2's",
    "flip_always": "touch: the contact normal is negated for either role",
    "inside_only": "touch: only a contact point inside the zone counts, the ray is ignored",
    "first_row_pyramidal": "touch: a pyramidal contact's normal force is its first row, not the sum of its rows",
    "count_nonpositive": "touch: contacts whose normal force is not positive are added too",
    "skip_exclusion": "rangefinder: the geoms of the site's own body are hit",
    "see_invisible": "rangefinder: geoms with alpha 0 are hit",
    "entry_only": "rangefinder: a ray that starts inside a geom misses it",
    "cylinder_only": "rangefinder: a capsule is its cylinder, the caps are not there",
    "clamp_miss": "rangefinder: the -1 of a miss is clamped to the cutoff like a hit",
}


def _check_mut(mut):
    if mut is not None and mut not in MUTATIONS:
        raise ValueError(f"unknown mutation {mut}")


def _ld(a):
    return np.asarray(a, dtype=LD)


def _norm(q):
    return np.sqrt((q * q).sum(-1))


def sdf(kind, size, q):
    """Exact signed distance of the local points q [..., 3] to the shape (size [3] or [..., 3]); negative inside."""
    size, q = _ld(size), _ld(q)
    if kind == SPHERE:
        return _norm(q) - size[..., 0]
    if kind == CAPSULE:
        h = size[..., 1]
        z = np.minimum(np.maximum(q[..., 2], -h), h)
        return np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2 + (q[..., 2] - z) ** 2) - size[..., 0]
    if kind == BOX:
        d = np.abs(q) - size[..., :3]
        return _norm(np.maximum(d, 0)) + np.minimum(d.max(-1), 0)
    if kind == "cylinder":   # (the "cylinder_only" mutation: the capsule's radius about its whole axis)
        return np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - size[..., 0]
    raise ValueError(f"no signed distance for shape {kind}")


def _reach(kind, size):
    """A radius about the shape's centre that holds all of it."""
    size = _ld(size)
    if kind == SPHERE:
        return size[..., 0]
    if kind == CAPSULE:
        return size[..., 0] + size[..., 1]
    return _norm(size[..., :3])


def _minimise(f, tmax):
    """Golden-section search: (t*, f(t*)) of a convex f over [0, tmax], elementwise."""
    a, b = np.zeros_like(tmax), tmax.copy()
    c, d = b - GOLD * (b - a), a + GOLD * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(N_GOLD):
        left = fc < fd
        a, b = np.where(left, a, c), np.where(left, d, b)
        # (one new evaluation per round would do; both are recomputed: N is small and the code stays plain)
        c, d = b - GOLD * (b - a), a + GOLD * (b - a)
        fc, fd = f(c), f(d)
    t = np.stack([a, c, d, b, np.zeros_like(a), tmax])
    ft = np.stack([f(x) for x in t])
    k = ft.argmin(0)
    return np.take_along_axis(t, k[None], 0)[0], np.take_along_axis(ft, k[None], 0)[0]


def _bisect(f, lo, hi, rising):
    """The sign change of f between lo and hi, elementwise; rising: f(lo) <= 0 < f(hi), else f(lo) > 0 >= f(hi).  Returns the end where f <= 0."""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(N_BISECT):
        mid = (lo + hi) / 2
        inside = f(mid) <= 0
        go_up = inside == rising           # the crossing lies above mid
        lo, hi = np.where(go_up, mid, lo), np.where(go_up, hi, mid)
    return np.where(rising, lo, hi)


def local_ray(pos, mat, p, v):
    """The ray in the shape's frame.  mat: [9] or [3, 3] (row-major, its columns the shape's axes in the world), or with a leading [N]."""
    pos, mat, p, v = _ld(pos), _ld(mat), _ld(p), _ld(v)
    if mat.shape[-1] == 9:
        mat = mat.reshape(mat.shape[:-1] + (3, 3))
    # local = mat^T (world - pos)
    lp = np.einsum("...ji,...j->...i", mat, p - pos)
    lv = np.einsum("...ji,...j->...i", mat, v)
    return lp, lv


def _ray_convex(kind, size, lp, lv, entry_only=False):
    """(distance or -1, min sdf along the ray, the ray starts inside) for local rays lp + t lv [N, 3]."""
    size = np.broadcast_to(_ld(size), lp.shape[:-1] + (_ld(size).shape[-1],))
    speed = _norm(lv)
    tmax = (_norm(lp) + _reach(kind if kind != "cylinder" else CAPSULE, size) + 1) / speed

    def f(t):
        return sdf(kind, size, lp + t[..., None] * lv)
    tstar, fmin = _minimise(f, tmax)
    start = f(np.zeros_like(tmax))
    inside = start <= 0
    hit = inside | (fmin <= 0)
    # one bisection serves both cases: exit on [0, tmax] for a start inside, entry on [0, t*] otherwise
    lo = np.zeros_like(tmax)
    hi = np.where(inside, tmax, tstar)
    x = _bisect(f, lo, hi, inside)
    dist = np.where(hit, x, LD(-1))
    if entry_only:
        dist = np.where(inside, LD(-1), dist)
    return dist, np.minimum(fmin, start), inside


def _ray_plane(size, lp, lv):
    """(distance or -1, margin): margin is how far the decision is from flipping (parallel, behind, or at an edge of the extent)."""
    size = np.broadcast_to(_ld(size), lp.shape[:-1] + (_ld(size).shape[-1],))
    front = (lp[..., 2] >= 0) & (lv[..., 2] < 0)
    vz = np.where(lv[..., 2] < 0, lv[..., 2], LD(-1))
    t = np.where(front, -lp[..., 2] / vz, LD(0))
    x, y = lp[..., 0] + t * lv[..., 0], lp[..., 1] + t * lv[..., 1]
    in_x = (size[..., 0] <= 0) | (np.abs(x) <= size[..., 0])
    in_y = (size[..., 1] <= 0) | (np.abs(y) <= size[..., 1])
    big = LD(1e30)
    edge = np.minimum(np.where(size[..., 0] > 0, np.abs(np.abs(x) - size[..., 0]), big), np.where(size[..., 1] > 0, np.abs(np.abs(y) - size[..., 1]), big))
    margin = np.minimum(np.minimum(np.abs(lp[..., 2]), np.abs(lv[..., 2]) / _norm(lv)), np.where(front, edge, big))
    return np.where(front & in_x & in_y, t, LD(-1)), margin


def _ray_shape(kind, size, lp, lv, mut=None):
    """(distance or -1, grazing measure) of local rays against one kind of shape: the one place that knows the shapes and the shape mutations."""
    if kind == PLANE:
        return _ray_plane(size, lp, lv)
    if kind == CAPSULE and mut == "cylinder_only":   # the radius about the whole axis, kept where the hit lies between the caps' centres
        size = np.broadcast_to(_ld(size), lp.shape[:-1] + (_ld(size).shape[-1],))
        dist, graze, _ = _ray_convex("cylinder", size, lp, lv)
        z = lp[..., 2] + dist * lv[..., 2]
        return np.where((dist >= 0) & (np.abs(z) <= size[..., 1]), dist, LD(-1)), graze
    dist, graze, _ = _ray_convex(int(kind), size, lp, lv, entry_only=(mut == "entry_only"))
    return dist, graze


def ray_distance(kind, size, pos, mat, p, v, mut=None):
    """Distance t >= 0 along p + t v to the shape of type `kind` and `size` at world pose (pos, mat), or -1 for no hit; and the grazing measure
    (min sdf along the ray for the convex shapes -- for a plane, how far the decision is from flipping).  A ray that starts inside a convex shape
    leaves through its far surface: the exit's distance.  p, v: [3] or [N, 3]."""
    _check_mut(mut)
    single = np.ndim(p) == 1
    lp, lv = local_ray(pos, mat, np.atleast_2d(_ld(p)), np.atleast_2d(_ld(v)))
    dist, graze = _ray_shape(kind, size, lp, lv, mut)
    return (dist[0], graze[0]) if single else (dist, graze)


def rangefinder(model, geom_xpos, geom_xmat, site_xpos, site_xmat, site, size=None, type=None, cutoff=0.0, mut=None):
    """The rangefinder on `site`: the ray runs from the site's position along its z axis; the reading is the nearest non-negative hit over all
    geoms except those on the site's body and those with rgba[3] == 0, -1 if there is none.  A positive cutoff clamps hits only: -1 stays -1.

    geom_xpos [ngeom, 3], geom_xmat [ngeom, 9], site_xpos [nsite, 3], site_xmat [nsite, 9] of one state, or each with a leading [N] for N states;
    size [ngeom, 3] / type [ngeom] (or [N, ..]) override the model's per state.  Returns (reading, graze): graze is the smallest grazing measure
    over the geoms looked at (ray_distance)."""
    _check_mut(mut)
    ngeom, nsite = int(model["ngeom"]), int(model["nsite"])
    gp = _ld(geom_xpos).reshape(-1, ngeom, 3)
    single = gp.shape[0] == 1   # (one state answers with scalars, also when it came with a leading [1])
    n = gp.shape[0]
    gm = _ld(geom_xmat).reshape(n, ngeom, 3, 3)
    sp = _ld(site_xpos).reshape(n, nsite, 3)[:, site]
    sm = _ld(site_xmat).reshape(n, nsite, 3, 3)[:, site]
    gsize = np.broadcast_to(_ld(model["geom_size"] if size is None else size).reshape(-1, ngeom, 3), (n, ngeom, 3))
    gtype = np.broadcast_to(np.asarray(model["geom_type"] if type is None else type, dtype=int).reshape(-1, ngeom), (n, ngeom))
    axis = sm[:, :, 2]
    best = np.full(n, LD(-1))
    graze = np.full(n, LD(1e30))
    for g in range(ngeom):
        if int(model["geom_bodyid"][g]) == int(model["site_bodyid"][site]) and mut != "skip_exclusion":
            continue
        if float(model["geom_rgba"][g][3]) == 0 and mut != "see_invisible":
            continue
        for kind in np.unique(gtype[:, g]):
            sel = np.nonzero(gtype[:, g] == kind)[0]
            lp, lv = local_ray(gp[sel, g], gm[sel, g], sp[sel], axis[sel])
            d, gz = _ray_shape(int(kind), gsize[sel, g], lp, lv, mut)
            take = (d >= 0) & ((best[sel] < 0) | (d < best[sel]))
            best[sel] = np.where(take, d, best[sel])
            graze[sel] = np.minimum(graze[sel], np.abs(gz))
    cutoff = LD(cutoff)
    if cutoff > 0:
        best = np.where((best >= 0) | (mut == "clamp_miss"), np.minimum(np.maximum(best, -cutoff), cutoff), best)
    return (best[0], graze[0]) if single else (best, graze)


def ray_meets_zone(site_type, site_size, site_xpos, site_xmat, p, dir):
    """Does the ray p + t dir, t >= 0, meet the site's volume (sphere or box)?  True if sdf(p) <= 0 or min_{t >= 0} sdf <= 0.
    Returns (meets, that minimum, "inside" / "ray" / "miss").  p, dir: [3] or [N, 3]."""
    single = np.ndim(p) == 1
    lp, lv = local_ray(site_xpos, site_xmat, np.atleast_2d(_ld(p)), np.atleast_2d(_ld(dir)))
    size = np.broadcast_to(_ld(site_size), lp.shape[:-1] + (3,))
    kind = int(site_type)
    tmax = (_norm(lp) + _reach(kind, size) + 1) / _norm(lv)

    def f(t):
        return sdf(kind, size, lp + t[..., None] * lv)
    start = f(np.zeros_like(tmax))
    _, fmin = _minimise(f, tmax)
    fmin = np.minimum(fmin, start)
    case = np.where(start <= 0, "inside", np.where(fmin <= 0, "ray", "miss"))
    meets = fmin <= 0
    return (bool(meets[0]), fmin[0], str(case[0])) if single else (meets, fmin, case)


def touch_detail(model, dump, sensor, mut=None, opposite=True):
    """One record per contact of the dump that involves the touch sensor's body and has constraint rows: dict(contact, role (1: the body owns the
    contact's geom1, 2: geom2), force (its normal force), meets, min_sdf, case (ray_meets_zone), counted and -- with `opposite` -- meets_opposite
    (the same with the ray reversed).  `dump` maps field names to one state's arrays (the oracle's fields, or one env's rows of Batch.get)."""
    _check_mut(mut)
    m = model
    site = int(m["sensor_objid"][sensor])
    body = int(m["site_bodyid"][site])
    ncon = int(np.asarray(dump["ncon"]).reshape(-1)[0])
    cgeom = np.asarray(dump["contact_geom"], dtype=int).reshape(-1, 2)
    cpos = _ld(dump["contact_pos"]).reshape(-1, 3)
    cframe = _ld(dump["contact_frame"]).reshape(-1, 9)
    cdim = np.asarray(dump["contact_dim"], dtype=int).reshape(-1)
    cadr = np.asarray(dump["contact_efc_address"], dtype=int).reshape(-1)
    etype = np.asarray(dump["efc_type"], dtype=int).reshape(-1)
    eforce = _ld(dump["efc_force"]).reshape(-1)
    zpos = _ld(dump["site_xpos"]).reshape(-1, 3)[site]
    zmat = _ld(dump["site_xmat"]).reshape(-1, 3, 3)[site]
    rec = []
    for c in range(ncon):
        if cadr[c] < 0:
            continue
        b1, b2 = int(m["geom_bodyid"][cgeom[c, 0]]), int(m["geom_bodyid"][cgeom[c, 1]])
        if body != b1 and body != b2:
            continue
        a = cadr[c]
        if etype[a] == CONTACT_PYRAMIDAL and mut != "first_row_pyramidal":
            force = eforce[a:a + 2 * (cdim[c] - 1)].sum()
        else:
            force = eforce[a]
        role = 2 if body == b2 else 1
        sign = -1 if role == 2 else 1
        if mut == "flip_body2":
            sign = 1
        elif mut == "flip_always":
            sign = -1
        rec.append(dict(contact=c, role=role, force=force, sign=sign))
    if rec:
        p = np.stack([cpos[r["contact"]] for r in rec])
        nrm = np.stack([r["sign"] * cframe[r["contact"], :3] for r in rec])
        n = len(rec)
        if opposite:   # (both directions in one call)
            p, nrm = np.concatenate([p, p]), np.concatenate([nrm, -nrm])
        meets, fmin, case = ray_meets_zone(m["site_type"][site], m["site_size"][site], zpos, zmat, p, nrm)
        for k, r in enumerate(rec):
            ok = bool(meets[k]) if mut != "inside_only" else case[k] == "inside"
            r.update(meets=bool(meets[k]), min_sdf=fmin[k], case=str(case[k]), counted=ok and (r["force"] > 0 or mut == "count_nonpositive"))
            if opposite:
                r.update(meets_opposite=bool(meets[n + k]), min_sdf_opposite=fmin[n + k])
    return rec


def touch(model, dump, sensor, mut=None, detail=None):
    """The touch sensor's reading from the engine's or the oracle's own full-frame dump (contact_geom, contact_pos, contact_frame, contact_dim,
    contact_efc_address, efc_type, efc_force, site_xpos, site_xmat, ncon): the sum, over the contacts with constraint rows (efc_address >= 0) that
    involve the site's body, of the contact's normal force where that force is > 0 -- the sum of the contact's 2 (dim - 1) rows for a pyramidal
    contact, its first row for an elliptic or frictionless one.  A contact counts only if the ray from contact_pos along the contact normal meets the
    site's volume; the normal (which points from geom1 to geom2) is negated when the site's body is the body of the contact's geom2, so that the
    ray leaves the sensor's body towards the other one in either role.  A positive cutoff clamps the result.

    The direction convention is the project's statement of mj_sensorAcc (the comment on the touch case in csrc/mjb_step.hip and the touch sensor in
    oracle/mjo_smooth.c); parity unpinned: no MuJoCo run stands behind it here.  What this reference pins is that kernel and oracle implement the
    stated convention, not the convention itself."""
    rec = touch_detail(model, dump, sensor, mut) if detail is None else detail
    total = LD(0)
    for r in rec:
        if r["counted"]:
            total += r["force"]
    cutoff = LD(float(model["sensor_cutoff"][sensor]))
    if cutoff > 0:
        total = min(max(total, -cutoff), cutoff)
    return total
