"""Scenes, ray sets and the nearest-hit reference of the batched ray casting tests (test_ray_cast.py, test_gpu_ray_cast.py): no tests here.

The reference is ray_zone_ref.py's ray_distance per geom (longdouble signed distances, golden section, bisection); nearest_hit() below only walks the
geoms in order with the interface's skip rules and keeps the smallest distance under a strict `<`, so the lower geom id keeps a tie.  The bounds and
the exclusion rules are those of test_ray_zone_sensors.py for the same comparison (RF_TOL, RF_GRAZE, RF_GRAZE_SHARE), plus, for the geom id, the rays
whose nearest and second-nearest reference distances are closer than ID_GAP."""
import functools

import numpy as np

import ray_zone_ref as rz
from test_ray_zone_sensors import RF_GRAZE, RF_GRAZE_SHARE, RF_TOL, oracle_forward
from mujoco_ros_pkgs_amd import mjcf
from mujoco_ros_pkgs_amd.engine import lidar_rays, pinhole_rays

LD = np.longdouble
ID_GAP = 1e-7
TILE_GEOMS = 64   # MJB_RAY_TILE of csrc/mjb_dev.h: the geom records the ray kernel stages through LDS at a time (a block of several envs shares them out)
POSE_FIELDS = ("geom_xpos", "geom_xmat", "site_xpos", "site_xmat")
NENV, NENV_MANY = 7, 70


def _q(*q):
    q = np.array(q, float)
    return " ".join(repr(float(x)) for x in q / np.linalg.norm(q))


# A small hinge / slide tree carries the ray sites: the base slides along x, the arm yaws about z, the head pitches about y.  The camera site looks
# along the head's +x (a pinhole camera looks along its -z: the site's z axis is the head's -x, its y axis the head's z); the lidar site sits inside
# the base's mast, tilted, so that no ring ray is parallel to the floor.  `shell` and `mast` hold the two sites: a ray that does not exclude its
# own body starts inside them.  `ghost` has alpha 0 and stands in front of the camera.
SCENE_XML = """
<mujoco model="ray_cast_scene{tag}">
  <compiler angle="radian"/>
  <option timestep="0.002">{flags}</option>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 0.1"/>
    <geom name="panel" type="plane" size="0.45 0.3 0.1" pos="1.5 0.1 0.35" quat="{panel}"/>
    <geom name="ghost" type="box" size="0.005 0.2 0.15" pos="0.35 0 0.35" rgba="1 0 0 0" contype="0" conaffinity="0"/>
    <geom name="ball" type="sphere" size="0.12" pos="0.75 0.2 0.32"/>
    <geom name="pebble" type="sphere" size="0.05" pos="0.5 -0.35 0.05"/>
    <geom name="rod" type="capsule" size="0.05 0.18" pos="0.7 -0.22 0.3" quat="{rod}"/>
    <geom name="log" type="capsule" size="0.04 0.25" pos="0.2 0.5 0.04" quat="{log}"/>
    <geom name="crate" type="box" size="0.1 0.08 0.12" pos="1.0 -0.02 0.14" quat="{crate}"/>
    <geom name="step" type="box" size="0.15 0.1 0.03" pos="-0.4 -0.3 0.03"/>{filler}
    <body name="base" pos="0 0 0.1">
      <joint name="slide" type="slide" axis="1 0 0"/>
      <geom name="mast" type="capsule" size="0.04 0.08" mass="2"/>
      <site name="lidar" pos="0.005 -0.004 0.05" quat="{lidar}"/>
      <body name="arm" pos="0 0 0.25">
        <joint name="yaw" type="hinge" axis="0 0 1"/>
        <geom name="boom" type="box" size="0.06 0.02 0.015" pos="0.0 0 -0.03" mass="0.5"/>
        <body name="head" pos="0.08 0 0.06">
          <joint name="pitch" type="hinge" axis="0 1 0"/>
          <geom name="shell" type="sphere" size="0.05" mass="0.3"/>
          <site name="cam" pos="0.01 0.002 0.004" quat="0.5 0.5 -0.5 -0.5"/>
        </body>
      </body>
    </body>
  </worldbody>
</mujoco>
"""


def _filler(n):
    """n small spheres on a lattice above and beside the scene: they push ngeom past one LDS tile and leave most rays their other targets."""
    rows = []
    for k in range(n):
        x, y, z = 0.3 + 0.11 * (k % 10), -0.55 + 0.22 * ((k // 10) % 6), 0.55 + 0.05 * ((k * 7) % 5)
        rows.append(f'\n    <geom name="f{k}" type="sphere" size="0.025" pos="{x!r} {y!r} {z!r}" contype="0" conaffinity="0"/>')
    return "".join(rows)


@functools.lru_cache(maxsize=None)
def scene_model(contacts=False, many_geoms=False):
    """contacts: left on -- per-env geom sizes and types exist for models with contacts only.  many_geoms: 60 more spheres, ngeom > TILE_GEOMS."""
    m = mjcf.compile_xml_string(SCENE_XML.format(tag=("_contacts" if contacts else "") + ("_many" if many_geoms else ""),
                                                 flags="" if contacts else '<flag contact="disable"/>', filler=_filler(60) if many_geoms else "",
                                                 panel=_q(0.5, 0.46, -0.54, -0.5), rod=_q(0.9, 0.3, 0.2, 0.1), log=_q(0.7, 0.7, 0.1, 0),
                                                 crate=_q(0.95, 0.1, -0.15, 0.2), lidar=_q(0.99, 0.06, -0.09, 0.05)))
    assert (int(m["ngeom"]) > TILE_GEOMS) == many_geoms
    return m


@functools.lru_cache(maxsize=None)
def scene_qpos(n=NENV_MANY, seed=3):
    """[n, 3] slide, yaw, pitch: env e has the same state in a batch of any size."""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.1, 0.45, n)], 1)
    q.setflags(write=False)
    return q


def geom_ids(m, *names):
    return [m["names"]["geom"].index(n) for n in names]


class RaySet:
    """site [n] (ids, -1 = world), pnt [n, 3], vec [n, 3], exclude [n] (bool)."""

    def __init__(self, site, pnt, vec, exclude):
        self.site, self.pnt, self.vec, self.exclude = (np.ascontiguousarray(a) for a in (site, pnt, vec, exclude))
        for a in (self.site, self.pnt, self.vec, self.exclude):
            a.setflags(write=False)

    def __len__(self):
        return len(self.site)

    def first(self, n):
        return RaySet(self.site[:n], self.pnt[:n], self.vec[:n], self.exclude[:n])

    def with_exclude(self, exclude):
        return RaySet(self.site, self.pnt, self.vec, np.asarray(exclude, bool))


N_PINHOLE, N_LIDAR, N_WORLD = 300, 37, 20


@functools.lru_cache(maxsize=None)
def scene_rays(seed=11):
    """One set for one configure call: 300 pinhole rays (20 x 15, unit vectors) on the camera site of the head, 37 lidar rays on the base's site (8 degrees
    below its x-y plane, scaled by 0.5: the results come in units of |vec|), 20 world-frame rays with pnt off the origin -- twelve of them start inside
    the ball, the rod and the crate, eight come down from above the scene."""
    m = scene_model()
    rng = np.random.default_rng(seed)
    cam, lidar = m["names"]["site"].index("cam"), m["names"]["site"].index("lidar")
    pin, _ = pinhole_rays(20, 15, 75.0)
    ring = 0.5 * lidar_rays(N_LIDAR, elevations_deg=(-8.0,))
    centres = {"ball": (0.75, 0.2, 0.32), "rod": (0.7, -0.22, 0.3), "crate": (1.0, -0.02, 0.14)}
    wp, wv = [], []
    for name in ("ball", "rod", "crate"):
        for _ in range(4):
            wp.append(np.array(centres[name]) + rng.uniform(-0.02, 0.02, 3))
            v = rng.normal(size=3)
            wv.append(v / np.linalg.norm(v) * rng.uniform(0.5, 2.0))
    for _ in range(8):
        wp.append(np.array([rng.uniform(0.2, 1.2), rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.2)]))
        wv.append(np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0]) * rng.uniform(0.5, 2.0))
    assert len(pin) == N_PINHOLE and len(ring) == N_LIDAR and len(wp) == N_WORLD
    site = np.r_[np.full(N_PINHOLE, cam), np.full(N_LIDAR, lidar), np.full(N_WORLD, -1)].astype(np.int32)
    pnt = np.concatenate([np.zeros((N_PINHOLE + N_LIDAR, 3)), np.array(wp)])
    vec = np.concatenate([pin, ring, np.array(wv)])
    return RaySet(site, pnt, vec, np.ones(len(site), bool))


def default_visible(m):
    return np.asarray(m["geom_rgba"], float).reshape(-1, 4)[:, 3] != 0


def nearest_hit(m, poses, rays, visible=None, size=None, gtype=None):
    """The contract of Batch.cast_rays from the reference alone.  poses: {geom_xpos, geom_xmat, site_xpos, site_xmat: [nenv, ...]}; visible [ngeom] (None:
    alpha != 0); size [nenv, ngeom, 3] / gtype [nenv, ngeom] override the model's.  Returns a dict of [nenv, nray] arrays: dist (longdouble, -1 = miss), geomid
    (-1 = miss), graze (the smallest grazing measure over the geoms looked at), gap (second-nearest minus nearest distance, inf without a second hit) and
    inside (the ray starts inside a convex geom it looks at)."""
    ngeom, nsite, nray = int(m["ngeom"]), int(m["nsite"]), len(rays)
    gp = rz._ld(poses["geom_xpos"]).reshape(-1, ngeom, 3)
    nenv = gp.shape[0]
    gm = rz._ld(poses["geom_xmat"]).reshape(nenv, ngeom, 3, 3)
    sp = rz._ld(poses["site_xpos"]).reshape(nenv, nsite, 3)
    sm = rz._ld(poses["site_xmat"]).reshape(nenv, nsite, 3, 3)
    visible = default_visible(m) if visible is None else np.asarray(visible) != 0
    gsize = np.broadcast_to(rz._ld(m["geom_size"] if size is None else size).reshape(-1, ngeom, 3), (nenv, ngeom, 3))
    gtype = np.broadcast_to(np.asarray(m["geom_type"] if gtype is None else gtype, dtype=int).reshape(-1, ngeom), (nenv, ngeom))
    # the rays in the world frame [nenv, nray, 3]
    on_site = rays.site >= 0
    s = np.where(on_site, rays.site, 0)
    pnt, vec = rz._ld(rays.pnt), rz._ld(rays.vec)
    org = np.where(on_site[None, :, None], sp[:, s] + np.einsum("erij,rj->eri", sm[:, s], pnt), pnt[None])
    dirn = np.where(on_site[None, :, None], np.einsum("erij,rj->eri", sm[:, s], vec), vec[None])
    own = np.where(on_site & rays.exclude, np.asarray(m["site_bodyid"], int)[s], -1)
    shape = (nenv, nray)
    best, second = np.full(shape, LD(-1)), np.full(shape, LD(np.inf))
    gid = np.full(shape, -1)
    graze = np.full(shape, LD(1e30))
    inside = np.zeros(shape, bool)
    for g in range(ngeom):
        if not visible[g]:
            continue
        look = np.broadcast_to(own != int(m["geom_bodyid"][g]), shape)
        for kind in np.unique(gtype[:, g]):
            sel = look & (gtype[:, g] == kind)[:, None]
            e, r = np.nonzero(sel)
            if len(e) == 0:
                continue
            d, gz = rz.ray_distance(int(kind), gsize[e, g], gp[e, g], gm[e, g], org[e, r], dirn[e, r])
            if int(kind) != rz.PLANE:
                lp, _ = rz.local_ray(gp[e, g], gm[e, g], org[e, r], dirn[e, r])
                inside[e, r] |= rz.sdf(int(kind), gsize[e, g], lp) <= 0
            b = best[e, r]
            take = (d >= 0) & ((b < 0) | (d < b))
            # the runner-up: the old best where the new one takes over, else the new distance where it is a hit
            second[e, r] = np.where(take, np.where(b >= 0, np.minimum(second[e, r], b), second[e, r]), np.where(d >= 0, np.minimum(second[e, r], d), second[e, r]))
            best[e, r] = np.where(take, d, b)
            gid[e, r] = np.where(take, g, gid[e, r])
            graze[e, r] = np.minimum(graze[e, r], np.abs(gz))
    gap = np.where(best >= 0, second - best, LD(np.inf))
    return dict(dist=best, geomid=gid, graze=graze, gap=gap, inside=inside)


def check_cast(dist, geomid, want, what):
    """The assertions on one case's rays; returns (worst relative error, rays excluded)."""
    got, ref = np.asarray(dist, dtype=LD), want["dist"]
    assert got.shape == ref.shape and np.asarray(geomid).shape == ref.shape, (what, got.shape, ref.shape)
    keep = np.asarray(want["graze"]) >= RF_GRAZE
    keep_id = keep & (np.asarray(want["gap"]) >= ID_GAP)
    assert (~keep_id).sum() <= RF_GRAZE_SHARE * ref.size, (what, "excluded rays", int((~keep_id).sum()), ref.size)
    bad = np.argwhere(keep & ((got < 0) != (ref < 0)))
    assert len(bad) == 0, (what, "hit / miss decision", bad[:5])
    bad = np.argwhere(keep & (ref < 0) & ((got != -1) | (np.asarray(geomid) != -1)))
    assert len(bad) == 0, (what, "a miss is not (-1, -1)", bad[:5])
    err = np.where(keep & (ref >= 0), np.abs(got - ref) / (1 + np.abs(ref)), 0)
    worst = float(err.max())
    print(f"{what}: worst |got - want| / (1 + want) = {worst:.2e}; excluded {int((~keep).sum())} grazing, {int((keep & ~keep_id).sum())} more for the id")
    assert worst <= RF_TOL, (what, np.unravel_index(int(err.argmax()), err.shape), got.ravel()[err.argmax()], ref.ravel()[err.argmax()])
    bad = np.argwhere(keep_id & (np.asarray(geomid) != want["geomid"]))
    assert len(bad) == 0, (what, "geom id", bad[:5])
    return worst, int((~keep_id).sum())


# ------------------------------------------------------------------------------------------------------------------ the cases of the GPU tests
@functools.lru_cache(maxsize=None)
def scene_poses(oracle, contacts=False):
    """The oracle's forward pass at the NENV states: what the references below are computed on when no device is there."""
    m = scene_model(contacts)
    return oracle_forward(oracle, m, scene_qpos()[:NENV], fields=POSE_FIELDS)


def masked_case(m, rays):
    """Case 4: a mask that removes the ball and the crate (and, being a mask, shows the ghost), own-body exclusion off on every other ray."""
    mask = np.ones(int(m["ngeom"]), np.uint8)
    mask[geom_ids(m, "ball", "crate")] = 0
    return mask, rays.with_exclude(np.arange(len(rays)) % 2 == 0)


def per_env_geometry(m, nenv=NENV):
    """Case 3: size [nenv, ngeom, 3], type [nenv, ngeom] -- every env scales the ball and the crate by a factor of its own; the odd envs turn the ball into a
    box and the rod into a sphere, with sizes that suit the new types."""
    rng = np.random.default_rng(5)
    size = np.tile(np.asarray(m["geom_size"], float).reshape(1, -1, 3), (nenv, 1, 1))
    gtype = np.tile(np.asarray(m["geom_type"], np.int32), (nenv, 1))
    ball, rod, crate = geom_ids(m, "ball", "rod", "crate")
    size[:, ball] *= rng.uniform(0.6, 1.5, (nenv, 1))
    size[:, crate] *= rng.uniform(0.6, 1.5, (nenv, 1))
    gtype[1::2, ball] = rz.BOX
    size[1::2, ball] = (0.1, 0.07, 0.12)
    gtype[1::2, rod] = rz.SPHERE
    size[1::2, rod] = (0.11, 0, 0)
    return size, gtype
