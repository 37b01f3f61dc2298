"""Batched ray casting without a device: the two pattern helpers of engine.py (pinhole_rays, lidar_rays), the nearest-hit reference of
ray_cast_models.py on closed forms, and the teeth of the GPU tests' scene and ray sets -- counted from the reference alone, on poses from the
oracle's forward pass, so that test_gpu_ray_cast.py cannot pass on a scene in which nothing happens."""
import numpy as np
import pytest

import ray_cast_models as rc
import ray_zone_ref as rz
from mujoco_ros_pkgs_amd.engine import lidar_rays, pinhole_rays


# ------------------------------------------------------------------------------------------------------------------ pinhole_rays
@pytest.mark.parametrize("w,h,fovy", [(20, 15, 75.0), (64, 48, 45.0), (5, 3, 90.0), (1, 1, 60.0)])
def test_pinhole_norms_cosz_and_corners(w, h, fovy):
    vec, cosz = pinhole_rays(w, h, fovy)
    assert vec.shape == (h * w, 3) and cosz.shape == (h * w,)
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-15
    assert np.array_equal(cosz, -vec[:, 2]) and (cosz > 0).all()
    # fovy is the angle between the outer pixel EDGES: the corner pixels' centres sit half a pixel inside the half extents tan(fovy / 2) (x: times w / h)
    half_h = np.tan(np.radians(fovy) / 2)
    half_w = half_h * w / h
    img = vec.reshape(h, w, 3)
    for (row, col, sx, sy) in ((0, 0, -1, 1), (0, w - 1, 1, 1), (h - 1, 0, -1, -1), (h - 1, w - 1, 1, -1)):
        v = img[row, col]
        assert np.isclose(np.arctan2(v[0], -v[2]), sx * np.arctan(half_w * (1 - 1 / w)), rtol=0, atol=1e-14), (row, col)
        assert np.isclose(np.arctan2(v[1], -v[2]), sy * np.arctan(half_h * (1 - 1 / h)), rtol=0, atol=1e-14), (row, col)


def test_pinhole_centre_order_and_fovy():
    vec, cosz = pinhole_rays(5, 3, 90.0)
    img = vec.reshape(3, 5, 3)
    assert np.array_equal(img[1, 2], [0.0, 0.0, -1.0]) and cosz.reshape(3, 5)[1, 2] == 1.0   # the centre of an odd-sized image looks straight ahead
    # rows run from the top (+y first), pixels from the left (-x first); x depends on the column only, y on the row only (before normalisation)
    assert (np.diff(img[:, :, 1] / -img[:, :, 2], axis=0) < 0).all() and (np.diff(img[:, :, 0] / -img[:, :, 2], axis=1) > 0).all()
    assert np.ptp(img[:, :, 0] / -img[:, :, 2], axis=0).max() < 1e-15 and np.ptp(img[:, :, 1] / -img[:, :, 2], axis=1).max() < 1e-15
    # a one-pixel-high image samples the middle of the field; two rows sample +-fovy/2 scaled by 1/2 in the tangent
    two, _ = pinhole_rays(1, 2, 90.0)
    assert np.allclose(two[:, 1] / -two[:, 2], [0.5, -0.5], rtol=0, atol=1e-15)
    # z-depth: a wall at depth 2 in front of the camera is hit at 2 / cosz along each unit ray
    assert np.allclose((2.0 / cosz) * cosz, 2.0)
    for bad in ((0, 3, 60.0), (3, 0, 60.0), (3, 3, 0.0), (3, 3, 180.0)):
        with pytest.raises(ValueError):
            pinhole_rays(*bad)


# ------------------------------------------------------------------------------------------------------------------ lidar_rays
def test_lidar_count_order_endpoint_and_elevation():
    v = lidar_rays(36)
    assert v.shape == (36, 3) and np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-15 and np.array_equal(v[:, 2], np.zeros(36))
    az = np.degrees(np.arctan2(v[:, 1], v[:, 0])) % 360
    assert np.allclose(az, np.arange(36) * 10.0, rtol=0, atol=1e-12)          # counter-clockwise from +x, a full turn without its endpoint
    assert np.array_equal(v[0], [1.0, 0.0, 0.0]) and v[9, 1] == 1.0 and abs(v[9, 0]) < 1e-15
    part = lidar_rays(5, azimuth_range_deg=(-90.0, 90.0))                      # not a full turn: both ends are rays
    assert np.allclose(np.degrees(np.arctan2(part[:, 1], part[:, 0])), [-90, -45, 0, 45, 90], rtol=0, atol=1e-12)
    multi = lidar_rays(4, elevations_deg=(-30.0, 0.0, 45.0))
    assert multi.shape == (12, 3)
    assert np.allclose(multi[:, 2], np.repeat(np.sin(np.radians([-30.0, 0.0, 45.0])), 4), rtol=0, atol=1e-15)   # azimuth runs fastest; up is +z
    assert np.allclose(multi[4:8], lidar_rays(4), rtol=0, atol=1e-15)
    assert np.allclose(multi[8], [np.cos(np.radians(45.0)), 0, np.sin(np.radians(45.0))], rtol=0, atol=1e-15)
    assert lidar_rays(1).shape == (1, 3)
    with pytest.raises(ValueError):
        lidar_rays(0)


# ------------------------------------------------------------------------------------------------------------------ the helper on closed forms
TWO_SPHERES = dict(ngeom=2, nsite=1, geom_type=np.array([rz.SPHERE, rz.SPHERE]), geom_size=np.array([[0.25, 0, 0], [0.5, 0, 0]]), geom_bodyid=np.array([0, 0]),
                   geom_rgba=np.ones((2, 4)), site_bodyid=np.array([1]))


def _two_sphere_poses(x0=2.0, x1=4.0):
    eye = np.eye(3).ravel()
    return dict(geom_xpos=np.array([[x0, 0, 0, x1, 0, 0]], float), geom_xmat=np.array([np.r_[eye, eye]]), site_xpos=np.zeros((1, 3)), site_xmat=np.array([eye]))


def test_nearest_hit_on_closed_forms():
    ray = rc.RaySet(np.array([0]), np.zeros((1, 3)), np.array([[1.0, 0, 0]]), np.array([True]))
    w = rc.nearest_hit(TWO_SPHERES, _two_sphere_poses(), ray)
    assert abs(float(w["dist"][0, 0]) - (2.0 - 0.25)) < 1e-15 and w["geomid"][0, 0] == 0      # a sphere at distance d: d - r; the nearer of two in line
    assert abs(float(w["gap"][0, 0]) - (3.5 - 1.75)) < 1e-15 and not w["inside"][0, 0]
    w = rc.nearest_hit(TWO_SPHERES, _two_sphere_poses(), ray, visible=[0, 1])
    assert abs(float(w["dist"][0, 0]) - (4.0 - 0.5)) < 1e-15 and w["geomid"][0, 0] == 1       # the mask removes the nearer one: the farther one is hit
    # distances come in units of |vec|; a world-frame ray with pnt; a ray that starts inside leaves through the far surface
    world = rc.RaySet(np.array([-1, -1]), np.array([[0.5, 0, 0], [2.1, 0, 0]]), np.array([[0.5, 0, 0], [-1.0, 0, 0]]), np.array([True, True]))
    w = rc.nearest_hit(TWO_SPHERES, _two_sphere_poses(), world)
    assert abs(float(w["dist"][0, 0]) - (1.75 - 0.5) / 0.5) < 1e-15 and abs(float(w["dist"][0, 1]) - 0.35) < 1e-15 and list(w["inside"][0]) == [False, True]
    away = rc.RaySet(np.array([0]), np.zeros((1, 3)), np.array([[-1.0, 0, 0]]), np.array([True]))
    w = rc.nearest_hit(TWO_SPHERES, _two_sphere_poses(), away)
    assert w["dist"][0, 0] == -1 and w["geomid"][0, 0] == -1 and np.isinf(w["gap"][0, 0])
    # equal distances: the lower geom id keeps the tie
    w = rc.nearest_hit(dict(TWO_SPHERES, geom_size=np.array([[0.5, 0, 0], [0.5, 0, 0]])), _two_sphere_poses(3.0, 3.0), ray)
    assert w["geomid"][0, 0] == 0 and w["gap"][0, 0] == 0
    # the own-body exclusion: with the first sphere on the site's body, an excluding ray passes it
    own = dict(TWO_SPHERES, geom_bodyid=np.array([1, 0]))
    assert rc.nearest_hit(own, _two_sphere_poses(), ray)["geomid"][0, 0] == 1
    assert rc.nearest_hit(own, _two_sphere_poses(), ray.with_exclude([False]))["geomid"][0, 0] == 0


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' inputs have teeth
def test_scene_and_ray_sets_have_teeth(oracle_built):
    m, rays = rc.scene_model(), rc.scene_rays()
    assert len(rays) == rc.N_PINHOLE + rc.N_LIDAR + rc.N_WORLD and (rays.site[-rc.N_WORLD:] == -1).all() and (np.abs(rays.pnt[-rc.N_WORLD:]).min(1) > 0).all()
    poses = rc.scene_poses(oracle_built)
    assert np.ptp(poses["site_xpos"], axis=0).max() > 0.05, "the envs' poses differ"
    w = rc.nearest_hit(m, poses, rays)
    types = np.asarray(m["geom_type"])[np.where(w["geomid"] >= 0, w["geomid"], 0)]
    counts = {k: int(((w["geomid"] >= 0) & (types == k)).sum()) for k in (rz.PLANE, rz.SPHERE, rz.CAPSULE, rz.BOX)}
    assert min(counts.values()) >= 20, counts
    assert (w["geomid"] < 0).sum() >= 20 and w["inside"].sum() >= 10
    for block in (slice(0, rc.N_PINHOLE), slice(rc.N_PINHOLE, rc.N_PINHOLE + rc.N_LIDAR), slice(-rc.N_WORLD, None)):
        assert (w["geomid"][:, block] >= 0).sum() >= 20, "every ray block hits something"
    ghost, panel = rc.geom_ids(m, "ghost", "panel")
    assert not (w["geomid"] == ghost).any() and (w["geomid"] == panel).sum() >= 20      # the invisible geom is never hit, the bounded plane is
    seen = rc.nearest_hit(m, poses, rays, visible=np.ones(int(m["ngeom"])))
    assert (seen["geomid"] == ghost).sum() >= 20, "... though it is the first geom on many rays"
    excluded = (w["graze"] < rc.RF_GRAZE) | (w["gap"] < rc.ID_GAP)
    assert excluded.sum() < rc.RF_GRAZE_SHARE * excluded.size

    mask, rays4 = rc.masked_case(m, rays)
    w4 = rc.nearest_hit(m, poses, rays4, visible=mask)
    excl_only = rc.nearest_hit(m, poses, rays4)
    mask_only = rc.nearest_hit(m, poses, rays, visible=mask)
    for what, other in (("exclusion", excl_only), ("mask", mask_only), ("both", w4)):
        changed = (other["geomid"] != w["geomid"]) | (np.abs(other["dist"] - w["dist"]) > 1e-6)
        assert changed.sum() >= 10, what
    assert ((excl_only["geomid"] != w["geomid"])[:, rays4.exclude]).sum() == 0, "a ray that still excludes its body keeps its answer"
    assert ((w4["graze"] < rc.RF_GRAZE) | (w4["gap"] < rc.ID_GAP)).sum() < rc.RF_GRAZE_SHARE * excluded.size


def test_per_env_geometry_changes_the_answers(oracle_built):
    m, rays = rc.scene_model(contacts=True), rc.scene_rays()
    assert m["nconmax"] > 0
    poses = rc.scene_poses(oracle_built, contacts=True)
    size, gtype = rc.per_env_geometry(m)
    plain, w = rc.nearest_hit(m, poses, rays), rc.nearest_hit(m, poses, rays, size=size, gtype=gtype)
    changed = (w["geomid"] != plain["geomid"]) | (np.abs(w["dist"] - plain["dist"]) > 1e-3)
    assert changed[0::2].sum() >= 20 and changed[1::2].sum() >= 20, (int(changed[0::2].sum()), int(changed[1::2].sum()))
    assert ((w["graze"] < rc.RF_GRAZE) | (w["gap"] < rc.ID_GAP)).sum() < rc.RF_GRAZE_SHARE * changed.size


def test_the_large_scene_crosses_a_tile():
    m = rc.scene_model(many_geoms=True)
    assert int(m["ngeom"]) > rc.TILE_GEOMS and int(m["ngeom"]) % rc.TILE_GEOMS != 0
