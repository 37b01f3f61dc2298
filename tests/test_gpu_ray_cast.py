"""Batched ray casting on the device (Batch.set_rays / cast_rays, csrc/mjb_ray.hip): against the rangefinder sensor bit for bit, against the independent
reference of ray_cast_models.py (ray_zone_ref.py per geom) under the bounds of test_ray_zone_sensors.py, across launch shapes bit for bit, and the
interface's contract.  The scenes, ray sets and their teeth are those test_ray_cast.py checks without a device.

Measured on an MI355X, worst |got - want| / (1 + want) against the reference (bound 1e-12), no ray excluded as grazing or as a tie of two geoms:
    357 rays x 7 envs 6.0e-15   mask + exclusion off on half the rays 1.4e-15   per-env sizes / types 6.0e-15   after step() with keep_frame 6.0e-15
    rangefinder identity and launch shapes: equal bits."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import ray_cast_models as rc
import test_ray_zone_sensors as cpu

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def compiled(m):
    from mujoco_ros_pkgs_amd import engine
    cm = engine.CompiledModel(m)
    try:
        yield cm
    finally:
        cm.close()


@contextlib.contextmanager
def batch(cm, qpos, qvel=None):
    from mujoco_ros_pkgs_amd import engine
    b = engine.Batch(cm, len(qpos))
    try:
        b.set("qpos", qpos)
        if qvel is not None:
            b.set("qvel", qvel)
        yield b
    finally:
        b.close()


def set_rays(b, rays, geom_mask=None):
    b.set_rays(rays.site, rays.vec, pnt=rays.pnt, exclude_own_body=rays.exclude, geom_mask=geom_mask)


def poses_of(b):
    return {f: b.get(f) for f in rc.POSE_FIELDS}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 1. rangefinder identity
def _rangefinder_rays(m):
    """One ray per rangefinder sensor: from its site along the site's z axis, excluding the site's body, no mask."""
    sens = [i for i in range(int(m["nsensor"])) if int(m["sensor_type"][i]) == RANGEFINDER]
    site = np.array([int(m["sensor_objid"][i]) for i in sens], np.int32)
    return sens, site


RANGEFINDER = 7   # MJB_SENS_RANGEFINDER of include/mjb.h


def _identity(m, qpos, qvel, what):
    sens, site = _rangefinder_rays(m)
    assert len(sens) >= 1, what
    with compiled(m) as cm, batch(cm, qpos, qvel) as b:
        b.set_rays(site, np.tile([0.0, 0.0, 1.0], (len(site), 1)))
        b.set_keep_frame(True)
        for path in ("forward", "step(2)"):
            b.forward() if path == "forward" else b.step(2)
            sd = b.get("sensordata")
            dist, gid = b.cast_rays()
            assert dist.shape == (len(qpos), len(sens)) and dist.dtype == np.float64 and gid.dtype == np.int32
            for k, i in enumerate(sens):
                got, cutoff = sd[:, int(m["sensor_adr"][i])], float(m["sensor_cutoff"][i])
                want = dist[:, k] if cutoff <= 0 else np.where(dist[:, k] >= 0, np.minimum(dist[:, k], cutoff), dist[:, k])
                assert same_bits(got, want), (what, path, i, np.nonzero(got != want)[0][:5])
                assert np.array_equal(dist[:, k] < 0, gid[:, k] < 0) and (dist[gid[:, k] < 0, k] == -1).all()
            assert (dist >= 0).sum() >= 40 and (dist < 0).sum() >= 5, (what, path, "hits and misses")


@pytest.mark.parametrize("name", list(cpu.PRIMITIVES))
def test_rangefinder_identity_single_targets(name):
    _identity(cpu.single_model(name), cpu.single_poses(name), None, name)


@pytest.mark.parametrize("layout", ["a", "b"])
def test_rangefinder_identity_scene(layout):
    """Two rangefinders on one site, the second with a cutoff of 0.4: min(x, cutoff) on hits, -1 stays -1."""
    qpos, qvel = cpu.scene_states()
    _identity(cpu.scene_model(layout), qpos, qvel, "scene " + layout)


# ------------------------------------------------------------------------------------------------------------------ 2. - 4. independent reference
def test_against_the_reference():
    m, rays = rc.scene_model(), rc.scene_rays()
    with compiled(m) as cm, batch(cm, rc.scene_qpos()[:rc.NENV]) as b:
        b.forward()
        poses = poses_of(b)
        set_rays(b, rays)
        dist, gid = b.cast_rays()
        want = rc.nearest_hit(m, poses, rays)
        rc.check_cast(dist, gid, want, "scene: 300 pinhole + 37 lidar + 20 world rays, 7 envs")
        assert np.ptp(dist[:, :rc.N_PINHOLE], axis=0).max() > 0.01, "the envs see different things"

        # 4. the same scene with a mask that removes two geoms and own-body exclusion off on half the rays
        mask, rays4 = rc.masked_case(m, rays)
        set_rays(b, rays4, geom_mask=mask)
        dist4, gid4 = b.cast_rays()
        want4 = rc.nearest_hit(m, poses, rays4, visible=mask)
        rc.check_cast(dist4, gid4, want4, "scene: mask without ball and crate, own-body exclusion off on the even rays")
        affected = (want4["geomid"] != want["geomid"]) | (np.abs(want4["dist"] - want["dist"]) > 1e-6)
        assert affected.sum() >= 10
        assert ((gid4 != gid) | (dist4 != dist))[affected].all(), "the rays the reference shows to be affected differ from the unmasked case"
        ball, crate = rc.geom_ids(m, "ball", "crate")
        assert not np.isin(gid4, [ball, crate]).any() and np.isin(gid, [ball, crate]).sum() >= 40


def test_per_env_geometry():
    """3. set_env_geom_size / set_env_geom_type on the contact-enabled variant: each env's rays meet that env's shapes."""
    m, rays = rc.scene_model(contacts=True), rc.scene_rays()
    size, gtype = rc.per_env_geometry(m)
    with compiled(m) as cm, batch(cm, rc.scene_qpos()[:rc.NENV]) as b:
        set_rays(b, rays)
        b.forward()
        plain, _ = b.cast_rays()
        b.set_env_geom_size(size)
        b.set_env_geom_type(gtype)
        b.forward()
        poses = poses_of(b)
        dist, gid = b.cast_rays()
    want = rc.nearest_hit(m, poses, rays, size=size, gtype=gtype)
    rc.check_cast(dist, gid, want, "per-env geom sizes and types")
    changed = np.abs(dist - plain) > 1e-3
    assert changed[0::2].sum() >= 20 and changed[1::2].sum() >= 20


# ------------------------------------------------------------------------------------------------------------------ 5. launch shapes
# The kernel stages rc.TILE_GEOMS = 64 geom records per block through LDS; a block of E envs gives each 64 // E of them.  Ray sets of 1, 37, 64 and 65
# rays put 64, 6, 4 and 3 whole envs into a block (tiles of 1, 10, 16 and 21 geoms), 300 rays make two ray tiles of one env (tiles of 64 geoms).
RAY_SETS = (1, 37, 64, 65, 300)
ENV_SETS = (1, 7, 70)


@pytest.mark.parametrize("many_geoms", [False, True], ids=["12 geoms", "72 geoms: more than one tile"])
def test_launch_shapes_give_the_same_bits(many_geoms):
    m = rc.scene_model(many_geoms=many_geoms)
    assert (int(m["ngeom"]) > rc.TILE_GEOMS) == many_geoms
    # ... with the last ray of every set on the lidar site and world-frame rays in between: the sets mix sites
    full = rc.scene_rays()
    order = np.r_[np.arange(0, 30), rc.N_PINHOLE + np.arange(4), len(full) - 1 - np.arange(3), np.arange(30, rc.N_PINHOLE - 7)]
    rays = rc.RaySet(full.site[order], full.pnt[order], full.vec[order], np.arange(len(order)) % 3 != 0)
    assert len(rays) == max(RAY_SETS)
    qpos = rc.scene_qpos()
    out = {}
    with compiled(m) as cm:
        for nenv in ENV_SETS:
            with batch(cm, qpos[:nenv]) as b:
                b.forward()
                for nray in RAY_SETS:
                    set_rays(b, rays.first(nray))
                    out[nenv, nray] = b.cast_rays()
    ref_d, ref_g = out[max(ENV_SETS), max(RAY_SETS)]
    assert (ref_g >= 0).sum() >= 1000 and (ref_g < 0).sum() >= 1000 and len(np.unique(ref_g)) >= (20 if many_geoms else 8)
    for (nenv, nray), (d, g) in out.items():
        assert same_bits(d, ref_d[:nenv, :nray]) and same_bits(g, ref_g[:nenv, :nray]), (nenv, nray)
    if many_geoms:   # geoms beyond the first tile are hit, in every shape
        assert (ref_g[:, :1] >= 0).any() and (ref_g >= rc.TILE_GEOMS).sum() >= 20


# ------------------------------------------------------------------------------------------------------------------ 6. contract
ONLY_AFTER = "only after mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame"


def test_contract():
    from mujoco_ros_pkgs_amd import engine
    m, rays = rc.scene_model(), rc.scene_rays()
    lib = engine._lib()
    live0 = lib.mjb_debug_live_resources()
    qpos = rc.scene_qpos()[:rc.NENV]
    with compiled(m) as cm:
        with batch(cm, qpos, np.full((rc.NENV, int(m["nv"])), 0.5)) as b:   # (moving: nothing in this tree falls by itself)
            with pytest.raises(engine.EngineError, match="before mjb_rays_configure"):
                b.cast_rays()
            with pytest.raises(engine.EngineError):
                b.rays_device_ptr(0)
            set_rays(b, rays)
            with pytest.raises(engine.EngineError, match=ONLY_AFTER):   # before any forward
                b.cast_rays()
            b.forward()
            first = b.cast_rays()
            b.step()
            with pytest.raises(engine.EngineError, match=ONLY_AFTER):   # after step() without keep_frame
                b.cast_rays()
            b.forward()
            assert lib.mjb_step1_prefix(b.ptr, 3) == 0
            with pytest.raises(engine.EngineError, match=ONLY_AFTER):   # the frames of a prefix of the envs only
                b.cast_rays()
            b.step()   # (abandons the open split step)
            # it works after step() with keep_frame, and between step1 and step2
            b.set_keep_frame(True)
            b.step()
            after_step = b.cast_rays()
            want = rc.nearest_hit(m, poses_of(b), rays)
            rc.check_cast(*after_step, want, "after step() with keep_frame")
            b.set_keep_frame(False)
            b.step1()
            between = b.cast_rays()
            rc.check_cast(*between, rc.nearest_hit(m, poses_of(b), rays), "between step1 and step2")
            b.step2()
            assert not same_bits(first[0], after_step[0]) and not same_bits(after_step[0], between[0]), "the casts followed the frames"

            # a second set_rays with another nray replaces the buffers; the device pointers serve the same numbers
            few = rays.first(37)
            set_rays(b, few)
            b.forward()
            b.cast_rays_async()
            p_dist, p_gid = b.rays_device_ptr(0), b.rays_device_ptr(1)
            assert p_dist and p_gid and int(lib.mjb_rays_count(b.ptr)) == 37
            dist, gid = b.cast_rays()
            assert dist.shape == (rc.NENV, 37)
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            d2, g2 = np.empty_like(dist), np.empty_like(gid)
            assert hip.hipMemcpy(d2.ctypes.data, p_dist, d2.nbytes, 2) == 0 and hip.hipMemcpy(g2.ctypes.data, p_gid, g2.nbytes, 2) == 0
            assert same_bits(d2, dist) and same_bits(g2, gid)
            lo_hi = b.cast_rays(2, 5)
            assert same_bits(lo_hi[0], dist[2:5]) and same_bits(lo_hi[1], gid[2:5])

            # configure refuses each invalid argument, and leaves the configuration it had
            ngeom, nsite = int(m["ngeom"]), int(m["nsite"])
            z = np.array([[0.0, 0.0, 1.0]])
            for why, kw in (("nray < 1", dict(site=[], vec=np.zeros((0, 3)))),
                            ("a site id outside [-1, nsite)", dict(site=nsite, vec=z)), ("a site id below -1", dict(site=-2, vec=z)),
                            ("a non-finite vec", dict(site=0, vec=[[0.0, np.nan, 1.0]])), ("a non-finite pnt", dict(site=0, vec=z, pnt=[[np.inf, 0.0, 0.0]])),
                            ("a zero vec", dict(site=0, vec=[[0.0, 0.0, 0.0]]))):
                with pytest.raises(engine.EngineError, match="mjb_rays_configure"):
                    b.set_rays(**kw)
                    pytest.fail(why + " was accepted")
            with pytest.raises(ValueError):
                b.set_rays(0, z, geom_mask=np.ones(ngeom + 1))
            with pytest.raises(ValueError):
                b.set_rays("no such site", z)
            b.set_rays("cam", z)   # a site by name
            assert int(lib.mjb_rays_count(b.ptr)) == 1
        with compiled(cpu.mjcf.compile_xml_string("<mujoco><worldbody><body><freejoint/><inertial pos='0 0 0' mass='1' diaginertia='1 1 1'/><site name='s'/></body></worldbody></mujoco>")) as cm0:
            with batch(cm0, np.array([[0, 0, 0, 1.0, 0, 0, 0]])) as b0:
                with pytest.raises(engine.EngineError, match="no geoms"):
                    b0.set_rays(0, [[0.0, 0.0, 1.0]])
    assert lib.mjb_debug_live_resources() == live0
