"""Python face of the C-ABI engine (libmjb.so): thin, typed wrappers -- no compute happens here.

``CompiledModel`` <-> ``mjb_model``  (takes the place of the reference's ``mjModelPtr model_``,
/root/reference mujoco_ros/include/mujoco_ros/mujoco_env.h:298), ``Batch`` <-> ``mjb_batch`` (N x
``mjDataPtr data_``, mujoco_env.h:300).  Every method maps 1:1 onto an entry point of include/mjb.h and
raises ``EngineError`` with ``mjb_last_error()`` on a non-zero return.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding
from .binding import Field


class EngineError(RuntimeError):
    pass


def _lib():
    return binding.load_library()


def _check(rc, what):
    if rc != 0:
        raise EngineError(f"{what} failed ({rc}): {_lib().mjb_last_error().decode()}")


def device_count():
    return _lib().mjb_device_count()


def pinhole_rays(width, height, fovy_deg):
    """Ray directions of a width x height pinhole image in MuJoCo's camera frame (the camera looks along -z, +y is up, +x is right): returns
    (vec [height*width, 3] unit vectors, cosz [height*width] = -vec_z).  Rows run from the top, pixels are sampled at their centres, and fovy_deg is the
    vertical angle between the outer pixel edges.  With dist from Batch.cast_rays, a z-depth image is dist * cosz wherever dist >= 0.  Plain numpy."""
    width, height = int(width), int(height)
    if width < 1 or height < 1 or not 0.0 < float(fovy_deg) < 180.0:
        raise ValueError("pinhole_rays: width and height must be at least 1, fovy_deg inside (0, 180)")
    half_h = np.tan(np.radians(float(fovy_deg)) / 2)
    half_w = half_h * width / height
    x = ((np.arange(width) + 0.5) / width * 2 - 1) * half_w
    y = (1 - (np.arange(height) + 0.5) / height * 2) * half_h
    v = np.empty((height, width, 3))
    v[..., 0] = x[None, :]
    v[..., 1] = y[:, None]
    v[..., 2] = -1.0
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v = v.reshape(-1, 3)
    return v, -v[:, 2]


def lidar_rays(n_azimuth, elevations_deg=(0.0,), azimuth_range_deg=(0.0, 360.0)):
    """Unit ray directions of a lidar in the site's frame: n_azimuth rays per elevation ring, azimuth counter-clockwise from +x in the x-y plane and running
    fastest, elevation positive towards +z.  The end of the azimuth range is left out when the range is a full turn, included otherwise.  Returns
    [len(elevations_deg) * n_azimuth, 3].  Plain numpy."""
    n = int(n_azimuth)
    if n < 1:
        raise ValueError("lidar_rays: n_azimuth must be at least 1")
    a0, a1 = (float(a) for a in azimuth_range_deg)
    full = abs(abs(a1 - a0) - 360.0) < 1e-9
    az = np.radians(np.linspace(a0, a1, n, endpoint=not full)) if n > 1 else np.radians(np.array([a0]))
    el = np.radians(np.atleast_1d(np.asarray(elevations_deg, dtype=np.float64)))
    v = np.empty((el.size, n, 3))
    v[..., 0] = np.cos(el)[:, None] * np.cos(az)[None, :]
    v[..., 1] = np.cos(el)[:, None] * np.sin(az)[None, :]
    v[..., 2] = np.sin(el)[:, None]
    return v.reshape(-1, 3)


def geoms_of_bodies(model, bodies, subtree=False):
    """Geom ids (ascending) of the given bodies -- names or ids, one or a sequence -- and, with subtree=True, of every body below them: a geom set for
    Batch.set_contact_queries.  Plain numpy."""
    names = model["names"]["body"]
    nbody = int(model["nbody"])
    want = np.zeros(nbody, bool)
    for b in ([bodies] if isinstance(bodies, (str, int, np.integer)) else list(bodies)):
        if isinstance(b, str):
            if b not in names:
                raise ValueError(f"geoms_of_bodies: no body named {b!r}")
            b = names.index(b)
        if not 0 <= int(b) < nbody:
            raise ValueError(f"geoms_of_bodies: body {int(b)} outside [0, {nbody})")
        want[int(b)] = True
    if subtree:
        parent = np.asarray(model["body_parentid"], dtype=np.int64)
        for b in range(1, nbody):   # (a body's parent has a lower id)
            want[b] |= want[parent[b]]
    return [g for g in range(int(model["ngeom"])) if want[int(model["geom_bodyid"][g])]]


class CompiledModel:
    def __init__(self, model):
        self.model = model
        self.lib = _lib()
        desc, self._keep = binding.make_desc(model)
        self.ptr = self.lib.mjb_compile(C.byref(desc))
        if not self.ptr:
            raise EngineError("mjb_compile failed: " + self.lib.mjb_last_error().decode())

    def field_size(self, name):
        return self.lib.mjb_field_size(self.ptr, Field.ids[name])

    def derive_mass_params(self, body_mass, body_inertia=None):
        """mj_setConst's constants for new body masses (mjb_derive_mass_params, host-side C++): the packed block of
        mjb_set_env_mass_params.  Needs no device."""
        nb = int(self.model["nbody"])
        bm = np.ascontiguousarray(np.asarray(body_mass, dtype=np.float64).reshape(nb))
        bi = None if body_inertia is None else np.ascontiguousarray(np.asarray(body_inertia, dtype=np.float64).reshape(nb, 3))
        out = np.zeros(self.lib.mjb_env_mass_stride(self.ptr))
        pd = C.POINTER(C.c_double)
        _check(self.lib.mjb_derive_mass_params(self.ptr, bm.ctypes.data_as(pd), None if bi is None else bi.ctypes.data_as(pd),
                                               out.ctypes.data_as(pd)), "mjb_derive_mass_params")
        return out

    def derive_mass_params_armature(self, body_mass=None, body_inertia=None, armature=None):
        """The same with a dof armature [nv] in place of the model's (mjb_derive_mass_params_armature; None: the model's values)."""
        m = self.model
        nb, nv = int(m["nbody"]), int(m["nv"])
        pd = C.POINTER(C.c_double)
        bm = np.ascontiguousarray(np.asarray(m["body_mass"] if body_mass is None else body_mass, dtype=np.float64).reshape(nb))
        bi = None if body_inertia is None else np.ascontiguousarray(np.asarray(body_inertia, dtype=np.float64).reshape(nb, 3))
        ar = None if armature is None else np.ascontiguousarray(np.asarray(armature, dtype=np.float64).reshape(nv))
        out = np.zeros(self.lib.mjb_env_mass_stride(self.ptr))
        _check(self.lib.mjb_derive_mass_params_armature(self.ptr, bm.ctypes.data_as(pd), None if bi is None else bi.ctypes.data_as(pd),
                                                        None if ar is None else ar.ctypes.data_as(pd), out.ctypes.data_as(pd)),
               "mjb_derive_mass_params_armature")
        return out

    @property
    def frame_doubles(self):
        return self.lib.mjb_frame_doubles(self.ptr)

    def lane_env_tape(self):
        """The lane = env kernel's constant tape of the model (mjb_model_lane_env_tape), or None when the model is not eligible."""
        return self._lane_env_doubles(self.lib.mjb_model_lane_env_tape)

    def lane_env_rows(self):
        """(total, joint-equality rows, joint-limit rows) of the lane = env kernel's constraint stage for this model (mjb_lane_env_rows); (0, 0, 0): the
        model has no such stage."""
        ne, nl = C.c_int(0), C.c_int(0)
        total = int(self.lib.mjb_lane_env_rows(self.ptr, C.byref(ne), C.byref(nl)))
        return total, ne.value, nl.value

    def lane_env_overlay(self):
        """One env's column of the per-env table of Batch.set_lane_env(2), with the model's own values (mjb_model_lane_env_overlay); None: not eligible."""
        return self._lane_env_doubles(self.lib.mjb_model_lane_env_overlay)

    def _lane_env_doubles(self, fn):
        n = fn(self.ptr, None, 0)
        if n < 0:
            return None
        out = np.zeros(n)
        fn(self.ptr, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    def frame_info(self):
        """(the row-slot Newton / CG solver runs, the full frame lives in HBM, the fused frame lives in HBM) -- mjb_model_frame_info."""
        full, fused = C.c_int(0), C.c_int(0)
        slot = self.lib.mjb_model_frame_info(self.ptr, C.byref(full), C.byref(fused))
        if slot < 0:
            raise EngineError("mjb_model_frame_info failed: " + self.lib.mjb_last_error().decode())
        return bool(slot), bool(full.value), bool(fused.value)

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.mjb_free_model(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """N env instances of one model on one GPU."""

    def __init__(self, cmodel: CompiledModel, nenv: int, device: int = 0):
        self.cm = cmodel
        self.lib = cmodel.lib
        self.nenv = int(nenv)
        self.ptr = self.lib.mjb_make_batch(cmodel.ptr, self.nenv, int(device))
        if not self.ptr:
            raise EngineError("mjb_make_batch failed: " + self.lib.mjb_last_error().decode())

    # ---- stepping
    def step(self, nsteps=1):
        _check(self.lib.mjb_step(self.ptr, int(nsteps)), "mjb_step")

    def step1(self):
        _check(self.lib.mjb_step1(self.ptr), "mjb_step1")

    def step2(self):
        _check(self.lib.mjb_step2(self.ptr), "mjb_step2")

    def forward(self):
        _check(self.lib.mjb_forward(self.ptr), "mjb_forward")

    def reset(self, mask=None):
        if mask is None:
            _check(self.lib.mjb_reset(self.ptr, None), "mjb_reset")
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (self.nenv,):
                raise ValueError("mask must have shape (nenv,)")
            _check(self.lib.mjb_reset(self.ptr, m.ctypes.data_as(C.POINTER(C.c_uint8))), "mjb_reset")

    def synchronize(self):
        _check(self.lib.mjb_synchronize(self.ptr), "mjb_synchronize")

    def set_launch(self, lanes_per_env=0, envs_per_block=0):
        _check(self.lib.mjb_set_launch(self.ptr, lanes_per_env, envs_per_block), "mjb_set_launch")

    def warning_count(self):
        """Number of auto-resets (mj_checkPos / Vel / Acc warnings) since the batch was made."""
        n = C.c_uint64(0)
        _check(self.lib.mjb_warning_count(self.ptr, C.byref(n)), "mjb_warning_count")
        return int(n.value)

    def warning(self, which):
        """mjData.warning[which].number summed over the envs (mjb_warning; which = binding.WARN[...] or its int value)."""
        n = C.c_uint64(0)
        _check(self.lib.mjb_warning(self.ptr, binding.WARN.get(which, which), C.byref(n)), "mjb_warning")
        return int(n.value)

    def metrics(self):
        """The 16-double metrics vector of include/mjb.h (mjb_metrics) as a dict + the raw array."""
        out = np.zeros(16)
        _check(self.lib.mjb_metrics(self.ptr, out.ctypes.data_as(C.POINTER(C.c_double))), "mjb_metrics")
        return dict(zip(binding.METRIC_NAMES, out)), out

    def metrics_device_ptr(self):
        p = self.lib.mjb_metrics_device(self.ptr)
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    def register_collision(self, geom_type1, geom_type2, func):
        """registerCollisionFunction's device-side form: func = 0 default, 1 none, 2 bounding spheres (mjb_register_collision)."""
        _check(self.lib.mjb_register_collision(self.ptr, int(geom_type1), int(geom_type2), int(func)), "mjb_register_collision")

    # ---- per-env model parameters ----
    def set_env_gravity(self, gravity, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        a = np.ascontiguousarray(gravity, dtype=np.float64).reshape(hi - lo, 3)
        _check(self.lib.mjb_set_env_gravity(self.ptr, lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_set_env_gravity")

    def set_env_geom_friction(self, friction, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        a = np.ascontiguousarray(friction, dtype=np.float64).reshape(hi - lo, self.cm.model["ngeom"] * 3)
        _check(self.lib.mjb_set_env_geom_friction(self.ptr, lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))),
               "mjb_set_env_geom_friction")

    def set_env_geom_size(self, size, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        a = np.ascontiguousarray(size, dtype=np.float64).reshape(hi - lo, self.cm.model["ngeom"] * 3)
        _check(self.lib.mjb_set_env_geom_size(self.ptr, lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_set_env_geom_size")

    def set_env_geom_type(self, types, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        a = np.ascontiguousarray(types, dtype=np.int32).reshape(hi - lo, self.cm.model["ngeom"])
        _check(self.lib.mjb_set_env_geom_type(self.ptr, lo, hi, a.ctypes.data_as(C.POINTER(C.c_int))), "mjb_set_env_geom_type")

    def set_env_equality(self, active=None, data=None, solref=None, solimp=None, lo=0, hi=None):
        """Per-env equality parameters (setEqualityConstraintParameters per env).  Each argument is None (the model's
        values) or an array [hi-lo, neq(, 11 | 2 | 5)]."""
        hi = self.nenv if hi is None else hi
        m, n, neq = self.cm.model, hi - lo, int(self.cm.model["neq"])
        p = np.zeros((n, neq, 19))
        p[:, :, 0] = np.asarray(m["eq_active"], dtype=np.float64) if active is None else np.asarray(active, dtype=np.float64).reshape(n, neq)
        p[:, :, 1:12] = np.asarray(m["eq_data"]).reshape(neq, 11) if data is None else np.asarray(data, dtype=np.float64).reshape(n, neq, 11)
        p[:, :, 12:14] = np.asarray(m["eq_solref"]).reshape(neq, 2) if solref is None else np.asarray(solref, dtype=np.float64).reshape(n, neq, 2)
        p[:, :, 14:19] = np.asarray(m["eq_solimp"]).reshape(neq, 5) if solimp is None else np.asarray(solimp, dtype=np.float64).reshape(n, neq, 5)
        p = np.ascontiguousarray(p)
        _check(self.lib.mjb_set_env_equality(self.ptr, lo, hi, p.ctypes.data_as(C.POINTER(C.c_double))), "mjb_set_env_equality")

    def set_env_body_mass(self, body_mass, body_inertia=None, lo=0, hi=None):
        """Per-env body masses [hi-lo, nbody] (and optionally principal inertias [hi-lo, nbody, 3]): mjb_set_env_body_mass
        derives what mj_setConst would (in C++, inside libmjb) and uploads the packed constants."""
        hi = self.nenv if hi is None else hi
        n = hi - lo
        nb = int(self.cm.model["nbody"])
        bm = np.ascontiguousarray(np.asarray(body_mass, dtype=np.float64).reshape(n, nb))
        bi = None if body_inertia is None else np.ascontiguousarray(np.asarray(body_inertia, dtype=np.float64).reshape(n, nb, 3))
        pd = C.POINTER(C.c_double)
        _check(self.lib.mjb_set_env_body_mass(self.ptr, lo, hi, bm.ctypes.data_as(pd), None if bi is None else bi.ctypes.data_as(pd)),
               "mjb_set_env_body_mass")

    def _env_array(self, a, n, *shape):
        if a is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape((n,) + shape))
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def set_env_dof_params(self, damping=None, armature=None, frictionloss=None, lo=0, hi=None):
        """Per-env dof_damping / dof_armature / dof_frictionloss, each [hi-lo, nv] or None to leave that array as it is
        (mjb_set_env_dof_params: the engine re-derives what mj_setConst derives from the armature, and the integrator's damping)."""
        hi = self.nenv if hi is None else hi
        nv = int(self.cm.model["nv"])
        d, dp = self._env_array(damping, hi - lo, nv)
        a, ap = self._env_array(armature, hi - lo, nv)
        f, fp = self._env_array(frictionloss, hi - lo, nv)
        _check(self.lib.mjb_set_env_dof_params(self.ptr, lo, hi, dp, ap, fp), "mjb_set_env_dof_params")

    def set_env_joint_stiffness(self, stiffness, lo=0, hi=None):
        """Per-env jnt_stiffness [hi-lo, njnt] (mjb_set_env_joint_stiffness)."""
        hi = self.nenv if hi is None else hi
        s, sp = self._env_array(stiffness, hi - lo, int(self.cm.model["njnt"]))
        _check(self.lib.mjb_set_env_joint_stiffness(self.ptr, lo, hi, sp), "mjb_set_env_joint_stiffness")

    def set_env_actuator_params(self, gainprm=None, biasprm=None, lo=0, hi=None):
        """Per-env actuator_gainprm / actuator_biasprm, each [hi-lo, nu, 3] or None (mjb_set_env_actuator_params): kp / kv of
        <position> / <velocity> / <general> actuators."""
        hi = self.nenv if hi is None else hi
        nu = int(self.cm.model["nu"])
        g, gp = self._env_array(gainprm, hi - lo, nu, 3)
        b, bp = self._env_array(biasprm, hi - lo, nu, 3)
        _check(self.lib.mjb_set_env_actuator_params(self.ptr, lo, hi, gp, bp), "mjb_set_env_actuator_params")

    def set_env_joint_params(self, params, lo=0, hi=None):
        """The same as one packed block per env, [hi-lo, mjb_env_joint_stride] (mjcf.joint_params lays one out)."""
        hi = self.nenv if hi is None else hi
        p, pp = self._env_array(params, hi - lo, int(self.lib.mjb_env_joint_stride(self.cm.ptr)))
        _check(self.lib.mjb_set_env_joint_params(self.ptr, lo, hi, pp), "mjb_set_env_joint_params")

    # ---- device-side DefaultRobotHWSim (mjb_hwsim_*) ----
    def hwsim_configure(self, joints):
        """joints: list of dicts(joint=<id>, method=..., kind=..., p, i, d, i_max, i_min, antiwindup, effort_limit, lower, upper)."""
        arr = (binding.HwsimJoint * max(1, len(joints)))()
        for k, j in enumerate(joints):
            arr[k] = binding.HwsimJoint(int(j["joint"]), binding.HW_METHODS[j.get("method", "effort")],
                                        binding.HW_KINDS[j.get("kind", "revolute")], int(j.get("antiwindup", 0)),
                                        float(j.get("p", 0)), float(j.get("i", 0)), float(j.get("d", 0)),
                                        float(j.get("i_max", 0)), float(j.get("i_min", 0)), float(j.get("effort_limit", 0)),
                                        float(j.get("lower", 0)), float(j.get("upper", 0)))
        _check(self.lib.mjb_hwsim_configure(self.ptr, len(joints), arr), "mjb_hwsim_configure")
        self._hw_n = len(joints)

    def hwsim_set_command(self, which, cmd, lo=0, hi=None):
        import numpy as np
        hi = self.nenv if hi is None else hi
        a = np.ascontiguousarray(cmd, dtype=np.float64).reshape(hi - lo, self._hw_n)
        _check(self.lib.mjb_hwsim_set_command(self.ptr, {"position": 0, "velocity": 1, "effort": 2}[which], lo, hi,
                                              a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_hwsim_set_command")

    def hwsim_set_period(self, control_period):
        """Controller cadence of MujocoRosControlPlugin::controlCallback (mjb_hwsim_set_period); <= 0 switches it off."""
        _check(self.lib.mjb_hwsim_set_period(self.ptr, float(control_period)), "mjb_hwsim_set_period")

    def hwsim_estop(self, active):
        _check(self.lib.mjb_hwsim_estop(self.ptr, 1 if active else 0), "mjb_hwsim_estop")

    # ---- sensors-plugin equivalent (mjb_sensor_*) ----
    def sensor_set_noise(self, sensor, set_flag, mean=(0, 0, 0), sigma=(0, 0, 0)):
        """registerNoiseModels: bit k of set_flag = noise on component k; the n-th set bit uses mean[n], sigma[n]."""
        import numpy as np
        mu = np.zeros(3)
        sg = np.zeros(3)
        mu[:len(mean)] = mean
        sg[:len(sigma)] = sigma
        pd = C.POINTER(C.c_double)
        _check(self.lib.mjb_sensor_set_noise(self.ptr, int(sensor), int(set_flag), mu.ctypes.data_as(pd), sg.ctypes.data_as(pd)),
               "mjb_sensor_set_noise")

    def sensor_pack(self, seed=0):
        _check(self.lib.mjb_sensor_pack(self.ptr, int(seed)), "mjb_sensor_pack")

    def sensor_messages(self, which="value", lo=0, hi=None):
        """float32 [hi-lo, nsensordata]: 'value' (with noise models applied) or 'truth' (sensordata / cutoff)."""
        import numpy as np
        hi = self.nenv if hi is None else hi
        out = np.empty((hi - lo, self.cm.model["nsensordata"]), dtype=np.float32)
        _check(self.lib.mjb_sensor_get(self.ptr, 0 if which == "value" else 1, lo, hi, out.ctypes.data_as(C.POINTER(C.c_float))),
               "mjb_sensor_get")
        return out

    # ---- batched ray casting (mjb_rays_*) ----
    def set_rays(self, site, vec, pnt=None, exclude_own_body=True, geom_mask=None):
        """The ray set every env casts (mjb_rays_configure): vec [nray, 3] (and pnt [nray, 3], default the origin) in the frame of `site` -- a site id, a
        site name, or one of either per ray; -1 = the world frame.  vec is not normalised: distances come in units of |vec|.  exclude_own_body (a bool or one
        per ray) skips the geoms of the site's body; geom_mask [ngeom] (0 = skip) replaces the default rule, which skips geoms with alpha 0.  A second call
        replaces the first.  pinhole_rays / lidar_rays build common patterns."""
        vec = np.ascontiguousarray(np.asarray(vec, dtype=np.float64).reshape(-1, 3))
        n = vec.shape[0]
        sites = [site] * n if isinstance(site, (str, int, np.integer)) else list(site)
        if len(sites) != n:
            raise ValueError(f"set_rays: {len(sites)} sites for {n} rays")
        names = self.cm.model["names"]["site"] if any(isinstance(s, str) for s in sites) else ()
        unknown = [s for s in sites if isinstance(s, str) and s not in names]
        if unknown:
            raise ValueError(f"set_rays: no site named {unknown[0]!r}")
        sid = np.ascontiguousarray([names.index(s) if isinstance(s, str) else int(s) for s in sites], dtype=np.int32)
        pd, pb = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        p = None if pnt is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pnt, dtype=np.float64), (n, 3)))
        ex = np.ascontiguousarray(np.broadcast_to(np.asarray(exclude_own_body, dtype=bool), (n,)), dtype=np.uint8)
        gm = None
        if geom_mask is not None:
            gm = np.ascontiguousarray(np.asarray(geom_mask).reshape(-1) != 0, dtype=np.uint8)
            if gm.size != int(self.cm.model["ngeom"]):
                raise ValueError(f"set_rays: geom_mask has {gm.size} entries, the model {int(self.cm.model['ngeom'])} geoms")
        _check(self.lib.mjb_rays_configure(self.ptr, n, sid.ctypes.data_as(C.POINTER(C.c_int)), None if p is None else p.ctypes.data_as(pd), vec.ctypes.data_as(pd),
                                           ex.ctypes.data_as(pb), None if gm is None else gm.ctypes.data_as(pb)), "mjb_rays_configure")

    def cast_rays_async(self):
        """Cast the configured rays of every env on the batch's stream (mjb_rays_cast); needs current frames: forward(), step1() / step2(), or step() with
        set_keep_frame().  The results stay on the device (rays_device_ptr) until cast_rays or the next cast."""
        _check(self.lib.mjb_rays_cast(self.ptr), "mjb_rays_cast")

    def cast_rays(self, lo=0, hi=None):
        """Cast, wait, and return (dist float64 [hi-lo, nray], geomid int32 [hi-lo, nray]) of envs [lo, hi): the distance to the nearest geom along each ray in
        units of |vec| and that geom's id, -1 and -1 for a miss."""
        hi = self.nenv if hi is None else hi
        self.cast_rays_async()
        n = int(self.lib.mjb_rays_count(self.ptr))
        dist = np.empty((hi - lo, n), dtype=np.float64)
        gid = np.empty((hi - lo, n), dtype=np.int32)
        _check(self.lib.mjb_rays_get(self.ptr, lo, hi, dist.ctypes.data_as(C.POINTER(C.c_double)), gid.ctypes.data_as(C.POINTER(C.c_int))), "mjb_rays_get")
        return dist, gid

    def rays_device_ptr(self, which):
        """Device address of the ray results: 0 = dist [nenv, nray] float64, 1 = geomid [nenv, nray] int32 (mjb_rays_device_ptr)."""
        p = self.lib.mjb_rays_device_ptr(self.ptr, int(which))
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    # ---- batched Jacobians (mjb_jac_*) ----
    _JAC_KINDS = {"site": 0, "body": 1, "bodycom": 2, "geom": 3}   # MJB_JAC_SITE ... of include/mjb.h; a body's names serve "bodycom" too
    _JAC_OUTPUTS = {"J": 1, "MinvJT": 2, "Ainv": 4, "vel": 8}      # MJB_JAC_OUT_*

    def _jac_shape(self, key, n, npoint):
        nv = int(self.cm.model["nv"])
        return {"J": (n, npoint, 6, nv), "MinvJT": (n, npoint, 6, nv), "Ainv": (n, npoint, 6, 6), "vel": (n, npoint, 6)}[key]

    def _resolve_points(self, who, points):
        """(object types, ids) as int32 arrays of a point list in set_jac_points' form"""
        pts = [("site", p) if isinstance(p, (str, int, np.integer)) else tuple(p) for p in points]
        n = len(pts)
        ty, oid = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k, (kind, ref) in enumerate(pts):
            if kind not in self._JAC_KINDS:
                raise ValueError(f"{who}: unknown kind {kind!r} (site, body, bodycom, geom)")
            ty[k] = self._JAC_KINDS[kind]
            if isinstance(ref, str):
                names = self.cm.model["names"]["body" if kind == "bodycom" else kind]
                if ref not in names:
                    raise ValueError(f"{who}: no {kind} named {ref!r}")
                ref = names.index(ref)
            oid[k] = int(ref)
        return ty, oid

    def set_jac_points(self, points, outputs=("J",), pnt=None):
        """The points whose Jacobians every env evaluates (mjb_jac_configure): `points` is a sequence of site names or ids, or of (kind, name_or_id)
        pairs with kind one of "site", "body", "bodycom", "geom" (mj_jacSite / mj_jacBody / mj_jacBodyCom / mj_jacGeom).  pnt [npoint, 3], default 0,
        moves a point off its object's origin, in the object's own frame.  outputs: any of "J", "MinvJT", "Ainv", "vel" -- only these are allocated
        and computed.  A second call replaces the first."""
        ty, oid = self._resolve_points("set_jac_points", points)
        n = len(ty)
        outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        unknown = [o for o in outs if o not in self._JAC_OUTPUTS]
        if unknown:
            raise ValueError(f"set_jac_points: unknown output {unknown[0]!r} (J, MinvJT, Ainv, vel)")
        bits = 0
        for o in outs:
            bits |= self._JAC_OUTPUTS[o]
        p = None if pnt is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pnt, dtype=np.float64), (n, 3)))
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        _check(self.lib.mjb_jac_configure(self.ptr, n, ty.ctypes.data_as(pi), oid.ctypes.data_as(pi), None if p is None else p.ctypes.data_as(pd), bits),
               "mjb_jac_configure")
        self._jac_outputs = tuple(k for k in self._JAC_OUTPUTS if bits & self._JAC_OUTPUTS[k])

    def eval_jacobians_async(self):
        """Evaluate the configured outputs for every env on the batch's stream (mjb_jac_eval); needs current frames: forward(), step1() / step2(), or
        step() with set_keep_frame() -- after a step the frame, and so J, belongs to the poses before the integration.  The results stay on the device
        (jac_device_ptr) until jacobians() or the next evaluation."""
        _check(self.lib.mjb_jac_eval(self.ptr), "mjb_jac_eval")

    def jacobians(self, lo=0, hi=None):
        """Evaluate, wait, and return the configured outputs of envs [lo, hi) as a dict of float64 arrays: "J" [n, npoint, 6, nv] (rows 0-2 translational,
        3-5 rotational, world axes), "MinvJT" [n, npoint, 6, nv] (row r = M^-1 J[r]'), "Ainv" [n, npoint, 6, 6] (J M^-1 J') and "vel" [n, npoint, 6]
        (J qvel: linear, then angular)."""
        hi = self.nenv if hi is None else hi
        self.eval_jacobians_async()
        npoint = int(self.lib.mjb_jac_count(self.ptr))
        out = {}
        for key in getattr(self, "_jac_outputs", ()):
            a = np.empty(self._jac_shape(key, hi - lo, npoint), dtype=np.float64)
            _check(self.lib.mjb_jac_get(self.ptr, self._JAC_OUTPUTS[key], lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_jac_get")
            out[key] = a
        return out

    def jac_device_ptr(self, which):
        """Device address of one output, by name ("J", "MinvJT", "Ainv", "vel") or MJB_JAC_OUT_* bit: float64, env-major, the shapes of jacobians()."""
        if isinstance(which, str) and which not in self._JAC_OUTPUTS:
            raise ValueError(f"jac_device_ptr: unknown output {which!r} (J, MinvJT, Ainv, vel)")
        p = self.lib.mjb_jac_device_ptr(self.ptr, self._JAC_OUTPUTS[which] if isinstance(which, str) else int(which))
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    # ---- batched joint-space dynamics (mjb_dyn_*) ----
    _DYN_OUTPUTS = {"M": 1, "MV": 2, "MinvV": 4, "ID": 8, "Jdotv": 16}   # MJB_DYN_OUT_* of include/mjb.h
    _DYN_IN_V = 256                                                       # MJB_DYN_IN_V

    def _dyn_counts(self):
        nvec, npoint = C.c_int(0), C.c_int(0)
        _check(self.lib.mjb_dyn_count(self.ptr, C.byref(nvec), C.byref(npoint)), "mjb_dyn_count")
        return nvec.value, npoint.value

    def _dyn_shape(self, key, n):
        nv = int(self.cm.model["nv"])
        nvec, npoint = self._dyn_counts()
        return (n, nv, nv) if key == "M" else ((n, npoint, 6) if key == "Jdotv" else (n, nvec, nv))

    def set_dynamics(self, nvec=0, outputs=("M",), points=None, pnt=None):
        """What every env evaluates of its joint-space dynamics (mjb_dyn_configure).  outputs: any of "M" (dense mass matrix, mj_fullM), "MV" (M V[k],
        mj_mulM), "MinvV" (M^-1 V[k], mj_solveM), "ID" ((M V[k] + qfrc_bias) - qfrc_passive: the generalized force under which qacc = V[k]) and "Jdotv"
        (Jdot qvel of the points, linear then angular) -- only these are allocated and computed.  nvec: vectors per env of the input block V, which the
        batch owns, zero from here on (set_dyn_vectors, or dyn_device_ptr("V")).  points / pnt: the points of "Jdotv", as in set_jac_points.  A second call
        replaces the first."""
        outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        unknown = [o for o in outs if o not in self._DYN_OUTPUTS]
        if unknown:
            raise ValueError(f"set_dynamics: unknown output {unknown[0]!r} (M, MV, MinvV, ID, Jdotv)")
        bits = 0
        for o in outs:
            bits |= self._DYN_OUTPUTS[o]
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        n, ty, oid, p = 0, None, None, None
        if points is not None:
            ty, oid = self._resolve_points("set_dynamics", points)
            n = len(ty)
            p = None if pnt is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pnt, dtype=np.float64), (n, 3)))
        _check(self.lib.mjb_dyn_configure(self.ptr, int(nvec), n, None if ty is None else ty.ctypes.data_as(pi), None if oid is None else oid.ctypes.data_as(pi),
                                          None if p is None else p.ctypes.data_as(pd), bits), "mjb_dyn_configure")
        self._dyn_outputs = tuple(k for k in self._DYN_OUTPUTS if bits & self._DYN_OUTPUTS[k])

    def set_dyn_vectors(self, V, lo=0, hi=None):
        """Write the input vectors of envs [lo, hi) from the host (mjb_dyn_set_vectors): V [n, nvec, nv], or [n, nv] when nvec is 1."""
        hi = self.nenv if hi is None else hi
        nvec, _ = self._dyn_counts()
        a = np.ascontiguousarray(np.asarray(V, dtype=np.float64).reshape(hi - lo, nvec, int(self.cm.model["nv"])))
        _check(self.lib.mjb_dyn_set_vectors(self.ptr, lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_dyn_set_vectors")

    def eval_dynamics_async(self):
        """Evaluate the configured outputs for every env on the batch's stream (mjb_dyn_eval); needs current frames: forward(), step1() / step2(), or
        step() with set_keep_frame() -- after a step the frame belongs to the state before the integration.  "ID" and "Jdotv" also refuse a qvel written
        since.  The results stay on the device (dyn_device_ptr) until dynamics() or the next evaluation."""
        _check(self.lib.mjb_dyn_eval(self.ptr), "mjb_dyn_eval")

    def dynamics(self, lo=0, hi=None):
        """Evaluate, wait, and return the configured outputs of envs [lo, hi) as a dict of float64 arrays: "M" [n, nv, nv], "MV" / "MinvV" / "ID"
        [n, nvec, nv] and "Jdotv" [n, npoint, 6] (linear, then angular, world axes)."""
        hi = self.nenv if hi is None else hi
        self.eval_dynamics_async()
        out = {}
        for key in getattr(self, "_dyn_outputs", ()):
            a = np.empty(self._dyn_shape(key, hi - lo), dtype=np.float64)
            _check(self.lib.mjb_dyn_get(self.ptr, self._DYN_OUTPUTS[key], lo, hi, a.ctypes.data_as(C.POINTER(C.c_double))), "mjb_dyn_get")
            out[key] = a
        return out

    def dyn_device_ptr(self, which):
        """Device address of one output by name ("M", "MV", "MinvV", "ID", "Jdotv") or MJB_DYN_OUT_* bit, or of the input block ("V", [nenv, nvec, nv]):
        float64, env-major, the shapes of dynamics()."""
        if isinstance(which, str) and which != "V" and which not in self._DYN_OUTPUTS:
            raise ValueError(f"dyn_device_ptr: unknown name {which!r} (M, MV, MinvV, ID, Jdotv, V)")
        bit = (self._DYN_IN_V if which == "V" else self._DYN_OUTPUTS[which]) if isinstance(which, str) else int(which)
        p = self.lib.mjb_dyn_device_ptr(self.ptr, bit)
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    # ---- batched contact wrenches (mjb_contact_*) ----
    _CON_OUTPUTS = {"wrench": 1, "normal": 2, "count": 4, "dist": 8, "contacts": 16}   # MJB_CON_OUT_* of include/mjb.h

    def _geom_mask(self, geoms, what):
        m = self.cm.model
        ngeom = int(m["ngeom"])
        mask = np.zeros(ngeom, np.uint8)
        for g in ([geoms] if isinstance(geoms, (str, int, np.integer)) else list(geoms)):
            if isinstance(g, str):
                if g not in m["names"]["geom"]:
                    raise ValueError(f"set_contact_queries: {what}: no geom named {g!r}")
                g = m["names"]["geom"].index(g)
            g = int(g)
            if not 0 <= g < ngeom:
                raise ValueError(f"set_contact_queries: {what}: geom {g} outside [0, {ngeom})")
            mask[g] = 1
        return mask

    def set_contact_queries(self, queries, outputs=("wrench",), ref_body=None):
        """The queries every env evaluates (mjb_contact_configure): `queries` is a list of (A, B) pairs of geom sets, each a sequence of geom ids or geom
        names (geoms_of_bodies builds one from bodies); B = None means every geom not in A.  A contact (g1, g2) matches with sign +1 when g2 is in A and
        g1 in B, with sign -1 when g1 is in A and g2 in B; A and B must be disjoint and neither may be empty.  ref_body: one body id or name per query
        (or one for all) about whose xpos the torque of "wrench" is taken; None or -1 = the world origin.  outputs: any of "wrench", "normal", "count",
        "dist", "contacts" -- only these are allocated and computed.  A second call replaces the first."""
        m = self.cm.model
        qs = list(queries)
        n, ngeom = len(qs), int(m["ngeom"])
        ga, gb = np.zeros((max(n, 1), ngeom), np.uint8), np.zeros((max(n, 1), ngeom), np.uint8)
        for q, (A, B) in enumerate(qs):
            ga[q] = self._geom_mask(A, f"query {q}, A")
            gb[q] = (1 - ga[q]) if B is None else self._geom_mask(B, f"query {q}, B")
        refs = [ref_body] * n if ref_body is None or isinstance(ref_body, (str, int, np.integer)) else list(ref_body)
        if len(refs) != n:
            raise ValueError(f"set_contact_queries: {len(refs)} ref_body entries for {n} queries")
        unknown = [r for r in refs if isinstance(r, str) and r not in m["names"]["body"]]
        if unknown:
            raise ValueError(f"set_contact_queries: no body named {unknown[0]!r}")
        rb = np.ascontiguousarray([-1 if r is None else (m["names"]["body"].index(r) if isinstance(r, str) else int(r)) for r in refs] or [-1], dtype=np.int32)
        outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        unknown = [o for o in outs if o not in self._CON_OUTPUTS]
        if unknown:
            raise ValueError(f"set_contact_queries: unknown output {unknown[0]!r} (wrench, normal, count, dist, contacts)")
        bits = 0
        for o in outs:
            bits |= self._CON_OUTPUTS[o]
        pb = C.POINTER(C.c_uint8)
        _check(self.lib.mjb_contact_configure(self.ptr, n, ga.ctypes.data_as(pb), gb.ctypes.data_as(pb), rb.ctypes.data_as(C.POINTER(C.c_int)), bits), "mjb_contact_configure")
        self._con_outputs = tuple(k for k in self._CON_OUTPUTS if bits & self._CON_OUTPUTS[k])

    def eval_contact_wrenches_async(self):
        """Evaluate the configured outputs for every env on the batch's stream (mjb_contact_eval); needs current frames WITH their efc_force: forward(),
        step2(), or step() with set_keep_frame() -- not between step1() and step2().  After a step the frame holds the contacts and forces before the
        integration.  The results stay on the device (contact_device_ptr) until contact_wrenches() or the next evaluation."""
        _check(self.lib.mjb_contact_eval(self.ptr), "mjb_contact_eval")

    def contact_wrenches(self, lo=0, hi=None):
        """Evaluate, wait, and return the configured outputs of envs [lo, hi) as a dict of arrays: "wrench" float64 [n, nquery, 6] (net force, then torque
        about r_q, in world axes, that the B side exerts on the A side), "normal" float64 [n, nquery] (sum of the normal forces lf[0]), "count" int32
        [n, nquery], "dist" float64 [n, nquery] (smallest contact_dist, +inf without a matching contact) and "contacts" float64 [n, nconmax, 6] (lf of
        every contact in its own frame, normal first; 0.0 beyond ncon)."""
        hi = self.nenv if hi is None else hi
        self.eval_contact_wrenches_async()
        n, nq, ncm = hi - lo, int(self.lib.mjb_contact_count(self.ptr)), int(self.cm.model["nconmax"])
        shapes = {"wrench": (n, nq, 6), "normal": (n, nq), "count": (n, nq), "dist": (n, nq), "contacts": (n, ncm, 6)}
        out = {}
        for key in getattr(self, "_con_outputs", ()):
            a = np.empty(shapes[key], dtype=np.int32 if key == "count" else np.float64)
            _check(self.lib.mjb_contact_get(self.ptr, self._CON_OUTPUTS[key], lo, hi, a.ctypes.data_as(C.c_void_p)), "mjb_contact_get")
            out[key] = a
        return out

    def contact_device_ptr(self, which):
        """Device address of one output, by name ("wrench", "normal", "count", "dist", "contacts") or MJB_CON_OUT_* bit: env-major, the shapes and dtypes of
        contact_wrenches()."""
        if isinstance(which, str) and which not in self._CON_OUTPUTS:
            raise ValueError(f"contact_device_ptr: unknown output {which!r} (wrench, normal, count, dist, contacts)")
        p = self.lib.mjb_contact_device_ptr(self.ptr, self._CON_OUTPUTS[which] if isinstance(which, str) else int(which))
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    # ---- device-side episode resets (mjb_episode_*) ----
    _EPISODE_PTRS = {"done": 0, "episode": 1, "ndone": 2}

    def set_episode_init(self, qpos=None, qvel=None, act=None):
        """The initial-state bank a reset env starts from (mjb_episode_set_init): qpos [ninit, nq], optionally qvel [ninit, nv] and act [ninit, na] (default
        zeros); each reset draws one row.  qpos=None clears the bank: qpos0, zero velocity, zero activation."""
        m = self.cm.model
        pd = C.POINTER(C.c_double)
        if qpos is None:
            _check(self.lib.mjb_episode_set_init(self.ptr, 0, None, None, None), "mjb_episode_set_init")
            return
        q = np.ascontiguousarray(np.asarray(qpos, dtype=np.float64).reshape(-1, int(m["nq"])))
        n = q.shape[0]
        v = None if qvel is None else np.ascontiguousarray(np.asarray(qvel, dtype=np.float64).reshape(n, int(m["nv"])))
        a = None if act is None else np.ascontiguousarray(np.asarray(act, dtype=np.float64).reshape(n, int(m["na"])))
        _check(self.lib.mjb_episode_set_init(self.ptr, n, q.ctypes.data_as(pd), None if v is None else v.ctypes.data_as(pd), None if a is None else a.ctypes.data_as(pd)),
               "mjb_episode_set_init")

    def set_episode_noise(self, seed, qpos_range=None, qvel_range=None, clamp=False, env_offset=0):
        """Seeded noise on the bank row (mjb_episode_set_noise): qpos_range / qvel_range are (lo, hi) pairs of [nv] arrays (or scalars) in tangent space, a
        uniform draw per dof and reset; None: no perturbation of that part.  clamp clips limited hinge / slide joints to jnt_range.  The draws are keyed by
        (seed, env_offset + env, the env's episode count, dof): shards of one population pass their first env's global index as env_offset."""
        nv = int(self.cm.model["nv"])
        pd = C.POINTER(C.c_double)
        keep, args = [], []
        for r in (qpos_range, qvel_range):
            for end in ((None, None) if r is None else r):
                if end is None:
                    args.append(None)
                else:
                    keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(end, dtype=np.float64), (nv,))))
                    args.append(keep[-1].ctypes.data_as(pd))
        _check(self.lib.mjb_episode_set_noise(self.ptr, int(seed), int(env_offset), args[0], args[1], args[2], args[3], 1 if clamp else 0), "mjb_episode_set_noise")

    def set_episode_rule(self, time_limit=0.0, qpos_box=None):
        """When an episode is over (mjb_episode_set_rule): time >= time_limit (<= 0: no time rule), or a qpos coordinate outside qpos_box = (lo, hi), [nq]
        arrays either of which may be None; a NaN coordinate is outside, an infinite bound is none."""
        nq = int(self.cm.model["nq"])
        pd = C.POINTER(C.c_double)
        lo, hi = (None, None) if qpos_box is None else qpos_box
        lo = None if lo is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (nq,)))
        hi = None if hi is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (nq,)))
        _check(self.lib.mjb_episode_set_rule(self.ptr, float(time_limit), None if lo is None else lo.ctypes.data_as(pd), None if hi is None else hi.ctypes.data_as(pd)),
               "mjb_episode_set_rule")

    def _episode_mask(self, mask):
        """A mask argument as a device address: None, an int (a device pointer to nenv bytes, e.g. tensor.data_ptr() or another batch's done buffer), or
        an array, which is uploaded.  The upload waits for the stream and goes into this batch's own done buffer -- the kernel has read an env's mask
        byte before it writes the env's done byte, so the two may be one array.  Pass a device address to stay asynchronous."""
        if mask is None or isinstance(mask, (int, np.integer)):
            return None if mask is None else int(mask)
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if m.shape != (self.nenv,):
            raise ValueError("mask must have shape (nenv,)")
        dst = self.episode_device_ptr("done")
        self.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipMemcpy(dst, m.ctypes.data, m.nbytes, 1) != 0:
            raise EngineError("episode mask upload failed")
        return dst

    def episode_reset(self, mask=None):
        """Reset the envs of `mask` (None: every env) to a drawn initial state on the batch's stream, without a synchronise (mjb_episode_reset); the rule
        is ignored.  Derived fields are unreadable until forward() or a step."""
        _check(self.lib.mjb_episode_reset(self.ptr, self._episode_mask(mask)), "mjb_episode_reset")

    def episode_step(self, extra_mask=None):
        """Evaluate the done rule for every env, OR extra_mask in, and reset the done envs, in one launch on the batch's stream (mjb_episode_step).  The
        decisions stay on the device (episode_device_ptr) until episode_done() / episode_ndone()."""
        _check(self.lib.mjb_episode_step(self.ptr, self._episode_mask(extra_mask)), "mjb_episode_step")

    def episode_done(self, lo=0, hi=None):
        """Wait, and return done uint8 [hi-lo] of the last episode_step / episode_reset."""
        hi = self.nenv if hi is None else hi
        out = np.zeros(max(hi - lo, 0), dtype=np.uint8)
        _check(self.lib.mjb_episode_get(self.ptr, lo, hi, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None), "mjb_episode_get")
        return out

    def episode_counts(self, lo=0, hi=None):
        """Wait, and return the resets so far of envs [lo, hi) as uint32: the episode index of an env's next draw."""
        hi = self.nenv if hi is None else hi
        out = np.zeros(max(hi - lo, 0), dtype=np.uint32)
        _check(self.lib.mjb_episode_get(self.ptr, lo, hi, None, out.ctypes.data_as(C.POINTER(C.c_uint32)), None), "mjb_episode_get")
        return out

    def episode_ndone(self):
        """Wait, and return how many envs the last episode_step / episode_reset found done."""
        n = C.c_uint32(0)
        _check(self.lib.mjb_episode_get(self.ptr, 0, 0, None, None, C.byref(n)), "mjb_episode_get")
        return int(n.value)

    def episode_device_ptr(self, name):
        """Device address of "done" [nenv] uint8, "episode" [nenv] uint32 or "ndone" (one uint32), or of the same by number (mjb_episode_device_ptr)."""
        if isinstance(name, str) and name not in self._EPISODE_PTRS:
            raise ValueError(f"episode_device_ptr: unknown buffer {name!r} (done, episode, ndone)")
        p = self.lib.mjb_episode_device_ptr(self.ptr, self._EPISODE_PTRS[name] if isinstance(name, str) else int(name))
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    def set_keep_frame(self, on=True):
        """Fused step() also leaves the derived fields of its last step readable through get()."""
        _check(self.lib.mjb_set_keep_frame(self.ptr, 1 if on else 0), "mjb_set_keep_frame")

    def set_ctrl_noise(self, std, rate, seed=0, env_offset=0):
        _check(self.lib.mjb_set_ctrl_noise(self.ptr, float(std), float(rate), int(seed), int(env_offset)),
               "mjb_set_ctrl_noise")

    def set_stats(self, on=True):
        """Start (and zero) / stop the device-side workload statistics of the constrained kernels (mjb_set_stats)."""
        _check(self.lib.mjb_set_stats(self.ptr, 1 if on else 0), "mjb_set_stats")

    def stats(self):
        """dict(evaluations, solver_iter_mean, ncon_{mean,p50,p99,max}, nefc_{mean,p50,p99,max}, rows_gt64_share, nefc_hist, ncon_hist)."""
        out = (C.c_ulonglong * 388)()
        _check(self.lib.mjb_get_stats(self.ptr, out), "mjb_get_stats")
        a = np.array(out[:], dtype=np.float64)
        n = a[0]
        he, hc = a[2:259], a[259:388]

        def summary(h):
            tot = h.sum()
            if tot <= 0:
                return 0.0, 0, 0, 0
            c = np.cumsum(h)
            q = lambda f: int(np.searchsorted(c, f * tot, side="left"))
            return float((h * np.arange(len(h))).sum() / tot), q(0.5), q(0.99), int(np.nonzero(h)[0].max())
        em, e50, e99, emx = summary(he)
        cm, c50, c99, cmx = summary(hc)
        return {"evaluations": int(n), "solver_iter_mean": float(a[1] / n) if n else 0.0,
                "ncon_mean": cm, "ncon_p50": c50, "ncon_p99": c99, "ncon_max": cmx,
                "nefc_mean": em, "nefc_p50": e50, "nefc_p99": e99, "nefc_max": emx,
                "rows_gt64_share": float(he[65:].sum() / he.sum()) if he.sum() else 0.0,
                "nefc_hist": he.astype(np.int64), "ncon_hist": hc.astype(np.int64)}

    def fused_frame(self):
        """(id, bytes) of the fused frame the batch's launches currently run on: 1 default, 2 wide (mjb_fused_frame)."""
        fid = int(self.lib.mjb_fused_frame(self.ptr))
        return fid, int(self.lib.mjb_frame_bytes(self.cm.ptr, fid))

    def noise_mode(self):
        """How the last fused launch got its ctrl-noise normals (mjb_noise_mode)."""
        return ("in-kernel", "same-stream", "side-stream")[int(self.lib.mjb_noise_mode(self.ptr))]

    def set_lane_env(self, mode):
        """-1 automatic, 0 never, 1 whenever eligible, 2 whenever eligible -- also when the batch carries per-env gravity or parameter blocks
        (set_env_gravity, set_env_body_mass, set_env_dof_params, set_env_joint_stiffness, set_env_actuator_params, ...), which the kernel then reads
        per env; such a batch runs the generic kernels in every other mode: the lane = env form of the unconstrained fused step (mjb_set_lane_env).
        Models with actuator activation states (integrator / filter; <intvelocity>, <cylinder>) are eligible too: the kernel carries `act` between
        get("act") / set("act") and the generic kernels, in its one-wavefront form; not together with a device hwsim stage.
        A hinge / slide tree whose only constraint rows are joint limits under PGS is eligible too (no contacts, equalities, tendons or frictionloss): in
        modes 1 and 2 its launches run the kernel's one-wavefront form with the constraint stage (joint-limit rows, PGS with warmstart) inside, and
        get("qfrc_constraint") / get("nefc") / get("solver_iter") read the last step's values afterwards; the automatic mode keeps the generic kernels for
        such a model, and so does a batch with per-env overrides, a hwsim stage or a written xfrc_applied.
        The same holds for a model with fixed tendons that only carry actuators (actuators with a tendon transmission) and with joint equalities, whose
        rows join the limit rows under PGS at exact njmax (CompiledModel.lane_env_rows()); per-env equality parameters (set_env_equality) keep the
        generic kernels."""
        _check(self.lib.mjb_set_lane_env(self.ptr, int(mode)), "mjb_set_lane_env")

    def set_lane_env_hwsim(self, on=True):
        """Opt-in: a batch with the device hwsim stage (hwsim_configure) may run the lane = env kernel, in its one-wavefront build that carries the
        stage; off (the default), such a batch runs the generic kernels (mjb_lane_env_set_hwsim)."""
        _check(self.lib.mjb_lane_env_set_hwsim(self.ptr, 1 if on else 0), "mjb_lane_env_set_hwsim")

    def set_lane_env_xfrc(self, on=True):
        """Opt-in: a batch whose xfrc_applied has been written may run the lane = env kernel, in its one-wavefront build that applies the wrenches
        (with mode 2: together with the per-env overlay); off (the default), such a batch runs the generic kernels (mjb_lane_env_set_xfrc)."""
        _check(self.lib.mjb_lane_env_set_xfrc(self.ptr, 1 if on else 0), "mjb_lane_env_set_xfrc")

    def lane_env_info(self):
        """(compiled-in topology index or -1, the last fused launch ran the lane = env kernel)."""
        used = C.c_int(0)
        topo = int(self.lib.mjb_lane_env_info(self.ptr, C.byref(used)))
        return topo, bool(used.value)

    def set_sensors_every_step(self, on=True):
        """The lane = env kernel evaluates the sensor stages at every step of a fused launch instead of its last one (mjb_set_sensors_every_step)."""
        _check(self.lib.mjb_set_sensors_every_step(self.ptr, 1 if on else 0), "mjb_set_sensors_every_step")

    def set_split_step(self, mode):
        """-1 automatic, 0 never, 1 whenever eligible: the split step of plain-PGS models -- smooth stages one env per lane, constraint stages one env
        per wavefront (mjb_set_split_step)."""
        _check(self.lib.mjb_set_split_step(self.ptr, int(mode)), "mjb_set_split_step")

    def split_step_info(self):
        """(topology index or -1, the last fused launch ran as a split step, its env slices)."""
        used, slices = C.c_int(0), C.c_int(0)
        topo = int(self.lib.mjb_split_step_info(self.ptr, C.byref(used), C.byref(slices)))
        return topo, bool(used.value), int(slices.value)

    def set_lane_env_form(self, form):
        """Process-wide: -1 by batch size, 0 one wavefront per 64 envs, 1 two (position / velocity halves), 2 two, pipelined (mjb_lane_env_set_form)."""
        return int(self.lib.mjb_lane_env_set_form(int(form)))

    def lane_env_last_form(self):
        return int(self.lib.mjb_lane_env_last_form())

    def set_lane_env_sweep_waves(self, waves):
        """Process-wide: form 3's sweep on 3 or 4 wavefronts, 0 = the launcher's rule (mjb_lane_env_set_sweep_waves).  Returns the previous setting."""
        return int(self.lib.mjb_lane_env_set_sweep_waves(int(waves)))

    def lane_env_last_sweep_waves(self):
        """3 / 4: the sweep wavefronts of the last lane = env launch if it ran form 3, else 0."""
        return int(self.lib.mjb_lane_env_last_sweep_waves())

    def lane_env_error(self):
        """Why the hiprtc build of this process's last lane = env topology was not available ('' if none failed)."""
        return self.lib.mjb_lane_env_error().decode()

    def time_steps(self, nsteps, nlaunch):
        ms = C.c_double(0)
        _check(self.lib.mjb_time_steps(self.ptr, int(nsteps), int(nlaunch), C.byref(ms)), "mjb_time_steps")
        return ms.value

    # ---- data access (env-major numpy arrays)
    def get(self, name, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        fid = Field.ids[name]
        n = self.cm.field_size(name)
        if Field.kinds[name] == "DI":
            out = np.zeros((hi - lo, n), dtype=np.int32)
            _check(self.lib.mjb_get_int(self.ptr, fid, lo, hi, out.ctypes.data_as(C.POINTER(C.c_int))), "mjb_get_int")
        else:
            out = np.zeros((hi - lo, n), dtype=np.float64)
            _check(self.lib.mjb_get(self.ptr, fid, lo, hi, out.ctypes.data_as(C.POINTER(C.c_double))), "mjb_get")
        return out

    def set(self, name, value, lo=0, hi=None):
        hi = self.nenv if hi is None else hi
        n = self.cm.field_size(name)
        if n == 0:  # (a world without this field -- empty_world has no dof: nothing to write)
            return
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64).reshape(-1, n) if np.ndim(value) > 1
                                                 else np.asarray(value, dtype=np.float64), (hi - lo, n)))
        _check(self.lib.mjb_set(self.ptr, Field.ids[name], lo, hi, v.ctypes.data_as(C.POINTER(C.c_double))), "mjb_set")

    def device_ptr(self, name):
        p = self.lib.mjb_device_ptr(self.ptr, Field.ids[name])
        if not p:
            raise EngineError(self.lib.mjb_last_error().decode())
        return p

    @property
    def stream(self):
        return self.lib.mjb_get_stream(self.ptr)

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.mjb_free_batch(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
