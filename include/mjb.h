/* mjb.h — C-ABI of the MI355X-native batched MuJoCo-style step engine (libmjb.so).
 *
 * This is the drop-in boundary for the ONE hot path of ubi-agni/mujoco_ros_pkgs: the `mj_step` loop
 * inside `MujocoEnv::physicsLoop` (/root/reference mujoco_ros/src/mujoco_env.cpp:436-639).  In the
 * reference that path sits behind the MuJoCo 2.3.7 C API (un-vendored third-party library,
 * mujoco_ros/CMakeLists.txt:61).  Every entry point below names the MuJoCo call, and the reference
 * call site(s), it takes the place of for a batch of N independent env instances that share one
 * constant model.  Plain C: pointers and sizes only, no torch / HIP types in any signature.
 *
 * Error convention: MuJoCo aborts through mju_error; this ABI never aborts or throws.  Functions
 * returning int give 0 on success and a negative MJB_E* code on failure; functions returning a
 * pointer give NULL on failure; mjb_last_error() returns the message of the calling thread's last
 * failure.  The engine has NO CPU fallback: without a usable HIP device every compute entry point
 * fails with MJB_ENODEVICE.
 */
#ifndef MJB_H_
#define MJB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJB_VERSION 100

/* error codes */
#define MJB_OK 0
#define MJB_EINVAL (-1)    /* bad argument / inconsistent model */
#define MJB_ENODEVICE (-2) /* no HIP device / HIP runtime failure */
#define MJB_ENOMEM (-3)
#define MJB_EUNSUPPORTED (-4) /* model uses a feature the engine does not implement */
#define MJB_ERANGE (-5)

/* MuJoCo 2.3.7 enum values used in mjb_model_desc (mjtJoint, mjtGeom, ...) */
enum { MJB_JNT_FREE = 0, MJB_JNT_BALL = 1, MJB_JNT_SLIDE = 2, MJB_JNT_HINGE = 3 };
enum { MJB_GEOM_PLANE = 0, MJB_GEOM_SPHERE = 2, MJB_GEOM_CAPSULE = 3, MJB_GEOM_BOX = 6 };
enum { MJB_INT_EULER = 0, MJB_INT_RK4 = 1, MJB_INT_IMPLICIT = 2, MJB_INT_IMPLICITFAST = 3 };
/* mjtIntegrator.  implicitfast: qacc = (M - h D)^-1 (qfrc_smooth + qfrc_constraint) with D = d qfrc_smooth / d qvel without the Coriolis terms
 * (mjd_passive_vel + mjd_actuator_vel) -- accepted when D is a model constant and diagonal: joint damping, and the velocity terms of affine
 * actuator biases on joint transmissions (a velocity term in an affine GAIN, tendon damping, or a velocity term in the bias of an actuator on a
 * tendon or a site makes mjb_compile refuse it).  mjINT_IMPLICIT
 * (the Coriolis derivatives, an LU factor) is refused. */
enum { MJB_CONE_PYRAMIDAL = 0, MJB_CONE_ELLIPTIC = 1 };
enum { MJB_SOL_PGS = 0, MJB_SOL_CG = 1, MJB_SOL_NEWTON = 2 };
enum { MJB_GAIN_FIXED = 0, MJB_GAIN_AFFINE = 1 };
enum { MJB_BIAS_NONE = 0, MJB_BIAS_AFFINE = 1 };
/* mjtTrn: joint (hinge / slide), fixed-tendon and site transmissions.  jointinparent on a hinge / slide joint is the joint transmission
 * (the loader maps it); slider-crank (2) and body (5) are refused.  actuator_trnid[i][0] is the joint / tendon / site, actuator_trnid[i][1]
 * the refsite of a site transmission (-1: none; MuJoCo's slot for it).  A site transmission's moment depends on the configuration: the
 * kernels compute it at every forward evaluation (mj_transmission, mjTRN_SITE). */
enum { MJB_TRN_JOINT = 0, MJB_TRN_TENDON = 3, MJB_TRN_SITE = 4 };
enum { MJB_DYN_NONE = 0, MJB_DYN_INTEGRATOR = 1, MJB_DYN_FILTER = 2 };  /* mjtDyn (mjDYN_MUSCLE = 3, mjDYN_USER = 4 are refused) */
enum { /* mjtDisableBit */
	MJB_DSBL_CONSTRAINT = 1 << 0, MJB_DSBL_EQUALITY = 1 << 1, MJB_DSBL_FRICTIONLOSS = 1 << 2,
	MJB_DSBL_LIMIT = 1 << 3, MJB_DSBL_CONTACT = 1 << 4, MJB_DSBL_PASSIVE = 1 << 5,
	MJB_DSBL_GRAVITY = 1 << 6, MJB_DSBL_CLAMPCTRL = 1 << 7, MJB_DSBL_WARMSTART = 1 << 8,
	MJB_DSBL_FILTERPARENT = 1 << 9, MJB_DSBL_ACTUATION = 1 << 10, MJB_DSBL_REFSAFE = 1 << 11,
	MJB_DSBL_SENSOR = 1 << 12, MJB_DSBL_EULERDAMP = 1 << 14
};
enum { MJB_ENBL_ENERGY = 1 << 1 }; /* mjtEnableBit (the only one implemented) */
enum { /* mjtWarning: index of mjData.warning[] -- see mjb_warning() */
	MJB_WARN_INERTIA = 0, MJB_WARN_CONTACTFULL = 1, MJB_WARN_CNSTRFULL = 2, MJB_WARN_VGEOMFULL = 3, MJB_WARN_BADQPOS = 4,
	MJB_WARN_BADQVEL = 5, MJB_WARN_BADQACC = 6, MJB_WARN_BADCTRL = 7, MJB_NWARNING = 8
};
enum { /* mjtObj */
	MJB_OBJ_UNKNOWN = 0, MJB_OBJ_BODY = 1, MJB_OBJ_XBODY = 2, MJB_OBJ_JOINT = 3, MJB_OBJ_GEOM = 5,
	MJB_OBJ_SITE = 6, MJB_OBJ_ACTUATOR = 18
};
enum { /* mjtSensor (subset implemented; values are MuJoCo's) */
	MJB_SENS_TOUCH = 0, MJB_SENS_ACCELEROMETER = 1, MJB_SENS_VELOCIMETER = 2, MJB_SENS_GYRO = 3, MJB_SENS_FORCE = 4,
	MJB_SENS_TORQUE = 5, MJB_SENS_MAGNETOMETER = 6, MJB_SENS_RANGEFINDER = 7, MJB_SENS_TENDONPOS = 10, MJB_SENS_TENDONVEL = 11,
	MJB_SENS_JOINTPOS = 8, MJB_SENS_JOINTVEL = 9, MJB_SENS_ACTUATORPOS = 12, MJB_SENS_ACTUATORVEL = 13,
	MJB_SENS_ACTUATORFRC = 14, MJB_SENS_BALLQUAT = 15, MJB_SENS_BALLANGVEL = 16, MJB_SENS_FRAMEPOS = 23,
	MJB_SENS_FRAMEQUAT = 24, MJB_SENS_FRAMEXAXIS = 25, MJB_SENS_FRAMEYAXIS = 26, MJB_SENS_FRAMEZAXIS = 27,
	MJB_SENS_FRAMELINVEL = 28, MJB_SENS_FRAMEANGVEL = 29, MJB_SENS_FRAMELINACC = 30, MJB_SENS_FRAMEANGACC = 31,
	MJB_SENS_SUBTREECOM = 32, MJB_SENS_CLOCK = 35,
	/* round 6: the rest of the scalar / 3-vector types MujocoRosSensorsPlugin serialises (mujoco_ros_sensors/src/mujoco_sensor_handler_plugin.cpp:76-105) */
	MJB_SENS_JOINTLIMITPOS = 17, MJB_SENS_JOINTLIMITVEL = 18, MJB_SENS_JOINTLIMITFRC = 19, MJB_SENS_TENDONLIMITPOS = 20,
	MJB_SENS_TENDONLIMITVEL = 21, MJB_SENS_TENDONLIMITFRC = 22, MJB_SENS_SUBTREELINVEL = 33, MJB_SENS_SUBTREEANGMOM = 34,
	/* (mjSENS_JOINTACTFRC's value in the pinned MuJoCo release cannot be read here -- the library and its headers are absent -- so the engine uses a
	 *  value outside mjtSensor's range; a binding that fills mjb_model_desc from a real mjModel maps mjSENS_JOINTACTFRC onto it) */
	MJB_SENS_JOINTACTFRC = 38
};
enum { MJB_STAGE_NONE = 0, MJB_STAGE_POS = 1, MJB_STAGE_VEL = 2, MJB_STAGE_ACC = 3 };
enum { MJB_EQ_CONNECT = 0, MJB_EQ_WELD = 1, MJB_EQ_JOINT = 2, MJB_EQ_TENDON = 3 }; /* mjtEq (distance not implemented) */
enum { /* mjtConstraint */
	MJB_CNSTR_EQUALITY = 0, MJB_CNSTR_FRICTION_DOF = 1, MJB_CNSTR_FRICTION_TENDON = 2, MJB_CNSTR_LIMIT_JOINT = 3, MJB_CNSTR_LIMIT_TENDON = 4, MJB_CNSTR_CONTACT_FRICTIONLESS = 5, MJB_CNSTR_CONTACT_PYRAMIDAL = 6,
	MJB_CNSTR_CONTACT_ELLIPTIC = 7
};

/* ---- model description: the mjModel arrays the path reads (see mjb_model_fields.def) ---- */
typedef struct mjb_model_desc {
#define MJB_SIZE(name) int name;
#define MJB_OPT_I(name) int name;
#define MJB_OPT_D(name, n) double name[n];
#define MJB_ARR_I(name, rows, cols) const int *name;
#define MJB_ARR_D(name, rows, cols) const double *name;
#include "mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
} mjb_model_desc;

/* ---- per-env data field ids (order of mjb_data_fields.def) ---- */
typedef enum mjb_field {
#define MJB_DS(name, rows, cols) MJB_F_##name,
#define MJB_DD(name, rows, cols) MJB_F_##name,
#define MJB_DD2(name, rows, cols) MJB_F_##name,
#define MJB_DI(name, rows, cols) MJB_F_##name,
#include "mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
	MJB_F_COUNT
} mjb_field;

typedef struct mjb_model mjb_model; /* compiled, immutable model (host copy + device blob) */
typedef struct mjb_batch mjb_batch; /* N env instances on one GPU */

/* Message of the calling thread's last failed call ("" if none). */
const char *mjb_last_error(void);
/* sizeof(mjb_model_desc) of the build: a binding generated from another revision of include/mjb_model_fields.def finds out here, not in a crash. */
int mjb_model_desc_size(void);
int mjb_version(void);
/* Number of usable HIP devices (0 when there is none; never fails). */
int mjb_device_count(void);

/* Validate + copy a model description.  Takes the place of `mj_loadXML`/`mj_loadModel` for the
 * batched path (reference: mujoco_env.cpp:836-843); the arrays are copied, `desc` may be freed.
 * Caps of the one-env-per-wavefront kernels: nv <= 64; nefcmax <= 128 under PGS (64 with elliptic contacts) and a per-env frame within one
 * CU's LDS (160 KB); nefcmax <= 1024 under Newton / CG, with a frame of any size.  Newton / CG models with more than 256 rows of capacity, or
 * whose full frame exceeds the LDS budget, run the row-slot solver, and any of their frames that exceeds the budget lives in HBM
 * (mjb_model_frame_info).  Beyond a cap the call fails with MJB_EUNSUPPORTED.
 *
 * body_gravcomp[nbody] (MuJoCo >= 2.3.1): mj_passive adds, for every body b >= 1 with body_gravcomp[b] != 0, the force
 * -gravity * body_mass[b] * body_gravcomp[b] at xipos[b] to qfrc_passive through the point Jacobian (mj_applyFT without torque) -- unless
 * mjDSBL_PASSIVE or mjDSBL_GRAVITY is set or gravity is zero.  Any finite value is taken (above 1 and below 0 too); a non-finite one fails
 * with MJB_EINVAL.  The mass and gravity are the env's (mjb_set_env_mass_params / mjb_set_env_gravity).  A body without a dof above it (welded to
 * the world, mocap) contributes nothing.  Energy, sensors and qfrc_bias do not see the term.  A model with a non-zero entry matches no compiled-in
 * topology of the lane = env kernel: an eligible one is built by hiprtc (mjb_model_lane_env == -2) and runs the one-wavefront form whatever form
 * is asked for; the split step stands down (mjb_model_split_step == -1).
 *
 * Sensors: the generic kernels evaluate every type of the enum above.  The lane = env kernel takes jointpos, jointvel, actuatorpos / -vel / -frc, clock,
 * framepos / framequat, and -- in its one-wavefront form, in a kernel built by hiprtc (mjb_model_lane_env == -2), never a compiled-in topology --
 * framexaxis / -yaxis / -zaxis, framelinvel, frameangvel, framelinacc, frameangacc on a body / xbody / site without a reference frame, and velocimeter,
 * gyro, accelerometer, force, torque on a site.  Any other sensor (a reference frame, touch, rangefinder, magnetometer, subtree and limit sensors)
 * leaves the model to the generic kernels (mjb_model_lane_env == -1). */
mjb_model *mjb_compile(const mjb_model_desc *desc);
void mjb_free_model(mjb_model *m); /* mj_deleteModel, mujoco_env.cpp:747 */

/* Dimension (doubles or ints per env) of a data field for this model; <0 on error. */
int mjb_field_size(const mjb_model *m, int field);
/* 1 if the field is an int field (MJB_DI), 0 if double. */
int mjb_field_is_int(int field);
/* 1 if the field is persistent state (MJB_DS). */
int mjb_field_is_state(int field);
const char *mjb_field_name(int field);
/* Doubles in one per-env LDS frame (all double fields) — layout documented in DESIGN.md. */
int mjb_frame_doubles(const mjb_model *m);
/* Bytes of LDS one env occupies (doubles + ints): fused != 0 -> the compact frame of mjb_step, else the full frame of
 * mjb_forward / mjb_step1 / mjb_step2.  Resident envs per CU = floor(160 KiB / that).
 * fused == 2: the WIDE fused frame of a Newton model with more than 128 rows of capacity (up to 128 rows of efc_J and of every per-row
 * array in LDS instead of 64, two rows per lane: the largest multiple of four >= 96 with which THREE frames share a CU -- 112 on the
 * Shadow-Hand-like model -- else 128 at two per CU; == the default fused frame for every other model).  A batch switches its long fused launches
 * to it when more than a quarter of the previous launch's env-steps had more than 64 rows, and back below 5 % (MJB_WIDE_FRAME=0 / 1
 * pins the choice); mjb_fused_frame(batch) tells which one the last launch ran on. */
int mjb_frame_bytes(const mjb_model *m, int fused);
/* Diagnostic: offset (doubles; ints for int fields; -1 = absent) of data field `field` in the fused / full frame. */
int mjb_frame_offset(const mjb_model *m, int field, int fused);

/* Allocate N env instances on HIP device `device`, all at the reset state (qpos = qpos0).
 * Takes the place of `mj_makeData` (mujoco_env.cpp:872), once per env. */
mjb_batch *mjb_make_batch(const mjb_model *m, int nenv, int device);
void mjb_free_batch(mjb_batch *b); /* mj_deleteData, mujoco_env.cpp:748 */
int mjb_nenv(const mjb_batch *b);

/* Launch geometry: lanes of a wavefront that cooperate on one env (8,16,32,64) and envs per
 * workgroup.  0 selects the engine default for the model.  Results do not depend on it. */
int mjb_set_launch(mjb_batch *b, int lanes_per_env, int envs_per_block);

/* Advance every env by `nsteps` full steps, fused in ONE kernel launch with the state held in LDS
 * between steps.  Takes the place of `nsteps` x `mj_step(model, data)` per env
 * (mujoco_env.cpp:498, :552, :593).  Asynchronous on the batch's stream. */
int mjb_step(mjb_batch *b, int nsteps);

/* Split step for host callbacks.  mjb_step1 runs position + velocity stages (everything `mj_step`
 * does before it invokes `mjcb_control`, incl. passive forces) and leaves the full frame in the
 * HBM workspace; the caller may then read/modify ctrl, qfrc_applied, xfrc_applied, qfrc_passive
 * (mjb_get/mjb_set) — this is where controlCallback / passiveCallback run (mujoco_env.h:242-251) —
 * and mjb_step2 finishes the step (actuation, acceleration, constraint solve, acc sensors,
 * integration).  step1+step2 == one mjb_step(b,1). */
int mjb_step1(mjb_batch *b);
int mjb_step2(mjb_batch *b);
/* The split for a PREFIX of the batch only -- the envs that have host callbacks (MujocoEnv's callback set): envs [0, ncb) are
 * stepped in two halves around the control-callback point, envs [ncb, nenv) take the same step as ONE fused launch.  Every env's
 * arithmetic is independent of the launch that carries it (same Philox key, same kernels): the result equals a whole-batch step.
 * One step = mjb_step1_prefix(ncb) -> copy the callback envs' fields out -> mjb_step_rest(ncb) [asynchronous: it runs while the
 * host callbacks do] -> copy their writes back -> mjb_step2_prefix(ncb) [advances the step counter; issues the rest itself if
 * the caller skipped mjb_step_rest].  Derived fields are readable for envs [0, ncb) only between the two halves.
 * Abandoning a split step: before mjb_step_rest, a new mjb_step1_prefix simply restarts it; after mjb_step_rest the other envs have
 * taken the step already, so only its second half (mjb_step2_prefix / mjb_step21_prefix / mjb_step2_rk_prefix) or a whole-batch
 * mjb_reset / mjb_step may follow -- mjb_step1_prefix returns MJB_EINVAL. */
int mjb_step1_prefix(mjb_batch *b, int ncb);
int mjb_step_rest(mjb_batch *b, int ncb);
int mjb_step2_prefix(mjb_batch *b, int ncb);
/* mjb_step2_prefix(ncb) of the split step in flight and mjb_step1_prefix(ncb) of the NEXT step as one launch for the callback envs
 * (one kernel and one device -> host round trip per step instead of two when steps follow each other: what a caller with control /
 * passive callbacks only needs -- the state it can read afterwards is the finished step's, the derived fields and the pos / vel
 * stage sensordata already the next step's).  Same results as the two calls it replaces: bit for bit when both run the same
 * kernel (every constrained model, and unconstrained ones outside the dense kernels' reach); for a model the two halves run through
 * the register-dense kernels (nv, nbody, nu, njnt <= 16, Euler, no constraint rows -- BASELINE config 2) the chained launch runs the
 * generic kernel instead, whose factor / solve sum in a different order: equal to rounding (tests/test_gpu_fused_consistency.py
 * bounds it at 1e-9 over a burst), not to the last bit. */
int mjb_step21_prefix(mjb_batch *b, int ncb);
/* The second half of an RK4 step (<option integrator="RK4">) cut at the callback points of its four evaluations: MuJoCo's
 * mj_RungeKutta evaluates mj_forwardSkip -- and with it mjcb_passive / mjcb_control -- once per evaluation (the reason the
 * reference has lastStageCallback at all, mujoco_ros/include/mujoco_ros/plugin_utils.h:119-125).  After mjb_step1_prefix and the
 * callbacks of evaluation 0: rk = 0, 1, 2 finish evaluation rk and run the first half of evaluation rk + 1 (its view, at
 * time = t0 + c h, is readable for the callback envs afterwards); rk = 3 finishes the step (advances the step counter).
 * Four calls in a row == mjb_step2_prefix of the same model, bit for bit (tests/test_rk4.py). */
int mjb_step2_rk_prefix(mjb_batch *b, int ncb, int rk);

/* Recompute all derived quantities without integrating (mj_forward: mujoco_env.cpp:329, :621;
 * callbacks.cpp:573) and leave the full frame in the HBM workspace for mjb_get. */
int mjb_forward(mjb_batch *b);

/* Reset envs with mask[i] != 0 (mask == NULL: all) to qpos0 / zero velocity, activation, control,
 * applied forces, warmstart, time (mj_resetData: mujoco_env.cpp:252). */
int mjb_reset(mjb_batch *b, const uint8_t *mask);

/* Copy a field for envs [env_lo, env_hi) between host memory (env-major, field_size per env) and
 * the device.  Derived fields are readable after mjb_forward / mjb_step1 / mjb_step2 (they come
 * from the frame workspace); only state fields and the callback-writable force fields can be set.
 * Synchronous. */
int mjb_get(mjb_batch *b, int field, int env_lo, int env_hi, double *host);
int mjb_set(mjb_batch *b, int field, int env_lo, int env_hi, const double *host);
int mjb_get_int(mjb_batch *b, int field, int env_lo, int env_hi, int *host);
/* The same for several double fields at once: every copy is enqueued asynchronously on the batch's stream and the call
 * synchronises ONCE (mjb_get_many) or not at all (mjb_set_many: ordered before the next launch).  This is what the host
 * runtime moves around a plugin callback round -- the mjData view fields of SURVEY.md 8a row T1 -- instead of one blocking
 * copy per field.  host[k] has the layout mjb_get / mjb_set use for fields[k].  Page-locking the host buffers
 * (mjb_host_register) makes the copies true DMA transfers. */
int mjb_get_many(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, double *const *host);
int mjb_set_many(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, const double *const *host);
/* The same through ONE transfer: a device kernel gathers the fields of envs [env_lo, env_hi) into one block laid out field after
 * field ([env][dim] each, in the order given; zero-sized fields take no room) and a single copy moves it -- what the callback
 * rounds of the host runtime use (a split step moves ~25 fields out and ~8 back; one copy per field costs more than the step).
 * mjb_get_packed synchronises; mjb_set_packed is asynchronous on the batch's stream (host_block must stay untouched until the
 * next synchronising call).  At most 40 fields. */
int mjb_get_packed(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, double *host_block);
int mjb_set_packed(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, const double *host_block);
int mjb_host_register(void *host, unsigned long long bytes);   /* hipHostRegister; 0 on success */
int mjb_host_unregister(void *host);

/* Raw HBM pointer of a state field's env-major array [nenv][field_size] (for RCCL gathers and
 * zero-copy tensor wrappers).  NULL for derived fields. */
void *mjb_device_ptr(mjb_batch *b, int field);

/* Device-side control noise, the reference's Ornstein-Uhlenbeck injector (mujoco_env.cpp:469-481):
 * before every step  noise = rate*noise + scale*N(0,1),  ctrl = noise  with
 * rate = exp(-dt/max(ctrl_noise_rate, mjMINVAL)), scale = ctrl_noise_std*sqrt(1-rate^2).
 * N(0,1) comes from a counter-based Philox-4x32-10 stream keyed (seed, global env id, step,
 * actuator), so a CPU oracle regenerates the identical sequence.  std == 0 disables it.
 * `env_offset` is the global index of this batch's env 0 (multi-GPU sharding). */
int mjb_set_ctrl_noise(mjb_batch *b, double ctrl_noise_std, double ctrl_noise_rate, uint64_t seed,
                       int64_t env_offset);
/* How the LAST fused mjb_step launch obtained the injector's normals (the values are identical in all three): 0 = generated inside the
 * step kernel, 1 = by mjb_noise_kernel ahead of the step kernel on the same stream, 2 = by mjb_noise_kernel on a side stream while
 * the previous launch ran (unconstrained kernels only; budget MJB_NOISE_PREGEN_MB).  Measurement aid, no reference counterpart. */
int mjb_noise_mode(const mjb_batch *b);
/* 1 = the default fused frame, 2 = the wide one (mjb_frame_bytes): what the batch's fused launches currently run on. */
int mjb_fused_frame(const mjb_batch *b);
/* The lane = env form of the unconstrained fused step (csrc/mjb_lane_env.hip): one env per LANE, the state of 64 envs in a
 * wavefront's registers, compiled per model topology (csrc/lane_env_topos.h).  Same step (mj_step, mujoco_env.cpp:498,552,593),
 * results equal to the generic kernels' to rounding (not bit for bit: a batch that mixes fused launches with split steps
 * should pin one form); measured on MI355X it is ahead of the 16-lanes-per-env kernel from 4096 envs (276 vs 227 M env-steps/s) and 12x
 * ahead at 65 536.  mode: -1 = automatic (fused launches over >= MJB_LANE_ENV_MIN_ENVS envs, default 4096 -- the whole batch, or the non-callback envs of a
 * split step, mjb_step_rest -- of a model whose
 * topology is compiled in, with no per-env model overrides / hwsim stage / xfrc_applied -- the last two unless mjb_lane_env_set_hwsim /
 * mjb_lane_env_set_xfrc, below, opt in), 0 = never, 1 = whenever eligible,
 * 2 = whenever eligible, ALSO with per-env gravity and parameter blocks (mjb_set_env_gravity, mjb_set_env_body_mass / _mass_params, mjb_set_env_dof_params /
 * _joint_stiffness / _actuator_params / _joint_params): such a batch stands the kernel down in every other mode; in mode 2 its launches run the kernel's
 * one-wavefront form (mjb_lane_env_last_form() == 0) in a build that reads each env's gravity, joint stiffness / damping / armature, masses, inertias and
 * actuator gain / bias parameters from a per-env table laid out [value][env] (built at the first such launch, its columns re-derived after every later
 * mjb_set_env_* call on these values; sized mjb_model_lane_env_overlay() doubles per env).  Every other condition stays (hwsim stage, xfrc_applied -- which mjb_lane_env_set_xfrc
 * lifts in this mode too --, frame dumps, statistics); a mode-2 batch WITHOUT overrides runs exactly what mode 1 runs.
 * The environment variable MJB_LANE_ENV (same values) sets the default of new batches (read by mjb_make_batch).  While mjb_set_stats is
 * counting, fused launches run the generic kernels whatever the mode (the counters live in those).
 * Actuator activation states (mjData.act; dyntype integrator / filter on joint transmissions: <general dyntype>, <intvelocity>, <cylinder>): such a model
 * is eligible like any other (mjb_model_lane_env() == -2, its kernel built by hiprtc).  act is read from the batch's `act` field at the start of a
 * launch, lives in the lane's registers, advances once per step as the generic kernels advance it (act_dot from the clamped ctrl, the force from the
 * current act, actrange where actlimited, zero after a mj_check* reset, frozen under mjDSBL_ACTUATION) and is written back at the launch's end: launch
 * splits and hand-overs to and from the generic kernels carry it.  Its launches run the one-wavefront form (mjb_lane_env_last_form() == 0) whatever
 * form is asked for, in the plain, mode-2 and xfrc builds; with a device hwsim stage such a batch keeps the generic kernels (there is no build with
 * both).  Measured on config 2's arm with <intvelocity> on its seven joints and one filter actuator (tools/lane_env_act_rate.py,
 * profiles/lane_env_act.txt): 278.9 against the generic kernel's 196.1 M env-steps/s at 4096 envs (1.42 x), 3121 against 197 at 65 536 (15.9 x), 0.92 / 0.84 of plain franka_like's rate in the same one-wavefront form; the lane = env kernel is ahead at 4096 envs, so mode -1 keeps its 4096-env threshold for these models.  No reference counterpart.
 * Frame-axis, velocity- and acceleration-stage sensors (the list at mjb_compile): such a model is eligible like any other (mjb_model_lane_env() == -2) and
 * its launches run the one-wavefront form whatever form is asked for, in the plain, mode-2, hwsim and xfrc builds, with activation states and gravity
 * compensation.  Velocity sensors are evaluated in the root -> leaf sweep; accelerometer, force, torque, framelinacc and frameangacc in a pass behind the
 * qacc solve and ahead of mj_checkAcc's verdict (mj_rnePostConstraint: cacc with qacc, cfrc_int with xfrc_applied as cfrc_ext in the xfrc builds), on the
 * steps that evaluate sensors -- the launch's last one, or every one under mjb_set_sensors_every_step.  One combination keeps the generic kernels: a
 * written xfrc_applied under mjb_lane_env_set_xfrc with a force / torque sensor on a body that has no joint on its path to the world (the kernel's wrench
 * table has no slot for such a body; mjb_lane_env_plan answers -1 for the xfrc builds).  Measured on config 2's arm with a wrist IMU, a wrist force /
 * torque pair, an end-effector framelinvel and a base force sensor (tools/lane_env_sensors_rate.py, profiles/lane_env_sensors.txt): 262 against the
 * generic kernel's 69 M env-steps/s at 4096 envs (3.8 x), 2783 against 93 at 65 536 (30.1 x); 0.87 / 0.74 of the same arm's rate without those sensors,
 * and 0.76 / 0.68 of its own rate when sensors are evaluated at every step.  No reference counterpart.
 * Joint limits under PGS: a hinge / slide tree whose ONLY constraint rows are joint-limit rows is eligible too (mjb_model_lane_env() == -2) -- solver PGS,
 * no contacts, equalities, tendons or dry friction (dof_frictionloss), every limited joint's range wider than twice its margin (at most one row per
 * joint at a time), and nefcmax equal to the number of limited joints (a <size njmax> that lowered the capacity keeps the generic kernels: truncation and
 * MJB_WARN_CNSTRFULL live there); Newton and CG models keep the generic kernels.  Such a model is never a compiled-in topology: its limit set is part of
 * the structure hiprtc builds the kernel for, and its launches run the one-wavefront form (mjb_lane_env_last_form() == 0) whatever form is asked for, in
 * the PLAIN build only -- with activation states, gravity compensation and the sensors above (the acceleration stage sees the constrained qacc).  The
 * constraint stage is mj_step's for one env per lane: the active rows from qpos (a wavefront in which no lane has a row pays the comparisons and nothing
 * else), mj_makeImpedance, AR = J M^-1 J' + R from the L'DL factor of M, the warmstart from qacc_warmstart -- read at the launch's start, carried across
 * its steps, zero after a mj_check* reset, written back at its end: launch splits and hand-overs to and from the generic kernels carry it --, mj_solPGS
 * with each lane's own stopping test, mj_checkAcc on the constrained qacc.  Beside the state and sensordata the launch leaves, of its LAST step,
 * qfrc_constraint, nefc (the env's active rows) and solver_iter, which mjb_get / mjb_get_int serve after such a launch without mjb_set_keep_frame; the
 * efc_* arrays are NOT written.  A batch with per-env gravity or parameter blocks (mode 2), a device hwsim stage or a written xfrc_applied keeps the generic
 * kernels for such a model (no overlay, hwsim or xfrc build has the stage; mjb_lane_env_plan answers -1 for builds 1 - 4), bit-equal to a mode-0 batch.
 * The automatic mode (-1) KEEPS THE GENERIC KERNELS for these models at every batch size: modes 1 and 2 (without overrides) take the kernel, at any batch
 * size.  Measured on config 2's arm with limited="true" on its nine joints under the benchmark's ctrl noise, where 59 % of the env-steps have at least one
 * active row and a step with rows takes 2.2 sweeps on average (tools/lane_env_limits_rate.py, profiles/lane_env_limits.txt; the median of 5): 90.8
 * against the generic kernels' 44.8 M env-steps/s at 4096 envs (2.03 x), 660 against 45.5 at 65 536 (14.5 x); 0.31 / 0.18 of plain franka_like's rate in
 * the same one-wavefront form -- with 64 envs to a wavefront nearly every step finds some lane at a limit, and the PGS loop runs as long as its slowest
 * lane.  The kernel is ahead at 4096 envs; switching the automatic rule is left to a later change.  No reference counterpart.
 * Fixed-tendon actuators and joint equalities under PGS (a gripper: two finger slides coupled by <equality><joint>, one actuator on a <tendon><fixed>
 * over both): taken in addition, under the same rules as the limit models (mjb_model_lane_env() == -2, form 0 of the PLAIN build whatever form is asked
 * for, modes 1 and 2 only, mjb_lane_env_plan -1 for builds 1 - 4, the generic kernels -- bit-equal to mode 0 -- for a batch with per-env overrides,
 * mjb_set_env_equality included, a hwsim stage or a written xfrc_applied).  TAKEN: fixed tendons that carry actuators and nothing else (no tendon is
 * limited; tendon_frictionloss, tendon_stiffness and tendon_damping are 0; no tendon sensor, no tendon equality); actuators with trntype MJB_TRN_TENDON on
 * them, in every gain / bias / dyntype combination the kernel runs for joint actuators, activation states and ctrl / force / act limits included
 * (actuator_length = gear sum_w coef_w qpos_w, actuator_velocity likewise from qvel, qfrc_actuator[dof_w] += gear coef_w force, and their actuatorpos /
 * actuatorvel / actuatorfrc sensors); joint equalities (MJB_EQ_JOINT) on hinge / slide joints in both forms, q1 - q1_0 = poly(q2 - q2_0) on two
 * different joints and q1 - q1_0 = polycoef[0] on one -- an equality with eq_active == 0 has no row and costs nothing.  Constraint rows may be
 * joint-equality rows and joint-limit rows together, equality rows first (MuJoCo's order): PGS, no dof friction loss, range > 2 margin on limited
 * joints, and nefcmax EXACTLY the active joint equalities + the limited joints (a model with equalities and no limits qualifies; one whose capacity
 * leaves room for an inactive equality does not).  An equality row is every env's at every step (unless mjDSBL_EQUALITY / mjDSBL_CONSTRAINT): its
 * J = e_d1 - poly'(x) e_d2 carries a per-env coefficient, its force is not clamped at 0 and its warmstart force is -D jar unconditionally; nefc counts
 * equality rows + active limit rows, qfrc_constraint = J' f reaches the equality dofs.  REFUSED as before (the generic kernels): a tendon with a spring,
 * a damper, a limit or friction; tendonpos / tendonvel sensors; connect, weld and tendon equalities; dof frictionloss; Newton and CG; a model whose packed
 * AR (rows (rows + 1) / 2 doubles per env) does not fit a CU's LDS beside the state -- refused at classification, not at the launch.  Measured on
 * assets/gripper/franka_gripper.xml (config 2's arm, nine limits, the fingers coupled by a joint equality and driven through a fixed tendon; 10 rows) with
 * tools/lane_env_gripper_rate.py, profiles/lane_env_gripper.txt (the benchmark's ctrl noise, K = 200, the median of 5): 38.7 against the generic kernels'
 * 34.4 M env-steps/s at 4096 envs (1.12 x), 285 against 34.9 at 65 536 (8.2 x); 0.13 / 0.08 of plain franka_like's rate in the same one-wavefront form.
 * 87 % of the env-steps have a limit row beside the equality row (mean nefc 3.0, max 7) and the mean solver_iter is 27: the finger equality and the
 * finger limits pull against each other through one small mass, and the PGS loop of a wavefront runs as long as its slowest lane.  The kernel is ahead
 * at both sizes, barely at 4096 envs; the automatic rule is untouched.  No reference counterpart. */
int mjb_set_lane_env(mjb_batch *b, int mode);
/* Opt-in (default off): with on = 1 the device hwsim stage (mjb_hwsim_configure, below) no longer stands the lane = env kernel down.  The batch's
 * eligible launches then run the kernel's one-wavefront form (mjb_lane_env_last_form() == 0, at the LDS budget the batch size gives, whatever form is
 * asked for) in a build that carries the stage: DefaultRobotHWSim::writeSim for one env per lane, at the control-callback point of every step (after
 * the position and velocity stages, before actuation; a second time in the retry after a mj_checkAcc reset), with the controller cadence of
 * mjb_hwsim_set_period, the e-stop rules, and the commands / PID state / cadence stamps read and written where mjb_hwsim_* keeps them -- the generic
 * kernels continue the same batch, results equal to theirs to rounding.  Every other condition of mjb_set_lane_env stays (mode 0 never, the 4096-env
 * threshold of mode -1, a compiled-in or hiprtc-built topology, whole fused launches, no xfrc_applied -- mjb_lane_env_set_xfrc does not lift this one for a batch
 * with a stage -- / frame dump / statistics, Euler).  A batch
 * that has BOTH a hwsim stage and per-env gravity or parameter blocks keeps the generic kernels in every mode (there is no build with both), and so
 * does a configuration in which two entries control one joint.  With the switch off, or without a hwsim stage, every launch runs what it ran without
 * this call.  Measured on config 2's model with a seven-controller set (tools/lane_env_hwsim_rate.py, profiles/lane_env_hwsim.txt): 9.65 x the generic
 * kernel's rate at 65 536 envs (1757 against 182 M env-steps/s), level with it at 4096 envs (189 against 182), and half the rate of the same kernel
 * without a stage.  No reference counterpart. */
int mjb_lane_env_set_hwsim(mjb_batch *b, int on);
/* Opt-in (default off): with on = 1 a written xfrc_applied no longer stands the lane = env kernel down.  The batch's eligible launches then run the
 * kernel's one-wavefront form (mjb_lane_env_last_form() == 0, at the LDS budget the batch size gives, whatever form is asked for) in a build that
 * applies the Cartesian wrenches as mj_xfrcAccumulate does: each moving body's (force, torque) at its xipos, folded into the body's own force in the
 * root -> leaf sweep.  The kernel reads the wrenches from a transposed copy of xfrc_applied, refilled on the launch's stream ahead of the first such
 * launch after any write of the field (mjb_set, mjb_set_many, mjb_set_packed, mjb_reset); they are constant over the K steps of a launch.  An env that
 * mj_check* resets inside a launch runs on without its wrench from there (the retry of that step included) and finds its rows of xfrc_applied zeroed
 * after the launch, as mj_resetData leaves them.  Composes with mode 2 of mjb_set_lane_env (per-env gravity and parameter blocks); a batch that has
 * BOTH a hwsim stage and a written xfrc_applied keeps the generic kernels (there is no build with both).  Every other condition of mjb_set_lane_env
 * stays (mode 0 never, the 4096-env threshold of mode -1, a compiled-in or hiprtc-built topology, whole fused launches, no frame dump / statistics,
 * Euler).  With the switch off, or while xfrc_applied has never been written, every launch runs what it ran without this call.  Measured on config 2's
 * model with a wrench on every body of every env (tools/lane_env_xfrc_rate.py, profiles/lane_env_xfrc.txt): 3.12 x the generic kernel's rate at 4096 envs
 * (276.5 against 88.8 M env-steps/s), 29.2 x at 65 536 (3482 against 119), and 0.92 / 0.93 of the same kernel's rate without a wrench.  No reference
 * counterpart. */
int mjb_lane_env_set_xfrc(mjb_batch *b, int on);
/* The lane = env kernel evaluates the sensor stages (A15) at the LAST step of a fused launch: sensordata is an output of the launch and nothing inside
 * it reads the values (the generic kernels evaluate them at every step into the LDS frame).  on = 1 makes it evaluate -- and store -- them at every
 * step: same results after the launch, and the per-step cost of A15 on that kernel becomes measurable (bench.py: other_configs.2_sensors_every_step). */
int mjb_set_sensors_every_step(mjb_batch *b, int on);
/* The SPLIT step of plain-PGS models (csrc/mjb_smooth_kernel.h + mjb_cstep_kernel in csrc/mjb_step.hip): per step, the smooth stages of mj_step
 * (kinematics .. qacc_smooth) run one env per LANE and hand geom frames, cdof, both L'DL factors,
 * qfrc_smooth and qacc_smooth to the constraint stages (A4 - A7, A13, A16) through a per-env record in HBM; those run one env per wavefront.  The
 * batch is cut into slices (MJB_SPLIT_SLICES, default 2) that alternate the two kernels on streams of their own.  Same step (mj_step, mujoco_env.cpp:498,552,593), results equal
 * to the fused kernel's to rounding.  Eligible: a model whose topology is compiled in (csrc/smooth_topos.h: free / ball / hinge / slide joints, one
 * per body), PGS with pyramidal or frictionless contacts, nv <= 16, Euler, no tendons / equalities / mocap bodies / activations, position- and
 * velocity-stage sensors of the lane = env list only, no per-env gravity / mass overrides, no hwsim stage, no xfrc_applied, no frame dump.
 * mode: 1 = whenever eligible, 0 = never, -1 (default) = only when the environment variable MJB_SPLIT_MIN_ENVS names a batch size (whole-batch
 * fused launches of at least that many envs).  A launch pair per step ends with its slice's slowest env, which only averages out over many envs per
 * slice: measured on config 3 (profiles/r06_split_step.txt) 33.2 M env-steps/s against the fused kernel's 27.5 M at 32 768 envs in the rollout's
 * light-contact phase, 26.2 against 23.3 M over steps 1000 - 4000, 23.4 against 24.6 M over steps 500 - 2000, 18.7 against 23.3 M at 4096 envs.
 * sensordata is that of the launch's LAST step (as in the lane = env kernel).  No reference counterpart. */
int mjb_set_split_step(mjb_batch *b, int mode);
/* >= 0: index of the compiled-in topology of the split step the batch's model matches, -1: none.  *used_last (may be NULL) = 1 when the last fused
 * launch ran as a split step, *slices (may be NULL) = the env slices it was cut into. */
int mjb_split_step_info(const mjb_batch *b, int *used_last, int *slices);
int mjb_model_split_step(const mjb_model *m);
/* 1: the model runs the row-slot Newton / CG solver (more than 256 rows of capacity, or a full frame beyond one CU's LDS), 0: it does not.
 * *full_hbm / *fused_hbm (may be NULL) = 1 when the full frame (mjb_forward, mjb_step1 / mjb_step2, frame dumps) / the fused frame of
 * mjb_step lives in the env's slot of an HBM workspace instead of LDS.  No reference counterpart. */
int mjb_model_frame_info(const mjb_model *m, int *full_hbm, int *fused_hbm);
/* >= 0: index of the compiled-in topology the batch's model matches; -2: none compiled in, but the model's structure fits the kernel -- its
 * first eligible launch builds the kernel for it through hiprtc (libhiprtc.so and csrc/mjb_lane_env_kernel.h next to libmjb.so; a few
 * seconds, cached per process); -3: that build was not possible (mjb_lane_env_error says why) and the generic kernels run; -1: the model does not
 * fit (constraint rows other than PGS joint equalities and joint limits alone, free / ball joints, RK4, a sensor outside the list at mjb_compile, ...).  *used_last (may be NULL) = 1 when the last fused launch ran the lane = env kernel. */
int mjb_lane_env_info(const mjb_batch *b, int *used_last);
/* hiprtc builds of the lane = env kernel are kept on disk: $MJB_JIT_CACHE (default $XDG_CACHE_HOME/mjb_jit or ~/.cache/mjb_jit; "0" = off), one code
 * object per (gfx arch, kernel-header fingerprint, LDS budget, form, topology).  Counts of this process: kernels compiled / taken from the cache. */
void mjb_lane_env_jit_counts(int *compiled, int *disk_hits);
/* The same classification for a compiled model, without a batch or a device (>= 0 / -2 / -1 as above). */
int mjb_model_lane_env(const mjb_model *m);
/* INTROSPECTION (debug / test aid; no caller needs them to run a batch): the constants of a lane = env eligible model (mjb_model_lane_env != -1) as
 * the kernel reads them, without a batch or a device.  Both return the
 * number of doubles and fill `out` when it is not NULL and `cap` is large enough; -1: the model is not eligible.
 * mjb_model_lane_env_tape: the constant tape -- dt gravity[3] pad[4] | per body, 32 doubles: pos[3] quat[4] jaxis[3] jpos[3] qpos0 stiffness spring
 * ipos[3] ibody[6] mass damping armature hdamping gravcomp pad[2] | per actuator, 16: gear ctrlrange[2] gain[3] bias[3] forcerange[2] dyntau actrange[2] pad[2]; ibody =
 * R(iquat) diag(inertia) R(iquat)' as xx yy zz xy xz yz, hdamping = timestep * damping, dyntau = max(mjMINVAL, dynprm[0]) of a filter actuator -- the
 * time constant itself, which act_dot divides by, not its reciprocal -- and 0 for every other; dyntau and actrange are 0 for a stateless actuator.
 * A model with joint-limit rows has, BEHIND those records (their offsets stay), 8 doubles: meaninertia tolerance iterations 1/(meaninertia max(1, nv))
 * mjDSBL_WARMSTART mjDSBL_REFSAFE pad[2] | per limited joint, in joint order, 16: range[2] margin solref[2] solimp[5] dof_invweight0 K B powa powb pad --
 * solref / solimp as getsolparam leaves them (a mixed-sign solref replaced by the default, refsafe, solimp clamped to its legal ranges), K / B the row's
 * stiffness and damping from them (mj_makeImpedance), powa / powb = 1 / mid^(power - 1) and 1 / (1 - mid)^(power - 1) of the impedance curve.
 * The 8-double header is there whenever the model has rows of either kind; BEHIND the limit records, per ACTIVE joint equality, in equality order, 24:
 * polycoef[5] qpos0[2] (of joint1, joint2; the second 0 in the one-joint form) solref[2] solimp[5] (as getsolparam leaves them)
 * dof_invweight0[d1] + dof_invweight0[d2] K B powa powb pad[5]; BEHIND those, per tendon wrap of a model with fixed tendons, in wrap order, 8: the PLAIN
 * coefficient (wrap_prm) pad[7] -- the actuator's gear, in its own record, multiplies it in the kernel.  A model without equalities and tendons has
 * none of these records.
 * mjb_model_lane_env_overlay: one env's column of the per-env table of mjb_set_lane_env's mode 2, here with the model's own values -- gravity[3] | per
 * jointed body: stiffness damping armature hdamping | per moving body (a joint on its path to the world): mass ibody[6] | per actuator: gain[3] bias[3]
 * | the mass of every other body but the world (mjENBL_ENERGY reads it). */
int mjb_model_lane_env_tape(const mjb_model *m, double *out, int cap);
int mjb_model_lane_env_overlay(const mjb_model *m, double *out, int cap);
/* mjb_lane_env_plan: the variant of the kernel the launcher picks ("The lane = env launcher"), as a pure function of its arguments -- the
 * process's environment variables and the settings of mjb_lane_env_set_form / mjb_lane_env_set_sweep_waves are NOT looked at, no device is touched.
 * m: the model (its layouts are counted when hiprtc builds its kernel), or NULL for "a compiled-in topology": no fit limit.  ncu: CUs of the device;
 * nenv: envs of the batch; build: 0 plain, 1 per-env overlay (mjb_set_lane_env mode 2), 2 hwsim stage, 3 xfrc_applied, 4 overlay + xfrc_applied;
 * form: -1 the rule, 0 .. 3 as mjb_lane_env_set_form; sweep_waves: 0 the rule, 3 / 4 as mjb_lane_env_set_sweep_waves; lds_kb: 0 by batch size,
 * 40 / 80 / 160 as MJB_LANE_ENV_LDS_KB.  Fills (each may be NULL) the form, form 3's sweep wavefronts (0 otherwise) and the LDS budget in KB, the
 * values mjb_lane_env_last_form / mjb_lane_env_last_sweep_waves report after such a launch.  A model with activation states (na > 0): form 0 whatever
 * is asked for, and no variant at all for build 2.  A model with a frame-axis, velocity- or acceleration-stage sensor: form 0 whatever is asked for,
 * and no variant for builds 3 and 4 when a force / torque sensor sits on a body without a joint on its path to the world.  A model with constraint
 * rows (joint equalities, joint limits) or fixed tendons: form 0 whatever is asked for, at the smallest budget its packed AR fits beside the state, and no variant for builds 1 - 4.  Returns 0; -1: the model is not eligible or needs more LDS than a CU has, there is no such variant,
 * or an argument is out of range. */
int mjb_lane_env_plan(const mjb_model *m, int ncu, int nenv, int build, int form, int sweep_waves, int lds_kb, int *out_form, int *out_sweep_waves, int *out_lds_kb);
/* The static row list of the lane = env kernel's constraint stage for this model: the joint-equality rows (its active joint equalities, first in the
 * list) and the joint-limit rows (its limited joints, behind them), each may be NULL.  Returns their sum; 0 for a model without a constraint stage
 * (not eligible, unconstrained, or its rows switched off by mjDSBL_EQUALITY / mjDSBL_LIMIT). */
int mjb_lane_env_rows(const mjb_model *m, int *neq_rows, int *nlimit_rows);
const char *mjb_lane_env_error(void);
/* The lane = env kernel's FORM, process-wide: how many wavefronts share the 64 envs of a block.  0 = one (the whole step in one instruction stream);
 * 1 = two, the step's position half (poses, cinert, composite inertias, qM, factors, solves, Euler) and velocity half (velocities, forces,
 * qfrc_smooth) side by side on two SIMDs of a CU, both computing the poses; 2 = two, PIPELINED: one wavefront computes every pose once and
 * hands it on body by body through LDS (a workgroup barrier per body), the other follows one body behind with cinert, cdof, velocities and
 * forces and hands cdof / cinert / qfrc_smooth back -- nothing is computed twice.  A lone wavefront on a SIMD issues one instruction every ~4
 * cycles whatever it is, so while the batch leaves SIMDs idle the step's length is the longest instruction stream; 3 = THREE: the first wavefront runs
 * the pose chain and nothing else, the second follows it with cinert and cdof and then takes the composite inertias, qM, the factors, the solves and
 * Euler, the third the velocities and forces.  Form 3 runs whenever a block has a CU's LDS to itself (<= 64 x CUs envs: 16 384 on MI355X; form 2 is
 * the same with two wavefronts, by request only), form 1 up to twice that, form 0 beyond.  -1 = that rule (default; the environment
 * variable MJB_LANE_ENV_DUO = 0 / 1 / 2 / 3 overrides it).  A forced form that does not fit (LDS) falls back to the next lower one.  Results of the
 * four forms agree to rounding.  Returns the previous setting.  mjb_lane_env_last_form: the form of this process's last lane = env launch (-1: none yet).
 * Measurement / test knob, no reference counterpart. */
int mjb_lane_env_set_form(int form);
int mjb_lane_env_last_form(void);
/* Form 3's root -> leaf sweep runs on three wavefronts (poses | inertias | velocities) or on FOUR (orientations | frames and positions | inertias |
 * velocities: the pose wavefront's chain cut in two, on the fourth SIMD of the block's CU; csrc/mjb_lane_env_kernel.h, roles 8 - 11).
 * mjb_lane_env_set_sweep_waves(3 | 4) asks for one of them, 0 = the launcher's rule (default; the environment variable MJB_LANE_ENV_SWEEP_WAVES = 3 / 4
 * overrides it): four whenever its two extra LDS rings fit the block's 160 KB, three otherwise -- a request for four falls back the same way.  Returns
 * the previous setting.  mjb_lane_env_last_sweep_waves: 3 or 4 for this process's last lane = env launch when it ran form 3, 0 otherwise.  Both
 * variants ARE form 3 (mjb_lane_env_last_form); their results agree to rounding.  Measurement / test knob, no reference counterpart. */
int mjb_lane_env_set_sweep_waves(int waves);
int mjb_lane_env_last_sweep_waves(void);

/* Stream control: the hipStream_t (as void*) kernels are launched on; default is a stream the
 * batch owns.  mjb_synchronize waits for it. */
void *mjb_get_stream(mjb_batch *b);
int mjb_set_stream(mjb_batch *b, void *hip_stream);
int mjb_synchronize(mjb_batch *b);

/* Number of env auto-resets so far (MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc warnings: a state
 * that went NaN or beyond mjMAXVAL is reset to qpos0 exactly as mj_step does). */
int mjb_warning_count(mjb_batch *b, unsigned long long *count);
/* mjData.warning[which].number summed over the batch's envs (which = MJB_WARN_*):
 *   BADQPOS / BADQVEL / BADQACC  mj_checkPos / mj_checkVel / mj_checkAcc found NaN or |x| > mjMAXVAL and reset the env
 *                                (mjb_warning_count is their sum);
 *   CONTACTFULL                  an env produced more contacts than nconmax in one step: the contacts past the capacity,
 *                                in pair order, were dropped (mj_addContact's rule);
 *   CNSTRFULL                    an env's constraint rows exceeded nefcmax in one step: the first item (equality, friction
 *                                row, limit, contact -- MuJoCo's row order) that did not fit and every item after it were
 *                                dropped.  (MuJoCo 2.3.7 sizes its rows from the arena and drops ALL rows when that fails;
 *                                with a fixed per-env capacity the engine keeps the prefix that fits -- the oracle applies the
 *                                same rule.)
 * The other entries stay 0. */
int mjb_warning(mjb_batch *b, int which, unsigned long long *count);

/* Workload statistics of the constrained kernels, accumulated on the device by every forward evaluation that reaches the constraint
 * solver (one per env-step under Euler): what the workload actually asks of the solver.  Off by default; mjb_set_stats(b, 1) allocates
 * and ZEROES the counters, mjb_set_stats(b, 0) stops counting.  Layout of out[MJB_NSTATS] (mjb_get_stats):
 *   [0] evaluations counted   [1] sum of mjData.solver_iter (PGS sweeps / Newton / CG iterations)
 *   [2 + r], r = 0..256       histogram of nefc (rows of the evaluation; the last bin collects r >= 256)
 *   [259 + c], c = 0..128     histogram of ncon
 * Measurement aid (bench.py's ncon / nefc fields); MuJoCo's counterpart is reading d->ncon, d->nefc, d->solver_iter after mj_step. */
enum { MJB_NSTATS = 2 + 257 + 129 };
int mjb_set_stats(mjb_batch *b, int on);
int mjb_get_stats(mjb_batch *b, unsigned long long *out);

/* Aggregate metrics of the batch (the <= 16-double vector the RCCL all-reduce carries), computed on the
 * device from the state arrays on the batch's stream:
 *   out[0..7]  additive:  env-steps taken, auto-resets (BADQPOS + BADQVEL + BADQACC), CONTACTFULL, CNSTRFULL,
 *                         sum of potential energy, sum of kinetic energy (both 0 unless mjENBL_ENERGY), nenv, 0
 *   out[8..15] maxima:    max |qacc|, max |qvel|, max time, 0 ...
 * so that a job-wide vector is one SUM all-reduce of the first half and one MAX all-reduce of the second.
 * mjb_metrics copies the vector to the host (synchronous); mjb_metrics_device enqueues the reduction and returns the
 * device pointer of the 16 doubles (valid until the next call; ordered on the batch's stream). */
int mjb_metrics(mjb_batch *b, double *out16);
void *mjb_metrics_device(mjb_batch *b);

/* mjData after mj_step holds the derived quantities of the last forward pass (xpos, contacts, efc_*, ...), which
 * the reference's lastStageCallback / renderCallback read (mujoco_env.cpp:506-515, 430-436).  Fused mjb_step
 * keeps them in LDS only; with keep_frame on, every launch also stores the full frame of its LAST step so that
 * mjb_get / mjb_get_int serve derived fields afterwards (costs the compact LDS layout and one frame store per
 * launch).  Off by default. */
int mjb_set_keep_frame(mjb_batch *b, int on);

/* ---- sensors-plugin equivalent ----
 * What MujocoRosSensorsPlugin::lastStageCallback publishes from sensordata after a step
 * (/root/reference mujoco_ros_sensors/src/mujoco_sensor_handler_plugin.cpp:175-437), for every env at once, on the
 * device, as float32 in sensordata layout ([nenv][nsensordata], quaternions stay (w, x, y, z)):
 *   which = 1 "ground truth" = sensordata / cutoff           (the plugin's gt publisher)
 *   which = 0 "value"        = the same when the sensor has no noise model, else sensordata + noise / cutoff
 *                              (scalars / vectors; per-axis N(mean, sigma)) or setRPY(noise) * q (quaternions).
 * mjb_sensor_set_noise is registerNoiseModelsCB (:123-173): bit k of set_flag enables noise on component k, the
 * n-th set bit reads mean3[n] / sigma3[n], flags accumulate; set_flag = 0 clears the sensor's model (extension).
 * The plugin's std::mt19937 is replaced by the engine's counter-based Philox stream keyed
 * (seed, global env, steps taken so far, component), so values are reproducible and identical on CPU and GPU. */
int mjb_sensor_set_noise(mjb_batch *b, int sensor, int set_flag, const double *mean3, const double *sigma3);
int mjb_sensor_pack(mjb_batch *b, uint64_t seed);
int mjb_sensor_get(mjb_batch *b, int which, int env_lo, int env_hi, float *host);
void *mjb_sensor_device_ptr(mjb_batch *b, int which);

/* ---- batched ray casting: mj_ray for many rays of every env at once ----
 * A lidar ring or a small depth image per env, cast on the device against the geom poses of the frame workspace (plane, sphere, capsule
 * and box: the rangefinder sensor's intersection, bit for bit).  Ray r hangs on site[r]: it starts at site_xpos + site_xmat pnt[r] and runs
 * along site_xmat vec[r]; site -1 gives pnt and vec in the world frame.  vec is not normalised (mj_ray): a result is in units of |vec|.
 * The result of a ray is the smallest x >= 0 over the geoms it may hit and that geom's id, -1 and -1 for a miss; the lower geom id keeps a
 * tie.  A geom is skipped when its geom_mask entry is 0 (NULL mask: when its geom_rgba alpha is 0, the rangefinder's rule), or when the ray
 * excludes its own body and the geom belongs to the site's body.  Per-env geom sizes and types (mjb_set_env_geom_size / _type) are honoured.
 * mjb_rays_configure validates (MJB_EINVAL: nray < 1, a site outside [-1, nsite), a non-finite entry, a zero vec, a model without geoms),
 * uploads the tables and (re)allocates the results; a second call replaces the first.  mjb_rays_cast reads derived fields, so like mjb_get
 * it is MJB_EINVAL unless the frame workspace is current for every env (after mjb_forward / mjb_step1 / mjb_step2, or a fused step with
 * keep_frame); it runs on the batch's stream behind the launch that produced the frame.  No reference counterpart (its depth images are
 * OpenGL renderings). */
int mjb_rays_configure(mjb_batch *b, int nray, const int *site /*[nray], -1 = world frame*/,
                       const double *pnt /*[nray][3], NULL = the frame's origin*/, const double *vec /*[nray][3]*/,
                       const unsigned char *exclude_own_body /*[nray], NULL = all 1; ignored for site -1*/,
                       const unsigned char *geom_mask /*[ngeom], NULL = visible geoms*/);
int mjb_rays_cast(mjb_batch *b);                       /* asynchronous on the batch's stream */
int mjb_rays_get(mjb_batch *b, int env_lo, int env_hi, double *dist, int *geomid);  /* synchronises; either pointer may be NULL */
void *mjb_rays_device_ptr(mjb_batch *b, int which);    /* 0: dist [nenv][nray] double, 1: geomid [nenv][nray] int */
int mjb_rays_count(const mjb_batch *b);

/* ---- batched Jacobians: mj_jacSite / mj_jacBody / mj_jacBodyCom / mj_jacGeom and mj_solveM for every env at once ----
 * Point k is fixed to the body of its object and sits at the object's world position plus its world rotation times pnt[k]: a site
 * (site_xpos, site_xmat, site_bodyid), a body (xpos, xmat), a body's inertial frame (xipos, ximat) or a geom (geom_xpos, geom_xmat,
 * geom_bodyid), all read from the frame workspace.  A point on the world body is legal; every output of it is zero.
 * Results are fp64, env-major and world-oriented, translational rows first (MuJoCo's jacp, then jacr):
 *   MJB_JAC_OUT_J       [nenv][npoint][6][nv]  column d = (cdof_ang x (p - subtree_com[root]) + cdof_lin, cdof_ang) when dof d moves the body,
 *                                              exactly 0.0 otherwise -- the arithmetic of the site transmission's moment arms
 *   MJB_JAC_OUT_MINVJT  [nenv][npoint][6][nv]  row r = M^-1 J[r]', mj_solveM on the frame's L'DL factor of qM (qLD / qLDiagInv as mjb_get
 *                                              serves them: the factor of M, never of the M + h B of implicit joint damping)
 *   MJB_JAC_OUT_AINV    [nenv][npoint][6][6]   J M^-1 J' of the point, the inverse operational-space inertia; summed in a fixed order over
 *                                              the half-solved rows, so it equals its transpose to the bit.  No blocks between two points.
 *   MJB_JAC_OUT_VEL     [nenv][npoint][6]      J qvel, LINEAR then angular -- mj_objectVelocity orders its result the other way round
 *                                              (angular first), and can rotate it into the object's frame; this one stays in world axes.
 * No result depends on the shape of the launch.
 * mjb_jac_configure validates (MJB_EINVAL: npoint < 1, an unknown object type, an id out of range, a non-finite pnt, outputs 0 or with
 * unknown bits, a model with nv == 0), uploads the point table and (re)allocates the requested outputs only; a second call replaces the
 * first.  mjb_jac_eval reads derived fields, so like mjb_get it is MJB_EINVAL unless the frame workspace is current for every env (after
 * mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame); it runs on the batch's stream behind the launch that produced
 * the frame.  It is MJB_EINVAL, too, once qpos or a mocap pose has been written through mjb_set / mjb_set_many / mjb_set_packed and no such call
 * has followed: mjb_get goes on serving the old frame (mjData's rule), but a Jacobian is applied to the state as it is now.  Only
 * writes through those three calls are seen: a caller that writes qpos through mjb_device_ptr calls mjb_forward itself before it evaluates.  VEL multiplies J with
 * the batch's qvel as it is when the evaluation runs.  After a step the frame holds the step's forward pass, that is the poses BEFORE the integration, as mjData does after
 * mj_step: J then belongs to site_xpos of that same frame, not to the new qpos.  mjb_jac_get / mjb_jac_device_ptr of an output that was not
 * configured: MJB_EINVAL / NULL. */
enum { MJB_JAC_SITE = 0, MJB_JAC_BODY = 1, MJB_JAC_BODYCOM = 2, MJB_JAC_GEOM = 3 };   /* mj_jacSite / mj_jacBody / mj_jacBodyCom / mj_jacGeom */
enum { MJB_JAC_OUT_J = 1, MJB_JAC_OUT_MINVJT = 2, MJB_JAC_OUT_AINV = 4, MJB_JAC_OUT_VEL = 8 };
int mjb_jac_configure(mjb_batch *b, int npoint, const int *objtype /*[npoint] MJB_JAC_SITE ...*/,const int *objid /*[npoint]*/,
                      const double *pnt /*[npoint][3] offset in the object's own frame, NULL = 0*/, int outputs /*MJB_JAC_OUT_* bits*/);
int mjb_jac_eval(mjb_batch *b);                                   /* asynchronous on the batch's stream */
int mjb_jac_get(mjb_batch *b, int which, int env_lo, int env_hi, double *host);   /* synchronises; which = one MJB_JAC_OUT_* bit */
void *mjb_jac_device_ptr(mjb_batch *b, int which);                /* which = one MJB_JAC_OUT_* bit */
int mjb_jac_count(const mjb_batch *b);                            /* points per env of the configuration, 0: none yet */

/* ---- batched joint-space dynamics: mj_fullM, mj_mulM, mj_solveM, inverse dynamics and Jdot qvel for every env at once ----
 * The other half of a model-based control law next to mjb_jac_*: everything is read from the frame workspace, V is a block of nvec vectors per
 * env that the batch owns ([nenv][nvec][nv], zero at configure; written through mjb_dyn_device_ptr(b, MJB_DYN_IN_V) on the batch's stream, or
 * from the host with mjb_dyn_set_vectors, which synchronises).  Results are fp64 and env-major; only the outputs asked for are allocated and computed:
 *   MJB_DYN_OUT_M      [nenv][nv][nv]      mj_fullM of the frame's qM: entry (i, j) is the qM element of the pair when one dof is the other's
 *                                          ancestor-or-self along dof_parentid, a literal +0.0 otherwise; symmetric to the bit
 *   MJB_DYN_OUT_MV     [nenv][nvec][nv]    M V[k] (mj_mulM): each row summed in ascending j with fused multiply-adds, structural zeros skipped
 *   MJB_DYN_OUT_MINVV  [nenv][nvec][nv]    M^-1 V[k] (mj_solveM) on the frame's L'DL factor of qM (qLD / qLDiagInv as mjb_get serves them: the
 *                                          factor of M, never of the M + h B of implicit joint damping)
 *   MJB_DYN_OUT_ID     [nenv][nvec][nv]    (M V[k] + qfrc_bias) - qfrc_passive, rounded in that order: the generalized force -- actuators + applied +
 *                                          constraints together -- under which qacc = V[k].  mj_inverse's qfrc_inverse leaves the constraint forces
 *                                          out: a caller who wants it subtracts the frame's qfrc_constraint (mjb_get) themselves.
 *   MJB_DYN_OUT_JDOTV  [nenv][npoint][6]   Jdot qvel of each configured point, LINEAR then angular, world axes: the bias acceleration of
 *                                          xddot = J qacc + Jdot qvel.  The points are mjb_jac_configure's (object types, ids, pnt, the same rules).
 *                                          With c = subtree_com[body_rootid[body]], r = p - c, (w, v) = cvel[body] and A = the sum of
 *                                          cdof_dot[d] qvel[d] over the dofs that move the body in ascending d: linear = A_lin + A_ang x r +
 *                                          w x (v + w x r), angular = A_ang.  A point on the world body gives +0.0.  For ball and free joints only
 *                                          the sum A is the physical derivative, the single cdof_dot columns are not: no Jdot matrix is offered.
 *                                          A <framelinacc> sensor on the same site reads J qacc + JDOTV - gravity, a <frameangacc> J qacc + JDOTV.
 * No result depends on the shape of the launch, on nvec, npoint or the set of outputs.
 * mjb_dyn_configure validates (MJB_EINVAL: outputs 0, with unknown bits or with MJB_DYN_IN_V; nvec < 1 with MV, MINVV or ID, nvec < 0; npoint < 1
 * or null arrays with JDOTV; a bad point by mjb_jac_configure's rules; a model with nv == 0), builds the dense index table of qM, and (re)allocates
 * V and the requested outputs only; a second call replaces the first and zeroes V.  nvec without MV / MINVV / ID and the points without JDOTV are ignored.
 * mjb_dyn_eval is MJB_EINVAL before mjb_dyn_configure and, like mjb_jac_eval, unless the frame workspace is current for every env (after mjb_forward /
 * mjb_step1 / mjb_step2, or a fused step with keep_frame) and once qpos or a mocap pose has been written through mjb_set / mjb_set_many /
 * mjb_set_packed since.  ID and JDOTV read the velocity stage (qfrc_bias, qfrc_passive, cvel, cdof_dot): with either configured the call refuses,
 * too, once qvel has been written through those three calls since the workspace was made current; M, MV and MINVV do not care about qvel.  Writes
 * through mjb_device_ptr are not seen: such a caller runs mjb_forward itself.  After a step (mjb_step2, a fused step with keep_frame) the frame holds
 * the step's forward pass, the poses and velocities BEFORE the integration, as mjData does after mj_step: M, ID and JDOTV belong to that state.
 * JDOTV then takes the step's update qvel += timestep * (the Euler stage's solution, kept in the frame) back to multiply cdof_dot with the
 * velocities it was computed from; behind an RK4 step those are not recoverable and JDOTV is MJB_EINVAL until mjb_forward / mjb_step1.
 * mjb_dyn_get / mjb_dyn_device_ptr of an output that was not configured: MJB_EINVAL / NULL. */
enum { MJB_DYN_OUT_M = 1, MJB_DYN_OUT_MV = 2, MJB_DYN_OUT_MINVV = 4, MJB_DYN_OUT_ID = 8, MJB_DYN_OUT_JDOTV = 16, MJB_DYN_IN_V = 256 };
int mjb_dyn_configure(mjb_batch *b, int nvec, int npoint, const int *objtype /*[npoint] MJB_JAC_SITE ...*/, const int *objid /*[npoint]*/,
                      const double *pnt /*[npoint][3] offset in the object's own frame, NULL = 0*/, int outputs /*MJB_DYN_OUT_* bits*/);
int mjb_dyn_set_vectors(mjb_batch *b, int env_lo, int env_hi, const double *host /*[envs][nvec][nv]*/);   /* synchronises */
int mjb_dyn_eval(mjb_batch *b);                                   /* asynchronous on the batch's stream */
int mjb_dyn_get(mjb_batch *b, int which, int env_lo, int env_hi, double *host);   /* synchronises; which = one MJB_DYN_OUT_* bit */
void *mjb_dyn_device_ptr(mjb_batch *b, int which);                /* which = one MJB_DYN_OUT_* bit, or MJB_DYN_IN_V */
int mjb_dyn_count(const mjb_batch *b, int *nvec, int *npoint);    /* vectors and points per env of the configuration (either pointer may be NULL) */

/* ---- batched contact wrenches: mj_contactForce and net contact forces between geom sets, for every env at once ----
 * Contact c of an env is read from the frame workspace (ncon, contact_geom, contact_dim, contact_efc_address, contact_frame, contact_pos,
 * contact_dist, contact_friction, efc_force).  A contact with contact_efc_address[c] < 0 has no rows and takes no part in any output.
 *   lf[6]  its local wrench, mj_contactForce: dim 1: lf[0] = efc_force[adr];  elliptic cone: lf[k] = efc_force[adr + k], k < dim;  pyramidal cone:
 *          lf[0] = sum of the 2 (dim - 1) edge forces, lf[1 + k] = (efc_force[adr + 2 k] - efc_force[adr + 2 k + 1]) contact_friction[c][k] -- the
 *          frame's contact_friction, so per-env geom friction (mjb_set_env_geom_friction) is honoured.  The other entries are 0.
 *   F, T   its world force F = contact_frame' lf[0:3] and world torque at contact_pos T = contact_frame' lf[3:6].  (F, T) acts with + on the body
 *          of contact_geom[c][1] and with - on the body of contact_geom[c][0] (mj_rnePostConstraint's sign).
 * Query q is two geom sets A and B, byte masks over the model's geoms (non-zero = member).  Contact (g1, g2) = contact_geom[c] matches q with sign
 * +1 when g2 is in A and g1 in B, with sign -1 when g1 is in A and g2 in B; A and B are disjoint, so no contact matches both ways.
 * Results are env-major; only the requested outputs are allocated and computed:
 *   MJB_CON_OUT_WRENCH    [nenv][nquery][6]  double  net force (3), then torque (3), in world axes, that the B side exerts on the A side.  The torque
 *                                                    is taken about r_q = xpos[ref_body[q]] of the same frame (the world origin for ref_body -1): each
 *                                                    matching contact adds sign (F, T + (contact_pos - r_q) x F), summed in ascending c
 *   MJB_CON_OUT_NORMAL    [nenv][nquery]     double  sum of lf[0] over the matching contacts in ascending c: what a touch sensor reports for a zone that
 *                                                    holds them all
 *   MJB_CON_OUT_COUNT     [nenv][nquery]     int32   number of matching contacts
 *   MJB_CON_OUT_DIST      [nenv][nquery]     double  smallest contact_dist of the matching contacts, +inf when there is none
 *   MJB_CON_OUT_CONTACTS  [nenv][nconmax][6] double  lf of every contact c < ncon in the contact's own frame, normal first; exactly 0.0 for
 *                                                    c >= ncon and for contacts without rows
 * No result depends on the shape of the launch: every value is computed by one lane, in a fixed order, from operands that do not depend on the
 * batch's size or on the number of queries.  An env without a matching contact has WRENCH and NORMAL exactly 0.0, COUNT 0 and DIST +inf.  Swapping A
 * and B under the same ref_body negates WRENCH to the bit (the same terms in the same order with the opposite sign).
 * Capacity: contacts dropped when an env's contact list is full (the CONTACTFULL warning) are not in the frame and therefore not in the sums.
 * mjb_contact_configure validates (MJB_EINVAL: nquery < 1, a model with nconmax == 0 or ngeom == 0, an empty A or B, A and B with a common geom,
 * a ref_body outside [-1, nbody), outputs 0 or with unknown bits), synchronises the stream, uploads the masks and (re)allocates the requested
 * outputs only; a second call replaces the first.  mjb_contact_eval reads derived fields, so like mjb_get it is MJB_EINVAL unless the frame
 * workspace is current for every env; it is MJB_EINVAL, too, when the frame was last written by mjb_step1 / mjb_step1_prefix and no mjb_step2* has
 * followed: the frame's contacts are then this state's, but efc_force is not.  It is legal after mjb_forward, mjb_step2 and a fused step with
 * keep_frame; not after mjb_reset / mjb_episode_* until the next forward pass or step.  It runs on the batch's stream behind the launch that
 * produced the frame.  After a step the frame holds the step's forward pass: the contacts and forces BEFORE the integration, as mjData after mj_step.
 * mjb_contact_get / mjb_contact_device_ptr of an output that was not configured: MJB_EINVAL / NULL. */
enum { MJB_CON_OUT_WRENCH = 1, MJB_CON_OUT_NORMAL = 2, MJB_CON_OUT_COUNT = 4, MJB_CON_OUT_DIST = 8, MJB_CON_OUT_CONTACTS = 16 };
int mjb_contact_configure(mjb_batch *b, int nquery, const unsigned char *geom_a /*[nquery][ngeom]*/, const unsigned char *geom_b /*[nquery][ngeom]*/,
                          const int *ref_body /*[nquery], -1 = world origin; NULL = all -1*/, int outputs /*MJB_CON_OUT_* bits*/);
int mjb_contact_eval(mjb_batch *b);                               /* asynchronous on the batch's stream */
int mjb_contact_get(mjb_batch *b, int which, int env_lo, int env_hi, void *host);   /* synchronises; which = one MJB_CON_OUT_* bit (COUNT: int32, the others double) */
void *mjb_contact_device_ptr(mjb_batch *b, int which);            /* which = one MJB_CON_OUT_* bit */
int mjb_contact_count(const mjb_batch *b);                        /* queries of the configuration, 0: none yet */

/* ---- device-side episode resets (MujocoEnv::resetSim: mj_resetData, then loadInitialJointStates, /root/reference mujoco_ros/src/mujoco_env.cpp:246-264) ----
 * mjb_reset takes a host mask and can only put an env back to qpos0.  These calls end and restart episodes without leaving the device: ONE launch
 * on the batch's stream decides for every env whether its episode is over, writes done[nenv] (uint8, 1 / 0) and ndone (one uint32, their sum), and
 * resets the done envs -- each to a row of an initial-state bank of its own drawing, perturbed by seeded noise.  Nothing synchronises.
 *   done   mjb_episode_step: the rule fires, or extra_mask_dev[env] != 0.  The rule reads state arrays only:  time_limit > 0 and time >= time_limit,
 *          or some coordinate k with !(qpos[k] >= lo[k] && qpos[k] <= hi[k]) -- a NaN is outside, an infinite bound is none.
 *          mjb_episode_reset: mask_dev[env] != 0, NULL = every env; the rule is ignored.
 *   reset  what mjb_reset does to an env (ctrl, ctrlnoise, qacc_warmstart, qfrc_applied, xfrc_applied, qacc, sensordata, time, energy zeroed, mocap
 *          poses back to the model's), except that  qpos = integrate_pos(bank_qpos[k], dq),  qvel = bank_qvel[k] + dv,  act = bank_act[k]:
 *          k = min(ninit - 1, floor(u(2 nv) ninit)) picks the bank row (no bank: qpos0, 0, 0);  dq[d] = lo[d] + (hi[d] - lo[d]) u(d) and
 *          dv[d] = lo[d] + (hi[d] - lo[d]) u(nv + d) are tangent-space vectors [nv];  integrate_pos adds on hinge and slide joints, right-multiplies
 *          a ball joint's quaternion by exp(dq) (after normalising it) and moves a free joint's position and quaternion likewise.  Without a qpos
 *          range the bank row's qpos is copied as it stands, without a qvel range its qvel.  clamp: limited hinge / slide joints are clipped to
 *          jnt_range afterwards.  episode[env] (uint32, 0 at first) is the draw's episode and is incremented by the reset.
 *   u(idx) = (w0 + 0.5) / 2^32, w0 the first word of Philox-4x32-10 with counter (genv lo32, genv hi32, episode, 0x80000000 + idx) and the 64-bit
 *          seed as key, low word first; genv = env_offset + env.  The generator of the ctrl-noise and sensor-noise streams; the top bit of the fourth
 *          counter word keeps this stream apart from theirs under one seed.  A draw depends on (seed, genv, episode, idx) alone, never on the
 *          batch's size or the launch.
 * Stream order: mask_dev / extra_mask_dev are DEVICE pointers to nenv bytes that the kernel reads on the batch's stream; the caller orders their
 * producer ahead of it (mjb_set_stream lets both run on one stream; a done buffer, mjb_episode_device_ptr(any batch, 0), is a legal mask -- this
 * batch's own too: the kernel has read an env's mask byte before it writes the env's done byte).
 * What the rule sees: it is evaluated between launches, on the state as the last launch left it.  With K fused steps (mjb_step(b, K)) an env may run
 * up to K - 1 steps past its limit before it is reset; resets inside the step kernel are out of scope (the step's own mj_check* auto-reset to qpos0
 * is unchanged).
 * Like mjb_reset, both calls abandon an open split step and leave the derived fields unreadable (mjb_get of one, mjb_rays_cast, mjb_jac_eval, mjb_contact_eval:
 * MJB_EINVAL) until mjb_forward or a step. */
/* The initial-state bank: qpos [ninit][nq], qvel [ninit][nv], act [ninit][na], copied to the device.  ninit == 0 clears it; qvel / act NULL = zeros.
 * MJB_EINVAL: ninit < 0, a non-finite entry, a zero quaternion in a ball or free joint. */
int mjb_episode_set_init(mjb_batch *b, int ninit, const double *qpos, const double *qvel, const double *act);
/* Seed, global index of env 0 and the ranges [nv] of dq and dv; a NULL pair = no perturbation of that part.  MJB_EINVAL: one end of a pair without the
 * other, lo > hi, a non-finite value. */
int mjb_episode_set_noise(mjb_batch *b, uint64_t seed, int64_t env_offset, const double *qpos_lo, const double *qpos_hi,
                          const double *qvel_lo, const double *qvel_hi, int clamp);
/* The done rule: time_limit <= 0 = no time rule; the bounds are [nq], either may be NULL (no bound on that side).  MJB_EINVAL: a NaN. */
int mjb_episode_set_rule(mjb_batch *b, double time_limit, const double *qpos_lo, const double *qpos_hi);
int mjb_episode_reset(mjb_batch *b, const uint8_t *mask_dev);        /* asynchronous; resets mask_dev[env] != 0 (NULL: every env), writes done / ndone */
int mjb_episode_step(mjb_batch *b, const uint8_t *extra_mask_dev);   /* asynchronous; done = rule OR extra mask (may be NULL) */
/* Synchronises; done / episode [env_hi - env_lo], ndone one word, any of them may be NULL.  MJB_EINVAL: an env range outside the batch. */
int mjb_episode_get(mjb_batch *b, int env_lo, int env_hi, uint8_t *done, uint32_t *episode, uint32_t *ndone);
void *mjb_episode_device_ptr(mjb_batch *b, int which);               /* 0 done [nenv] uint8, 1 episode [nenv] uint32, 2 ndone uint32; NULL: unknown `which` */

/* ---- collision-function overrides (MujocoEnv::registerCollisionFunction, /root/reference mujoco_ros/src/mujoco_env.cpp:163-176) ----
 * The reference lets a plugin replace MuJoCo's pair function for a geom-type pair (the mjCOLLISIONFUNC table) with a host
 * callback until the next reload (:950-954).  Host callbacks cannot run inside the fused device step, so the override names
 * one of the engine's device-side pair functions instead:
 *   MJB_COLFUNC_DEFAULT  the built-in primitive function of the pair (restores the default)
 *   MJB_COLFUNC_NONE     the pair type produces no contacts (a collision function that returns 0)
 *   MJB_COLFUNC_SPHERES  both geoms are replaced by their bounding spheres (planes stay planes): at most one contact
 * geom_type1 / geom_type2 are mjtGeom values in either order; the override applies to every candidate pair of those types of
 * this batch from the next launch on.  As in the reference, whose mjCOLLISIONFUNC table is indexed by the geoms' CURRENT types, an env whose
 * geom types were changed with mjb_set_env_geom_type gets, for each candidate pair, the override registered for the pair's types in THAT env. */
enum { MJB_COLFUNC_DEFAULT = 0, MJB_COLFUNC_NONE = 1, MJB_COLFUNC_SPHERES = 2 };
int mjb_register_collision(mjb_batch *b, int geom_type1, int geom_type2, int func);

/* ---- per-env model parameters (the subset that needs no mj_setConst) ----
 * The reference mutates its single mjModel through services (setGravity, setGeomProperties friction:
 * /root/reference mujoco_ros/src/callbacks.cpp:462-592, 641-884); in a batch every env may carry its own value (domain
 * randomisation).  Envs never written keep the model's value.  gravity: [env][3]; friction: [env][ngeom][3].
 * (masses: mjb_set_env_mass_params below.)  A <contact><pair> that states its friction keeps it: mjModel.pair_friction is a compiled constant
 * the geoms' frictions do not reach (collpair_param, include/mjb_model_fields.def). */
int mjb_set_env_gravity(mjb_batch *b, int env_lo, int env_hi, const double *gravity);
int mjb_set_env_geom_friction(mjb_batch *b, int env_lo, int env_hi, const double *friction);
/* setGeomProperties' set_size / set_type (callbacks.cpp:555-575) per env: size [env][ngeom][3], type [env][ngeom] (mjtGeom: plane,
 * sphere, capsule, box; ellipsoid / cylinder are accepted and yield no contacts).  As in the reference the bounding radii are NOT recomputed ("AABBs are not recomputed", :557-560) and the
 * candidate pair list stays the model's; a pair whose new types have no pair function yields no contacts. */
int mjb_set_env_geom_size(mjb_batch *b, int env_lo, int env_hi, const double *size);
int mjb_set_env_geom_type(mjb_batch *b, int env_lo, int env_hi, const int *type);
/* setEqualityConstraintParameters (/root/reference mujoco_ros/src/callbacks.cpp:641-884: active flag, solref, solimp and the
 * type's data -- anchor / relpose / torquescale / polycoef) per env: params[env][neq][19] =
 * { active (0 / 1), eq_data[11], solref[2], solimp[5] } for every equality of the model, in model order. */
int mjb_set_env_equality(mjb_batch *b, int env_lo, int env_hi, const double *params);
/* setBodyState's mass (callbacks.cpp:210-370) followed by mj_setConst (:251-256): the engine takes, per env, the masses AND
 * what mj_setConst derives from them -- the caller computes those (the reference has libmujoco: mj_setConst on a scratch
 * mjModel; mujoco_ros_pkgs_amd/engine.py does it with its own numpy dynamics).  params[env][mjb_env_mass_stride(model)] =
 * body_mass[nbody] | body_subtreemass[nbody] | body_inertia[nbody][3] | dof_invweight0[nv] | body_invweight0[nbody][2] |
 * tendon_invweight0[ntendon] | meaninertia.  (Batches carrying these overrides run the generic kernels.)  This is the mass section of the per-env
 * block that EnvBlockLayout (csrc/mjb_dev.h) defines, the one statement of the format in the library; the block goes on with the joint and actuator
 * parameters below (model values until set). */
int mjb_env_mass_stride(const mjb_model *m);
int mjb_set_env_mass_params(mjb_batch *b, int env_lo, int env_hi, const double *params);
/* The same without the caller having MuJoCo (or Python) at hand: mj_setConst's derivation is done here, host side, in plain C++
 * (body Jacobians at qpos0 -> joint-space inertia -> its inverse; mjb_api.hip).  mjb_derive_mass_params fills ONE packed block
 * (out[mjb_env_mass_stride(model)]) from body_mass[nbody] and body_inertia[nbody][3] (NULL: the model's principal inertias) and
 * needs no device; mjb_set_env_body_mass derives a block per env (body_mass[env][nbody], body_inertia[env][nbody][3] or NULL)
 * and uploads them (= callbacks.cpp:244-258: model_->body_mass[id] = mass; mj_setConst). */
int mjb_derive_mass_params(const mjb_model *m, const double *body_mass, const double *body_inertia, double *out);
int mjb_set_env_body_mass(mjb_batch *b, int env_lo, int env_hi, const double *body_mass, const double *body_inertia);
/* ---- per-env joint and actuator parameters (domain randomisation of a robot: the values an MJCF states as <joint damping= armature=
 * frictionloss= stiffness=> and as kp / kv of <position> / <velocity> / <general>).  The reference has no service for them (its mjModel's
 * arrays are simply writable); here every env may carry its own.  The structure is the model's, the values are the env's: frame layouts,
 * item lists and kernel variants stay what mjb_compile made them.  Same conventions as above: envs [env_lo, env_hi), envs never written keep
 * the model's values, effective from the next launch, kept across mjb_reset.  (Batches carrying these overrides run the generic kernels.)
 *   mjb_set_env_dof_params       damping, armature, frictionloss: [env][nv] each, or NULL to leave that array as it is.  All finite and >= 0.
 *                                Armature changes what mj_setConst derives (dof_invweight0, body_invweight0, tendon_invweight0, meaninertia):
 *                                the engine re-derives them host side from the env's current masses, inertias and armature -- after any sequence
 *                                of mjb_set_env_body_mass and armature calls an env's constants are those of its current values.  (A packed
 *                                mjb_set_env_mass_params block is taken as given: its caller derives it, armature included.)
 *   mjb_set_env_joint_stiffness  stiffness: [env][njnt], finite and >= 0.
 *   mjb_set_env_actuator_params  gainprm, biasprm: [env][nu][3] each, or NULL: the three parameters of fixed / affine gain and bias.
 *   mjb_set_env_joint_params     all six as one block per env, params[env][mjb_env_joint_stride(model)] =
 *                                dof_damping[nv] | dof_armature[nv] | dof_frictionloss[nv] | jnt_stiffness[njnt] | gainprm[nu][3] | biasprm[nu][3]:
 *                                the joint section of EnvBlockLayout without the dof_damping_int the engine derives (mjb_env_joint_packed, csrc/mjb_dev.h).
 * What the integrator adds to M's diagonal (damping under Euler, -diag(D) under implicitfast incl. gear^2 biasprm[2] of joint actuators) is
 * derived per env from these values.  Refused, with mjb_last_error naming the reason and the batch left as it was:
 *   MJB_EINVAL        an env range outside the batch; a non-finite or negative damping / armature / frictionloss / stiffness; a non-finite gain / bias
 *   MJB_EUNSUPPORTED  positive damping under Euler (a non-zero velocity-dependent diagonal under implicitfast) on a model compiled without a
 *                     damped dof: its frames hold no M + h B;  positive frictionloss on a model compiled without dry friction: its item list
 *                     holds no friction rows (give the model one positive value; a model with mjDSBL_FRICTIONLOSS takes any value, none acts);  under implicitfast a gainprm[2] != 0 of an affine gain, or a
 *                     biasprm[2] != 0 of a site / tendon actuator, as mjb_compile refuses them on the model.
 * A dof gets its dry-friction row in the envs where its frictionloss is > 0, within the model's nefcmax (overflow: MJB_WARN_CNSTRFULL).
 * An env that sets every damping of a damped model to 0 still takes the implicit-damping solve (with h B = 0): equal to MuJoCo's explicit
 * update to rounding, not to the last bit. */
int mjb_env_joint_stride(const mjb_model *m);
int mjb_set_env_joint_params(mjb_batch *b, int env_lo, int env_hi, const double *params);
int mjb_set_env_dof_params(mjb_batch *b, int env_lo, int env_hi, const double *damping, const double *armature, const double *frictionloss);
int mjb_set_env_joint_stiffness(mjb_batch *b, int env_lo, int env_hi, const double *stiffness);
int mjb_set_env_actuator_params(mjb_batch *b, int env_lo, int env_hi, const double *gainprm, const double *biasprm);
/* mjb_derive_mass_params with a dof armature of the caller's (dof_armature[nv]; NULL: the model's) on M's diagonal: what the setters above use
 * for an env that carries its own armature.  Needs no device. */
int mjb_derive_mass_params_armature(const mjb_model *m, const double *body_mass, const double *body_inertia, const double *dof_armature, double *out);

/* ---- device-side DefaultRobotHWSim::writeSim ----
 * The reference's ros_control bridge writes the controllers' joint commands into mjData on every control callback
 * (/root/reference mujoco_ros_control/src/default_robot_hw_sim.cpp:248-326): EFFORT -> qfrc_applied, POSITION -> qpos
 * (qvel = 0), VELOCITY -> qvel, POSITION_PID / VELOCITY_PID -> qfrc_applied = clamp(PID(error, dt), +-effort_limit),
 * with the e-stop rules (:251-261, :275, :305, :313-316).  Here the same write runs on the device at the start of
 * every step of every env, from per-env command arrays resident in HBM, so closed-loop batches need no host
 * callback.  PID = control_toolbox::Pid::computeCommand (absent dependency; restated from its documented algorithm:
 * p e + clamp(i int(e), i_min, i_max) + d de/dt, anti-windup variant clamps the integral).  Position errors:
 * prismatic cmd - q; continuous shortest angular distance; revolute: cmd clamped to [lower, upper] minus q (the
 * reference calls angles::shortest_angular_distance_with_limits, equal to this whenever both lie inside the limits).
 * Deviations, deliberate: joints are addressed by their MuJoCo joint id and qposadr (the reference indexes
 * jnt_dofadr with the transmission index, which only coincides for hinge / slide-only models in URDF order). */
enum { MJB_HW_EFFORT = 0, MJB_HW_POSITION = 1, MJB_HW_POSITION_PID = 2, MJB_HW_VELOCITY = 3, MJB_HW_VELOCITY_PID = 4 };
enum { MJB_HW_REVOLUTE = 0, MJB_HW_CONTINUOUS = 1, MJB_HW_PRISMATIC = 2 };
typedef struct mjb_hwsim_joint {
	int joint;            /* MuJoCo joint id (hinge or slide) */
	int method;           /* MJB_HW_* control method */
	int kind;             /* MJB_HW_REVOLUTE / CONTINUOUS / PRISMATIC */
	int antiwindup;
	double p, i, d, i_max, i_min;
	double effort_limit;  /* <= 0: unlimited */
	double lower, upper;  /* joint limits (revolute / prismatic) */
} mjb_hwsim_joint;
/* Register the controlled joints (replaces any previous set; n = 0 switches the stage off).  Commands start at 0. */
int mjb_hwsim_configure(mjb_batch *b, int n, const mjb_hwsim_joint *joints);
/* which: 0 position, 1 velocity, 2 effort commands; cmd is [env_hi - env_lo][n] in registration order */
int mjb_hwsim_set_command(mjb_batch *b, int which, int env_lo, int env_hi, const double *cmd);
void *mjb_hwsim_command_ptr(mjb_batch *b, int which); /* device [nenv][n] */
int mjb_hwsim_estop(mjb_batch *b, int active);
/* The controller cadence MujocoRosControlPlugin::controlCallback wraps around writeSim (mujoco_ros_control/src/
 * mujoco_ros_control_plugin.cpp:153-194), for the device-side stage: readSim -- the joint state the PIDs see -- every
 * `control_period` of sim time (ros::Duration arithmetic, first at the first non-zero time: nothing is read or written at t = 0,
 * :171-176), writeSim at every step after the first update with period = time - last write (:190-193), a time that went
 * backwards re-arms both stamps (:160-169).  control_period <= 0: a write at every step on the step's own state (default).
 * A control_period below the timestep is accepted with a warning on stderr (the reference: ROS_WARN, :100-105) -- the controller
 * then updates at every step.
 * The e-stop EDGE of :180-185 restarts the controller manager's controllers -- host-side objects; the PIDs of DefaultRobotHWSim
 * itself are never reset by the reference, nor here. */
int mjb_hwsim_set_period(mjb_batch *b, double control_period);

/* Profiling builds only (libmjb_prof.so): per-stage shader-cycle sums [0..31] and call counts [32..63] of
 * env 0; all zero in the production build.  A launch records the TWO probe ids [first_id, first_id + 2) selected by
 * mjb_debug_profile_window (32 bytes of LDS: the profiled kernel keeps the shipped kernel's residency); the tool
 * sweeps the window (tools/profile_stages.py).  No reference counterpart (MuJoCo's own mjTIMER_* slots are the
 * buckets the reference's GUI profiler plots, viewer.cpp:335-346). */
int mjb_debug_profile(mjb_batch *b, unsigned long long *out64, int clear);
int mjb_debug_profile_window(mjb_batch *b, int first_id);
/* Four 64-bit FNV-1a words over the members of a compiled model: [0] the copied description, [1] every table and scalar mjb_compile derives,
 * [2] the three frame layouts, the field sizes and the frame residency, [3] the lane = env / split-step classification and tape.  Two models with
 * equal words were compiled alike; which word differs says where to look.  Needs no device.  No reference counterpart. */
int mjb_debug_model_digest(const mjb_model *m, unsigned long long out[4]);
/* Three such words over the device model blob a batch of the model would upload: [0] the offset of every table from the blob's base (16-byte
 * aligned int tables, the lane = env tape on a 64-byte boundary: checked on the way, a broken promise is MJB_EINVAL), [1] the tables' contents,
 * [2] the sizes, options and derived scalars the kernels read next to them.  Needs no device.  No reference counterpart. */
int mjb_debug_blob_digest(const mjb_model *m, unsigned long long out[3]);
/* How many device buffers, pinned host buffers, streams and events the library's batches hold right now, over all batches of the process: back at
 * its earlier value once a batch is freed.  No reference counterpart. */
int mjb_debug_live_resources(void);

/* Timing helper for bench.py: run `nlaunch` launches of mjb_step(b, nsteps) bracketed by HIP
 * events recorded on the batch's stream; returns the mean per-launch duration in milliseconds
 * through *ms_per_launch. */
int mjb_time_steps(mjb_batch *b, int nsteps, int nlaunch, double *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* MJB_H_ */
