// mjb_api.hip — the batch side of the C-ABI declared in include/mjb.h (libmjb.so).
// Owns batches: the device model blob, HBM state arrays, the launch policy and the launches, host<->device copies, the per-env parameter
// setters, the device hwsim stage and the sensor messages, with the few small kernels they need.  The model itself -- mjb_compile, the frame
// layouts, the getters that need no batch, mjb_derive_mass_params -- is mjb_model.hip's (struct mjb_model, fail(): mjb_model.h).
// What a batch holds on the device is held through the owner types of mjb_resources.h: no raw allocation, stream or event call here.
// No CPU compute path exists here: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "mjb_dev.h"
#include "mjb_episode.h"
#include "mjb_contact.h"
#include "mjb_jac.h"
#include "mjb_dyn.h"
#include "mjb_model.h"
#include "mjb_resources.h"

#define HIP_TRY(expr)                                                                                   \
	do {                                                                                                \
		hipError_t _e = (expr);                                                                         \
		if (_e != hipSuccess) return fail(MJB_ENODEVICE, "%s: %s", #expr, hipGetErrorString(_e));     \
	} while (0)

// Groups of resources that are created together, in one function each, and go together
struct RestStream {  // mjb_step_rest: the fused launch of the non-callback envs runs beside the callback envs' second half
	Stream stream;
	Event fork, join;
	int create();
};
struct NoiseStream {  // the NEXT launch's ctrl-noise normals are generated here while the current launch runs
	Stream stream;
	Event done, go;
	int create();
};
struct HwSimBufs {  // device-side DefaultRobotHWSim (mjb_hwsim_*): what HwSim points into
	DevBuf<int> ints;      // joint | method | kind | antiwindup, [4][n], then the same by dof [nv][4]
	DevBuf<double> gains;  // [n][8], then by dof [nv][8]
	DevBuf<double> cmd;    // pos | vel | eff | hold, [4][nenv][n]
	DevBuf<double> pid;    // [nenv][n][2]
	DevBuf<double> cad;    // [nenv][2 + 2 n] controller cadence (mjb_hwsim_set_period)
};
struct RayBufs {  // batched ray casting (mjb_rays_*): the ray / mask table of mjb_launch_rays and the results
	DevBuf<double> tab;
	DevBuf<double> dist;
	DevBuf<int> geomid;
};
struct JacBufs {  // batched Jacobians (mjb_jac_*): the point table of mjb_launch_jac and the outputs that were asked for (the others stay empty)
	DevBuf<double> tab;
	DevBuf<double> J, MinvJT, Ainv, vel;
};
struct DynBufs {  // batched joint-space dynamics (mjb_dyn_*): the dense index table of qM, the point table of JDOTV, the input vectors and the outputs that were asked for (the others stay empty)
	DevBuf<int> full_adr;
	DevBuf<double> tab, V;
	DevBuf<double> M, MV, MinvV, ID, Jdotv;
};
struct ConBufs {  // batched contact wrenches (mjb_contact_*): the query table of mjb_launch_contact and the outputs that were asked for (the others stay empty)
	DevBuf<unsigned int> tab;
	DevBuf<double> wrench, normal, dist, contacts;
	DevBuf<int> count;
};
struct EpisodeBufs {  // device-side episode resets (mjb_episode_*): the configuration the kernel reads and its outputs
	DevBuf<double> bank;          // qpos[ninit][nq] | qvel[ninit][nv] | act[ninit][na] (mjb_episode_set_init)
	DevBuf<double> qrange, vrange;  // lo[nv] | hi[nv] each (mjb_episode_set_noise; empty: no perturbation of that part)
	DevBuf<double> box;           // lo[nq] | hi[nq] (mjb_episode_set_rule; empty: no box)
	DevBuf<unsigned char> done;   // [nenv]
	DevBuf<unsigned int> episode, ndone;  // [nenv] | one word
};
struct SensorBufs {  // sensors-plugin equivalent (mjb_sensor_*): device copy of the noise models and the packed messages
	DevBuf<int> flag;
	DevBuf<double> mean, sigma;
	DevBuf<float> value, truth;
	bool alloc(size_t nsensor, size_t ndata) { return flag.alloc_zeroed(nsensor) && mean.alloc_zeroed(3 * nsensor) && sigma.alloc_zeroed(3 * nsensor) && value.alloc_zeroed(ndata) && truth.alloc_zeroed(ndata); }
};

// Every stream, event and buffer below has ONE owner, here; DevState, HwSim and KernelParams::le_con hold the raw views the kernels read, installed by
// set_view().  Members are destroyed in reverse order of declaration: the buffers are released first, then the side streams and the events, the batch's
// own stream last (mjb_free_batch has drained them all by then).
struct mjb_batch {
	const mjb_model *model = nullptr;
	int device = 0, nenv = 0;
	Stream stream;                // the batch's own, or the caller's (mjb_set_stream)
	RestStream rest;
	NoiseStream noise;
	std::vector<Stream> split_streams;  // the split step's env slices
	std::vector<Event> split_events;
	Event ev_split_fork, ev_rowstat;
	DevBuf<unsigned char> blob;   // device model blob
	DevModel dm{};
	DevState st{};
	DevBuf<double> state[MJB_F_COUNT];  // the state fields' arrays (MJB_DS of include/mjb_data_fields.def; the other entries stay empty)
	DevBuf<double> frame_ws, efc_Jg, pgs_B;
	DevBuf<unsigned long long> nwarn, prof;
	DevBuf<int> sched;
	FrameLayout L{};
	NoiseCfg nz{};
	int lanes = 0, epb = 0;
	unsigned int step_counter = 0;
	bool frame_valid = false;
	bool frame_half = false;      // the frame's last writer was a step's first half (mjb_step1 / mjb_step1_prefix, or a closer that ends in one): its contacts are
	                              // this state's, efc_force is not -- mjb_contact_eval refuses it
	int frame_hi = 0;             // the frame workspace is current for envs [0, frame_hi) (a prefix after mjb_step1_prefix)
	int split_ncb = -1;           // inside a split step of this prefix (mjb_step1_prefix .. mjb_step2_prefix)
	bool split_rest_done = false;
	bool rest_pending = false;
	// wide-frame policy of kernel variant 4 (launch()): counters of the last long fused launch -- env-steps, those beyond 64 rows, those
	// beyond 128 -- copied to pinned host memory behind it; the next long launch waits for that copy (the launch has ended by then or is
	// about to) and picks its frame from them: deterministic for a given sequence of launches
	bool wide = false;
	DevBuf<unsigned long long> rowstat_dev;  // (64-bit: envs x steps of one launch may exceed 2^32)
	PinnedBuf<unsigned long long> rowstat_host;
	bool rowstat_pending = false;
	bool rowstat_ever = false;     // a sample of the CURRENT workload has been looked at (cleared by mjb_reset / a new qpos: the next long launch probes first)
	bool probe_now = false, decide_now = false;  // mjb_step's probe launch / the launch behind it (launch())
	DevBuf<unsigned char> mask_dev;
	DevBuf<KernelParams> params_dev;  // device copy of {dm, L, st, nz}
	DevBuf<double> metrics_dev;       // [16] mjb_metrics
	DevBuf<unsigned long long> stats_dev;  // [MJB_NSTATS] mjb_set_stats (st.stats points here while counting)
	int *pair_i_dev = nullptr;           // device address of the per-pair int records inside the blob (mjb_register_collision patches them)
	unsigned long long steps_taken = 0;  // steps since the batch was made (step_counter is the 32-bit Philox counter)
	bool params_dirty = true;
	// sensors-plugin equivalent (mjb_sensor_*): noise models (host mirror + device copy) and the packed messages
	std::vector<int> sens_flag;
	std::vector<double> sens_mean, sens_sigma;
	SensorBufs sens;
	bool sens_dirty = true, sens_packed = false;
	RayBufs rays;                     // mjb_rays_configure
	int nray = 0;                     // rays per env of that configuration (0: none yet)
	JacBufs jac;                      // mjb_jac_configure
	int njac = 0, jac_outputs = 0;    // points per env of that configuration (0: none yet), its MJB_JAC_OUT_* bits
	DynBufs dyn;                      // mjb_dyn_configure
	int dyn_nvec = 0, dyn_npoint = 0, dyn_outputs = 0;  // vectors and points per env of that configuration, its MJB_DYN_OUT_* bits (0: none yet)
	ConBufs con;                      // mjb_contact_configure
	int ncquery = 0, con_outputs = 0; // queries of that configuration (0: none yet), its MJB_CON_OUT_* bits
	EpisodeBufs epi;                  // mjb_episode_*: the outputs are allocated at the first call that needs them
	int ep_ninit = 0, ep_clamp = 0;   // rows of the bank, clip limited hinge / slide joints to their range
	unsigned long long ep_seed = 0;   // Philox key of the episode stream ...
	long long ep_env_offset = 0;      // ... and the global index of env 0
	double ep_time_limit = 0;         // <= 0: no time rule
	bool pose_written = false;        // qpos or a mocap pose has been written through mjb_set* since the frame workspace was last made current: mjb_get still serves
	                                  // the old frame (mjData's rule); mjb_jac_eval, whose results a controller applies to the NEW state, refuses it
	bool vel_written = false;         // the same for qvel: the frame's velocity-stage fields (cvel, cdof_dot, qfrc_bias, qfrc_passive) belong to the old velocities; mjb_dyn_eval
	                                  // refuses it when ID or JDOTV is configured
	bool vel_integrated = false;      // the launch that made the frame current also advanced qvel behind it (a fused step with keep_frame, a step's second half): the
	                                  // frame's velocity stage belongs to qvel BEFORE that update (mjb_dyn_eval, JDOTV)
	DevBuf<double> pack_dev;          // staging block of mjb_get_packed / mjb_set_packed
	size_t pack_cap = 0;
	DevBuf<double> env_geom_size;
	DevBuf<int> env_geom_type;
	DevBuf<double> env_gravity, env_geom_friction, env_equality, env_mass;  // per-env model parameter overrides (mjb_set_env_*)
	std::vector<double> env_block;  // host mirror of env_mass, there whenever env_mass is: what an armature or mass change re-derives the env's mj_setConst constants from
	// device-side DefaultRobotHWSim (mjb_hwsim_*)
	HwSim hw{};
	HwSimBufs hwb;
	DevBuf<double> zbuf;           // pre-generated ctrl-noise normals of one fused launch (launch())
	size_t zcap = 0;               // its capacity in doubles PER HALF
	bool zdouble = false;          // two halves allocated (side-stream speculation possible)
	size_t zfail = (size_t)-1;     // smallest total allocation (doubles) that failed: not retried
	bool lane_env_hwsim = false;   // mjb_lane_env_set_hwsim: a batch with the device hwsim stage may run the lane = env kernel's HW build
	bool hw_le_ok = false;         // the hwsim configuration has a per-dof table (HwSim::le_tab): no dof controlled by two entries
	bool lane_env_xfrc = false;    // mjb_lane_env_set_xfrc: a batch whose xfrc_applied has been written may run the lane = env kernel's XF builds
	DevBuf<double> le_xfrc;        // their wrench table, [6 * mjb_lane_env_xfrc_slots][nenv] (DevState::le_xfrc), built at the first such launch
	bool le_xfrc_stale = true;     // xfrc_applied has been written (or reset) since the table was last filled
	int lane_env_mode = -1;        // mjb_set_lane_env: -1 automatic, 0 never, 1 whenever eligible, 2 whenever eligible, also with per-env gravity / parameter blocks
	DevBuf<double> le_con;         // lane = env kernel, a model with joint limits: qfrc_constraint | nefc | solver_iter of a launch's last step, [nenv][nv + 2] (KernelParams::le_con), allocated at the first such launch
	bool le_con_valid = false;     // ... and the last launch was one: mjb_get / mjb_get_int serve those three fields from it
	DevBuf<double> le_overlay;     // mode 2: the per-env overlay of the lane = env kernel, [mjb_lane_env_overlay_slots][nenv] (DevState::le_overlay), built at the first such launch
	int le_ov_lo = 0, le_ov_hi = 0;  // envs [lo, hi) whose overlay columns a setter has outdated since (empty: lo >= hi)
	// the split step (mjb_set_split_step): smooth half in lane = env form + constraint half per wavefront, alternating on a few streams of env slices
	int split_mode = -1;           // -1 automatic (whole-batch fused launches of >= MJB_SPLIT_MIN_ENVS envs), 0 never, 1 whenever eligible
	bool split_used = false;       // the last fused launch ran that way
	int split_slices_last = 0;
	DevBuf<double> handoff_dev;    // DevState::handoff
	DevBuf<double> reset_step_dev; // DevState::reset_step
	bool lane_env_used = false;    // the last fused launch ran the lane = env kernel
	bool le_unavailable = false;   // the model's topology had to be built by hiprtc and that failed (mjb_lane_env_jit_error): generic kernels from then on
	int noise_mode = 0;            // how the last fused launch got its ctrl-noise normals: 0 in-kernel, 1 same-stream, 2 side-stream (mjb_noise_mode)
	DevBuf<unsigned int> zinfo;    // two records (one per half of zbuf)
	bool zvalid = false;           // a record names a launch: cleared (on the stream) before any step launch that does not use the buffer
	bool spec_valid = false;       // half `spec_half` holds (or will, once noise.done fires) the normals of launch (spec_step0, spec_nsteps)
	int spec_half = 0, spec_nsteps = 0;
	unsigned int spec_step0 = 0;
};

namespace {

// a state field the poses of the frame are computed from (mjb_batch::pose_written)
bool pose_field(int field) { return field == MJB_F_qpos || field == MJB_F_mocap_pos || field == MJB_F_mocap_quat; }

// the kernels' raw view of one of the batch's buffers (a member of b->st or b->hw): assigned here, so that the parameter block is uploaded again
template <typename V, typename P> void set_view(mjb_batch *b, V &view, P p)
{
	view = p;
	b->params_dirty = true;
}

struct BatchDeleter {
	void operator()(mjb_batch *b) const { mjb_free_batch(b); }
};
typedef std::unique_ptr<mjb_batch, BatchDeleter> BatchPtr;

}  // namespace

// (all three or none: a group that exists is whole)
int RestStream::create()
{
	hipError_t e = stream.create();
	if (e == hipSuccess) e = fork.create();
	if (e == hipSuccess) e = join.create();
	if (e == hipSuccess) return MJB_OK;
	*this = RestStream{};
	return fail(MJB_ENODEVICE, "rest stream: %s", hipGetErrorString(e));
}
int NoiseStream::create()
{
	hipError_t e = stream.create();
	if (e == hipSuccess) e = done.create();
	if (e == hipSuccess) e = go.create();
	if (e == hipSuccess) return MJB_OK;
	*this = NoiseStream{};
	return fail(MJB_ENODEVICE, "noise stream: %s", hipGetErrorString(e));
}

extern "C" {

int mjb_model_desc_size(void) { return (int)sizeof(mjb_model_desc); }
int mjb_version(void) { return MJB_VERSION; }

int mjb_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int mjb_debug_live_resources(void) { return g_live_resources.load(); }

void mjb_free_batch(mjb_batch *b)
{
	if (!b) return;
	hipSetDevice(b->device);
	if (b->stream.get()) hipStreamSynchronize(b->stream.get());
	if (b->rest.stream.get()) hipStreamSynchronize(b->rest.stream.get());
	if (b->noise.stream.get()) hipStreamSynchronize(b->noise.stream.get());
	for (const Stream &st : b->split_streams) hipStreamSynchronize(st.get());
	delete b;
}

}  // extern "C"

// ---- mjb_make_batch, step by step: each returns false after fail()
static bool batch_check_device(int device)
{
	const int ndev = mjb_device_count();
	if (ndev <= 0) return fail(MJB_ENODEVICE, "mjb_make_batch: no HIP device available (this engine has no CPU fallback)"), false;
	if (device < 0 || device >= ndev) return fail(MJB_EINVAL, "mjb_make_batch: device %d out of range (%d devices)", device, ndev), false;
	if (hipSetDevice(device) != hipSuccess) return fail(MJB_ENODEVICE, "mjb_make_batch: hipSetDevice(%d) failed", device), false;
	return true;
}

// the model blob (build_model_blob, mjb_model.hip) as it stands, and the DevModel that points into it
static bool batch_upload_model(mjb_batch *b)
{
	ModelBlob B = build_model_blob(*b->model);
	if (!b->blob.alloc(B.image.size())) return fail(MJB_ENOMEM, "mjb_make_batch: hipMalloc(model blob) failed"), false;  // (the upload writes all of it)
	if (hipMemcpy(b->blob.get(), B.image.data(), B.image.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(MJB_ENODEVICE, "mjb_make_batch: model upload failed"), false;
	b->dm = B.dm;
	rebase_model_blob(*b->model, b->dm, b->blob.get());
	b->pair_i_dev = reinterpret_cast<int *>(b->blob.get() + B.pair_i_offset);
	return true;
}

static bool batch_alloc_state(mjb_batch *b)
{
	const mjb_model *M = b->model;
	DevState &s = b->st;
	s.nenv = b->nenv;
	bool ok = true;
	int fidx = 0;
#define MJB_DS(name, rows, cols)                                                                       \
	ok = ok && b->state[fidx].alloc_zeroed((size_t)b->nenv * M->field_size[fidx]);                     \
	s.name = b->state[fidx].get();                                                                     \
	fidx++;
#define MJB_DD(name, rows, cols) fidx++;
#define MJB_DD2(name, rows, cols) fidx++;
#define MJB_DI(name, rows, cols) fidx++;
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
	ok = ok && b->nwarn.alloc_zeroed(MJB_NWARNING) && b->prof.alloc_zeroed(64);
	s.nwarn = b->nwarn.get();
	s.prof = b->prof.get();
	s.frame_stride = b->L.ndouble + b->L.nint / 2;
	if (M->slot) s.frame_stride = std::max(s.frame_stride, M->Lc.ndouble + M->Lc.nint / 2);  // (row-slot kernels: fused frames in HBM live there too)
	for (int k = 0; k < 64; k++) s.colfunc[k] = MJB_COLFUNC_DEFAULT;
	if (!ok) fail(MJB_ENOMEM, "mjb_make_batch: hipMalloc(state) failed for %d envs", b->nenv);
	return ok;
}

// what the model's solver needs beside the frames
static bool batch_alloc_solver_scratch(mjb_batch *b)
{
	const mjb_model *M = b->model;
	const mjb_model_desc &h = M->h;
	const int nenv = b->nenv;
	DevState &s = b->st;
	bool ok = true;
	if (h.nefcmax > 0) {  // constrained kernels: work queue of the chunked fused launches
		ok = ok && b->sched.alloc_zeroed((size_t)nenv + 1);
		s.sched = b->sched.get();
	}
	if (M->hbm_full) {  // row-slot kernels: launches on the full frame (and on the fused one, when it is too large too) run in the workspace
		ok = ok && b->frame_ws.alloc_zeroed((size_t)nenv * s.frame_stride);
		s.frame_ws = b->frame_ws.get();
	}
	if (h.solver == MJB_SOL_NEWTON && h.nefcmax > 128 && !M->slot) {  // kernel variant 4: row data of the env-steps beyond the fused frame's 64 rows
		// (stride: the kernels index the block with the cone-block stride of the frame THEY run on -- the wide frame of an all-condim-3 model has
		//  hcs 16 where the default frame has 10: size for the largest of the three layouts)
		s.efc_Jg_stride = mjb_rowblock_doubles(h.nefcmax, h.nv, h.nconmax, std::max(M->L.hcs, std::max(M->Lc.hcs, M->Lw.hcs)));
		ok = ok && b->efc_Jg.alloc_zeroed((size_t)nenv * s.efc_Jg_stride);
		s.efc_Jg = b->efc_Jg.get();
		if (M->has_wide)  // row counters of the wide-frame policy (launch(), which points DevState::rowstat at them for the launches that count)
			ok = ok && b->rowstat_dev.alloc_zeroed(4) && b->rowstat_host.alloc_zeroed(4) && b->ev_rowstat.create() == hipSuccess;
	}
	if (h.solver == MJB_SOL_PGS && h.nv <= 16 && h.nefcmax > 64) {
		ok = ok && b->pgs_B.alloc_zeroed((size_t)nenv * h.nefcmax * h.nv);  // (elliptic PGS never exceeds 64 rows: mjb_compile)
		s.pgs_B = b->pgs_B.get();
	}
	if (!ok) fail(MJB_ENOMEM, "mjb_make_batch: hipMalloc(state) failed for %d envs", nenv);
	return ok;
}

static bool batch_create_stream(mjb_batch *b)
{
	if (b->stream.create() != hipSuccess) return fail(MJB_ENODEVICE, "mjb_make_batch: hipStreamCreate failed"), false;
	mjb_set_launch(b, 0, 0);
	return true;
}

static bool batch_first_reset(mjb_batch *b) { return mjb_reset(b, nullptr) == MJB_OK && mjb_synchronize(b) == MJB_OK; }

extern "C" {

mjb_batch *mjb_make_batch(const mjb_model *M, int nenv, int device)
{
	if (!M || nenv <= 0) {
		fail(MJB_EINVAL, "mjb_make_batch: bad argument");
		return nullptr;
	}
	if (!batch_check_device(device)) return nullptr;
	BatchPtr b(new (std::nothrow) mjb_batch);
	if (!b) {
		fail(MJB_ENOMEM, "mjb_make_batch: out of memory");
		return nullptr;
	}
	b->model = M;
	b->device = device;
	b->nenv = nenv;
	b->L = M->L;
	if (const char *v = getenv("MJB_LANE_ENV")) {  // default lane_env_mode of new batches (include/mjb.h, mjb_set_lane_env)
		const int k = atoi(v);
		if (k >= -1 && k <= 2) b->lane_env_mode = k;
	}
	if (!batch_upload_model(b.get()) || !batch_alloc_state(b.get()) || !batch_alloc_solver_scratch(b.get()) || !batch_create_stream(b.get()) || !batch_first_reset(b.get()))
		return nullptr;
	clear_error();
	return b.release();
}

int mjb_nenv(const mjb_batch *b) { return b ? b->nenv : fail(MJB_EINVAL, "null batch"); }

int mjb_set_launch(mjb_batch *b, int lanes_per_env, int envs_per_block)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const bool constrained = b->model->h.nefcmax > 0;
	if (lanes_per_env == 0) lanes_per_env = constrained ? 64 : 16;
	if (constrained && lanes_per_env != 64)
		return fail(MJB_EINVAL, "mjb_set_launch: models with constraint rows run one env per wavefront (lanes_per_env = 64)");
	if (lanes_per_env != 8 && lanes_per_env != 16 && lanes_per_env != 32 && lanes_per_env != 64)
		return fail(MJB_EINVAL, "mjb_set_launch: lanes_per_env must be 8, 16, 32 or 64");
	if (envs_per_block <= 0) envs_per_block = 64 / lanes_per_env;  // one wavefront per workgroup
	if (envs_per_block * lanes_per_env > 256) envs_per_block = 256 / lanes_per_env;
	b->lanes = lanes_per_env;
	b->epb = envs_per_block;
	return MJB_OK;
}

static int ensure_ws(mjb_batch *b)
{
	if (b->frame_ws) return MJB_OK;
	if (!b->frame_ws.alloc_zeroed((size_t)b->nenv * b->st.frame_stride)) return fail(MJB_ENOMEM, "frame workspace allocation failed");
	set_view(b, b->st.frame_ws, b->frame_ws.get());
	return MJB_OK;
}

// (re)upload the launch parameters when anything in them changed; ordered on the batch's stream
static int sync_params(mjb_batch *b)
{
	if (!b->params_dev) {
		if (!b->params_dev.alloc(1)) return fail(MJB_ENOMEM, "launch parameters: allocation failed");  // (uploaded whole below)
		b->params_dirty = true;
	}
	if (b->params_dirty) {
		KernelParams kp;
		kp.m = b->dm;
		kp.L = b->L;
		kp.Lc = b->wide ? b->model->Lw : b->model->Lc;
		kp.use_compact = (b->st.use_xfrc || b->st.keep_frame) ? 0 : (b->wide ? 2 : 1);  // (the value doubles as the layout's index into the host-built copy tables)
		kp.pad0 = 0;
		kp.s = b->st;
		kp.nz = b->nz;
		kp.hw = b->hw;
		kp.le_con = b->le_con.get();
		// pageable source: the copy is staged before the call returns, so the local may go out of scope
		HIP_TRY(hipStreamSynchronize(b->stream.get()));
		// (the fused launch of the non-callback envs, mjb_step_rest, runs on its own non-blocking stream and reads *params_dev lazily
		//  through scalar loads -- use_compact, use_xfrc, the layouts: an upload between mjb_step_rest and the second half, e.g. the
		//  first pushViews that carries a non-zero xfrc_applied, must not overtake it)
		if (b->rest_pending && b->rest.stream.get()) HIP_TRY(hipStreamSynchronize(b->rest.stream.get()));
		if (b->spec_valid && b->noise.stream.get()) HIP_TRY(hipStreamSynchronize(b->noise.stream.get()));  // (the side-stream noise generator reads nz)
		HIP_TRY(hipMemcpy(b->params_dev.get(), &kp, sizeof kp, hipMemcpyHostToDevice));
		b->params_dirty = false;
	}
	return MJB_OK;
}

// whole-batch operations on the batch's stream wait for a fused launch of the non-callback envs that is still pending on the rest
// stream (a split step abandoned between mjb_step_rest and its second half -- an error, a reset raised inside a callback)
static int join_rest(mjb_batch *b)
{
	if (b->rest_pending) {
		HIP_TRY(hipStreamWaitEvent(b->stream.get(), b->rest.join.get(), 0));
		b->rest_pending = false;
	}
	return MJB_OK;
}

// the model's kernel variant (MJB_KV_*, mjb_dev.h) before launch() looks at the frame and the mode
static int kernel_variant(const mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	const bool cg = h.solver == MJB_SOL_CG;
	if (h.nefcmax <= 0) return MJB_KV_NONE;
	if (M->slot) return cg ? MJB_KV_SLOT_CG : MJB_KV_SLOT_NEWTON;
	if (h.solver == MJB_SOL_PGS) return (h.cone == MJB_CONE_ELLIPTIC && h.nconmax > 0) ? MJB_KV_PGS_ELL : MJB_KV_PGS;
	if (h.nefcmax <= 64) return cg ? MJB_KV_CG1 : MJB_KV_NEWTON1;
	if (h.nefcmax <= 128) return cg ? MJB_KV_CG2 : MJB_KV_NEWTON2;
	return cg ? MJB_KV_CG4 : MJB_KV_NEWTON4;
}

// the dense-M build of the unconstrained 16-lane kernel (StepLaunch::dense): small Euler models without per-env inertia, not the chained step
static int dense_build(const mjb_batch *b, int mode)
{
	const mjb_model_desc &h = b->model->h;
	if (!(b->lanes == 16 && !b->env_mass.get() && mode != MJB_MODE_STEP21 && h.integrator == MJB_INT_EULER && h.nefcmax <= 0 && h.nv <= 16 && h.nbody <= 16 && h.nu <= 16 &&
	      h.njnt <= 16))
		return 0;
	return h.nv <= 8 ? 8 : (h.nv <= 12 ? 12 : 16);
}

static bool stream_capturing(hipStream_t st)
{
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
		(void)hipGetLastError();
		return false;
	}
	return cs != hipStreamCaptureStatusNone;
}

// ---- the split step: per step, the smooth half of every env of a slice in lane = env form (mjb_smooth_kernel.h), then the slice's
// constraint half one env per wavefront (mjb_cstep_kernel).  The smooth kernel is a latency (a few dozen wavefronts, ~20 us), the constraint kernel is
// the throughput: the batch is cut into slices that alternate the two on streams of their own, so one slice's smooth half runs beside the others'
// constraint halves.  A slice's launches are ordered by its stream; slices share nothing (no data-path exchange between envs).
static int split_slices(const mjb_batch *b, int nenv)
{
	static const int forced = mjb_env_int("MJB_SPLIT_SLICES", 0);  // measurement knob
	// (measured on config 3, MI355X, profiles/r06_split_step.txt: two slices are best from 32 768 envs up -- 33.2 M env-steps/s against the fused kernel's
	//  27.5 M; more slices mean shorter launches, and a launch ends with its slowest env)
	int n = forced > 0 ? forced : 2;
	const int waves = (nenv + 63) / 64;
	if (n > waves) n = waves;
	if (n > 16) n = 16;
	(void)b;
	return n < 1 ? 1 : n;
}

// the state one step after mj_resetData (mj_checkAcc's reset inside mjb_cstep_kernel), from a one-env batch on the generic kernels
static int split_reset_state(mjb_batch *b)
{
	const mjb_model_desc &h = b->model->h;
	BatchPtr owner(mjb_make_batch(b->model, 1, b->device));
	mjb_batch *t = owner.get();
	if (!t) return MJB_ENOMEM;
	t->split_mode = 0;
	std::vector<double> buf((size_t)h.nq + 2 * h.nv);
	int rc = mjb_reset(t, nullptr);
	if (rc == MJB_OK) rc = mjb_step(t, 1);
	if (rc == MJB_OK) rc = mjb_get(t, MJB_F_qpos, 0, 1, buf.data());
	if (rc == MJB_OK) rc = mjb_get(t, MJB_F_qvel, 0, 1, buf.data() + h.nq);
	if (rc == MJB_OK) rc = mjb_get(t, MJB_F_qacc_warmstart, 0, 1, buf.data() + h.nq + h.nv);
	owner.reset();
	if (rc != MJB_OK) return rc;
	HIP_TRY(hipSetDevice(b->device));
	DevBuf<double> dev;
	if (!dev.alloc(buf.size())) return fail(MJB_ENOMEM, "split step: reset state");  // (the upload writes all of it)
	HIP_TRY(hipMemcpy(dev.get(), buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
	b->reset_step_dev = std::move(dev);
	set_view(b, b->st.reset_step, b->reset_step_dev.get());
	return MJB_OK;
}

static int split_prepare(mjb_batch *b)
{
	const mjb_model_desc &h = b->model->h;
	if (!b->reset_step_dev) {
		int rc = split_reset_state(b);
		if (rc) return rc;
	}
	if (!b->handoff_dev) {
		const HandoffLayout hl = mjb_handoff_layout(h.ngeom, h.nv, h.nbody, h.nM);
		if (!b->handoff_dev.alloc_zeroed((size_t)b->nenv * hl.stride)) return fail(MJB_ENOMEM, "split step: hand-off records");
		b->st.handoff_stride = hl.stride;
		set_view(b, b->st.handoff, b->handoff_dev.get());
	}
	if (!b->ev_split_fork) HIP_TRY(b->ev_split_fork.create());
	return MJB_OK;
}

static int launch_split(mjb_batch *b, int nsteps, int env_lo, int env_hi, hipStream_t stream)
{
	const int nenv = env_hi - env_lo;
	const int ns = split_slices(b, nenv);
	while ((int)b->split_streams.size() < ns) {  // (a slice's stream and its event: in step)
		Stream st;
		Event ev;
		HIP_TRY(st.create());
		HIP_TRY(ev.create());
		b->split_streams.push_back(std::move(st));
		b->split_events.push_back(std::move(ev));
	}
	const FrameLayout &Lc = b->model->Lc;
	const int cflags = b->st.stats ? 1 : 0;
	// slices of whole wavefronts of the smooth kernel
	const int waves = (nenv + 63) / 64;
	HIP_TRY(hipEventRecord(b->ev_split_fork.get(), stream));
	for (int k = 0; k < ns; k++) {
		const int w0 = (int)((long long)waves * k / ns), w1 = (int)((long long)waves * (k + 1) / ns);
		const int lo = env_lo + 64 * w0, hi = std::min(env_hi, env_lo + 64 * w1);
		if (hi <= lo) continue;
		hipStream_t st = ns == 1 ? stream : b->split_streams[k].get();
		if (ns > 1) HIP_TRY(hipStreamWaitEvent(st, b->ev_split_fork.get(), 0));
		for (int i = 0; i < nsteps; i++) {
			int rc = mjb_launch_smooth(b->params_dev.get(), b->model->sm_topo, lo, hi, b->step_counter + (unsigned int)i, i == nsteps - 1 ? 1 : 0, st);
			if (rc == 0) rc = mjb_launch_cstep(b->params_dev.get(), Lc, lo, hi, b->epb, cflags, st);
			if (rc != 0) return fail(MJB_ENODEVICE, "split step launch failed: %s", hipGetErrorString((hipError_t)rc));
		}
		if (ns > 1) {
			HIP_TRY(hipEventRecord(b->split_events[k].get(), st));
			HIP_TRY(hipStreamWaitEvent(stream, b->split_events[k].get(), 0));
		}
	}
	b->split_slices_last = ns;
	return MJB_OK;
}

// what one launch() call was asked for: the decisions below read it
struct LaunchReq {
	int mode, nsteps, env_lo, env_hi;
	hipStream_t stream;
	bool whole;    // the whole batch
	bool compact;  // runs on the fused frame
};

// facts more than one decision asks
static bool no_env_overrides(const mjb_batch *b) { return b->hw.n == 0 && !b->env_mass.get() && !b->env_gravity.get(); }  // no per-env inertia / gravity, no device hwsim stage
static bool eight_lean_frames_fit(const mjb_model *M) { return 8 * mjb_frame_bytes(M, 1) <= mjb_max_lds_bytes(); }  // ... one CU's LDS
static bool chained_mode(int mode) { return mode == MJB_MODE_STEP21 || mode == MJB_MODE_RKMID || mode == MJB_MODE_RKLAST; }

// the model's variant on the frame this launch runs on: the row-slot kernels take a frame beyond one CU's LDS from HBM
static int frame_variant(mjb_batch *b, const LaunchReq &q, int *variant)
{
	*variant = kernel_variant(b->model);
	if (mjb_kv_slot(*variant) && (q.compact ? b->model->hbm_fused : b->model->hbm_full)) {
		if (int wrc = ensure_ws(b)) return wrc;
		*variant = mjb_kv_hbm(*variant);
	}
	return MJB_OK;
}

// Which fused frame (kernel variant 4 with a wide frame): a long whole-batch launch looks at the row counters of the previous one.
// More than a quarter of the env-steps beyond 64 rows: the wide frame (128 rows in LDS, two envs per CU) -- measured on the
// power-grasp workload of config 5 (94 % beyond 64 rows): 0.72 -> 2.41 M env-steps/s; fewer than 5 %: back to the default frame
// (four envs per CU: the light workload runs 7.8 M on it, 4.2 M on the wide one).  MJB_WIDE_FRAME=0 / 1 pins the choice.
// *count_rows: this launch counts its rows for the next one's choice.
static int choose_fused_frame(mjb_batch *b, const LaunchReq &q, int variant, bool *count_rows)
{
	*count_rows = false;
	if (!(variant == MJB_KV_NEWTON4 && b->model->has_wide && b->rowstat_dev.get())) return MJB_OK;
	static const int pinned = mjb_env_int("MJB_WIDE_FRAME", -1);
	bool want = b->wide;
	if (pinned >= 0) want = pinned != 0;
	else if (q.compact && q.whole && (q.nsteps >= 100 || b->probe_now || b->decide_now) && !stream_capturing(q.stream)) {  // (under stream capture nothing can be waited for: the frame stays)
		if (b->rowstat_pending) {
			// (the newest COMPLETED sample: a launch behind a running counting launch does not wait for it -- back-to-back launches stay
			//  enqueued ahead of the device -- except right behind mjb_step's probe launch, whose whole point is this decision)
			// Default: WAIT for the previous counting launch's sample (it has ended or is about to) -- the choice is then a function of the
			// sequence of launches alone, and a rollout reproduces bit for bit.  MJB_WIDE_POLICY_NOWAIT=1: take it only if it has landed
			// (back-to-back launches stay enqueued ahead of the device; which launch switches frames then depends on timing, results agree to
			// rounding).  Right behind mjb_step's probe launch the wait is the point.
			static const bool nowait = [] { const char *v = getenv("MJB_WIDE_POLICY_NOWAIT"); return v && *v == '1'; }();
			const hipError_t e = (b->decide_now || !nowait) ? hipEventSynchronize(b->ev_rowstat.get()) : hipEventQuery(b->ev_rowstat.get());
			if (e == hipSuccess) {
				b->rowstat_pending = false;
				b->rowstat_ever = true;
				const double tot = (double)b->rowstat_host.get()[0], gt64 = (double)b->rowstat_host.get()[1];
				if (tot > 0) {
					if (!b->wide && gt64 > 0.25 * tot) want = true;
					else if (b->wide && gt64 < 0.05 * tot) want = false;
				}
			} else if (e != hipErrorNotReady)
				return fail(MJB_ENODEVICE, "hipEventQuery(row counters): %s", hipGetErrorString(e));
			else
				(void)hipGetLastError();
		}
		*count_rows = !b->rowstat_pending;  // (one sample in flight at a time: the pinned words belong to it)
	}
	if (want != b->wide) {
		b->wide = want;
		b->params_dirty = true;
	}
	return MJB_OK;
}

// The split step for plain-PGS models whose smooth stages have a lane = env kernel (config 3): fused launches of the whole batch (or, forced, any range)
static int choose_split_step(mjb_batch *b, const LaunchReq &q, int variant, bool *use_split)
{
	*use_split = false;
	if (q.mode == MJB_MODE_STEP && q.compact && variant == MJB_KV_PGS && b->model->sm_topo >= 0 && b->split_mode != 0 && no_env_overrides(b) && !b->env_equality.get() &&
	    eight_lean_frames_fit(b->model) && !stream_capturing(q.stream)) {
		// (automatic mode: OFF unless MJB_SPLIT_MIN_ENVS names a batch size.  Measured on config 3 at 32 768 envs, profiles/r06_split_step.txt: +21 % in the
		//  rollout's light-contact phase, +12 % over steps 1000 - 4000, -5 % over steps 500 - 2000 -- a launch pair per step ends with the slice's slowest env,
		//  and the heavy phase has the long PGS tails.  Not a rule to apply behind the user's back.)
		static const int min_envs = mjb_env_int("MJB_SPLIT_MIN_ENVS", 0);
		*use_split = b->split_mode == 1 || (min_envs > 0 && q.whole && b->nenv >= min_envs);
		if (*use_split) return split_prepare(b);
	}
	return MJB_OK;
}

// which build of the plain PGS step
static int pgs_build(const mjb_batch *b, const LaunchReq &q, int variant)
{
	// on the lean frame: when eight envs fit one CU's LDS, the 256-register build runs two waves per SIMD
	if (variant == MJB_KV_PGS && q.compact && eight_lean_frames_fit(b->model)) variant = MJB_KV_PGS256;
	static const int forced = mjb_env_int("MJB_DEBUG_VARIANT", -1);  // measurement knob
	if ((forced == MJB_KV_PGS || forced == MJB_KV_PGS256) && (variant == MJB_KV_PGS || variant == MJB_KV_PGS256)) variant = forced;  // (only the two builds of the same PGS step are interchangeable)
	if (chained_mode(q.mode) && variant == MJB_KV_PGS256) variant = MJB_KV_PGS;  // (the 256-register build carries no chained-step / cut-RK4 mode)
	return variant;
}

// Steps per work item: long fused launches of the constrained kernels hand out (chunk of steps, env) work items dynamically (mjb_step.hip)
// ... unless every env gets a slot of its own (envs <= resident envs per CU x CUs): then the queue has nothing to even out, an
// item taken by a wave whose env's previous chunk is still running elsewhere only waits, and the launch is fastest with each
// env's steps run back to back on its slot.  Measured on config 5 (4 envs per CU = 1024 slots, MI355X), chunked / unchunked:
// 1024 envs x 100 steps 4.04 / 4.72 M env-steps/s, x 1000 steps 4.20 / 5.00 M, 768 envs 3.40 / 3.75 M; 1280 envs 5.32 / 3.38 M.
// A chunked launch (*chunk > 0) gets its work counters cleared on the stream.
static int choose_chunk(mjb_batch *b, const LaunchReq &q, int variant, int *chunk)
{
	bool own_slot = false;
	if (q.compact && variant != MJB_KV_NONE) {
		int ncu = 0;  // (of THIS batch's device: a process may drive several)
		if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess) ncu = 0;
		const int granules = (mjb_frame_bytes(b->model, b->wide ? 2 : 1) + 1279) / 1280;  // (gfx950: 128 LDS granules of 1280 bytes per CU)
		const int occ = std::min(variant == MJB_KV_PGS256 ? 8 : 4, 128 / std::max(1, granules));  // (512-register kernels: one wave per SIMD)
		own_slot = ncu > 0 && b->nenv <= occ * ncu;
	}
	*chunk = 0;
	static const int forced = mjb_env_int("MJB_DEBUG_CHUNK", 0);  // measurement knob (also overrides own_slot)
	if (q.mode == MJB_MODE_STEP && variant != MJB_KV_NONE && q.nsteps >= 100 && b->st.sched && q.whole && (!own_slot || forced > 0)) {
		static const bool off = mjb_env_flag("MJB_DEBUG_NO_CHUNKS");  // measurement knob
		if (!off) {
			// (measured on MI355X: 10 - 40 steps per item are equally good on config 3; config 5 -- three envs per CU, a few heavy envs
			//  on the critical path -- likes them finer: 3 - 5 steps per item 3.85 M, 10 steps 3.79 M, 20 steps 3.63 M)
			*chunk = forced > 0 ? forced : (mjb_kv_newton(variant) ? std::max(5, (q.nsteps + 19) / 20) : std::max(10, (q.nsteps + 15) / 16));
			*chunk = std::min(*chunk, 65535);
			HIP_TRY(hipMemsetAsync(b->st.sched, 0, ((size_t)b->nenv + 1) * sizeof(int), q.stream));
		}
	}
	return MJB_OK;
}

// the ctrl-noise buffer grows to `need` doubles per half (two halves when want_double): both streams drain before the old one is freed
static int grow_noise_buffer(mjb_batch *b, const LaunchReq &q, size_t need, bool want_double)
{
	const size_t total = want_double ? 2 * need : need;
	HIP_TRY(hipStreamSynchronize(q.stream));
	if (b->noise.stream.get()) HIP_TRY(hipStreamSynchronize(b->noise.stream.get()));
	b->spec_valid = false;
	if (!b->zbuf.alloc_zeroed(total)) b->zfail = total;  // (the old one is gone; remembered: a launch of this size or larger generates in the kernel from now on)
	b->zcap = b->zbuf ? need : 0;
	b->zdouble = b->zbuf && want_double;
	if (!b->zinfo) b->zinfo.alloc_zeroed(8);
	if (b->zinfo) HIP_TRY(hipMemset(b->zinfo.get(), 0xff, 8 * sizeof(unsigned int)));
	b->zvalid = false;
	if (b->zdouble && !b->noise.stream) {
		if (int rc = b->noise.create()) return rc;
	}
	b->st.zhalf = (unsigned long long)b->zcap;
	set_view(b, b->st.zbuf, b->zbuf.get());
	set_view(b, b->st.zinfo, b->zbuf ? b->zinfo.get() : nullptr);
	return sync_params(b);
}

// ctrl noise of a long fused launch: its normals are generated by a throughput kernel (mjb_noise_kernel) instead of inside every
// step's dependent chain, when they fit the budget (MJB_NOISE_PREGEN_MB = the TOTAL allocation, default 2048; 0: always inside
// the step kernel -- same values either way).  Unconstrained kernels (one wave per SIMD, 320 VGPRs: a second kernel finds room) get
// a buffer of two halves: this launch reads one while the other is filled, on a side stream, for the launch expected next (same
// length, the step counter this one ends at); a launch that finds its normals ready only waits for that event, anything else
// generates them on its own stream first.  The constrained kernels fill the register file (256 / 512 VGPRs at two / one waves per
// SIMD): a side-stream generator only finds a slot when the step launch drains (rocprofv3 showed it spanning the whole 130 - 180 ms
// launch), so they -- and launches whose two halves exceed the budget -- generate one half on their own stream.
// *zuse: the launch reads pre-generated normals, from half *zhalf of the buffer.
static int stage_ctrl_noise(mjb_batch *b, const LaunchReq &q, int variant, bool *zuse, int *zhalf)
{
	*zuse = false;
	*zhalf = 0;
	b->noise_mode = 0;
	const int nu = b->model->h.nu;
	if (q.mode == MJB_MODE_STEP && q.whole && b->nz.enabled && q.nsteps >= 16 && nu > 0 && nu <= b->lanes) {
		static const size_t cap_doubles = [] { const char *v = getenv("MJB_NOISE_PREGEN_MB"); return (size_t)(v ? atol(v) : 2048) * (1u << 20) / sizeof(double); }();
		const size_t need = (size_t)q.nsteps * b->nenv * nu;
		const bool want_double = variant == MJB_KV_NONE && 2 * need <= cap_doubles;
		const size_t total = want_double ? 2 * need : need;
		if (total <= cap_doubles && total < b->zfail) {
			if (need > b->zcap || (want_double && !b->zdouble)) {
				if (int rc = grow_noise_buffer(b, q, need, want_double)) return rc;
			}
			if (b->zbuf.get() && b->zinfo.get()) {
				if (b->spec_valid && b->spec_step0 == b->step_counter && b->spec_nsteps == q.nsteps) {
					*zhalf = b->spec_half;
					HIP_TRY(hipStreamWaitEvent(q.stream, b->noise.done.get(), 0));  // generated while the previous launch ran
					b->noise_mode = 2;
				} else {
					if (b->spec_valid) HIP_TRY(hipStreamWaitEvent(q.stream, b->noise.done.get(), 0));  // (a generator still writing its half: let it finish first)
					HIP_TRY(hipMemsetAsync(b->zinfo.get() + 4, 0xff, 4 * sizeof(unsigned int), q.stream));
					int nrc = mjb_launch_noise(b->params_dev.get(), b->zbuf.get(), b->zinfo.get(), b->nenv, nu, q.nsteps, b->step_counter, q.stream);
					if (nrc != 0) return fail(MJB_ENODEVICE, "noise kernel launch failed: %s", hipGetErrorString((hipError_t)nrc));
					b->noise_mode = 1;
				}
				b->spec_valid = false;
				*zuse = b->zvalid = true;
			}
		}
	}
	if (!*zuse && b->zvalid) {  // (a launch that generates its normals itself must not match a record left by an earlier one)
		if (b->spec_valid) HIP_TRY(hipStreamWaitEvent(q.stream, b->noise.done.get(), 0));
		b->spec_valid = false;
		HIP_TRY(hipMemsetAsync(b->zinfo.get(), 0xff, 8 * sizeof(unsigned int), q.stream));
		b->zvalid = false;
	}
	return MJB_OK;
}

// the next launch's normals, into the half this one does not read, beside it (ev_noise_go: recorded ahead of this launch on its stream)
static int speculate_ctrl_noise(mjb_batch *b, const LaunchReq &q, int zhalf_now)
{
	const int other = 1 - zhalf_now;
	const unsigned int next0 = b->step_counter + (unsigned int)q.nsteps;
	HIP_TRY(hipStreamWaitEvent(b->noise.stream.get(), b->noise.go.get(), 0));
	int nrc = mjb_launch_noise(b->params_dev.get(), b->zbuf.get() + (size_t)other * b->zcap, b->zinfo.get() + 4 * other, b->nenv, b->model->h.nu, q.nsteps, next0, b->noise.stream.get());
	if (nrc == 0) {
		HIP_TRY(hipEventRecord(b->noise.done.get(), b->noise.stream.get()));
		b->spec_valid = true;
		b->spec_half = other;
		b->spec_step0 = next0;
		b->spec_nsteps = q.nsteps;
	}
	return MJB_OK;
}

// The lane = env kernel (mjb_lane_env.hip) for fused launches of a model whose topology is compiled in: one env per lane, no frame.
// Per-env model overrides (but mode 2), the device hwsim stage (but mjb_lane_env_set_hwsim), xfrc_applied (but mjb_lane_env_set_xfrc) and frame dumps
// keep the generic kernels.
// (mjb_lane_env_set_hwsim: the hwsim stage rides along in the kernel's HW build -- unless the batch has per-env gravity or parameter blocks too)
// (... or the model has activation states: no build of the kernel has both, mjb_lane_env_plan answers -1)
// (... or joint limits: the plain build alone has the constraint stage -- no overlay, hwsim or xfrc build of such a model, mjb_lane_env_plan answers -1)
// (... or joint equalities, or fixed tendons under its actuators: the same -- le_solo_only; le_limits: the model has rows, of either kind)
static bool le_limits(const mjb_batch *b) { return b->model->le_topo == MJB_LE_TOPO_JIT && mjb_lane_env_limits(&b->model->h) + mjb_lane_env_eq_rows(&b->model->h) > 0; }
static bool le_solo_only(const mjb_batch *b) { return b->model->le_topo == MJB_LE_TOPO_JIT && mjb_lane_env_solo_only(&b->model->h) != 0; }
static bool le_hwsim(const mjb_batch *b) { return b->hw.n > 0 && b->lane_env_hwsim && b->hw_le_ok && !b->env_mass.get() && !b->env_gravity.get() && b->model->h.na <= 0 && !le_solo_only(b); }
// (mjb_lane_env_set_xfrc: a written xfrc_applied rides along in the kernel's XF builds -- unless the batch has a hwsim stage, there is no build with both.
//  LaunchReq::compact stays what the generic path's frame choice reads; for this kernel, which has no frame, the xfrc term of it is lifted)
// (... or the model has a force / torque sensor on a body at rest: the wrench table has no slot for that body's xfrc_applied, mjb_lane_env_plan answers -1)
static bool le_xfrc(const mjb_batch *b) { return b->st.use_xfrc && b->lane_env_xfrc && b->hw.n == 0 && !mjb_lane_env_wrench_at_rest(&b->model->h) && !le_solo_only(b); }
static bool want_lane_env(const mjb_batch *b, const LaunchReq &q, int variant)
{
	const bool frameless = q.compact || (le_xfrc(b) && !b->st.keep_frame);
	// (a model with joint limits is a PGS model to the generic kernels: the lane = env kernel takes it when asked to, modes 1 and 2 -- the automatic mode
	//  keeps the generic kernels for it -- and without per-env overrides of any kind)
	// (... nor per-env equality parameters; a model with fixed tendons and no rows is an unconstrained model to the generic kernels, and treated alike)
	const bool lim = le_solo_only(b);
	if (!(q.mode == MJB_MODE_STEP && frameless && (lim ? ((le_limits(b) ? mjb_kv_pgs(variant) : variant == MJB_KV_NONE) && b->lane_env_mode >= 1 && !b->env_equality.get()) : variant == MJB_KV_NONE) &&
	      b->model->le_topo != MJB_LE_TOPO_NONE && !b->le_unavailable && b->lane_env_mode != 0 &&
	      (no_env_overrides(b) || (b->lane_env_mode == 2 && b->hw.n == 0 && !lim) || le_hwsim(b)) && !b->st.stats))  // (mode 2: per-env gravity and parameter blocks ride along, le_overlay_sync)
		return false;
	static const int min_envs = mjb_env_int("MJB_LANE_ENV_MIN_ENVS", 4096);
	return b->lane_env_mode >= 1 || q.env_hi - q.env_lo >= min_envs;  // (also the fused launch of a split step's non-callback envs, mjb_step_rest)
}

// an env's row of the host mirror of env_mass; NULL while the batch has no block, i.e. every env still runs on the model's values
static double *env_block_row(mjb_batch *b, int env)
{
	return b->env_mass ? b->env_block.data() + (size_t)env * mjb_env_block_layout(b->model->h).doubles : nullptr;
}

// Mode 2 of mjb_set_lane_env: the per-env overlay (DevState::le_overlay; PeSlots, mjb_lane_env_kernel.h) of a batch with per-env gravity or parameter
// blocks.  Built for every env at the first such launch; afterwards the columns of the envs a mjb_set_env_* call has touched (le_overlay_touch) are
// derived again ahead of the next launch.  Sources: env_gravity, the env's block of env_mass (its host mirror), else the model.
static void le_overlay_touch(mjb_batch *b, int env_lo, int env_hi)
{
	if (!b->le_overlay.get() || env_lo >= env_hi) return;
	const bool none = b->le_ov_lo >= b->le_ov_hi;
	b->le_ov_lo = none ? env_lo : std::min(b->le_ov_lo, env_lo);
	b->le_ov_hi = none ? env_hi : std::max(b->le_ov_hi, env_hi);
}
static int le_overlay_sync(mjb_batch *b)
{
	const mjb_model_desc &h = b->model->h;
	const int ns = mjb_lane_env_overlay_slots(&h), nenv = b->nenv;
	if (!b->le_overlay) {
		if (!b->le_overlay.alloc_zeroed((size_t)ns * nenv)) return fail(MJB_ENOMEM, "lane = env kernel: allocation of the per-env overlay failed");
		set_view(b, b->st.le_overlay, b->le_overlay.get());
		b->le_ov_lo = 0;
		b->le_ov_hi = nenv;
	}
	const int lo = b->le_ov_lo, hi = b->le_ov_hi, n = hi - lo;
	if (n <= 0) return MJB_OK;
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (an earlier launch may still read the columns)
	if (b->rest_pending && b->rest.stream.get()) HIP_TRY(hipStreamSynchronize(b->rest.stream.get()));
	std::vector<double> grav;
	if (b->env_gravity.get()) {
		grav.resize((size_t)3 * n);
		HIP_TRY(hipMemcpy(grav.data(), b->env_gravity.get() + (size_t)3 * lo, grav.size() * sizeof(double), hipMemcpyDeviceToHost));
	}
	std::vector<double> col((size_t)ns), stage((size_t)ns * n);
	for (int e = 0; e < n; e++) {
		mjb_lane_env_overlay_row(&h, grav.empty() ? nullptr : grav.data() + (size_t)3 * e, env_block_row(b, lo + e), col.data());
		for (int k = 0; k < ns; k++) stage[(size_t)k * n + e] = col[k];
	}
	// slot k of envs [lo, hi): n consecutive doubles at le_overlay + k * nenv + lo
	HIP_TRY(hipMemcpy2D(b->le_overlay.get() + lo, (size_t)nenv * sizeof(double), stage.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)ns,
	                    hipMemcpyHostToDevice));
	b->le_ov_lo = b->le_ov_hi = 0;
	return MJB_OK;
}

// mjb_lane_env_set_xfrc: the wrench table of the XF builds (DevState::le_xfrc; XfSlots, mjb_lane_env_kernel.h).  Allocated at the first such launch and
// filled from xfrc_applied by a transpose kernel on the launch's stream, again whenever the field has been written or reset since the last fill (the
// kernel itself keeps the two in step when it resets an env).
static int le_xfrc_sync(mjb_batch *b, hipStream_t stream)
{
	const mjb_model_desc &h = b->model->h;
	if (!b->le_xfrc) {
		if (!b->le_xfrc.alloc((size_t)6 * mjb_lane_env_xfrc_slots(&h) * b->nenv))  // (the fill below writes every entry)
			return fail(MJB_ENOMEM, "lane = env kernel: allocation of the xfrc_applied table failed");
		set_view(b, b->st.le_xfrc, b->le_xfrc.get());
		b->le_xfrc_stale = true;
	}
	if (!b->le_xfrc_stale) return MJB_OK;
	if (b->rest_pending && b->rest.stream.get() && b->rest.stream.get() != stream) HIP_TRY(hipStreamSynchronize(b->rest.stream.get()));  // (an earlier launch may still read the table)
	const int rc = mjb_lane_env_xfrc_fill(&h, b->st.xfrc_applied, b->le_xfrc.get(), b->nenv, stream);
	if (rc != 0) return fail(MJB_ENODEVICE, "lane = env kernel: xfrc_applied table fill failed: %s", hipGetErrorString((hipError_t)rc));
	b->le_xfrc_stale = false;
	return MJB_OK;
}

static int launch(mjb_batch *b, int mode, int nsteps, int env_lo = 0, int env_hi = -1, hipStream_t on = nullptr)
{
	if (env_hi < 0) env_hi = b->nenv;
	LaunchReq q = { mode, nsteps, env_lo, env_hi, on ? on : b->stream.get(), env_lo == 0 && env_hi == b->nenv, mode == MJB_MODE_STEP && !b->st.use_xfrc && !b->st.keep_frame };
	HIP_TRY(hipSetDevice(b->device));
	int variant, chunk, zhalf_now, rc;
	bool count_rows, use_split, zuse;
	if ((rc = frame_variant(b, q, &variant))) return rc;
	if ((rc = choose_fused_frame(b, q, variant, &count_rows))) return rc;
	if ((rc = choose_split_step(b, q, variant, &use_split))) return rc;
	b->split_used = use_split;
	{  // the kernels count rows (three atomics per env-step on one address) only in the launches whose counters are read
		unsigned long long *rs = count_rows ? b->rowstat_dev.get() : nullptr;
		if (b->st.rowstat != rs) set_view(b, b->st.rowstat, rs);
	}
	const bool le_per_env = b->lane_env_mode == 2 && (b->env_mass.get() || b->env_gravity.get()) && !use_split && want_lane_env(b, q, variant);
	if (le_per_env && (rc = le_overlay_sync(b))) return rc;
	const bool le_xf = le_xfrc(b) && !use_split && want_lane_env(b, q, variant);
	if (le_xf && (rc = le_xfrc_sync(b, q.stream))) return rc;
	if (!b->le_con && le_limits(b) && !use_split && want_lane_env(b, q, variant)) {  // what the kernel leaves of its constraint stage: allocated at the first such launch
		if (!b->le_con.alloc_zeroed((size_t)b->nenv * (size_t)(b->model->h.nv + 2))) return fail(MJB_ENOMEM, "lane = env kernel: allocation of the constraint stage's output failed");
		b->params_dirty = true;  // (KernelParams::le_con: sync_params reads the owner)
	}
	if ((rc = sync_params(b))) return rc;
	if (use_split) {
		if (b->zvalid) {  // (the pre-generated ctrl-noise buffer names an older launch: this path draws its normals in the smooth kernel)
			HIP_TRY(hipMemsetAsync(b->zinfo.get(), 0xff, 8 * sizeof(unsigned int), q.stream));
			b->zvalid = false;
		}
		b->lane_env_used = false;
		b->le_con_valid = false;
		b->noise_mode = 0;
		return launch_split(b, nsteps, env_lo, env_hi, q.stream);
	}
	variant = pgs_build(b, q, variant);
	chunk = 0;
	if (!(le_limits(b) && want_lane_env(b, q, variant)) && (rc = choose_chunk(b, q, variant, &chunk))) return rc;  // (a limit model on the lane = env kernel: no work queue)
	if ((rc = stage_ctrl_noise(b, q, variant, &zuse, &zhalf_now))) return rc;
	const bool zspec = zuse && b->zdouble;
	if (zspec) HIP_TRY(hipEventRecord(b->noise.go.get(), q.stream));  // (everything before this launch -- the last reader of the other half -- is done)
	if (count_rows) HIP_TRY(hipMemsetAsync(b->rowstat_dev.get(), 0, 4 * sizeof(unsigned long long), q.stream));
	bool use_le = want_lane_env(b, q, variant);
	b->lane_env_used = use_le;
	if (use_le) {
		rc = mjb_launch_lane_env(b->params_dev.get(), b->model->le_topo, &b->model->h, b->nenv, env_lo, env_hi, nsteps, b->step_counter, q.stream,
		                         le_xf ? (le_per_env ? MJB_LE_OVERLAY_XFRC : MJB_LE_XFRC) : le_per_env ? MJB_LE_OVERLAY : (b->hw.n > 0 ? MJB_LE_HWSIM : MJB_LE_PLAIN));
		if (rc == MJB_LE_UNAVAILABLE) {  // (no hiprtc / no kernel header / compile error: remembered, the generic kernel runs -- mjb_lane_env_info says why)
			b->le_unavailable = true;
			b->lane_env_used = use_le = false;
		}
	}
	b->le_con_valid = use_le && q.whole && le_limits(b);
	if (!use_le) {
		const StepLaunch a = { b->params_dev.get(), q.compact ? (b->wide ? &b->model->Lw : &b->model->Lc) : &b->L, env_lo, env_hi, mode, nsteps, b->step_counter,
			                   b->lanes, b->epb, variant, chunk, dense_build(b, mode), q.stream };
		rc = mjb_launch_step(a);
	}
	if (rc != 0) return fail(MJB_ENODEVICE, "kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
	if (count_rows) {  // this launch's row counters, to pinned host memory behind it
		HIP_TRY(hipMemcpyAsync(b->rowstat_host.get(), b->rowstat_dev.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, q.stream));
		HIP_TRY(hipEventRecord(b->ev_rowstat.get(), q.stream));
		b->rowstat_pending = true;
	}
	if (zspec) return speculate_ctrl_noise(b, q, zhalf_now);
	return MJB_OK;
}

int mjb_step(mjb_batch *b, int nsteps)
{
	if (!b || nsteps < 0) return fail(MJB_EINVAL, "mjb_step: bad argument");
	if (nsteps == 0) return MJB_OK;
	int jrc = join_rest(b);
	if (jrc) return jrc;
	b->split_ncb = -1;  // (an open split step is abandoned)
	// Kernel variant 4 with a wide fused frame: a long launch on a workload nobody has looked at yet (a new batch, after mjb_reset or a new
	// qpos) starts with a short PROBE launch that counts this state's rows, and picks its frame from that -- the first rollout of a
	// high-contact batch used to run on the default frame (r05: 1461 ms against 288 ms in steady state).  A launch cut in two is the same
	// rollout (the state crosses HBM between launches exactly as between the chunks of one).
	int rc = MJB_OK;
	if (nsteps >= 100 && b->rowstat_dev.get() && b->model->has_wide && !b->rowstat_ever && !b->rowstat_pending && !b->st.use_xfrc && !b->st.keep_frame) {
		const int probe = 4;
		b->probe_now = true;
		rc = launch(b, MJB_MODE_STEP, probe);
		b->probe_now = false;
		if (rc != MJB_OK) return rc;
		b->step_counter += (unsigned int)probe;
		b->steps_taken += (unsigned long long)probe;
		nsteps -= probe;
		b->decide_now = b->rowstat_pending;
	}
	rc = launch(b, MJB_MODE_STEP, nsteps);
	b->decide_now = false;
	if (rc == MJB_OK) {
		b->step_counter += (unsigned int)nsteps;
		b->steps_taken += (unsigned long long)nsteps;
		b->frame_valid = b->st.keep_frame != 0;
		b->frame_half = false;
		b->frame_hi = b->nenv;
		b->pose_written = false;
		b->vel_written = false;
		b->vel_integrated = true;
	}
	return rc;
}

int mjb_set_keep_frame(mjb_batch *b, int on)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (on) {
		int rc = ensure_ws(b);
		if (rc) return rc;
	}
	if ((b->st.keep_frame != 0) != (on != 0)) {
		b->st.keep_frame = on ? 1 : 0;
		b->params_dirty = true;
		b->frame_valid = false;
	}
	return MJB_OK;
}

// a forward pass of the whole batch on the full frame: all of it (mjb_forward) or a step's first half (mjb_step1)
static int forward_whole(mjb_batch *b, int mode)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (int rc = ensure_ws(b)) return rc;
	if (int rc = join_rest(b)) return rc;
	int rc = launch(b, mode, 1);
	if (rc == MJB_OK) {
		b->frame_valid = true;
		b->frame_half = mode == MJB_MODE_STEP1;
		b->frame_hi = b->nenv;
		b->pose_written = false;
		b->vel_written = false;
		b->vel_integrated = false;
	}
	return rc;
}

int mjb_step1(mjb_batch *b) { return forward_whole(b, MJB_MODE_STEP1); }

int mjb_step2(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (!b->frame_valid || !b->st.frame_ws || b->frame_hi < b->nenv) return fail(MJB_EINVAL, "mjb_step2 without a preceding mjb_step1");
	int rc = launch(b, MJB_MODE_STEP2, 1);
	if (rc == MJB_OK) {
		b->step_counter += 1;
		b->steps_taken += 1;
		b->frame_half = false;
		b->vel_integrated = true;
	}
	return rc;
}

// ---- split step for a PREFIX of the batch (the host runtime's callback envs): envs [0, ncb) are stepped in two halves around
// the control-callback point, envs [ncb, nenv) take the SAME step as one fused launch (same Philox step counter, same results as
// a whole-batch launch: every env's arithmetic is independent of which launch carries it).  Order of calls for one step:
//   mjb_step1_prefix(ncb) -> [copy the callback envs' fields out] -> mjb_step_rest(ncb) -> [host callbacks run while it executes]
//   -> [copy their writes back] -> mjb_step2_prefix(ncb)   (advances the step counter)
int mjb_step1_prefix(mjb_batch *b, int ncb)
{
	if (!b || ncb < 0 || ncb > b->nenv) return fail(MJB_EINVAL, "mjb_step1_prefix: bad argument");
	// A split step abandoned AFTER mjb_step_rest: the rest envs already took a step the step counter never recorded (they would redraw
	// the same Philox step), and their launch may still be running on the rest stream.  Only mjb_step2_prefix / mjb_step21_prefix /
	// mjb_step2_rk_prefix (finish it) or mjb_reset / mjb_step (abandon it, whole batch) may follow; a split abandoned BEFORE
	// mjb_step_rest is simply restarted here.
	if (b->split_ncb >= 0 && b->split_rest_done && b->split_ncb < b->nenv)
		return fail(MJB_EINVAL, "mjb_step1_prefix: a split step of prefix %d is still open and its other envs already took the step "
		                        "(finish it with mjb_step2_prefix, or abandon it with mjb_reset / mjb_step)", b->split_ncb);
	int rc = join_rest(b);
	if (rc) return rc;
	rc = ensure_ws(b);
	if (rc) return rc;
	b->split_ncb = ncb;
	b->split_rest_done = false;
	if (ncb == 0) return MJB_OK;
	rc = launch(b, MJB_MODE_STEP1, 1, 0, ncb);
	if (rc == MJB_OK) {
		b->frame_valid = true;
		b->frame_half = true;
		b->frame_hi = ncb;
		b->pose_written = false;
		b->vel_written = false;
		b->vel_integrated = false;
	}
	return rc;
}

int mjb_step_rest(mjb_batch *b, int ncb)
{
	if (!b || ncb != b->split_ncb) return fail(MJB_EINVAL, "mjb_step_rest: not inside a split step of this prefix (mjb_step1_prefix first)");
	if (b->split_rest_done) return fail(MJB_EINVAL, "mjb_step_rest: called twice in one split step");
	b->split_rest_done = true;
	if (ncb >= b->nenv) return MJB_OK;
	// on its own stream, forked from the batch's stream here and joined in mjb_step2_prefix: the two groups of envs are independent,
	// so the callback envs' second half does not queue behind this launch
	HIP_TRY(hipSetDevice(b->device));
	if (!b->rest.stream) {
		if (int crc = b->rest.create()) return crc;
	}
	int prc = sync_params(b);  // (uploads, if any, on the batch's stream BEFORE the fork)
	if (prc) return prc;
	HIP_TRY(hipEventRecord(b->rest.fork.get(), b->stream.get()));
	HIP_TRY(hipStreamWaitEvent(b->rest.stream.get(), b->rest.fork.get(), 0));
	int rc = launch(b, MJB_MODE_STEP, 1, ncb, b->nenv, b->rest.stream.get());
	HIP_TRY(hipEventRecord(b->rest.join.get(), b->rest.stream.get()));
	b->rest_pending = true;
	return rc;
}

// What the closers of a prefix step share.  Before their launch: a caller that skipped mjb_step_rest -- the rest must not miss the step;
// and the prefix's first half must have left its frames (who: the function the user called)
static int prefix_second_half(mjb_batch *b, int ncb, const char *who)
{
	int rc = MJB_OK;
	if (!b->split_rest_done) rc = mjb_step_rest(b, ncb);
	if (rc != MJB_OK) return rc;
	if (ncb > 0 && (!b->frame_valid || !b->st.frame_ws || b->frame_hi < ncb)) return fail(MJB_EINVAL, "%s without a preceding mjb_step1_prefix", who);
	return MJB_OK;
}

// ... and behind it (rc: the launch's result): join -- whatever follows on the batch's stream sees the rest's step too --, then the step is counted
static int prefix_step_done(mjb_batch *b, int rc)
{
	if (int jrc = join_rest(b)) return jrc;
	if (rc == MJB_OK) {
		b->step_counter += 1;
		b->steps_taken += 1;
	}
	return rc;
}

int mjb_step2_prefix(mjb_batch *b, int ncb)
{
	if (!b || ncb != b->split_ncb) return fail(MJB_EINVAL, "mjb_step2_prefix without the matching mjb_step1_prefix");
	int rc = prefix_second_half(b, ncb, "mjb_step2_prefix");
	if (rc != MJB_OK) return rc;
	if (ncb > 0) rc = launch(b, MJB_MODE_STEP2, 1, 0, ncb);
	rc = prefix_step_done(b, rc);
	if (rc == MJB_OK) {
		b->split_ncb = -1;
		b->frame_half = false;
		b->vel_integrated = true;
	}
	return rc;
}

int mjb_step21_prefix(mjb_batch *b, int ncb)
{
	if (!b || ncb != b->split_ncb) return fail(MJB_EINVAL, "mjb_step21_prefix without the matching mjb_step1_prefix");
	int rc = prefix_second_half(b, ncb, "mjb_step21_prefix");
	if (rc != MJB_OK) return rc;
	// (trip 1 of the launch -- the next step's first half -- draws its ctrl noise at step_counter + 1, as mjb_step1_prefix would
	//  after mjb_step2_prefix advanced the counter)
	if (ncb > 0) rc = launch(b, MJB_MODE_STEP21, 1, 0, ncb);
	rc = prefix_step_done(b, rc);
	if (rc == MJB_OK) {
		b->split_ncb = ncb;  // ... and the next split step is open: its first half has run
		b->split_rest_done = false;
		b->frame_valid = true;
		b->frame_half = true;
		b->frame_hi = ncb;
		b->pose_written = false;
		b->vel_written = false;
		b->vel_integrated = false;
	}
	return rc;
}

// ---- the second half of an RK4 step cut at the callback points of its four evaluations (mj_RungeKutta runs mj_forwardSkip, and with
// it mjcb_passive / mjcb_control, once per evaluation: plugin_utils.h:119-125 is why lastStageCallback exists).  After
// mjb_step1_prefix (evaluation 0's first half) and the host's callbacks:  rk = 0, 1, 2 finishes evaluation rk, folds it into the
// weighted sums, sets the state of evaluation rk + 1 and runs ITS first half -- the host's callbacks then see that evaluation's view
// (time = t0 + c h); rk = 3 finishes evaluation 3, advances the state and closes the step like mjb_step2_prefix.  The envs beyond
// the prefix take the whole RK4 step as one fused launch (mjb_step_rest, issued with rk = 0 if the caller did not).
int mjb_step2_rk_prefix(mjb_batch *b, int ncb, int rk)
{
	if (!b || ncb != b->split_ncb || rk < 0 || rk > 3) return fail(MJB_EINVAL, "mjb_step2_rk_prefix without the matching mjb_step1_prefix, or evaluation index outside 0..3");
	if (b->model->h.integrator != MJB_INT_RK4) return fail(MJB_EINVAL, "mjb_step2_rk_prefix: the model's integrator is not RK4");
	int rc = prefix_second_half(b, ncb, "mjb_step2_rk_prefix");
	if (rc != MJB_OK) return rc;
	if (ncb > 0) rc = launch(b, rk == 3 ? MJB_MODE_RKLAST : MJB_MODE_RKMID, rk, 0, ncb);  // (the evaluation index travels as the kernel's nsteps)
	if (rc != MJB_OK || rk < 3) return rc;  // (rk < 3 ends in the first half of the next evaluation: frame_half stays)
	rc = prefix_step_done(b, rc);
	if (rc == MJB_OK) {
		b->split_ncb = -1;
		b->frame_half = false;
		b->vel_integrated = true;
	}
	return rc;
}

int mjb_forward(mjb_batch *b) { return forward_whole(b, MJB_MODE_FORWARD); }

int mjb_reset(mjb_batch *b, const uint8_t *mask)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	HIP_TRY(hipSetDevice(b->device));
	const unsigned char *md = nullptr;
	if (mask) {
		if (!b->mask_dev && !b->mask_dev.alloc((size_t)b->nenv)) return fail(MJB_ENOMEM, "mjb_reset: mask allocation failed");  // (the copy below writes all of it)
		HIP_TRY(hipMemcpyAsync(b->mask_dev.get(), mask, (size_t)b->nenv, hipMemcpyHostToDevice, b->stream.get()));
		md = b->mask_dev.get();
	}
	int prc = join_rest(b);
	if (prc) return prc;
	b->split_ncb = -1;  // (an open split step is abandoned: mjb_step1_prefix starts the next one)
	prc = sync_params(b);
	if (prc) return prc;
	int rc = mjb_launch_reset(b->params_dev.get(), b->nenv, md, b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "reset launch failed: %s", hipGetErrorString((hipError_t)rc));
	if (mask) HIP_TRY(hipStreamSynchronize(b->stream.get()));
	b->frame_valid = false;
	b->le_con_valid = false;
	b->le_xfrc_stale = true;  // (mj_resetData zeroes xfrc_applied)
	if (!mask) b->rowstat_ever = false;  // (a new workload: the next long launch probes its rows first)
	return MJB_OK;
}

static double *state_ptr(mjb_batch *b, int field)
{
	switch (field) {
#define MJB_DS(name, rows, cols) case MJB_F_##name: return b->st.name;
#define MJB_DD(name, rows, cols)
#define MJB_DD2(name, rows, cols)
#define MJB_DI(name, rows, cols)
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
	default: return nullptr;
	}
}

static int frame_offset(const mjb_batch *b, int field) { return field_slot(b->L, field); }

static int check_range(mjb_batch *b, int field, int lo, int hi)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (field < 0 || field >= MJB_F_COUNT) return fail(MJB_EINVAL, "bad field id %d", field);
	if (lo < 0 || hi > b->nenv || lo > hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", lo, hi, b->nenv);
	return MJB_OK;
}

int mjb_get(mjb_batch *b, int field, int env_lo, int env_hi, double *host)
{
	int rc = check_range(b, field, env_lo, env_hi);
	if (rc) return rc;
	if (kFields[field].kind == 3) return fail(MJB_EINVAL, "field %s is an int field; use mjb_get_int", kFields[field].name);
	const int n = b->model->field_size[field];
	if (n == 0 || env_lo == env_hi) return MJB_OK;
	if (!host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (kFields[field].kind == 0) {
		double *p = state_ptr(b, field);
		HIP_TRY(hipMemcpy(host, p + (size_t)env_lo * n, (size_t)(env_hi - env_lo) * n * sizeof(double),
		                  hipMemcpyDeviceToHost));
		return MJB_OK;
	}
	if (b->le_con_valid && !b->frame_valid && !strcmp(kFields[field].name, "qfrc_constraint")) {  // (what the lane = env kernel left of a limit model's last step)
		const size_t ld = (size_t)b->model->h.nv + 2;
		HIP_TRY(hipMemcpy2D(host, (size_t)n * sizeof(double), b->le_con.get() + (size_t)env_lo * ld, ld * sizeof(double), (size_t)n * sizeof(double), (size_t)(env_hi - env_lo),
		                    hipMemcpyDeviceToHost));
		return MJB_OK;
	}
	if (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi)
		return fail(MJB_EINVAL, "derived field %s is only readable after mjb_forward / mjb_step1 / mjb_step2",
		            kFields[field].name);
	const int off = frame_offset(b, field);
	HIP_TRY(hipMemcpy2D(host, (size_t)n * sizeof(double), b->st.frame_ws + (size_t)env_lo * b->st.frame_stride + off,
	                    (size_t)b->st.frame_stride * sizeof(double), (size_t)n * sizeof(double),
	                    (size_t)(env_hi - env_lo), hipMemcpyDeviceToHost));
	return MJB_OK;
}

int mjb_get_int(mjb_batch *b, int field, int env_lo, int env_hi, int *host)
{
	int rc = check_range(b, field, env_lo, env_hi);
	if (rc) return rc;
	if (kFields[field].kind != 3) return fail(MJB_EINVAL, "field %s is not an int field", kFields[field].name);
	const int n = b->model->field_size[field];
	if (n == 0 || env_lo == env_hi) return MJB_OK;
	if (!host) return fail(MJB_EINVAL, "null host buffer");
	if (b->le_con_valid && !b->frame_valid && (!strcmp(kFields[field].name, "nefc") || !strcmp(kFields[field].name, "solver_iter"))) {  // (the lane = env kernel keeps the two counts as doubles)
		const size_t ld = (size_t)b->model->h.nv + 2, nrow = (size_t)(env_hi - env_lo);
		std::vector<double> v(nrow);
		HIP_TRY(hipSetDevice(b->device));
		HIP_TRY(hipStreamSynchronize(b->stream.get()));
		HIP_TRY(hipMemcpy2D(v.data(), sizeof(double), b->le_con.get() + (size_t)env_lo * ld + (size_t)b->model->h.nv + (strcmp(kFields[field].name, "nefc") ? 1 : 0), ld * sizeof(double),
		                    sizeof(double), nrow, hipMemcpyDeviceToHost));
		for (size_t e = 0; e < nrow; e++) host[e] = (int)v[e];
		return MJB_OK;
	}
	if (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi)
		return fail(MJB_EINVAL, "int field %s is only readable after mjb_forward / mjb_step1 / mjb_step2",
		            kFields[field].name);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const int off = frame_offset(b, field);
	const int *base = reinterpret_cast<const int *>(b->st.frame_ws + (size_t)env_lo * b->st.frame_stride + b->L.ndouble) + off;
	HIP_TRY(hipMemcpy2D(host, (size_t)n * sizeof(int), base, (size_t)b->st.frame_stride * sizeof(double),
	                    (size_t)n * sizeof(int), (size_t)(env_hi - env_lo), hipMemcpyDeviceToHost));
	return MJB_OK;
}

int mjb_set(mjb_batch *b, int field, int env_lo, int env_hi, const double *host)
{
	int rc = check_range(b, field, env_lo, env_hi);
	if (rc) return rc;
	const int n = b->model->field_size[field];
	if (n == 0 || env_lo == env_hi) return MJB_OK;
	if (!host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (kFields[field].kind == 0) {
		double *p = state_ptr(b, field);
		HIP_TRY(hipMemcpy(p + (size_t)env_lo * n, host, (size_t)(env_hi - env_lo) * n * sizeof(double),
		                  hipMemcpyHostToDevice));
		if (field == MJB_F_xfrc_applied) b->le_xfrc_stale = true;
		if (field == MJB_F_xfrc_applied && !b->st.use_xfrc) {
			b->st.use_xfrc = 1;
			b->params_dirty = true;
		}
		if (field == MJB_F_qpos && env_lo == 0 && env_hi == b->nenv) b->rowstat_ever = false;  // (wide-frame policy: a new workload)
		if (pose_field(field)) b->pose_written = true;
		if (field == MJB_F_qvel) b->vel_written = true;
		return MJB_OK;
	}
	if (field != MJB_F_qfrc_passive)
		return fail(MJB_EINVAL, "field %s is derived and cannot be set (only state fields and qfrc_passive can)",
		            kFields[field].name);
	if (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi)
		return fail(MJB_EINVAL, "qfrc_passive can only be modified between mjb_step1 and mjb_step2");
	const int off = frame_offset(b, field);
	HIP_TRY(hipMemcpy2D(b->st.frame_ws + (size_t)env_lo * b->st.frame_stride + off,
	                    (size_t)b->st.frame_stride * sizeof(double), host, (size_t)n * sizeof(double),
	                    (size_t)n * sizeof(double), (size_t)(env_hi - env_lo), hipMemcpyHostToDevice));
	return MJB_OK;
}

int mjb_register_collision(mjb_batch *b, int geom_type1, int geom_type2, int func)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	auto known = [](int t) { return t == MJB_GEOM_PLANE || t == MJB_GEOM_SPHERE || t == MJB_GEOM_CAPSULE || t == MJB_GEOM_BOX; };
	if (!known(geom_type1) || !known(geom_type2)) return fail(MJB_EINVAL, "mjb_register_collision: geom types must be plane / sphere / capsule / box");
	if (func < MJB_COLFUNC_DEFAULT || func > MJB_COLFUNC_SPHERES) return fail(MJB_EINVAL, "mjb_register_collision: unknown function %d", func);
	const mjb_model *M = b->model;
	const int np = M->h.ncollpair;
	if (np == 0) return MJB_OK;
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const int lo = geom_type1 < geom_type2 ? geom_type1 : geom_type2, hi = geom_type1 < geom_type2 ? geom_type2 : geom_type1;
	if (b->st.colfunc[8 * lo + hi] != func) {  // the table by current types (read when per-env geom types are in play)
		b->st.colfunc[8 * lo + hi] = func;
		b->params_dirty = true;
	}
	for (int p = 0; p < np; p++) {  // (pairs are stored with type1 <= type2)
		if (M->pair_i[8 * p + 2] != lo || M->pair_i[8 * p + 3] != hi) continue;
		HIP_TRY(hipMemcpy(b->pair_i_dev + 8 * p + 6, &func, sizeof(int), hipMemcpyHostToDevice));
	}
	return MJB_OK;
}

int mjb_get_many(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, double *const *host)
{
	if (!b || n < 0 || (n && (!fields || !host))) return fail(MJB_EINVAL, "mjb_get_many: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	// every argument is checked BEFORE the first copy is enqueued: a refusal never leaves transfers in flight
	for (int k = 0; k < n; k++) {
		const int field = fields[k];
		int rc = check_range(b, field, env_lo, env_hi);
		if (rc) return rc;
		if (kFields[field].kind == 3) return fail(MJB_EINVAL, "field %s is an int field; use mjb_get_int", kFields[field].name);
		if (b->model->field_size[field] == 0 || env_lo == env_hi) continue;
		if (!host[k]) return fail(MJB_EINVAL, "null host buffer");
		if (kFields[field].kind != 0 && (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi))
			return fail(MJB_EINVAL, "derived field %s is only readable after mjb_forward / mjb_step1 / mjb_step2", kFields[field].name);
	}
	hipError_t err = hipSuccess;
	for (int k = 0; k < n && err == hipSuccess; k++) {
		const int field = fields[k], sz = b->model->field_size[field];
		if (sz == 0 || env_lo == env_hi) continue;
		if (kFields[field].kind == 0)
			err = hipMemcpyAsync(host[k], state_ptr(b, field) + (size_t)env_lo * sz, (size_t)(env_hi - env_lo) * sz * sizeof(double),
			                     hipMemcpyDeviceToHost, b->stream.get());
		else
			err = hipMemcpy2DAsync(host[k], (size_t)sz * sizeof(double), b->st.frame_ws + (size_t)env_lo * b->st.frame_stride + frame_offset(b, field),
			                       (size_t)b->st.frame_stride * sizeof(double), (size_t)sz * sizeof(double), (size_t)(env_hi - env_lo),
			                       hipMemcpyDeviceToHost, b->stream.get());
	}
	const hipError_t serr = hipStreamSynchronize(b->stream.get());  // (also after a failed enqueue: the copies before it are drained)
	if (err != hipSuccess) return fail(MJB_ENODEVICE, "mjb_get_many: %s", hipGetErrorString(err));
	if (serr != hipSuccess) return fail(MJB_ENODEVICE, "mjb_get_many: %s", hipGetErrorString(serr));
	return MJB_OK;
}

// (asynchronous on the batch's stream: the host buffers must stay untouched until the next synchronising call -- mjb_synchronize,
//  mjb_get*, a blocking mjb_step; page-locked buffers make these true DMA transfers.  MujocoEnv::commitData synchronises.)
int mjb_set_many(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, const double *const *host)
{
	if (!b || n < 0 || (n && (!fields || !host))) return fail(MJB_EINVAL, "mjb_set_many: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	for (int k = 0; k < n; k++) {
		const int field = fields[k];
		int rc = check_range(b, field, env_lo, env_hi);
		if (rc) return rc;
		if (b->model->field_size[field] == 0 || env_lo == env_hi) continue;
		if (!host[k]) return fail(MJB_EINVAL, "null host buffer");
		if (kFields[field].kind != 0) {
			if (field != MJB_F_qfrc_passive)
				return fail(MJB_EINVAL, "field %s is derived and cannot be set (only state fields and qfrc_passive can)", kFields[field].name);
			if (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi) return fail(MJB_EINVAL, "qfrc_passive can only be modified between mjb_step1 and mjb_step2");
		}
	}
	hipError_t err = hipSuccess;
	for (int k = 0; k < n && err == hipSuccess; k++) {
		const int field = fields[k], sz = b->model->field_size[field];
		if (sz == 0 || env_lo == env_hi) continue;
		if (kFields[field].kind == 0) {
			err = hipMemcpyAsync(state_ptr(b, field) + (size_t)env_lo * sz, host[k], (size_t)(env_hi - env_lo) * sz * sizeof(double),
			                     hipMemcpyHostToDevice, b->stream.get());
			if (pose_field(field)) b->pose_written = true;
			if (field == MJB_F_qvel) b->vel_written = true;
			if (field == MJB_F_xfrc_applied) b->le_xfrc_stale = true;
			if (field == MJB_F_xfrc_applied && !b->st.use_xfrc) {
				b->st.use_xfrc = 1;
				b->params_dirty = true;
			}
		} else {
			err = hipMemcpy2DAsync(b->st.frame_ws + (size_t)env_lo * b->st.frame_stride + frame_offset(b, field),
			                       (size_t)b->st.frame_stride * sizeof(double), host[k], (size_t)sz * sizeof(double), (size_t)sz * sizeof(double),
			                       (size_t)(env_hi - env_lo), hipMemcpyHostToDevice, b->stream.get());
		}
	}
	if (err != hipSuccess) {
		hipStreamSynchronize(b->stream.get());  // drain what was enqueued before the failure
		return fail(MJB_ENODEVICE, "mjb_set_many: %s", hipGetErrorString(err));
	}
	return MJB_OK;
}

// ---- several fields in ONE transfer --------------------------------------------------------------------------------------
// A callback round of the host runtime moves ~25 fields of the callback envs to the host and ~8 back (mujoco_env.cpp stepBurst);
// one hipMemcpy(2D)Async per field is ~8 us of driver time each, 350 us per split step against ~50 us of kernels
// (profiles/r02_callback_path.txt).  Here a small kernel gathers the fields into one device block laid out field after field
// ([env][dim] each, in the order given) and ONE copy moves the block; the reverse for the writes.
namespace {
struct PackDesc {
	double *src;       // env-major source: state array, or the frame workspace + the field's offset
	long long stride;  // doubles from one env to the next in the source
	int dim;           // doubles per env
	long long dst;     // offset of the field's block inside the packed block
};
struct PackArgs {
	PackDesc d[40];
	int n, nenv;
};
__global__ void mjb_pack_kernel(PackArgs a, double *block, int env_lo, int unpack)
{
	const int f = blockIdx.y;
	if (f >= a.n) return;
	const PackDesc d = a.d[f];
	const long long total = (long long)a.nenv * d.dim;
	for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
		const long long e = t / d.dim, k = t - e * d.dim;
		double *s = d.src + (env_lo + e) * d.stride + k;
		if (unpack) *s = block[d.dst + t];
		else block[d.dst + t] = *s;
	}
}
}  // namespace

static int packed_transfer(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, double *host_block, bool to_host, const char *who)
{
	if (!b || n < 0 || n > 40 || (n && (!fields || !host_block))) return fail(MJB_EINVAL, "%s: bad argument (at most 40 fields)", who);
	HIP_TRY(hipSetDevice(b->device));
	PackArgs a{};
	long long total = 0;
	int maxdim = 1;
	bool writes_pose = false, writes_vel = false;
	for (int k = 0; k < n; k++) {
		const int field = fields[k];
		int rc = check_range(b, field, env_lo, env_hi);
		if (rc) return rc;
		if (kFields[field].kind == 3) return fail(MJB_EINVAL, "%s: field %s is an int field", who, kFields[field].name);
		const int sz = b->model->field_size[field];
		PackDesc &d = a.d[a.n];
		if (kFields[field].kind == 0) {
			d.src = state_ptr(b, field);
			d.stride = sz;
		} else {
			if (!to_host && field != MJB_F_qfrc_passive)
				return fail(MJB_EINVAL, "field %s is derived and cannot be set (only state fields and qfrc_passive can)", kFields[field].name);
			if (!b->frame_valid || !b->st.frame_ws || env_hi > b->frame_hi)
				return fail(MJB_EINVAL, "derived field %s is only accessible after mjb_forward / mjb_step1 / mjb_step2", kFields[field].name);
			d.src = b->st.frame_ws + frame_offset(b, field);
			d.stride = b->st.frame_stride;
		}
		d.dim = sz;
		d.dst = total;
		total += (long long)(env_hi - env_lo) * sz;
		if (sz > 0) a.n++;
		if (sz > maxdim) maxdim = sz;
		if (!to_host && sz > 0 && pose_field(field)) writes_pose = true;
		if (!to_host && sz > 0 && field == MJB_F_qvel) writes_vel = true;
		if (!to_host && field == MJB_F_xfrc_applied) b->le_xfrc_stale = true;
		if (!to_host && field == MJB_F_xfrc_applied && !b->st.use_xfrc) {
			b->st.use_xfrc = 1;
			b->params_dirty = true;
		}
	}
	if (total == 0 || env_lo == env_hi) return MJB_OK;
	if (writes_pose) b->pose_written = true;  // (every field has been checked: the write goes ahead)
	if (writes_vel) b->vel_written = true;
	a.nenv = env_hi - env_lo;
	if ((long long)b->pack_cap < total) {
		if (!b->pack_dev.alloc_zeroed((size_t)total)) {
			b->pack_cap = 0;
			return fail(MJB_ENOMEM, "%s: staging allocation failed", who);
		}
		b->pack_cap = (size_t)total;
	}
	const int threads = 256;
	int bx = (int)std::min<long long>(((long long)a.nenv * maxdim + threads - 1) / threads, 64);
	if (bx < 1) bx = 1;
	if (!to_host)
		HIP_TRY(hipMemcpyAsync(b->pack_dev.get(), host_block, (size_t)total * sizeof(double), hipMemcpyHostToDevice, b->stream.get()));
	hipLaunchKernelGGL(mjb_pack_kernel, dim3(bx, a.n), dim3(threads), 0, b->stream.get(), a, b->pack_dev.get(), env_lo, to_host ? 0 : 1);
	HIP_TRY(hipGetLastError());
	if (to_host) {
		HIP_TRY(hipMemcpyAsync(host_block, b->pack_dev.get(), (size_t)total * sizeof(double), hipMemcpyDeviceToHost, b->stream.get()));
		HIP_TRY(hipStreamSynchronize(b->stream.get()));
	}
	return MJB_OK;
}

int mjb_get_packed(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, double *host_block)
{
	return packed_transfer(b, n, fields, env_lo, env_hi, host_block, true, "mjb_get_packed");
}

int mjb_set_packed(mjb_batch *b, int n, const int *fields, int env_lo, int env_hi, const double *host_block)
{
	return packed_transfer(b, n, fields, env_lo, env_hi, const_cast<double *>(host_block), false, "mjb_set_packed");
}

int mjb_host_register(void *host, unsigned long long bytes)
{
	if (!host || !bytes) return fail(MJB_EINVAL, "mjb_host_register: bad argument");
	if (hipHostRegister(host, (size_t)bytes, hipHostRegisterPortable)  /* every device of a sharded batch may DMA from it */ != hipSuccess) {
		(void)hipGetLastError();
		return fail(MJB_ENODEVICE, "hipHostRegister failed");
	}
	return MJB_OK;
}

int mjb_host_unregister(void *host)
{
	if (!host) return MJB_OK;
	if (hipHostUnregister(host) != hipSuccess) (void)hipGetLastError();
	return MJB_OK;
}

void *mjb_device_ptr(mjb_batch *b, int field)
{
	if (!b || field < 0 || field >= MJB_F_COUNT || kFields[field].kind != 0) {
		fail(MJB_EINVAL, "mjb_device_ptr: not a state field");
		return nullptr;
	}
	return state_ptr(b, field);
}

int mjb_set_ctrl_noise(mjb_batch *b, double ctrl_noise_std, double ctrl_noise_rate, uint64_t seed, int64_t env_offset)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (ctrl_noise_std < 0) return fail(MJB_EINVAL, "ctrl_noise_std must be >= 0");
	const double dt = b->model->h.timestep[0];
	const double rate = std::exp(-dt / std::fmax(ctrl_noise_rate, 1e-15));
	b->nz.rate = rate;
	b->nz.scale = ctrl_noise_std * std::sqrt(1 - rate * rate);
	b->nz.seed = seed;
	b->nz.env_offset = env_offset;
	b->nz.enabled = ctrl_noise_std > 0;
	b->params_dirty = true;
	if (b->zinfo.get()) {  // normals generated under the old key (also the ones a side-stream generator is still writing) are void
		HIP_TRY(hipSetDevice(b->device));
		if (b->noise.stream.get()) HIP_TRY(hipStreamSynchronize(b->noise.stream.get()));
		HIP_TRY(hipStreamSynchronize(b->stream.get()));
		HIP_TRY(hipMemset(b->zinfo.get(), 0xff, 8 * sizeof(unsigned int)));
		b->spec_valid = false;
		b->zvalid = false;
	}
	return MJB_OK;
}

int mjb_set_stats(mjb_batch *b, int on)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	HIP_TRY(hipSetDevice(b->device));
	int rc = join_rest(b);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (on) {
		if (!b->stats_dev && !b->stats_dev.alloc_zeroed(MJB_NSTATS)) return fail(MJB_ENOMEM, "mjb_set_stats: allocation failed");
		HIP_TRY(hipMemset(b->stats_dev.get(), 0, MJB_NSTATS * sizeof(unsigned long long)));
	}
	set_view(b, b->st.stats, on ? b->stats_dev.get() : nullptr);
	return MJB_OK;
}

int mjb_get_stats(mjb_batch *b, unsigned long long *out)
{
	if (!b || !out) return fail(MJB_EINVAL, "mjb_get_stats: bad argument");
	if (!b->stats_dev.get()) return fail(MJB_EINVAL, "mjb_get_stats before mjb_set_stats(b, 1)");
	HIP_TRY(hipSetDevice(b->device));
	int rc = join_rest(b);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	HIP_TRY(hipMemcpy(out, b->stats_dev.get(), MJB_NSTATS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return MJB_OK;
}

int mjb_noise_mode(const mjb_batch *b) { return b ? b->noise_mode : 0; }
int mjb_set_lane_env(mjb_batch *b, int mode)
{
	if (!b || mode < -1 || mode > 2) return fail(MJB_EINVAL, "mjb_set_lane_env: bad argument");
	b->lane_env_mode = mode;
	return MJB_OK;
}
int mjb_lane_env_set_hwsim(mjb_batch *b, int on)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	b->lane_env_hwsim = on != 0;
	return MJB_OK;
}
int mjb_lane_env_set_xfrc(mjb_batch *b, int on)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	b->lane_env_xfrc = on != 0;
	return MJB_OK;
}
int mjb_set_sensors_every_step(mjb_batch *b, int on)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if ((b->st.sens_every_step != 0) != (on != 0)) {
		b->st.sens_every_step = on ? 1 : 0;
		b->params_dirty = true;
	}
	return MJB_OK;
}
int mjb_set_split_step(mjb_batch *b, int mode)
{
	if (!b || mode < -1 || mode > 1) return fail(MJB_EINVAL, "mjb_set_split_step: bad argument");
	b->split_mode = mode;
	return MJB_OK;
}
int mjb_split_step_info(const mjb_batch *b, int *used_last, int *slices)
{
	if (used_last) *used_last = b && b->split_used ? 1 : 0;
	if (slices) *slices = b ? b->split_slices_last : 0;
	return b ? b->model->sm_topo : -1;
}
const char *mjb_lane_env_error(void) { return mjb_lane_env_jit_error(); }
void mjb_lane_env_jit_counts(int *compiled, int *disk_hits) { mjb_lane_env_jit_stats(compiled, disk_hits); }
int mjb_lane_env_plan(const mjb_model *m, int ncu, int nenv, int build, int form, int sweep_waves, int lds_kb, int *out_form, int *out_sweep_waves, int *out_lds_kb)
{
	if (m && m->le_topo == MJB_LE_TOPO_NONE) return -1;
	return mjb_lane_env_plan_for(m && m->le_topo == MJB_LE_TOPO_JIT ? &m->h : nullptr, ncu, nenv, build, form, sweep_waves, lds_kb, out_form, out_sweep_waves, out_lds_kb);
}
int mjb_lane_env_rows(const mjb_model *m, int *neq_rows, int *nlimit_rows)
{
	const bool rows = m && m->le_topo == MJB_LE_TOPO_JIT;
	const int ne = rows ? mjb_lane_env_eq_rows(&m->h) : 0, nl = rows ? mjb_lane_env_limits(&m->h) : 0;
	if (neq_rows) *neq_rows = ne;
	if (nlimit_rows) *nlimit_rows = nl;
	return ne + nl;
}
int mjb_lane_env_info(const mjb_batch *b, int *used_last)
{
	if (used_last) *used_last = b && b->lane_env_used ? 1 : 0;
	return b ? (b->le_unavailable ? -3 : b->model->le_topo) : -1;
}
int mjb_fused_frame(const mjb_batch *b) { return b && b->wide ? 2 : 1; }

void *mjb_get_stream(mjb_batch *b) { return b ? (void *)b->stream.get() : nullptr; }

int mjb_set_stream(mjb_batch *b, void *hip_stream)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	HIP_TRY(hipSetDevice(b->device));
	if (b->stream) HIP_TRY(hipStreamSynchronize(b->stream.get()));
	b->stream.borrow((hipStream_t)hip_stream);  // (a stream of the batch's own is destroyed)
	return MJB_OK;
}

int mjb_synchronize(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	return MJB_OK;
}

int mjb_debug_profile(mjb_batch *b, unsigned long long *out64, int clear)
{
	if (!b || !out64) return fail(MJB_EINVAL, "mjb_debug_profile: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	HIP_TRY(hipMemcpy(out64, b->st.prof, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	if (clear) HIP_TRY(hipMemset(b->st.prof, 0, 64 * sizeof(unsigned long long)));
	return MJB_OK;
}

int mjb_debug_profile_window(mjb_batch *b, int first_id)
{
	if (!b || first_id < 0 || first_id > 31) return fail(MJB_EINVAL, "mjb_debug_profile_window: bad argument");
	if (b->st.prof_base != first_id) {
		b->st.prof_base = first_id;
		b->params_dirty = true;
	}
	return MJB_OK;
}

int mjb_warning(mjb_batch *b, int which, unsigned long long *count)
{
	if (!b || !count || which < 0 || which >= MJB_NWARNING) return fail(MJB_EINVAL, "mjb_warning: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	HIP_TRY(hipMemcpy(count, b->st.nwarn + which, sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return MJB_OK;
}

int mjb_warning_count(mjb_batch *b, unsigned long long *count)
{
	if (!b || !count) return fail(MJB_EINVAL, "mjb_warning_count: bad argument");
	unsigned long long w[MJB_NWARNING];
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	HIP_TRY(hipMemcpy(w, b->st.nwarn, sizeof w, hipMemcpyDeviceToHost));
	*count = w[MJB_WARN_BADQPOS] + w[MJB_WARN_BADQVEL] + w[MJB_WARN_BADQACC];
	return MJB_OK;
}

}  // extern "C"

// ---- aggregate metrics (mjb_metrics): one workgroup reduces the state arrays of the batch ----
__global__ void mjb_metrics_kernel(const double *qacc, const double *qvel, const double *time, const double *energy,
                                   const unsigned long long *nwarn, int nenv, int nv, double env_steps, double *out)
{
	__shared__ double red[4][256];
	double mq = 0, mv = 0, mt = 0, pe = 0, ke = 0;
	for (size_t k = threadIdx.x; k < (size_t)nenv * nv; k += blockDim.x) {
		mq = fmax(mq, fabs(qacc[k]));
		mv = fmax(mv, fabs(qvel[k]));
	}
	for (int e = threadIdx.x; e < nenv; e += blockDim.x) {
		mt = fmax(mt, time[e]);
		pe += energy[2 * e];
		ke += energy[2 * e + 1];
	}
	// (fmax drops NaNs: an env that went non-finite inside a launch has been reset before the state was stored)
	double v[5] = { mq, mv, mt, pe, ke };
	double res[5];
	for (int q = 0; q < 5; q++) {
		red[0][threadIdx.x] = v[q];
		__syncthreads();
		for (int s = blockDim.x / 2; s > 0; s >>= 1) {
			if ((int)threadIdx.x < s)
				red[0][threadIdx.x] = q < 3 ? fmax(red[0][threadIdx.x], red[0][threadIdx.x + s]) : red[0][threadIdx.x] + red[0][threadIdx.x + s];
			__syncthreads();
		}
		res[q] = red[0][0];
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		out[0] = env_steps;
		out[1] = (double)(nwarn[MJB_WARN_BADQPOS] + nwarn[MJB_WARN_BADQVEL] + nwarn[MJB_WARN_BADQACC]);
		out[2] = (double)nwarn[MJB_WARN_CONTACTFULL];
		out[3] = (double)nwarn[MJB_WARN_CNSTRFULL];
		out[4] = res[3];
		out[5] = res[4];
		out[6] = (double)nenv;
		out[7] = 0;
		out[8] = res[0];
		out[9] = res[1];
		out[10] = res[2];
		for (int k = 11; k < 16; k++) out[k] = 0;
	}
}

// one per-env override array of the mjb_set_env_* setters below that need no mj_setConst
template <typename T>
static int env_param(mjb_batch *b, DevBuf<T> &arr, const T *&view, int per_env, const T *model_vals, int env_lo, int env_hi, const T *vals, const char *what)
{
	if (!b || !vals) return fail(MJB_EINVAL, "%s: bad argument", what);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "%s: bad env range", what);
	if (per_env <= 0) return fail(MJB_EINVAL, "%s: the model has nothing to override", what);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (!arr) {  // first use: every env starts from the model's values (uploaded for every env: no zeroing)
		DevBuf<T> dev;
		if (!dev.alloc((size_t)b->nenv * per_env)) return fail(MJB_ENOMEM, "%s: allocation failed", what);
		std::vector<T> init((size_t)b->nenv * per_env);
		for (int e = 0; e < b->nenv; e++) memcpy(init.data() + (size_t)e * per_env, model_vals, (size_t)per_env * sizeof(T));
		HIP_TRY(hipMemcpy(dev.get(), init.data(), init.size() * sizeof(T), hipMemcpyHostToDevice));
		arr = std::move(dev);
		set_view(b, view, arr.get());
	}
	HIP_TRY(hipMemcpy(arr.get() + (size_t)env_lo * per_env, vals, (size_t)(env_hi - env_lo) * per_env * sizeof(T), hipMemcpyHostToDevice));
	return MJB_OK;
}

extern "C" {

void *mjb_metrics_device(mjb_batch *b)
{
	if (!b) {
		fail(MJB_EINVAL, "null batch");
		return nullptr;
	}
	if (hipSetDevice(b->device) != hipSuccess) return nullptr;
	if (!b->metrics_dev) {
		if (!b->metrics_dev.alloc_zeroed(16)) {
			fail(MJB_ENOMEM, "mjb_metrics: allocation failed");
			return nullptr;
		}
	}
	hipLaunchKernelGGL(mjb_metrics_kernel, dim3(1), dim3(256), 0, b->stream.get(), b->st.qacc, b->st.qvel, b->st.time, b->st.energy,
	                   b->st.nwarn, b->nenv, b->model->h.nv, (double)b->nenv * (double)b->steps_taken, b->metrics_dev.get());
	if (hipGetLastError() != hipSuccess) {
		fail(MJB_ENODEVICE, "mjb_metrics: launch failed");
		return nullptr;
	}
	return b->metrics_dev.get();
}

int mjb_metrics(mjb_batch *b, double *out16)
{
	if (!b || !out16) return fail(MJB_EINVAL, "mjb_metrics: bad argument");
	void *p = mjb_metrics_device(b);
	if (!p) return MJB_ENODEVICE;
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	HIP_TRY(hipMemcpy(out16, p, 16 * sizeof(double), hipMemcpyDeviceToHost));
	return MJB_OK;
}

// ---- per-env model parameters (the subset that needs no mj_setConst) ----
int mjb_set_env_gravity(mjb_batch *b, int env_lo, int env_hi, const double *gravity)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const int rc = env_param(b, b->env_gravity, b->st.env_gravity, 3, b->model->h.gravity, env_lo, env_hi, gravity, "mjb_set_env_gravity");
	if (rc == MJB_OK) le_overlay_touch(b, env_lo, env_hi);
	return rc;
}

int mjb_set_env_geom_friction(mjb_batch *b, int env_lo, int env_hi, const double *friction)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	return env_param(b, b->env_geom_friction, b->st.env_geom_friction, h.nconmax > 0 ? 3 * h.ngeom : 0, h.geom_friction, env_lo,
	                 env_hi, friction, "mjb_set_env_geom_friction");
}

int mjb_set_env_geom_size(mjb_batch *b, int env_lo, int env_hi, const double *size)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	return env_param(b, b->env_geom_size, b->st.env_geom_size, h.nconmax > 0 ? 3 * h.ngeom : 0, h.geom_size, env_lo, env_hi, size,
	                 "mjb_set_env_geom_size");
}

int mjb_set_env_geom_type(mjb_batch *b, int env_lo, int env_hi, const int *type)
{
	if (!b) return fail(MJB_EINVAL, "mjb_set_env_geom_type: bad argument");
	const mjb_model_desc &h = b->model->h;
	const int per_env = h.nconmax > 0 ? h.ngeom : 0;
	if (type && env_lo >= 0 && env_hi <= b->nenv && env_lo <= env_hi)  // (any other call is env_param's to refuse)
		for (size_t k = 0; k < (size_t)(env_hi - env_lo) * per_env; k++)
			if (type[k] != MJB_GEOM_PLANE && type[k] != MJB_GEOM_SPHERE && type[k] != MJB_GEOM_CAPSULE && type[k] != MJB_GEOM_BOX &&
			    type[k] != 4 && type[k] != 5)  // (mjGEOM_ELLIPSOID / mjGEOM_CYLINDER are accepted as "no pair function": the geom yields no contacts)
				return fail(MJB_EUNSUPPORTED, "mjb_set_env_geom_type: geom type %d is neither a primitive of the engine nor ellipsoid / cylinder", type[k]);
	return env_param(b, b->env_geom_type, b->st.env_geom_type, per_env, h.geom_type, env_lo, env_hi, type, "mjb_set_env_geom_type");
}

int mjb_set_env_equality(mjb_batch *b, int env_lo, int env_hi, const double *params)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	std::vector<double> packed((size_t)19 * (h.neq > 0 ? h.neq : 1));
	for (int q = 0; q < h.neq; q++) {
		double *o = packed.data() + 19 * q;
		o[0] = h.eq_active[q] ? 1.0 : 0.0;
		for (int k = 0; k < 11; k++) o[1 + k] = h.eq_data[11 * q + k];
		for (int k = 0; k < 2; k++) o[12 + k] = h.eq_solref[2 * q + k];
		for (int k = 0; k < 5; k++) o[14 + k] = h.eq_solimp[5 * q + k];
	}
	return env_param(b, b->env_equality, b->st.env_equality, 19 * h.neq, packed.data(), env_lo, env_hi, params, "mjb_set_env_equality");
}

// The env's block of inertial, joint and actuator constants (DevState::env_mass, laid out by EnvBlockLayout, mjb_dev.h): one allocation, and its
// host mirror b->env_block from the same moment on.  The first override of either family fills every env's block with the model's values; a setter
// then edits its rows in the mirror (env_block_row) and uploads them.

// what the integrator adds to M's diagonal per unit of h, from an env's damping and bias parameters: mjb_compile's rule (damp_int)
static void env_damping_int(const mjb_model_desc &h, const double *damping, const double *biasprm, double *out)
{
	for (int i = 0; i < h.nv; i++) out[i] = damping[i];
	if (h.integrator != MJB_INT_IMPLICITFAST) return;
	for (int i = 0; i < h.nv; i++) out[i] = (h.disableflags & MJB_DSBL_PASSIVE) ? 0.0 : damping[i];
	if (h.disableflags & MJB_DSBL_ACTUATION) return;
	for (int i = 0; i < h.nu; i++) {
		if (h.actuator_trntype[i] != MJB_TRN_JOINT) continue;  // (site / tendon actuators: a velocity term is refused)
		const double bv = h.actuator_biastype[i] == MJB_BIAS_AFFINE ? biasprm[3 * i + 2] : 0.0, g = h.actuator_gear[6 * i];
		out[h.jnt_dofadr[h.actuator_trnid[2 * i]]] -= g * g * bv;
	}
}

static int env_block_ensure(mjb_batch *b, const char *what)
{
	if (b->env_mass) return MJB_OK;
	const mjb_model_desc &h = b->model->h;
	const EnvBlockLayout B = mjb_env_block_layout(h);
	const struct { int off; const double *src; int n; } sections[] = {
		{ B.body_mass, h.body_mass, h.nbody }, { B.body_subtreemass, h.body_subtreemass, h.nbody }, { B.body_inertia, h.body_inertia, 3 * h.nbody },
		{ B.dof_invweight0, h.dof_invweight0, h.nv }, { B.body_invweight0, h.body_invweight0, 2 * h.nbody }, { B.tendon_invweight0, h.tendon_invweight0, h.ntendon },
		{ B.meaninertia, h.meaninertia, 1 }, { B.dof_damping, h.dof_damping, h.nv }, { B.dof_armature, h.dof_armature, h.nv },
		{ B.dof_frictionloss, h.dof_frictionloss, h.nv }, { B.dof_damping_int, b->model->damp_int.data(), h.nv }, { B.jnt_stiffness, h.jnt_stiffness, h.njnt },
		{ B.actuator_gainprm, h.actuator_gainprm, 3 * h.nu }, { B.actuator_biasprm, h.actuator_biasprm, 3 * h.nu },
	};
	std::vector<double> row((size_t)B.doubles), init((size_t)b->nenv * B.doubles);
	for (const auto &s : sections) std::copy_n(s.src, s.n, row.data() + s.off);
	for (int e = 0; e < b->nenv; e++) memcpy(init.data() + (size_t)e * B.doubles, row.data(), (size_t)B.doubles * sizeof(double));
	DevBuf<double> dev;
	if (!dev.alloc(init.size())) return fail(MJB_ENOMEM, "%s: allocation failed", what);  // (uploaded for every env)
	if (hipMemcpy(dev.get(), init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(MJB_ENODEVICE, "%s: upload failed", what);
	b->env_mass = std::move(dev);
	b->env_block = std::move(init);
	set_view(b, b->st.env_mass, b->env_mass.get());
	return MJB_OK;
}

static int env_block_upload(mjb_batch *b, int env_lo, int env_hi)
{
	const size_t stride = (size_t)mjb_env_block_layout(b->model->h).doubles;
	HIP_TRY(hipMemcpy(b->env_mass.get() + (size_t)env_lo * stride, b->env_block.data() + (size_t)env_lo * stride, (size_t)(env_hi - env_lo) * stride * sizeof(double),
	                  hipMemcpyHostToDevice));
	le_overlay_touch(b, env_lo, env_hi);
	return MJB_OK;
}

int mjb_set_env_mass_params(mjb_batch *b, int env_lo, int env_hi, const double *params)
{
	const char *what = "mjb_set_env_mass_params";
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (!params) return fail(MJB_EINVAL, "%s: bad argument", what);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "%s: bad env range", what);
	const EnvBlockLayout B = mjb_env_block_layout(b->model->h);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const int rc = env_block_ensure(b, what);
	if (rc != MJB_OK) return rc;
	for (int e = env_lo; e < env_hi; e++) memcpy(env_block_row(b, e), params + (size_t)(e - env_lo) * B.mass_doubles, (size_t)B.mass_doubles * sizeof(double));
	if (env_hi > env_lo)  // the mass section of each env's row: rows of mass_doubles into rows of the block's stride
		HIP_TRY(hipMemcpy2D(b->env_mass.get() + (size_t)env_lo * B.doubles, (size_t)B.doubles * sizeof(double), params, (size_t)B.mass_doubles * sizeof(double),
		                    (size_t)B.mass_doubles * sizeof(double), (size_t)(env_hi - env_lo), hipMemcpyHostToDevice));
	le_overlay_touch(b, env_lo, env_hi);
	return MJB_OK;
}

int mjb_set_env_body_mass(mjb_batch *b, int env_lo, int env_hi, const double *body_mass, const double *body_inertia)
{
	if (!b || !body_mass) return fail(MJB_EINVAL, "mjb_set_env_body_mass: bad argument");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "mjb_set_env_body_mass: bad env range");
	const mjb_model_desc &h = b->model->h;
	const EnvBlockLayout B = mjb_env_block_layout(h);
	const int stride = B.mass_doubles, n = env_hi - env_lo;
	std::vector<double> packed((size_t)std::max(1, n) * stride);
	// (the derivation is mj_setConst -- Jacobians of every body, an O(nbody nv^2) mass matrix and its inverse -- and a service call that
	//  sets one mass on the whole batch, setBodyStateCB with the default env range, hands over nenv identical rows under the physics
	//  mutex: derived once per DISTINCT row, the block of a row equal to its predecessor is copied)
	// (an env that carries its own armature, mjb_set_env_dof_params, is derived with it: its row of the mirror has it)
	auto arm = [&](int e) { return b->env_mass ? env_block_row(b, env_lo + e) + B.dof_armature : h.dof_armature; };
	for (int e = 0; e < n; e++) {
		const double *bm = body_mass + (size_t)e * h.nbody, *bi = body_inertia ? body_inertia + (size_t)e * 3 * h.nbody : nullptr;
		double *dst = packed.data() + (size_t)e * stride;
		if (e > 0 && std::memcmp(bm, bm - h.nbody, sizeof(double) * h.nbody) == 0 &&
		    (!bi || std::memcmp(bi, bi - 3 * h.nbody, sizeof(double) * 3 * h.nbody) == 0) &&
		    (arm(e) == arm(e - 1) || std::memcmp(arm(e), arm(e - 1), sizeof(double) * h.nv) == 0)) {
			std::memcpy(dst, dst - stride, sizeof(double) * stride);
			continue;
		}
		const int rc = mjb_derive_mass_params_armature(b->model, bm, bi, arm(e), dst);
		if (rc != MJB_OK) return rc;
	}
	return mjb_set_env_mass_params(b, env_lo, env_hi, packed.data());
}

// ---- per-env joint and actuator parameters ----
// One implementation behind the four setters: every array is optional and comes with its own per-env stride (the packed form hands
// over six views of one block).  Everything is checked before anything is written: a refused call leaves the batch as it was.
static int env_joint_set(mjb_batch *b, int env_lo, int env_hi, const double *damping, const double *armature, const double *frictionloss,
                         const double *stiffness, const double *gainprm, const double *biasprm, int src_stride, const char *what)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (!damping && !armature && !frictionloss && !stiffness && !gainprm && !biasprm) return fail(MJB_EINVAL, "%s: bad argument", what);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "%s: bad env range", what);
	const mjb_model *M = b->model;
	const mjb_model_desc &h = M->h;
	const EnvBlockLayout B = mjb_env_block_layout(h);
	if (B.doubles == B.mass_doubles) return fail(MJB_EINVAL, "%s: the model has nothing to override", what);
	const int n = env_hi - env_lo;
	// a packed block (src_stride > 0) or a dense [env][len] array per argument
	auto at = [&](const double *p, int e, int len) { return p + (size_t)e * (src_stride > 0 ? src_stride : len); };
	auto nonneg = [&](const double *p, int len, const char *name, const char *unit) -> int {
		if (!p) return MJB_OK;
		for (int e = 0; e < n; e++)
			for (int i = 0; i < len; i++) {
				const double v = at(p, e, len)[i];
				if (!std::isfinite(v) || v < 0)
					return fail(MJB_EINVAL, "%s: %s of env %d, %s %d is %g: it must be finite and non-negative", what, name, env_lo + e, unit, i, v);
			}
		return MJB_OK;
	};
	int rc;
	if ((rc = nonneg(damping, h.nv, "damping", "dof")) != MJB_OK) return rc;
	if ((rc = nonneg(armature, h.nv, "armature", "dof")) != MJB_OK) return rc;
	if ((rc = nonneg(frictionloss, h.nv, "frictionloss", "dof")) != MJB_OK) return rc;
	if ((rc = nonneg(stiffness, h.njnt, "stiffness", "joint")) != MJB_OK) return rc;
	for (const double *p : { gainprm, biasprm })
		if (p)
			for (int e = 0; e < n; e++)
				for (int k = 0; k < 3 * h.nu; k++)
					if (!std::isfinite(at(p, e, 3 * h.nu)[k]))
						return fail(MJB_EINVAL, "%s: %s of env %d, actuator %d is not finite", what, p == gainprm ? "gainprm" : "biasprm", env_lo + e, k / 3);
	// (FRICTIONLOSS disabled: no friction rows by the model's own choice, any value is inert)
	if (frictionloss && M->nfriction == 0 && !(h.disableflags & MJB_DSBL_FRICTIONLOSS))
		for (int e = 0; e < n; e++)
			for (int i = 0; i < h.nv; i++)
				if (at(frictionloss, e, h.nv)[i] > 0)
					return fail(MJB_EUNSUPPORTED, "%s: positive frictionloss (env %d, dof %d) on a model compiled without dry-friction rows: give one joint of the "
					                              "model a positive frictionloss so that its frames hold them", what, env_lo + e, i);
	if (h.integrator == MJB_INT_IMPLICITFAST) {
		if (gainprm)
			for (int e = 0; e < n; e++)
				for (int i = 0; i < h.nu; i++)
					if (h.actuator_gaintype[i] == MJB_GAIN_AFFINE && at(gainprm, e, 3 * h.nu)[3 * i + 2] != 0)
						return fail(MJB_EUNSUPPORTED, "%s: integrator implicitfast with a velocity term in an affine actuator gain is not supported (env %d, actuator %d)",
						            what, env_lo + e, i);
		if (biasprm)
			for (int e = 0; e < n; e++)
				for (int i = 0; i < h.nu; i++) {
					const int trn = h.actuator_trntype[i];
					if ((trn == MJB_TRN_SITE || trn == MJB_TRN_TENDON) && h.actuator_biastype[i] == MJB_BIAS_AFFINE && at(biasprm, e, 3 * h.nu)[3 * i + 2] != 0)
						return fail(MJB_EUNSUPPORTED, "%s: integrator implicitfast with a velocity-dependent actuator on a %s is not supported (env %d, actuator %d)",
						            what, trn == MJB_TRN_SITE ? "site" : "tendon", env_lo + e, i);
				}
	}
	// the model's frames hold M + h B and its factor only when mjb_compile found something to put there (DevModel::eulerdamp)
	const bool euler_implicit = h.integrator == MJB_INT_EULER && !(h.disableflags & MJB_DSBL_EULERDAMP);
	if (M->eulerdamp == 0 && (euler_implicit || h.integrator == MJB_INT_IMPLICITFAST) && (damping || biasprm)) {
		std::vector<double> di((size_t)std::max(1, h.nv));
		for (int e = 0; e < n; e++) {
			const double *cur = env_block_row(b, env_lo + e);  // (no block yet: the model's values)
			const double *d = damping ? at(damping, e, h.nv) : (cur ? cur + B.dof_damping : h.dof_damping);
			const double *bp = biasprm ? at(biasprm, e, 3 * h.nu) : (cur ? cur + B.actuator_biasprm : h.actuator_biasprm);
			env_damping_int(h, d, bp, di.data());
			for (int i = 0; i < h.nv; i++)
				if (di[i] != 0)
					return fail(MJB_EUNSUPPORTED, "%s: %s (env %d, dof %d) on a model compiled without the implicit-damping factor (no damped dof: its frames hold no "
					                              "M + h B): give one joint of the model a positive damping", what,
					            euler_implicit ? "positive damping under the Euler integrator" : "a velocity-dependent force under implicitfast", env_lo + e, i);
		}
	}
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if ((rc = env_block_ensure(b, what)) != MJB_OK) return rc;
	std::vector<double> saved;  // (a failed derivation -- a singular inertia -- restores the rows)
	if (armature) saved.assign(b->env_block.begin() + (size_t)env_lo * B.doubles, b->env_block.begin() + (size_t)env_hi * B.doubles);
	for (int e = 0; e < n; e++) {
		double *row = env_block_row(b, env_lo + e);
		if (damping) memcpy(row + B.dof_damping, at(damping, e, h.nv), sizeof(double) * h.nv);
		if (armature) memcpy(row + B.dof_armature, at(armature, e, h.nv), sizeof(double) * h.nv);
		if (frictionloss) memcpy(row + B.dof_frictionloss, at(frictionloss, e, h.nv), sizeof(double) * h.nv);
		if (stiffness) memcpy(row + B.jnt_stiffness, at(stiffness, e, h.njnt), sizeof(double) * h.njnt);
		if (gainprm) memcpy(row + B.actuator_gainprm, at(gainprm, e, 3 * h.nu), sizeof(double) * 3 * h.nu);
		if (biasprm) memcpy(row + B.actuator_biasprm, at(biasprm, e, 3 * h.nu), sizeof(double) * 3 * h.nu);
		if (damping || biasprm) env_damping_int(h, row + B.dof_damping, row + B.actuator_biasprm, row + B.dof_damping_int);
		if (armature) {
			// mj_setConst with the env's own masses, inertias and armature (derived once per distinct row, as mjb_set_env_body_mass does)
			const double *prev = e > 0 ? row - B.doubles : nullptr;
			if (prev && std::memcmp(row + B.body_mass, prev + B.body_mass, sizeof(double) * h.nbody) == 0 &&
			    std::memcmp(row + B.body_inertia, prev + B.body_inertia, sizeof(double) * 3 * h.nbody) == 0 &&
			    std::memcmp(row + B.dof_armature, prev + B.dof_armature, sizeof(double) * h.nv) == 0) {
				memcpy(row, prev, sizeof(double) * B.mass_doubles);
				continue;
			}
			const std::vector<double> mass(row + B.body_mass, row + B.body_mass + h.nbody), inertia(row + B.body_inertia, row + B.body_inertia + 3 * h.nbody);
			rc = mjb_derive_mass_params_armature(M, mass.data(), inertia.data(), row + B.dof_armature, row);
			if (rc != MJB_OK) {
				std::copy(saved.begin(), saved.end(), b->env_block.begin() + (size_t)env_lo * B.doubles);
				return rc;
			}
		}
	}
	return env_block_upload(b, env_lo, env_hi);
}

int mjb_set_env_dof_params(mjb_batch *b, int env_lo, int env_hi, const double *damping, const double *armature, const double *frictionloss)
{
	return env_joint_set(b, env_lo, env_hi, damping, armature, frictionloss, nullptr, nullptr, nullptr, 0, "mjb_set_env_dof_params");
}

int mjb_set_env_joint_stiffness(mjb_batch *b, int env_lo, int env_hi, const double *stiffness)
{
	return env_joint_set(b, env_lo, env_hi, nullptr, nullptr, nullptr, stiffness, nullptr, nullptr, 0, "mjb_set_env_joint_stiffness");
}

int mjb_set_env_actuator_params(mjb_batch *b, int env_lo, int env_hi, const double *gainprm, const double *biasprm)
{
	return env_joint_set(b, env_lo, env_hi, nullptr, nullptr, nullptr, nullptr, gainprm, biasprm, 0, "mjb_set_env_actuator_params");
}

int mjb_set_env_joint_params(mjb_batch *b, int env_lo, int env_hi, const double *params)
{
	if (!b || !params) return fail(MJB_EINVAL, "mjb_set_env_joint_params: bad argument");
	const mjb_model_desc &h = b->model->h;
	const EnvBlockLayout B = mjb_env_block_layout(h);
	// the block's section at `off`, n entries: where the packed form has it, NULL when the model has none
	auto view = [&](int off, int n) { return n ? params + mjb_env_joint_packed(B, off) : nullptr; };
	return env_joint_set(b, env_lo, env_hi, view(B.dof_damping, h.nv), view(B.dof_armature, h.nv), view(B.dof_frictionloss, h.nv), view(B.jnt_stiffness, h.njnt),
	                     view(B.actuator_gainprm, h.nu), view(B.actuator_biasprm, h.nu), mjb_env_joint_packed(B, B.doubles), "mjb_set_env_joint_params");
}

// ---- device-side DefaultRobotHWSim::writeSim (stage hwsim_write in mjb_step.hip) ----
int mjb_hwsim_configure(mjb_batch *b, int n, const mjb_hwsim_joint *joints)
{
	if (!b || n < 0 || (n > 0 && !joints)) return fail(MJB_EINVAL, "mjb_hwsim_configure: bad argument");
	const mjb_model_desc &h = b->model->h;
	for (int k = 0; k < n; k++) {
		const mjb_hwsim_joint &j = joints[k];
		if (j.joint < 0 || j.joint >= h.njnt || h.jnt_type[j.joint] < MJB_JNT_SLIDE)
			return fail(MJB_EINVAL, "mjb_hwsim_configure: entry %d: joint %d is not a hinge / slide joint of the model", k, j.joint);
		if (j.method < MJB_HW_EFFORT || j.method > MJB_HW_VELOCITY_PID || j.kind < MJB_HW_REVOLUTE || j.kind > MJB_HW_PRISMATIC)
			return fail(MJB_EINVAL, "mjb_hwsim_configure: entry %d: bad control method / joint kind", k);
	}
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	b->hwb = HwSimBufs{};
	set_view(b, b->hw, HwSim{});
	b->hw_le_ok = false;
	if (n == 0) return MJB_OK;
	// (behind the [n] arrays: the same entries by dof for the lane = env kernel, HwSim::le_tab / le_gains; a dof two entries claim has no such table)
	const int nv = h.nv;
	std::vector<int> ints((size_t)4 * n + (size_t)4 * nv, 0);
	std::vector<double> gains((size_t)8 * n + (size_t)8 * nv, 0.0);
	for (int d = 0; d < nv; d++) ints[(size_t)4 * n + 4 * d] = -1;
	b->hw_le_ok = true;
	for (int k = 0; k < n; k++) {
		const mjb_hwsim_joint &j = joints[k];
		ints[k] = j.joint; ints[n + k] = j.method; ints[2 * n + k] = j.kind; ints[3 * n + k] = j.antiwindup ? 1 : 0;
		const double g[8] = { j.p, j.i, j.d, j.i_max, j.i_min, j.effort_limit, j.lower, j.upper };
		for (int q = 0; q < 8; q++) gains[(size_t)8 * k + q] = g[q];
		int *t = ints.data() + (size_t)4 * n + 4 * h.jnt_dofadr[j.joint];
		if (t[0] >= 0) b->hw_le_ok = false;
		t[0] = k; t[1] = j.method; t[2] = j.kind; t[3] = j.antiwindup ? 1 : 0;
		for (int q = 0; q < 8; q++) gains[(size_t)8 * n + (size_t)8 * h.jnt_dofadr[j.joint] + q] = g[q];
	}
	const size_t per = (size_t)b->nenv * n;
	HwSimBufs &B = b->hwb;
	if (!B.ints.alloc(ints.size()) || !B.gains.alloc(gains.size()) /* (both uploaded whole) */ || !B.cmd.alloc_zeroed(4 * per) || !B.pid.alloc_zeroed(2 * per)) {
		B = HwSimBufs{};
		return fail(MJB_ENOMEM, "mjb_hwsim_configure: allocation failed");
	}
	HIP_TRY(hipMemcpy(B.ints.get(), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(B.gains.get(), gains.data(), gains.size() * sizeof(double), hipMemcpyHostToDevice));
	HwSim hw{};
	hw.n = n;
	hw.joint = B.ints.get(); hw.method = B.ints.get() + n; hw.kind = B.ints.get() + 2 * n; hw.antiwindup = B.ints.get() + 3 * n;
	hw.gains = B.gains.get();
	hw.le_tab = (mjb_ciptr)(B.ints.get() + 4 * n);
	hw.le_gains = (mjb_cdptr)(B.gains.get() + (size_t)8 * n);
	hw.cmd_pos = B.cmd.get(); hw.cmd_vel = B.cmd.get() + per; hw.cmd_eff = B.cmd.get() + 2 * per; hw.cmd_hold = B.cmd.get() + 3 * per;
	hw.pid = B.pid.get();
	set_view(b, b->hw, hw);
	return MJB_OK;
}

int mjb_hwsim_set_command(mjb_batch *b, int which, int env_lo, int env_hi, const double *cmd)
{
	if (!b || !cmd || which < 0 || which > 2) return fail(MJB_EINVAL, "mjb_hwsim_set_command: bad argument");
	if (b->hw.n <= 0) return fail(MJB_EINVAL, "mjb_hwsim_set_command before mjb_hwsim_configure");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "mjb_hwsim_set_command: bad env range");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const size_t per = (size_t)b->nenv * b->hw.n;
	HIP_TRY(hipMemcpy(b->hwb.cmd.get() + which * per + (size_t)env_lo * b->hw.n, cmd, (size_t)(env_hi - env_lo) * b->hw.n * sizeof(double),
	                  hipMemcpyHostToDevice));
	return MJB_OK;
}

void *mjb_hwsim_command_ptr(mjb_batch *b, int which)
{
	if (!b || which < 0 || which > 2 || b->hw.n <= 0) return nullptr;
	return b->hwb.cmd.get() + (size_t)which * b->nenv * b->hw.n;
}

// MujocoRosControlPlugin::controlCallback's cadence (mujoco_ros_control_plugin.cpp:153-194) for the device-side stage: with a control
// period the joint state the PIDs see is the one sampled at the last controller update (readSim, every control_period of sim
// time; first at the first non-zero time), writeSim runs at every step after it with period = time - last write, and nothing is
// read or written at t = 0.  control_period <= 0 switches back to a write at every step on the step's own state.
int mjb_hwsim_set_period(mjb_batch *b, double control_period)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->hw.n <= 0) return fail(MJB_EINVAL, "mjb_hwsim_set_period before mjb_hwsim_configure");
	// (a period below the timestep is accepted with a warning, as the reference's load() does, :100-105 -- ROS_WARN and carry on: the
	//  cadence test `sim_period >= control_period` then holds at every step, i.e. the controller updates every step)
	if (control_period > 0 && control_period < b->model->h.timestep[0])
		fprintf(stderr, "mjb_hwsim_set_period: desired controller update period (%g s) is faster than the simulation timestep (%g s)\n",
		        control_period, b->model->h.timestep[0]);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const int n = b->hw.n;
	if (control_period > 0) {
		const size_t per = 2 + 2 * (size_t)n;
		std::vector<double> init((size_t)b->nenv * per, 0.0);
		for (int e = 0; e < b->nenv; e++)
			for (int k = 0; k < n; k++) init[(size_t)e * per + 2 + k] = 1.0;  // joint_position_ starts at 1.0 (default_robot_hw_sim.cpp:129)
		if (!b->hwb.cad && !b->hwb.cad.alloc(init.size())) return fail(MJB_ENOMEM, "mjb_hwsim_set_period: allocation failed");  // (uploaded whole below)
		HIP_TRY(hipMemcpy(b->hwb.cad.get(), init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
		const double sec = std::floor(control_period);
		b->hw.period_ns = (long long)sec * 1000000000LL + (long long)std::floor((control_period - sec) * 1e9 + 0.5);
		set_view(b, b->hw.cad, b->hwb.cad.get());
	} else {
		b->hw.period_ns = 0;
		set_view(b, b->hw.cad, nullptr);
	}
	return MJB_OK;
}

int mjb_hwsim_estop(mjb_batch *b, int active)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->hw.n <= 0) return fail(MJB_EINVAL, "mjb_hwsim_estop before mjb_hwsim_configure");
	const int on = active ? 1 : 0;
	if (on == b->hw.estop) return MJB_OK;
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (on) {  // position-controlled joints hold the command they had when the e-stop came (default_robot_hw_sim.cpp:251-258)
		const size_t per = (size_t)b->nenv * b->hw.n;
		HIP_TRY(hipMemcpy(b->hwb.cmd.get() + 3 * per, b->hwb.cmd.get(), per * sizeof(double), hipMemcpyDeviceToDevice));
	}
	b->hw.estop = on;
	b->params_dirty = true;
	return MJB_OK;
}

// ---- sensors-plugin equivalent (kernel in mjb_sensor_pack.hip) ----
static int sensor_buffers(mjb_batch *b)
{
	const mjb_model_desc &h = b->model->h;
	const size_t ns = (size_t)(h.nsensor > 0 ? h.nsensor : 1), nd = (size_t)b->nenv * (size_t)(h.nsensordata > 0 ? h.nsensordata : 1);
	if (b->sens_flag.empty()) {
		b->sens_flag.assign(ns, 0);
		b->sens_mean.assign(3 * ns, 0.0);
		b->sens_sigma.assign(3 * ns, 0.0);
	}
	if (!b->sens.truth) {
		if (!b->sens.alloc(ns, nd)) {
			b->sens = SensorBufs{};
			return fail(MJB_ENOMEM, "sensor message buffers: allocation failed");
		}
		b->sens_dirty = true;
	}
	return MJB_OK;
}

int mjb_sensor_set_noise(mjb_batch *b, int sensor, int set_flag, const double *mean3, const double *sigma3)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (sensor < 0 || sensor >= h.nsensor) return fail(MJB_EINVAL, "mjb_sensor_set_noise: no sensor %d", sensor);
	if (set_flag < 0 || set_flag > 7 || (set_flag && (!mean3 || !sigma3))) return fail(MJB_EINVAL, "mjb_sensor_set_noise: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	int rc = sensor_buffers(b);
	if (rc) return rc;
	// registerNoiseModelsCB: the n-th SET bit of this request takes mean[n] / std[n]; bits accumulate (is_set |= flag)
	int idx = 0;
	for (int k = 0; k < 3; k++)
		if (set_flag & (1 << k)) {
			b->sens_mean[3 * sensor + idx] = mean3[idx];
			b->sens_sigma[3 * sensor + idx] = sigma3[idx];
			idx++;
		}
	if (set_flag == 0) b->sens_flag[sensor] = 0;  // (extension: a zero flag clears the model)
	else b->sens_flag[sensor] |= set_flag;
	b->sens_dirty = true;
	return MJB_OK;
}

int mjb_sensor_pack(mjb_batch *b, uint64_t seed)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	HIP_TRY(hipSetDevice(b->device));
	int rc = sensor_buffers(b);
	if (rc) return rc;
	rc = sync_params(b);
	if (rc) return rc;
	if (b->sens_dirty) {
		HIP_TRY(hipStreamSynchronize(b->stream.get()));
		HIP_TRY(hipMemcpy(b->sens.flag.get(), b->sens_flag.data(), b->sens_flag.size() * sizeof(int), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(b->sens.mean.get(), b->sens_mean.data(), b->sens_mean.size() * sizeof(double), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(b->sens.sigma.get(), b->sens_sigma.data(), b->sens_sigma.size() * sizeof(double), hipMemcpyHostToDevice));
		b->sens_dirty = false;
	}
	rc = mjb_launch_sensor_pack(b->params_dev.get(), b->nenv, h.nsensor, b->sens.flag.get(), b->sens.mean.get(), b->sens.sigma.get(), seed,
	                            b->nz.env_offset, b->step_counter, b->sens.value.get(), b->sens.truth.get(), b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "sensor pack launch failed: %s", hipGetErrorString((hipError_t)rc));
	b->sens_packed = true;
	return MJB_OK;
}

int mjb_sensor_get(mjb_batch *b, int which, int env_lo, int env_hi, float *host)
{
	if (!b || !host || which < 0 || which > 1) return fail(MJB_EINVAL, "mjb_sensor_get: bad argument");
	if (!b->sens_packed) return fail(MJB_EINVAL, "mjb_sensor_get before mjb_sensor_pack");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "mjb_sensor_get: bad env range");
	const size_t S = (size_t)b->model->h.nsensordata;
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	const float *src = (which == 0 ? b->sens.value.get() : b->sens.truth.get()) + (size_t)env_lo * S;
	HIP_TRY(hipMemcpy(host, src, (size_t)(env_hi - env_lo) * S * sizeof(float), hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_sensor_device_ptr(mjb_batch *b, int which)
{
	if (!b || which < 0 || which > 1 || sensor_buffers(b) != MJB_OK) return nullptr;
	return which == 0 ? (void *)b->sens.value.get() : (void *)b->sens.truth.get();
}

// ---- batched ray casting (kernel in mjb_ray.hip) ----
int mjb_rays_configure(mjb_batch *b, int nray, const int *site, const double *pnt, const double *vec, const unsigned char *exclude_own_body, const unsigned char *geom_mask)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (nray < 1 || !site || !vec) return fail(MJB_EINVAL, "mjb_rays_configure: nray must be at least 1, with a site and a vec per ray");
	if (h.ngeom < 1) return fail(MJB_EINVAL, "mjb_rays_configure: the model has no geoms");
	// the table of mjb_launch_rays: pnt[3][nray] | vec[3][nray] as doubles, then {site, exclude own body}[nray] and visible[ngeom] as ints
	const size_t n = (size_t)nray, nints = 2 * n + (size_t)h.ngeom, ndoubles = 6 * n + (nints + 1) / 2;
	std::vector<double> tab(ndoubles, 0.0);
	int *itab = reinterpret_cast<int *>(tab.data() + 6 * n);
	for (size_t r = 0; r < n; r++) {
		if (site[r] < -1 || site[r] >= h.nsite) return fail(MJB_EINVAL, "mjb_rays_configure: ray %zu: site %d outside [-1, %d)", r, site[r], h.nsite);
		for (int k = 0; k < 3; k++) {
			const double p = pnt ? pnt[3 * r + k] : 0.0, v = vec[3 * r + k];
			if (!std::isfinite(p) || !std::isfinite(v)) return fail(MJB_EINVAL, "mjb_rays_configure: ray %zu: non-finite pnt or vec", r);
			tab[(size_t)k * n + r] = p;
			tab[(size_t)(3 + k) * n + r] = v;
		}
		if (vec[3 * r] == 0 && vec[3 * r + 1] == 0 && vec[3 * r + 2] == 0) return fail(MJB_EINVAL, "mjb_rays_configure: ray %zu: vec is zero", r);
		itab[2 * r] = site[r];
		itab[2 * r + 1] = (site[r] >= 0 && (!exclude_own_body || exclude_own_body[r])) ? 1 : 0;
	}
	for (int g = 0; g < h.ngeom; g++) itab[2 * n + g] = geom_mask ? (geom_mask[g] != 0) : (h.geom_rgba[4 * g + 3] != 0);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (a cast of the previous configuration may still read what goes now)
	RayBufs rb;
	if (!rb.tab.alloc(ndoubles) || !rb.dist.alloc_zeroed((size_t)b->nenv * n) || !rb.geomid.alloc_zeroed((size_t)b->nenv * n))
		return fail(MJB_ENOMEM, "mjb_rays_configure: allocation failed for %d envs x %d rays", b->nenv, nray);
	HIP_TRY(hipMemcpy(rb.tab.get(), tab.data(), ndoubles * sizeof(double), hipMemcpyHostToDevice));
	b->rays = std::move(rb);
	b->nray = nray;
	return MJB_OK;
}

int mjb_rays_cast(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->nray < 1) return fail(MJB_EINVAL, "mjb_rays_cast before mjb_rays_configure");
	if (!b->frame_valid || !b->st.frame_ws || b->frame_hi < b->nenv)
		return fail(MJB_EINVAL, "mjb_rays_cast reads the geom and site poses of every env: only after mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame");
	HIP_TRY(hipSetDevice(b->device));
	if (int rc = join_rest(b)) return rc;
	if (int rc = sync_params(b)) return rc;
	const int rc = mjb_launch_rays(b->params_dev.get(), b->rays.tab.get(), b->nenv, b->nray, b->rays.dist.get(), b->rays.geomid.get(), b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "ray launch failed: %s", hipGetErrorString((hipError_t)rc));
	return MJB_OK;
}

int mjb_rays_get(mjb_batch *b, int env_lo, int env_hi, double *dist, int *geomid)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->nray < 1) return fail(MJB_EINVAL, "mjb_rays_get before mjb_rays_configure");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	const size_t n = (size_t)(env_hi - env_lo) * b->nray, off = (size_t)env_lo * b->nray;
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (dist && n) HIP_TRY(hipMemcpy(dist, b->rays.dist.get() + off, n * sizeof(double), hipMemcpyDeviceToHost));
	if (geomid && n) HIP_TRY(hipMemcpy(geomid, b->rays.geomid.get() + off, n * sizeof(int), hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_rays_device_ptr(mjb_batch *b, int which)
{
	if (!b || which < 0 || which > 1 || b->nray < 1) {
		fail(MJB_EINVAL, "mjb_rays_device_ptr: bad argument, or no mjb_rays_configure yet");
		return nullptr;
	}
	return which == 0 ? (void *)b->rays.dist.get() : (void *)b->rays.geomid.get();
}

int mjb_rays_count(const mjb_batch *b) { return b ? b->nray : fail(MJB_EINVAL, "null batch"); }

// ---- batched Jacobians (kernel in mjb_jac.hip) ----
static const int kJacOutputs = MJB_JAC_OUT_J | MJB_JAC_OUT_MINVJT | MJB_JAC_OUT_AINV | MJB_JAC_OUT_VEL;
// the buffer of one output bit and its doubles per (env, point); NULL: not one bit, or not configured
static DevBuf<double> *jac_output(mjb_batch *b, int which, size_t *per_point)
{
	const size_t nv = (size_t)b->model->h.nv;
	if (!(which & b->jac_outputs)) return nullptr;
	switch (which) {
	case MJB_JAC_OUT_J: *per_point = 6 * nv; return &b->jac.J;
	case MJB_JAC_OUT_MINVJT: *per_point = 6 * nv; return &b->jac.MinvJT;
	case MJB_JAC_OUT_AINV: *per_point = 36; return &b->jac.Ainv;
	case MJB_JAC_OUT_VEL: *per_point = 6; return &b->jac.vel;
	default: return nullptr;
	}
}

// The point table of mjb_launch_jac and mjb_launch_dyn (mjb_jac.h): pnt[npoint][3] as doubles, then one JacPoint per point -- validated and resolved
// for `who` (mjb_jac_configure, mjb_dyn_configure), whose name the refusals carry.
static int resolve_points(const mjb_batch *b, const char *who, int npoint, const int *objtype, const int *objid, const double *pnt, std::vector<double> &tab)
{
	const mjb_model_desc &h = b->model->h;
	const size_t n = (size_t)npoint, ndoubles = 3 * n + n * (sizeof(JacPoint) / sizeof(double));
	tab.assign(ndoubles, 0.0);
	JacPoint *rec = reinterpret_cast<JacPoint *>(tab.data() + 3 * n);
	for (size_t k = 0; k < n; k++) {
		const int ty = objtype[k], id = objid[k];
		int count, body;
		switch (ty) {
		case MJB_JAC_SITE: count = h.nsite; break;
		case MJB_JAC_BODY: case MJB_JAC_BODYCOM: count = h.nbody; break;
		case MJB_JAC_GEOM: count = h.ngeom; break;
		default: return fail(MJB_EINVAL, "%s: point %zu: unknown object type %d", who, k, ty);
		}
		if (id < 0 || id >= count) return fail(MJB_EINVAL, "%s: point %zu: id %d outside [0, %d)", who, k, id, count);
		body = ty == MJB_JAC_SITE ? h.site_bodyid[id] : (ty == MJB_JAC_GEOM ? h.geom_bodyid[id] : id);
		for (int c = 0; c < 3; c++) {
			const double p = pnt ? pnt[3 * k + c] : 0.0;
			if (!std::isfinite(p)) return fail(MJB_EINVAL, "%s: point %zu: non-finite pnt", who, k);
			tab[3 * k + c] = p;
		}
		rec[k].type = ty;
		rec[k].id = id;
		rec[k].body = body;
		rec[k].root = h.body_rootid[body];
		rec[k].mask[0] = (unsigned int)b->model->body_dofmask[2 * body];
		rec[k].mask[1] = (unsigned int)b->model->body_dofmask[2 * body + 1];
	}
	return MJB_OK;
}

int mjb_jac_configure(mjb_batch *b, int npoint, const int *objtype, const int *objid, const double *pnt, int outputs)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (npoint < 1 || !objtype || !objid) return fail(MJB_EINVAL, "mjb_jac_configure: npoint must be at least 1, with an object type and an id per point");
	if (outputs == 0 || (outputs & ~kJacOutputs)) return fail(MJB_EINVAL, "mjb_jac_configure: outputs 0x%x: at least one of the MJB_JAC_OUT_* bits and no other", (unsigned)outputs);
	if (h.nv < 1) return fail(MJB_EINVAL, "mjb_jac_configure: the model has no dofs");
	std::vector<double> tab;
	if (int rc = resolve_points(b, "mjb_jac_configure", npoint, objtype, objid, pnt, tab)) return rc;
	const size_t n = (size_t)npoint, ndoubles = tab.size();
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (an evaluation of the previous configuration may still read what goes now)
	JacBufs jb;
	const size_t np = (size_t)b->nenv * n, nv = (size_t)h.nv;
	if (!jb.tab.alloc(ndoubles) || ((outputs & MJB_JAC_OUT_J) && !jb.J.alloc_zeroed(np * 6 * nv)) || ((outputs & MJB_JAC_OUT_MINVJT) && !jb.MinvJT.alloc_zeroed(np * 6 * nv)) ||
	    ((outputs & MJB_JAC_OUT_AINV) && !jb.Ainv.alloc_zeroed(np * 36)) || ((outputs & MJB_JAC_OUT_VEL) && !jb.vel.alloc_zeroed(np * 6)))
		return fail(MJB_ENOMEM, "mjb_jac_configure: allocation failed for %d envs x %d points", b->nenv, npoint);
	HIP_TRY(hipMemcpy(jb.tab.get(), tab.data(), ndoubles * sizeof(double), hipMemcpyHostToDevice));
	b->jac = std::move(jb);
	b->njac = npoint;
	b->jac_outputs = outputs;
	return MJB_OK;
}

int mjb_jac_eval(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->njac < 1) return fail(MJB_EINVAL, "mjb_jac_eval before mjb_jac_configure");
	if (!b->frame_valid || !b->st.frame_ws || b->frame_hi < b->nenv)
		return fail(MJB_EINVAL, "mjb_jac_eval reads cdof, the poses and the factor of qM of every env: only after mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame");
	if (b->pose_written)
		return fail(MJB_EINVAL, "mjb_jac_eval: qpos or a mocap pose has been written since the frame was computed, its Jacobians belong to the old poses: only after mjb_forward / mjb_step1 / "
		                        "mjb_step2, or a fused step with keep_frame");
	HIP_TRY(hipSetDevice(b->device));
	if (int rc = join_rest(b)) return rc;
	if (int rc = sync_params(b)) return rc;
	const int rc = mjb_launch_jac(b->params_dev.get(), b->jac.tab.get(), b->nenv, b->njac, b->model->h.nv, b->model->h.nM, b->jac.J.get(), b->jac.MinvJT.get(), b->jac.Ainv.get(),
	                              b->jac.vel.get(), b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "Jacobian launch failed: %s", hipGetErrorString((hipError_t)rc));
	return MJB_OK;
}

int mjb_jac_get(mjb_batch *b, int which, int env_lo, int env_hi, double *host)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->njac < 1) return fail(MJB_EINVAL, "mjb_jac_get before mjb_jac_configure");
	size_t per_point = 0;
	DevBuf<double> *buf = jac_output(b, which, &per_point);
	if (!buf) return fail(MJB_EINVAL, "mjb_jac_get: output 0x%x is not one MJB_JAC_OUT_* bit of the configuration (0x%x)", (unsigned)which, (unsigned)b->jac_outputs);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	const size_t n = (size_t)(env_hi - env_lo) * b->njac * per_point, off = (size_t)env_lo * b->njac * per_point;
	if (n && !host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (n) HIP_TRY(hipMemcpy(host, buf->get() + off, n * sizeof(double), hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_jac_device_ptr(mjb_batch *b, int which)
{
	size_t per_point = 0;
	DevBuf<double> *buf = (b && b->njac >= 1) ? jac_output(b, which, &per_point) : nullptr;
	if (!buf) {
		fail(MJB_EINVAL, "mjb_jac_device_ptr: bad argument, or an output that mjb_jac_configure was not asked for");
		return nullptr;
	}
	return buf->get();
}

int mjb_jac_count(const mjb_batch *b) { return b ? b->njac : fail(MJB_EINVAL, "null batch"); }

// ---- batched joint-space dynamics (kernel in mjb_dyn.hip) ----
static const int kDynOutputs = MJB_DYN_OUT_M | MJB_DYN_OUT_MV | MJB_DYN_OUT_MINVV | MJB_DYN_OUT_ID | MJB_DYN_OUT_JDOTV;
static const int kDynVecOutputs = MJB_DYN_OUT_MV | MJB_DYN_OUT_MINVV | MJB_DYN_OUT_ID;
// the buffer of one output bit (or of MJB_DYN_IN_V) and its doubles per env; NULL: not one bit, or not configured
static DevBuf<double> *dyn_buffer(mjb_batch *b, int which, size_t *per_env)
{
	const size_t nv = (size_t)b->model->h.nv, nvec = (size_t)b->dyn_nvec;
	if (which == MJB_DYN_IN_V) {
		*per_env = nvec * nv;
		return b->dyn.V ? &b->dyn.V : nullptr;
	}
	if (!(which & b->dyn_outputs)) return nullptr;
	switch (which) {
	case MJB_DYN_OUT_M: *per_env = nv * nv; return &b->dyn.M;
	case MJB_DYN_OUT_MV: *per_env = nvec * nv; return &b->dyn.MV;
	case MJB_DYN_OUT_MINVV: *per_env = nvec * nv; return &b->dyn.MinvV;
	case MJB_DYN_OUT_ID: *per_env = nvec * nv; return &b->dyn.ID;
	case MJB_DYN_OUT_JDOTV: *per_env = (size_t)b->dyn_npoint * 6; return &b->dyn.Jdotv;
	default: return nullptr;
	}
}

int mjb_dyn_configure(mjb_batch *b, int nvec, int npoint, const int *objtype, const int *objid, const double *pnt, int outputs)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (outputs & MJB_DYN_IN_V) return fail(MJB_EINVAL, "mjb_dyn_configure: outputs 0x%x: MJB_DYN_IN_V names the input of mjb_dyn_device_ptr, it is not an output", (unsigned)outputs);
	if (outputs == 0 || (outputs & ~kDynOutputs)) return fail(MJB_EINVAL, "mjb_dyn_configure: outputs 0x%x: at least one of the MJB_DYN_OUT_* bits and no other", (unsigned)outputs);
	if (nvec < 0 || ((outputs & kDynVecOutputs) && nvec < 1)) return fail(MJB_EINVAL, "mjb_dyn_configure: nvec %d: at least 1 for MV, MINVV or ID, never negative", nvec);
	const bool jdot = (outputs & MJB_DYN_OUT_JDOTV) != 0;
	if (jdot && (npoint < 1 || !objtype || !objid)) return fail(MJB_EINVAL, "mjb_dyn_configure: JDOTV: npoint must be at least 1, with an object type and an id per point");
	if (h.nv < 1) return fail(MJB_EINVAL, "mjb_dyn_configure: the model has no dofs");
	if (!jdot) npoint = 0;  // (points without JDOTV are not looked at)
	if (!(outputs & kDynVecOutputs)) nvec = 0;  // (nor vectors without an output of theirs)
	std::vector<double> tab;
	if (jdot)
		if (int rc = resolve_points(b, "mjb_dyn_configure", npoint, objtype, objid, pnt, tab)) return rc;
	std::vector<int> full((size_t)h.nv * h.nv);
	mjb_dyn_full_adr(h.nv, h.dof_Madr, h.dof_parentid, full.data());
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (an evaluation of the previous configuration may still read what goes now)
	DynBufs db;
	const size_t ne = (size_t)b->nenv, nv = (size_t)h.nv, nvv = ne * (size_t)nvec * nv;
	if (!db.full_adr.alloc(full.size()) || (jdot && !db.tab.alloc(tab.size())) || (nvec > 0 && !db.V.alloc_zeroed(nvv)) || ((outputs & MJB_DYN_OUT_M) && !db.M.alloc_zeroed(ne * nv * nv)) ||
	    ((outputs & MJB_DYN_OUT_MV) && !db.MV.alloc_zeroed(nvv)) || ((outputs & MJB_DYN_OUT_MINVV) && !db.MinvV.alloc_zeroed(nvv)) || ((outputs & MJB_DYN_OUT_ID) && !db.ID.alloc_zeroed(nvv)) ||
	    (jdot && !db.Jdotv.alloc_zeroed(ne * (size_t)npoint * 6)))
		return fail(MJB_ENOMEM, "mjb_dyn_configure: allocation failed for %d envs x %d vectors, %d points", b->nenv, nvec, npoint);
	HIP_TRY(hipMemcpy(db.full_adr.get(), full.data(), full.size() * sizeof(int), hipMemcpyHostToDevice));
	if (jdot) HIP_TRY(hipMemcpy(db.tab.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
	b->dyn = std::move(db);
	b->dyn_nvec = nvec;
	b->dyn_npoint = npoint;
	b->dyn_outputs = outputs;
	return MJB_OK;
}

int mjb_dyn_set_vectors(mjb_batch *b, int env_lo, int env_hi, const double *host)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->dyn_outputs == 0) return fail(MJB_EINVAL, "mjb_dyn_set_vectors before mjb_dyn_configure");
	if (b->dyn_nvec < 1) return fail(MJB_EINVAL, "mjb_dyn_set_vectors: the configuration has no vectors (none of MV, MINVV, ID)");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	const size_t per_env = (size_t)b->dyn_nvec * b->model->h.nv, n = (size_t)(env_hi - env_lo) * per_env;
	if (n && !host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (an evaluation in flight still reads the vectors)
	if (n) HIP_TRY(hipMemcpy(b->dyn.V.get() + (size_t)env_lo * per_env, host, n * sizeof(double), hipMemcpyHostToDevice));
	return MJB_OK;
}

int mjb_dyn_eval(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->dyn_outputs == 0) return fail(MJB_EINVAL, "mjb_dyn_eval before mjb_dyn_configure");
	if (!b->frame_valid || !b->st.frame_ws || b->frame_hi < b->nenv)
		return fail(MJB_EINVAL, "mjb_dyn_eval reads qM, its factor and the velocity stage of every env: only after mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame");
	if (b->pose_written)
		return fail(MJB_EINVAL, "mjb_dyn_eval: qpos or a mocap pose has been written since the frame was computed, its mass matrix belongs to the old poses: only after mjb_forward / mjb_step1 / "
		                        "mjb_step2, or a fused step with keep_frame");
	const bool reads_vel = (b->dyn_outputs & (MJB_DYN_OUT_ID | MJB_DYN_OUT_JDOTV)) != 0, jdot = (b->dyn_outputs & MJB_DYN_OUT_JDOTV) != 0;
	if (reads_vel && b->vel_written)
		return fail(MJB_EINVAL, "mjb_dyn_eval: qvel has been written since the frame was computed, qfrc_bias, qfrc_passive, cvel and cdof_dot (ID, JDOTV) belong to the old velocities: "
		                        "only after mjb_forward / mjb_step1 / mjb_step2, or a fused step with keep_frame");
	if (jdot && b->vel_integrated && b->model->h.integrator == MJB_INT_RK4)
		return fail(MJB_EINVAL, "mjb_dyn_eval: JDOTV behind an RK4 step: the frame belongs to the step's last evaluation, whose velocities the batch no longer holds: only after "
		                        "mjb_forward / mjb_step1");
	HIP_TRY(hipSetDevice(b->device));
	if (int rc = join_rest(b)) return rc;
	if (int rc = sync_params(b)) return rc;
	const int rc = mjb_launch_dyn(b->params_dev.get(), b->dyn.full_adr.get(), b->dyn.tab.get(), b->dyn.V.get(), b->nenv, b->dyn_nvec, b->dyn_npoint, b->model->h.nv, b->model->h.nM,
	                              b->vel_integrated ? 1 : 0, b->dyn.M.get(), b->dyn.MV.get(), b->dyn.MinvV.get(), b->dyn.ID.get(), b->dyn.Jdotv.get(), b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "dynamics launch failed: %s", hipGetErrorString((hipError_t)rc));
	return MJB_OK;
}

int mjb_dyn_get(mjb_batch *b, int which, int env_lo, int env_hi, double *host)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->dyn_outputs == 0) return fail(MJB_EINVAL, "mjb_dyn_get before mjb_dyn_configure");
	size_t per_env = 0;
	DevBuf<double> *buf = which == MJB_DYN_IN_V ? nullptr : dyn_buffer(b, which, &per_env);
	if (!buf) return fail(MJB_EINVAL, "mjb_dyn_get: output 0x%x is not one MJB_DYN_OUT_* bit of the configuration (0x%x)", (unsigned)which, (unsigned)b->dyn_outputs);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	const size_t n = (size_t)(env_hi - env_lo) * per_env, off = (size_t)env_lo * per_env;
	if (n && !host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (n) HIP_TRY(hipMemcpy(host, buf->get() + off, n * sizeof(double), hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_dyn_device_ptr(mjb_batch *b, int which)
{
	size_t per_env = 0;
	DevBuf<double> *buf = (b && b->dyn_outputs != 0) ? dyn_buffer(b, which, &per_env) : nullptr;
	if (!buf) {
		fail(MJB_EINVAL, "mjb_dyn_device_ptr: bad argument, or an output (or the input MJB_DYN_IN_V) that mjb_dyn_configure was not asked for");
		return nullptr;
	}
	return buf->get();
}

int mjb_dyn_count(const mjb_batch *b, int *nvec, int *npoint)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (nvec) *nvec = b->dyn_nvec;
	if (npoint) *npoint = b->dyn_npoint;
	return MJB_OK;
}

// ---- batched contact wrenches (kernel in mjb_contact.hip) ----
static const int kConOutputs = MJB_CON_OUT_WRENCH | MJB_CON_OUT_NORMAL | MJB_CON_OUT_COUNT | MJB_CON_OUT_DIST | MJB_CON_OUT_CONTACTS;
// the device address of one output bit, its elements per env and their size; NULL: not one bit, or not configured
static void *con_output(mjb_batch *b, int which, size_t *per_env, size_t *elem)
{
	if (!(which & b->con_outputs)) return nullptr;
	const size_t nq = (size_t)b->ncquery;
	*elem = sizeof(double);
	switch (which) {
	case MJB_CON_OUT_WRENCH: *per_env = nq * 6; return b->con.wrench.get();
	case MJB_CON_OUT_NORMAL: *per_env = nq; return b->con.normal.get();
	case MJB_CON_OUT_COUNT: *per_env = nq; *elem = sizeof(int); return b->con.count.get();
	case MJB_CON_OUT_DIST: *per_env = nq; return b->con.dist.get();
	case MJB_CON_OUT_CONTACTS: *per_env = (size_t)b->model->h.nconmax * 6; return b->con.contacts.get();
	default: return nullptr;
	}
}

int mjb_contact_configure(mjb_batch *b, int nquery, const unsigned char *geom_a, const unsigned char *geom_b, const int *ref_body, int outputs)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (nquery < 1 || !geom_a || !geom_b) return fail(MJB_EINVAL, "mjb_contact_configure: nquery must be at least 1, with two geom sets per query");
	if (outputs == 0 || (outputs & ~kConOutputs)) return fail(MJB_EINVAL, "mjb_contact_configure: outputs 0x%x: at least one of the MJB_CON_OUT_* bits and no other", (unsigned)outputs);
	if (h.nconmax < 1 || h.ngeom < 1) return fail(MJB_EINVAL, "mjb_contact_configure: the model has no contacts (nconmax %d, ngeom %d)", h.nconmax, h.ngeom);
	// the table of mjb_launch_contact (mjb_contact.h): mask[nquery][2][nwords] as bit words, then ref_body[nquery]
	const size_t n = (size_t)nquery, ng = (size_t)h.ngeom, nw = (size_t)mjb_contact_mask_words(h.ngeom), nwords = mjb_contact_table_words(h.ngeom, nquery);
	std::vector<unsigned int> tab(nwords, 0u);
	for (size_t q = 0; q < n; q++) {
		size_t na = 0, nb = 0;
		for (size_t g = 0; g < ng; g++) {
			const bool a = geom_a[q * ng + g] != 0, bb = geom_b[q * ng + g] != 0;
			if (a && bb) return fail(MJB_EINVAL, "mjb_contact_configure: query %zu: geom %zu is in both sets", q, g);
			if (a) tab[(q * 2) * nw + (g >> 5)] |= 1u << (g & 31), na++;
			if (bb) tab[(q * 2 + 1) * nw + (g >> 5)] |= 1u << (g & 31), nb++;
		}
		if (na == 0 || nb == 0) return fail(MJB_EINVAL, "mjb_contact_configure: query %zu: set %s is empty", q, na == 0 ? "A" : "B");
		const int rb = ref_body ? ref_body[q] : -1;
		if (rb < -1 || rb >= h.nbody) return fail(MJB_EINVAL, "mjb_contact_configure: query %zu: ref_body %d outside [-1, %d)", q, rb, h.nbody);
		tab[n * 2 * nw + q] = (unsigned int)rb;
	}
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));  // (an evaluation of the previous configuration may still read what goes now)
	ConBufs cb;
	const size_t ne = (size_t)b->nenv;
	if (!cb.tab.alloc(nwords) || ((outputs & MJB_CON_OUT_WRENCH) && !cb.wrench.alloc_zeroed(ne * n * 6)) || ((outputs & MJB_CON_OUT_NORMAL) && !cb.normal.alloc_zeroed(ne * n)) ||
	    ((outputs & MJB_CON_OUT_COUNT) && !cb.count.alloc_zeroed(ne * n)) || ((outputs & MJB_CON_OUT_DIST) && !cb.dist.alloc_zeroed(ne * n)) ||
	    ((outputs & MJB_CON_OUT_CONTACTS) && !cb.contacts.alloc_zeroed(ne * (size_t)h.nconmax * 6)))
		return fail(MJB_ENOMEM, "mjb_contact_configure: allocation failed for %d envs x %d queries", b->nenv, nquery);
	HIP_TRY(hipMemcpy(cb.tab.get(), tab.data(), nwords * sizeof(unsigned int), hipMemcpyHostToDevice));
	b->con = std::move(cb);
	b->ncquery = nquery;
	b->con_outputs = outputs;
	return MJB_OK;
}

int mjb_contact_eval(mjb_batch *b)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->ncquery < 1) return fail(MJB_EINVAL, "mjb_contact_eval before mjb_contact_configure");
	if (!b->frame_valid || !b->st.frame_ws || b->frame_hi < b->nenv)
		return fail(MJB_EINVAL, "mjb_contact_eval reads the contacts and efc_force of every env: only after mjb_forward / mjb_step2, or a fused step with keep_frame");
	if (b->frame_half)
		return fail(MJB_EINVAL, "mjb_contact_eval: the frame was written by mjb_step1 and no mjb_step2 has followed, its efc_force is not this state's: only after mjb_forward / "
		                        "mjb_step2, or a fused step with keep_frame");
	HIP_TRY(hipSetDevice(b->device));
	if (int rc = join_rest(b)) return rc;
	if (int rc = sync_params(b)) return rc;
	const int rc = mjb_launch_contact(b->params_dev.get(), b->con.tab.get(), b->nenv, b->ncquery, b->model->h.ngeom, b->model->h.nconmax, b->con.wrench.get(), b->con.normal.get(),
	                                  b->con.count.get(), b->con.dist.get(), b->con.contacts.get(), b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "contact wrench launch failed: %s", hipGetErrorString((hipError_t)rc));
	return MJB_OK;
}

int mjb_contact_get(mjb_batch *b, int which, int env_lo, int env_hi, void *host)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (b->ncquery < 1) return fail(MJB_EINVAL, "mjb_contact_get before mjb_contact_configure");
	size_t per_env = 0, elem = 0;
	const char *buf = static_cast<const char *>(con_output(b, which, &per_env, &elem));
	if (!buf) return fail(MJB_EINVAL, "mjb_contact_get: output 0x%x is not one MJB_CON_OUT_* bit of the configuration (0x%x)", (unsigned)which, (unsigned)b->con_outputs);
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_ERANGE, "env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	const size_t n = (size_t)(env_hi - env_lo) * per_env * elem, off = (size_t)env_lo * per_env * elem;
	if (n && !host) return fail(MJB_EINVAL, "null host buffer");
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (n) HIP_TRY(hipMemcpy(host, buf + off, n, hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_contact_device_ptr(mjb_batch *b, int which)
{
	size_t per_env = 0, elem = 0;
	void *buf = (b && b->ncquery >= 1) ? con_output(b, which, &per_env, &elem) : nullptr;
	if (!buf) {
		fail(MJB_EINVAL, "mjb_contact_device_ptr: bad argument, or an output that mjb_contact_configure was not asked for");
		return nullptr;
	}
	return buf;
}

int mjb_contact_count(const mjb_batch *b) { return b ? b->ncquery : fail(MJB_EINVAL, "null batch"); }

// ---- device-side episode resets (kernel in mjb_episode.hip) ----
// done | episode | ndone, zeroed: made by the first call that launches the kernel or hands out their addresses
static int episode_outputs(mjb_batch *b)
{
	if (b->epi.done) return MJB_OK;
	HIP_TRY(hipSetDevice(b->device));
	DevBuf<unsigned char> done;
	DevBuf<unsigned int> episode, ndone;
	if (!done.alloc_zeroed((size_t)b->nenv) || !episode.alloc_zeroed((size_t)b->nenv) || !ndone.alloc_zeroed(1))
		return fail(MJB_ENOMEM, "mjb_episode: allocation failed for %d envs", b->nenv);
	b->epi.done = std::move(done);
	b->epi.episode = std::move(episode);
	b->epi.ndone = std::move(ndone);
	return MJB_OK;
}

// a configuration array of the episode kernel replaces the one before it (n == 0: none); an earlier launch may still read what goes
static int episode_upload(mjb_batch *b, DevBuf<double> &dst, const std::vector<double> &v)
{
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	DevBuf<double> buf;
	if (!v.empty()) {
		if (!buf.alloc(v.size())) return fail(MJB_ENOMEM, "mjb_episode: allocation failed for %zu doubles", v.size());  // (the upload writes all of it)
		HIP_TRY(hipMemcpy(buf.get(), v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
	}
	dst = std::move(buf);
	return MJB_OK;
}

int mjb_episode_set_init(mjb_batch *b, int ninit, const double *qpos, const double *qvel, const double *act)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const mjb_model_desc &h = b->model->h;
	if (ninit < 0) return fail(MJB_EINVAL, "mjb_episode_set_init: ninit %d is negative", ninit);
	const size_t n = (size_t)ninit, nq = (size_t)h.nq, nv = (size_t)h.nv, na = (size_t)h.na;
	if (ninit > 0 && nq > 0 && !qpos) return fail(MJB_EINVAL, "mjb_episode_set_init: a bank of %d rows needs qpos", ninit);
	std::vector<double> bank(n * (nq + nv + na), 0.0);
	for (size_t k = 0; k < n * nq; k++) bank[k] = qpos[k];
	for (size_t k = 0; qvel && k < n * nv; k++) bank[n * nq + k] = qvel[k];
	for (size_t k = 0; act && k < n * na; k++) bank[n * (nq + nv) + k] = act[k];
	for (size_t k = 0; k < bank.size(); k++)
		if (!std::isfinite(bank[k])) return fail(MJB_EINVAL, "mjb_episode_set_init: non-finite entry in %s", k < n * nq ? "qpos" : (k < n * (nq + nv) ? "qvel" : "act"));
	for (size_t r = 0; r < n; r++)
		for (int j = 0; j < h.njnt; j++) {
			if (h.jnt_type[j] != MJB_JNT_FREE && h.jnt_type[j] != MJB_JNT_BALL) continue;
			const double *q = bank.data() + r * nq + h.jnt_qposadr[j] + (h.jnt_type[j] == MJB_JNT_FREE ? 3 : 0);
			if (std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) < 1e-15)  // (mjMINVAL: what normalize4 replaces by the identity)
				return fail(MJB_EINVAL, "mjb_episode_set_init: row %zu: zero quaternion in joint %d", r, j);
		}
	if (int rc = episode_upload(b, b->epi.bank, bank)) return rc;
	b->ep_ninit = b->epi.bank ? ninit : 0;  // (a model without state has no bank to pick from)
	return MJB_OK;
}

int mjb_episode_set_noise(mjb_batch *b, uint64_t seed, int64_t env_offset, const double *qpos_lo, const double *qpos_hi, const double *qvel_lo, const double *qvel_hi, int clamp)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const size_t nv = (size_t)b->model->h.nv;
	if (!qpos_lo != !qpos_hi || !qvel_lo != !qvel_hi) return fail(MJB_EINVAL, "mjb_episode_set_noise: a range needs both of its ends (or neither)");
	std::vector<double> range[2];
	const double *ends[2][2] = { { qpos_lo, qpos_hi }, { qvel_lo, qvel_hi } };
	for (int part = 0; part < 2; part++) {
		if (!ends[part][0] || nv == 0) continue;
		range[part].resize(2 * nv);
		for (size_t d = 0; d < nv; d++) {
			const double lo = ends[part][0][d], hi = ends[part][1][d];
			if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi)
				return fail(MJB_EINVAL, "mjb_episode_set_noise: %s range of dof %zu: [%g, %g] is not finite or has lo > hi", part ? "qvel" : "qpos", d, lo, hi);
			range[part][d] = lo;
			range[part][nv + d] = hi;
		}
	}
	if (int rc = episode_upload(b, b->epi.qrange, range[0])) return rc;
	if (int rc = episode_upload(b, b->epi.vrange, range[1])) return rc;
	b->ep_seed = seed;
	b->ep_env_offset = env_offset;
	b->ep_clamp = clamp != 0;
	return MJB_OK;
}

int mjb_episode_set_rule(mjb_batch *b, double time_limit, const double *qpos_lo, const double *qpos_hi)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	const size_t nq = (size_t)b->model->h.nq;
	if (std::isnan(time_limit)) return fail(MJB_EINVAL, "mjb_episode_set_rule: time_limit is NaN");
	std::vector<double> box;
	if ((qpos_lo || qpos_hi) && nq > 0) {
		box.resize(2 * nq);
		for (size_t k = 0; k < nq; k++) {
			box[k] = qpos_lo ? qpos_lo[k] : -INFINITY;
			box[nq + k] = qpos_hi ? qpos_hi[k] : INFINITY;
			if (std::isnan(box[k]) || std::isnan(box[nq + k])) return fail(MJB_EINVAL, "mjb_episode_set_rule: bound of coordinate %zu is NaN", k);
		}
	}
	if (int rc = episode_upload(b, b->epi.box, box)) return rc;
	b->ep_time_limit = time_limit;
	return MJB_OK;
}

// one launch of the episode kernel with the host-side bookkeeping of a masked mjb_reset, minus its synchronise
static int episode_launch(mjb_batch *b, const uint8_t *mask_dev, int use_rule)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	HIP_TRY(hipSetDevice(b->device));
	if (int rc = episode_outputs(b)) return rc;
	if (int rc = join_rest(b)) return rc;
	b->split_ncb = -1;  // (an open split step is abandoned: mjb_step1_prefix starts the next one)
	if (int rc = sync_params(b)) return rc;
	EpisodeArgs a{};
	a.mask = mask_dev;
	a.use_rule = use_rule;
	a.ninit = b->ep_ninit;
	a.time_limit = b->ep_time_limit;
	a.box = b->epi.box.get();
	a.bank = b->epi.bank.get();
	a.qrange = b->epi.qrange.get();
	a.vrange = b->epi.vrange.get();
	a.clamp = b->ep_clamp;
	a.seed = b->ep_seed;
	a.env_offset = b->ep_env_offset;
	a.done = b->epi.done.get();
	a.episode = b->epi.episode.get();
	a.ndone = b->epi.ndone.get();
	const int rc = mjb_launch_episode(b->params_dev.get(), a, b->nenv, b->stream.get());
	if (rc != 0) return fail(MJB_ENODEVICE, "episode launch failed: %s", hipGetErrorString((hipError_t)rc));
	b->frame_valid = false;
	b->le_con_valid = false;
	b->le_xfrc_stale = true;  // (a reset env's xfrc_applied is zero again)
	return MJB_OK;
}

int mjb_episode_reset(mjb_batch *b, const uint8_t *mask_dev) { return episode_launch(b, mask_dev, 0); }
int mjb_episode_step(mjb_batch *b, const uint8_t *extra_mask_dev) { return episode_launch(b, extra_mask_dev, 1); }

int mjb_episode_get(mjb_batch *b, int env_lo, int env_hi, uint8_t *done, uint32_t *episode, uint32_t *ndone)
{
	if (!b) return fail(MJB_EINVAL, "null batch");
	if (env_lo < 0 || env_hi > b->nenv || env_lo > env_hi) return fail(MJB_EINVAL, "mjb_episode_get: env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->nenv);
	if (int rc = episode_outputs(b)) return rc;
	const size_t n = (size_t)(env_hi - env_lo);
	HIP_TRY(hipSetDevice(b->device));
	HIP_TRY(hipStreamSynchronize(b->stream.get()));
	if (done && n) HIP_TRY(hipMemcpy(done, b->epi.done.get() + env_lo, n, hipMemcpyDeviceToHost));
	if (episode && n) HIP_TRY(hipMemcpy(episode, b->epi.episode.get() + env_lo, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (ndone) HIP_TRY(hipMemcpy(ndone, b->epi.ndone.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
	return MJB_OK;
}

void *mjb_episode_device_ptr(mjb_batch *b, int which)
{
	if (!b || which < 0 || which > 2) {
		fail(MJB_EINVAL, "mjb_episode_device_ptr: null batch, or `which` %d outside 0 (done), 1 (episode), 2 (ndone)", which);
		return nullptr;
	}
	if (episode_outputs(b)) return nullptr;
	return which == 0 ? (void *)b->epi.done.get() : (which == 1 ? (void *)b->epi.episode.get() : (void *)b->epi.ndone.get());
}

int mjb_time_steps(mjb_batch *b, int nsteps, int nlaunch, double *ms_per_launch)
{
	if (!b || nsteps <= 0 || nlaunch <= 0 || !ms_per_launch) return fail(MJB_EINVAL, "mjb_time_steps: bad argument");
	HIP_TRY(hipSetDevice(b->device));
	Event e0, e1;
	HIP_TRY(e0.create(hipEventDefault));
	HIP_TRY(e1.create(hipEventDefault));
	HIP_TRY(hipEventRecord(e0.get(), b->stream.get()));
	for (int i = 0; i < nlaunch; i++) {
		int rc = mjb_step(b, nsteps);
		if (rc) return rc;
	}
	HIP_TRY(hipEventRecord(e1.get(), b->stream.get()));
	HIP_TRY(hipEventSynchronize(e1.get()));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0.get(), e1.get()));
	*ms_per_launch = (double)ms / nlaunch;
	return MJB_OK;
}

}  // extern "C"
