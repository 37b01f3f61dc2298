// mjb_lane_env.hip -- the LANE = ENV form of the unconstrained fused step (SURVEY.md §7 "measure a 64-envs-per-wave (lane = env)
// variant for the smooth-dynamics phases and report both").
//
// mjb_step_kernel<16, 0, DENSE> spreads ONE env over 16 lanes: every stage is a chain of cross-lane exchanges (DPP, LDS rounds at
// ~110 cycles each) with a third of the lanes doing fp64 work, one wavefront per SIMD -- 42.8 k cycles per step whatever the batch
// size (profiles/r03_batch_size.txt: 222 - 230 M env-steps/s from 4096 to 65 536 envs).  Here a lane owns an env:
//   * no cross-lane traffic at all -- a step is one straight line of fp64 VALU work per wavefront of 64 envs, every fp64 issue slot
//     does 64 envs' worth of arithmetic;
//   * the model is the same for every lane, so every model constant is a SCALAR load into SGPRs (one per wavefront) and rides along
//     as the scalar operand of the VALU instruction that uses it;
//   * nothing per-env can be indexed at run time (a lane's "arrays" are registers), so the kernel is a template over the model's
//     INTEGER structure (csrc/lane_env_topos.h, tools/gen_lane_env_topo.py): parent ids, joint kinds and dof ancestry are
//     compile-time constants, every loop over bodies / dofs is unrolled, zero blocks of qM never exist.  Numeric constants stay
//     run-time data;
//   * the state of 64 envs lives in the wavefront's registers for all K fused steps (512 per lane at one wavefront per SIMD);
//     what does not fit spills to the AGPR half of the file and then to scratch -- `tools/kernel_meta.py` reports both.
// Same step as the oracle's mjo_step / mj_step (mujoco_env.cpp:498,552,593) for models the topology tables cover: hinge / slide
// trees without constraint rows, Euler with implicit joint damping, joint-transmission actuators -- stateless, or with an integrator / filter
// activation state (mjData.act: in registers for the launch, one-wavefront form, hiprtc-built models) --, the sensors listed in
// gen_lane_env_topo.py, ctrl noise (mujoco_env.cpp:469-481), mj_check* resets, mjENBL_ENERGY.  Arithmetic follows MuJoCo's
// com-based formulation stage by stage (oracle/mjo_smooth.c); sums over bodies run in ascending instead of leaf-to-root order and
// reciprocals are Newton-refined hardware seeds, so results agree with the oracle to rounding, not bit for bit (tests/test_gpu_lane_env.py).
//
// The host side in this file, in order: which models the kernel takes (mjb_lane_env_match / _eligible); LeVariant and the table of the variants that
// exist (le_rows); the hiprtc build of a variant for a model without a compiled-in topology (jit_get); the tape, overlay and wrench tables; the PLAN
// (le_plan: CU count, batch size, build, the knobs' values and, for a hiprtc model, its slot counts -> a LeVariant; pure, DESIGN.md "The lane = env
// launcher" has the rule and what it reaches by default); and mjb_launch_lane_env, which gathers the plan's inputs, asks it, records and launches.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mjb_lane_env_kernel.h"
#include "lane_env_topos.h"

namespace {

using namespace mjb_le;

template <class T, int LP, bool PE = false, bool HW = false, bool XF = false>  // (PE: per-env overrides from DevState::le_overlay, mjb_set_lane_env mode 2; HW: the device hwsim stage, mjb_lane_env_set_hwsim; XF: xfrc_applied from DevState::le_xfrc, mjb_lane_env_set_xfrc)
__global__ void __launch_bounds__(64) mjb_lane_env_kernel(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0,
                                                          const int env_lo, const int env_hi)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_le[];
	lane_env_body<T, LP, LE_SOLO, PE, HW, XF>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

template <class T, int LP>
__global__ void __launch_bounds__(128) mjb_lane_env_duo_kernel(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0,
                                                               const int env_lo, const int env_hi)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_le[];
	lane_env_duo<T, LP>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

template <class T>
__global__ void __launch_bounds__(128) mjb_lane_env_duo2_kernel(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0,
                                                                const int env_lo, const int env_hi)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_le[];
	lane_env_duo2<T, 160>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

// (form 3 under either count of sweep wavefronts, NW = 3 or 4: one name for the tools that look the kernel up by it)
template <class T, int NW>
__global__ void __launch_bounds__(64 * NW) mjb_lane_env_trio_kernel(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0,
                                                                    const int env_lo, const int env_hi)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_le[];
	if constexpr (NW == 4) lane_env_quartet<T, 160>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else lane_env_trio<T, 160>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

// the joint's anchor is off centre (jnt_pos != 0): structure of a topology, LeOffc
static bool le_jnt_offc(const mjb_model_desc &h, int j) { return h.jnt_pos[3 * j] != 0 || h.jnt_pos[3 * j + 1] != 0 || h.jnt_pos[3 * j + 2] != 0; }

template <class T> bool topo_matches(const mjb_model_desc &h)
{
	if (h.nbody != T::NBODY || h.nq != T::NQ || h.nv != T::NV || h.nu != T::NU || h.na != T::NA || h.njnt != T::NJNT || h.nsite != T::NSITE ||
	    h.nsensor != T::NSENSOR || h.nsensordata != T::NSENSORDATA || h.nM != T::NM)
		return false;
	for (int b = 0; b < h.nbody; b++) {
		const int jn = h.body_jntnum[b] == 1 ? h.body_jntadr[b] : -1;
		if (h.body_jntnum[b] > 1 || h.body_parentid[b] != T::body_parentid[b] || h.body_rootid[b] != T::body_rootid[b] || jn != T::body_jnt[b] ||
		    (h.body_sameframe[b] != 0) != (T::body_sameframe[b] != 0))
			return false;
	}
	for (int j = 0; j < h.njnt; j++)
		if (h.jnt_type[j] != T::jnt_type[j] || h.jnt_bodyid[j] != T::jnt_bodyid[j] || h.jnt_qposadr[j] != j || h.jnt_dofadr[j] != j) return false;
	if constexpr (LeOffc<T>::known)  // (an anchor off centre where the table has none, or the reverse: the compiled-in kernel has no code for this model)
		for (int j = 0; j < h.njnt; j++)
			if (le_jnt_offc(h, j) != LeOffc<T>::on(j)) return false;
	for (int d = 0; d < h.nv; d++)
		if (h.dof_parentid[d] != T::dof_parentid[d] || h.dof_Madr[d] != T::dof_Madr[d] || h.dof_jntid[d] != d) return false;
	for (int i = 0; i < h.nu; i++)
		if (h.actuator_trntype[i] != MJB_TRN_JOINT || h.actuator_dyntype[i] != T::act_dyntype[i] || h.actuator_trnid[2 * i] != T::act_jnt[i] ||
		    h.actuator_gaintype[i] != T::act_gaintype[i] || h.actuator_biastype[i] != T::act_biastype[i] ||
		    (h.actuator_ctrllimited[i] != 0) != (T::act_ctrllimited[i] != 0) || (h.actuator_forcelimited[i] != 0) != (T::act_forcelimited[i] != 0) ||
		    (h.na > 0 && (h.actuator_actadr[i] != T::act_actadr[i] || (h.actuator_actlimited[i] != 0) != (T::act_actlimited[i] != 0))))
			return false;
	for (int i = 0; i < h.nsite; i++)
		if (h.site_bodyid[i] != T::site_bodyid[i] || (h.site_sameframe[i] != 0) != (T::site_sameframe[i] != 0)) return false;
	for (int i = 0; i < h.nsensor; i++)
		if (h.sensor_type[i] != T::sensor_type[i] || h.sensor_objtype[i] != T::sensor_objtype[i] || h.sensor_objid[i] != T::sensor_objid[i] ||
		    h.sensor_adr[i] != T::sensor_adr[i] || h.sensor_refid[i] >= 0)
			return false;
	return true;
}

}  // namespace

// Constraint rows the kernel takes: every row the model can ever have is a joint-equality row or a joint-limit row (of hinges and slides:
// mjb_lane_env_eligible asks for the joint kinds) swept by PGS -- no dry friction, a range wider than twice the margin on every limited joint (at most
// one row per joint at a time), every equality a joint equality (on two different joints, or on one), and room for exactly these rows: the active joint
// equalities and the limited joints (a model whose <size njmax> lowered the capacity keeps the generic kernels: truncation and mjWARN_CNSTRFULL live
// there; one with room to spare could activate an equality per env).  A row kind mjDSBL_EQUALITY / mjDSBL_LIMIT switches off has no rows.
static thread_local const char *le_refusal = "";  // why mjb_lane_env_eligible last refused a model for its size (mjb_lane_env_refusal)
static int le_count_limits(const mjb_model_desc *h)
{
	int nl = 0;
	if (!(h->disableflags & MJB_DSBL_LIMIT))
		for (int j = 0; j < h->njnt; j++) nl += h->jnt_limited[j] != 0;
	return nl;
}
static int le_count_eqs(const mjb_model_desc *h)
{
	int ne = 0;
	if (!(h->disableflags & MJB_DSBL_EQUALITY))
		for (int e = 0; e < h->neq; e++) ne += h->eq_active[e] != 0;
	return ne;
}
static bool le_limit_rows(const mjb_model_desc *h)
{
	if (h->solver != MJB_SOL_PGS) return false;
	for (int d = 0; d < h->nv; d++)
		if (h->dof_frictionloss[d] > 0) return false;
	if (!(h->disableflags & MJB_DSBL_LIMIT))
		for (int j = 0; j < h->njnt; j++)
			if (h->jnt_limited[j] && !(h->jnt_range[2 * j + 1] - h->jnt_range[2 * j] > 2 * h->jnt_margin[j])) return false;
	const int nr = le_count_limits(h) + le_count_eqs(h);
	return nr > 0 && h->nefcmax == nr;
}
// equalities: joint equalities alone, each on one joint or on two different ones (their rows: le_limit_rows)
static bool le_joint_equalities(const mjb_model_desc *h)
{
	for (int e = 0; e < h->neq; e++) {
		const int j1 = h->eq_obj1id[e], j2 = h->eq_obj2id[e];
		if (h->eq_type[e] != MJB_EQ_JOINT || j1 < 0 || j1 >= h->njnt || j2 >= h->njnt || j2 == j1) return false;
	}
	return true;
}
// tendons: fixed tendons that do nothing but carry actuators -- no limit, dry friction, spring or damper (tendon sensors and tendon equalities are refused
// with the sensors and the equalities)
static bool le_bare_tendons(const mjb_model_desc *h)
{
	for (int t = 0; t < h->ntendon; t++) {
		if (h->tendon_limited[t] || h->tendon_frictionloss[t] != 0 || h->tendon_stiffness[t] != 0 || h->tendon_damping[t] != 0) return false;
		if (h->tendon_num[t] < 1 || h->tendon_adr[t] < 0 || h->tendon_adr[t] + h->tendon_num[t] > h->nwrap) return false;
		for (int w = h->tendon_adr[t]; w < h->tendon_adr[t] + h->tendon_num[t]; w++)
			if (h->wrap_objid[w] < 0 || h->wrap_objid[w] >= h->njnt) return false;
	}
	return true;
}
// what both classifications below ask first: an Euler model of one-dof joints, without contacts or mocap bodies, and without constraint rows -- or with
// joint-equality and joint-limit rows alone
static bool le_plain_tree(const mjb_model_desc *h)
{
	return h && h->nconmax <= 0 && h->integrator == MJB_INT_EULER && h->nmocap <= 0 && h->nq == h->nv && h->njnt == h->nv &&
	       (h->ntendon <= 0 || le_bare_tendons(h)) && (h->neq <= 0 || le_joint_equalities(h)) && (h->nefcmax <= 0 || le_limit_rows(h));
}
// the dofs the rows touch (one-dof joints in dof order: a joint's id is its dof)
static int le_row_dofs(const mjb_model_desc *h)
{
	int n = 0;
	for (int j = 0; j < h->njnt; j++) {
		bool in = h->jnt_limited[j] != 0 && !(h->disableflags & MJB_DSBL_LIMIT);
		if (!(h->disableflags & MJB_DSBL_EQUALITY))
			for (int e = 0; e < h->neq; e++) in = in || (h->eq_active[e] && (h->eq_obj1id[e] == j || h->eq_obj2id[e] == j));
		n += in;
	}
	return n;
}
int mjb_lane_env_limits(const mjb_model_desc *h)
{
	return (h && h->nefcmax > 0 && mjb_lane_env_eligible(h)) ? le_count_limits(h) : 0;
}
int mjb_lane_env_eq_rows(const mjb_model_desc *h)
{
	return (h && h->nefcmax > 0 && mjb_lane_env_eligible(h)) ? le_count_eqs(h) : 0;
}
int mjb_lane_env_solo_only(const mjb_model_desc *h)
{
	return (h && (h->nefcmax > 0 || h->ntendon > 0) && mjb_lane_env_eligible(h)) ? 1 : 0;
}
// an actuator's dynamics the kernel runs: none, or an activation state of its own that integrates ctrl / filters it (muscle and user dynamics: the loader's refusal)
static bool le_dyntype_ok(const mjb_model_desc *h, int i)
{
	const int d = h->actuator_dyntype[i];
	if (d == MJB_DYN_NONE) return h->na <= 0 || h->actuator_actadr[i] < 0;
	return (d == MJB_DYN_INTEGRATOR || d == MJB_DYN_FILTER) && h->actuator_actadr[i] >= 0 && h->actuator_actadr[i] < h->na;
}

// a sensor of the types the one-wavefront form alone evaluates (LeSens, mjb_lane_env_kernel.h): frame axes, the velocity and the acceleration stage
static bool le_extra_sensors(const mjb_model_desc *h)
{
	for (int i = 0; i < h->nsensor; i++)
		if (mjb_le::le_axis_type(h->sensor_type[i]) || mjb_le::le_vel_type(h->sensor_type[i]) || mjb_le::le_acc_type(h->sensor_type[i])) return true;
	return false;
}
// ... and a force / torque sensor whose site sits on a body at rest: the wrench table of the xfrc builds has no slot for such a body's xfrc_applied
static bool le_wrench_at_rest(const mjb_model_desc *h);

// Index of the compiled-in topology the model has, or -1 (mjb_compile; the generic kernels run every model).
int mjb_lane_env_match(const mjb_model_desc *h)
{
	if (!le_plain_tree(h) || h->nefcmax > 0) return -1;  // (joint limits are a compile-time list of rows, LeLim: such a model is hiprtc's)
	if (h->ntendon > 0 || h->neq > 0) return -1;         // (... and so are the tendons' wraps, LeTen, and the joint equalities, LeEq)
	for (int b = 1; b < h->nbody; b++)
		if (h->body_gravcomp[b] != 0) return -1;  // (gravity compensation is a compile-time flag per body, LeGc: no compiled-in topology has one set)
	if (le_extra_sensors(h)) return -1;  // (... and none carries a frame-axis, velocity- or acceleration-stage sensor, LeSens: such a model is hiprtc's)
#define MJB_LE_X(id, T) \
	if (topo_matches<T>(*h)) return id;
	MJB_LE_TOPOS(MJB_LE_X)
#undef MJB_LE_X
	return -1;
}

// ---- ONE description of a kernel variant: what the plan (le_plan, below) returns; the compiled-in dispatch, the hiprtc source, the in-process cache
// key, the block size and the LDS bytes all come from it ----
namespace {
struct LeVariant {
	int form;                 // 0 one wavefront per 64 envs, 1 two halves, 2 pipelined, 3 the sweep on three or four wavefronts (include/mjb.h)
	int sweep;                // form 3: the wavefronts of its root -> leaf sweep, 3 / 4; 0 in every other form
	int lds_kb;               // the instantiation's LDS budget LP, in pair slots = KB: 40 / 80 / 160 (form 1: 80 / 160; forms 2 and 3: 160)
	LeBuild build;            // a build other than the plain one exists in form 0 alone
	int wave_lanes;           // envs per wavefront: 64 (16 / 32: the measurement knob, plain build)
	const char *unavailable;  // non-null: there is no variant for the request, and why
};
// the variants that exist, and what tells them apart everywhere: the template flags of the compiled-in kernel, the tag of the cache key, and the two
// expressions of the hiprtc source ($ = the budget)
struct LeRow {
	int form, sweep;
	LeBuild build;
	bool pe, hw, xf;
	const char *tag, *bytes, *body;
};
constexpr LeRow le_rows[] = {
	{ 0, 0, MJB_LE_PLAIN, false, false, false, "|", "Lds<LeTopo_rt, $>::bytes()", "lane_env_body<LeTopo_rt, $>" },
	{ 0, 0, MJB_LE_OVERLAY, true, false, false, "e|", "Lds<LeTopo_rt, $>::bytes()", "lane_env_body<LeTopo_rt, $, 0, true>" },
	{ 0, 0, MJB_LE_HWSIM, false, true, false, "h|", "Lds<LeTopo_rt, $>::bytes()", "lane_env_body<LeTopo_rt, $, 0, false, true>" },
	{ 0, 0, MJB_LE_XFRC, false, false, true, "x|", "Lds<LeTopo_rt, $>::bytes()", "lane_env_body<LeTopo_rt, $, 0, false, false, true>" },
	{ 0, 0, MJB_LE_OVERLAY_XFRC, true, false, true, "ex|", "Lds<LeTopo_rt, $>::bytes()", "lane_env_body<LeTopo_rt, $, 0, true, false, true>" },
	{ 1, 0, MJB_LE_PLAIN, false, false, false, "d|", "duo_bytes<LeTopo_rt, $>()", "lane_env_duo<LeTopo_rt, $>" },
	{ 2, 0, MJB_LE_PLAIN, false, false, false, "p|", "duo2_bytes<LeTopo_rt>()", "lane_env_duo2<LeTopo_rt, 160>" },
	{ 3, 3, MJB_LE_PLAIN, false, false, false, "t|", "trio_bytes<LeTopo_rt>()", "lane_env_trio<LeTopo_rt, 160>" },
	{ 3, 4, MJB_LE_PLAIN, false, false, false, "q|", "quartet_bytes<LeTopo_rt>()", "lane_env_quartet<LeTopo_rt, 160>" },
};
constexpr const LeRow *le_row(int form, int sweep, LeBuild build)
{
	for (const LeRow &r : le_rows)
		if (r.form == form && r.sweep == sweep && r.build == build) return &r;
	return nullptr;
}
constexpr int le_block(const LeVariant &v) { return v.form == 3 ? 64 * v.sweep : (v.form ? 128 : v.wave_lanes); }  // threads of a block: 64 envs (form 0: wave_lanes)
template <class T, int LP> constexpr int le_lds_bytes(int form, int sweep)  // dynamic LDS of the compiled-in kernel
{
	return form == 3 ? (sweep == 4 ? quartet_bytes<T>() : trio_bytes<T>()) : (form == 2 ? duo2_bytes<T>() : (form == 1 ? duo_bytes<T, LP>() : Lds<T, LP>::bytes()));
}
}  // namespace

// ---- any other eligible model: the same template, compiled for the model's structure by hiprtc at its first fused launch ----
// (hiprtc is dlopen'ed: libmjb.so does not depend on it.  Whatever goes wrong -- no libhiprtc, the kernel header not next to the
//  library, a compile error -- the launch runs the generic kernel instead and the reason is kept for mjb_lane_env_info.)

// 1 when the model's structure fits the kernel (what tools/gen_lane_env_topo.py's eligible() accepts), whether or not a topology is compiled in
int mjb_lane_env_eligible(const mjb_model_desc *h)
{
	if (!le_plain_tree(h) || h->nv < 1 || h->nbody > 24 || h->nv > 20) return 0;  // (size: ~22 doubles of state per body must fit the register file)
	for (int j = 0; j < h->njnt; j++)
		if ((h->jnt_type[j] != MJB_JNT_SLIDE && h->jnt_type[j] != MJB_JNT_HINGE) || h->jnt_qposadr[j] != j || h->jnt_dofadr[j] != j || h->dof_jntid[j] != j) return 0;
	for (int b = 0; b < h->nbody; b++)
		if (h->body_jntnum[b] > 1) return 0;
	for (int i = 0; i < h->nsensor; i++) {
		const int t = h->sensor_type[i], ot = h->sensor_objtype[i];
		// on a frame (body / xbody / site), without a reference frame; on a site (velocimeter, gyro, accelerometer, force, torque)
		const bool frame = t == MJB_SENS_FRAMEPOS || t == MJB_SENS_FRAMEQUAT || mjb_le::le_axis_type(t) || t == MJB_SENS_FRAMELINVEL || t == MJB_SENS_FRAMEANGVEL ||
		                   t == MJB_SENS_FRAMELINACC || t == MJB_SENS_FRAMEANGACC;
		const bool site = t == MJB_SENS_VELOCIMETER || t == MJB_SENS_GYRO || t == MJB_SENS_ACCELEROMETER || mjb_le::le_wrench_type(t);
		if (!(frame || site || t == MJB_SENS_JOINTPOS || t == MJB_SENS_JOINTVEL || t == MJB_SENS_ACTUATORFRC || t == MJB_SENS_ACTUATORPOS || t == MJB_SENS_ACTUATORVEL ||
		      t == MJB_SENS_CLOCK))
			return 0;
		if (frame && (h->sensor_refid[i] >= 0 || (ot != MJB_OBJ_BODY && ot != MJB_OBJ_XBODY && ot != MJB_OBJ_SITE))) return 0;
		if (site && ot != MJB_OBJ_SITE) return 0;
	}
	for (int i = 0; i < h->nu; i++)
		if (!(h->actuator_trntype[i] == MJB_TRN_JOINT || (h->actuator_trntype[i] == MJB_TRN_TENDON && h->actuator_trnid[2 * i] >= 0 && h->actuator_trnid[2 * i] < h->ntendon)) ||
		    !le_dyntype_ok(h, i))
			return 0;
	int owned = 0;  // (every slot of act has its one actuator: the kernel writes a slot where it runs its owner)
	for (int i = 0; i < h->nu; i++) owned += h->actuator_dyntype[i] != MJB_DYN_NONE;
	if (owned != (h->na > 0 ? h->na : 0)) return 0;
	// (constraint rows: the packed AR and the rows' qacc_warmstart beside the state must fit the largest LDS budget -- refused here, not at the launch)
	if (h->nefcmax > 0 && le_state_slots(h->nv, mjb_lane_env_xfrc_slots(h), le_count_limits(h) + le_count_eqs(h), le_row_dofs(h)) > LE_MAX_SLOTS) {
		le_refusal = "the packed AR of the model's constraint rows needs more than 160 KB of LDS per wavefront";
		return 0;
	}
	return 1;
}
const char *mjb_lane_env_refusal(void) { return le_refusal; }

namespace {

// the model's integer structure as the LeTopo struct the kernel template takes (the text doubles as the cache key)
std::string topo_source(const mjb_model_desc &h)
{
	std::string s = "struct LeTopo_rt {\n";
	auto scalar = [&](const char *n, int v) { s += std::string("\tstatic constexpr int ") + n + " = " + std::to_string(v) + ";\n"; };
	auto arr = [&](const char *n, int count, auto get) {
		s += std::string("\tstatic constexpr int ") + n + "[" + std::to_string(count > 0 ? count : 1) + "] = { ";
		for (int i = 0; i < (count > 0 ? count : 1); i++) s += (i ? ", " : "") + std::to_string(count > 0 ? (int)get(i) : 0);
		s += " };\n";
	};
	scalar("NBODY", h.nbody); scalar("NQ", h.nq); scalar("NV", h.nv); scalar("NU", h.nu); scalar("NA", h.na); scalar("NJNT", h.njnt); scalar("NSITE", h.nsite);
	scalar("NSENSOR", h.nsensor); scalar("NSENSORDATA", h.nsensordata); scalar("NM", h.nM);
	arr("body_parentid", h.nbody, [&](int i) { return h.body_parentid[i]; });
	arr("body_rootid", h.nbody, [&](int i) { return h.body_rootid[i]; });
	arr("body_jnt", h.nbody, [&](int i) { return h.body_jntnum[i] == 1 ? h.body_jntadr[i] : -1; });
	arr("body_sameframe", h.nbody, [&](int i) { return h.body_sameframe[i] != 0; });
	arr("body_gc", h.nbody, [&](int i) { return i > 0 && h.body_gravcomp[i] != 0; });
	arr("jnt_type", h.njnt, [&](int i) { return h.jnt_type[i]; });
	arr("jnt_bodyid", h.njnt, [&](int i) { return h.jnt_bodyid[i]; });
	arr("jnt_offc", h.njnt, [&](int i) { return le_jnt_offc(h, i); });
	arr("dof_parentid", h.nv, [&](int i) { return h.dof_parentid[i]; });
	arr("dof_Madr", h.nv, [&](int i) { return h.dof_Madr[i]; });
	arr("act_jnt", h.nu, [&](int i) { return h.actuator_trnid[2 * i]; });
	arr("act_gaintype", h.nu, [&](int i) { return h.actuator_gaintype[i]; });
	arr("act_biastype", h.nu, [&](int i) { return h.actuator_biastype[i]; });
	arr("act_ctrllimited", h.nu, [&](int i) { return h.actuator_ctrllimited[i] != 0; });
	arr("act_forcelimited", h.nu, [&](int i) { return h.actuator_forcelimited[i] != 0; });
	arr("act_dyntype", h.nu, [&](int i) { return h.actuator_dyntype[i]; });
	arr("act_actadr", h.nu, [&](int i) { return h.na > 0 ? h.actuator_actadr[i] : 0; });
	arr("act_actlimited", h.nu, [&](int i) { return h.na > 0 && h.actuator_actlimited[i] != 0; });
	arr("site_bodyid", h.nsite, [&](int i) { return h.site_bodyid[i]; });
	arr("site_sameframe", h.nsite, [&](int i) { return h.site_sameframe[i] != 0; });
	arr("sensor_type", h.nsensor, [&](int i) { return h.sensor_type[i]; });
	arr("sensor_objtype", h.nsensor, [&](int i) { return h.sensor_objtype[i]; });
	arr("sensor_objid", h.nsensor, [&](int i) { return h.sensor_objid[i]; });
	arr("sensor_adr", h.nsensor, [&](int i) { return h.sensor_adr[i]; });
	if (h.nefcmax > 0) arr("jnt_limited", h.njnt, [&](int i) { return h.jnt_limited[i] != 0 && !(h.disableflags & MJB_DSBL_LIMIT); });  // (the rows of the constraint stage, LeLim: a model without them has no such line)
	if (h.ntendon > 0) {  // (fixed tendons, LeTen: which actuators drive one, and every tendon's wraps -- a model without tendons has none of these lines)
		arr("act_trntype", h.nu, [&](int i) { return h.actuator_trntype[i]; });
		arr("act_tendon", h.nu, [&](int i) { return h.actuator_trntype[i] == MJB_TRN_TENDON ? h.actuator_trnid[2 * i] : -1; });
		arr("tendon_adr", h.ntendon, [&](int i) { return h.tendon_adr[i]; });
		arr("tendon_num", h.ntendon, [&](int i) { return h.tendon_num[i]; });
		arr("wrap_jnt", h.nwrap, [&](int i) { return h.wrap_objid[i]; });
	}
	if (h.nefcmax > 0 && !(h.disableflags & MJB_DSBL_EQUALITY)) {  // (the equality rows, LeEq: the joint pairs of the ACTIVE joint equalities, -1 = the one-joint form)
		std::vector<int> e1, e2;
		for (int e = 0; e < h.neq; e++)
			if (h.eq_active[e]) e1.push_back(h.eq_obj1id[e]), e2.push_back(h.eq_obj2id[e] >= 0 ? h.eq_obj2id[e] : -1);
		if (!e1.empty()) {
			arr("eq_jnt1", (int)e1.size(), [&](int i) { return e1[i]; });
			arr("eq_jnt2", (int)e2.size(), [&](int i) { return e2[i]; });
		}
	}
	s += "};\n";
	return s;
}

struct RtcApi {
	void *lib = nullptr;
	int (*create)(void **, const char *, const char *, int, const char **, const char **) = nullptr;
	int (*compile)(void *, int, const char **) = nullptr;
	int (*log_size)(void *, size_t *) = nullptr;
	int (*log)(void *, char *) = nullptr;
	int (*code_size)(void *, size_t *) = nullptr;
	int (*code)(void *, char *) = nullptr;
	int (*destroy)(void **) = nullptr;
	bool ok = false;
};
RtcApi &rtc()
{
	static RtcApi a = [] {
		RtcApi r;
		for (const char *n : { "libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so" }) {
			r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
			if (r.lib) break;
		}
		if (!r.lib) return r;
		r.create = (decltype(r.create))dlsym(r.lib, "hiprtcCreateProgram");
		r.compile = (decltype(r.compile))dlsym(r.lib, "hiprtcCompileProgram");
		r.log_size = (decltype(r.log_size))dlsym(r.lib, "hiprtcGetProgramLogSize");
		r.log = (decltype(r.log))dlsym(r.lib, "hiprtcGetProgramLog");
		r.code_size = (decltype(r.code_size))dlsym(r.lib, "hiprtcGetCodeSize");
		r.code = (decltype(r.code))dlsym(r.lib, "hiprtcGetCode");
		r.destroy = (decltype(r.destroy))dlsym(r.lib, "hiprtcDestroyProgram");
		r.ok = r.create && r.compile && r.log_size && r.log && r.code_size && r.code && r.destroy;
		return r;
	}();
	return a;
}

struct JitKernel {
	hipModule_t mod = nullptr;
	hipFunction_t fn = nullptr;
	std::string error;  // non-empty: not available, why
};
std::mutex jit_mutex;
std::map<std::string, JitKernel> jit_cache;  // key: device | LDS budget, the variant's tag (le_rows) | topology text
std::string jit_last_error;  // guarded by jit_err_mutex; mjb_lane_env_jit_error() hands out a thread-local copy
std::mutex jit_err_mutex;
void set_jit_error(const std::string &e)
{
	std::lock_guard<std::mutex> lock(jit_err_mutex);
	jit_last_error = e;
}
// gfx target of the device the kernel is built for (the in-tree build's $(ARCH) is gfx950; a hiprtc build follows the device it runs on)
std::string device_arch(int dev)
{
	hipDeviceProp_t p;
	if (hipGetDeviceProperties(&p, dev) != hipSuccess) return "gfx950";
	std::string a = p.gcnArchName;
	const size_t c = a.find(':');
	return c == std::string::npos ? a : a.substr(0, c);
}

// directory of the kernel header: next to libmjb.so (the in-tree build), or MJB_LANE_ENV_SRC
std::string source_dir()
{
	if (const char *v = getenv("MJB_LANE_ENV_SRC")) return v;
	Dl_info info;
	if (dladdr((const void *)&mjb_lane_env_eligible, &info) && info.dli_fname) {
		std::string p = info.dli_fname;
		const size_t k = p.rfind('/');
		return k == std::string::npos ? "." : p.substr(0, k);
	}
	return ".";
}

// ---- on-disk cache of the hiprtc builds: a new model's first eligible launch costs ~3 s of compilation per LDS budget and form; the code
// object is kept under $MJB_JIT_CACHE (default $XDG_CACHE_HOME/mjb_jit or ~/.cache/mjb_jit; MJB_JIT_CACHE=0 turns it off) in a file named by a hash of
// everything the build depends on: gfx arch, the TEXT of every header the source includes (the source fingerprint), LDS budget, form, the topology.
std::atomic<int> jit_compiled{ 0 }, jit_disk_hits{ 0 };
unsigned long long fnv1a(unsigned long long hsh, const std::string &t)
{
	for (unsigned char c : t) {
		hsh ^= c;
		hsh *= 1099511628211ull;
	}
	return hsh;
}
bool read_file(const std::string &path, std::string &out)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	char buf[65536];
	size_t n;
	out.clear();
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
	fclose(f);
	return true;
}
std::string cache_dir()
{
	if (const char *v = getenv("MJB_JIT_CACHE")) return (*v == '0' && !v[1]) ? std::string() : std::string(v);
	if (const char *x = getenv("XDG_CACHE_HOME")) if (*x) return std::string(x) + "/mjb_jit";
	if (const char *hm = getenv("HOME")) if (*hm) return std::string(hm) + "/.cache/mjb_jit";
	return "/tmp/mjb_jit";
}
void make_dirs(const std::string &d)
{
	for (size_t k = 1; k <= d.size(); k++)
		if (k == d.size() || d[k] == '/') (void)mkdir(d.substr(0, k).c_str(), 0755);
}
// hash of the headers the generated source pulls in (a changed kernel header or data-field list invalidates every cached build)
bool source_fingerprint(const std::string &dir, unsigned long long &hsh)
{
	static const char *files[] = { "/mjb_lane_env_kernel.h", "/mjb_dev.h", "/mjb_math.h", "/../../include/mjb.h", "/../../include/mjb_model_fields.def",
		                           "/../../include/mjb_data_fields.def" };
	hsh = 1469598103934665603ull;
	std::string text;
	for (const char *f : files) {
		if (!read_file(dir + f, text)) return false;
		hsh = fnv1a(hsh, text);
	}
	return true;
}

// the source hiprtc compiles for a variant: the kernel header, the topology, one kernel `le_rt` with the variant's launch bounds, LDS and body
std::string jit_source(const LeRow &r, const LeVariant &v, const std::string &topo)
{
	auto with_budget = [&](std::string t) {
		const size_t at = t.find('$');
		return at == std::string::npos ? t : t.replace(at, 1, std::to_string(v.lds_kb));
	};
	return "#include \"mjb_lane_env_kernel.h\"\n" + topo + "extern \"C\" __global__ void __launch_bounds__(" + std::to_string(v.form ? le_block(v) : 64) +
	       ") le_rt(const KernelParams MJB_AS4 *P, int nsteps, unsigned int step0, int lo, int hi)\n{\n"
	       "\t__shared__ __attribute__((aligned(16))) unsigned char smem[mjb_le::" + with_budget(r.bytes) + "];\n"
	       "\tmjb_le::" + with_budget(r.body) + "(P, nsteps, step0, lo, hi, smem);\n}\n";
}

const JitKernel &jit_get(const mjb_model_desc &h, const LeVariant &v)
{
	static const JitKernel no_such_variant{ nullptr, nullptr, "no such variant of the kernel" };
	const LeRow *const row = le_row(v.form, v.sweep, v.build);
	if (!row) return no_such_variant;  // (never from le_plan)
	int dev = 0;
	(void)hipGetDevice(&dev);
	const std::string topo = topo_source(h);
	const std::string key = std::to_string(dev) + "|" + std::to_string(v.lds_kb) + row->tag + topo;
	std::lock_guard<std::mutex> lock(jit_mutex);
	auto it = jit_cache.find(key);
	if (it != jit_cache.end()) return it->second;
	JitKernel &k = jit_cache[key];
	static const bool off = [] { const char *e = getenv("MJB_LANE_ENV_JIT"); return e && *e == '0'; }();
	if (off) { k.error = "disabled (MJB_LANE_ENV_JIT=0)"; return k; }
	RtcApi &r = rtc();
	if (!r.ok) { k.error = "libhiprtc.so not found"; return k; }
	const std::string dir = source_dir();
	const std::string src = jit_source(*row, v, topo);
	// the disk cache first
	std::string cpath;
	{
		const std::string cdir = cache_dir();
		unsigned long long fp = 0;
		if (!cdir.empty() && source_fingerprint(dir, fp)) {
			unsigned long long hk = fnv1a(fnv1a(fnv1a(fp, device_arch(dev)), src), "O3 fp-contract=fast no-machine-licm v1");
			char name[64];
			snprintf(name, sizeof name, "/le_%016llx.hsaco", hk);
			cpath = cdir + name;
			std::string blob;
			if (read_file(cpath, blob) && blob.size() > 64) {
				if (hipModuleLoadData(&k.mod, blob.data()) == hipSuccess && hipModuleGetFunction(&k.fn, k.mod, "le_rt") == hipSuccess) {
					jit_disk_hits++;
					return k;
				}
				(void)hipGetLastError();  // (a truncated or foreign file: rebuilt and overwritten below)
				k.mod = nullptr;
				k.fn = nullptr;
			}
		}
	}
	void *prog = nullptr;
	if (r.create(&prog, src.c_str(), "mjb_lane_env_rt.hip", 0, nullptr, nullptr) != 0) { k.error = "hiprtcCreateProgram failed"; return k; }
	const std::string i1 = "-I" + dir, i2 = "-I" + dir + "/../../include";
	const std::string archopt = "--offload-arch=" + device_arch(dev);
	const char *opts[] = { archopt.c_str(), "-O3", "-std=c++17", "-ffp-contract=fast", "-mllvm", "-disable-machine-licm", i1.c_str(), i2.c_str() };
	const int crc = r.compile(prog, (int)(sizeof opts / sizeof *opts), opts);
	if (crc != 0) {
		size_t n = 0;
		r.log_size(prog, &n);
		std::string log(n + 1, '\0');
		if (n) r.log(prog, &log[0]);
		k.error = "hiprtc compile failed: " + log.substr(0, 600);
		r.destroy(&prog);
		return k;
	}
	size_t n = 0;
	r.code_size(prog, &n);
	std::vector<char> code(n);
	r.code(prog, code.data());
	r.destroy(&prog);
	jit_compiled++;
	if (!cpath.empty()) {  // (written under a temporary name and renamed: a concurrent process never reads half a file)
		make_dirs(cpath.substr(0, cpath.rfind('/')));
		const std::string tmp = cpath + "." + std::to_string((long long)getpid()) + ".tmp";
		FILE *f = fopen(tmp.c_str(), "wb");
		if (f) {
			const bool okw = fwrite(code.data(), 1, code.size(), f) == code.size();
			fclose(f);
			if (!okw || rename(tmp.c_str(), cpath.c_str()) != 0) (void)remove(tmp.c_str());
		}
	}
	if (hipModuleLoadData(&k.mod, code.data()) != hipSuccess || hipModuleGetFunction(&k.fn, k.mod, "le_rt") != hipSuccess) {
		(void)hipGetLastError();
		k.error = "hipModuleLoadData / hipModuleGetFunction failed";
		k.mod = nullptr;
		k.fn = nullptr;
	}
	return k;
}

}  // namespace

namespace {
// CU count and the kernels' LDS attribute, cached per device (hipFuncSetAttribute acts on the current device's copy of the function)
int device_cus(int dev)
{
	static std::mutex mu;
	static std::map<int, int> cus;
	std::lock_guard<std::mutex> lock(mu);
	auto it = cus.find(dev);
	if (it != cus.end()) return it->second;
	int c = 0;
	if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 0;
	cus[dev] = c;
	return c;
}
hipError_t lds_attr_once(const void *fn, int bytes, int dev)
{
	if (bytes <= 65536) return hipSuccess;
	static std::mutex mu;
	static std::map<std::pair<const void *, int>, hipError_t> done;
	std::lock_guard<std::mutex> lock(mu);
	auto key = std::make_pair(fn, dev);
	auto it = done.find(key);
	if (it != done.end()) return it->second;
	const hipError_t r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
	done[key] = r;
	return r;
}
}  // namespace

void mjb_lane_env_jit_stats(int *compiled, int *disk_hits)
{
	if (compiled) *compiled = jit_compiled.load();
	if (disk_hits) *disk_hits = jit_disk_hits.load();
}

const char *mjb_lane_env_jit_error(void)
{
	thread_local std::string copy;
	std::lock_guard<std::mutex> lock(jit_err_mutex);
	copy = jit_last_error;
	return copy.c_str();
}

// process-wide choice of the kernel's FORM (include/mjb.h): -1 = by batch size (default; MJB_LANE_ENV_DUO overrides), 0 / 1 / 2
static std::atomic<int> le_form_override{ -1 }, le_form_last{ -1 };
// ... and, of form 3, of the wavefronts its root -> leaf sweep runs on: 0 = by the rule below (default; MJB_LANE_ENV_SWEEP_WAVES overrides), 3 / 4
static std::atomic<int> le_sweep_override{ 0 }, le_sweep_last{ 0 };
int mjb_lane_env_set_sweep_waves(int waves)
{
	return le_sweep_override.exchange((waves == 3 || waves == 4) ? waves : 0);
}
int mjb_lane_env_last_sweep_waves(void) { return le_sweep_last; }
int mjb_lane_env_set_form(int form)
{
	return le_form_override.exchange((form >= 0 && form <= 3) ? form : -1);
}
int mjb_lane_env_last_form(void) { return le_form_last; }

size_t mjb_lane_env_tape_doubles(const mjb_model_desc *h)
{
	// (constraint rows: a header, a record per limited joint and one per active joint equality behind the rest; fixed tendons: a record per wrap behind those)
	const int nl = mjb_lane_env_limits(h), ne = mjb_lane_env_eq_rows(h), nw = mjb_lane_env_solo_only(h) && h->ntendon > 0 ? h->nwrap : 0;
	return (sizeof(LeTapeHdr) + (size_t)h->nbody * sizeof(LeTapeBody) + (size_t)h->nu * sizeof(LeTapeAct) +
	        (nl + ne > 0 ? sizeof(LeTapeLimHdr) + (size_t)nl * sizeof(LeTapeLim) + (size_t)ne * sizeof(LeTapeEq) : 0) + (size_t)nw * sizeof(LeTapeWrap)) /
	       sizeof(double);
}

// Ib = R(iquat) diag(inertia) R(iquat)': xx yy zz xy xz yz
static void le_ibody(const double *q, const double *in, double *ibody)
{
	double R[9];
	const double q00 = q[0] * q[0], q01 = q[0] * q[1], q02 = q[0] * q[2], q03 = q[0] * q[3], q11 = q[1] * q[1], q12 = q[1] * q[2], q13 = q[1] * q[3],
	             q22 = q[2] * q[2], q23 = q[2] * q[3], q33 = q[3] * q[3];
	R[0] = q00 + q11 - q22 - q33; R[4] = q00 - q11 + q22 - q33; R[8] = q00 - q11 - q22 + q33;
	R[1] = 2 * (q12 - q03); R[2] = 2 * (q13 + q02); R[3] = 2 * (q12 + q03); R[5] = 2 * (q23 - q01); R[6] = 2 * (q13 - q02); R[7] = 2 * (q23 + q01);
	auto e = [&](int r, int c) { return R[3 * r] * in[0] * R[3 * c] + R[3 * r + 1] * in[1] * R[3 * c + 1] + R[3 * r + 2] * in[2] * R[3 * c + 2]; };
	ibody[0] = e(0, 0); ibody[1] = e(1, 1); ibody[2] = e(2, 2); ibody[3] = e(0, 1); ibody[4] = e(0, 2); ibody[5] = e(1, 2);
}

// ---- the per-env overlay of the PE kernels (PeSlots, mjb_lane_env_kernel.h): one env's column, in slot order ----
static bool le_moving(const mjb_model_desc *h, int b)  // a joint on the body's path to the world
{
	for (int a = b; a > 0; a = h->body_parentid[a])
		if (h->body_jntnum[a] > 0) return true;
	return false;
}
int mjb_lane_env_wrench_at_rest(const mjb_model_desc *h) { return h && le_wrench_at_rest(h) ? 1 : 0; }
static bool le_wrench_at_rest(const mjb_model_desc *h)
{
	for (int i = 0; i < h->nsensor; i++)
		if (mjb_le::le_wrench_type(h->sensor_type[i]) && h->sensor_objtype[i] == MJB_OBJ_SITE && !le_moving(h, h->site_bodyid[h->sensor_objid[i]])) return true;
	return false;
}
int mjb_lane_env_overlay_slots(const mjb_model_desc *h)
{
	int nj = 0, nm = 0;
	for (int b = 1; b < h->nbody; b++) {
		nj += h->body_jntnum[b] == 1;
		nm += le_moving(h, b);
	}
	return 3 + 4 * nj + 7 * nm + 6 * h->nu + (h->nbody - 1 - nm);
}
// ---- the wrench table of the XF kernels (XfSlots, mjb_lane_env_kernel.h): a slot per moving body, in body order ----
int mjb_lane_env_xfrc_slots(const mjb_model_desc *h)
{
	int nm = 0;
	for (int b = 1; b < h->nbody; b++) nm += le_moving(h, b);
	return nm;
}
namespace {
struct XfMap { int body[24], n; };  // (mjb_lane_env_eligible: at most 24 bodies)
// one thread per (env, slot): the six doubles of a wrench to six rows; consecutive threads = consecutive envs, the stores coalesce
__global__ void mjb_le_xfrc_fill_kernel(const double *__restrict__ xfrc, double *__restrict__ table, const XfMap map, const int nbody, const int nenv)
{
	const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x), sl = (int)blockIdx.y;
	if (env >= nenv || sl >= map.n) return;
	const double *src = xfrc + ((size_t)env * nbody + map.body[sl]) * 6;
	for (int k = 0; k < 6; k++) table[(size_t)(6 * sl + k) * nenv + env] = src[k];
}
}  // namespace
int mjb_lane_env_xfrc_fill(const mjb_model_desc *h, const double *xfrc_applied, double *table, int nenv, void *stream)
{
	XfMap map{};
	for (int b = 1; b < h->nbody && map.n < 24; b++)
		if (le_moving(h, b)) map.body[map.n++] = b;
	if (map.n == 0 || nenv <= 0) return 0;
	hipLaunchKernelGGL(mjb_le_xfrc_fill_kernel, dim3((unsigned int)((nenv + 255) / 256), (unsigned int)map.n), dim3(256), 0, (hipStream_t)stream, xfrc_applied, table,
	                   map, h->nbody, nenv);
	return (int)hipGetLastError();
}
// gravity: the env's (NULL: the model's); env_block: the env's block of DevState::env_mass, mass and joint section (NULL: the model's values)
void mjb_lane_env_overlay_row(const mjb_model_desc *h, const double *gravity, const double *env_block, double *out)
{
	const int nb = h->nbody;
	const EnvBlockLayout B = mjb_env_block_layout(*h);
	const double *mass = env_block ? env_block + B.body_mass : h->body_mass, *inertia = env_block ? env_block + B.body_inertia : h->body_inertia;
	const double *damping = env_block ? env_block + B.dof_damping : h->dof_damping, *armature = env_block ? env_block + B.dof_armature : h->dof_armature;
	const double *stiffness = env_block ? env_block + B.jnt_stiffness : h->jnt_stiffness;
	const double *gain = env_block ? env_block + B.actuator_gainprm : h->actuator_gainprm, *bias = env_block ? env_block + B.actuator_biasprm : h->actuator_biasprm;
	double *o = out;
	for (int k = 0; k < 3; k++) *o++ = gravity ? gravity[k] : h->gravity[k];
	for (int b = 1; b < nb; b++)
		if (h->body_jntnum[b] == 1) {
			const int j = h->body_jntadr[b], da = h->jnt_dofadr[j];
			*o++ = stiffness[j];
			*o++ = damping[da];
			*o++ = armature[da];
			*o++ = h->timestep[0] * damping[da];
		}
	for (int b = 1; b < nb; b++)
		if (le_moving(h, b)) {
			*o++ = mass[b];
			le_ibody(h->body_iquat + 4 * b, inertia + 3 * b, o);
			o += 6;
		}
	for (int i = 0; i < h->nu; i++) {
		for (int k = 0; k < 3; k++) *o++ = gain[3 * i + k];
		for (int k = 0; k < 3; k++) *o++ = bias[3 * i + k];
	}
	for (int b = 1; b < nb; b++)
		if (!le_moving(h, b)) *o++ = mass[b];
}

void mjb_lane_env_tape(const mjb_model_desc *h, double *tape)
{
	LeTapeHdr *th = reinterpret_cast<LeTapeHdr *>(tape);
	LeTapeBody *tb = reinterpret_cast<LeTapeBody *>(th + 1);
	LeTapeAct *ta = reinterpret_cast<LeTapeAct *>(tb + h->nbody);
	th->dt = h->timestep[0];
	for (int k = 0; k < 3; k++) th->gravity[k] = h->gravity[k];
	for (int b = 0; b < h->nbody; b++) {
		LeTapeBody &t = tb[b];
		for (int k = 0; k < 3; k++) { t.pos[k] = h->body_pos[3 * b + k]; t.ipos[k] = h->body_ipos[3 * b + k]; }
		for (int k = 0; k < 4; k++) t.quat[k] = h->body_quat[4 * b + k];
		le_ibody(h->body_iquat + 4 * b, h->body_inertia + 3 * b, t.ibody);
		t.mass = h->body_mass[b];
		t.gravcomp = h->body_gravcomp[b];  // (gravity compensation: read where the topology flags the body, LeGc)
		if (h->body_jntnum[b] == 1) {
			const int j = h->body_jntadr[b];
			for (int k = 0; k < 3; k++) { t.jaxis[k] = h->jnt_axis[3 * j + k]; t.jpos[k] = h->jnt_pos[3 * j + k]; }
			const int qa = h->jnt_qposadr[j], da = h->jnt_dofadr[j];  // (== j for the lane = env topologies; the split step's smooth kernel reads the tape of models with free / ball joints too: their first coordinate)
			t.qpos0 = h->qpos0[qa];
			t.stiffness = h->jnt_stiffness[j];
			t.spring = h->qpos_spring[qa];
			t.damping = h->dof_damping[da];
			t.armature = h->dof_armature[da];
			t.hdamping = h->timestep[0] * h->dof_damping[da];
		}
	}
	for (int i = 0; i < h->nu; i++) {
		LeTapeAct &a = ta[i];
		a.gear = h->actuator_gear[6 * i];
		a.ctrllo = h->actuator_ctrlrange[2 * i];
		a.ctrlhi = h->actuator_ctrlrange[2 * i + 1];
		for (int k = 0; k < 3; k++) { a.gain[k] = h->actuator_gainprm[3 * i + k]; a.bias[k] = h->actuator_biasprm[3 * i + k]; }
		a.forcelo = h->actuator_forcerange[2 * i];
		a.forcehi = h->actuator_forcerange[2 * i + 1];
		if (h->na > 0 && h->actuator_actadr[i] >= 0) {  // (an activation state: the filter's time constant as act_dot divides by it, and actrange)
			if (h->actuator_dyntype[i] == MJB_DYN_FILTER) a.dyntau = h->actuator_dynprm[3 * i] > MJB_MINVAL ? h->actuator_dynprm[3 * i] : MJB_MINVAL;
			a.actlo = h->actuator_actrange[2 * i];
			a.acthi = h->actuator_actrange[2 * i + 1];
		}
	}
	// getsolparam + mj_makeImpedance's constants of one row: a mixed-sign solref is replaced by the default, refsafe, solimp clamped to its legal ranges
	// (mjMINIMP, mjMAXIMP, width >= 0, power >= 1); K, B the row's stiffness and damping; powa, powb the two constant factors of the impedance curve
	auto solparam = [&](const double *sr_in, const double *si, double *solref, double *solimp, double &K, double &B, double &powa, double &powb) {
		double sr[2] = { sr_in[0], sr_in[1] };
		if ((sr[0] > 0) != (sr[1] > 0)) sr[0] = 0.02, sr[1] = 1.0;
		if (!(h->disableflags & MJB_DSBL_REFSAFE) && sr[0] > 0) sr[0] = fmax(sr[0], 2 * h->timestep[0]);
		const double imp[5] = { fmin(0.9999, fmax(0.0001, si[0])), fmin(0.9999, fmax(0.0001, si[1])), fmax(0.0, si[2]), fmin(0.9999, fmax(0.0001, si[3])), fmax(1.0, si[4]) };
		solref[0] = sr[0], solref[1] = sr[1];
		for (int k = 0; k < 5; k++) solimp[k] = imp[k];
		if (sr[0] > 0) {
			K = 1 / fmax(MJB_MINVAL, imp[1] * imp[1] * sr[0] * sr[0] * sr[1] * sr[1]);
			B = 2 / fmax(MJB_MINVAL, imp[1] * sr[0]);
		} else {
			K = -sr[0] / fmax(MJB_MINVAL, imp[1] * imp[1]);
			B = -sr[1] / fmax(MJB_MINVAL, imp[1]);
		}
		powa = 1 / pow(imp[3], imp[4] - 1);
		powb = 1 / pow(1 - imp[3], imp[4] - 1);
	};
	const int nlim = mjb_lane_env_limits(h), neqr = mjb_lane_env_eq_rows(h);
	unsigned char *behind = reinterpret_cast<unsigned char *>(ta + h->nu);
	if (nlim + neqr > 0) {
		LeTapeLimHdr *lh = reinterpret_cast<LeTapeLimHdr *>(behind);
		LeTapeLim *tl = reinterpret_cast<LeTapeLim *>(lh + 1);
		lh->meaninertia = h->meaninertia[0];
		lh->tolerance = h->tolerance[0];
		lh->iterations = h->iterations;
		lh->scale = 1.0 / (h->meaninertia[0] * (h->nv > 1 ? h->nv : 1));
		lh->nowarm = (h->disableflags & MJB_DSBL_WARMSTART) ? 1.0 : 0.0;
		lh->norefsafe = (h->disableflags & MJB_DSBL_REFSAFE) ? 1.0 : 0.0;
		for (int j = 0; j < h->njnt && nlim > 0; j++) {
			if (!h->jnt_limited[j]) continue;
			LeTapeLim &l = *tl++;
			l.range[0] = h->jnt_range[2 * j];
			l.range[1] = h->jnt_range[2 * j + 1];
			l.margin = h->jnt_margin[j];
			solparam(h->jnt_solref + 2 * j, h->jnt_solimp + 5 * j, l.solref, l.solimp, l.K, l.B, l.powa, l.powb);
			l.invweight0 = h->dof_invweight0[h->jnt_dofadr[j]];
		}
		LeTapeEq *te = reinterpret_cast<LeTapeEq *>(tl);
		for (int e = 0; e < h->neq && neqr > 0; e++) {
			if (!h->eq_active[e]) continue;
			LeTapeEq &q = *te++;
			const int j1 = h->eq_obj1id[e], j2 = h->eq_obj2id[e];
			for (int k = 0; k < 5; k++) q.polycoef[k] = h->eq_data[11 * e + k];
			q.qpos0[0] = h->qpos0[h->jnt_qposadr[j1]];
			q.qpos0[1] = j2 >= 0 ? h->qpos0[h->jnt_qposadr[j2]] : 0.0;
			solparam(h->eq_solref + 2 * e, h->eq_solimp + 5 * e, q.solref, q.solimp, q.K, q.B, q.powa, q.powb);
			q.invweight0 = h->dof_invweight0[h->jnt_dofadr[j1]] + (j2 >= 0 ? h->dof_invweight0[h->jnt_dofadr[j2]] : 0.0);
		}
		behind = reinterpret_cast<unsigned char *>(te);
	}
	if (mjb_lane_env_solo_only(h) && h->ntendon > 0) {
		LeTapeWrap *tw = reinterpret_cast<LeTapeWrap *>(behind);
		for (int w = 0; w < h->nwrap; w++) tw[w].coef = h->wrap_prm[w];
	}
}

const char *mjb_lane_env_name(int topo)
{
#define MJB_LE_X(id, T) \
	if (topo == id) return T::name;
	MJB_LE_TOPOS(MJB_LE_X)
#undef MJB_LE_X
	return "";
}

// ---- THE PLAN: which variant a launch runs, as a pure function of what it is given -- no environment variable, no atomic, no device is read here
// (mjb_launch_lane_env gathers them; mjb_lane_env_plan, the introspection entry, and tests/test_lane_env_plan.py call it with values of their own) ----
namespace {
struct LePlanIn {
	int ncu;            // CUs of the device (0: not known -- the leanest budget, one wavefront)
	int nenv_batch;     // envs of the BATCH, not of the launch's range: the instantiations agree to rounding, not bit for bit (the compiler contracts a few
	                    // multiply-adds differently around where data waits), so every launch of a batch -- whole, a prefix, the rest of a split step -- runs one
	LeBuild build;
	int form;           // -1: by batch size; 0: one wavefront always; 1 / 2 / 3: that form whenever the LDS allows (mjb_lane_env_set_form, else MJB_LANE_ENV_DUO)
	int duo_max_waves;  // the automatic rule runs more than one wavefront per 64 envs up to this many wavefronts of envs; -1: 2 x CUs (MJB_LANE_ENV_DUO_MAX_WAVES)
	int sweep;          // form 3's sweep wavefronts, 3 / 4; 0: by batch size (mjb_lane_env_set_sweep_waves, else MJB_LANE_ENV_SWEEP_WAVES)
	int lds_kb;         // 40 / 80 / 160; anything else: by batch size (MJB_LANE_ENV_LDS_KB)
	int wave_lanes;     // 16 / 32: envs per wavefront of the plain one-wavefront form; anything else: 64 (MJB_LANE_ENV_WAVE_LANES)
	bool fit;           // a hiprtc-built model: the layouts are counted for it, and what does not fit a CU's LDS steps down
	int nv, nmov, nbody;  // ... from these: dofs, moving bodies (mjb_lane_env_xfrc_slots), bodies
	int na;             // ... and its activation states: the one-wavefront form alone carries them, and no build with the hwsim stage
	bool gc;            // ... and whether a body has gravity compensation: the one-wavefront form alone has the term, in every build
	bool sens;          // ... and whether it has a frame-axis, velocity- or acceleration-stage sensor (LeSens): the one-wavefront form alone evaluates them, in every build
	bool wrench_rest;   // ... one of them a force / torque sensor on a body at rest: not in the xfrc builds, whose wrench table has no slot for such a body
	int nl;             // ... and its constraint rows (mjb_lane_env_eq_rows + mjb_lane_env_limits): the plain build of the one-wavefront form alone has the constraint stage
	int nwd;            // ... the dofs those rows touch (their qacc_warmstart lives in LDS beside the packed AR)
	bool solo;          // ... rows or fixed tendons (mjb_lane_env_solo_only): form 0 of the plain build and no other variant
};

LeVariant le_plan(const LePlanIn &in)
{
	LeVariant v{ 0, 0, 0, in.build, 64, nullptr };
	const bool plain = in.build == MJB_LE_PLAIN;
	if (plain && !in.solo && (in.wave_lanes == 16 || in.wave_lanes == 32)) v.wave_lanes = in.wave_lanes;  // (the overlay, hwsim and xfrc builds always run full wavefronts)
	// the LDS budget per wavefront from the CUs the batch leaves idle: one wavefront per CU may take all of its LDS, two half of it each
	const int ncu = in.ncu, waves = (in.nenv_batch + 63) / 64;
	v.lds_kb = (in.lds_kb == 40 || in.lds_kb == 80 || in.lds_kb == 160) ? in.lds_kb : ((ncu > 0 && waves <= ncu) ? 160 : ((ncu > 0 && waves <= 2 * ncu) ? 80 : 40));
	// the form: more than one wavefront per 64 envs in the plain build alone.  A model with activation states (act lives in the registers of the one
	// wavefront that assembles the forces and integrates), gravity compensation (the one-wavefront form alone has the term) or a sensor beyond poses and
	// joint / actuator scalars (the one-wavefront form alone has the velocity sensors in its sweep and the pass behind the qacc solve) -- always hiprtc's --
	// is planned as if form 0 had been asked for, whatever is: the same budget and lanes per wavefront as that request
	const int form = (in.fit && (in.na > 0 || in.gc || in.sens || in.solo)) ? 0 : in.form;
	if (plain && form > 0 && v.lds_kb < 80) {
		// a forced multi-wavefront form on a batch that would run four wavefronts per CU: the two halves at two per CU
		v.form = 1;
		v.lds_kb = 80;
	} else if (plain && v.wave_lanes == 64 && v.lds_kb >= 80 && form != 0 && (form > 0 || waves <= (in.duo_max_waves >= 0 ? in.duo_max_waves : 2 * ncu))) {
		// two wavefronts per 64 envs while the batch leaves at least every second SIMD idle: the step's position half and velocity half side by side ...
		v.form = 1;
		// ... pipelined (nothing computed twice) when a workgroup has a CU's LDS to itself; form 1 asked for: the two halves only
		if (v.lds_kb == 160 && form != 1) v.form = 2;
		// ... and three wavefronts (the pose chain alone on the first) while three SIMDs per block are there: the same LDS layout, so the same bound
		if (v.form == 2 && form != 2 && 3 * waves <= 4 * ncu) v.form = 3;
		// ... its sweep on four when the block still has a SIMD of its CU to itself per wavefront: the pose wavefront's chain cut in two
		if (v.form == 3) v.sweep = (in.sweep == 3 || in.sweep == 4) ? in.sweep : (waves <= ncu ? 4 : 3);
	}  // (otherwise -- the overlay / hwsim / xfrc builds whatever is asked for -- the solo form at that budget)
	if (!in.fit) return v;
	if (in.na > 0 && in.build == MJB_LE_HWSIM) {
		v.unavailable = "no build of the kernel has both the hwsim stage and activation states";
		return v;
	}
	if (in.wrench_rest && (in.build == MJB_LE_XFRC || in.build == MJB_LE_OVERLAY_XFRC)) {
		v.unavailable = "no xfrc build of the kernel has a force / torque sensor on a body at rest: the wrench table has no slot for that body";
		return v;
	}
	if (in.solo && !plain) {
		v.unavailable = "no overlay, hwsim or xfrc build of the kernel has the constraint stage or the tendon actuators of a model with constraint rows or fixed tendons";
		return v;
	}
	// a hiprtc-built model may be larger than the compiled-in ones: the smallest budget its (qpos, qvel) pairs and body forces fit (fewer wavefronts per
	// CU then), and of the forms the first one down whose layout fits
	const int state = le_state_slots(in.nv, in.nmov, in.nl, in.nwd);  // (with the packed AR and the warmstart of a model with constraint rows)
	if (state > LE_MAX_SLOTS) {
		v.unavailable = in.nl > 0 ? "the model, with the packed AR of its constraint rows, needs more than 160 KB of LDS per wavefront" : "the model needs more than 160 KB of LDS per wavefront";
		return v;
	}
	const int least = state <= 40 ? 40 : (state <= 80 ? 80 : 160);
	if (least > v.lds_kb) v.lds_kb = least;
	if (v.sweep == 4 && le_quartet_slots(in.nv, in.nmov, in.nbody) > LE_MAX_SLOTS) v.sweep = 3;
	if (v.form == 3 && le_trio_slots(in.nv, in.nmov, in.nbody) > LE_MAX_SLOTS) v.form = 2, v.sweep = 0;
	if (v.form == 2 && le_duo2_slots(in.nv, in.nmov) > LE_MAX_SLOTS) v.form = 1;
	if (v.form == 1 && state + le_exchange_slots(in.nv) > v.lds_kb) v.form = 0;
	return v;
}
// ---- end of the plan ----

// ---- launching a compiled-in variant: one helper does the launch, a compile-time walk over (topology, build, form, budget) finds the kernel ----
struct LeLaunch {
	const KernelParams *Pdev;
	const mjb_model_desc *h;  // (may be NULL: the overlay / xfrc builds check their slot counts against it)
	int env_lo, env_hi, nsteps;
	unsigned int step0;
	hipStream_t stream;
	int dev;
};
unsigned int le_grid(const LeVariant &v, const LeLaunch &a) { return (unsigned int)((a.env_hi - a.env_lo + v.wave_lanes - 1) / v.wave_lanes); }
// `ran`: the variant the kernel is, for the record -- the one asked for, or the next one down that the topology's layout fits
template <class K> int le_go(K kern, int bytes, const LeVariant &ran, const LeLaunch &a)
{
	const hipError_t attr = lds_attr_once(reinterpret_cast<const void *>(kern), bytes, a.dev);
	if (attr != hipSuccess) return (int)attr;
	le_form_last = ran.form, le_sweep_last = ran.sweep;
	hipLaunchKernelGGL(kern, dim3(le_grid(ran, a)), dim3((unsigned int)le_block(ran)), bytes, a.stream, (const KernelParams MJB_AS4 *)a.Pdev, a.nsteps, a.step0, a.env_lo,
	                   a.env_hi);
	return (int)hipGetLastError();
}
template <class T, int LP, LeBuild B> int le_go_solo(const LeVariant &v, const LeLaunch &a)
{
	constexpr LeRow r = *le_row(0, 0, B);
	if (r.pe && (!a.h || PeSlots<T>::n != mjb_lane_env_overlay_slots(a.h))) return (int)hipErrorInvalidValue;
	if (r.xf && (!a.h || XfSlots<T>::n != mjb_lane_env_xfrc_slots(a.h))) return (int)hipErrorInvalidValue;
	return le_go(mjb_lane_env_kernel<T, LP, r.pe, r.hw, r.xf>, le_lds_bytes<T, LP>(0, 0), v, a);
}
template <class T, LeBuild B> int le_go_build(const LeVariant &v, const LeLaunch &a)  // a build of the solo form, at the budget
{
	return v.lds_kb == 160 ? le_go_solo<T, 160, B>(v, a) : (v.lds_kb == 80 ? le_go_solo<T, 80, B>(v, a) : le_go_solo<T, 40, B>(v, a));
}
template <class T> int le_go_topo(const LeVariant &v, const LeLaunch &a)
{
	switch (v.build) {  // the opt-in builds: the solo form alone
	case MJB_LE_HWSIM: return le_go_build<T, MJB_LE_HWSIM>(v, a);
	case MJB_LE_OVERLAY: return le_go_build<T, MJB_LE_OVERLAY>(v, a);
	case MJB_LE_XFRC: return le_go_build<T, MJB_LE_XFRC>(v, a);
	case MJB_LE_OVERLAY_XFRC: return le_go_build<T, MJB_LE_OVERLAY_XFRC>(v, a);
	case MJB_LE_PLAIN: break;
	}
	// the plain build: forms 3 and 2 exist at 160 KB alone, form 1 at 160 and 80.  A form whose layout is beyond a CU's LDS for this topology steps
	// down to the next one, as the plan does for a hiprtc-built model
	auto as = [&](int form, int sweep) { LeVariant ran = v; ran.form = form, ran.sweep = sweep; return ran; };
	if constexpr (le_lds_bytes<T, 160>(3, 4) <= mjb_max_lds_bytes())
		if (v.form == 3 && v.sweep == 4) return le_go(mjb_lane_env_trio_kernel<T, 4>, le_lds_bytes<T, 160>(3, 4), as(3, 4), a);
	if constexpr (le_lds_bytes<T, 160>(3, 3) <= mjb_max_lds_bytes())
		if (v.form == 3) return le_go(mjb_lane_env_trio_kernel<T, 3>, le_lds_bytes<T, 160>(3, 3), as(3, 3), a);
	if constexpr (le_lds_bytes<T, 160>(2, 0) <= mjb_max_lds_bytes())
		if (v.form >= 2) return le_go(mjb_lane_env_duo2_kernel<T>, le_lds_bytes<T, 160>(2, 0), as(2, 0), a);
	if (v.form >= 1 && v.lds_kb == 160) return le_go(mjb_lane_env_duo_kernel<T, 160>, le_lds_bytes<T, 160>(1, 0), as(1, 0), a);
	if (v.form >= 1 && v.lds_kb == 80) return le_go(mjb_lane_env_duo_kernel<T, 80>, le_lds_bytes<T, 80>(1, 0), as(1, 0), a);
	return le_go_build<T, MJB_LE_PLAIN>(v, a);
}
LePlanIn le_plan_in(const mjb_model_desc *fit_model, int ncu, int nenv_batch, LeBuild build, int form, int duo_max_waves, int sweep, int lds_kb, int wave_lanes)
{
	LePlanIn in{ ncu, nenv_batch, build, form, duo_max_waves, sweep, lds_kb, wave_lanes, fit_model != nullptr, 0, 0, 0, 0, false, false, false, 0, 0, false };
	if (fit_model) {
		in.sens = le_extra_sensors(fit_model), in.wrench_rest = le_wrench_at_rest(fit_model);
		in.nv = fit_model->nv, in.nmov = mjb_lane_env_xfrc_slots(fit_model), in.nbody = fit_model->nbody, in.na = fit_model->na;
		for (int b = 1; b < fit_model->nbody; b++) in.gc = in.gc || fit_model->body_gravcomp[b] != 0;
		in.nl = mjb_lane_env_limits(fit_model) + mjb_lane_env_eq_rows(fit_model);
		in.nwd = in.nl > 0 ? le_row_dofs(fit_model) : 0;
		in.solo = mjb_lane_env_solo_only(fit_model) != 0;
	}
	return in;
}
}  // namespace

// the plan for (device size, batch size, build, requests) with every knob of the environment at its default (include/mjb.h: mjb_lane_env_plan);
// fit_model: the model when hiprtc builds its kernel, NULL for a compiled-in topology
int mjb_lane_env_plan_for(const mjb_model_desc *fit_model, int ncu, int nenv_batch, int build, int form, int sweep_waves, int lds_kb, int *out_form, int *out_sweep,
                          int *out_lds_kb)
{
	if (build < MJB_LE_PLAIN || build > MJB_LE_OVERLAY_XFRC || nenv_batch <= 0) return -1;
	const LeVariant v = le_plan(le_plan_in(fit_model, ncu, nenv_batch, (LeBuild)build, (form >= 0 && form <= 3) ? form : -1, -1, sweep_waves, lds_kb, 64));
	if (v.unavailable) return -1;
	if (out_form) *out_form = v.form;
	if (out_sweep) *out_sweep = v.sweep;
	if (out_lds_kb) *out_lds_kb = v.lds_kb;
	return 0;
}

// topo >= 0: a compiled-in topology; MJB_LE_TOPO_JIT: the model's own, compiled by hiprtc on first use (h = the model; returns
// MJB_LE_UNAVAILABLE when that is not possible: the caller launches the generic kernel).  Gathers the plan's inputs, asks it, launches.
int mjb_launch_lane_env(const KernelParams *Pdev, int topo, const mjb_model_desc *h, int nenv_batch, int env_lo, int env_hi, int nsteps, unsigned int step0,
                        void *stream, LeBuild build)
{
	if (env_hi - env_lo <= 0) return 0;
	if (topo == MJB_LE_TOPO_JIT && !h) return (int)hipErrorInvalidValue;
	// the measurement knobs of the environment, read once; the two process-wide requests go first
	static const int wl_env = mjb_env_int("MJB_LANE_ENV_WAVE_LANES", 64);
	static const int lds_env = mjb_env_int("MJB_LANE_ENV_LDS_KB", 0);
	static const int duo_env = mjb_env_int("MJB_LANE_ENV_DUO", -1);
	static const int duo_max_waves = mjb_env_int("MJB_LANE_ENV_DUO_MAX_WAVES", -1);
	static const int sweep_env = mjb_env_int("MJB_LANE_ENV_SWEEP_WAVES", 0);
	const int form_ov = le_form_override.load(), sweep_ov = le_sweep_override.load();
	LeLaunch a{ Pdev, h, env_lo, env_hi, nsteps, step0, (hipStream_t)stream, 0 };
	(void)hipGetDevice(&a.dev);  // (the CU count per DEVICE: a process may drive several GPUs, one batch each -- ADVICE r05)
	const LeVariant v = le_plan(le_plan_in(topo == MJB_LE_TOPO_JIT ? h : nullptr, device_cus(a.dev), nenv_batch, build, form_ov >= 0 ? form_ov : duo_env, duo_max_waves,
	                                       sweep_ov ? sweep_ov : sweep_env, lds_env, wl_env));
	if (v.unavailable) {
		set_jit_error(v.unavailable);
		return MJB_LE_UNAVAILABLE;
	}
	if (topo == MJB_LE_TOPO_JIT) {
		const JitKernel &k = jit_get(*h, v);
		if (!k.fn) {
			set_jit_error(k.error);
			return MJB_LE_UNAVAILABLE;
		}
		const KernelParams MJB_AS4 *Pd = (const KernelParams MJB_AS4 *)Pdev;
		void *args[] = { (void *)&Pd, (void *)&a.nsteps, (void *)&a.step0, (void *)&a.env_lo, (void *)&a.env_hi };
		le_form_last = v.form, le_sweep_last = v.sweep;
		return (int)hipModuleLaunchKernel(k.fn, le_grid(v, a), 1, 1, (unsigned int)le_block(v), 1, 1, 0, a.stream, args, nullptr);  // (the kernel's LDS is static)
	}
#define MJB_LE_X(id, T) \
	if (topo == id) return le_go_topo<T>(v, a);
	MJB_LE_TOPOS(MJB_LE_X)
#undef MJB_LE_X
	return (int)hipErrorInvalidValue;
}
