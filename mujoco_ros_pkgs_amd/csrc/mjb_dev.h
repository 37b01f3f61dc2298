// mjb_dev.h — structures shared by the host API (mjb_api.hip) and the gfx950 kernels (mjb_step.hip).
//
// DevModel mirrors mjb_model_desc (include/mjb_model_fields.def) with every array living in one
// device blob.  The pointers are declared in the AMDGPU *constant* address space (4): model data is
// immutable and wave-uniformly indexed, so the compiler fetches it with scalar loads (s_load_*)
// into SGPRs instead of spending vector-memory issue slots and VGPRs on it.
#pragma once

#include <stdint.h>

#include "../../include/mjb.h"

#define MJB_AS4 __attribute__((address_space(4)))
typedef const int MJB_AS4 *mjb_ciptr;
typedef const double MJB_AS4 *mjb_cdptr;

struct DevModel {
#define MJB_SIZE(name) int name;
#define MJB_OPT_I(name) int name;
#define MJB_OPT_D(name, n) double name[n];
#define MJB_ARR_I(name, rows, cols) mjb_ciptr name;
#define MJB_ARR_D(name, rows, cols) mjb_cdptr name;
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	// engine-derived constant tables (built in mjb_compile)
	mjb_ciptr M_rowdof;    // [nM] dof i of qM entry e
	mjb_ciptr M_coldof;    // [nM] ancestor dof j of qM entry e
	mjb_ciptr dof_depth;   // [nv] number of entries in row i of qM (self + ancestors)
	mjb_ciptr dof_jstart;  // [nv] first dof of the "velocity group" the dof belongs to (see com_vel)
	mjb_ciptr body_rec;    // [nbody][4] packed {parentid, dofadr, dofnum, rootid}   (one s_load_dwordx4 per body)
	mjb_ciptr body_rec2;   // [nbody][4] packed {jntadr, jntnum, sameframe, weldid}
	mjb_ciptr dof_rec;     // [nv][4]    packed {Madr, nancestor, bodyid, parentid}
	mjb_ciptr dof_rec2;    // [nv][4]    packed {translational dof of a free joint, first joint of its body, parent of its body, bodyid}
	mjb_ciptr jnt_rec;     // [njnt][4]  packed {bodyid, type, dofadr, rootid of its body}
	mjb_ciptr fac_ops;     // [nfac][4]  factorisation micro-ops {dst, srcA, srcB, 0}: LD[dst] -= LD[srcA]/LD[kk]*LD[srcB]
	mjb_ciptr fac_beg;     // [nv+1]     first micro-op of pivot k
	mjb_ciptr flv_hdr;     // [flv_n][4] the same updates by levels of the elimination tree (mjb_api.hip): { slots, longest list of slot 0 / 1 / 2 }
	mjb_ciptr flv_rec;     // [flv_n + 3][3][64][4] the levels' contributions, one 16-byte word per lane and slot
	mjb_ciptr flv_ent;     // [nM, padded to 4 x 64] row | diagonal << 16 of every qM entry
	int flv_n;
	mjb_ciptr sens_copy;     // [2][3][sens_ncopy_max][2] (layout full/compact, stage-1): {dst offset in sensordata, src frame offset}
	mjb_ciptr sens_slow;     // [3][nsensor] ids of the sensors of each stage that need real work
	mjb_ciptr dof_act_adr;   // [nv+1] CSR: the actuators driving each dof (a tendon transmission appears under every joint of its tendon)
	mjb_ciptr dof_act_id;    // [dof_act_adr[nv]]
	mjb_ciptr pair_i;        // [ncollpair][8]  candidate-pair records: g1, g2, type1, type2, condim, friction rule (0 max, 1 geom1, 2 geom2, 4 the pair's own: <contact><pair friction>), collision-function override (MJB_COLFUNC_*), 0
	mjb_cdptr pair_d;        // [ncollpair][24] size1[3] size2[3] margin gap rbound1 rbound2 solref[2] solimp[5] includemargin friction[3] tran pad[2] (rule 4: friction = tangent 1, spin, roll 1; pad = tangent 2, roll 2)
	                         //   ([21] tran = body_invweight0[2 b1] + body_invweight0[2 b2] of the two geoms' bodies: the contact rows' diagApprox)
	// limit items (joints, then tendons) of make_constraint as records in pair_d's slots -- a lane fetches ITS item's record, contact or
	// limit, with one batch of unconditional loads before the kinds diverge: [0..1] range, [6] margin, [10..11] solref, [12..16] solimp,
	// [21] dof_invweight0 / tendon_invweight0;  lim_i [4]: limited (and slide / hinge), qpos address (tendon: its id), dof address, pad
	mjb_cdptr lim_d;         // [njnt + ntendon][24]
	mjb_cdptr dof_act_mom;   // [dof_act_adr[nv]] moment arm of each (dof, actuator) entry: gear (joint transmission) / gear * coefficient (tendon transmission)
	int act_tendon;          // some actuator drives a fixed tendon (the per-actuator lane caches of the dense kernels stand down)
	mjb_cdptr dof_damping_int;  // [nv] what the integrator's implicit matrix adds to M's diagonal, per unit of h: dof_damping (Euler), -diag(D) (implicitfast)
	mjb_ciptr lim_i;         // [njnt + ntendon][4]
	int sens_ncopy[3];       // plain-copy elements per stage
	int sens_nslow[3];       // complex sensors per stage
	int sens_ncopy_max;
	mjb_ciptr body_dofmask;  // [nbody][2] bit i set: dof i moves the body (ancestor-or-self dofs), nv <= 64
	mjb_ciptr M_dense;       // [16][16] qM address of entry (i, j) (dof j ancestor-or-self of dof i) or -1; nv <= 16 only
	mjb_ciptr M_sym;         // [32][32] qM address of the symmetric entry (i, j) or -1; nv <= 32 only (primal solvers: M rows in registers)
	mjb_ciptr body_anc;      // [kin_rounds + 1][nbody] ancestor at distance 2^r (0 = world / beyond the root)
	mjb_ciptr dof_bodymask;  // [nv][2] bit b set: dof i moves body b (transpose of body_dofmask), nbody <= 64
	mjb_ciptr body_submask;  // [nbody][2] bit i set: body i belongs to the body's subtree (incl. itself), nbody <= 64
	int eulerdamp;           // any dof_damping > 0 and EULERDAMP not disabled
	int nfriction;           // number of dofs + tendons with frictionloss > 0 (0 when FRICTIONLOSS is disabled): friction rows exist
	int need_rnepost;        // an acceleration-stage sensor needs mj_rnePostConstraint (cacc / cfrc_int / cfrc_ext)
	int kin_rounds;          // ceil(log2(max body depth)): rounds of the pointer-jumping kinematics
	int maxdepth;          // max dof_depth
	// leaf-to-root sums of the smooth stages (subtree com, composite inertia, RNE's backward pass) as a product with the 0/1 subtree
	// matrix: [sub_nt][4 sub_nt][64] doubles, the A operands of v_mfma_f64_16x16x4_f64 (mjb_step.hip, subtree_sum)
	mjb_cdptr sub_S;
	int sub_nt;              // row tiles (1: nbody <= 16, 2: nbody <= 32; 0: larger models keep the flat sums)
	// root-to-leaf sums (cvel, cacc): [nbody][4] = the body's ancestor-or-self dofs, ASCENDING, one byte each (0xFF = none), at most 16
	mjb_ciptr body_dofanc;
	int dofanc_max;          // longest list (0: some body has more than 16 -- or nv > 255 --: the mask loops run instead)
	// lane = env kernel (mjb_lane_env.hip): the model's numeric constants as ONE tape in the order the kernel consumes them --
	// LeTapeHdr, LeTapeBody[nbody], LeTapeAct[nu] -- read by wide scalar loads off a single base address (NULL: no compiled-in topology)
	mjb_cdptr le_tape;
	// site transmissions (mjTRN_SITE): their actuators in actuator order.  Their moments depend on the configuration: the transmission stage
	// computes one row of nv per actuator into the frame (FrameLayout::act_mom) at every forward evaluation (mjb_step.hip, site_transmission)
	mjb_ciptr site_act;      // [nsite_act] actuator ids
	int nsite_act;
	// gravity compensation (mjModel.body_gravcomp): the bodies b >= 1 with a non-zero coefficient, ascending; mjModel.ngravcomp of them.  The passive
	// stage adds their forces to qfrc_passive from xipos, cdof and subtree_com of the position stage (mjb_step.hip, gravcomp): no frame storage
	mjb_ciptr gravcomp_body;  // [ngravcomp]
	int ngravcomp;
};

// (64-byte records: one s_load_dwordx16 per half)
struct LeTapeHdr { double dt, gravity[3], pad[4]; };
struct LeTapeBody {
	// pose half: what mj_kinematics needs of the body and its (single) joint
	double pos[3], quat[4], jaxis[3], jpos[3], qpos0, stiffness, spring;
	// inertial half
	double ipos[3], ibody[6] /* R(iquat) diag(inertia) R(iquat)': xx yy zz xy xz yz */, mass, damping, armature, hdamping /* timestep * damping */, gravcomp /* mjModel.body_gravcomp */, pad[2];
};
// The record as the kernels fetch it, 16 doubles a half: LE_<FIELD> is the field's index in the whole record, LE_I_<FIELD> its index in the inertial half
#define LE_OFS(f) ((int)(__builtin_offsetof(LeTapeBody, f) / sizeof(double)))  /* (offsetof without <cstddef>: hiprtc compiles this header too) */
enum {
	LE_POS = LE_OFS(pos), LE_QUAT = LE_OFS(quat), LE_JAXIS = LE_OFS(jaxis), LE_JPOS = LE_OFS(jpos), LE_QPOS0 = LE_OFS(qpos0), LE_STIFFNESS = LE_OFS(stiffness), LE_SPRING = LE_OFS(spring),
	LE_HALF = 16,
	LE_IPOS = LE_OFS(ipos), LE_IBODY = LE_OFS(ibody), LE_MASS = LE_OFS(mass), LE_DAMPING = LE_OFS(damping), LE_ARMATURE = LE_OFS(armature), LE_HDAMPING = LE_OFS(hdamping), LE_GRAVCOMP = LE_OFS(gravcomp),
	LE_I_IPOS = LE_IPOS - LE_HALF, LE_I_IBODY = LE_IBODY - LE_HALF, LE_I_MASS = LE_MASS - LE_HALF,
	LE_A_N = LE_QPOS0 + 1, LE_I_N = LE_I_MASS + 1,  // what the sweep fetches of either half: up to qpos0 | up to mass
};
#undef LE_OFS
static_assert(LE_POS == 0 && LE_SPRING == LE_HALF - 1 && LE_IPOS == LE_HALF && LE_GRAVCOMP == 29 && sizeof(LeTapeBody) == 2 * LE_HALF * sizeof(double), "lane = env body record: the pose half is doubles 0 - 15, the inertial half 16 - 31");
// (dyntau: a filter actuator's max(mjMINVAL, dynprm[0]) -- the divisor of act_dot, not its reciprocal; actlo / acthi: actrange.  Zero for a stateless actuator)
struct LeTapeAct { double gear, ctrllo, ctrlhi, gain[3], bias[3], forcelo, forcehi, dyntau, actlo, acthi, pad[2]; };
static_assert(sizeof(LeTapeHdr) == 64 && sizeof(LeTapeBody) == 256 && sizeof(LeTapeAct) == 128, "lane = env tape records");
// Joint limits (a model whose only constraint rows are hinge / slide joint-limit rows under PGS, mjb_lane_env_eligible): BEHIND the records above -- their
// offsets stay where they are -- one LeTapeLimHdr, then one LeTapeLim per limited joint, in joint order.  solref / solimp are stored as getsolparam
// leaves them (a mixed-sign solref replaced by the default, refsafe, solimp clamped to its legal ranges); K and B are mj_makeImpedance's stiffness and
// damping of the row from them, powa / powb the two wave-uniform factors of the impedance curve, 1 / mid^(power - 1) and 1 / (1 - mid)^(power - 1).
struct LeTapeLimHdr { double meaninertia, tolerance, iterations, scale /* 1 / (meaninertia max(1, nv)) */, nowarm /* mjDSBL_WARMSTART */, norefsafe /* mjDSBL_REFSAFE */, pad[2]; };
struct LeTapeLim { double range[2], margin, solref[2], solimp[5], invweight0, K, B, powa, powb, pad; };
static_assert(sizeof(LeTapeLimHdr) == 64 && sizeof(LeTapeLim) == 128, "lane = env tape records of the joint limits");
// Joint equalities and fixed tendons (mjb_lane_env_eligible): BEHIND the limit records, one LeTapeEq per active joint equality in equality order (the
// header above is there whenever the model has rows of either kind), then one LeTapeWrap per tendon wrap in wrap order (mjModel.wrap_prm).  An equality
// record holds polycoef, qpos0 of its two joints (the second 0 in the one-joint form), solref / solimp as getsolparam leaves them, the sum of the two
// dofs' invweight0 and K / B / powa / powb as LeTapeLim does.  A wrap record holds the PLAIN coefficient: the actuator's gear (LeTapeAct) multiplies it
// in the kernel, actuator_length = gear sum_w coef_w qpos_w.
struct LeTapeEq { double polycoef[5], qpos0[2], solref[2], solimp[5], invweight0, K, B, powa, powb, pad[5]; };
struct LeTapeWrap { double coef, pad[7]; };
static_assert(sizeof(LeTapeEq) == 192 && sizeof(LeTapeWrap) == 64, "lane = env tape records of the joint equalities and tendon wraps");

// Offsets (in doubles / ints) of every data field inside one per-env frame.
struct FrameLayout {
#define MJB_DS(name, rows, cols) int name;
#define MJB_DD(name, rows, cols) int name;
#define MJB_DD2(name, rows, cols) int name;
#define MJB_DI(name, rows, cols) int name;
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
	int MhB;       // [nM]  M + h*diag(damping) (Euler implicit damping), built and factorised next to qM
	int qH;        // [nM]  its L'DL factor
	int qHdi;      // [nv]  1 / diag
	int nwt_M;     // [nv*nv] Newton: dense M          (size 0 unless solver == Newton with constraint rows)
	int nwt_H;     // [nv*nv] Newton: Hessian / its Cholesky factor
	int nwt_vec;   // [5*nv]  Newton: qacc, Ma, grad, search, Mv
	int nwt_row;   // [3*nefcmax] Newton: per-row jaref, jv, Hessian weight
	int nwt_hc;    // [hcs*nconmax] Newton: Hessian blocks of the elliptic cones (size 0 unless cone == elliptic); PGS + elliptic: blocks of AR
	int hcs, hcd;  // cone blocks are hcd x hcd, hcs doubles apart (primal solvers: hcd = the model's largest contact dim, hcs = max(hcd^2, 10); PGS: 36, 6)
	int iscratch;  // transient int scratch: max(ncollpair, njnt + nconmax)
	int gravity;   // [3] this env's gravity (model value or per-env override, loaded with the state)
	int gfriction; // [3*ngeom] this env's geom friction (models with contacts only)
	int eqparam;   // [19*neq] this env's equality parameters: active | eq_data[11] | solref[2] | solimp[5] per equality
	int cwrench;  // [nconmax][6] world contact wrenches (rne_post scratch)
	int kinloc;    // [7*nbody] kinematics: pose of each body in its parent frame (transient)
	int crbbuf;    // [6*nv]    crb: crb[body(i)] * cdof_i (transient)
	int eulerx;    // [nv]      Euler: velocity-update right-hand side / solution (transient)
	int dadr;      // [64 ints] constrained kernels, nv <= 16: packed dense address map of lanes 0-15 (int frame)
	int tri;       // transient scratch: packed dense triangle of the L'DL factor (PGS, nv <= 16: 128 doubles; 16 < nv <= 32: 496, solve_tri32)
	int rk;        // [nq + 4 nv + nsensordata] RK4 bookkeeping (rk4_stage), -1 under Euler
	int jrows;     // rows of efc_J the frame holds (nefcmax, except in the fused frame of kernel variant 4: 64, the rest in DevState::efc_Jg)
	int rcap;      // rows every OTHER per-row array holds (efc_D / aref / b / force / frictionloss / type / id, nwt_row, the row metadata in
	               // iscratch): nefcmax, except in the X-layout fused frame of kernel variant 4, where it equals jrows (an env-step with
	               // more rows keeps ALL of its row data in the env's block of DevState::efc_Jg, see RowBlock)
	int hcrow;     // 1: the cone block of a contact sits at nwt_hc + hcd * (its first row) [hcd * rcap doubles]; 0: at nwt_hc + hcs * contact
	int solvescr;  // [32]      pivot-row scratch of the dense M^-1 solves in fwd_acceleration / Euler (the factorisation uses crbbuf)
	int bbscr;     // [216]     transient scratch of the box - box narrow phase (alive inside collision only)
	int act_mom;   // [nsite_act * nv] moment rows of the site transmissions (transmission -> velocity stage -> actuation: own storage, never overlaid)
	int ndouble;   // doubles per frame
	int nint;      // ints per frame (follow the doubles)
	int nstate;    // doubles in the persistent prefix
};

// HBM arrays of the persistent state, env-major [nenv][dim]
struct DevState {
#define MJB_DS(name, rows, cols) double *name;
#define MJB_DD(name, rows, cols)
#define MJB_DD2(name, rows, cols)
#define MJB_DI(name, rows, cols)
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
	double *frame_ws;              // optional [nenv][ndouble + nint/2 padded] full-frame workspace
	unsigned long long *nwarn;     // [MJB_NWARNING] mjData.warning[].number summed over the envs (mjb_warning)
	unsigned long long *prof;      // [64] per-stage cycle sums + call counts (profiling build only), else NULL
	unsigned long long *stats;     // [MJB_NSTATS] workload statistics (mjb_set_stats), NULL when off
	unsigned long long *rowstat;         // [4] evaluations | beyond 64 rows | beyond 128 rows | - of the current long fused launch (kernel variant 4's wide-frame policy), or NULL
	int nenv;
	int frame_stride;              // doubles per env in frame_ws
	const double *env_gravity;       // [nenv][3] per-env gravity override (NULL: the model's)
	const double *env_geom_friction; // [nenv][ngeom][3] per-env geom friction override (NULL: the model's)
	const double *env_geom_size;     // [nenv][ngeom][3] per-env geom sizes (NULL: the model's)
	const int *env_geom_type;        // [nenv][ngeom] per-env geom types (NULL: the model's)
	const double *env_equality;      // [nenv][neq][19] per-env equality parameters (NULL: the model's)
	const double *env_mass;          // [nenv][EnvBlockLayout::doubles] per-env inertial, joint and actuator constants (NULL: the model's), laid out by EnvBlockLayout below
	int *sched;                      // [1 + nenv] work counter | chunks done per env, of a chunked fused launch (constrained kernels); NULL otherwise
	double *efc_Jg;                  // [nenv][mjb_rowblock_doubles] row data of the env-steps whose rows outnumber the fused frame's share (kernel variant 4, RowBlock); NULL otherwise
	unsigned long long efc_Jg_stride;  // doubles per env of efc_Jg: sized for the largest cone-block stride of the model's three frame layouts (the kernels lay a block out with the stride of the frame they run on)
	double *pgs_B;                   // [nenv][nefcmax * nv] rows of J M^-1 of the PGS steps beyond 64 rows (nv <= 16 models keep them out of LDS); NULL otherwise
	int use_xfrc;                  // xfrc_applied has ever been written
	const double *zbuf;            // [nsteps][nenv][nu] standard normals of the ctrl-noise injector for ONE fused launch, pre-generated by
	                               // mjb_noise_kernel on the same stream (NULL: generated inside the step kernel)
	const unsigned int *zinfo;     // two records { step0, nsteps, nenv, - }: what the generator wrote each HALF of zbuf for; a launch uses the half
	                               // whose record is its own (the other half is being filled for the NEXT launch, on a side stream, meanwhile)
	unsigned long long zhalf;      // doubles per half
	int keep_frame;                // fused mjb_step also dumps the last step's full frame to frame_ws
	double *handoff;               // [nenv][handoff_stride] hand-off records of the split step (HandoffLayout): written by the lane = env smooth kernel
	                               // (mjb_smooth_kernel.h), read by mjb_cstep_kernel; NULL until the batch first steps that way
	int handoff_stride;
	int sens_every_step;           // lane = env kernel: evaluate the sensors at every step of a fused launch instead of its last one (mjb_set_sensors_every_step)
	int colfunc[64];               // mjCOLLISIONFUNC-style table of MujocoEnv::registerCollisionFunction's overrides by (geom type 1, geom type 2), type1 <= type2,
	                               // index 8 * type1 + type2: read instead of the pair record's copy when per-env geom TYPES are in play (a pair's current types)
	const double *reset_step;      // [nq + nv + nv] qpos | qvel | qacc_warmstart one step after mj_resetData (mj_checkAcc's reset inside the split step), or NULL
	int prof_base;                 // profiling build: first of the two probe ids this launch records (mjb_debug_profile_window)
	const double *le_overlay;      // [slots][nenv] lane = env kernel, mjb_set_lane_env mode 2: each env's own gravity, joint constants, masses / inertias and
	                               // actuator gains in the kernel's terms (PeSlots, mjb_lane_env_kernel.h); NULL until such a launch builds it
	double *le_xfrc;               // [6 * slots][nenv] lane = env kernel, mjb_lane_env_set_xfrc: xfrc_applied of the moving bodies, transposed (XfSlots,
	                               // mjb_lane_env_kernel.h); NULL until such a launch builds it.  The kernel zeroes the column of an env it resets
};

// The env's spill-over block in DevState::efc_Jg (kernel variant 4): efc_J [nefcmax][nv], then -- used only when the frame's row
// arrays are capped too (FrameLayout::rcap < nefcmax) -- D | aref | b | force | frictionloss | jaref | jv | hw [nefcmax each],
// the cone blocks [hcs * nconmax], and three int arrays type | id | meta [nefcmax each].
#if defined(__HIPCC__)
#define MJB_HD __host__ __device__
#else
#define MJB_HD
#endif
MJB_HD inline size_t mjb_rowblock_doubles(int nefcmax, int nv, int nconmax, int hcs)
{
	return (size_t)nefcmax * nv + (size_t)8 * nefcmax + (size_t)hcs * nconmax + (size_t)2 * nefcmax;
}
// One env's block of DevState::env_mass: the offset of each section, in doubles and in this order.  The sections up to mass_doubles are the
// public mass block (mjb_set_env_mass_params, mjb_env_mass_stride), the rest is the joint section; doubles is the stride.  Host, kernels and
// the lane = env overlay all index the block through this one definition.
struct EnvBlockLayout {
	int body_mass, body_subtreemass, body_inertia /* [3] */, dof_invweight0, body_invweight0 /* [2] */, tendon_invweight0, meaninertia, mass_doubles;
	int dof_damping, dof_armature, dof_frictionloss, dof_damping_int, jnt_stiffness, actuator_gainprm /* [3] */, actuator_biasprm /* [3] */, doubles;
};
MJB_HD constexpr EnvBlockLayout mjb_env_block_layout(int nbody, int nv, int ntendon, int njnt, int nu)
{
	EnvBlockLayout B{};
	int o = 0;
	B.body_mass = o, o += nbody;
	B.body_subtreemass = o, o += nbody;
	B.body_inertia = o, o += 3 * nbody;
	B.dof_invweight0 = o, o += nv;
	B.body_invweight0 = o, o += 2 * nbody;
	B.tendon_invweight0 = o, o += ntendon;
	B.meaninertia = o, o += 1;
	B.mass_doubles = o;
	B.dof_damping = o, o += nv;
	B.dof_armature = o, o += nv;
	B.dof_frictionloss = o, o += nv;
	B.dof_damping_int = o, o += nv;
	B.jnt_stiffness = o, o += njnt;
	B.actuator_gainprm = o, o += 3 * nu;
	B.actuator_biasprm = o, o += 3 * nu;
	B.doubles = o;
	return B;
}
inline EnvBlockLayout mjb_env_block_layout(const mjb_model_desc &h) { return mjb_env_block_layout(h.nbody, h.nv, h.ntendon, h.njnt, h.nu); }
// The public packed joint block (mjb_set_env_joint_params, mjb_env_joint_stride) is the joint section without dof_damping_int, which the
// engine derives: where the section at block offset `off` sits in it (off = doubles: its length)
MJB_HD constexpr int mjb_env_joint_packed(const EnvBlockLayout &B, int off)
{
	return off - B.mass_doubles - (off > B.dof_damping_int ? B.jnt_stiffness - B.dof_damping_int : 0);
}
namespace mjb_env_block_sample {  // the format, pinned on (nbody, nv, ntendon, njnt, nu) = (3, 4, 2, 5, 6)
constexpr EnvBlockLayout B = mjb_env_block_layout(3, 4, 2, 5, 6);
static_assert(B.body_mass == 0 && B.body_subtreemass == 3 && B.body_inertia == 6 && B.dof_invweight0 == 15 && B.body_invweight0 == 19 &&
                  B.tendon_invweight0 == 25 && B.meaninertia == 27 && B.mass_doubles == 28,
              "mass section of the per-env block");
static_assert(B.dof_damping == 28 && B.dof_armature == 32 && B.dof_frictionloss == 36 && B.dof_damping_int == 40 && B.jnt_stiffness == 44 &&
                  B.actuator_gainprm == 49 && B.actuator_biasprm == 67 && B.doubles == 85,
              "joint section of the per-env block");
static_assert(mjb_env_joint_packed(B, B.dof_damping) == 0 && mjb_env_joint_packed(B, B.dof_frictionloss) == 8 && mjb_env_joint_packed(B, B.jnt_stiffness) == 12 &&
                  mjb_env_joint_packed(B, B.actuator_biasprm) == 35 && mjb_env_joint_packed(B, B.doubles) == 53,
              "public packed joint block: 3 nv + njnt + 6 nu");
}  // namespace mjb_env_block_sample
struct RowBlock {
	double *J, *D, *aref, *b, *force, *fl, *nwt_row, *hc;
	int *type, *id, *meta;
};
MJB_HD inline RowBlock mjb_rowblock(double *base, int nefcmax, int nv, int nconmax, int hcs)
{
	RowBlock g;
	g.J = base;
	g.D = base + (size_t)nefcmax * nv;
	g.aref = g.D + nefcmax;
	g.b = g.aref + nefcmax;
	g.force = g.b + nefcmax;
	g.fl = g.force + nefcmax;
	g.nwt_row = g.fl + nefcmax;
	g.hc = g.nwt_row + 3 * nefcmax;
	g.type = reinterpret_cast<int *>(g.hc + (size_t)hcs * nconmax);
	g.id = g.type + nefcmax;
	g.meta = g.id + nefcmax;
	return g;
}

// The hand-off record of the split step (mjb_smooth_kernel.h -> mjb_cstep_kernel): what the constraint stages read of the smooth stages'
// results, one contiguous record per env in HBM, in this order.  subtree_com holds, for a tree's ROOT body, the point the tree's spatial
// quantities (cdof, hence the contact Jacobians) are taken about -- the root body's origin; the other bodies' entries are not written.
struct HandoffLayout {
	int geom_xpos, geom_xmat, cdof, subtree_com, qLD, qLDiagInv, qH, qHdi, qfrc_smooth, qacc_smooth, ndouble, stride;
};
MJB_HD inline HandoffLayout mjb_handoff_layout(int ngeom, int nv, int nbody, int nM)
{
	HandoffLayout h;
	int o = 0;
	h.geom_xpos = o; o += 3 * ngeom;
	h.geom_xmat = o; o += 9 * ngeom;
	h.cdof = o; o += 6 * nv;
	h.subtree_com = o; o += 3 * nbody;
	h.qLD = o; o += nM;
	h.qLDiagInv = o; o += nv;
	h.qH = o; o += nM;
	h.qHdi = o; o += nv;
	h.qfrc_smooth = o; o += nv;
	h.qacc_smooth = o; o += nv;
	h.ndouble = o;
	h.stride = (o + 7) & ~7;  // records start on 64-byte boundaries
	return h;
}

struct NoiseCfg {
	double rate;   // exp(-dt / max(ctrl_noise_rate, mjMINVAL))
	double scale;  // ctrl_noise_std * sqrt(1 - rate^2)
	unsigned long long seed;
	long long env_offset;
	int enabled;
	int pad;
};

// device-side DefaultRobotHWSim::writeSim (mjb_hwsim_*): controlled joints and their per-env commands / PID state
struct HwSim {
	int n;             // controlled joints (0: stage off)
	int estop;         // e-stop active
	const int *joint, *method, *kind, *antiwindup;          // [n]
	const double *gains;                                     // [n][8]: p, i, d, i_max, i_min, effort_limit, lower, upper
	const double *cmd_pos, *cmd_vel, *cmd_eff, *cmd_hold;    // [nenv][n]; cmd_hold = position commands frozen at e-stop
	double *pid;                                             // [nenv][n][2]: integral of the error, previous error
	// controller cadence of MujocoRosControlPlugin::controlCallback (mjb_hwsim_set_period; period_ns == 0: writeSim at every step on
	// the step's own joint state with the model's timestep, the round-2 behaviour)
	long long period_ns;                                     // control_period as ros::Duration counts it
	double *cad;                                             // [nenv][2 + 2 n]: last update / last write [ns], joint_position_[n], joint_velocity_[n]
	// the same configuration by DOF, for the lane = env kernel's HW build (mjb_lane_env_set_hwsim): a lane's forces are registers, so that kernel walks the
	// dofs at compile time and reads what controls each one as scalars
	mjb_ciptr le_tab;                                        // [nv][4]: entry k (-1: not controlled) | method | kind | antiwindup
	mjb_cdptr le_gains;                                      // [nv][8]: the entry's gains
};

// Everything a launch needs, resident in device memory (uploaded when it changes); kernels get one
// constant-address-space pointer to it.
struct KernelParams {
	DevModel m;
	FrameLayout L;    // full layout: every field has its own storage (forward / split step / dumps)
	FrameLayout Lc;   // compact layout of the fused step: fields with disjoint lifetimes share storage
	int use_compact;  // fused launches use Lc
	int pad0;
	DevState s;
	NoiseCfg nz;
	HwSim hw;
	// (behind everything the kernels compiled before it read: their offsets stay) lane = env kernel, a model with joint limits: what the launch leaves of the
	// constraint stage of its last step, [nenv][nv + 2] = qfrc_constraint[nv] | nefc | solver_iter (as doubles); NULL until such a launch allocates it
	double *le_con;
};

// ---- the step kernel's variants: the value of mjb_step_kernel's template parameter CON (TAG in the constraint stages), of MJB_DEV_ONLY_CON and
// MJB_DEBUG_VARIANT, and the number DESIGN.md, the tests and the tools call a variant by.  Separate kernels keep each instruction stream and
// register budget small (mjb_step.hip, "the kernel").  The predicates below are what the kernels and the host ask of a variant; this header is
// also compiled by hiprtc, so they are plain constexpr functions of int.
enum {
	MJB_KV_NONE = 0,                                             // model without constraint rows
	MJB_KV_PGS = 1,                                              // PGS, 512-register build
	MJB_KV_NEWTON1 = 2, MJB_KV_NEWTON2 = 3, MJB_KV_NEWTON4 = 4,  // Newton, 1 / 2 / 4 rows per lane in registers (nefcmax <= 64 / 128 / 256); 4: the fused frame
	                                                             //   holds FrameLayout::jrows rows of efc_J, the rest lives in DevState::efc_Jg
	MJB_KV_PGS_ELL = 5,                                          // PGS with elliptic cone blocks
	MJB_KV_CG1 = 6, MJB_KV_CG2 = 7, MJB_KV_CG4 = 8,              // CG (the Newton solver without its Hessian), 1 / 2 / 4 rows per lane
	MJB_KV_PGS256 = 9,                                           // the plain PGS step under a 256-register cap (eight lean frames fit one CU's LDS: two waves per SIMD)
	MJB_KV_SLOT_NEWTON = 10, MJB_KV_SLOT_CG = 11,                // the row-slot solver (up to 1024 rows), Newton / CG, frame in LDS
	MJB_KV_SLOT_NEWTON_HBM = 12, MJB_KV_SLOT_CG_HBM = 13,        // the same with the frame in HBM (DevState::frame_ws)
};
constexpr bool mjb_kv_pgs(int v) { return v == MJB_KV_PGS || v == MJB_KV_PGS_ELL || v == MJB_KV_PGS256; }
constexpr bool mjb_kv_newton(int v) { return v >= MJB_KV_NEWTON1 && v <= MJB_KV_NEWTON4; }  // register-row Newton
constexpr bool mjb_kv_cg(int v) { return v >= MJB_KV_CG1 && v <= MJB_KV_CG4; }              // register-row CG
constexpr bool mjb_kv_slot(int v) { return v >= MJB_KV_SLOT_NEWTON && v <= MJB_KV_SLOT_CG_HBM; }
constexpr bool mjb_kv_slot_cg(int v) { return v == MJB_KV_SLOT_CG || v == MJB_KV_SLOT_CG_HBM; }  // the CG one of a row-slot pair
constexpr bool mjb_kv_hbm_frame(int v) { return v == MJB_KV_SLOT_NEWTON_HBM || v == MJB_KV_SLOT_CG_HBM; }
constexpr int mjb_kv_hbm(int v) { return v == MJB_KV_SLOT_NEWTON ? MJB_KV_SLOT_NEWTON_HBM : (v == MJB_KV_SLOT_CG ? MJB_KV_SLOT_CG_HBM : v); }  // its build for a frame in HBM
constexpr int mjb_kv_rows_per_lane(int v) { return (v == MJB_KV_NEWTON4 || v == MJB_KV_CG4) ? 4 : ((v == MJB_KV_NEWTON2 || v == MJB_KV_CG2) ? 2 : 1); }  // register-row solvers
// carries the chained-step / cut-RK4 modes (MJB_MODE_STEP21, RKMID, RKLAST); dense: the kernel's DENSE parameter
constexpr bool mjb_kv_chained(int v, int dense) { return dense == 0 && v != MJB_KV_PGS256; }
// minimum waves per SIMD of __launch_bounds__: G lanes per env (unconstrained kernels), occ = MJB_DEV_OCC (the 512-register kernels)
constexpr int mjb_kv_min_waves(int v, int G, int occ) { return v == MJB_KV_NONE ? (G == 64 ? 4 : (G == 32 ? 2 : 1)) : ((mjb_kv_cg(v) || v == MJB_KV_PGS256 || mjb_kv_slot_cg(v)) ? 2 : occ); }
// the build slice (Makefile: GROUPS, mjb_step.hip: MJB_GROUP) a variant is compiled in; slice 6 is the split step's constraint kernel
constexpr int mjb_kv_slice(int v) { return v == MJB_KV_NONE ? 0 : (v == MJB_KV_PGS256 ? 5 : (mjb_kv_pgs(v) ? 1 : (v == MJB_KV_NEWTON4 ? 3 : (mjb_kv_newton(v) ? 2 : (mjb_kv_cg(v) ? 4 : (mjb_kv_hbm_frame(v) ? 8 : 7)))))); }

constexpr int mjb_max_lds_bytes() { return 160 * 1024; }  // LDS of one gfx950 CU
inline int mjb_layout_bytes(const FrameLayout &L) { return ((L.ndouble * 8 + L.nint * 4) + 15) & ~15; }  // one env's frame, rounded to 16 bytes

#ifndef __HIPCC_RTC__
#include <cstdlib>
// knobs read from the environment (host code).  A knob read once per process is a `static const` at its point of use, initialised by one of these.
inline int mjb_env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
inline bool mjb_env_flag(const char *name) { const char *v = getenv(name); return v && *v && *v != '0'; }
#endif

enum { MJB_MODE_STEP = 0, MJB_MODE_FORWARD = 1, MJB_MODE_STEP1 = 2, MJB_MODE_STEP2 = 3, MJB_MODE_STEP21 = 4 /* STEP2 of one step, then STEP1 of the next */,
       // STEP2 of an RK4 step cut at the callback points of its evaluations (mjb_step2_rk_prefix; the evaluation index travels in the
       // kernel's `nsteps` argument): RKMID = second half of evaluation rk, rk4_stage(rk), first half of evaluation rk + 1;
       // RKLAST = second half of evaluation 3 + the final advance
       MJB_MODE_RKMID = 5, MJB_MODE_RKLAST = 6 };

// launches (implemented in mjb_step.hip); returns hipError_t as int
// (a step launch covers the whole batch, or a prefix / the rest for the split steps of the host runtime)
int mjb_launch_noise(const KernelParams *Pdev, double *zbuf, unsigned int *zinfo, int nenv, int nu, int nsteps, unsigned int step0, void *stream);
struct StepLaunch {
	const KernelParams *params;  // device copy
	const FrameLayout *L;        // the layout the kernel runs on (host copy)
	int env_lo, env_hi;          // steps envs [env_lo, env_hi)
	int mode, nsteps;            // MJB_MODE_*; steps of a fused launch (cut-RK4 modes: the evaluation index)
	unsigned int step0;          // the step counter the launch starts at
	int lanes, epb;              // lanes per env, envs per block
	int variant;                 // MJB_KV_*
	int chunk;                   // steps per work item of a chunked launch, 0 = one item per env
	int dense;                   // unconstrained 16-lane kernels: 8 / 12 / 16 = the dense-M build for nv up to that, 0 = the generic one
	void *stream;
};
int mjb_launch_step(const StepLaunch &a);
int mjb_launch_reset(const KernelParams *Pdev, int nenv, const unsigned char *mask_dev, void *stream);
// lane = env form of the unconstrained fused step (mjb_lane_env.hip)
int mjb_lane_env_match(const mjb_model_desc *h);
size_t mjb_lane_env_tape_doubles(const mjb_model_desc *h);      // size of the constant tape
void mjb_lane_env_tape(const mjb_model_desc *h, double *tape);  // fills it
const char *mjb_lane_env_name(int topo);
enum { MJB_LE_TOPO_NONE = -1, MJB_LE_TOPO_JIT = -2, MJB_LE_UNAVAILABLE = -1000 };
int mjb_lane_env_eligible(const mjb_model_desc *h);   // the model's structure fits the kernel (compiled in or not)
int mjb_lane_env_limits(const mjb_model_desc *h);     // the joint-limit rows of a model the kernel takes WITH constraint rows (its limited joints), 0: it has none
int mjb_lane_env_eq_rows(const mjb_model_desc *h);    // ... and its joint-equality rows (the active joint equalities), 0: it has none
const char *mjb_lane_env_refusal(void);               // why mjb_lane_env_eligible last refused a model for its size ("" if it did not)
int mjb_lane_env_solo_only(const mjb_model_desc *h);  // 1: constraint rows or fixed tendons -- the plain build of the one-wavefront form alone runs such a model
const char *mjb_lane_env_jit_error(void);                    // why the last hiprtc build of a topology was not available ("" if none failed)
void mjb_lane_env_jit_stats(int *compiled, int *disk_hits);  // hiprtc builds of this process / builds taken from the disk cache instead
// which build of the kernel a launch runs: the plain one (any form), or one of the two that exist for the solo form only and run it whatever the batch size --
// the one that reads DevState::le_overlay (template flag PE), the one with the device hwsim stage, KernelParams::hw (template flag HW), and the two
// that apply xfrc_applied from DevState::le_xfrc (template flag XF), without and with the overlay
enum LeBuild { MJB_LE_PLAIN = 0, MJB_LE_OVERLAY = 1, MJB_LE_HWSIM = 2, MJB_LE_XFRC = 3, MJB_LE_OVERLAY_XFRC = 4 };
int mjb_launch_lane_env(const KernelParams *Pdev, int topo, const mjb_model_desc *h, int nenv_batch, int env_lo, int env_hi, int nsteps, unsigned int step0,
                        void *stream, LeBuild build);
// the launcher's plan with the environment's knobs at their defaults (mjb_lane_env_plan of include/mjb.h; fit_model: the model when hiprtc builds its
// kernel, NULL for a compiled-in topology); 0, or -1: no variant
int mjb_lane_env_plan_for(const mjb_model_desc *fit_model, int ncu, int nenv_batch, int build, int form, int sweep_waves, int lds_kb, int *out_form, int *out_sweep,
                          int *out_lds_kb);
// the per-env overlay of that kernel: its slot count, and one env's column from the env's gravity and its block of DevState::env_mass (NULL: the model's values)
int mjb_lane_env_overlay_slots(const mjb_model_desc *h);
// the wrench table of that kernel's XF builds: its slot count (the model's moving bodies), and the transpose of xfrc_applied [nenv][nbody][6] into
// table [6 * slots][nenv] for every env, on `stream`
int mjb_lane_env_xfrc_slots(const mjb_model_desc *h);
int mjb_lane_env_wrench_at_rest(const mjb_model_desc *h);  // 1: a force / torque sensor sits on a body at rest, whose xfrc_applied has no slot in that table -- no XF build for the model
int mjb_lane_env_xfrc_fill(const mjb_model_desc *h, const double *xfrc_applied, double *table, int nenv, void *stream);
void mjb_lane_env_overlay_row(const mjb_model_desc *h, const double *gravity, const double *env_block, double *out);
// the split step (mjb_smooth_kernel.h + mjb_cstep_kernel): one step of envs [env_lo, env_hi) -- smooth half in lane = env form, then the constraint half
int mjb_smooth_match(const mjb_model_desc *h);  // index of the compiled-in SmTopo the model has, or -1
const char *mjb_smooth_name(int topo);
int mjb_launch_smooth(const KernelParams *Pdev, int topo, int env_lo, int env_hi, unsigned int step, int flags, void *stream);
int mjb_launch_cstep(const KernelParams *Pdev, const FrameLayout &L, int env_lo, int env_hi, int envs_per_block, int flags, void *stream);
// batched ray casting (mjb_ray.hip): every ray of the table `tab` (pnt[3][nray] | vec[3][nray] as doubles, then {site, exclude own body}[nray] and visible[ngeom] as
// ints) against the geoms of every env, from the poses in DevState::frame_ws; results [nenv][nray].  The kernel stages geoms through LDS MJB_RAY_TILE records at a time
#define MJB_RAY_TILE 64
int mjb_launch_rays(const KernelParams *Pdev, const double *tab, int nenv, int nray, double *dist, int *geomid, void *stream);
// sensors-plugin equivalent (mjb_sensor_pack.hip)
int mjb_launch_sensor_pack(const KernelParams *Pdev, int nenv, int nsensor, const int *set_flag, const double *mean,
                           const double *sigma, unsigned long long seed, long long env_offset, unsigned int step,
                           float *value, float *truth, void *stream);
