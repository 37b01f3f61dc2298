// mjb_lane_env_kernel.h -- device code of the lane = env kernel (see mjb_lane_env.hip for what it is): a template over the model's integer
// structure `T` (a LeTopo_* struct: csrc/lane_env_topos.h, or the one mjb_lane_env.hip writes for hiprtc) and the LDS budget LP.
// Included by mjb_lane_env.hip (the compiled-in topologies) and by the source hiprtc compiles for any other eligible model.
//
// One body of the root -> leaf sweep as helpers, each per-body quantity once for `consume`, the quartet's o_body / x_body / v_* and the rest-pose prologue:
//   mj_kinematics   le_xipos (a frame's point in the world: a child's origin, xipos, an anchor), le_xquat, le_anchor, le_hinge_quat, le_pos_slide / _offcentre
//   mj_comPos       le_inert_rot + le_cinert_com (cinert in two halves: the quartet's C fetches between them), le_cdof_hinge / le_cdof_slide
//   mj_comVel, RNE  le_parent_motion (at rest | the parent's), le_body_motion<REST> (cvel, cacc), le_cfrc (cfrc_body's two summands)       (all: mjb_math.h)
//   across LDS      le_pairs_put / _get (cinert: 5 pairs, cdof: 3, a quaternion: 2), le_cfrc_put, le_ring_put / le_ring_get<MATFIRST>, le_cdof_ring_get<SLIDE>
// RULE: a helper holds arithmetic and LDS pair accesses only.  Every wait, pin and fetch (sched_barrier, touch_*, pinv / pins, LE_PK, le_barrier, loads of a
// tape record, an overlay or a wrench value) stays at the call site, in its order relative to the arithmetic.  Record fields are read by name (LE_*, mjb_dev.h).
// NOT on the helpers: the fused sweep (solo, two halves, the P of the pipelined duo and of the trio) and mjb_smooth_kernel.h keep the same expressions written
// out.  Under -ffp-contract=fast the backend picks which product of a sum of two it fuses, and moving those two bodies behind the helpers flipped some picks:
// same f64 opcode counts, results off by an ulp in a few envs (profiles/lane_env_body_math.txt).  Change a formula there AND in its helper.  `consume` also
// writes its cfrc store out (le_cfrc_put is v_force's): behind the helper the pipelined duo of franka_like gained 15 register copies and lost 0.2 % of its rate.
#pragma once
#ifndef __HIPCC_RTC__  // (hiprtc brings its own runtime header)
#include <hip/hip_runtime.h>
#endif

#include "mjb_dev.h"
#include "mjb_math.h"

namespace mjb_le {

// compile-time loop: f(IC<0>{}), f(IC<1>{}), ...  (own three-line integer sequence: the header is also compiled by hiprtc, without <utility>)
template <int V> struct IC {
	static constexpr int value = V;
	constexpr operator int() const { return V; }
};
template <int... Is> struct ISeq {};
template <int N, int... Is> struct MkSeq : MkSeq<N - 1, N - 1, Is...> {};
template <int... Is> struct MkSeq<0, Is...> { using type = ISeq<Is...>; };
template <typename F, int... Is> DEVI void sfor_impl(F &&f, ISeq<Is...>) { (f(IC<Is>{}), ...); }
template <int N, typename F> DEVI void sfor(F &&f) { sfor_impl(f, typename MkSeq<N>::type{}); }

DEVI double frcp(double x)
{
	double r = __builtin_amdgcn_rcp(x);
	r = fma(fma(-x, r, 1.0), r, r);
	r = fma(fma(-x, r, 1.0), r, r);
	return r;
}

// compile-time queries on a topology
template <class T> struct Tq {
	// dof a is dof i or one of its ancestors
	static constexpr bool anc(int a, int i)
	{
		for (int j = i; j >= 0; j = T::dof_parentid[j])
			if (j == a) return true;
		return false;
	}
	static constexpr bool is_root(int b) { return b > 0 && T::body_rootid[b] == b; }
	// entry e of MuJoCo's sparse qM (dof_Madr[i] + k: dof i with its k-th ancestor, itself first) -> i, a
	static constexpr int ent_i(int e)
	{
		int i = 0;
		for (int d = 0; d < T::NV; d++)
			if (T::dof_Madr[d] <= e) i = d;
		return i;
	}
	static constexpr int ent_a(int e)
	{
		int a = ent_i(e);
		for (int k = T::dof_Madr[ent_i(e)]; k < e; k++) a = T::dof_parentid[a];
		return a;
	}
	// some sensor of the model needs the pose of this site / body
	static constexpr bool has_actuator_sensor()
	{
		for (int i = 0; i < T::NSENSOR; i++)
			if (T::sensor_type[i] == MJB_SENS_ACTUATORFRC) return true;
		return false;
	}
};

// 1 / sqrt(x): hardware seed + two Newton steps (x > 0)
DEVI double frsq(double x)
{
	double y = __builtin_amdgcn_rsq(x);
	y = y * fma(-0.5 * x * y, y, 1.5);
	y = y * fma(-0.5 * x * y, y, 1.5);
	return y;
}

// mju_normalize4 of a body's world quaternion: untouched within mjMINVAL of unit length.  (Its identity case for a vanishing quaternion cannot
// occur here: the argument is a product of the model's unit quaternions and of (cos, axis sin) hinge quaternions.)
DEVI void normalize4_sel(double *q)
{
	const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
	const double r = frsq(n2), n = n2 * r;
	const double s = (fabs(n - 1) > MJB_MINVAL) ? r : 1.0;
	q[0] *= s;
	q[1] *= s;
	q[2] *= s;
	q[3] *= s;
}

// A loaded value the optimiser must treat as already there: `cond ? k : load` otherwise becomes a per-lane branch around the load.
DEVI double pinv(double x)
{
	asm volatile("" : "+v"(x));
	return x;
}
// "This value has to be HERE": the wait for a prefetched scalar / LDS value is taken at this point, BEFORE the next prefetch is issued.
// LDS reads and scalar loads share one counter and scalar loads return out of order, so any wait is a wait for everything in
// flight: a region that issues its successor's fetches first and then touches its own data waits for both.
DEVI void touch_s(double x) { asm volatile("" ::"s"(x)); }
DEVI void touch_v(double x) { asm volatile("" ::"v"(x)); }
// ... and a whole half record: placed at the END of the region that issued its loads, it keeps every one of them inside that region
// (left alone, the loads of entries first used late in the next region are sunk there and waited for on the spot)
template <int N> DEVI void touch_rec(const double *h)  // (the N entries the sweep reads)
{
	asm volatile("" ::"s"(h[0]), "s"(h[1]), "s"(h[2]), "s"(h[3]), "s"(h[4]), "s"(h[5]), "s"(h[6]), "s"(h[7]), "s"(h[8]), "s"(h[9]));
	if constexpr (N > 10) asm volatile("" ::"s"(h[10]), "s"(h[11]), "s"(h[12]), "s"(h[13]));
}
// ... and N loaded per-lane values at once (a row of the packed AR): their reads leave together and are waited for once, instead of one wait per use
template <int N> DEVI void touch_vn(const double *a)
{
	if constexpr (N >= 8) {
		asm volatile("" ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]));
		touch_vn<N - 8>(a + 8);
	} else if constexpr (N >= 4) {
		asm volatile("" ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
		touch_vn<N - 4>(a + 4);
	} else if constexpr (N >= 2) {
		asm volatile("" ::"v"(a[0]), "v"(a[1]));
		touch_vn<N - 2>(a + 2);
	} else if constexpr (N == 1) asm volatile("" ::"v"(a[0]));
}
DEVI double pins(double x)  // the same for a wave-uniform (scalar) value
{
	asm volatile("" : "+s"(x));
	return x;
}
// clamp by v_max / v_min, NaN passed through as the ternary chain of mj_fwdActuation passes it
DEVI double clampd(double c, double lo, double hi)
{
	const double v = fmin(fmax(c, lo), hi);
	return c != c ? c : v;
}

DEVI bool bad_val(double x) { return !(fabs(x) <= MJB_MAXVAL); }  // NaN or beyond mjMAXVAL: one unordered compare

// sin and cos of a joint half-angle, branch-free: k = round(x * 2/pi), r = x - k * pi/2 through three fma steps (pi/2 split into
// 53-bit pieces: exact to rounding while |x| < ~1e6 rad; beyond, the absolute error grows like |x| * 2^-53 * k-independent terms --
// a hinge wound up that far is not a simulation any more, and mj_check* only stops it at 1e10), then the fdlibm kernel polynomials on
// [-pi/4, pi/4] and a quadrant swap.  libm's sincos carries a divergent slow path for huge arguments; this kernel must not branch
// per lane (see the note on divergent control flow at the kernel).
DEVI void sincos_nb(double x, double *sn, double *cs)
{
	const double k = rint(x * 0.63661977236758134308);
	double r = fma(-k, 1.57079632679489655800e+00, x);
	r = fma(-k, 6.12323399573676603587e-17, r);
	r = fma(-k, -1.49738490485916983827e-33, r);
	const double z = r * r;
	// __kernel_sin / __kernel_cos (fdlibm), tail argument dropped (|r| <= pi/4 to rounding)
	const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
	             S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
	const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
	             C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
	const double ps = fma(fma(fma(fma(fma(S6, z, S5), z, S4), z, S3), z, S2), z, S1);
	const double sr = fma(z * r, ps, r);
	const double pc = fma(fma(fma(fma(fma(C6, z, C5), z, C4), z, C3), z, C2), z, C1);
	const double cr = fma(z * z, pc, fma(-0.5, z, 1.0));
	const int q = (int)k & 3;
	const double s0 = (q & 1) ? cr : sr, c0 = (q & 1) ? sr : cr;
	*sn = (q & 2) ? -s0 : s0;
	*cs = ((q + 1) & 2) ? -c0 : c0;
}

// ---- the hwsim stage's helpers (HW builds; hwsim_write of mjb_step.hip for one env per lane), branch-free: lanes of one wavefront disagree on every
// test in them.  Same operations on the same values as the generic kernel's ros_ns / angdist / angdist_with_limits, as selects.
// fmod(x, y), y > 0, without libm's per-lane loop: the truncated quotient from one IEEE division (off by at most one while |x / y| < 2^53), put right by
// the sign of a first remainder, then x - q y in one fma -- fmod's result is exactly representable, so that fma returns it exactly.  (|x / y| >= 2^53,
// i.e. an angle beyond 5e16 rad, is not reduced exactly; mj_checkPos stops a joint at 1e10.)
DEVI double seld(bool c, double a, double b) { return c ? a : b; }  // (both values evaluated by the caller: a select, whatever they cost)
DEVI long long sell(bool c, long long a, long long b) { return c ? a : b; }
DEVI double fmod_nb(double x, double y)
{
	const double ax = fabs(x);
	const double q0 = trunc(ax / y);
	const double r0 = fma(-q0, y, ax);
	const double q = seld(r0 < 0, q0 - 1.0, seld(r0 >= y, q0 + 1.0, q0));
	return copysign(fma(-q, y, ax), x);
}
DEVI long long ros_ns_nb(double t)  // ros::Time(double).toNSec(): sec = floor(t), nsec = round((t - sec) 1e9)
{
	const double sec = floor(t);
	return (long long)sec * 1000000000LL + (long long)floor((t - sec) * 1e9 + 0.5);
}
DEVI double angdist_nb(double from, double to)  // angles::shortest_angular_distance
{
	const double two_pi = 6.283185307179586476925;
	const double a = fmod_nb(fmod_nb(to - from, two_pi) + two_pi, two_pi);  // normalize_angle_positive
	return seld(a > 0.5 * two_pi, a - two_pi, a);
}
DEVI double two_pi_complement_nb(double a0)
{
	const double two_pi = 6.283185307179586476925;
	const double a = seld((a0 > two_pi) | (a0 < -two_pi), fmod_nb(a0, two_pi), a0);
	return seld(a < 0, two_pi + a, seld(a > 0, -two_pi + a, two_pi));
}
DEVI bool find_min_max_delta_nb(double from, double left, double right, double &dmin, double &dmax)
{
	const double pi = 3.14159265358979323846;
	const double d0 = angdist_nb(from, left), d1 = angdist_nb(from, right), d2 = two_pi_complement_nb(d0), d3 = two_pi_complement_nb(d1);
	const bool c2 = d2 < d0, c3 = d3 > d1;
	const double lo = seld(c2, d2, d0), lo2 = seld(c2, d0, d2), hi = seld(c3, d3, d1), hi2 = seld(c3, d1, d3);
	const bool cross = (lo <= hi2) | (hi >= lo2), z0 = d0 == 0, z1 = d1 == 0;
	dmin = seld(z0, d0, seld(z1, fmin(d0, d2), seld(cross, hi2, lo)));
	dmax = seld(z0, fmax(d1, d3), seld(z1, d1, seld(cross, lo2, hi)));
	return z0 | z1 | !cross | ((left == -pi) & (right == pi));
}
DEVI double angdist_with_limits_nb(double from, double to, double left, double right)  // angles::shortest_angular_distance_with_limits
{
	double dmin, dmax, tmin, tmax;
	const bool inside = find_min_max_delta_nb(from, left, right, dmin, dmax);
	const double delta = angdist_nb(from, to), comp = two_pi_complement_nb(delta);
	find_min_max_delta_nb(to, left, right, tmin, tmax);
	const double nearer = seld(fabs(delta) < fabs(comp), delta, comp), mx = fmax(delta, comp), mn = fmin(delta, comp);
	const double byto = seld(fabs(tmin) < fabs(tmax), mx, seld(fabs(tmin) > fabs(tmax), mn, nearer));
	const double in = seld((delta >= dmin) & (delta <= dmax), delta, seld((comp >= dmin) & (comp <= dmax), comp, byto));
	const double out = seld(fabs(dmin) < fabs(dmax), mn, seld(fabs(dmin) > fabs(dmax), mx, nearer));
	return seld(inside, in, out);
}

// LDS of a block (= one wavefront): pair slot q of lane l = the two doubles at (q * 64 + l) * 16 bytes -- one ds_read_b128 /
// ds_write_b128 per pair, conflict-free.  Slots [0, NV): (qpos_i, qvel_i); then three slots per body whose force the backward
// sweep reads (cfrc_body); then, while the budget LP lasts, five per body for its cinert (leaf-most bodies first): the wavefront's
// overflow space next to its registers.  LP = 40 pair slots (40 KB) when four wavefronts share a CU, 80 / 160 when the batch leaves
// a CU to two / one (the launcher picks): what does not fit stays in registers, i.e. mostly in their AGPR half, at four moves per
// double and round trip against one LDS instruction per PAIR and direction.
// ---- the LDS layouts of every form, counted ONCE, in pair slots, from plain integers: nv, nmov = the bodies whose force the backward sweep reads
// (Lds<>::needed), nbody, and a budget.  The kernel's offsets and the *_bytes<T>() of the compiled-in topologies below are written with these; the
// launcher's fit test for hiprtc-built models (le_plan, mjb_lane_env.hip) calls them with the model's counts.  A slot is one KB: budgets are in both.
constexpr int LE_SLOT_BYTES = 64 * 16;
constexpr int LE_MAX_SLOTS = mjb_max_lds_bytes() / LE_SLOT_BYTES;  // a CU's LDS
constexpr int RING_DUO2 = 2, RING_TRIO = 3;  // depth of the pose ring: the pipelined duo's V reads one body behind P, the trio's (and quartet's) two
constexpr int le_ring_slots(int depth) { return 6 * depth; }  // (xpos, xmat) of a body: 12 doubles
// pair slots of a quartet block behind the trio's layout: O's quaternion ring (2 x 4), C's cdof ring (2 x 3), X's mail slot
constexpr int QUARTET_EXTRA = 15;
// (nr: the constraint rows of a model that has them, LeLimQ -- the packed AR of the constraint stage, nr (nr + 1) / 2 doubles, and qacc_warmstart of the
//  nw dofs the rows touch (a limit-only model: nw = nr), two doubles to a pair slot, behind cfrc_body: one-wavefront form only)
constexpr int le_lim_slots(int nr, int nw) { return (nr * (nr + 1) / 2 + nw + 1) / 2; }
constexpr int le_state_slots(int nv, int nmov, int nr = 0, int nw = 0) { return nv + 3 * nmov + le_lim_slots(nr, nw); }  // (qpos, qvel) pairs + cfrc_body: what every form must hold
constexpr int le_solo_slots(int nv, int nmov, int budget, int nr = 0, int nw = 0)  // ... + five of cinert per body while the budget lasts
{
	int at = le_state_slots(nv, nmov, nr, nw);
	for (int k = 0; k < nmov; k++)
		if (at + 5 <= budget) at += 5;
	return at;
}
constexpr int le_full_slots(int nv, int nmov) { return le_state_slots(nv, nmov) + 5 * nmov; }  // ... of every body (the pipelined forms)
constexpr int le_exchange_slots(int nv) { return (nv + 1) / 2 + 1; }                           // qfrc_smooth pairs + the mail slot
constexpr int le_duo_slots(int nv, int nmov, int budget) { return le_solo_slots(nv, nmov, budget - le_exchange_slots(nv)) + le_exchange_slots(nv); }
constexpr int le_duo2_slots(int nv, int nmov) { return le_full_slots(nv, nmov) + le_ring_slots(RING_DUO2) + le_exchange_slots(nv); }
constexpr int le_trio_slots(int nv, int nmov, int nbody) { return le_full_slots(nv, nmov) + le_ring_slots(RING_TRIO) + le_exchange_slots(nv) + nbody; }  // (+ a (sin, cos) slot per body)
constexpr int le_quartet_slots(int nv, int nmov, int nbody) { return le_trio_slots(nv, nmov, nbody) + QUARTET_EXTRA; }

// Constraint rows (a model whose only rows are joint-equality rows and hinge / slide joint-limit rows under PGS, mjb_lane_env_eligible): a topology may
// list its limited joints, jnt_limited[NJNT], and the joint pairs of its active joint equalities, eq_jnt1[] / eq_jnt2[] (-1: the one-joint form) -- the
// hiprtc-built ones of such models do; a topology without the arrays has no constraint stage.  The static row list is MuJoCo's: the equalities in equality
// order, then the limited joints in joint order; every number of a row is run-time data (LeTapeEq, LeTapeLim).  One-wavefront form, plain build only.
template <class T, class = void> struct LeLim { static constexpr bool on(int) { return false; } };
template <class T> struct LeLim<T, decltype((void)T::jnt_limited)> { static constexpr bool on(int j) { return T::jnt_limited[j] != 0; } };
template <class T, class = void> struct LeEq {
	static constexpr int n = 0;
	static constexpr int j1(int) { return 0; }
	static constexpr int j2(int) { return -1; }
};
template <class T> struct LeEq<T, decltype((void)T::eq_jnt1)> {
	static constexpr int n = (int)(sizeof(T::eq_jnt1) / sizeof(int));
	static constexpr int j1(int e) { return T::eq_jnt1[e]; }
	static constexpr int j2(int e) { return T::eq_jnt2[e]; }
};
template <class T> struct LeLimQ {
	static constexpr int ne() { return LeEq<T>::n; }                                                                     // equality rows: the first ne()
	static constexpr int nl() { int k = 0; for (int j = 0; j < T::NJNT; j++) if (LeLim<T>::on(j)) k++; return k; }  // limit rows: behind them
	static constexpr int n() { return ne() + nl(); }
	static constexpr bool is_eq(int r) { return r < ne(); }
	// the row's joint (= its dof: one-dof joints in dof order), and an equality row's second joint (-1: none)
	static constexpr int jnt(int r)
	{
		if (r < ne()) return LeEq<T>::j1(r);
		int k = ne();
		for (int j = 0; j < T::NJNT; j++) if (LeLim<T>::on(j) && k++ == r) return j;
		return 0;
	}
	static constexpr int jnt2(int r) { return r < ne() ? LeEq<T>::j2(r) : -1; }
	// entry a of M^-1 e_j is not a known zero: dofs a and j share an ancestor (or one is the other's)
	static constexpr bool coupled(int a, int j) { for (int d = 0; d < T::NV; d++) if (Tq<T>::anc(d, a) && Tq<T>::anc(d, j)) return true; return false; }
	// ... of M^-1 J_r': the union over the row's dofs;  dof i is one of the row's dofs or an ancestor of one;  AR_kr is not a known zero
	static constexpr bool rcoupled(int a, int r) { return coupled(a, jnt(r)) || (jnt2(r) >= 0 && coupled(a, jnt2(r))); }
	static constexpr bool ranc(int i, int r) { return Tq<T>::anc(i, jnt(r)) || (jnt2(r) >= 0 && Tq<T>::anc(i, jnt2(r))); }
	static constexpr bool rows_coupled(int k, int r) { return rcoupled(jnt(k), r) || (jnt2(k) >= 0 && rcoupled(jnt2(k), r)); }
	// the dofs some row touches, in dof order: their qacc_warmstart and qfrc_constraint live with the stage (a limit-only model: the limited dofs, row order)
	static constexpr bool in_rows(int d) { for (int r = 0; r < n(); r++) if (jnt(r) == d || jnt2(r) == d) return true; return false; }
	static constexpr int nw() { int k = 0; for (int d = 0; d < T::NV; d++) if (in_rows(d)) k++; return k; }
	static constexpr int widx(int d) { int k = 0; for (int a = 0; a < d; a++) if (in_rows(a)) k++; return k; }
	static constexpr int wdof(int w) { int k = 0; for (int d = 0; d < T::NV; d++) if (in_rows(d) && k++ == w) return d; return 0; }
	static constexpr int ar(int i, int k) { const int a = i < k ? i : k, b = i < k ? k : i; return a * n() - a * (a - 1) / 2 + (b - a); }  // AR_ik = AR_ki in the packed triangle
	static constexpr int ws(int w) { return n() * (n() + 1) / 2 + w; }  // qacc_warmstart of the w-th such dof, behind the triangle
	static constexpr int slots() { return le_lim_slots(n(), nw()); }
};
// Fixed tendons (mjb_lane_env_eligible: they carry actuators and nothing else): a topology may list which actuators drive a tendon, act_tendon[NU] (-1:
// a joint actuator), and every tendon's wraps, tendon_adr[] / tendon_num[] / wrap_jnt[] -- the hiprtc-built ones of such models do; for a topology without
// the arrays every actuator is a joint actuator.  The moment arm of a tendon actuator is the compile-time list of its wraps' dofs; the coefficients are
// run-time data (LeTapeWrap, behind the row records of the tape).
template <class T, class = void> struct LeTen {
	static constexpr int nwrap = 0;
	static constexpr bool on(int) { return false; }
	static constexpr int num(int) { return 0; }
	static constexpr int wrap(int, int) { return 0; }
	static constexpr int jnt(int, int) { return 0; }
};
template <class T> struct LeTen<T, decltype((void)T::act_tendon)> {
	static constexpr int nwrap = (int)(sizeof(T::wrap_jnt) / sizeof(int));
	static constexpr bool on(int i) { return T::act_tendon[i] >= 0; }
	static constexpr int num(int i) { return on(i) ? T::tendon_num[T::act_tendon[i]] : 0; }
	static constexpr int wrap(int i, int k) { return T::tendon_adr[T::act_tendon[i]] + k; }  // the actuator's k-th wrap: its record of the tape ...
	static constexpr int jnt(int i, int k) { return T::wrap_jnt[wrap(i, k)]; }               // ... and its dof
};

template <class T, int LP> struct Lds {
	using Q = Tq<T>;
	// the body's cfrc is consumed by the backward sweep (it, or an ancestor, carries a joint)
	static constexpr bool needed(int b)
	{
		for (int a = b; a > 0; a = T::body_parentid[a])
			if (T::body_jnt[a] >= 0) return true;
		return false;
	}
	static constexpr int slot(int b)  // first of the body's three pair slots
	{
		int n = 0;
		for (int a = 1; a < b; a++)
			if (needed(a)) n++;
		return T::NV + 3 * n;
	}
	static constexpr int cin_slot(int b)  // first of the body's five cinert slots, -1: the body's cinert stays in registers
	{
		int at = slot(T::NBODY) + LeLimQ<T>::slots();
		for (int a = T::NBODY - 1; a >= 1; a--) {
			if (!needed(a)) continue;
			if (at + 5 > LP) return -1;
			if (a == b) return at;
			at += 5;
		}
		return -1;
	}
	static constexpr int nmov() { return (slot(T::NBODY) - T::NV) / 3; }  // the needed bodies
	static constexpr int nslots() { return le_solo_slots(T::NV, nmov(), LP, LeLimQ<T>::n(), LeLimQ<T>::nw()); }
	static constexpr int bytes() { return nslots() * LE_SLOT_BYTES; }
};

struct alignas(16) Pair { double a, b; };

// The per-env overlay (DevState::le_overlay, PE kernels): the tape's numbers an env may carry its own value of (mjb_set_env_*), as rows
// [slot][env] -- a wavefront's 64 lanes read 64 consecutive doubles.  Slots: gravity[3]; per JOINTED body, in body order, stiffness |
// damping | armature | hdamping; per MOVING body (a joint on its path to the world) mass | ibody[6]; per actuator gain[3] | bias[3];
// then the mass of every body at rest but the world (mj_energyPos alone reads it).  mjb_lane_env_overlay_row (mjb_lane_env.hip) fills
// a column in this order.
template <class T> struct PeSlots {
	static constexpr bool moving(int b) { return Lds<T, (1 << 20)>::needed(b); }
	static constexpr int njb(int b) { int n = 0; for (int a = 1; a < b; a++) if (T::body_jnt[a] >= 0) n++; return n; }  // jointed bodies ahead of b
	static constexpr int nmb(int b) { int n = 0; for (int a = 1; a < b; a++) if (moving(a)) n++; return n; }             // moving bodies ahead of b
	static constexpr int gravity(int k) { return k; }
	static constexpr int joint(int b, int f) { return 3 + 4 * njb(b) + f; }  // f: 0 stiffness, 1 damping, 2 armature, 3 hdamping
	static constexpr int inert(int b, int f) { return 3 + 4 * njb(T::NBODY) + 7 * nmb(b) + f; }  // f: 0 mass, 1 .. 6 ibody
	static constexpr int act(int i, int f) { return 3 + 4 * njb(T::NBODY) + 7 * nmb(T::NBODY) + 6 * i + f; }  // f: 0 .. 2 gain, 3 .. 5 bias
	static constexpr int rest(int b) { return act(T::NU, 0) + (b - 1 - nmb(b)); }
	static constexpr int n = act(T::NU, 0) + (T::NBODY - 1 - nmb(T::NBODY));
};

// The wrench table (DevState::le_xfrc, XF kernels): xfrc_applied of the MOVING bodies as rows [6 * slot + k][env], k = force[3] | torque[3] as in
// mjData.xfrc_applied -- a wavefront's 64 lanes read 64 consecutive doubles.  A body at rest (the world, a jointless chain down from it) has no
// slot: its wrench moves nothing.  mjb_lane_env_xfrc_fill (mjb_lane_env.hip) transposes the canonical [env][nbody][6] array into it.
template <class T> struct XfSlots {
	static constexpr int slot(int b) { return PeSlots<T>::nmb(b); }
	static constexpr int n = PeSlots<T>::nmb(T::NBODY);
};

// Gravity compensation (mjModel.body_gravcomp): a topology may flag its compensated bodies, body_gc[NBODY] (the hiprtc-built ones do; a topology
// without the array has none).  The coefficient itself is run-time data, LeTapeBody::gravcomp.
template <class T, class = void> struct LeGc { static constexpr bool on(int) { return false; } };
template <class T> struct LeGc<T, decltype((void)T::body_gc)> { static constexpr bool on(int b) { return T::body_gc[b] != 0; } };
template <class T> constexpr bool le_any_gc() { for (int b = 1; b < T::NBODY; b++) if (LeGc<T>::on(b)) return true; return false; }

// Sensors beyond poses and joint / actuator scalars: the set is a compile-time fact of the topology (T::sensor_type[]), like LeGc.  Frame axes ride with
// the pose sensors; velocity-stage sensors (velocimeter, gyro, framelinvel, frameangvel) are evaluated in the root -> leaf sweep where cvel is formed;
// acceleration-stage sensors (accelerometer, force, torque, framelinacc, frameangacc) in a post pass behind the qacc solve -- mj_rnePostConstraint for the
// lane.  A topology without them has none of that code.  One-wavefront form only, every build of it.
constexpr bool le_axis_type(int t) { return t == MJB_SENS_FRAMEXAXIS || t == MJB_SENS_FRAMEYAXIS || t == MJB_SENS_FRAMEZAXIS; }
constexpr bool le_vel_type(int t) { return t == MJB_SENS_VELOCIMETER || t == MJB_SENS_GYRO || t == MJB_SENS_FRAMELINVEL || t == MJB_SENS_FRAMEANGVEL; }
constexpr bool le_wrench_type(int t) { return t == MJB_SENS_FORCE || t == MJB_SENS_TORQUE; }
constexpr bool le_accel_type(int t) { return t == MJB_SENS_ACCELEROMETER || t == MJB_SENS_FRAMELINACC || t == MJB_SENS_FRAMEANGACC; }
constexpr bool le_acc_type(int t) { return le_wrench_type(t) || le_accel_type(t); }
template <class T> struct LeSens {
	static constexpr bool any(bool (*is)(int)) { for (int i = 0; i < T::NSENSOR; i++) if (is(T::sensor_type[i])) return true; return false; }
	static constexpr bool vel() { return any(le_vel_type); }  // has a velocity-stage sensor
	static constexpr bool acc() { return any(le_acc_type); }  // has an acceleration-stage sensor
	static constexpr bool extra() { return vel() || acc() || any(le_axis_type); }
	static constexpr int body(int i) { return T::sensor_objtype[i] == MJB_OBJ_SITE ? T::site_bodyid[T::sensor_objid[i]] : T::sensor_objid[i]; }  // the body sensor i's object sits on
	static constexpr bool on(int b, bool (*is)(int)) { for (int i = 0; i < T::NSENSOR; i++) if (is(T::sensor_type[i]) && body(i) == b) return true; return false; }
	static constexpr bool under(int b, int a) { for (int c = b; c > 0; c = T::body_parentid[c]) if (c == a) return true; return false; }  // b is a or in a's subtree (a > 0)
	// some body of b's subtree (b included) carries such a sensor / b is in the subtree of a body that does
	static constexpr bool above(int b, bool (*is)(int)) { for (int c = b; c < T::NBODY; c++) if (under(c, b) && on(c, is)) return true; return false; }
	static constexpr bool below(int b, bool (*is)(int)) { for (int a = b; a > 0; a = T::body_parentid[a]) if (on(a, is)) return true; return false; }
};

// Off-centre anchors (mjModel.jnt_pos != 0): a topology may flag them per joint, jnt_offc[NJNT] (the generated and the hiprtc-built ones do, and
// mjb_lane_env_match compares the flags).  Where the flags are known AND the caller asks for them (USE: the quartet's roles -- every other form keeps
// its code as it is), "is this anchor off centre" is a constant and the untaken side compiles to nothing; otherwise it is the run-time test on the
// tape's jpos, wave-uniform.
template <class T, class = void> struct LeOffc { static constexpr bool known = false; static constexpr bool on(int) { return false; } };
template <class T> struct LeOffc<T, decltype((void)T::jnt_offc)> { static constexpr bool known = true; static constexpr bool on(int j) { return T::jnt_offc[j] != 0; } };
template <class T, bool USE, int J> DEVI bool le_offc(const double jx, const double jy, const double jz)
{
	if constexpr (USE && LeOffc<T>::known) return LeOffc<T>::on(J);
	else return jx != 0 || jy != 0 || jz != 0;
}

// ROLE of a wavefront (lane_env_body's template argument, an int with these values): which part of the step of its block's 64 envs it runs.
enum LeRole : int {
	// one wavefront runs the whole step of its 64 envs
	LE_SOLO = 0,
	// the DUO form, two wavefronts of one workgroup (on two SIMDs of a CU) share the 64 envs of the block: the step's two independent halves -- what
	// depends on qpos alone (poses, cinert, composite inertias, qM, both factors: "P") and what depends on qvel too (velocities, the bodies' forces, the
	// force block, qfrc_smooth: "V") -- run side by side, V hands qfrc_smooth over through LDS, P solves and integrates, and hands the new state (which
	// lives in LDS anyway) and the mj_check* verdicts back.  Both compute the poses, cdof and cinert (the shared prefix).  A lone wavefront issues one
	// instruction every ~4 cycles whatever it is, so the step's length is its instruction count: ~6.2 k in one piece, ~max(P, V) + solve + Euler in
	// two.  Pays while the batch leaves SIMDs idle (the launcher).
	LE_DUO_P = 1,
	LE_DUO_V = 2,
	// the PIPELINED duo: P computes every pose and cinert ONCE and passes them on body by body -- a workgroup barrier per body, a two-deep ring of
	// (xpos, xmat) in LDS -- V follows one body behind with cdof, velocities and forces and passes cdof back for P's composite-inertia sweep.  Nothing
	// is computed twice; needs every needed body's cinert and cdof in LDS: duo2_bytes<T>().
	LE_PIPE_P = 3,
	LE_PIPE_V = 4,
	// the TRIO, three wavefronts per 64 envs: P runs the pose chain and nothing else; C follows it through the ring with cinert and cdof, then takes
	// the composite-inertia sweep, qM, both factors, the solves and Euler; V as the pipelined V, with its own cinert of every body.  P's sweep is the
	// step's critical chain: everything that is not a pose is off it.
	LE_TRIO_P = 5,
	LE_TRIO_C = 6,
	LE_TRIO_V = 7,
	// the QUARTET, the trio with its pose wavefront cut in two, on the CU's fourth SIMD: O runs the ORIENTATION chain and nothing else -- xquat[b] =
	// normalize(xquat[p] body_quat hinge_quat), the one part of a pose the next body's waits for -- with every hinge's half-angle sine and cosine one
	// body ahead, and passes the unit quaternion on through a two-deep ring; X follows one body behind: rotation matrix, the position chain, inertial
	// frame, mj_energyPos, frame sensors, the pose ring; C as the trio's C one body behind X, without the sines, and it publishes cdof; V as the trio's V
	// one body behind C, with C's cdof instead of its own.  One barrier per MOVING body plus two to drain: sweep phase k has O on the k-th moving body,
	// X on the one before, C two and V three before; the bodies at rest are O's and X's own business ahead of the phases.
	// The quartet's tail is split by MATRIX: X takes every joint's cdof from C's ring one phase after C wrote it (where V reads it, one phase before C
	// writes the slot again -- X computes none: it is the wavefront the phases wait for), reads C's cinert from LDS behind the sweep's last barrier,
	// builds qM a second time beside C from those very numbers, factors M, solves qacc = M^-1 f and takes mj_checkAcc's decision; C factors M + h B alone, solves the acceleration Euler advances with
	// and integrates SPECULATIVELY -- X's verdict, read by all four behind rendezvous B, either lets the step stand or has C put the old state back.
	// Nothing but V's qfrc_smooth and the two mail slots crosses LDS, and the step has no barrier the trio's tail does not have.
	// Where a phase's loads and stores sit (one wavefront per SIMD: nobody covers a wait): O and X fetch the next body's tape record at the top of a phase
	// and pin it at its end; X reads C's cdof beside O's quaternion at the top.  C holds its body's record (ipos, ibody, mass, jaxis, an off-centre jpos:
	// hC) from the phase BEFORE -- the first from ahead of the phases --, so the pose ring's six reads are waited for by count, in the order of their
	// use, and fetches the next record once they have landed, under the rest of cinert and the cdof half.  V runs a body's force half one phase BEHIND
	// its velocity half: a phase issues its body's nine reads (cinert, cdof, qvel), works off the previous body's cfrc from registers while they land --
	// the three cfrc writes leave mid-phase and drain under the velocities --, then takes its body's cvel / cacc; the cinert waits in registers across
	// the barrier, and the last body's forces come behind the sweep's last barrier with its velocities.
	LE_QUAD_O = 8,
	LE_QUAD_X = 9,
	LE_QUAD_C = 10,
	LE_QUAD_V = 11,
};
constexpr bool le_two_halves(int role) { return role == LE_DUO_P || role == LE_DUO_V; }
constexpr bool le_pipelined_duo(int role) { return role == LE_PIPE_P || role == LE_PIPE_V; }
constexpr bool le_trio(int role) { return role == LE_TRIO_P || role == LE_TRIO_C || role == LE_TRIO_V; }
constexpr bool le_quartet(int role) { return role == LE_QUAD_O || role == LE_QUAD_X || role == LE_QUAD_C || role == LE_QUAD_V; }
// rendezvous of a DUO block's two wavefronts: LDS traffic done, then the barrier.  (__syncthreads() also waits for the wavefront's outstanding GLOBAL
// loads -- V's ctrl-noise normals and qfrc_applied are fetched a sweep ahead of their use precisely so that nobody waits for HBM)
DEVI void le_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int NV> struct DuoSlots { static constexpr int n = le_exchange_slots(NV); };  // qfrc_smooth pairs + the mail slot
// ---- the per-body quantities that cross LDS, each layout once (slot: the lane's first pair slot of the quantity, pair k at slot[64 * k]); no wait, pin or fetch
template <int N> DEVI void le_pairs_put(Pair *slot, const double *v) { for (int k = 0; k < N; k++) slot[64 * k] = Pair{ v[2 * k], v[2 * k + 1] }; }  // cinert: 5 | cdof: 3
template <int N> DEVI void le_pairs_get(double *v, const Pair *slot)
{
	for (int k = 0; k < N; k++) {
		const Pair c = slot[64 * k];
		v[2 * k] = c.a;
		v[2 * k + 1] = c.b;
	}
}
DEVI void le_cfrc_put(Pair *slot, const double *cf, const double *t1)
{
	slot[0] = Pair{ cf[0] + t1[0], cf[1] + t1[1] };
	slot[64] = Pair{ cf[2] + t1[2], cf[3] + t1[3] };
	slot[128] = Pair{ cf[4] + t1[4], cf[5] + t1[5] };
}
// the pose ring, six pairs a body: its position relative to the tree root's origin, then its frame.  MATFIRST (the quartet's C): the reads in the
// order of their first use -- the matrix rows, then the position --, so that its counted waits release the cinert chain first
DEVI void le_ring_put(Pair *slot, const double *xp, const double *xm)
{
	slot[0] = Pair{ xp[0], xp[1] };
	slot[64] = Pair{ xp[2], xm[0] };
	slot[128] = Pair{ xm[1], xm[2] };
	slot[192] = Pair{ xm[3], xm[4] };
	slot[256] = Pair{ xm[5], xm[6] };
	slot[320] = Pair{ xm[7], xm[8] };
}
template <bool MATFIRST> DEVI void le_ring_get(double *xp, double *xm, const Pair *slot)
{
	Pair a0, a1, a2, a3, a4, a5;
	if constexpr (MATFIRST) { a1 = slot[64]; a2 = slot[128]; a3 = slot[192]; a4 = slot[256]; a5 = slot[320]; a0 = slot[0]; }
	else { a0 = slot[0]; a1 = slot[64]; a2 = slot[128]; a3 = slot[192]; a4 = slot[256]; a5 = slot[320]; }
	xp[0] = a0.a; xp[1] = a0.b; xp[2] = a1.a; xm[0] = a1.b; xm[1] = a2.a; xm[2] = a2.b; xm[3] = a3.a; xm[4] = a3.b; xm[5] = a4.a; xm[6] = a4.b; xm[7] = a5.a; xm[8] = a5.b;
}
// the quartet's cdof ring (C's le_pairs_put<3>): a slide's rotational half is zero whatever the slots hold
template <bool SLIDE> DEVI void le_cdof_ring_get(double *cd, const Pair *slot)
{
	const Pair d0 = slot[0], d1 = slot[64], d2 = slot[128];
	cd[0] = d0.a; cd[1] = d0.b; cd[2] = d1.a; cd[3] = d1.b; cd[4] = d2.a; cd[5] = d2.b;
	if constexpr (SLIDE) cd[0] = cd[1] = cd[2] = 0;
}
// PE: the batch carries per-env overrides (mjb_set_lane_env mode 2): gravity, the joint constants, masses / inertias and the actuator gains come
// per lane from DevState::le_overlay instead of the tape (solo form only).
// HW: the batch has a device hwsim stage (KernelParams::hw, mjb_lane_env_set_hwsim): DefaultRobotHWSim::writeSim runs per lane where the forces are
// assembled -- behind the root -> leaf sweep, which is where the generic kernels run hwsim_write (between forward_first and forward_rest), inside the
// attempt loop.  Which dof is controlled, and how, is wave-uniform run-time data (HwSim::le_tab / le_gains, by dof): scalar loads and wave-uniform
// branches around per-lane selects.  Commands, PID state and cadence stamps are fetched per lane ([env][n] rows: strided) in the sweep's last region,
// beside qfrc_applied, and PID state, stamps and the controlled dofs' qfrc_applied go back to HBM at every step -- qfrc_applied is STATE under the
// stage (a step without a write keeps the last one's) and the generic kernels continue the same batch.  A POSITION / VELOCITY joint's new qpos / qvel
// wait in registers for mj_Euler: everything between the stage and Euler (passive forces, actuator length / velocity, joint sensors, energy) was
// computed by forward_first from the old state in the generic kernels.  Solo form only; no build with PE.
// XF: the batch carries xfrc_applied (mjb_lane_env_set_xfrc): mj_xfrcAccumulate rides in the root -> leaf sweep.  A moving body's wrench (f, t) acts at
// its xipos; as a spatial force about the tree root's origin, (t + (xipos - origin) x f ; f), it is taken off the body's cfrc_body where that is
// formed, so the leaf -> root sweep's projection on cdof yields qfrc_bias - J' xfrc and qfrc_smooth gains + J' xfrc: no pass of its own.  The wrench
// is constant over the launch but there is no register or LDS to keep 6 doubles per body in: every step re-reads it from DevState::le_xfrc
// (XfSlots), coalesced, one region ahead of its use.  mj_resetData zeroes xfrc_applied: a lane reset inside the launch reads zero from then on
// (the retry after a mj_checkAcc reset included), and at the launch's end its rows of xfrc_applied and its column of the table are zeroed in HBM.
// Solo form only; composes with PE, not with HW.
// Gravity compensation (LeGc<T>: a compile-time flag per body, no code for the others): mj_passive's force F = -gravity * mass * gravcomp at the
// body's xipos is folded where XF folds a wrench -- (xd x F ; F) about the tree root's origin off the body's cfrc_body -- with the step's own
// grav[] (zero under mjDSBL_GRAVITY, the env's under PE), the mass the inertial half already holds (the env's under PE) and pas_on.  The kernel keeps
// no qfrc_passive: the term reaches qfrc_smooth through the leaf -> root projection.  Solo form only, every build of it.
template <class T, int LP, int ROLE = LE_SOLO, bool PE = false, bool HW = false, bool XF = false>
DEVI void lane_env_body(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0, const int env_lo, const int env_hi,
                        unsigned char *const smem_le)
{
	constexpr int NB = T::NBODY, NV = T::NV, NU = T::NU, NA = T::NA;
	// ---- what this wavefront does, from its role: the one place a role is looked at by group
	constexpr bool QUAD = le_quartet(ROLE), TRIQ = le_trio(ROLE) || QUAD;  // of four wavefronts / of three or four
	constexpr bool HALVES = ROLE == LE_SOLO || le_two_halves(ROLE);         // computes every pose and cinert itself: solo, or either half of the two-halves duo
	constexpr bool DP = ROLE == LE_SOLO || ROLE == LE_DUO_P || ROLE == LE_PIPE_P || ROLE == LE_TRIO_C || ROLE == LE_QUAD_C, DV = ROLE == LE_SOLO || ROLE == LE_DUO_V || ROLE == LE_PIPE_V || ROLE == LE_TRIO_V || ROLE == LE_QUAD_V, DUO = ROLE != LE_SOLO;  // this wavefront does the position half (inertias, factors, solves, Euler) / the velocity half
	constexpr bool PIPE = le_pipelined_duo(ROLE) || TRIQ;  // bodies pass between wavefronts through the pose ring
	constexpr bool POSE = HALVES || ROLE == LE_PIPE_P || ROLE == LE_TRIO_P, RINGC = ROLE == LE_PIPE_V || ROLE == LE_TRIO_C || ROLE == LE_TRIO_V;  // computes the poses / takes them from the ring (the quartet's roles have a sweep of their own below)
	constexpr bool VLDS = ROLE == LE_TRIO_V;  // V of three wavefronts: cinert from C through LDS (the quartet's V reads it in v_fetch)
	constexpr bool EPOS = ROLE == LE_SOLO || ROLE == LE_DUO_P || ROLE == LE_PIPE_P || ROLE == LE_TRIO_P || ROLE == LE_QUAD_X;                     // gathers mj_energyPos along its pose sweep
	constexpr bool SENSF = ROLE == LE_SOLO || ROLE == LE_DUO_V || ROLE == LE_PIPE_P || ROLE == LE_TRIO_P || ROLE == LE_QUAD_X;  // frame sensors: who holds the poses (and, of two, who has the time)
	[[maybe_unused]] constexpr bool XW = ROLE == LE_QUAD_X;               // X of four wavefronts: the walk's position half, the M factor, the qacc solve, mj_checkAcc
	[[maybe_unused]] constexpr bool DPW = DP || XW;               // runs the position half of the leaf -> root walk
	[[maybe_unused]] constexpr bool FM = ROLE != LE_QUAD_C, FH = !XW;    // factors and solves with M (and so holds qacc) / with M + h B
	[[maybe_unused]] constexpr bool POSEW = ROLE == LE_TRIO_P || ROLE == LE_QUAD_X;  // the pose wavefront of three / four: mj_energyPos is its only result past the sweep
	[[maybe_unused]] constexpr bool OWNCIN = ROLE != LE_TRIO_V;                     // a ring consumer that computes the cinert of the body it takes (the trio's V takes C's, one phase later)
	using Q = Tq<T>;
	static_assert(!PE || ROLE == LE_SOLO, "lane = env kernel: per-env overrides run the solo form");
	static_assert(!HW || (ROLE == LE_SOLO && !PE), "lane = env kernel: the hwsim stage runs the solo form, without per-env overrides");
	static_assert(!XF || (ROLE == LE_SOLO && !HW), "lane = env kernel: xfrc_applied runs the solo form, without the hwsim stage");
	static_assert(NA == 0 || (ROLE == LE_SOLO && !HW), "lane = env kernel: activation states run the solo form, without the hwsim stage");
	static_assert(!le_any_gc<T>() || ROLE == LE_SOLO, "lane = env kernel: gravity compensation runs the solo form");
	using SN = LeSens<T>;
	static_assert(!SN::extra() || ROLE == LE_SOLO, "lane = env kernel: frame-axis, velocity- and acceleration-stage sensors run the solo form");
	using OV = PeSlots<T>;
	using XS6 = XfSlots<T>;
	constexpr int LPE = PIPE ? (1 << 20) : (DUO ? LP - DuoSlots<NV>::n : LP);
	using LD = Lds<T, LPE>;
	using LM = LeLimQ<T>;
	// constraint rows: equality rows first, limit rows behind (NR == 0: the model has no constraint stage, and none of its code) | the dofs they touch
	constexpr int NR = LM::n(), NE = LM::ne(), NL = LM::nl(), NW = LM::nw();
	constexpr bool TEN = [] { for (int i = 0; i < NU; i++) if (LeTen<T>::on(i)) return true; return false; }();  // some actuator drives a fixed tendon
	static_assert((NR == 0 && !TEN) || (ROLE == LE_SOLO && !PE && !HW && !XF), "lane = env kernel: constraint rows and tendon actuators run the plain build of the solo form");
	static_assert(LD::slot(T::NBODY) + LM::slots() <= LPE, "lane = env kernel: state and forces of the topology need more LDS than this instantiation's budget");
	[[maybe_unused]] constexpr int LIM0 = LD::slot(T::NBODY);  // (NR > 0) first pair slot of the packed AR | qacc_warmstart doubles
	// (trio) body b's half-angle (sin, cos) comes from C: a hinge whose two predecessors in the sweep are needed bodies too (C publishes them two barriers ahead)
	constexpr auto SCUSE = [](int b) {
		if (b < 3 || b >= T::NBODY || T::body_jnt[b] < 0) return false;
		if (T::jnt_type[T::body_jnt[b]] != MJB_JNT_HINGE) return false;
		return LD::needed(b) && LD::needed(b - 1) && LD::needed(b - 2);
	};
	constexpr int RINGN = TRIQ ? RING_TRIO : RING_DUO2;  // depth of the pose ring (the trio's V reads two bodies behind P)
	constexpr int LASTB = [] { for (int c = NB - 1; c >= 1; c--) if (LD::needed(c)) return c; return 0; }();  // the leaf the composite-inertia sweep starts at
	constexpr int RING = LD::nslots();  // (PIPE) the pose ring, RINGN x 6 pair slots, behind the solo layout
	constexpr int QR0 = RING + le_ring_slots(RING_TRIO) + DuoSlots<NV>::n + NB, CD0 = QR0 + 8;  // (quartet, behind the trio's layout) O's quaternion ring: 2 x (xquat, the frame before the joint); C's cdof ring: 2 x 3
	[[maybe_unused]] constexpr int XMAIL = CD0 + 6;  // (quartet) X's verdict on the step (mj_checkAcc), a slot nobody else writes: the last of QUARTET_EXTRA
	static_assert(XMAIL + 1 == QR0 + QUARTET_EXTRA, "lane = env kernel: the quartet's slots end where le_quartet_slots() says");
	constexpr int XS = PIPE ? RING + le_ring_slots(RINGN) : LD::nslots(), MAIL = XS + (NV + 1) / 2, SC0 = MAIL + 1;  // (trio) SC0 + b: body b's half-angle (sin, cos), from C to P  // (DUO) pair slots of qfrc_smooth, and of P's verdicts for V
	const int lane_le = DUO ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
	Pair *const lp = reinterpret_cast<Pair *>(smem_le) + lane_le;  // pair slot q of this lane: lp[64 * q]
	// (a tail lane without an env keeps running on the last env's data: no divergent exit, the wave-uniform branches below stay uniform. It stores
	//  nothing of its own -- what it does store, at the launch's end and in the HW stage, is the last env's own value to the last env's address a second time)
	const int env_raw = env_lo + (int)(blockIdx.x * (DUO ? 64u : blockDim.x)) + lane_le;  // (solo: blockDim.x = 64; fewer: a measurement knob, MJB_LANE_ENV_WAVE_LANES)
	const bool live = env_raw < env_hi;
	const int env = live ? env_raw : env_hi - 1;
	const size_t ev = (size_t)env;
	// (NR > 0) double k of this lane's constraint-stage storage: the packed AR triangle (LM::ar), then qacc_warmstart of the rows' dofs (LM::ws)
	[[maybe_unused]] auto lim_ld = [&](auto K) -> double {
		constexpr int k = K;
		if constexpr (k & 1) return lp[64 * (LIM0 + k / 2)].b;
		else return lp[64 * (LIM0 + k / 2)].a;
	};
	[[maybe_unused]] auto lim_st = [&](auto K, const double v) {
		constexpr int k = K;
		if constexpr (k & 1) lp[64 * (LIM0 + k / 2)].b = v;
		else lp[64 * (LIM0 + k / 2)].a = v;
	};

	// ---- the env's state: (qpos, qvel) in LDS, the OU noise state and the activation states (mjData.act, NA > 0) in registers
	double cn[NU > 0 ? NU : 1];
	[[maybe_unused]] double act[NA > 0 ? NA : 1];
	double time;
	bool badp_next = false, badv_next = false;  // mj_checkPos / mj_checkVel verdict on the state the next step starts from
	bool wasreset = false;  // mj_resetData ran inside this launch: ctrl / qfrc_applied read as zero from then on (the frame copy of the generic kernels)
	{
		const DevState MJB_AS4 &s = P->s;
		if constexpr (DP) {
			sfor<NV>([&](auto I) {
				const Pair s2{ s.qpos[ev * NV + I], s.qvel[ev * NV + I] };
				lp[64 * I] = s2;
				badp_next |= bad_val(s2.a);
				badv_next |= bad_val(s2.b);
			});
		}
		sfor<NU>([&](auto I) { cn[I] = DV ? s.ctrlnoise[ev * NU + I] : 0.0; });
		if constexpr (NA > 0) sfor<NA>([&](auto I) { act[I] = s.act[ev * NA + I]; });
		if constexpr (NR > 0) sfor<NW>([&](auto W) { lim_st(IC<LM::ws(W)>{}, s.qacc_warmstart[ev * NV + LM::wdof(W)]); });  // (lives with the lane across the fused steps)
		time = s.time[ev];
		if constexpr (DUO) {  // the load is "Euler of step -1": P's verdicts on the loaded state go to V by mail
			if constexpr (DP) lp[64 * MAIL] = Pair{ (double)((badp_next ? 2 : 0) | (badv_next ? 1 : 0)), 0.0 };
			le_barrier();
			if constexpr (!DP) {
				const int code = (int)lp[64 * MAIL].a;
				badp_next = (code & 2) != 0;
				badv_next = (code & 1) != 0;
			}
		}
	}
	const bool nz_on = P->nz.enabled != 0;
	// ctrl noise from the launch's pre-generated buffer when the host filled one for exactly this launch (mjb_api.hip: launch)
	int zhalf_i = -1;
	if (nz_on && P->s.zbuf != nullptr) {
		const unsigned int *zi = P->s.zinfo;
		if (zi[0] == step0 && (int)zi[1] == nsteps && (int)zi[2] == P->s.nenv) zhalf_i = 0;
		else if (zi[4] == step0 && (int)zi[5] == nsteps && (int)zi[6] == P->s.nenv) zhalf_i = 1;
	}
	const bool zpre = zhalf_i >= 0;

	// ---- (the quartet's O and X) a body at rest -- no joint on its path to the world -- has a pose made of model constants alone: computed ONCE per launch,
	// here, and kept in registers.  O keeps the quaternion its moving children chain from; X the frame its children, the tree root's offset, mj_energyPos and
	// the frame sensors read (what nobody reads is dead code).  The expressions are the sweep's for such a body; neither the retry trip of the attempt loop
	// nor an in-launch mj_resetData changes a rest pose.
	constexpr bool RESTO = ROLE == LE_QUAD_O || ROLE == LE_QUAD_X, RESTX = ROLE == LE_QUAD_X;
	[[maybe_unused]] double rxq[RESTO ? NB : 1][4], rxm[RESTX ? NB : 1][9], rxp[RESTX ? NB : 1][3], rxi[RESTX ? NB : 1][3];
	if constexpr (RESTO) {
		const LeTapeBody MJB_AS4 *const tb0 = reinterpret_cast<const LeTapeBody MJB_AS4 *>(reinterpret_cast<const LeTapeHdr MJB_AS4 *>(P->m.le_tape) + 1);
		sfor<NB>([&](auto Bq) {
			constexpr int b = Bq;
			if constexpr (b > 0 && !LD::needed(b)) {
				constexpr int p = T::body_parentid[b];
				const double MJB_AS4 *const A = reinterpret_cast<const double MJB_AS4 *>(tb0 + b);
				double quat[4] = { A[LE_QUAT], A[LE_QUAT + 1], A[LE_QUAT + 2], A[LE_QUAT + 3] };
				if constexpr (p != 0) le_xquat(quat, rxq[p]);
				normalize4_sel(quat);
				for (int k = 0; k < 4; k++) rxq[b][k] = quat[k];
				if constexpr (RESTX) {
					double pos[3] = { A[LE_POS], A[LE_POS + 1], A[LE_POS + 2] };
					if constexpr (p != 0) le_xipos(pos, rxm[p], rxp[p], pos);
					quat2mat_nocheck(rxm[b], quat);
					for (int k = 0; k < 3; k++) rxp[b][k] = pos[k];
					if constexpr (T::body_sameframe[b]) {
						for (int k = 0; k < 3; k++) rxi[b][k] = rxp[b][k];
					} else {
						const double ip[3] = { A[LE_IPOS], A[LE_IPOS + 1], A[LE_IPOS + 2] };
						le_xipos(rxi[b], rxm[b], rxp[b], ip);
					}
				}
			}
		});
	}

#ifdef MJB_LE_PROBE  // (measurement build: cycle stamps of the step's phases, summed over the launch, into the env-0 sensordata of the role)
	unsigned long long pk_t = 0, pk_acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };  // ([8], the quartet's C and V: from a sweep barrier to where the phase's reads have landed -- V: and the previous body's forces are done)
#define LE_PK0() pk_t = __builtin_readcyclecounter()
#define LE_PK(i) do { const unsigned long long n_ = __builtin_readcyclecounter(); pk_acc[i] += n_ - pk_t; pk_t = n_; } while (0)
#else
#define LE_PK0() do { } while (0)
#define LE_PK(i) do { } while (0)
#endif
#pragma nounroll
	for (int st = 0; st < nsteps; st++) {
		LE_PK0();
		// (the parameter pointer laundered per step: model constants are re-fetched by scalar loads where they are used instead of
		//  being hoisted out of the step loop into ~700 SGPRs the wavefront does not have)
		const KernelParams MJB_AS4 *Pq = P;
		asm volatile("" : "+s"(Pq));
		const DevModel MJB_AS4 &m = Pq->m;
		const DevState MJB_AS4 &s = Pq->s;
		const bool last = st == nsteps - 1;
		// the model's numeric constants: one tape in consumption order (mjb_dev.h), a half record (64 bytes) per scalar load
		const LeTapeHdr MJB_AS4 *th = reinterpret_cast<const LeTapeHdr MJB_AS4 *>(m.le_tape);
		const LeTapeBody MJB_AS4 *tb = reinterpret_cast<const LeTapeBody MJB_AS4 *>(th + 1);
		const double dt = th->dt;

		// ---- H10: the reference's ctrl-noise injector (mujoco_env.cpp:469-481): this step's normals are FETCHED here and folded into
		// the OU state where the forces are assembled, after the root -> leaf sweep -- the trip to HBM hides behind the sweep
		double z[NU > 0 ? NU : 1];
		sfor<NU>([&](auto I) { z[I] = 0; });
		if (DV && nz_on) {
			if (zpre) {
				asm volatile("" ::: "memory");
				const double *zb = s.zbuf + (zhalf_i > 0 ? s.zhalf : 0ull) + ((size_t)st * s.nenv + ev) * NU;
				sfor<NU>([&](auto I) { z[I] = zb[I]; });
			} else {
				asm volatile("" ::: "memory");
				// (one copy of the generator in the instruction stream: the normals go through the cfrc slots, free at this point)
				const unsigned long long seed = Pq->nz.seed, genv = (unsigned long long)(Pq->nz.env_offset + env);
				double *zl = reinterpret_cast<double *>(smem_le) + 2 * 64 * NV + lane_le;
#pragma nounroll
				for (int i = 0; i < NU; i++) zl[64 * i] = philox_normal(seed, genv, step0 + (unsigned int)st, (unsigned int)i);
				sfor<NU>([&](auto I) { z[I] = zl[64 * I]; });
			}
		}
		bool rs = false;  // mj_resetData ran in THIS step (after the injector wrote ctrl: ctrl and the OU state read zero)

		// ---- mj_checkPos / mj_checkVel (qpos first: its reset hides a bad qvel)
		{
			// (the flags were computed where the state was last in registers: at the load, and in the previous step's mj_Euler)
			const bool badp = badp_next, badv = badv_next;
			// (NO per-lane branch anywhere in this kernel: with ~200 live doubles the register allocator spills around every join, and
			//  ROCm 7.2's LLVM places such spills ahead of the exec restore -- the parked lanes lose them, tools/check_spill_exec.py.
			//  A reset is a handful of selects under a wave-uniform test; every lane issues the counter's atomic, with 0 or 1.)
			const bool bad = badp || badv;
			if (__builtin_amdgcn_ballot_w64(bad)) {
				if constexpr (DP) {
					atomicAdd(s.nwarn + MJB_WARN_BADQPOS, (badp && live) ? 1ull : 0ull);
					atomicAdd(s.nwarn + MJB_WARN_BADQVEL, (!badp && badv && live) ? 1ull : 0ull);
					sfor<NV>([&](auto I) {
						const Pair o = lp[64 * I];
						const double oa = pinv(o.a), ob = pinv(o.b), q0 = pins(tb[T::jnt_bodyid[I]].qpos0);  // (evaluated before the selects, not inside them)
						lp[64 * I] = Pair{ bad ? q0 : oa, bad ? 0.0 : ob };
					});
				}
				if constexpr (NA > 0) sfor<NA>([&](auto I) { act[I] = bad ? 0.0 : act[I]; });
				if constexpr (NR > 0) sfor<NW>([&](auto W) { const double w = pinv(lim_ld(IC<LM::ws(W)>{})); lim_st(IC<LM::ws(W)>{}, bad ? 0.0 : w); });  // (mj_resetData: qacc_warmstart = 0)
				time = bad ? 0.0 : time;
				wasreset = wasreset || bad;
				rs = bad;
				if constexpr (DUO) le_barrier();  // (both wavefronts hold the same verdicts: both are here) V reads the reset state
			}
		}

		double qacc[NV], qaccd[NV];  // M^-1 f, and the acceleration Euler advances with: (M + h B)^-1 f under implicit joint damping
		// (NR > 0) what the constraint stage leaves: qfrc_constraint = J' f on the dofs the rows touch, the env's active rows, its PGS sweeps
		[[maybe_unused]] double qfc[NW > 0 ? NW : 1];
		[[maybe_unused]] int c_nefc = 0, c_iter = 0;
		// (NA > 0) the activation states mj_Euler commits: act + h act_dot, clamped to actrange.  Formed where the forces are assembled, on either trip of the
		// loop below from the trip's own act -- a lane mj_checkAcc reset forms it again from zero --, and committed once, behind the loop
		[[maybe_unused]] double actn[NA > 0 ? NA : 1];
		// (HW) mj_checkAcc reset this lane: the retry runs the stage a second time for it and for no other lane | the stage wrote at this step |
		// what it wrote to a POSITION / VELOCITY joint's qpos / qvel (applied in mj_Euler)
		[[maybe_unused]] bool hw_bad = false, hw_wr = false;
		[[maybe_unused]] double hov[NV > 0 ? NV : 1];
		if constexpr (HW) sfor<NV>([&](auto I) { hov[I] = 0; });
		double en_pe = 0, en_ke = 0;
#pragma nounroll
		for (int attempt = 0; attempt < 2; attempt++) {
			// (the tape address laundered per trip: its loads are invariants of this two-trip loop, and the optimiser hoists every one of
			//  them -- ~350 doubles -- in front of it)
			{
				const double MJB_AS4 *tp = m.le_tape;
				asm volatile("" : "+s"(tp));
				th = reinterpret_cast<const LeTapeHdr MJB_AS4 *>(tp);
				tb = reinterpret_cast<const LeTapeBody MJB_AS4 *>(th + 1);
			}
			const LeTapeAct MJB_AS4 *const ta = reinterpret_cast<const LeTapeAct MJB_AS4 *>(tb + NB);
			// (PE) the env's own value of overlay slot sl: base + sl * nenv + env, the address re-derived on every trip like the tape's (a tail lane reads
			//  the last env's column, as `ev` does everywhere else)
			[[maybe_unused]] const char *ovb = nullptr;
			[[maybe_unused]] size_t ovs = 0;
			if constexpr (PE) {
				const double *o = s.le_overlay;
				asm volatile("" : "+s"(o));
				ovb = reinterpret_cast<const char *>(o);
				ovs = (size_t)s.nenv * sizeof(double);
			}
			[[maybe_unused]] const unsigned int ovl = (unsigned int)env * (unsigned int)sizeof(double);
			// (XF) row r of the wrench table, this lane's env: base + r * nenv + env, re-derived on every trip like the overlay's
			[[maybe_unused]] const char *xfb = nullptr;
			[[maybe_unused]] size_t xfs = 0;
			if constexpr (XF) {
				const double *o = s.le_xfrc;
				asm volatile("" : "+s"(o));
				xfb = reinterpret_cast<const char *>(o);
				xfs = (size_t)s.nenv * sizeof(double);
			}
			[[maybe_unused]] auto xf_ld = [&](int row) -> double {
				return *(const double __attribute__((address_space(1))) *)(xfb + (size_t)row * xfs + ovl);
			};
			[[maybe_unused]] auto pe_ld = [&](int sl) -> double {
				return *(const double __attribute__((address_space(1))) *)(ovb + (size_t)sl * ovs + ovl);
			};
			const bool e_on = DP && last && (m.enableflags & MJB_ENBL_ENERGY);
			bool ep_on = e_on;
			if constexpr (EPOS != DP) ep_on = EPOS && last && (m.enableflags & MJB_ENBL_ENERGY);
			const bool eg_on = ep_on && !(m.disableflags & MJB_DSBL_GRAVITY);
			// (sensordata is an output of the LAUNCH: evaluated at its last step -- or, mjb_set_sensors_every_step, at every step as the generic kernels do:
			//  what A15 costs per step on this kernel is a bench line, other_configs.2_sensors_every_step)
			const bool sens_step = last || s.sens_every_step != 0;
			const bool sens_on = DV && sens_step && !(m.disableflags & MJB_DSBL_SENSOR);  // (a tail lane rewrites the last env's values)
			const bool sensf_on = SENSF && sens_step && !(m.disableflags & MJB_DSBL_SENSOR);
			double *sd = s.sensordata + ev * T::NSENSORDATA;
			double pe = 0;

			// ============ one sweep root -> leaf: A1 mj_kinematics, comPos (cinert, cdof), A8 comVel, A9 RNE's forward pass ============
			// Spatial quantities of a tree are taken about the origin of its root body instead of MuJoCo's subtree com (any common point
			// gives the same qM / qfrc_bias; the com would need every body's pose before the first inertia, i.e. a second sweep with
			// 15 doubles per body kept across).
			double xpos[NB][3], xquat[NB][4], xmat[NB][9];
			double cin[NB][10];  // cinert of the bodies that found no room in LDS
			double cdof[NV > 0 ? NV : 1][6];
			double cvel[NB][6], cacc[NB][6];
			double f[NV > 0 ? NV : 1];  // qfrc_passive + qfrc_applied + qfrc_actuator, then (- qfrc_bias) qfrc_smooth
			double grav[3];
			[[maybe_unused]] double rw[SN::acc() ? NB : 1][4];  // (a force / torque sensor on a body at rest) mass * (xipos - the root's origin) | mass of the bodies at rest under it
			{
				const bool g_on = !(m.disableflags & MJB_DSBL_GRAVITY);
				if constexpr (PE) {
					for (int k = 0; k < 3; k++) { const double g = pinv(pe_ld(OV::gravity(k))); grav[k] = g_on ? g : 0.0; }
				} else
				for (int k = 0; k < 3; k++) grav[k] = g_on ? th->gravity[k] : 0.0;
			}
			const bool pas_on = !(m.disableflags & MJB_DSBL_PASSIVE);
			__builtin_amdgcn_sched_barrier(0);
			// (two scheduling regions per body, each fetching the NEXT region's half record at its top: the scalar loads of a region
			//  cannot be hoisted beyond it -- left alone, the compiler issues them bodies ahead and parks ~540 SGPRs in VGPR lanes)
			double hA[NB + 1][16], hB[NB][16];
			[[maybe_unused]] double vB[PE ? NB : 1][7];  // (PE) the env's mass | ibody[6] of a body, fetched with the body's inertial half record
			[[maybe_unused]] double xw[XF ? NB : 1][6];  // (XF) the env's wrench on a moving body, fetched with the body's inertial half record
			// (the quartet's C) what C reads of a needed body's record -- the inertial half up to the mass, as it stands (LE_I_*) | jaxis[3] | jpos[3] --, fetched one phase ahead as O and X
			// fetch theirs: with no scalar load in flight while C works off the pose ring, its waits for the ring's reads are counted ones
			[[maybe_unused]] double hC[ROLE == LE_QUAD_C ? NB + 1 : 1][16];
			constexpr int HC_JAXIS = LE_I_N, HC_JPOS = HC_JAXIS + 3;
			[[maybe_unused]] auto c_fetch = [&](auto Bn) {
				constexpr int nb = Bn, jn = T::body_jnt[nb];
				const double MJB_AS4 *const rec = reinterpret_cast<const double MJB_AS4 *>(tb + nb);
				for (int k = 0; k < LE_I_N; k++) hC[nb][k] = rec[LE_HALF + k];
				if constexpr (jn >= 0) {
					for (int k = 0; k < 3; k++) hC[nb][HC_JAXIS + k] = rec[LE_JAXIS + k];
					if constexpr (T::jnt_type[jn < 0 ? 0 : jn] != MJB_JNT_SLIDE && (!LeOffc<T>::known || LeOffc<T>::on(jn < 0 ? 0 : jn))) for (int k = 0; k < 3; k++) hC[nb][HC_JPOS + k] = rec[LE_JPOS + k];
				}
			};
			// ... pinned at the end of the region that issued the loads (the entries C reads, no others: see touch_rec)
			[[maybe_unused]] auto c_touch = [&](auto Bn) {
				constexpr int nb = Bn, jn = T::body_jnt[nb];
				const double *const h = hC[nb];
				asm volatile("" ::"s"(h[LE_I_IBODY]), "s"(h[LE_I_IBODY + 1]), "s"(h[LE_I_IBODY + 2]), "s"(h[LE_I_IBODY + 3]), "s"(h[LE_I_IBODY + 4]), "s"(h[LE_I_IBODY + 5]), "s"(h[LE_I_MASS]));
				if constexpr (!T::body_sameframe[nb]) asm volatile("" ::"s"(h[LE_I_IPOS]), "s"(h[LE_I_IPOS + 1]), "s"(h[LE_I_IPOS + 2]));
				if constexpr (jn >= 0) {
					asm volatile("" ::"s"(h[HC_JAXIS]), "s"(h[HC_JAXIS + 1]), "s"(h[HC_JAXIS + 2]));
					if constexpr (T::jnt_type[jn < 0 ? 0 : jn] != MJB_JNT_SLIDE && (!LeOffc<T>::known || LeOffc<T>::on(jn < 0 ? 0 : jn))) asm volatile("" ::"s"(h[HC_JPOS]), "s"(h[HC_JPOS + 1]), "s"(h[HC_JPOS + 2]));
				}
			};
			for (int k = 0; k < LE_A_N; k++) hA[1][k] = reinterpret_cast<const double MJB_AS4 *>(tb + 1)[k];
			// ... and the (qpos, qvel) pair of the next jointed body: LDS reads and scalar loads share one counter, so a read issued where
			// it is needed would wait for the record fetched beside it
			double qfa[NV > 0 ? NV : 1];  // qfrc_applied: fetched in the sweep's last region, read by the force block behind it
			Pair pq[NB + 1];
			{
				constexpr int j1 = [] { for (int c = 1; c < NB; c++) if (T::body_jnt[c] >= 0) return T::body_jnt[c]; return -1; }();
				if constexpr (j1 >= 0) pq[T::jnt_bodyid[j1]] = lp[64 * j1];
			}
			// (the trio's P) a hinge's half-angle sine / cosine one body AHEAD: the two polynomial chains depend on qpos alone, so they run beside the
			// previous body's pose chain (quaternion product, normalisation, rsqrt, matrix) and fill its dependency stalls instead of lengthening the
			// critical chain; the body's (qpos, qvel) pair and qpos0 are fetched one more region ahead for that
			[[maybe_unused]] double psn[NB + 2], pcs[NB + 2], q0n[NB + 2];
			[[maybe_unused]] Pair pqn[NB + 2], scq[NB + 2];
			if constexpr (ROLE == LE_TRIO_P && NB > 2) {
				if constexpr (T::body_jnt[2] >= 0) {
					if constexpr (T::jnt_type[T::body_jnt[2]] == MJB_JNT_HINGE) {
						pqn[2] = lp[64 * T::body_jnt[2]];
						q0n[2] = tb[2].qpos0;
					}
				}
			}
			// (frame-axis, velocity- and acceleration-stage sensors) the frame of the object sensor S sits on, from its body's pose: origin relative to the
			// origin of the tree's root body -- the point this kernel takes spatial quantities about -- and rotation matrix (mj_local2Global: the quaternion product)
			[[maybe_unused]] auto sens_frame = [&](auto S, double *dif, double *R) {
				constexpr int i = S, ot = T::sensor_objtype[i], id = T::sensor_objid[i], b = SN::body(i), r = T::body_rootid[b];
				constexpr bool same = ot == MJB_OBJ_XBODY || (ot == MJB_OBJ_SITE ? T::site_sameframe[id] != 0 : T::body_sameframe[b] != 0);
				for (int k = 0; k < 3; k++) dif[k] = r == b ? 0.0 : xpos[b][k] - xpos[r][k];
				if constexpr (!same) {
					double lp3[3], v[3];
					if constexpr (ot == MJB_OBJ_SITE) ldc3(lp3, m.site_pos + 3 * id);
					else { lp3[0] = tb[b].ipos[0]; lp3[1] = tb[b].ipos[1]; lp3[2] = tb[b].ipos[2]; }
					matvec3(v, xmat[b], lp3);
					for (int k = 0; k < 3; k++) dif[k] += v[k];
				}
				if constexpr (ot == MJB_OBJ_XBODY) {
					for (int k = 0; k < 9; k++) R[k] = xmat[b][k];
				} else {
					double lq[4], q[4];
					if constexpr (ot == MJB_OBJ_SITE) ldc4(lq, m.site_quat + 4 * id);
					else ldc4(lq, m.body_iquat + 4 * b);
					qmul(q, xquat[b], lq);
					quat2mat_nocheck(R, q);
				}
			};
			// position-stage sensors on a body's frames (the last step's values are the launch's sensordata)
			auto frame_sensors = [&](auto Bq, const double *xipos) {
				constexpr int b = Bq;
				if (sensf_on) {
					sfor<T::NSENSOR>([&](auto S) {
						constexpr int i = S, type = T::sensor_type[i], ot = T::sensor_objtype[i], id = T::sensor_objid[i], adr = T::sensor_adr[i];
						if constexpr (le_axis_type(type) && SN::body(i) == b) {  // a column of the object's rotation matrix (mjDATATYPE_AXIS: no cutoff)
							double dif[3], R[9];
							sens_frame(S, dif, R);
							constexpr int c = type - MJB_SENS_FRAMEXAXIS;
							for (int k = 0; k < 3; k++) sd[adr + k] = R[3 * k + c];
						}
						if constexpr (type == MJB_SENS_FRAMEPOS || type == MJB_SENS_FRAMEQUAT) {
							constexpr int sb = ot == MJB_OBJ_SITE ? T::site_bodyid[id] : id;
							if constexpr (sb == b) {
								double o3[3], o4[4];
								if constexpr (ot == MJB_OBJ_SITE) {
									if constexpr (type == MJB_SENS_FRAMEPOS) {
										if constexpr (T::site_sameframe[id]) {
											for (int k = 0; k < 3; k++) o3[k] = xpos[b][k];
										} else {
											double sp[3], v[3];
											ldc3(sp, m.site_pos + 3 * id);
											matvec3(v, xmat[b], sp);
											for (int k = 0; k < 3; k++) o3[k] = v[k] + xpos[b][k];
										}
									} else {
										double sq[4];
										ldc4(sq, m.site_quat + 4 * id);
										qmul(o4, xquat[b], sq);
									}
								} else if constexpr (ot == MJB_OBJ_BODY) {
									if constexpr (type == MJB_SENS_FRAMEPOS) {
										for (int k = 0; k < 3; k++) o3[k] = xipos[k];
									} else {
										double iq[4];
										ldc4(iq, m.body_iquat + 4 * b);
										qmul(o4, xquat[b], iq);
									}
								} else {  // xbody
									for (int k = 0; k < 3; k++) o3[k] = xpos[b][k];
									for (int k = 0; k < 4; k++) o4[k] = xquat[b][k];
								}
								if constexpr (type == MJB_SENS_FRAMEPOS) {
									const double cut = m.sensor_cutoff[i];
									for (int k = 0; k < 3; k++) sd[adr + k] = cut > 0 ? clampd(o3[k], -cut, cut) : o3[k];
								} else {
									for (int k = 0; k < 4; k++) sd[adr + k] = o4[k];
								}
							}
						}
					});
				}
			};
			// velocity-stage sensors on a body (mj_objectVelocity): cvel, taken about the tree root's origin, moved to the object -- the lever arm is the object's
			// position relative to that origin, the result does not depend on the point -- in the object's frame (velocimeter, gyro) or the world's (framelinvel,
			// frameangvel without a reference frame).  A body at rest reads zero.
			[[maybe_unused]] auto vel_sensors = [&](auto Bq) {
				constexpr int b = Bq;
				if (sensf_on) {
					sfor<T::NSENSOR>([&](auto S) {
						constexpr int i = S, type = T::sensor_type[i], adr = T::sensor_adr[i];
						if constexpr (le_vel_type(type) && SN::body(i) == b) {
							double out[3] = { 0, 0, 0 };
							if constexpr (LD::needed(b)) {
								double dif[3], R[9], cr[3], w[3];
								sens_frame(S, dif, R);
								cross3(cr, dif, cvel[b]);
								constexpr bool ang = type == MJB_SENS_GYRO || type == MJB_SENS_FRAMEANGVEL;
								for (int k = 0; k < 3; k++) w[k] = ang ? cvel[b][k] : cvel[b][3 + k] - cr[k];
								if constexpr (type == MJB_SENS_GYRO || type == MJB_SENS_VELOCIMETER) matTvec3(out, R, w);
								else for (int k = 0; k < 3; k++) out[k] = w[k];
							}
							const double cut = m.sensor_cutoff[i];
							for (int k = 0; k < 3; k++) sd[adr + k] = cut > 0 ? clampd(out[k], -cut, cut) : out[k];
						}
					});
				}
			};
			// (ring consumers) one body off the ring: its pose (position relative to the tree root's origin), cinert, cdof; V: velocities and the body's force
			auto consume = [&](auto Bq) {
				constexpr int b = Bq;
				constexpr int p = T::body_parentid[b], j = T::body_jnt[b];
				constexpr int ord = (LD::slot(b) - NV) / 3, rg = RING + 6 * (ord % RINGN), c0 = LD::cin_slot(b);
				static_assert(c0 >= 0, "pipelined forms: every needed body's cinert lives in LDS");
				static_assert(ROLE != LE_QUAD_V || b < 0, "the quartet's V takes a body in pieces: v_fetch, v_kin, v_force");
				[[maybe_unused]] double xp[3], xm[9];
				double ci[10];
				le_ring_get<ROLE == LE_QUAD_C>(xp, xm, lp + 64 * rg);
				if constexpr ((ROLE == LE_PIPE_V && b == LASTB) || VLDS) {
					// the LAST needed body's cinert came with its pose: P computes that one itself and goes from its last pose straight into the
					// composite-inertia sweep, which starts at this body -- it never waits for V's last phase
					le_pairs_get<5>(ci, lp + 64 * c0);
				} else
				{
					// cinert about the tree root's origin; handed to P's composite-inertia sweep
					const LeTapeBody MJB_AS4 &tj = tb[b];
					constexpr bool CREC = ROLE == LE_QUAD_C;  // (the quartet's C: the record is in hC[b], fetched a phase ago)
					[[maybe_unused]] const double *const hc = hC[CREC ? b : 0];
					double dif[3] = { xp[0], xp[1], xp[2] };
					if constexpr (!T::body_sameframe[b]) {
						double ip[3];
						if constexpr (CREC) { ip[0] = hc[LE_I_IPOS]; ip[1] = hc[LE_I_IPOS + 1]; ip[2] = hc[LE_I_IPOS + 2]; }
						else { ip[0] = tj.ipos[0]; ip[1] = tj.ipos[1]; ip[2] = tj.ipos[2]; }
						double v[3];
						matvec3(v, xm, ip);
						for (int k = 0; k < 3; k++) dif[k] += v[k];
					}
					double mass, ib[6];
					if constexpr (CREC) { mass = hc[LE_I_MASS]; for (int k = 0; k < 6; k++) ib[k] = hc[LE_I_IBODY + k]; }
					else { mass = tj.mass; for (int k = 0; k < 6; k++) ib[k] = tj.ibody[k]; }
					double Tm[9];
					le_inert_rot(Tm, xm, ib[0], ib[1], ib[2], ib[3], ib[4], ib[5]);
					if constexpr (CREC) {
						// (every read of the ring has landed: the next needed body's record is fetched from here on, under the rest of cinert and the cdof
						//  half -- the compiler may not lift its loads into the counted waits above)
						constexpr int nx = [] { for (int q = b + 1; q < T::NBODY; q++) if (LD::needed(q)) return q; return T::NBODY; }();
						touch_v(dif[0]);
						touch_v(dif[1]);
						touch_v(dif[2]);
						LE_PK(8);
						__builtin_amdgcn_sched_barrier(0);
						if constexpr (nx < NB) c_fetch(IC<nx>{});
					}
					le_cinert_com(ci, Tm, xm, mass, dif);
					if constexpr (OWNCIN) le_pairs_put<5>(lp + 64 * c0, ci);  // (for the composite-inertia sweep of P / of C itself)
				}
				constexpr bool prest = p == 0 || !LD::needed(p);  // the world, or a jointless chain down from it: at rest
				[[maybe_unused]] double pv[6], pa[6];
				if constexpr (!DV) {
				} else if constexpr (prest) le_parent_motion(pv, pa, grav);
				else le_parent_motion(pv, pa, cvel[p], cacc[p]);
				if constexpr (j >= 0) {
					[[maybe_unused]] double qv = 0;
					if constexpr (DV) qv = lp[64 * j].b;
					double *cd = cdof[j];
					constexpr int cq = CD0 + 3 * (ord % 2);  // (quartet) the body's slots of the cdof ring
					{
					const LeTapeBody MJB_AS4 &tj = tb[b];
					constexpr bool CREC = ROLE == LE_QUAD_C;
					[[maybe_unused]] const double *const hc = hC[CREC ? b : 0];
					double ax[3];
					if constexpr (CREC) { ax[0] = hc[HC_JAXIS]; ax[1] = hc[HC_JAXIS + 1]; ax[2] = hc[HC_JAXIS + 2]; }
					else { ax[0] = tj.jaxis[0]; ax[1] = tj.jaxis[1]; ax[2] = tj.jaxis[2]; }
					double xaxis[3];
					matvec3(xaxis, xm, ax);
					if constexpr (T::jnt_type[j] == MJB_JNT_SLIDE) le_cdof_slide(cd, xaxis);
					else {
						// (the anchor from the body's FINAL frame: xpos + xmat jnt_pos -- the point mj_kinematics' off-centre correction keeps fixed)
						double jp[3] = { 0, 0, 0 };
						if constexpr (!CREC) { jp[0] = tj.jpos[0]; jp[1] = tj.jpos[1]; jp[2] = tj.jpos[2]; }
						else if constexpr (!LeOffc<T>::known || LeOffc<T>::on(j)) { jp[0] = hc[HC_JPOS]; jp[1] = hc[HC_JPOS + 1]; jp[2] = hc[HC_JPOS + 2]; }
						double xanch[3] = { xp[0], xp[1], xp[2] }, off[3];
						if (le_offc<T, QUAD, j>(jp[0], jp[1], jp[2])) le_xipos(xanch, xm, xanch, jp);
						for (int k = 0; k < 3; k++) off[k] = -xanch[k];  // (root origin - anchor)
						le_cdof_hinge(cd, xaxis, off);
					}
					if constexpr (ROLE == LE_QUAD_C) le_pairs_put<3>(lp + 64 * cq, cd);  // (the quartet's C: cdof to V)
					}
					if constexpr (DV) le_body_motion<prest>(cvel[b], cacc[b], pv, pa, cd, qv);
				} else if constexpr (DV) {
					for (int k = 0; k < 6; k++) { cvel[b][k] = pv[k]; cacc[b][k] = pa[k]; }
				}
				if constexpr (DV) {
					double cf[6], t1[6];
					le_cfrc(cf, t1, ci, cvel[b], cacc[b]);
					constexpr int q0 = LD::slot(b);
					lp[64 * q0] = Pair{ cf[0] + t1[0], cf[1] + t1[1] };
					lp[64 * (q0 + 1)] = Pair{ cf[2] + t1[2], cf[3] + t1[3] };
					lp[64 * (q0 + 2)] = Pair{ cf[4] + t1[4], cf[5] + t1[5] };
				}
			};
			// (HW) the env's commands, PID state and cadence record: fetched in the sweep's last region, read by the force block behind it
			[[maybe_unused]] double hcmd[NV > 0 ? NV : 1], hpi[NV > 0 ? NV : 1], hpl[NV > 0 ? NV : 1], hjp[NV > 0 ? NV : 1], hjv[NV > 0 ? NV : 1], hlu = 0, hlw = 0;
			[[maybe_unused]] auto hw_fetch = [&]() __attribute__((always_inline)) {
				// (every pointer taken from the parameter block where it is used: a local copy captured by the dof loop's closure keeps that closure in scratch)
				if (Pq->hw.period_ns > 0) {
					const double *const cad = Pq->hw.cad + ev * (size_t)(2 + 2 * Pq->hw.n);
					hlu = cad[0];
					hlw = cad[1];
				}
				sfor<NV>([&](auto I) __attribute__((always_inline)) {
					hcmd[I] = hpi[I] = hpl[I] = hjp[I] = hjv[I] = 0;
					const HwSim MJB_AS4 &hw = Pq->hw;
					const int k = hw.le_tab[4 * I];
					if (k >= 0) {
						const int method = hw.le_tab[4 * I + 1], hn = hw.n;
						const size_t at = ev * (size_t)hn + (size_t)k;
						if (method == MJB_HW_EFFORT) hcmd[I] = hw.cmd_eff[at];
						else if (method == MJB_HW_VELOCITY || method == MJB_HW_VELOCITY_PID) hcmd[I] = hw.cmd_vel[at];
						else if (hw.estop != 0) hcmd[I] = hw.cmd_hold[at];
						else hcmd[I] = hw.cmd_pos[at];
						if (method == MJB_HW_POSITION_PID || method == MJB_HW_VELOCITY_PID) {
							hpi[I] = hw.pid[2 * at];
							hpl[I] = hw.pid[2 * at + 1];
						}
						if (hw.period_ns > 0) {
							const double *const cad = hw.cad + ev * (size_t)(2 + 2 * hn);
							hjp[I] = cad[2 + k];
							hjv[I] = cad[2 + hn + k];
						}
					}
				});
			};
			sfor<NB>([&](auto B) {
				constexpr int b = B;
				if constexpr (b > 0 && RINGC) {
					// ---- the pipelined V (and the trio's C): body b's pose and cinert come through LDS, one barrier per needed body.  The trio's V runs TWO bodies
					// behind P: it takes the cinert C computed one phase earlier instead of computing its own, and never paces the pose chain
					if constexpr (LD::needed(b)) {
						if constexpr (ROLE == LE_TRIO_C) {
							// (the trio's C) a hinge's half-angle sine and cosine are a third of the pose chain's instructions and depend on qpos alone: C computes them
							// two bodies ahead of P, in the time it would wait at this barrier, and P picks them up from LDS
							constexpr int t2 = [] {
								int c = b, hops = 0;
								for (int q = b + 1; q < NB && hops < 2; q++) if (LD::needed(q)) { c = q; hops++; }
								return hops == 2 ? c : 0;
							}();
							if constexpr (t2 > 0 && SCUSE(t2)) {
								double sn, cs;
								const double qp2 = lp[64 * T::body_jnt[t2]].a;
								sincos_nb((qp2 - tb[t2].qpos0) * 0.5, &sn, &cs);
								lp[64 * (SC0 + t2)] = Pair{ sn, cs };
							}
						}
						LE_PK(0);
						le_barrier();
						LE_PK(2);
						if constexpr (OWNCIN) consume(IC<b>{});
						else {
							constexpr int pb = [] { for (int c = b - 1; c >= 1; c--) if (LD::needed(c)) return c; return 0; }();
							if constexpr (pb > 0) consume(IC<pb>{});
						}
					}
					if constexpr (DV && b == 1) sfor<NV>([&](auto I) { qfa[I] = s.qfrc_applied[ev * NV + I]; });  // (read by the force block behind the sweep: a trip to HBM)
					__builtin_amdgcn_sched_barrier(0);
				}
				if constexpr (b > 0 && POSE) {
				constexpr int p = T::body_parentid[b], j = T::body_jnt[b], r = T::body_rootid[b];
				touch_s(hA[b][0]);
				if constexpr (j >= 0) touch_v(pq[b].a);
				for (int k = 0; k < LE_I_N; k++) hB[b][k] = reinterpret_cast<const double MJB_AS4 *>(tb + b)[LE_HALF + k];
				if constexpr (PE) {
					if constexpr (OV::moving(b)) for (int k = 0; k < 7; k++) vB[b][k] = pe_ld(OV::inert(b, k));
					else vB[b][0] = pe_ld(OV::rest(b));
				}
				if constexpr (XF && LD::needed(b)) for (int k = 0; k < 6; k++) xw[b][k] = xf_ld(6 * XS6::slot(b) + k);
				const double *const A = hA[b];  // the pose half (LE_POS .. LE_QPOS0)
				if constexpr (ROLE == LE_TRIO_P && b == 1 && b + 1 < NB) {
					if constexpr (T::body_jnt[b + 1] >= 0) {
						if constexpr (T::jnt_type[T::body_jnt[b + 1]] == MJB_JNT_HINGE) sincos_nb((pqn[b + 1].a - q0n[b + 1]) * 0.5, &psn[b + 1], &pcs[b + 1]);
					}
				}
				double pos[3] = { A[LE_POS], A[LE_POS + 1], A[LE_POS + 2] }, quat[4] = { A[LE_QUAT], A[LE_QUAT + 1], A[LE_QUAT + 2], A[LE_QUAT + 3] };
				if constexpr (p != 0) {
					double v[3], q[4];
					matvec3(v, xmat[p], pos);
					for (int k = 0; k < 3; k++) pos[k] = v[k] + xpos[p][k];
					qmul(q, xquat[p], quat);
					for (int k = 0; k < 4; k++) quat[k] = q[k];
				}
				[[maybe_unused]] double xaxis[3], xanch[3], qp = 0, qv = 0;
				[[maybe_unused]] bool offc = false;
				if constexpr (j >= 0) {
					qp = pq[b].a;
					qv = pq[b].b;
					// The joint's world axis is its local axis through the body's FINAL orientation (a hinge turns about it, a slide does not
					// turn), and a hinge's anchor stays where it was: the frame before the joint motion -- mj_kinematics' xaxis / xanchor
					// source -- is only needed for an off-centre anchor (jnt_pos != 0, wave-uniform).
					const double jp[3] = { A[LE_JPOS], A[LE_JPOS + 1], A[LE_JPOS + 2] };
					offc = jp[0] != 0 || jp[1] != 0 || jp[2] != 0;
					for (int k = 0; k < 3; k++) xanch[k] = pos[k];
					if (offc) {
						double M0[9], v[3];
						quat2mat_nocheck(M0, quat);
						matvec3(v, M0, jp);
						for (int k = 0; k < 3; k++) xanch[k] += v[k];
					}
					if constexpr (T::jnt_type[j] == MJB_JNT_HINGE) {
						double sn, cs, ql[4], q[4];
						if constexpr (ROLE == LE_TRIO_P && SCUSE(b)) { sn = scq[b].a; cs = scq[b].b; }  // (C's, fetched in the previous body's second region)
						else if constexpr (ROLE == LE_TRIO_P && b == 2) { sn = psn[b]; cs = pcs[b]; }  // (computed beside the first body's chain)
						else sincos_nb((qp - A[LE_QPOS0]) * 0.5, &sn, &cs);
						ql[0] = cs; ql[1] = A[LE_JAXIS] * sn; ql[2] = A[LE_JAXIS + 1] * sn; ql[3] = A[LE_JAXIS + 2] * sn;
						qmul(q, quat, ql);
						for (int k = 0; k < 4; k++) quat[k] = q[k];
					}
					if (ep_on && pas_on) {  // mj_energyPos: the joint spring
						const double dqs = qp - tb[b].spring;  // (last step only)
						if constexpr (PE) pe += 0.5 * pe_ld(OV::joint(b, 0)) * dqs * dqs;
						else
						pe += 0.5 * tb[b].stiffness * dqs * dqs;
					}
				}
				normalize4_sel(quat);
				for (int k = 0; k < 4; k++) xquat[b][k] = quat[k];
				quat2mat_nocheck(xmat[b], quat);
				if constexpr (j >= 0) {
					const double ax[3] = { A[LE_JAXIS], A[LE_JAXIS + 1], A[LE_JAXIS + 2] };
					matvec3(xaxis, xmat[b], ax);
					if constexpr (T::jnt_type[j] == MJB_JNT_SLIDE) {
						const double dq = qp - A[LE_QPOS0];
						for (int k = 0; k < 3; k++) pos[k] += xaxis[k] * dq;
					} else if (offc) {  // correct for off-centre rotation
						const double jp[3] = { A[LE_JPOS], A[LE_JPOS + 1], A[LE_JPOS + 2] };
						double v[3];
						matvec3(v, xmat[b], jp);
						for (int k = 0; k < 3; k++) pos[k] = xanch[k] - v[k];
					}
				}
				for (int k = 0; k < 3; k++) xpos[b][k] = pos[k];
				touch_rec<LE_I_N>(hB[b]);
				__builtin_amdgcn_sched_barrier(0);
				// ---- second region: inertial frame, cinert, velocities, forces; the next body's pose half on its way
				touch_s(hB[b][0]);
				if constexpr (b + 1 < NB) for (int k = 0; k < LE_A_N; k++) hA[b + 1][k] = reinterpret_cast<const double MJB_AS4 *>(tb + b + 1)[k];
				{
					constexpr int nb = [] { for (int c = b + 1; c < NB; c++) if (T::body_jnt[c] >= 0) return c; return -1; }();
					if constexpr (nb >= 0) pq[nb] = lp[64 * T::body_jnt[nb]];
				}
				if constexpr (ROLE == LE_TRIO_P && SCUSE(b + 1)) scq[b + 1] = lp[64 * (SC0 + b + 1)];
				const double *const Bh = hB[b];  // the inertial half (LE_I_IPOS .. LE_I_MASS)
				// inertial frame
				double xipos[3];
				if constexpr (T::body_sameframe[b]) {
					for (int k = 0; k < 3; k++) xipos[k] = xpos[b][k];
				} else {
					double ip[3] = { Bh[LE_I_IPOS], Bh[LE_I_IPOS + 1], Bh[LE_I_IPOS + 2] }, v[3];
					matvec3(v, xmat[b], ip);
					for (int k = 0; k < 3; k++) xipos[k] = v[k] + xpos[b][k];
				}
				const double mass = [&] { if constexpr (PE) return vB[b][0]; else return Bh[LE_I_MASS]; }();
				if (eg_on) pe -= mass * (grav[0] * xipos[0] + grav[1] * xipos[1] + grav[2] * xipos[2]);
				frame_sensors(B, xipos);
				if constexpr (LD::needed(b)) {
					// cinert about the tree root's origin (mju_inertCom with that offset)
					[[maybe_unused]] double ci[10];
					if constexpr (HALVES || (ROLE == LE_PIPE_P && b == LASTB)) {
						double dif[3];
						if constexpr (r == b) { dif[0] = xipos[0] - pos[0]; dif[1] = xipos[1] - pos[1]; dif[2] = xipos[2] - pos[2]; }
						else for (int k = 0; k < 3; k++) dif[k] = xipos[k] - xpos[r][k];
						// world inertia X Ib X' with the body-frame inertia matrix Ib = R(iquat) diag(inertia) R(iquat)' from the tape
						// (mju_inertCom builds the same matrix as ximat diag ximat', ximat = X R(iquat))
						const double *X = xmat[b];
						const double *const Ib = [&] { if constexpr (PE) return vB[b] + 1; else return Bh + LE_I_IBODY; }();
						const double ixx = Ib[0], iyy = Ib[1], izz = Ib[2], ixy = Ib[3], ixz = Ib[4], iyz = Ib[5];
						double Tm[9];
						for (int rr = 0; rr < 3; rr++) {
							Tm[3 * rr + 0] = X[3 * rr] * ixx + X[3 * rr + 1] * ixy + X[3 * rr + 2] * ixz;
							Tm[3 * rr + 1] = X[3 * rr] * ixy + X[3 * rr + 1] * iyy + X[3 * rr + 2] * iyz;
							Tm[3 * rr + 2] = X[3 * rr] * ixz + X[3 * rr + 1] * iyz + X[3 * rr + 2] * izz;
						}
						double *res = ci;
						res[0] = Tm[0] * X[0] + Tm[1] * X[1] + Tm[2] * X[2] + mass * (dif[1] * dif[1] + dif[2] * dif[2]);
						res[1] = Tm[3] * X[3] + Tm[4] * X[4] + Tm[5] * X[5] + mass * (dif[0] * dif[0] + dif[2] * dif[2]);
						res[2] = Tm[6] * X[6] + Tm[7] * X[7] + Tm[8] * X[8] + mass * (dif[0] * dif[0] + dif[1] * dif[1]);
						res[3] = Tm[0] * X[3] + Tm[1] * X[4] + Tm[2] * X[5] - mass * dif[0] * dif[1];
						res[4] = Tm[0] * X[6] + Tm[1] * X[7] + Tm[2] * X[8] - mass * dif[0] * dif[2];
						res[5] = Tm[3] * X[6] + Tm[4] * X[7] + Tm[5] * X[8] - mass * dif[1] * dif[2];
						res[6] = mass * dif[0];
						res[7] = mass * dif[1];
						res[8] = mass * dif[2];
						res[9] = mass;
					}
					// parent's velocity / acceleration (the world, or a jointless chain down from it: at rest)
					[[maybe_unused]] double pv[6], pa[6];
					if constexpr (!DV) {
					} else if constexpr (p == 0 || !LD::needed(p)) {
						for (int k = 0; k < 6; k++) pv[k] = 0;
						pa[0] = pa[1] = pa[2] = 0;
						for (int k = 0; k < 3; k++) pa[3 + k] = -grav[k];
					} else {
						for (int k = 0; k < 6; k++) { pv[k] = cvel[p][k]; pa[k] = cacc[p][k]; }
					}
					if constexpr (ROLE == LE_TRIO_P) {  // (the trio's P: poses only)
					} else if constexpr (j >= 0) {
						double *cd = cdof[j];
						if constexpr (T::jnt_type[j] == MJB_JNT_SLIDE) {
							cd[0] = cd[1] = cd[2] = 0;
							for (int k = 0; k < 3; k++) cd[3 + k] = xaxis[k];
						} else {
							double off[3];
							if constexpr (r == b) for (int k = 0; k < 3; k++) off[k] = pos[k] - xanch[k];
							else for (int k = 0; k < 3; k++) off[k] = xpos[r][k] - xanch[k];
							for (int k = 0; k < 3; k++) cd[k] = xaxis[k];
							cross3(cd + 3, xaxis, off);
						}
						if constexpr (!DV) {
						} else if constexpr (p == 0 || !LD::needed(p)) {
							// cdof_dot = cvel(parent) x cdof = 0
							for (int k = 0; k < 6; k++) { cvel[b][k] = cd[k] * qv; cacc[b][k] = pa[k]; }
						} else {
							double cdd[6];
							cross_motion(cdd, pv, cd);
							for (int k = 0; k < 6; k++) { cvel[b][k] = pv[k] + cd[k] * qv; cacc[b][k] = pa[k] + cdd[k] * qv; }
						}
					} else if constexpr (DV) {
						for (int k = 0; k < 6; k++) { cvel[b][k] = pv[k]; cacc[b][k] = pa[k]; }
					}
					if constexpr (SN::vel()) vel_sensors(B);
					if constexpr (DP && (ROLE != LE_PIPE_P || b == LASTB)) {  // the composite-inertia sweep reads it back (pipelined duo: the last body's, which V's force computation reads too)
						if constexpr (LD::cin_slot(b) >= 0) {
							constexpr int c0 = LD::cin_slot(b);
							for (int k = 0; k < 5; k++) lp[64 * (c0 + k)] = Pair{ ci[2 * k], ci[2 * k + 1] };
						} else {
							for (int k = 0; k < 10; k++) cin[b][k] = ci[k];
						}
					}
					if constexpr (DV) {
						// cfrc_body = cinert * cacc + cvel x* (cinert * cvel): parked in LDS for the backward sweep
						double cf[6], t0[6], t1[6];
						mul_inert_vec(cf, ci, cacc[b]);
						mul_inert_vec(t0, ci, cvel[b]);
						cross_force(t1, cvel[b], t0);
						if constexpr (XF) {
							// mj_xfrcAccumulate: the body's wrench at xipos as a spatial force about the tree root's origin, off the body's own force
							double xd[3], w[6], tq[3];
							if constexpr (r == b) for (int k = 0; k < 3; k++) xd[k] = xipos[k] - pos[k];
							else for (int k = 0; k < 3; k++) xd[k] = xipos[k] - xpos[r][k];
							for (int k = 0; k < 6; k++) { const double v = pinv(xw[b][k]); w[k] = seld(wasreset, 0.0, v); }  // (zero after mj_resetData; load first, then select)
							cross3(tq, xd, w);
							for (int k = 0; k < 3; k++) { cf[k] -= w[3 + k] + tq[k]; cf[3 + k] -= w[k]; }
						}
						if constexpr (LeGc<T>::on(b)) {
							// mj_passive, body_gravcomp: -gravity * mass * gravcomp at xipos, folded as the wrench above (no torque)
							double xd[3], F[3], tq[3];
							if constexpr (r == b) for (int k = 0; k < 3; k++) xd[k] = xipos[k] - pos[k];
							else for (int k = 0; k < 3; k++) xd[k] = xipos[k] - xpos[r][k];
							const double sc = pas_on ? -mass * tb[b].gravcomp : 0.0;
							for (int k = 0; k < 3; k++) F[k] = sc * grav[k];
							cross3(tq, xd, F);
							for (int k = 0; k < 3; k++) { cf[k] -= tq[k]; cf[3 + k] -= F[k]; }
						}
						constexpr int q0 = LD::slot(b);
						lp[64 * q0] = Pair{ cf[0] + t1[0], cf[1] + t1[1] };
						lp[64 * (q0 + 1)] = Pair{ cf[2] + t1[2], cf[3] + t1[3] };
						lp[64 * (q0 + 2)] = Pair{ cf[4] + t1[4], cf[5] + t1[5] };
					}
					if constexpr (ROLE == LE_PIPE_P || ROLE == LE_TRIO_P) {  // the pose to V (and, of three, to C)
						constexpr int ord = (LD::slot(b) - NV) / 3, rg = RING + 6 * (ord % RINGN);
						double xp[3] = { 0, 0, 0 };  // relative to the tree root's origin: what cdof is taken about
						if constexpr (r != b) for (int k = 0; k < 3; k++) xp[k] = xpos[b][k] - xpos[r][k];
						le_ring_put(lp + 64 * rg, xp, xmat[b]);
						LE_PK(0);
						le_barrier();
						LE_PK(2);
					}
				} else {  // a body at rest: swept for its pose alone.  Its velocity sensors read zero; a force / torque sensor above it takes its weight
					if constexpr (SN::vel()) vel_sensors(B);
					if constexpr (SN::below(b, le_wrench_type)) {
						for (int k = 0; k < 3; k++) rw[b][k] = mass * (xipos[k] - xpos[r][k]);  // (r is at rest too: b == r reads its own xpos)
						rw[b][3] = mass;
					}
				}
				if constexpr (b + 1 < NB) touch_rec<LE_A_N>(hA[b + 1]);
				if constexpr (DV && b == NB - 1) sfor<NV>([&](auto I) { qfa[I] = s.qfrc_applied[ev * NV + I]; });
				if constexpr (HW && b == NB - 1) hw_fetch();
				__builtin_amdgcn_sched_barrier(0);
				}
			});


			// ============ the quartet's sweep: the same quantities, dealt over four wavefronts in phases (see the roles at the top) ============
			// A body without a joint on its path to the world never moves and nobody downstream takes anything of it through LDS: O (its quaternion) and
			// X (its frame, sensors, energy) each compute those bodies for themselves ahead of the step loop, once per launch; the phases count the NEEDED bodies only.
			if constexpr (QUAD) {
				constexpr auto HINGE = [](int c) {
					if (c < 1 || c >= T::NBODY || T::body_jnt[c < T::NBODY ? (c < 0 ? 0 : c) : 0] < 0) return false;
					return T::jnt_type[T::body_jnt[c]] == MJB_JNT_HINGE;
				};
				constexpr auto NEXTN = [](int c) { for (int q = c + 1; q < T::NBODY; q++) if (LD::needed(q)) return q; return T::NBODY; };  // the needed body after c (NBODY: none)
				constexpr auto NTH = [](int k) { int c = 0; for (int i = 0; i < k && c < T::NBODY; i++) { c++; while (c < T::NBODY && !LD::needed(c)) c++; } return k < 1 ? T::NBODY : c; };
				constexpr int KN = [] { int n = 0; for (int c = 1; c < T::NBODY; c++) if (LD::needed(c)) n++; return n; }();
				constexpr int N1 = NEXTN(0), N2 = NEXTN(N1 < NB ? N1 : NB - 1);
				[[maybe_unused]] double osn[NB + 1], ocs[NB + 1], oq0[NB + 1];  // O: a hinge's half-angle (sin, cos), computed one phase ahead; its qpos0 and (qpos, qvel), fetched two ahead
				[[maybe_unused]] Pair opq[NB + 1];
				// O, body b: the orientation chain (hA[b] is there)
				auto o_body = [&](auto Bq) {
					constexpr int b = Bq;
					constexpr int p = T::body_parentid[b], j = T::body_jnt[b];
					static_assert(LD::needed(b), "the quartet: a body at rest has its quaternion from ahead of the step loop");
					const double *const A = hA[b];  // the pose half
					constexpr int qr = QR0 + 4 * (((LD::slot(b) - NV) / 3) % 2);
					double quat[4] = { A[LE_QUAT], A[LE_QUAT + 1], A[LE_QUAT + 2], A[LE_QUAT + 3] };
					if constexpr (p != 0) le_xquat(quat, xquat[p]);
					if constexpr (j >= 0) {
						// (an off-centre anchor -- the topology's flag, or wave-uniform: X needs the frame before the joint motion too)
						if (le_offc<T, true, j>(A[LE_JPOS], A[LE_JPOS + 1], A[LE_JPOS + 2])) le_pairs_put<2>(lp + 64 * (qr + 2), quat);
						if constexpr (T::jnt_type[j] == MJB_JNT_HINGE) le_hinge_quat(quat, A + LE_JAXIS, osn[b], ocs[b]);
					}
					normalize4_sel(quat);
					for (int k = 0; k < 4; k++) xquat[b][k] = quat[k];
					if constexpr (LD::needed(b)) le_pairs_put<2>(lp + 64 * qr, quat);
				};
				auto o_phase = [&](auto Bq) {
					constexpr int b = Bq, nx = NEXTN(b), nx2 = NEXTN(nx < NB ? nx : NB - 1);
					touch_s(hA[b][0]);
					if constexpr (nx < NB) for (int k = 0; k < LE_A_N; k++) hA[nx][k] = reinterpret_cast<const double MJB_AS4 *>(tb + nx)[k];
					if constexpr (nx < NB && HINGE(nx2)) {
						opq[nx2] = lp[64 * T::body_jnt[nx2 < NB ? nx2 : 0]];
						oq0[nx2] = tb[nx2].qpos0;
					}
					// (the next hinge's two polynomial chains depend on qpos alone: they fill this body's dependency stalls)
					if constexpr (HINGE(nx)) sincos_nb((opq[nx].a - oq0[nx]) * 0.5, &osn[nx], &ocs[nx]);
					o_body(Bq);
					if constexpr (nx < NB) touch_rec<LE_A_N>(hA[nx]);
				};
				// X, body b: O's quaternion into the frame, the position chain, what hangs on the pose (hA[b], hB[b] are there)
				auto x_body = [&](auto Bq) {
					constexpr int b = Bq;
					constexpr int p = T::body_parentid[b], j = T::body_jnt[b], r = T::body_rootid[b];
					constexpr int qr = QR0 + 4 * (((LD::slot(b) - NV) / 3) % 2);
					const double *const A = hA[b];
					double pos[3] = { A[LE_POS], A[LE_POS + 1], A[LE_POS + 2] }, quat[4];
					static_assert(LD::needed(b), "the quartet: a body at rest has its pose from ahead of the step loop");
					le_pairs_get<2>(quat, lp + 64 * qr);
					[[maybe_unused]] Pair sp{ 0, 0 };
					if constexpr (j >= 0) sp = lp[64 * j];
					if constexpr (p != 0) le_xipos(pos, xmat[p], xpos[p], pos);
					[[maybe_unused]] double xanch[3], qp = 0;
					[[maybe_unused]] bool offc = false;
					if constexpr (j >= 0) {
						qp = sp.a;
						const double *const jp = A + LE_JPOS;
						offc = le_offc<T, true, j>(jp[0], jp[1], jp[2]);
						for (int k = 0; k < 3; k++) xanch[k] = pos[k];
						if (offc) {
							double q0[4];
							le_pairs_get<2>(q0, lp + 64 * (qr + 2));
							le_anchor(xanch, q0, jp);
						}
						if (ep_on && pas_on) {  // mj_energyPos: the joint spring
							const double dqs = qp - tb[b].spring;  // (last step only)
							pe += 0.5 * tb[b].stiffness * dqs * dqs;
						}
					}
					for (int k = 0; k < 4; k++) xquat[b][k] = quat[k];
					quat2mat_nocheck(xmat[b], quat);
					if constexpr (j >= 0) {
						if constexpr (T::jnt_type[j] == MJB_JNT_SLIDE) {
							double xaxis[3];
							matvec3(xaxis, xmat[b], A + LE_JAXIS);
							le_pos_slide(pos, xaxis, qp - A[LE_QPOS0]);
						} else if (offc) le_pos_offcentre(pos, xanch, xmat[b], A + LE_JPOS);  // correct for off-centre rotation
					}
					for (int k = 0; k < 3; k++) xpos[b][k] = pos[k];
					const double *const Bh = hB[b];  // the inertial half
					double xipos[3];
					if constexpr (T::body_sameframe[b]) for (int k = 0; k < 3; k++) xipos[k] = xpos[b][k];
					else le_xipos(xipos, xmat[b], xpos[b], Bh + LE_I_IPOS);
					if (eg_on) pe -= Bh[LE_I_MASS] * (grav[0] * xipos[0] + grav[1] * xipos[1] + grav[2] * xipos[2]);
					frame_sensors(Bq, xipos);
					if constexpr (LD::needed(b)) {  // the pose to C
						constexpr int ord = (LD::slot(b) - NV) / 3, rg = RING + 6 * (ord % RINGN);
						double xp[3] = { 0, 0, 0 };  // relative to the tree root's origin: what cdof is taken about
						if constexpr (r != b) for (int k = 0; k < 3; k++) xp[k] = xpos[b][k] - xpos[r][k];
						le_ring_put(lp + 64 * rg, xp, xmat[b]);
					}
				};
				// X, cdof for its own leaf -> root walk: the six doubles C publishes for V (consume), taken from the ring where V takes them -- the phase after
				// C wrote the slot, one before C writes it again; the last needed body's behind the sweep's last barrier.  Kept in registers to the tail.
				[[maybe_unused]] auto x_cdof = [&](auto Bq) {
					constexpr int b = Bq, j = T::body_jnt[b];
					if constexpr (j >= 0) {
						constexpr int cq = CD0 + 3 * (((LD::slot(b) - NV) / 3) % 2);
						le_cdof_ring_get<T::jnt_type[j] == MJB_JNT_SLIDE>(cdof[j], lp + 64 * cq);
					}
				};
				auto x_phase = [&](auto Bq, auto Cq) {  // (Cq: the body whose cdof this phase takes from C's ring, 0: none yet)
					constexpr int b = Bq, nx = NEXTN(b);
					touch_s(hA[b][0]);
					touch_s(hB[b][0]);
					if constexpr (nx < NB) {
						for (int k = 0; k < LE_A_N; k++) hA[nx][k] = reinterpret_cast<const double MJB_AS4 *>(tb + nx)[k];
						for (int k = 0; k < LE_I_N; k++) hB[nx][k] = reinterpret_cast<const double MJB_AS4 *>(tb + nx)[LE_HALF + k];
					}
					// (the cdof reads beside the quaternion's at the top of the phase, not between the pose writes and the barrier: they land under the body)
					constexpr int cb = Cq;
					if constexpr (cb > 0) {
						x_cdof(Cq);
						__builtin_amdgcn_sched_barrier(0);
					}
					x_body(Bq);
					if constexpr (nx < NB) {
						// (the entries X reads of a needed body's record, no others: its orientation is O's, its cdof C's -- the joint axis and qpos0 are a
						//  slide's business here, jpos an off-centre anchor's, and the inertia matrix nobody's)
						constexpr int jn = T::body_jnt[nx];
						const double *const a = hA[nx], *const h = hB[nx];
						asm volatile("" ::"s"(a[LE_POS]), "s"(a[LE_POS + 1]), "s"(a[LE_POS + 2]), "s"(h[LE_I_MASS]));
						if constexpr (!T::body_sameframe[nx]) asm volatile("" ::"s"(h[LE_I_IPOS]), "s"(h[LE_I_IPOS + 1]), "s"(h[LE_I_IPOS + 2]));
						if constexpr (jn >= 0) {
							if constexpr (T::jnt_type[jn < 0 ? 0 : jn] == MJB_JNT_SLIDE) asm volatile("" ::"s"(a[LE_JAXIS]), "s"(a[LE_JAXIS + 1]), "s"(a[LE_JAXIS + 2]), "s"(a[LE_QPOS0]));
							if constexpr (!LeOffc<T>::known || LeOffc<T>::on(jn < 0 ? 0 : jn)) asm volatile("" ::"s"(a[LE_JPOS]), "s"(a[LE_JPOS + 1]), "s"(a[LE_JPOS + 2]));
						}
					}
				};
				// V, body b: consume's velocity half in three pieces, so that the force half runs ONE BODY BEHIND the kinematic half.  A phase issues its body's
				// nine reads (C's cinert and cdof, qvel), works off the PREVIOUS body's forces from registers while they land -- the three cfrc writes leave
				// early in the phase and have drained long before the barrier; nobody reads them ahead of V's own leaf -> root walk -- and then takes its own
				// body's velocities.  The body's cinert waits in registers across the barrier.  The arithmetic is consume's, expression for expression.
				[[maybe_unused]] double vci[ROLE == LE_QUAD_V ? NB : 1][10], vqv[ROLE == LE_QUAD_V ? NB : 1];
				[[maybe_unused]] auto v_fetch = [&](auto Bq) {
					constexpr int b = Bq, j = T::body_jnt[b], c0 = LD::cin_slot(b);
					static_assert(c0 >= 0, "the quartet: every needed body's cinert lives in LDS");
					if constexpr (j >= 0) {
						constexpr int cq = CD0 + 3 * (((LD::slot(b) - NV) / 3) % 2);
						le_cdof_ring_get<T::jnt_type[j] == MJB_JNT_SLIDE>(cdof[j], lp + 64 * cq);
						vqv[b] = lp[64 * j].b;
					}
					le_pairs_get<5>(vci[b], lp + 64 * c0);
				};
				[[maybe_unused]] auto v_kin = [&](auto Bq) {
					constexpr int b = Bq, p = T::body_parentid[b], j = T::body_jnt[b];
					constexpr bool prest = p == 0 || !LD::needed(p);  // the world, or a jointless chain down from it: at rest
					double pv[6], pa[6];
					if constexpr (prest) le_parent_motion(pv, pa, grav);
					else le_parent_motion(pv, pa, cvel[p], cacc[p]);
					if constexpr (j >= 0) le_body_motion<prest>(cvel[b], cacc[b], pv, pa, cdof[j], vqv[b]);
					else for (int k = 0; k < 6; k++) { cvel[b][k] = pv[k]; cacc[b][k] = pa[k]; }
				};
				[[maybe_unused]] auto v_force = [&](auto Bq) {
					constexpr int b = Bq;
					double cf[6], t1[6];
					le_cfrc(cf, t1, vci[b], cvel[b], cacc[b]);
					le_cfrc_put(lp + 64 * LD::slot(b), cf, t1);
				};
				if constexpr (ROLE == LE_QUAD_C) {  // the first needed body's record, ahead of the phases as O's and X's
					if constexpr (N1 < NB) {
						c_fetch(IC<(N1 < NB ? N1 : 1)>{});
						c_touch(IC<(N1 < NB ? N1 : 1)>{});
					}
				}
				if constexpr (ROLE == LE_QUAD_O || ROLE == LE_QUAD_X) {
					// the bodies at rest: their poses from the launch's registers -- what is left per step is X's mj_energyPos term and frame sensors, at the
					// last step (or at every one, mjb_set_sensors_every_step) under their wave-uniform tests --, then the first needed body's record
					sfor<NB>([&](auto Bq) {
						constexpr int b = Bq;
						if constexpr (b > 0 && !LD::needed(b)) {
							for (int k = 0; k < 4; k++) xquat[b][k] = rxq[b][k];
							if constexpr (ROLE == LE_QUAD_X) {
								for (int k = 0; k < 9; k++) xmat[b][k] = rxm[b][k];
								for (int k = 0; k < 3; k++) xpos[b][k] = rxp[b][k];
								if (eg_on) pe -= tb[b].mass * (grav[0] * rxi[b][0] + grav[1] * rxi[b][1] + grav[2] * rxi[b][2]);
								frame_sensors(Bq, rxi[b]);
							}
						}
					});
					if constexpr (N1 < NB) {
						for (int k = 0; k < LE_A_N; k++) hA[N1][k] = reinterpret_cast<const double MJB_AS4 *>(tb + N1)[k];
						if constexpr (ROLE == LE_QUAD_X) for (int k = 0; k < LE_I_N; k++) hB[N1][k] = reinterpret_cast<const double MJB_AS4 *>(tb + N1)[LE_HALF + k];
					}
					if constexpr (ROLE == LE_QUAD_O) {
						if constexpr (HINGE(N1)) {
							opq[N1] = lp[64 * T::body_jnt[N1 < NB ? N1 : 0]];
							oq0[N1] = tb[N1].qpos0;
						}
						if constexpr (N1 < NB && HINGE(N2)) {
							opq[N2] = lp[64 * T::body_jnt[N2 < NB ? N2 : 0]];
							oq0[N2] = tb[N2].qpos0;
						}
						if constexpr (HINGE(N1)) sincos_nb((opq[N1].a - oq0[N1]) * 0.5, &osn[N1], &ocs[N1]);
					}
				}
				__builtin_amdgcn_sched_barrier(0);
				// phase k: O on the k-th needed body, X on the one before, C two, V three before (and X picks up the cdof of V's body); every wavefront takes the KN + 2 barriers, V's last body comes behind the last one
				sfor<KN + 3>([&](auto Ki) {
					constexpr int k = Ki + 1;
					constexpr int kk = k - (ROLE - LE_QUAD_O);  // this role's body, counted among the needed ones
					// (X) cdof of the body C handled one phase ago, beside V's read of the same slot; in phase KN + 3, behind the last barrier, the last body's
					constexpr bool xcd = ROLE == LE_QUAD_X && k - 3 >= 1 && k - 3 <= KN;
					constexpr int xcb = xcd ? NTH(k - 3 >= 1 ? k - 3 : 1) : 0;
					if constexpr (kk >= 1 && kk <= KN) {
						constexpr int bb = NTH(kk);
						if constexpr (ROLE == LE_QUAD_O) o_phase(IC<bb>{});
						else if constexpr (ROLE == LE_QUAD_X) x_phase(IC<bb>{}, IC<xcb>{});
						else if constexpr (ROLE == LE_QUAD_C) {
							consume(IC<bb>{});
							if constexpr (kk < KN) c_touch(IC<NTH(kk < KN ? kk + 1 : 1)>{});
						} else {
							// (V) this body's reads, the previous body's forces, this body's velocities; behind the sweep's last barrier the last body's forces too
							v_fetch(IC<bb>{});
							__builtin_amdgcn_sched_barrier(0);
							if constexpr (kk > 1) v_force(IC<NTH(kk > 1 ? kk - 1 : 1)>{});
							__builtin_amdgcn_sched_barrier(0);  // (the cfrc writes leave here, ahead of the body's velocities, and drain under them)
#ifdef MJB_LE_PROBE
							if constexpr (T::body_jnt[bb] >= 0) touch_v(vqv[bb]);
							LE_PK(8);
#endif
							v_kin(IC<bb>{});
							if constexpr (kk == KN) v_force(IC<bb>{});
						}
					} else if constexpr (xcd) x_cdof(IC<xcb>{});
					if constexpr (DV && k == 1) sfor<NV>([&](auto I) { qfa[I] = s.qfrc_applied[ev * NV + I]; });  // (read by the force block behind the sweep: a trip to HBM)
					if constexpr (k <= KN + 2) {
						LE_PK(0);
						le_barrier();
						LE_PK(2);
					}
					__builtin_amdgcn_sched_barrier(0);
				});
			}

			LE_PK(0);
			if constexpr (TRIQ && !QUAD) {  // (the trio: C's cinert of the last body is in LDS; V takes that body now)
				le_barrier();
				if constexpr (ROLE == LE_TRIO_V) consume(IC<LASTB>{});
			}
			LE_PK(1);
			// ============ A8 mj_passive, the injector's OU update, A12 mj_fwdActuation (joint transmission), qfrc_applied ============
			if constexpr (DV) {
				if (nz_on && attempt == 0) {
					const double rate = Pq->nz.rate, scale = Pq->nz.scale;
					sfor<NU>([&](auto I) { const double v = rate * cn[I] + scale * z[I]; cn[I] = rs ? 0.0 : v; });
				}
				double ctrl[NU > 0 ? NU : 1];
				if (nz_on) {
					sfor<NU>([&](auto I) { ctrl[I] = cn[I]; });
				} else {
					sfor<NU>([&](auto I) { const double c = pinv(s.ctrl[ev * NU + I]); ctrl[I] = wasreset ? 0.0 : c; });  // (load first: a select around a load becomes a per-lane branch)
				}
				// ---- (HW) MujocoRosControlPlugin::controlCallback's cadence around writeSim (hwsim_write, mjb_step.hip): the decisions differ between
				// the lanes, so they are selects; a lane the retry does not concern (h_run false) stores back what it loaded
				[[maybe_unused]] bool h_upd = false, h_wr = false;
				[[maybe_unused]] double h_dt = dt;
				[[maybe_unused]] const bool h_run = attempt == 0 || hw_bad;
				if constexpr (HW) {
					const HwSim MJB_AS4 &hw = Pq->hw;
					const long long per_ns = hw.period_ns;
					h_wr = true;
					if (per_ns > 0) {
						const double lu0 = pinv(hlu), lw0 = pinv(hlw);
						const long long t = ros_ns_nb(time);
						long long lu = (long long)lu0, lw = (long long)lw0;
						const bool back = t < lu;  // the time went backwards (reset): both stamps re-armed
						lu = sell(back, t, lu);
						lw = sell(back, t, lw);
						const long long sim_period = t - lu;
						h_upd = (sim_period >= per_ns) | ((lu == 0) & (sim_period != 0));  // (nothing happens at t = 0)
						lu = sell(h_upd, t, lu);
						h_wr = (lu != 0) & (t > lw);
						h_dt = 1e-9 * (double)(t - lw);
						double *const cad = hw.cad + ev * (size_t)(2 + 2 * hw.n);
						const double lu1 = (double)lu, lw1 = (double)sell(h_wr, t, lw);
						cad[0] = seld(h_run, lu1, lu0);
						cad[1] = seld(h_run, lw1, lw0);
					}
					h_upd = h_upd & h_run;
					hw_wr = (h_run & h_wr) | (!h_run & hw_wr);
					h_wr = h_wr & h_run;
				}
				// (HW) dof j's qfrc_applied after the stage; sj: the dof's (qpos, qvel)
				[[maybe_unused]] auto hw_dof = [&](auto I, const Pair sj) __attribute__((always_inline)) -> double {
					constexpr int j = I;
					const HwSim MJB_AS4 &hw = Pq->hw;
					const double fa0 = pinv(qfa[j]);
					const int k = hw.le_tab[4 * j];
					if (k < 0) {  // not controlled: the user's value, zero after an in-launch reset -- and so it stands in HBM after the launch, as the generic kernels' frame copy does
						const double v = seld(wasreset, 0.0, fa0);
						if (last && __builtin_amdgcn_ballot_w64(wasreset)) s.qfrc_applied[ev * NV + j] = v;
						return v;
					}
					const int method = hw.le_tab[4 * j + 1], kind = hw.le_tab[4 * j + 2], aw = hw.le_tab[4 * j + 3], hn = hw.n;
					const double MJB_AS4 *const gn = hw.le_gains + 8 * j;
					const bool estop = hw.estop != 0;
					const size_t at = ev * (size_t)hn + (size_t)k;
					double pos = sj.a, vel = sj.b;
					if (hw.period_ns > 0) {  // readSim at an update: the joint state the PIDs see until the next one
						const double jp0 = pinv(hjp[j]), jv0 = pinv(hjv[j]);
						double jpn = sj.a;
						if (kind != MJB_HW_PRISMATIC) jpn = jp0 + angdist_nb(jp0, sj.a);
						pos = seld(h_upd, jpn, jp0);
						vel = seld(h_upd, sj.b, jv0);
						double *const cad = hw.cad + ev * (size_t)(2 + 2 * hn);
						cad[2 + k] = pos;
						cad[2 + hn + k] = vel;
					}
					const double cmd = pinv(hcmd[j]);
					double out = 0, error = 0;
					if (method == MJB_HW_EFFORT) out = estop ? 0.0 : cmd;
					else if (method == MJB_HW_POSITION) hov[j] = cmd;
					else if (method == MJB_HW_VELOCITY) hov[j] = estop ? 0.0 : cmd;
					else if (method == MJB_HW_POSITION_PID) {
						if (kind == MJB_HW_REVOLUTE) {
							const double lower = gn[6], upper = gn[7];
							if (upper > lower) error = angdist_with_limits_nb(pos, fmin(fmax(cmd, lower), upper), lower, upper);
							else error = cmd - pos;
						} else if (kind == MJB_HW_CONTINUOUS) error = angdist_nb(pos, cmd);
						else error = cmd - pos;
					} else error = estop ? -vel : cmd - vel;
					if (method == MJB_HW_POSITION_PID || method == MJB_HW_VELOCITY_PID) {
						const double ierr0 = pinv(hpi[j]), last0 = pinv(hpl[j]);
						const double gi = gn[1];
						const double derr = (error - last0) / h_dt;
						double ierr = ierr0 + h_dt * error;
						if (aw && gi != 0) ierr = fmin(fmax(ierr, gn[4] / fabs(gi)), gn[3] / fabs(gi));
						double iterm = gi * ierr;
						if (!aw) iterm = fmin(fmax(iterm, gn[4]), gn[3]);
						out = gn[0] * error + iterm + gn[2] * derr;
						const double el = gn[5];
						if (el > 0) out = fmin(fmax(out, -el), el);
						double *const pp = hw.pid + 2 * at;
						pp[0] = seld(h_wr, ierr, ierr0);
						pp[1] = seld(h_wr, error, last0);
					}
					// (the frame's qfrc_applied is zero after mj_resetData in this step; the stage then rewrites the dof if it writes. Only where the stage
					//  runs on this trip: a lane that mj_checkPos / mj_checkVel reset and another lane's retry does not concern keeps what trip 0 stored)
					const double fa = seld(h_wr, out, seld(h_run & (rs | hw_bad), 0.0, fa0));
					s.qfrc_applied[ev * NV + j] = fa;
					return fa;
				};
				Pair sq[NV > 0 ? NV : 1];
				sfor<NV>([&](auto I) {
					constexpr int j = I;
					sq[j] = lp[64 * j];
					const LeTapeBody MJB_AS4 &tj = tb[T::jnt_bodyid[j]];
					double pas = 0;
					if constexpr (PE) {
						if (pas_on) {
							pas = -pe_ld(OV::joint(T::jnt_bodyid[j], 0)) * (sq[j].a - tj.spring);
							pas -= pe_ld(OV::joint(T::jnt_bodyid[j], 1)) * sq[j].b;
						}
					} else
					if (pas_on) {
						pas = -tj.stiffness * (sq[j].a - tj.spring);
						pas -= tj.damping * sq[j].b;
					}
					if constexpr (HW) f[j] = pas + hw_dof(I, sq[j]);
					else
					f[j] = pas + (wasreset ? 0.0 : qfa[j]);
				});
				const bool act_on = !(m.disableflags & MJB_DSBL_ACTUATION);
				const bool clamp_on = !(m.disableflags & MJB_DSBL_CLAMPCTRL);
				// (TEN) the wrap records of the tape, behind the row records: the coefficients of the tendons' moment arms
				[[maybe_unused]] const LeTapeWrap MJB_AS4 *const tw = reinterpret_cast<const LeTapeWrap MJB_AS4 *>(
					reinterpret_cast<const unsigned char MJB_AS4 *>(ta + NU) + (NR > 0 ? sizeof(LeTapeLimHdr) + NL * sizeof(LeTapeLim) + NE * sizeof(LeTapeEq) : 0));
				sfor<NU>([&](auto U) {
					// (an actuator on a fixed tendon, LeTen: its moment arm is the compile-time list of its wraps' dofs, gear * the tape's coefficients)
					constexpr int i = U;
					constexpr bool ten = LeTen<T>::on(i);
					constexpr int j = ten ? 0 : T::act_jnt[i], nwr = LeTen<T>::num(i);
					double force = 0;
					const LeTapeAct MJB_AS4 &A = ta[i];
					const double gear = A.gear;
					// actuator_length = gear * the joint's position | the tendon's length, sum_w coef_w qpos_w;  actuator_velocity = moment . qvel
					auto alen = [&]() -> double {
						if constexpr (ten) {
							double sm = 0;
							sfor<nwr>([&](auto K) { sm += tw[LeTen<T>::wrap(i, K)].coef * sq[LeTen<T>::jnt(i, K)].a; });
							return sm * gear;
						} else return sq[j].a * gear;
					};
					auto avel = [&]() -> double {
						if constexpr (ten) {
							double sm = 0;
							sfor<nwr>([&](auto K) { sm += gear * tw[LeTen<T>::wrap(i, K)].coef * sq[LeTen<T>::jnt(i, K)].b; });
							return sm;
						} else return sq[j].b * gear;
					};
					// (NA > 0) an actuator with an activation state: its force is gain * act + bias on the CURRENT act, and the clamped ctrl drives act_dot
					constexpr bool stateful = NA > 0 && T::act_dyntype[i] != MJB_DYN_NONE;
					constexpr int ja = stateful ? T::act_actadr[i] : 0;
					static_assert(!stateful || (ja >= 0 && ja < NA), "lane = env kernel: a stateful actuator's slot of act");
					[[maybe_unused]] double dot = 0;  // act_dot (zero under mjDSBL_ACTUATION: act keeps its value, clamped)
					if (act_on) {
						double c = ctrl[i];
						if constexpr (T::act_ctrllimited[i]) {
							if (clamp_on) c = clampd(c, A.ctrllo, A.ctrlhi);
						}
						if constexpr (stateful) {
							const double a0 = act[ja];
							if constexpr (T::act_dyntype[i] == MJB_DYN_INTEGRATOR) dot = c;
							else dot = (c - a0) / A.dyntau;  // (filter: the tape holds max(mjMINVAL, dynprm[0]))
							c = a0;
						}
						const double len = alen(), vel = avel();
						double gain = 0, bs = 0;
						if constexpr (PE) {
							gain = pe_ld(OV::act(i, 0));
							if constexpr (T::act_gaintype[i] == MJB_GAIN_AFFINE) gain = gain + pe_ld(OV::act(i, 1)) * len + pe_ld(OV::act(i, 2)) * vel;
							if constexpr (T::act_biastype[i] == MJB_BIAS_AFFINE) bs = pe_ld(OV::act(i, 3)) + pe_ld(OV::act(i, 4)) * len + pe_ld(OV::act(i, 5)) * vel;
						} else {
						gain = A.gain[0];
						if constexpr (T::act_gaintype[i] == MJB_GAIN_AFFINE) gain = gain + A.gain[1] * len + A.gain[2] * vel;
						if constexpr (T::act_biastype[i] == MJB_BIAS_AFFINE) bs = A.bias[0] + A.bias[1] * len + A.bias[2] * vel;
						}
						force = gain * c + bs;
						if constexpr (T::act_forcelimited[i]) force = clampd(force, A.forcelo, A.forcehi);
						if constexpr (ten) sfor<nwr>([&](auto K) { f[LeTen<T>::jnt(i, K)] += gear * tw[LeTen<T>::wrap(i, K)].coef * force; });
						else
						f[j] += gear * force;
					}
					if constexpr (stateful) {  // mj_advance's half of mj_Euler for this actuator (advance_act, mjb_step.hip)
						double a = act[ja] + dt * dot;
						if constexpr (T::act_actlimited[i]) a = clampd(a, A.actlo, A.acthi);
						actn[ja] = a;
					}
					if (sens_on) {
						sfor<T::NSENSOR>([&](auto S) {
							constexpr int q = S;
							if constexpr (T::sensor_objid[q] == i && (T::sensor_type[q] == MJB_SENS_ACTUATORFRC || T::sensor_type[q] == MJB_SENS_ACTUATORPOS || T::sensor_type[q] == MJB_SENS_ACTUATORVEL)) {
								double v = T::sensor_type[q] == MJB_SENS_ACTUATORFRC ? force : (T::sensor_type[q] == MJB_SENS_ACTUATORPOS ? alen() : avel());
								const double cut = m.sensor_cutoff[q];
								sd[T::sensor_adr[q]] = cut > 0 ? clampd(v, -cut, cut) : v;
							}
						});
					}
				});
			}
			if (sens_on) {
				sfor<T::NSENSOR>([&](auto S) {
					constexpr int q = S, type = T::sensor_type[q];
					if constexpr (type == MJB_SENS_JOINTPOS || type == MJB_SENS_JOINTVEL || type == MJB_SENS_CLOCK) {
						constexpr int jj = T::sensor_objid[q] < 0 ? 0 : T::sensor_objid[q];
						const Pair s3 = lp[64 * jj];
						const double v = type == MJB_SENS_CLOCK ? time : (type == MJB_SENS_JOINTPOS ? s3.a : s3.b);
						const double cut = m.sensor_cutoff[q];
						sd[T::sensor_adr[q]] = cut > 0 ? clampd(v, -cut, cut) : v;
					}
				});
			}
			__builtin_amdgcn_sched_barrier(0);

			LE_PK(2);
			// ================= A2 mj_crb + A9 RNE backward pass, one sweep leaf -> root =================
			double qM[NV > 0 ? NV : 1][NV > 0 ? NV : 1];  // [i][a], a = i or an ancestor of i (the other entries never exist)
			double csum[NB][6], crbs[NB][10];             // forces / composite inertias of a body's children, summed as the sweep passes them
			double pcf[NB][6], pcb[NB][10], parm[NB];     // the NEXT body's force / cinert / joint armature, fetched one region ahead
			auto fetch_body = [&](auto Bn) {
				constexpr int nb = Bn;
				constexpr int q0 = LD::slot(nb);
				if constexpr (PE && T::body_jnt[nb] >= 0) parm[nb] = pe_ld(OV::joint(nb, 2));
				else
				if constexpr (DPW && T::body_jnt[nb] >= 0) parm[nb] = tb[nb].armature;
				if constexpr (DV) {
					const Pair c0 = lp[64 * q0], c1 = lp[64 * (q0 + 1)], c2 = lp[64 * (q0 + 2)];
					pcf[nb][0] = c0.a; pcf[nb][1] = c0.b; pcf[nb][2] = c1.a; pcf[nb][3] = c1.b; pcf[nb][4] = c2.a; pcf[nb][5] = c2.b;
				}
				if constexpr (DPW && LD::cin_slot(nb) >= 0) {
					constexpr int cs = LD::cin_slot(nb);
					for (int k = 0; k < 5; k++) {
						const Pair c = lp[64 * (cs + k)];
						pcb[nb][2 * k] = c.a;
						pcb[nb][2 * k + 1] = c.b;
					}
				}
			};
			{
				constexpr int lastb = [] { for (int c = NB - 1; c >= 1; c--) if (LD::needed(c)) return c; return 0; }();
				if constexpr (lastb > 0) fetch_body(IC<lastb>{});
			}
			sfor<NB - 1>([&](auto Bi) {
				constexpr int b = NB - 1 - Bi;
				constexpr int p = T::body_parentid[b], j = T::body_jnt[b];
				if constexpr (LD::needed(b)) {
					if constexpr (DV) touch_v(pcf[b][0]);
					else if constexpr (DPW && LD::cin_slot(b) >= 0) touch_v(pcb[b][0]);
					if constexpr (PE && j >= 0) touch_v(parm[b]);
					else
					if constexpr (DPW && j >= 0) touch_s(parm[b]);
					{
						constexpr int nb = [] { for (int c = b - 1; c >= 1; c--) if (LD::needed(c)) return c; return 0; }();
						if constexpr (nb > 0) fetch_body(IC<nb>{});
					}
					[[maybe_unused]] double cf[6] = { 0, 0, 0, 0, 0, 0 };
					if constexpr (DV) for (int k = 0; k < 6; k++) cf[k] = pcf[b][k];
					// (children have larger ids: their sums are complete; cset is a compile-time fact after unrolling)
					constexpr bool has_child = [] { for (int c = b + 1; c < NB; c++) if (T::body_parentid[c] == b && LD::needed(c)) return true; return false; }();
					if constexpr (DV && has_child) for (int k = 0; k < 6; k++) cf[k] += csum[b][k];
					[[maybe_unused]] double cb[10];  // composite inertia of the body (mj_crb)
					if constexpr (DPW) {
						if constexpr (LD::cin_slot(b) >= 0) {
							for (int k = 0; k < 10; k++) cb[k] = pcb[b][k];
						} else {
							for (int k = 0; k < 10; k++) cb[k] = cin[b][k];
						}
						if constexpr (has_child) for (int k = 0; k < 10; k++) cb[k] += crbs[b][k];
					}
					if constexpr (j >= 0) {
						if constexpr (DV) f[j] -= dot6r(cdof[j], cf);
						if constexpr (DPW) {
							double buf[6];
							mul_inert_vec(buf, cb, cdof[j]);
							sfor<NV>([&](auto A) {
								constexpr int a = A;
								if constexpr (Q::anc(a, j)) qM[j][a] = (a == j ? parm[b] : 0.0) + dot6r(cdof[a], buf);
							});
						}
					}
					if constexpr (p > 0 && LD::needed(p)) {
						constexpr bool first = [] { for (int c = b + 1; c < NB; c++) if (T::body_parentid[c] == p && LD::needed(c)) return false; return true; }();
						if constexpr (DV) {
							if constexpr (first) for (int k = 0; k < 6; k++) csum[p][k] = cf[k];
							else for (int k = 0; k < 6; k++) csum[p][k] += cf[k];
						}
						if constexpr (DPW) {
							if constexpr (first) for (int k = 0; k < 10; k++) crbs[p][k] = cb[k];
							else for (int k = 0; k < 10; k++) crbs[p][k] += cb[k];
						}
					}
				}
				__builtin_amdgcn_sched_barrier(0);
			});
			LE_PK(3);
			if constexpr (POSEW) en_pe = pe;
			if constexpr (DUO && !DP && !XW) {
				// ---- V's half ends here: qfrc_smooth to P, then P's verdict on the step (the trio's P: the two rendezvous and the verdict)
				if constexpr (DV) sfor<(NV + 1) / 2>([&](auto K) {
					constexpr int k = K;
					lp[64 * (XS + k)] = Pair{ f[2 * k], 2 * k + 1 < NV ? f[2 * k + 1 < NV ? 2 * k + 1 : 0] : 0.0 };
				});
				LE_PK(4);
				le_barrier();  // (A) qfrc_smooth is in LDS; P's factors are ready
				LE_PK(5);
				le_barrier();  // (B) P has solved and either integrated or -- bad qacc -- reset its lanes
				int code = (int)lp[64 * MAIL].a;
				if constexpr (QUAD) code |= (int)lp[64 * XMAIL].a;  // (four wavefronts: bits 0 / 1 are C's, on the state it committed; bits 2 / 3 X's, mj_checkAcc)
				LE_PK(6);
				if (!(__builtin_amdgcn_readfirstlane(code) & 8)) {  // (bit 3: P's ballot, the same in every lane)
					badp_next = (code & 2) != 0;
					badv_next = (code & 1) != 0;
					break;
				}
				const bool bada = (code & 4) != 0;  // mj_checkAcc reset this lane: the forward pass runs once more
				sfor<NU>([&](auto I) { cn[I] = bada ? 0.0 : cn[I]; });
				time = bada ? 0.0 : time;
				wasreset = wasreset || bada;
				if constexpr (QUAD) le_barrier();  // (R) C has put the old state back, the reset lanes' qpos0: the second trip reads it
				continue;
			}
			if (e_on) {  // mj_energyVel: 0.5 qvel' M qvel (mj_energyPos was gathered along the sweep)
				double ke = 0, qv[NV > 0 ? NV : 1];
				sfor<NV>([&](auto I) { qv[I] = lp[64 * I].b; });
				sfor<NV>([&](auto I) {
					sfor<NV>([&](auto A) {
						constexpr int i = I, a = A;
						if constexpr (Q::anc(a, i)) ke += (a == i ? 0.5 : 1.0) * qM[i][a] * qv[i] * qv[a];
					});
				});
				if constexpr (EPOS) en_pe = pe;
				en_ke = ke;
			}

			// ================= A3 mj_factorM + A12 mj_fwdAcceleration; A16's (M + h B) factor and solve beside them =================
			// L'DL in place, pivots from the last dof up: row k scaled by 1 / D_k, then row i -= L_ki * (row k restricted to i's ancestors)
			const bool damp_on = m.eulerdamp != 0;
			// (four wavefronts: X has the M of every line below and no other, C the M + h B -- with mjDSBL_EULERDAMP C's h B is zero and its arithmetic X's)
			double qH[NV > 0 ? NV : 1][NV > 0 ? NV : 1], dinv[NV > 0 ? NV : 1], hinv[NV > 0 ? NV : 1];
			if constexpr (FH) {
				sfor<NV>([&](auto I) {
					sfor<NV>([&](auto A) {
						constexpr int i = I, a = A;
						if constexpr (PE) {
							if constexpr (Q::anc(a, i) && a == i) qH[i][a] = qM[i][a] + pe_ld(OV::joint(T::jnt_bodyid[i], 3));
							else if constexpr (Q::anc(a, i)) qH[i][a] = qM[i][a];
						} else
						if constexpr (Q::anc(a, i) && a == i && !FM) {
							const double hd = pins(tb[T::jnt_bodyid[i]].hdamping);  // (loaded, then selected)
							qH[i][a] = qM[i][a] + (damp_on ? hd : 0.0);
						} else
						if constexpr (Q::anc(a, i)) qH[i][a] = qM[i][a] + (a == i ? tb[T::jnt_bodyid[i]].hdamping : 0.0);
					});
				});
			}
			sfor<NV>([&](auto Ki) {
				constexpr int k = NV - 1 - Ki;
				if constexpr (FM) dinv[k] = frcp(qM[k][k]);
				if constexpr (FH) hinv[k] = frcp(qH[k][k]);
				sfor<NV>([&](auto Ii) {
					constexpr int i = NV - 1 - Ii;  // ancestors of k, nearest first
					if constexpr (i < k && Q::anc(i, k)) {
						[[maybe_unused]] double tm = 0;
						if constexpr (FM) tm = qM[k][i] * dinv[k];
						[[maybe_unused]] double th = 0;
						if constexpr (FH) th = qH[k][i] * hinv[k];
						sfor<NV>([&](auto A) {
							constexpr int a = A;
							if constexpr (Q::anc(a, i)) {
								if constexpr (FM) qM[i][a] -= tm * qM[k][a];
								if constexpr (FH) qH[i][a] -= th * qH[k][a];
							}
						});
						if constexpr (FM) qM[k][i] = tm;
						if constexpr (FH) qH[k][i] = th;
					}
				});
			});
			// x = M^-1 f and y = (M + h B)^-1 f: L' sweep, D, L sweep
			double x[NV > 0 ? NV : 1], y[NV > 0 ? NV : 1];
			if constexpr (DUO && DPW && NV > 0) {  // (the factors BEFORE the rendezvous: left alone the compiler sinks them behind it, next to the solves)
				if constexpr (FM) touch_v(dinv[0]);
				if constexpr (FH) touch_v(hinv[0]);
			}
			LE_PK(4);
			if constexpr (DUO && DPW) {
				le_barrier();  // (A) V's qfrc_smooth
				LE_PK(5);
				sfor<(NV + 1) / 2>([&](auto K) {
					constexpr int k = K;
					const Pair v = lp[64 * (XS + k)];
					f[2 * k] = v.a;
					if constexpr (2 * k + 1 < NV) f[2 * k + 1] = v.b;
				});
			}
			sfor<NV>([&](auto I) { x[I] = f[I]; y[I] = f[I]; });
			sfor<NV>([&](auto Ii) {
				constexpr int i = NV - 1 - Ii;
				sfor<NV>([&](auto A) {
					constexpr int a = A;
					if constexpr (a < i && Q::anc(a, i)) { if constexpr (FM) x[a] -= qM[i][a] * x[i]; if constexpr (FH) y[a] -= qH[i][a] * y[i]; }
				});
			});
			sfor<NV>([&](auto I) { if constexpr (FM) x[I] *= dinv[I]; if constexpr (FH) y[I] *= hinv[I]; });
			sfor<NV>([&](auto I) {
				constexpr int i = I;
				sfor<NV>([&](auto Ai) {
					constexpr int a = NV - 1 - Ai;  // nearest ancestor first, as mj_solveLD walks them
					if constexpr (a < i && Q::anc(a, i)) { if constexpr (FM) x[i] -= qM[i][a] * x[a]; if constexpr (FH) y[i] -= qH[i][a] * y[a]; }
				});
			});
			if constexpr (XW) sfor<NV>([&](auto I) { qacc[I] = x[I]; });
			else if constexpr (!FM) sfor<NV>([&](auto I) { qaccd[I] = y[I]; });
			else
			sfor<NV>([&](auto I) { qacc[I] = x[I]; qaccd[I] = damp_on ? y[I] : x[I]; });

			// ================= the constraint stage of a model with constraint rows: mj_makeConstraint, mj_projectConstraint, mj_referenceConstraint, mj_solPGS =================
			// One env per lane, the oracle's mjo_make_constraint (joint equalities, hinge / slide limits) .. mjo_fwd_constraint (PGS) in its operation order.  The
			// row list is static, in MuJoCo's order: the NE joint-equality rows -- J = e_d1 - poly'(x) e_d2, the second coefficient per-lane data --, then the NL
			// limit rows -- the r-th limited joint, J = +- e_j.  An equality row is every lane's unless mjDSBL_EQUALITY / mjDSBL_CONSTRAINT is set (wave-uniform):
			// its gates are compile-time.  Which limit rows an env has is per-lane data: selects.  Which of them ANY lane of the wavefront has is a ballot: rows
			// nobody has are skipped by scalar branches, a wavefront without rows pays the NL comparisons and nothing else.  Row constants (LeTapeEq, LeTapeLim)
			// are wave-uniform, and so are the branches on them.  qacc (= qacc_smooth so far) and qaccd come out constrained: the acceleration-stage sensors,
			// mj_checkAcc and mj_Euler below see them.  On the retry of the attempt loop the stage runs again on the reset state.
			if constexpr (NR > 0) {
				const LeTapeLimHdr MJB_AS4 *const tlh = reinterpret_cast<const LeTapeLimHdr MJB_AS4 *>(ta + NU);
				const LeTapeLim MJB_AS4 *const tl = reinterpret_cast<const LeTapeLim MJB_AS4 *>(tlh + 1);
				[[maybe_unused]] const LeTapeEq MJB_AS4 *const te = reinterpret_cast<const LeTapeEq MJB_AS4 *>(tl + NL);
				[[maybe_unused]] const bool lim_on = !(m.disableflags & (MJB_DSBL_CONSTRAINT | MJB_DSBL_LIMIT));
				[[maybe_unused]] const bool eq_on = !(m.disableflags & (MJB_DSBL_CONSTRAINT | MJB_DSBL_EQUALITY));
				bool ract[NR], rwav[NR], anyw = false, has = false;  // the lane has the row | some lane of the wavefront has it (an equality row: always)
				double rsg[NR], rpos[NR];                            // J's entry at the row's joint (equality +1; limit: lower +1, upper -1) | efc_pos
				[[maybe_unused]] double rc2[NE > 0 ? NE : 1];        // an equality row's entry at its second joint, -poly'(x)
				int nrow = 0;
				sfor<NW>([&](auto W) { qfc[W] = 0; });
				sfor<NR>([&](auto R) {
					constexpr int r = R, j = LM::jnt(r);
					if constexpr (LM::is_eq(r)) {
						constexpr int j2 = LM::jnt2(r);
						const LeTapeEq MJB_AS4 &E = te[r];
						double poly = E.polycoef[0], der = 0;
						if constexpr (j2 >= 0) {
							const double x = lp[64 * (j2 < 0 ? 0 : j2)].a - E.qpos0[1];
							poly = E.polycoef[0] + x * (E.polycoef[1] + x * (E.polycoef[2] + x * (E.polycoef[3] + x * E.polycoef[4])));
							der = E.polycoef[1] + x * (2 * E.polycoef[2] + x * (3 * E.polycoef[3] + x * 4 * E.polycoef[4]));
						}
						ract[r] = eq_on;
						rwav[r] = true;
						rsg[r] = 1.0;
						rc2[r] = -der;
						rpos[r] = lp[64 * j].a - E.qpos0[0] - poly;
						anyw = anyw || eq_on;
						has = has || eq_on;
						nrow += eq_on ? 1 : 0;
					} else {
						constexpr int l = r - NE;
						const double q = lp[64 * j].a, mg = tl[l].margin;
						const double dlo = q - tl[l].range[0], dhi = tl[l].range[1] - q;
						const bool up = dhi < mg, a = lim_on && ((dlo < mg) || up);  // (range > 2 margin: at most one side)
						ract[r] = a;
						rsg[r] = up ? -1.0 : 1.0;
						rpos[r] = up ? dhi : dlo;
						rwav[r] = __builtin_amdgcn_ballot_w64(a) != 0;
						anyw = anyw || rwav[r];
						has = has || a;
						nrow += a ? 1 : 0;
					}
				});
				c_nefc = nrow;
				c_iter = 0;
				if (anyw) {  // (wave-uniform)
					double rD[NR], raref[NR], rb[NR], rf[NR], rinv[NR];
					// J_r . v for a vector held per dof: the row's one or two entries
					auto jdot = [&](auto R, const double *v) -> double {
						constexpr int r = R, j = LM::jnt(r), j2 = LM::jnt2(r);
						if constexpr (j2 >= 0) return rsg[r] * v[j] + rc2[r < NE ? r : 0] * v[j2 < 0 ? 0 : j2];
						else return rsg[r] * v[j];
					};
					// mj_makeImpedance's impedance of a row at pm = pos - margin (row_params_x / impedance) from its clamped solimp and the curve's two constants
					auto impedance = [&](const double MJB_AS4 *si, const double powa, const double powb, const double pm) -> double {
						const double d0 = si[0], d1 = si[1], wd = si[2], mid = si[3], pw = si[4];
						double imp;
						if (d0 == d1 || wd <= MJB_MINVAL) imp = 0.5 * (d0 + d1);
						else {
							const double xi = fabs(pm / wd);
							double yv;
							if (pw == 1) yv = xi;
							else {
								const bool lowh = xi <= mid;
								const double xx = lowh ? xi : 1 - xi;
								double px;
								if (pw == 2) px = xx * xx;
								else px = pow(xx, pw);
								const double ya = powa * px, yb = 1 - powb * px;
								yv = lowh ? ya : yb;
							}
							const double mixed = d0 + yv * (d1 - d0);
							imp = (xi >= 1) ? d1 : ((xi <= 0) ? d0 : mixed);
						}
						return imp;
					};
					// ---- row parameters (mj_makeImpedance), aref (mj_referenceConstraint), b = J qacc_smooth - aref
					[[maybe_unused]] double rR[NR];
					sfor<NR>([&](auto R) {
						constexpr int r = R, j = LM::jnt(r), j2 = LM::jnt2(r);
						rD[r] = 1, raref[r] = 0, rb[r] = 0, rf[r] = 0, rinv[r] = 1, rR[r] = 1;
						if (rwav[r]) {
							double imp, pm, invw, Kk, Bb;
							if constexpr (LM::is_eq(r)) {
								const LeTapeEq MJB_AS4 &E = te[r];
								pm = rpos[r];  // (margin 0)
								imp = impedance(E.solimp, E.powa, E.powb, pm);
								invw = E.invweight0, Kk = E.K, Bb = E.B;
							} else {
								const LeTapeLim MJB_AS4 &L = tl[r - NE];
								pm = rpos[r] - L.margin;
								imp = impedance(L.solimp, L.powa, L.powb, pm);
								invw = L.invweight0, Kk = L.K, Bb = L.B;
							}
							const double Rr = fmax(MJB_MINVAL, (1 - imp) * invw / imp);
							const double Ra = ract[r] ? Rr : 1.0;  // (a lane without the row: harmless numbers, its force stays zero)
							double vel = rsg[r] * lp[64 * j].b, acc = rsg[r] * qacc[j];
							if constexpr (j2 >= 0) {
								vel += rc2[r < NE ? r : 0] * lp[64 * (j2 < 0 ? 0 : j2)].b;
								acc += rc2[r < NE ? r : 0] * qacc[j2 < 0 ? 0 : j2];
							}
							const double ar = -Bb * vel - Kk * imp * pm;
							rR[r] = Ra;
							rD[r] = 1.0 / Ra;
							raref[r] = ract[r] ? ar : 0.0;
							rb[r] = ract[r] ? acc - ar : 0.0;
						}
					});
					// ---- AR = J M^-1 J' + diag(R): M^-1 J_r' of the wave-active rows from the L'DL factor of M (the right-hand side is the row's one or two
					// entries, the known zeros skipped on the union of their patterns), AR_kr = J_k . (M^-1 J_r'), symmetrised as the oracle does and packed into
					// LDS.  Column r leaves its entries for the rows behind it raw; the rows behind symmetrise them with their own where both rows are wave-active
					sfor<NR>([&](auto R) {
						constexpr int r = R, j = LM::jnt(r), j2 = LM::jnt2(r);
						if (rwav[r]) {
							double c[NV];
							sfor<NV>([&](auto I) {
								if constexpr ((int)I == j) c[I] = rsg[r];
								else if constexpr ((int)I == j2) c[I] = rc2[r < NE ? r : 0];
								else c[I] = 0.0;
							});
							sfor<NV>([&](auto Ii) {
								constexpr int i = NV - 1 - Ii;
								if constexpr (LM::ranc(i, r))
									sfor<NV>([&](auto A) {
										constexpr int a = A;
										if constexpr (a < i && Q::anc(a, i)) c[a] -= qM[i][a] * c[i];
									});
							});
							sfor<NV>([&](auto I) { if constexpr (LM::ranc(I, r)) c[I] *= dinv[I]; });
							sfor<NV>([&](auto I) {
								constexpr int i = I;
								sfor<NV>([&](auto Ai) {
									constexpr int a = NV - 1 - Ai;
									if constexpr (a < i && Q::anc(a, i) && LM::rcoupled(a, r)) c[i] -= qM[i][a] * c[a];
								});
							});
							sfor<NR>([&](auto K) {
								constexpr int k = K;
								if constexpr (k == r) {
									const double aii = jdot(R, c) + rR[r];
									lim_st(IC<LM::ar(r, r)>{}, aii);
									rinv[r] = 1.0 / aii;
								} else if constexpr (!LM::rows_coupled(k, r)) {
									if constexpr (k > r) lim_st(IC<LM::ar(r, k)>{}, 0.0);  // (two trees: a known zero on both sides)
								} else if constexpr (k > r) {
									lim_st(IC<LM::ar(r, k)>{}, jdot(K, c));
								} else {
									if (rwav[k]) {
										const double g = lim_ld(IC<LM::ar(k, r)>{});
										lim_st(IC<LM::ar(k, r)>{}, 0.5 * (jdot(K, c) + g));
									}
								}
							});
						}
					});
					// (read unconditionally, zero by select where row k is nobody's: a row's reads leave together instead of one behind each scalar branch -- and a
					//  stale entry of an inactive row never meets a force, not even a zero one)
					auto AR = [&](auto I, auto K) -> double { const double a = lim_ld(IC<LM::ar(I, K)>{}); return rwav[K] ? a : 0.0; };
					// ---- warmstart: the forces qacc_warmstart implies -- an equality row's unconditionally, a limit row's where it pushes --, kept if their dual
					// cost 0.5 f' AR f + f' b is not positive
					if (tlh->nowarm == 0) {
						sfor<NR>([&](auto R) {
							constexpr int r = R, j = LM::jnt(r), j2 = LM::jnt2(r);
							if (rwav[r]) {
								double jw = rsg[r] * lim_ld(IC<LM::ws(LM::widx(j))>{});
								if constexpr (j2 >= 0) jw += rc2[r < NE ? r : 0] * lim_ld(IC<LM::ws(LM::widx(j2 < 0 ? 0 : j2))>{});
								const double jar = jw - raref[r];
								double fw;
								if constexpr (LM::is_eq(r)) fw = -rD[r] * jar;
								else fw = jar < 0 ? -rD[r] * jar : 0.0;
								rf[r] = ract[r] ? fw : 0.0;
							}
						});
						double cost = 0;
						sfor<NR>([&](auto I) {
							constexpr int i = I;
							if (rwav[i]) {
								double sm = 0;
								sfor<NR>([&](auto K) { sm += AR(I, K) * rf[K]; });
								cost += 0.5 * rf[i] * sm + rf[i] * rb[i];
							}
						});
						const bool drop = cost > 0;
						sfor<NR>([&](auto R) { rf[R] = drop ? 0.0 : rf[R]; });
					}
					// ---- mj_solPGS: sweeps over the rows until the lane's improvement falls under the tolerance or its sweeps run out; a lane that is done keeps
					// its forces, the loop runs while a lane is not.  A limit row's force is clamped at zero, an equality row's is not
					const double scale = tlh->scale, tol = tlh->tolerance;
					const int itmax = (int)tlh->iterations;
					bool done = !has || itmax <= 0;
					int iter = 0;
					while (__builtin_amdgcn_ballot_w64(!done)) {
						double improvement = 0;
						sfor<NR>([&](auto I) {
							constexpr int i = I;
							// (a row is swept while a lane that has it is still sweeping: the loop's long tail is a few lanes' rows, not the wavefront's)
							if (__builtin_amdgcn_ballot_w64(ract[i] && !done)) {
								double arow[NR];
								sfor<NR>([&](auto K) { arow[K] = lim_ld(IC<LM::ar(I, K)>{}); });
								touch_vn<NR>(arow);  // (the row's reads, issued together)
								double res = rb[i];
								sfor<NR>([&](auto K) { res += (rwav[K] ? arow[K] : 0.0) * rf[K]; });
								const double aii = arow[i];
								const double old = rf[i];
								const double f1 = old - res * rinv[i];
								double f2 = f1;
								if constexpr (!LM::is_eq(i)) f2 = f1 < 0 ? 0.0 : f1;
								const double delta = f2 - old;
								const double change = 0.5 * delta * delta * aii + delta * res;
								const bool revert = change > 1e-10;
								const bool upd = ract[i] && !done;
								rf[i] = (upd && !revert) ? f2 : old;
								improvement -= (upd && !revert) ? change : 0.0;
							}
						});
						improvement *= scale;
						iter += done ? 0 : 1;
						done = done || improvement < tol || iter >= itmax;
					}
					c_iter = iter;
					// ---- qfrc_constraint = J' f;  qacc = qacc_smooth + M^-1 qfrc_constraint;  Euler's acceleration + (M + h B)^-1 qfrc_constraint
					double x2[NV], y2[NV];
					sfor<NV>([&](auto I) { x2[I] = 0; y2[I] = 0; });
					sfor<NW>([&](auto W) {
						constexpr int d = LM::wdof(W);
						double sacc = 0;
						sfor<NR>([&](auto R) {
							constexpr int r = R;
							if constexpr (LM::jnt(r) == d) sacc += rsg[r] * rf[r];
							else if constexpr (LM::jnt2(r) == d) sacc += rc2[r < NE ? r : 0] * rf[r];
						});
						qfc[W] = sacc;
						x2[d] = sacc;
						y2[d] = sacc;
					});
					sfor<NV>([&](auto Ii) {
						constexpr int i = NV - 1 - Ii;
						sfor<NV>([&](auto A) {
							constexpr int a = A;
							if constexpr (a < i && Q::anc(a, i)) { x2[a] -= qM[i][a] * x2[i]; y2[a] -= qH[i][a] * y2[i]; }
						});
					});
					sfor<NV>([&](auto I) { x2[I] *= dinv[I]; y2[I] *= hinv[I]; });
					sfor<NV>([&](auto I) {
						constexpr int i = I;
						sfor<NV>([&](auto Ai) {
							constexpr int a = NV - 1 - Ai;
							if constexpr (a < i && Q::anc(a, i)) { x2[i] -= qM[i][a] * x2[a]; y2[i] -= qH[i][a] * y2[a]; }
						});
					});
					sfor<NV>([&](auto I) {
						const double qd = qaccd[I] + y2[I];
						qacc[I] += x2[I];
						qaccd[I] = damp_on ? qd : qacc[I];
					});
				}
			}

			if constexpr (XW) {
				// ---- (four wavefronts) mj_checkAcc on X: the verdict goes to the other three by mail -- bit 3 = some lane of the wavefront is bad, bit 2 = this
				// lane is -- while C integrates on the assumption that nobody is.  The second trip checks nothing and mails 0.
				bool bada = false;
				sfor<NV>([&](auto I) { bada |= bad_val(qacc[I]); });
				const bool retry = attempt == 0 && __builtin_amdgcn_ballot_w64(bada) != 0;  // (wave-uniform)
				if (retry) atomicAdd(s.nwarn + MJB_WARN_BADQACC, (bada && live) ? 1ull : 0ull);
				const double verdict = bada ? 12.0 : 8.0;
				lp[64 * XMAIL] = Pair{ retry ? verdict : 0.0, 0.0 };
				LE_PK(6);
				le_barrier();  // (B) C's new state and its verdicts on it
				LE_PK(7);
				if (!retry) {
					const int code = (int)lp[64 * MAIL].a;
					badp_next = (code & 2) != 0;
					badv_next = (code & 1) != 0;
					break;
				}
				sfor<NU>([&](auto I) { cn[I] = bada ? 0.0 : cn[I]; });
				time = bada ? 0.0 : time;
				wasreset = wasreset || bada;
				le_barrier();  // (R) C has put the old state back
				continue;
			}
			if constexpr (ROLE == LE_QUAD_C) {
				// ---- (four wavefronts) C: mj_Euler at once, on the assumption that X finds qacc good; the nine (qpos, qvel) pairs it read stay in registers
				// until X's verdict is in, and `time` waits for it too
				Pair sv[NV > 0 ? NV : 1];
				bool bp = false, bv = false;
				sfor<NV>([&](auto I) {
					Pair s2 = lp[64 * I];
					sv[I] = s2;
					s2.b += dt * qaccd[I];
					s2.a += dt * s2.b;
					lp[64 * I] = s2;
					bp |= bad_val(s2.a);  // the next step's mj_checkPos / mj_checkVel
					bv |= bad_val(s2.b);
				});
				badp_next = bp;
				badv_next = bv;
				lp[64 * MAIL] = Pair{ (double)((bp ? 2 : 0) | (bv ? 1 : 0)), 0.0 };
				LE_PK(6);
				le_barrier();  // (B) the new state and its verdicts; X's verdict on qacc
				LE_PK(7);
				const int xc = (int)lp[64 * XMAIL].a;
				if (!(__builtin_amdgcn_readfirstlane(xc) & 8)) break;  // (bit 3: X's ballot, the same in every lane and for all four wavefronts)
				// the rare path: some lane's qacc was bad.  The step is undone -- a bad lane gets mj_resetData's state, every other lane the pair it had -- and the
				// forward pass runs once more for the whole wavefront
				const bool bada = (xc & 4) != 0;
				sfor<NV>([&](auto I) {
					const double q0 = pins(tb[T::jnt_bodyid[I]].qpos0);
					lp[64 * I] = Pair{ bada ? q0 : sv[I].a, bada ? 0.0 : sv[I].b };
				});
				sfor<NU>([&](auto I) { cn[I] = bada ? 0.0 : cn[I]; });
				time = bada ? 0.0 : time;
				wasreset = wasreset || bada;
				le_barrier();  // (R) the old state is back: the second trip reads it
				continue;
			}
			// ================= mj_rnePostConstraint for the lane: the acceleration-stage sensors =================
			// Behind the qacc solve and ahead of mj_checkAcc's verdict, where the generic kernels run rne_post: a lane that verdict resets gets its sensordata
			// from the retry.  On sensor steps only (wave-uniform), selects only.  What is still there from the sweep: cdof in registers, (qpos, qvel) and each
			// body's bias force -- cinert cacc + cvel x* (cinert cvel), cacc without qacc, less the body's xfrc_applied wrench (XF) and its gravity compensation --
			// in LDS, cinert in LDS or cin[], the poses.  The pass adds what qacc contributes: dq[b] = sum over the dofs on b's path of cdof qacc, one more
			// root -> leaf accumulation, and cfrc_int[a] = sum over a's subtree of (bias force + cinert dq), with the gravity compensation put back (a passive
			// force: not part of cfrc_int in MuJoCo).  cvel and the bias part of cacc are formed again from cdof and qvel for the bodies between the root and
			// an accelerometer / framelinacc / frameangacc, and for no other.  A body at rest: cvel = 0, cacc = (0, -gravity), its own force its weight.
			if constexpr (SN::acc()) {
				constexpr bool wrench_at_rest = [] { for (int a = 1; a < NB; a++) if (!LD::needed(a) && SN::on(a, le_wrench_type)) return true; return false; }();
				static_assert(!XF || !wrench_at_rest, "lane = env kernel: the wrench table has no slot for a body at rest -- no xfrc build with a force / torque sensor on one (le_plan)");
				if (sens_on) {
					double pv[NB][6], pb[NB][6], dq[NB][6], fs[NB][6];  // cvel | cacc's bias part | cacc's qacc part | cfrc_int of a body with a force / torque sensor
					sfor<NB>([&](auto B) {
						constexpr int b = B;
						if constexpr (b > 0 && LD::needed(b)) {
							constexpr int p = T::body_parentid[b], j = T::body_jnt[b];
							constexpr bool prest = p == 0 || !LD::needed(p);
							constexpr bool wr = SN::above(b, le_wrench_type) || SN::below(b, le_wrench_type);
							constexpr bool kin = SN::above(b, le_accel_type) || (HW && wr);  // (HW: cvel of every body of the pass -- the stage's write to a joint's qvel, below)
							if constexpr (kin || wr) {
								for (int k = 0; k < 6; k++) dq[b][k] = prest ? 0.0 : dq[p][k];
								if constexpr (j >= 0) for (int k = 0; k < 6; k++) dq[b][k] += cdof[j][k] * qacc[j];
							}
							if constexpr (kin) {
								for (int k = 0; k < 6; k++) pv[b][k] = prest ? 0.0 : pv[p][k];
								for (int k = 0; k < 3; k++) { pb[b][k] = prest ? 0.0 : pb[p][k]; pb[b][3 + k] = prest ? -grav[k] : pb[p][3 + k]; }
								if constexpr (j >= 0) {
									const double qv = lp[64 * j].b;
									if constexpr (!prest) {  // (cdof_dot = cvel(parent) x cdof: zero under a parent at rest)
										double cdd[6];
										cross_motion(cdd, pv[p], cdof[j]);
										for (int k = 0; k < 6; k++) pb[b][k] += cdd[k] * qv;
										if constexpr (HW) {
											// (the generic kernels' hwsim_write puts a POSITION / VELOCITY joint's new qvel into the frame ahead of rne_post, which forms cdof_dot qvel
											//  with it -- cdof_dot and cvel still those of the old state.  Here that qvel waits for mj_Euler in hov[]: the difference goes into the qacc
											//  part, and with it into the forces)
											const HwSim MJB_AS4 &hw = Pq->hw;
											if (hw.le_tab[4 * j] >= 0) {
												const int method = hw.le_tab[4 * j + 1];
												if (method == MJB_HW_POSITION || method == MJB_HW_VELOCITY) {
													const double qn = seld(hw_wr, method == MJB_HW_POSITION ? 0.0 : hov[j], qv);
													for (int k = 0; k < 6; k++) dq[b][k] += cdd[k] * (qn - qv);
												}
											}
										}
									}
									for (int k = 0; k < 6; k++) pv[b][k] += cdof[j][k] * qv;
								}
							}
						}
					});
					// cfrc_int of the bodies that carry a force / torque sensor: the weights of the bodies at rest in the subtree, then every moving body's own force
					sfor<NB>([&](auto A) {
						constexpr int a = A;
						if constexpr (a > 0 && SN::on(a, le_wrench_type)) {
							for (int k = 0; k < 6; k++) fs[a][k] = 0;
							if constexpr (!LD::needed(a)) {
								sfor<NB>([&](auto Cq) {
									constexpr int c = Cq;
									if constexpr (c >= a && !LD::needed(c) && SN::under(c, a)) {
										double tq[3];
										cross3(tq, rw[c], grav);
										for (int k = 0; k < 3; k++) { fs[a][k] -= tq[k]; fs[a][3 + k] -= rw[c][3] * grav[k]; }
									}
								});
							}
						}
					});
					sfor<NB>([&](auto B) {
						constexpr int b = B;
						if constexpr (b > 0 && LD::needed(b) && SN::below(b, le_wrench_type)) {
							constexpr int q0 = LD::slot(b), c0 = LD::cin_slot(b);
							double ci[10], own[6];
							if constexpr (c0 >= 0) le_pairs_get<5>(ci, lp + 64 * c0);
							else for (int k = 0; k < 10; k++) ci[k] = cin[b][k];
							const Pair f0 = lp[64 * q0], f1 = lp[64 * (q0 + 1)], f2 = lp[64 * (q0 + 2)];
							mul_inert_vec(own, ci, dq[b]);
							own[0] += f0.a; own[1] += f0.b; own[2] += f1.a; own[3] += f1.b; own[4] += f2.a; own[5] += f2.b;
							if constexpr (LeGc<T>::on(b)) {  // (the sweep took (xd x F ; F), F = -gravity mass gravcomp, off the bias force; mass xd is cinert's [6 .. 8])
								const double sc = pas_on ? -tb[b].gravcomp : 0.0;
								double F[3], tq[3];
								for (int k = 0; k < 3; k++) F[k] = sc * grav[k];
								cross3(tq, ci + 6, F);
								for (int k = 0; k < 3; k++) { own[k] += tq[k]; own[3 + k] += ci[9] * F[k]; }
							}
							sfor<NB>([&](auto A) {
								constexpr int a = A;
								if constexpr (a > 0 && SN::on(a, le_wrench_type) && SN::under(b, a)) for (int k = 0; k < 6; k++) fs[a][k] += own[k];
							});
						}
					});
					sfor<T::NSENSOR>([&](auto S) {
						constexpr int i = S, type = T::sensor_type[i], adr = T::sensor_adr[i], b = SN::body(i);
						if constexpr (le_acc_type(type)) {
							double dif[3], R[9], w[3], out[3];
							sens_frame(S, dif, R);
							if constexpr (le_wrench_type(type)) {  // cfrc_int (torque ; force) about the root's origin, moved to the site and turned into its frame
								if constexpr (type == MJB_SENS_FORCE) for (int k = 0; k < 3; k++) w[k] = fs[b][3 + k];
								else {
									double cr[3];
									cross3(cr, dif, fs[b] + 3);
									for (int k = 0; k < 3; k++) w[k] = fs[b][k] - cr[k];
								}
								matTvec3(out, R, w);
							} else {  // mj_objectAcceleration: cacc moved to the object, + omega x v of its origin
								if constexpr (!LD::needed(b)) {
									for (int k = 0; k < 3; k++) w[k] = type == MJB_SENS_FRAMEANGACC ? 0.0 : -grav[k];
								} else if constexpr (type == MJB_SENS_FRAMEANGACC) {
									for (int k = 0; k < 3; k++) w[k] = pb[b][k] + dq[b][k];
								} else {
									double a6[6], ca[3], cv[3], vl[3], wv[3];
									for (int k = 0; k < 6; k++) a6[k] = pb[b][k] + dq[b][k];
									cross3(ca, dif, a6);
									cross3(cv, dif, pv[b]);
									for (int k = 0; k < 3; k++) vl[k] = pv[b][3 + k] - cv[k];
									cross3(wv, pv[b], vl);
									for (int k = 0; k < 3; k++) w[k] = a6[3 + k] - ca[k] + wv[k];
								}
								if constexpr (type == MJB_SENS_ACCELEROMETER) matTvec3(out, R, w);
								else for (int k = 0; k < 3; k++) out[k] = w[k];
							}
							const double cut = m.sensor_cutoff[i];
							for (int k = 0; k < 3; k++) sd[adr + k] = cut > 0 ? clampd(out[k], -cut, cut) : out[k];
						}
					});
				}
			}
			// ---- mj_checkAcc: a bad qacc resets the env and the forward pass runs once more (mj_step)
			if (attempt) break;
			bool bada = false;
			sfor<NV>([&](auto I) { bada |= bad_val(qacc[I]); });
			if (!__builtin_amdgcn_ballot_w64(bada)) break;  // (wave-uniform: the rare second trip recomputes every lane; the others get the same values)
			atomicAdd(s.nwarn + MJB_WARN_BADQACC, (bada && live) ? 1ull : 0ull);
			sfor<NV>([&](auto I) {
				const Pair o = lp[64 * I];
				const double oa = pinv(o.a), ob = pinv(o.b), q0 = pins(tb[T::jnt_bodyid[I]].qpos0);
				lp[64 * I] = Pair{ bada ? q0 : oa, bada ? 0.0 : ob };
			});
			sfor<NU>([&](auto I) { cn[I] = bada ? 0.0 : cn[I]; });
			if constexpr (NA > 0) sfor<NA>([&](auto I) { act[I] = bada ? 0.0 : act[I]; });
			if constexpr (NR > 0) sfor<NW>([&](auto W) { const double w = pinv(lim_ld(IC<LM::ws(W)>{})); lim_st(IC<LM::ws(W)>{}, bada ? 0.0 : w); });  // (the retry's warmstart is mj_resetData's)
			time = bada ? 0.0 : time;
			wasreset = wasreset || bada;
			if constexpr (HW) hw_bad = bada;
			if constexpr (DUO && DP) {
				lp[64 * MAIL] = Pair{ (double)(8 | (bada ? 4 : 0)), 0.0 };
				le_barrier();  // (B, retry) V runs its half again on the reset state
			}
		}
		if constexpr (POSEW) {
			if (last && (m.enableflags & MJB_ENBL_ENERGY)) s.energy[2 * ev] = en_pe;  // (C stores the kinetic half)
		}
		if constexpr (XW) {
			if (last) {  // (four wavefronts: qacc is X's)
				sfor<NV>([&](auto I) {
					s.qacc[ev * NV + I] = qacc[I];
					s.qacc_warmstart[ev * NV + I] = qacc[I];
				});
			}
		}
		if constexpr (DUO && !DP) {
			time += dt;
			continue;
		}

		if (last) {  // mj_advance's qacc_warmstart = qacc; mjData.energy of the launch's last step
			if constexpr (FM)
			sfor<NV>([&](auto I) {
				s.qacc[ev * NV + I] = qacc[I];
				s.qacc_warmstart[ev * NV + I] = qacc[I];
			});
			if (m.enableflags & MJB_ENBL_ENERGY) {
				if constexpr (EPOS) s.energy[2 * ev] = en_pe;
				s.energy[2 * ev + 1] = en_ke;
			}
			if constexpr (NR > 0) {  // what the launch leaves of its last constraint stage (efc_* are not written): qfrc_constraint | nefc | solver_iter
				double *const co = Pq->le_con;
				if (co) {
					double *const o = co + ev * (size_t)(NV + 2);
					sfor<NV>([&](auto I) {
						constexpr int j = I;
						double v = 0;
						if constexpr (LM::in_rows(j)) v = qfc[LM::widx(j)];
						o[j] = v;
					});
					o[NV] = (double)c_nefc;
					o[NV + 1] = (double)c_iter;
				}
			}
		}
		if constexpr (ROLE == LE_QUAD_C) {  // (four wavefronts: C has integrated inside the loop, ahead of X's verdict)
			time += dt;
			continue;
		}
		// ================= A16 mj_Euler =================
		badp_next = badv_next = false;
		sfor<NV>([&](auto I) {
			Pair s2 = lp[64 * I];
			if constexpr (HW) {  // what the stage wrote to the state: Euler integrates from it
				const HwSim MJB_AS4 &hw = Pq->hw;
				if (hw.le_tab[4 * I] >= 0) {
					const int method = hw.le_tab[4 * I + 1];
					if (method == MJB_HW_POSITION) {
						s2.a = seld(hw_wr, hov[I], s2.a);
						s2.b = seld(hw_wr, 0.0, s2.b);
					} else if (method == MJB_HW_VELOCITY) s2.b = seld(hw_wr, hov[I], s2.b);
				}
			}
			s2.b += dt * qaccd[I];
			s2.a += dt * s2.b;
			lp[64 * I] = s2;
			badp_next |= bad_val(s2.a);  // the next step's mj_checkPos / mj_checkVel
			badv_next |= bad_val(s2.b);
		});
		if constexpr (NA > 0) sfor<NA>([&](auto I) { act[I] = actn[I]; });
		if constexpr (NR > 0) sfor<NW>([&](auto W) { lim_st(IC<LM::ws(W)>{}, qacc[LM::wdof(W)]); });  // mj_advance: qacc_warmstart = qacc
		time += dt;
		if constexpr (DUO && DP) {
			lp[64 * MAIL] = Pair{ (double)((badp_next ? 2 : 0) | (badv_next ? 1 : 0)), 0.0 };
			LE_PK(6);
			le_barrier();  // (B) the new state and its verdicts
			LE_PK(7);
		}
	}
#ifdef MJB_LE_PROBE
	if (env_raw == env_lo && QUAD) P->s.sensordata[32 + (ROLE - LE_QUAD_O)] = (double)pk_acc[8] / nsteps;  // (behind X's eight, in env 1's sensordata)
	if (env_raw == env_lo) for (int k = 0; k < 8; k++) P->s.sensordata[(ROLE == LE_PIPE_V || ROLE == LE_DUO_V || ROLE == LE_TRIO_C || ROLE == LE_QUAD_C ? 8 : (ROLE == LE_TRIO_V || ROLE == LE_QUAD_V ? 16 : (ROLE == LE_QUAD_X ? 24 : 0))) + k] = (double)pk_acc[k] / nsteps;
#endif

	// ---- the launch's state back to HBM (store_state of the generic kernels; sensordata went out from the last step)
	{  // (tail lanes store the last env's state a second time)
		const DevState MJB_AS4 &s = P->s;
		if constexpr (DP) {
			sfor<NV>([&](auto I) {
				const Pair s2 = lp[64 * I];
				s.qpos[ev * NV + I] = s2.a;
				s.qvel[ev * NV + I] = s2.b;
			});
			s.time[ev] = time;
			if constexpr (NA > 0) sfor<NA>([&](auto I) { s.act[ev * NA + I] = act[I]; });
		}
		if constexpr (DV) {
			sfor<NU>([&](auto I) { s.ctrlnoise[ev * NU + I] = cn[I]; });
			if (nz_on) sfor<NU>([&](auto I) { s.ctrl[ev * NU + I] = cn[I]; });
			else if (__builtin_amdgcn_ballot_w64(wasreset)) sfor<NU>([&](auto I) { const double c = pinv(s.ctrl[ev * NU + I]); s.ctrl[ev * NU + I] = wasreset ? 0.0 : c; });
		}
		if constexpr (XF) {
			// mj_resetData zeroed the env's xfrc_applied: the canonical rows (every body's) and the table's column, under the wave-uniform test -- every
			// lane of such a wavefront stores, a lane that was not reset what it loaded
			if (__builtin_amdgcn_ballot_w64(wasreset)) {
				double *const xa = s.xfrc_applied + ev * (size_t)(6 * NB);
				sfor<6 * NB>([&](auto I) { const double c = pinv(xa[I]); xa[I] = seld(wasreset, 0.0, c); });
				double *const xt = s.le_xfrc + ev;
				const size_t ne = (size_t)s.nenv;
				sfor<6 * XS6::n>([&](auto I) { const double c = pinv(xt[(size_t)I * ne]); xt[(size_t)I * ne] = seld(wasreset, 0.0, c); });
			}
		}
	}
}

// LDS of a DUO block: the solo layout under a budget reduced by the exchange slots, then those
template <class T, int LP> constexpr int duo_bytes() { return le_duo_slots(T::NV, Lds<T, LP>::nmov(), LP) * LE_SLOT_BYTES; }

// ... of a pipelined DUO block: every needed body's cinert, the pose ring, the exchange slots
template <class T> constexpr int duo2_bytes() { return le_duo2_slots(T::NV, Lds<T, 0>::nmov()) * LE_SLOT_BYTES; }
// ... of a trio block: the same with the deeper ring and a (sin, cos) slot per body
template <class T> constexpr int trio_bytes() { return le_trio_slots(T::NV, Lds<T, 0>::nmov(), T::NBODY) * LE_SLOT_BYTES; }
// ... and of a quartet block: the trio's layout, then O's quaternion ring (2 x 4 pair slots), C's cdof ring (2 x 3) and X's mail slot
template <class T> constexpr int quartet_bytes() { return le_quartet_slots(T::NV, Lds<T, 0>::nmov(), T::NBODY) * LE_SLOT_BYTES; }
template <class T, int LP>
DEVI void lane_env_duo2(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0, const int env_lo, const int env_hi,
                        unsigned char *const smem_le)
{
	if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) < 64) lane_env_body<T, LP, LE_PIPE_P>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else lane_env_body<T, LP, LE_PIPE_V>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

// the TRIO: wavefront 0 = the pose chain, 1 = inertias / factors / solves / Euler, 2 = velocities and forces (blockDim.x = 192; the pipelined duo's LDS layout)
template <class T, int LP>
DEVI void lane_env_trio(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0, const int env_lo, const int env_hi,
                        unsigned char *const smem_le)
{
	const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
	if (w == 0) lane_env_body<T, LP, LE_TRIO_P>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else if (w == 1) lane_env_body<T, LP, LE_TRIO_C>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else lane_env_body<T, LP, LE_TRIO_V>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

// the QUARTET: wavefront 0 = the orientation chain, 1 = frames and positions, 2 = inertias / factors / solves / Euler, 3 = velocities and forces (blockDim.x = 256)
template <class T, int LP>
DEVI void lane_env_quartet(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0, const int env_lo, const int env_hi,
                           unsigned char *const smem_le)
{
	const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
	if (w == 0) lane_env_body<T, LP, LE_QUAD_O>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else if (w == 1) lane_env_body<T, LP, LE_QUAD_X>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else if (w == 2) lane_env_body<T, LP, LE_QUAD_C>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else lane_env_body<T, LP, LE_QUAD_V>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

// the DUO kernel's body: wavefront 0 of the block takes the position half, wavefront 1 the velocity half (blockDim.x = 128)
template <class T, int LP>
DEVI void lane_env_duo(const KernelParams MJB_AS4 *__restrict__ P, const int nsteps, const unsigned int step0, const int env_lo, const int env_hi,
                       unsigned char *const smem_le)
{
	if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) < 64) lane_env_body<T, LP, LE_DUO_P>(P, nsteps, step0, env_lo, env_hi, smem_le);
	else lane_env_body<T, LP, LE_DUO_V>(P, nsteps, step0, env_lo, env_hi, smem_le);
}

}  // namespace mjb_le
