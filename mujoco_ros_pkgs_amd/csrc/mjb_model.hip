// mjb_model.hip — the model compiler: mjb_compile turns a model description into an mjb_model (validated host copy, derived tables, frame
// layouts, kernel classification), in the named stages listed above mjb_compile; the getters that need the model only; the host mirror of
// mj_setConst (mjb_derive_mass_params); and the error string of the whole C-ABI.  Host code throughout: it is built by hipcc for the types of
// mjb_dev.h (FrameLayout), calls no HIP runtime function and defines no kernel.  Batches, launches and transfers live in mjb_api.hip.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "mjb_model.h"

namespace {
thread_local std::string g_err;
}

int fail(int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_err = buf;
	return code;
}
void clear_error() { g_err.clear(); }

const FieldInfo kFields[MJB_F_COUNT] = {
#define MJB_DS(name, rows, cols) { #name, #rows, #cols, 0 },
#define MJB_DD(name, rows, cols) { #name, #rows, #cols, 1 },
#define MJB_DD2(name, rows, cols) { #name, #rows, #cols, 2 },
#define MJB_DI(name, rows, cols) { #name, #rows, #cols, 3 },
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
};

namespace {
int FrameLayout::*const kFieldSlot[MJB_F_COUNT] = {
#define MJB_DS(name, rows, cols) &FrameLayout::name,
#define MJB_DD(name, rows, cols) &FrameLayout::name,
#define MJB_DD2(name, rows, cols) &FrameLayout::name,
#define MJB_DI(name, rows, cols) &FrameLayout::name,
#include "../../include/mjb_data_fields.def"
#undef MJB_DS
#undef MJB_DD
#undef MJB_DD2
#undef MJB_DI
};
}  // namespace
int &field_slot(FrameLayout &L, int i) { return L.*kFieldSlot[i]; }
int field_slot(const FrameLayout &L, int i) { return L.*kFieldSlot[i]; }

int size_by_name(const mjb_model_desc &d, const char *n)
{
#define MJB_SIZE(name) if (!strcmp(n, #name)) return d.name;
#define MJB_OPT_I(name)
#define MJB_OPT_D(name, k)
#define MJB_ARR_I(name, rows, cols)
#define MJB_ARR_D(name, rows, cols)
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	if (!strcmp(n, "one")) return 1;
	return atoi(n);
}

namespace {

// an acceleration-stage sensor needs mj_rnePostConstraint (cacc / cfrc_int / cfrc_ext)
bool needs_rnepost(const mjb_model_desc &d)
{
	for (int i = 0; i < d.nsensor; i++) {
		const int t = d.sensor_type[i];
		if (t == MJB_SENS_TOUCH || t == MJB_SENS_ACCELEROMETER || t == MJB_SENS_FORCE || t == MJB_SENS_TORQUE ||
		    t == MJB_SENS_FRAMELINACC || t == MJB_SENS_FRAMEANGACC)
			return true;
	}
	return false;
}

// elements of data field idx as mjb_get / mjb_field_size see it: the declared rows x cols, less the fields this model has no use for
int field_elements(const mjb_model &M, int idx)
{
	const mjb_model_desc &d = M.h;
	if (idx == MJB_F_efc_AR) return 0;  // (the PGS kernel keeps each row of AR in its lane's registers)
	if (idx == MJB_F_efc_frictionloss && M.nfriction == 0) return 0;  // no dry-friction rows in this model
	if (idx == MJB_F_efc_B && d.solver != MJB_SOL_PGS) return 0;  // the primal solvers need no J M^-1
	return size_by_name(d, kFields[idx].rows) * size_by_name(d, kFields[idx].cols);
}

// Frame layout.  compact == false: every field owns its storage (what mjb_forward / mjb_step1 dump and mjb_get
// reads).  compact == true (fused mjb_step only): xfrc_applied is absent and fields whose lifetimes never
// overlap inside one step share storage --
//   region A: kinloc (kinematics)  |  crb + crbbuf (crb)  |  cacc + cfrc_body (rne)  |  eulerx (euler)
//   region B: ximat (kinematics -> comPos)  |  cvel + cdof_dot (comVel -> rne / vel sensors)
// which brings the Franka frame from 12.6 KB to 9.3 KB, i.e. from 12 to 16 resident envs per CU.
//
// compact AND constrained (nefcmax > 0) -- "lean": the fused step builds the constraint rows AFTER the velocity stage (nothing
// between collision and the solver reads them; the kernel defers make_constraint whenever it runs on this layout), so
//   * efc_J overlays everything that is dead by then (region U): regions A and B, cinert, geom_xpos / geom_xmat, xanchor / xaxis,
//     site_xquat and -- without equalities -- xmat / xquat   [only when no sensor needs rne_post, which re-reads them];
//   * row bookkeeping shrinks to what the solver reads: efc_pos / efc_margin / efc_KBIP / efc_vel are gone (efc_aref holds
//     K imp (pos - margin) and efc_b the damping gain until reference_constraint folds them into aref), efc_D is gone for PGS
//     (1 / R on the fly) and efc_R for the primal solvers;
//   * contact_solref / contact_solimp are gone (make_constraint reads the pair record the contact came from);
//   * the PGS triangle scratch sits on the dead contact arrays, the box - box clipping scratch at the start of U.
// jrows_req > 0: rows of efc_J the fused frame of kernel variant 4 holds (choose_layout picks it); 0 = the default
//
// Reads of the model: the description, nfriction, need_rnepost, pair_i, site_act and slot.  Writes nothing but the layout it returns.
FrameLayout compute_layout(const mjb_model &M, bool compact, int jrows_req = 0)
{
	const mjb_model_desc &d = M.h;
	FrameLayout L{};
	int off = 0, ioff = 0, nstate = 0;
	int idx = 0;
	bool body_sensor = false;
	for (int i = 0; i < d.nsensor; i++)
		if (d.sensor_objtype[i] == MJB_OBJ_BODY || d.sensor_reftype[i] == MJB_OBJ_BODY) body_sensor = true;
	const bool alias_b = compact && !body_sensor;
	const bool need_post = M.need_rnepost != 0;
	const bool lean = compact && d.nefcmax > 0;
	const bool u_ok = lean && !need_post;
	const bool primal = d.solver == MJB_SOL_NEWTON || d.solver == MJB_SOL_CG;
	const bool ell_con = d.cone == MJB_CONE_ELLIPTIC && d.nconmax > 0;
	// kernel variant 4 (Newton, more than 128 rows of capacity), fused frame: the first 64 rows of efc_J only; an env-step with
	// more rows keeps J in the env's block of DevState::efc_Jg (config 5 never has: what lets two of its envs share a CU's LDS)
	int jrows = d.nefcmax;
	if (compact && d.solver == MJB_SOL_NEWTON && d.nefcmax > 128 && !M.slot) {
		jrows = jrows_req > 0 ? std::max(4, std::min(128, jrows_req)) : 64;
		if (const char *v = getenv("MJB_DEBUG_JROWS")) jrows = std::max(4, std::min(64, atoi(v)));  // test knob: force the HBM path
	}
	L.jrows = jrows;
	std::vector<int> u_members;  // field ids overlaid by efc_J, in placement order
	// "X layout" -- lean frames of the Newton kernels (nv <= 32: M lives in registers inside the solver).  One region X is shared by
	// three generations of data:
	//   X = [ D | R ],  D = cdof | qM | qLD | qLDiagInv | contact dist / pos / frame / includemargin   (dead once the solver has
	//                       gathered its rows of M: nothing after make_constraint / fwd_acceleration reads them)
	//                   R = position / velocity-stage scratch (regions A, B, the U members)           (dead at make_constraint)
	//   make_constraint .. solver:   efc_J | efc_D | efc_aref | efc_b | efc_force at the END of X
	//   fwd_acceleration, Euler:     the dense-triangle scratch (tri | solvescr | eulerx) right below efc_J, inside R
	//   solver only:                 nwt_H | nwt_vec | nwt_row | nwt_hc from the START of X (over D and the head of R)
	// (a jointlimitfrc / tendonlimitfrc sensor reads efc_force of its row after the solve: such a model keeps every row array whole in the frame)
	bool row_sensor = false;
	for (int i = 0; i < d.nsensor; i++) row_sensor = row_sensor || d.sensor_type[i] == MJB_SENS_JOINTLIMITFRC || d.sensor_type[i] == MJB_SENS_TENDONLIMITFRC;
	const bool xl = u_ok && !row_sensor && d.solver == MJB_SOL_NEWTON && d.nv <= 32;
	// ... and, when the frame holds only `jrows` rows of efc_J (kernel variant 4), every other per-row array is capped at the same
	// count: an env-step with more rows keeps all of its row data in the env's block of DevState::efc_Jg (mjb_dev.h, RowBlock).
	// Config 5: 53.0 -> 40.9 KB = four envs per CU, one per SIMD.
	const int rcap = (xl && jrows < d.nefcmax) ? jrows : d.nefcmax;
	L.rcap = rcap;
	L.hcrow = (rcap < d.nefcmax) ? 1 : 0;
	std::vector<int> d_members, p2_members;
	int fsize[MJB_F_COUNT];
	for (const FieldInfo &fi : kFields) {
		int n = field_elements(M, idx);
		// (nv <= 16: the PGS kernel solves for its row of B in registers; the field only exists in the full layout, for mjb_get)
		const bool no_B = idx == MJB_F_efc_B && n > 0 && compact && d.nv <= 16 && !(d.cone == MJB_CONE_ELLIPTIC && d.nconmax > 0);
		if ((idx == MJB_F_cfrc_int || idx == MJB_F_cfrc_ext) && !need_post) n = 0;  // computed only when a sensor needs them
		// (with rne_post the true cacc is written between fwd_acceleration and Euler, whose rhs shares region A)
		const bool in_a = compact && (idx == MJB_F_crb || (idx == MJB_F_cacc && !need_post) || idx == MJB_F_cfrc_body);
		const bool in_b = alias_b && (idx == MJB_F_ximat || idx == MJB_F_cvel || idx == MJB_F_cdof_dot);
		if (compact && idx == MJB_F_xfrc_applied) n = 0;
		if (idx == MJB_F_efc_J && n > 0) n = jrows * d.nv;
		if (rcap < d.nefcmax && n > 0 && (idx == MJB_F_efc_D || idx == MJB_F_efc_aref || idx == MJB_F_efc_b || idx == MJB_F_efc_force ||
		                                  idx == MJB_F_efc_frictionloss || idx == MJB_F_efc_type || idx == MJB_F_efc_id))
			n = n / d.nefcmax * rcap;
		fsize[idx] = n;
		const bool gone = lean && (idx == MJB_F_efc_pos || idx == MJB_F_efc_margin || idx == MJB_F_efc_KBIP || idx == MJB_F_efc_vel ||
		                           (idx == MJB_F_efc_D && d.solver == MJB_SOL_PGS && !ell_con) || (idx == MJB_F_efc_R && primal) ||
		                           idx == MJB_F_contact_solref || idx == MJB_F_contact_solimp);
		const bool in_u = u_ok && (idx == MJB_F_efc_J || idx == MJB_F_cinert || idx == MJB_F_geom_xpos || idx == MJB_F_geom_xmat ||
		                           idx == MJB_F_xanchor || idx == MJB_F_xaxis || idx == MJB_F_site_xquat ||
		                           (d.neq == 0 && (idx == MJB_F_xmat || idx == MJB_F_xquat)));
		if (gone) {
			field_slot(L, idx) = -1;  // kernels test the offset
			idx++;
			continue;
		}
		if (xl && (idx == MJB_F_cdof || idx == MJB_F_qM || idx == MJB_F_qLD || idx == MJB_F_qLDiagInv || idx == MJB_F_contact_dist ||
		           idx == MJB_F_contact_pos || idx == MJB_F_contact_frame || idx == MJB_F_contact_includemargin)) {
			d_members.push_back(idx);
			field_slot(L, idx) = -1;  // placed below
			idx++;
			continue;
		}
		if (xl && (idx == MJB_F_efc_D || idx == MJB_F_efc_aref || idx == MJB_F_efc_b || idx == MJB_F_efc_force || idx == MJB_F_efc_frictionloss)) {
			p2_members.push_back(idx);
			field_slot(L, idx) = -1;  // placed below
			idx++;
			continue;
		}
		if (in_u && !in_a && !in_b) {
			if (idx != MJB_F_efc_J) u_members.push_back(idx);
			field_slot(L, idx) = -1;  // placed below
			idx++;
			continue;
		}
		if (no_B) {
			field_slot(L, idx) = -1;  // kernels test L.efc_B >= 0
			idx++;
			continue;
		}
		if (fi.kind == 3) {
			field_slot(L, idx) = ioff;
			ioff += n;
		} else if (in_a || in_b) {
			field_slot(L, idx) = -1;  // placed below
		} else {
			field_slot(L, idx) = off;
			off += n;
			if (fi.kind == 0) nstate = off;
		}
		idx++;
	}
	const bool newton = d.nefcmax > 0 && (d.solver == MJB_SOL_NEWTON || d.solver == MJB_SOL_CG);  // primal solvers
	const int off_before_nwt = off;
	L.nwt_M = off;
	off += (newton && d.nv > 32) ? d.nv * d.nv : 0;  // (nv <= 32: the solver keeps row `lane` of M in registers, host table M_sym)
	L.nwt_H = off;
	// (nv <= 32: the packed lower triangle + one dump slot, mjb_constraint.h MJB_HPACK; 16 < nv: at least chol_schur16's 16 x 17 scratch)
	off += newton ? (d.nv <= 32 ? std::max(d.nv * (d.nv + 1) / 2 + 1, d.nv > 16 ? 272 : 0) : d.nv * d.nv) : 0;
	L.nwt_vec = off;
	off += newton ? 5 * d.nv : 0;  // qacc | M qacc | grad | search | (CG: M^-1 grad)
	L.nwt_row = off;
	off += newton ? 3 * rcap : 0;
	L.nwt_hc = off;
	// cone blocks: the primal solvers size them by the model's largest contact dimension (config 5: condim 4 -> 16 doubles instead
	// of 36; at least 10, the line-search constants a contact parks there); PGS keeps its 6 x 6 blocks of AR
	L.hcd = 6;
	L.hcs = 36;
	if (newton) {
		int maxdim = 1;
		for (int p = 0; p < d.ncollpair; p++) maxdim = std::max(maxdim, M.pair_i[(size_t)8 * p + 4]);
		L.hcd = std::min(6, maxdim);
		// (blocks laid out by row on a frame with more than one row per lane: the line search parks its ten constants per contact in the contact's block, and a
		//  contact of dimension 3 owns 3 x hcd doubles -- nine at hcd = 3.  Round 5, tools/wide_dim3_check.py: the neighbour's first constant was overwritten)
		if (L.hcrow && rcap > 64 && L.hcd < 4) L.hcd = 4;
		L.hcs = std::max(L.hcd * L.hcd, 10);
	}
	// (hcrow: a contact's block sits at hcd * its first row -- rows, not contacts, bound the solver that runs on this frame)
	off += ((newton || (d.nefcmax > 0 && d.solver == MJB_SOL_PGS)) && d.cone == MJB_CONE_ELLIPTIC) ? (L.hcrow ? L.hcd * rcap : L.hcs * d.nconmax) : 0;  // (PGS: the contacts' blocks of AR)
	const int n_nwt = off - off_before_nwt;  // nwt_M | nwt_H | nwt_vec | nwt_row | nwt_hc
	if (xl) off = off_before_nwt;            // (X layout: they overlay the head of X, placed below)
	L.gravity = off;
	off += 3;
	// (lean frame: collision takes the mixed friction from the pair record, or from the per-env override in HBM)
	L.gfriction = lean ? -1 : off;
	off += (d.nconmax > 0 && !lean) ? 3 * d.ngeom : 0;
	L.eqparam = off;
	off += 19 * d.neq;
	L.cwrench = off;
	off += need_post ? 6 * d.nconmax : 0;
	L.MhB = off;
	off += d.nM;
	L.qH = lean ? L.MhB : off;  // (lean frame: factorised in place -- nothing reads M + h B after its factor exists)
	off += lean ? 0 : d.nM;
	L.qHdi = off;
	off += d.nv;
	L.rk = d.integrator == MJB_INT_RK4 ? off : -1;  // (persistent across the evaluations of one step)
	off += d.integrator == MJB_INT_RK4 ? d.nq + 4 * d.nv + d.nsensordata + 1 + 2 * d.na : 0;  // X0 | sums | warmstart | the step's sensordata | t0 | act0 | sum B act_dot
	L.act_mom = off;  // (alive from the transmission stage to actuation, across the overlays of every layout: own storage)
	off += (int)M.site_act.size() * d.nv;
	// transient scratch of the constrained kernels: ntri doubles for the packed dense triangle of the L'DL factor (nv <= 16, PGS:
	// the J M^-1 rows; 16 < nv <= 32: the M^-1 solves of fwd_acceleration / Euler, solve_tri32), 128 for the box - box narrow phase
	const int ntri = d.nefcmax <= 0 ? 0 : ((d.nv <= 16 && d.solver == MJB_SOL_PGS) ? 128 : ((d.nv > 16 && d.nv <= 32) ? 496 : 0));
	const int nbb = d.nconmax > 0 ? 216 : 0;  // (MJB_BBSCR of mjb_constraint.h)
	const int n_kin = 7 * d.nbody, n_crb = 10 * d.nbody, n_buf = 6 * d.nv < 32 ? 32 : 6 * d.nv, n_c6 = 6 * d.nbody;  // (crbbuf doubles as the 32-double pivot-row scratch of the dense factor)
	if (compact && xl) {
		const int x0 = off;
		for (int id : d_members) {
			field_slot(L, id) = off;
			off += fsize[id];
		}
		const int a0 = off;  // start of R
		L.kinloc = a0;
		L.crb = a0;
		L.crbbuf = a0 + n_crb;
		L.cacc = a0;
		L.cfrc_body = a0 + n_c6;
		L.bbscr = a0;
		{
			int sz = n_kin;
			if (nbb > sz) sz = nbb;
			if (n_crb + n_buf > sz) sz = n_crb + n_buf;
			if (2 * n_c6 > sz) sz = 2 * n_c6;
			if (d.nv > sz) sz = d.nv;
			off += sz;
		}
		if (alias_b) {
			const int b0 = off;
			L.ximat = b0;
			L.cvel = b0;
			L.cdof_dot = b0 + n_c6;
			int szb = 9 * d.nbody;
			if (n_c6 + 6 * d.nv > szb) szb = n_c6 + 6 * d.nv;
			off += szb;
		}
		for (int id : u_members) {
			field_slot(L, id) = off;
			off += fsize[id];
		}
		int n_p2 = fsize[MJB_F_efc_J];
		for (int id : p2_members) n_p2 += fsize[id];
		const int n_scr = ntri + 32 + d.nv;
		// (the triangle scratch of fwd_acceleration / Euler: on the contact arrays at the end of D when they are large enough --
		//  dist | pos | frame | includemargin are contiguous and dead after make_constraint, while qM / qLD next to them are still
		//  read -- otherwise at the start of R)
		const bool tri_in_d = 14 * d.nconmax >= n_scr;
		int jstart = std::max(x0 + n_nwt, tri_in_d ? a0 : a0 + n_scr);  // the solver's arrays and the triangle scratch both end below efc_J, which never reaches into D (make_constraint reads cdof and the contacts while it writes J)
		if (jstart + n_p2 > off) off = jstart + n_p2;
		jstart = off - n_p2;                             // ... which sits at the end of X
		L.efc_J = jstart;
		{
			int o = jstart + fsize[MJB_F_efc_J];
			for (int id : p2_members) {
				field_slot(L, id) = o;
				o += fsize[id];
			}
		}
		L.tri = tri_in_d ? L.contact_dist : jstart - n_scr;
		L.solvescr = L.tri + ntri;
		L.eulerx = L.solvescr + 32;
		{
			const int shift = x0 - off_before_nwt;
			L.nwt_M += shift; L.nwt_H += shift; L.nwt_vec += shift; L.nwt_row += shift; L.nwt_hc += shift;
		}
	} else if (compact) {
		const int a0 = off;
		L.kinloc = a0;
		L.crb = a0;
		L.crbbuf = a0 + n_crb;
		if (!need_post) L.cacc = a0;
		L.cfrc_body = a0 + n_c6;
		L.eulerx = a0;
		L.tri = a0 + 32;  // (alive inside the PGS stage / the M^-1 solves: cacc / cfrc_body are dead by then; Euler's vector sits below it)
		L.bbscr = a0;
		L.solvescr = L.crbbuf;
		int sz = n_kin;
		if (ntri > 0 && sz < 32 + ntri) sz = 32 + ntri;
		if (nbb > sz) sz = nbb;
		if (n_crb + n_buf > sz) sz = n_crb + n_buf;
		if (2 * n_c6 > sz) sz = 2 * n_c6;
		if (d.nv > sz) sz = d.nv;
		off += sz;
		if (alias_b) {
			const int b0 = off;
			L.ximat = b0;
			L.cvel = b0;
			L.cdof_dot = b0 + n_c6;
			int szb = 9 * d.nbody;
			if (n_c6 + 6 * d.nv > szb) szb = n_c6 + 6 * d.nv;
			off += szb;
		}
		if (u_ok) {
			for (int id : u_members) {
				field_slot(L, id) = off;
				off += fsize[id];
			}
			L.efc_J = a0;
			if (off - a0 < fsize[MJB_F_efc_J]) off = a0 + fsize[MJB_F_efc_J];
			// (efc_J is alive from the end of the velocity stage to the end of the solver: what runs in between -- the dense
			//  M^-1 solve of fwd_acceleration, the PGS stage's triangle -- takes its scratch, and Euler its right-hand side, from
			//  the contact arrays nobody reads after make_constraint: dist | pos | frame | includemargin are contiguous, 14
			//  doubles per contact; friction, which the elliptic solvers read, stays intact)
			const int late = ntri + 32 + d.nv;
			int ls = off;
			if (14 * d.nconmax >= late) ls = L.contact_dist;
			else off += late;
			L.tri = ls;
			L.solvescr = ls + ntri;
			L.eulerx = L.solvescr + 32;
		}
	} else {
		L.kinloc = off;
		off += n_kin;
		L.crbbuf = off;
		off += n_buf;
		L.eulerx = off;
		off += d.nv;
		L.solvescr = L.crbbuf;
		L.tri = off;
		off += ntri;
		L.bbscr = off;
		off += nbb;
	}
	if (off & 1) off++;
	L.ndouble = off;
	L.iscratch = ioff;
	{
		int a = d.ncollpair, b = d.neq + d.nv + d.njnt + 2 * d.ntendon + d.nconmax;
		if (newton && rcap > a) a = rcap;  // (the primal solvers park one int of row metadata per constraint row here)
		ioff += a > b ? a : b;
	}
	L.dadr = ioff;
	ioff += (d.nefcmax > 0 && d.nv <= 16) ? 64 : 0;
	L.nint = (ioff + 1) & ~1;
	L.nstate = nstate;
	return L;
}

// development knob MJB_DEBUG_LAYOUT: every field's offset in the fused frame, sorted (doubles, then ints)
void dump_layout(const FrameLayout &L)
{
	std::vector<std::pair<int, std::string>> dd, ii;
	for (int i = 0; i < MJB_F_COUNT; i++)
		if (field_slot(L, i) >= 0) (kFields[i].kind == 3 ? ii : dd).push_back({ field_slot(L, i), kFields[i].name });
	const std::pair<int, const char *> extra[] = { { L.MhB, "MhB" }, { L.qH, "qH" }, { L.qHdi, "qHdi" }, { L.nwt_M, "nwt_M" }, { L.nwt_H, "nwt_H" },
		{ L.nwt_vec, "nwt_vec" }, { L.nwt_row, "nwt_row" }, { L.nwt_hc, "nwt_hc" }, { L.gravity, "gravity" }, { L.gfriction, "gfriction" },
		{ L.eqparam, "eqparam" }, { L.cwrench, "cwrench" }, { L.kinloc, "kinloc" }, { L.crbbuf, "crbbuf" }, { L.eulerx, "eulerx" },
		{ L.tri, "tri" }, { L.solvescr, "solvescr" }, { L.bbscr, "bbscr" }, { L.act_mom, "act_mom" } };
	for (auto &x : extra)
		if (x.first >= 0) dd.push_back({ x.first, std::string("*") + x.second });
	ii.push_back({ L.iscratch, "*iscratch" });
	ii.push_back({ L.dadr, "*dadr" });
	std::sort(dd.begin(), dd.end());
	std::sort(ii.begin(), ii.end());
	fprintf(stderr, "mjb fused layout: %d bytes, jrows %d, hcs %d, hcd %d, ndouble %d, nint %d, nstate %d\n doubles:", mjb_layout_bytes(L), L.jrows, L.hcs,
	        L.hcd, L.ndouble, L.nint, L.nstate);
	for (auto &x : dd) fprintf(stderr, " %s@%d", x.second.c_str(), x.first);
	fprintf(stderr, "\n ints:");
	for (auto &x : ii) fprintf(stderr, " %s@%d", x.second.c_str(), x.first);
	fprintf(stderr, "\n");
}

// The fused frames of a model: the default one, and the wide one of kernel variant 4 (== the default one when the model has none).
struct FusedLayouts {
	FrameLayout Lc, Lw;
	bool has_wide;
};

// The fused frame of kernel variant 4 (Newton, capacity > 128 rows) keeps only `jrows` rows of efc_J in LDS (the rest, and all of J
// of an env-step with more rows, live in DevState::efc_Jg).  Residency beats the price of the HBM path (measured 10 % on the steps
// that take it): pick the row count that lets the most envs share a CU's LDS, and the largest such.
FusedLayouts choose_fused_layouts(const mjb_model &M)
{
	const mjb_model_desc &d = M.h;
	const bool dump = getenv("MJB_DEBUG_LAYOUT") != nullptr;  // development knob
	const bool variant4 = d.solver == MJB_SOL_NEWTON && d.nefcmax > 128 && !M.slot;  // (the row-slot kernels: every row in the fused frame)
	FusedLayouts f{ compute_layout(M, true), {}, false };
	if (variant4 && getenv("MJB_DEBUG_FRAME_ROWS")) f.Lc = compute_layout(M, true, atoi(getenv("MJB_DEBUG_FRAME_ROWS")));  // measurement knob: rows of J in THE fused frame
	else if (variant4 && !getenv("MJB_DEBUG_JROWS")) {
		auto occ = [&](int jr) {
			// (gfx950 hands out its 160 KB of LDS in 128 granules of 1280 bytes -- measured: a 54000-byte frame runs two to a CU, a
			//  50272-byte one three; 512-register kernels: one wave per SIMD, four envs per CU at most)
			return std::min(4, 128 / ((mjb_layout_bytes(compute_layout(M, true, jr)) + 1279) / 1280));
		};
		const int best = occ(16);
		int pick = 64;
		if (best > occ(64))
			for (pick = 60; pick > 16 && occ(pick) < best; pick -= 4) {}
		f.Lc = compute_layout(M, true, pick);
		// the wide frame: up to 128 rows (two per lane) -- the largest multiple of four with which THREE frames share a CU's LDS when at least
		// 96 rows do (the power grasp of config 5: p99 of nefc = 111, 112 rows fit three times; an env-step beyond them takes the HBM row block),
		// else 128 when two fit
		int wrows = 128;
		for (int jr = 124; jr >= 96; jr -= 4)
			if (occ(jr) >= 3) { wrows = jr; break; }
		if (const char *v = getenv("MJB_WIDE_ROWS")) wrows = std::max(68, std::min(128, atoi(v)));  // measurement knob
		f.Lw = compute_layout(M, true, wrows);
		f.has_wide = f.Lw.jrows > f.Lc.jrows && 2 * ((mjb_layout_bytes(f.Lw) + 1279) / 1280) <= 128;
	}
	if (!f.has_wide) f.Lw = f.Lc;
	if (dump) dump_layout(f.Lc);
	if (dump && f.has_wide) dump_layout(f.Lw);
	return f;
}

// Sensors whose value is a plain copy of frame doubles (joint / actuator scalars, clock, subtree com, global
// frame positions) become {dst, src} pairs resolved against both layouts; the rest stay on the general path.
void build_sensor_tables(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	std::vector<std::pair<int, int>> cp[3][3];  // layouts: 0 full, 1 fused, 2 wide fused (== 1 when the model has none)
	std::vector<int> slow[3];
	for (int i = 0; i < h.nsensor; i++) {
		const int st = h.sensor_needstage[i] - 1;
		if (st < 0 || st > 2) continue;
		const int type = h.sensor_type[i], id = h.sensor_objid[i], ot = h.sensor_objtype[i];
		bool simple = h.sensor_cutoff[i] <= 0;
		for (int lay = 0; lay < 3 && simple; lay++) {
			const FrameLayout &L = lay == 0 ? M->L : (lay == 1 ? M->Lc : M->Lw);
			int src = -1, n = 1;
			switch (type) {
			case MJB_SENS_JOINTPOS: src = L.qpos + h.jnt_qposadr[id]; break;
			case MJB_SENS_JOINTVEL: src = L.qvel + h.jnt_dofadr[id]; break;
			case MJB_SENS_ACTUATORPOS: src = L.actuator_length + id; break;
			case MJB_SENS_ACTUATORVEL: src = L.actuator_velocity + id; break;
			case MJB_SENS_ACTUATORFRC: src = L.actuator_force + id; break;
			case MJB_SENS_CLOCK: src = L.time; break;
			case MJB_SENS_SUBTREECOM: src = L.subtree_com + 3 * id; n = 3; break;
			case MJB_SENS_BALLANGVEL: src = L.qvel + h.jnt_dofadr[id]; n = 3; break;
			case MJB_SENS_FRAMEQUAT:
				if (h.sensor_refid[i] >= 0 || (ot != MJB_OBJ_XBODY && ot != MJB_OBJ_SITE)) { simple = false; break; }
				n = 4;
				src = ot == MJB_OBJ_XBODY ? L.xquat + 4 * id : L.site_xquat + 4 * id;
				break;
			case MJB_SENS_FRAMEPOS:
				if (h.sensor_refid[i] >= 0) { simple = false; break; }
				n = 3;
				if (ot == MJB_OBJ_BODY) src = L.xipos + 3 * id;
				else if (ot == MJB_OBJ_XBODY) src = L.xpos + 3 * id;
				else if (ot == MJB_OBJ_GEOM) src = L.geom_xpos + 3 * id;
				else src = L.site_xpos + 3 * id;
				break;
			default: simple = false;
			}
			if (simple)
				for (int k = 0; k < n; k++) cp[lay][st].push_back({ h.sensor_adr[i] + k, src + k });
		}
		if (!simple) slow[st].push_back(i);
	}
	int mx = 0;
	for (int st = 0; st < 3; st++) {
		M->sens_ncopy[st] = (int)cp[0][st].size();
		M->sens_nslow[st] = (int)slow[st].size();
		if (M->sens_ncopy[st] > mx) mx = M->sens_ncopy[st];
	}
	M->sens_ncopy_max = mx;
	M->sens_copy.assign((size_t)3 * 3 * (mx ? mx : 1) * 2, 0);
	for (int lay = 0; lay < 3; lay++)
		for (int st = 0; st < 3; st++)
			for (size_t k = 0; k < cp[lay][st].size() && (int)k < M->sens_ncopy[st]; k++) {
				M->sens_copy[((size_t)(lay * 3 + st) * (mx ? mx : 1) + k) * 2] = cp[lay][st][k].first;
				M->sens_copy[((size_t)(lay * 3 + st) * (mx ? mx : 1) + k) * 2 + 1] = cp[lay][st][k].second;
			}
	M->sens_slow.assign((size_t)3 * (h.nsensor ? h.nsensor : 1), 0);
	for (int st = 0; st < 3; st++)
		for (size_t k = 0; k < slow[st].size(); k++) M->sens_slow[(size_t)st * (h.nsensor ? h.nsensor : 1) + k] = slow[st][k];
}

// ---- the stages of mjb_compile, in the order it runs them (their dependencies are listed there).  A stage that can refuse the model calls fail
// and returns false.

// the description itself: sizes, options and arrays present, every actuator / sensor / equality of an implemented kind, the solver caps
bool check_description(const mjb_model_desc &d)
{
	if (d.nq < 0 || d.nv < 0 || d.nbody < 1 || d.njnt < 0 || d.nu < 0 || d.nM < 0) {
		fail(MJB_EINVAL, "mjb_compile: negative size");
		return false;
	}
	{  // activations: one variable per stateful actuator, in actuator order; integrator / filter dynamics
		int na = 0;
		for (int i = 0; i < d.nu; i++) {
			const int dt = d.actuator_dyntype[i];
			if (dt != MJB_DYN_NONE && dt != MJB_DYN_INTEGRATOR && dt != MJB_DYN_FILTER) {
				fail(MJB_EUNSUPPORTED, "mjb_compile: actuator dyntype (muscle / user dynamics) is not supported");
				return false;
			}
			if (d.na > 0 && d.actuator_actadr[i] != (dt != MJB_DYN_NONE ? na : -1)) {
				fail(MJB_EINVAL, "mjb_compile: actuator_actadr must number the stateful actuators in order (-1: stateless)");
				return false;
			}
			if (d.na > 0 && dt != MJB_DYN_NONE && d.actuator_actlimited[i] && !(d.actuator_actrange[2 * i] < d.actuator_actrange[2 * i + 1])) {
				fail(MJB_EINVAL, "mjb_compile: actlimited actuator with an empty actrange");
				return false;
			}
			na += dt != MJB_DYN_NONE ? 1 : 0;
		}
		if (na != d.na) {
			fail(MJB_EINVAL, "mjb_compile: na does not match the number of stateful actuators");
			return false;
		}
	}
	if (d.integrator != MJB_INT_EULER && d.integrator != MJB_INT_RK4 && d.integrator != MJB_INT_IMPLICITFAST) {
		fail(MJB_EUNSUPPORTED, "mjb_compile: integrators Euler, RK4 and implicitfast are implemented (implicit is refused)");
		return false;
	}
	if (!(d.timestep[0] > 0)) {
		fail(MJB_EINVAL, "mjb_compile: timestep must be positive");
		return false;
	}
	if (d.nv > 64 || d.nbody > 64) {
		fail(MJB_EUNSUPPORTED, "mjb_compile: nv = %d, nbody = %d: the tree stages use 64-bit ancestor / subtree masks "
		                       "(nv <= 64, nbody <= 64)", d.nv, d.nbody);
		return false;
	}
	// every array the description declares must be there before anything below reads it
#define MJB_SIZE(name)                                                                    \
	if (d.name < 0) {                                                                     \
		fail(MJB_EINVAL, "mjb_compile: negative size %s", #name);                         \
		return false;                                                                     \
	}
#define MJB_OPT_I(name)
#define MJB_OPT_D(name, n)
#define MJB_ARR_I(name, rows, cols)                                                       \
	if ((size_t)d.rows * (cols) && !d.name) {                                             \
		fail(MJB_EINVAL, "mjb_compile: array %s is NULL", #name);                         \
		return false;                                                                     \
	}
#define MJB_ARR_D(name, rows, cols) MJB_ARR_I(name, rows, cols)
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	for (int i = 0; i < d.nsensor; i++) {
		static const int ok[] = { MJB_SENS_MAGNETOMETER, MJB_SENS_RANGEFINDER, MJB_SENS_TOUCH, MJB_SENS_ACCELEROMETER, MJB_SENS_VELOCIMETER, MJB_SENS_GYRO, MJB_SENS_FORCE,
			                      MJB_SENS_TORQUE, MJB_SENS_JOINTPOS, MJB_SENS_JOINTVEL, MJB_SENS_TENDONPOS, MJB_SENS_TENDONVEL,
			                      MJB_SENS_ACTUATORPOS, MJB_SENS_ACTUATORVEL, MJB_SENS_ACTUATORFRC, MJB_SENS_BALLQUAT,
			                      MJB_SENS_BALLANGVEL, MJB_SENS_FRAMEPOS, MJB_SENS_FRAMEQUAT, MJB_SENS_FRAMEXAXIS,
			                      MJB_SENS_FRAMEYAXIS, MJB_SENS_FRAMEZAXIS, MJB_SENS_FRAMELINVEL, MJB_SENS_FRAMEANGVEL,
			                      MJB_SENS_FRAMELINACC, MJB_SENS_FRAMEANGACC, MJB_SENS_SUBTREECOM, MJB_SENS_CLOCK, MJB_SENS_JOINTLIMITPOS, MJB_SENS_JOINTLIMITVEL,
			                      MJB_SENS_JOINTLIMITFRC, MJB_SENS_TENDONLIMITPOS, MJB_SENS_TENDONLIMITVEL, MJB_SENS_TENDONLIMITFRC, MJB_SENS_SUBTREELINVEL,
			                      MJB_SENS_SUBTREEANGMOM, MJB_SENS_JOINTACTFRC };
		bool found = false;
		for (int t : ok) found = found || t == d.sensor_type[i];
		if (!found) {
			fail(MJB_EUNSUPPORTED, "mjb_compile: sensor %d has type %d, which is not implemented", i, d.sensor_type[i]);
			return false;
		}
	}
	for (int i = 0; i < d.neq; i++) {
		const int t = d.eq_type[i], a = d.eq_obj1id[i], b = d.eq_obj2id[i];
		const bool body_ok = a >= 0 && a < d.nbody && b >= 0 && b < d.nbody;
		const bool jnt_ok = a >= 0 && a < d.njnt && b >= -1 && b < d.njnt;
		const bool ten_ok = a >= 0 && a < d.ntendon && b >= -1 && b < d.ntendon;
		if (!((t == MJB_EQ_CONNECT || t == MJB_EQ_WELD) ? body_ok : ((t == MJB_EQ_JOINT && jnt_ok) || (t == MJB_EQ_TENDON && ten_ok)))) {
			fail(MJB_EUNSUPPORTED, "mjb_compile: equality %d: type %d with objects (%d, %d) is not supported "
			                       "(connect / weld between bodies, joint between hinge / slide joints)", i, t, a, b);
			return false;
		}
	}
	if (d.neq > 0 && d.nefcmax <= 0) {
		fail(MJB_EINVAL, "mjb_compile: equality constraints need nefcmax > 0");
		return false;
	}
	if (d.nefcmax > 0 || d.nconmax > 0) {
		if (d.solver != MJB_SOL_PGS && d.solver != MJB_SOL_NEWTON && d.solver != MJB_SOL_CG) {
			fail(MJB_EUNSUPPORTED, "mjb_compile: unknown solver (PGS = 0, CG = 1, Newton = 2)");
			return false;
		}
		const int rowcap = d.solver != MJB_SOL_PGS ? 1024 : ((d.cone == MJB_CONE_ELLIPTIC && d.nconmax > 0) ? 64 : 128);
		if (d.nefcmax > rowcap) {  // (nv <= 64: checked above)
			fail(MJB_EUNSUPPORTED, "mjb_compile: one env per wavefront: nv <= 64 and nefcmax <= 128 (PGS; 64 with elliptic cones) / "
			                       "1024 (Newton / CG; lower <size njmax>); got nefcmax = %d, nv = %d", d.nefcmax, d.nv);
			return false;
		}
		if (!(d.meaninertia[0] > 0)) {
			fail(MJB_EINVAL, "mjb_compile: meaninertia must be positive");
			return false;
		}
	}
	return true;
}

// the host copy: every array behind the other in hint / hdbl (declaration order), the copy's pointers re-pointed at them
void copy_description(mjb_model *M, const mjb_model_desc &d)
{
	M->h = d;
	// copy arrays (declaration order; check_description has seen every one that has elements)
#define MJB_SIZE(name)
#define MJB_OPT_I(name)
#define MJB_OPT_D(name, n)
#define MJB_ARR_I(name, rows, cols)                                                       \
	{                                                                                     \
		size_t n = (size_t)d.rows * (cols);                                               \
		M->ioff.push_back(M->hint.size());                                                \
		M->hint.insert(M->hint.end(), d.name, d.name + n);                                \
		if ((M->hint.size() & 1)) M->hint.push_back(0);                                   \
	}
#define MJB_ARR_D(name, rows, cols)                                                       \
	{                                                                                     \
		size_t n = (size_t)d.rows * (cols);                                               \
		M->doff.push_back(M->hdbl.size());                                                \
		M->hdbl.insert(M->hdbl.end(), d.name, d.name + n);                                \
	}
#include "../../include/mjb_model_fields.def"
#undef MJB_ARR_I
#undef MJB_ARR_D
	// re-point the host copy
	{
		size_t ii = 0, di = 0;
#define MJB_ARR_I(name, rows, cols) M->h.name = M->hint.data() + M->ioff[ii++];
#define MJB_ARR_D(name, rows, cols) M->h.name = M->hdbl.data() + M->doff[di++];
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	}
}

// every index a kernel (or a later stage) follows stays inside its table; free joints and the body tree are where the kinematics expect them
bool check_index_tables(const mjb_model_desc &h)
{
	// ---- every index table a kernel uses as an LDS / HBM offset must stay inside its target
	{
		auto in = [](int v, int lo, int hi) { return v >= lo && v < hi; };
		const char *bad = nullptr;
		for (int b = 0; b < h.nbody && !bad; b++) {
			if (!in(h.body_mocapid[b], -1, h.nmocap)) bad = "body_mocapid";
			if (!in(h.body_rootid[b], 0, h.nbody) || !in(h.body_weldid[b], 0, h.nbody)) bad = "body_rootid / body_weldid";
			if (h.body_jntnum[b] < 0 || h.body_dofnum[b] < 0 || (h.body_jntnum[b] && !in(h.body_jntadr[b], 0, h.njnt)) ||
			    h.body_jntnum[b] + (h.body_jntnum[b] ? h.body_jntadr[b] : 0) > h.njnt || (h.body_dofnum[b] && !in(h.body_dofadr[b], 0, h.nv)) ||
			    h.body_dofnum[b] + (h.body_dofnum[b] ? h.body_dofadr[b] : 0) > h.nv)
				bad = "body_jntadr / body_jntnum / body_dofadr / body_dofnum";
		}
		for (int j = 0; j < h.njnt && !bad; j++) {
			const int t = h.jnt_type[j], nq = t == MJB_JNT_FREE ? 7 : (t == MJB_JNT_BALL ? 4 : 1), nd = t == MJB_JNT_FREE ? 6 : (t == MJB_JNT_BALL ? 3 : 1);
			if (!in(t, 0, 4)) bad = "jnt_type";
			else if (!in(h.jnt_bodyid[j], 0, h.nbody)) bad = "jnt_bodyid";
			else if (h.jnt_qposadr[j] < 0 || h.jnt_qposadr[j] + nq > h.nq) bad = "jnt_qposadr";
			else if (h.jnt_dofadr[j] < 0 || h.jnt_dofadr[j] + nd > h.nv) bad = "jnt_dofadr";
		}
		for (int i = 0; i < h.nv && !bad; i++) {
			if (!in(h.dof_bodyid[i], 0, h.nbody)) bad = "dof_bodyid";
			if (!in(h.dof_jntid[i], 0, h.njnt)) bad = "dof_jntid";
			if (!in(h.dof_parentid[i], -1, i)) bad = "dof_parentid";
		}
		for (int g = 0; g < h.ngeom && !bad; g++) {
			if (!in(h.geom_bodyid[g], 0, h.nbody)) bad = "geom_bodyid";
			const int t = h.geom_type[g];
			if (t != MJB_GEOM_PLANE && t != MJB_GEOM_SPHERE && t != MJB_GEOM_CAPSULE && t != MJB_GEOM_BOX) bad = "geom_type (plane / sphere / capsule / box)";
			if (!in(h.geom_condim[g], 1, 7) || h.geom_condim[g] == 2 || h.geom_condim[g] == 5) bad = "geom_condim (1, 3, 4, 6)";
		}
		for (int p = 0; p < 2 * h.ncollpair && !bad; p++)
			if (!in(h.collpair_geom[p], 0, h.ngeom)) bad = "collpair_geom";
		for (int p = 0; p < h.ncollpair && !bad; p++)
			if (h.collpair_explicit[p] && h.collpair_condim[p] > 0 && h.collpair_condim[p] != 1 && h.collpair_condim[p] != 3 && h.collpair_condim[p] != 4 && h.collpair_condim[p] != 6)
				bad = "collpair_condim (1, 3, 4, 6)";
		for (int st = 0; st < h.nsite && !bad; st++)
			if (!in(h.site_bodyid[st], 0, h.nbody)) bad = "site_bodyid";
		for (int t = 0; t < h.ntendon && !bad; t++)
			if (h.tendon_num[t] < 0 || h.tendon_adr[t] < 0 || h.tendon_adr[t] + h.tendon_num[t] > h.nwrap) bad = "tendon_adr / tendon_num";
		for (int w = 0; w < h.nwrap && !bad; w++)
			if (!in(h.wrap_objid[w], 0, h.njnt) || h.jnt_type[h.wrap_objid[w]] < MJB_JNT_SLIDE) bad = "wrap_objid (hinge / slide joints)";
		auto objcount = [&](int ot) {
			switch (ot) {
			case MJB_OBJ_BODY: case MJB_OBJ_XBODY: return h.nbody;
			case MJB_OBJ_JOINT: return h.njnt;
			case MJB_OBJ_GEOM: return h.ngeom;
			case MJB_OBJ_SITE: return h.nsite;
			case MJB_OBJ_ACTUATOR: return h.nu;
			default: return 0;
			}
		};
		for (int i = 0; i < h.nsensor && !bad; i++) {
			const int t = h.sensor_type[i];
			int cnt;
			if (t == MJB_SENS_JOINTPOS || t == MJB_SENS_JOINTVEL || t == MJB_SENS_BALLQUAT || t == MJB_SENS_BALLANGVEL || t == MJB_SENS_JOINTACTFRC ||
			    (t >= MJB_SENS_JOINTLIMITPOS && t <= MJB_SENS_JOINTLIMITFRC))
				cnt = h.njnt;
			else if (t == MJB_SENS_TENDONPOS || t == MJB_SENS_TENDONVEL || (t >= MJB_SENS_TENDONLIMITPOS && t <= MJB_SENS_TENDONLIMITFRC)) cnt = h.ntendon;
			else if (t == MJB_SENS_ACTUATORPOS || t == MJB_SENS_ACTUATORVEL || t == MJB_SENS_ACTUATORFRC) cnt = h.nu;
			else if (t == MJB_SENS_SUBTREECOM || t == MJB_SENS_SUBTREELINVEL || t == MJB_SENS_SUBTREEANGMOM) cnt = h.nbody;
			else if (t == MJB_SENS_CLOCK) cnt = 1 << 30;
			else if (t >= MJB_SENS_FRAMEPOS && t <= MJB_SENS_FRAMEANGACC) cnt = objcount(h.sensor_objtype[i]);
			else cnt = h.nsite;  // touch, accelerometer, velocimeter, gyro, force, torque
			if (t != MJB_SENS_CLOCK && !in(h.sensor_objid[i], 0, cnt)) bad = "sensor_objid";
			else if (t >= MJB_SENS_JOINTLIMITPOS && t <= MJB_SENS_JOINTLIMITFRC && h.jnt_type[h.sensor_objid[i]] < MJB_JNT_SLIDE) bad = "sensor_objid (joint limit sensors: hinge / slide joints)";
			if (h.sensor_refid[i] >= 0 && !in(h.sensor_refid[i], 0, objcount(h.sensor_reftype[i]))) bad = "sensor_refid";
			if (!in(h.sensor_dim[i], 1, 5) || h.sensor_adr[i] < 0 || h.sensor_adr[i] + h.sensor_dim[i] > h.nsensordata) bad = "sensor_adr / sensor_dim";
			if (!in(h.sensor_needstage[i], 1, 4)) bad = "sensor_needstage";
		}
		if (bad) {
			fail(MJB_EINVAL, "mjb_compile: index table %s is out of range", bad);
			return false;
		}
		// the kinematics (every kernel's, and mj_setConst's mirror below) takes `jntnum == 1 && FREE` as the only free-joint case
		for (int b = 0; b < h.nbody; b++)
			for (int j = h.body_jntadr[b]; j < h.body_jntadr[b] + h.body_jntnum[b]; j++)
				if (h.jnt_type[j] == MJB_JNT_FREE && (h.body_jntnum[b] != 1 || h.body_parentid[b] != 0)) {
					fail(MJB_EINVAL, "mjb_compile: the free joint %d must be the only joint of a top-level body (body %d has %d joints, parent %d)", j, b,
					     h.body_jntnum[b], h.body_parentid[b]);
					return false;
				}
	}
	// ---- validation of the tree tables the kernels index with
	for (int b = 1; b < h.nbody; b++)
		if (h.body_parentid[b] < 0 || h.body_parentid[b] >= b) {
			fail(MJB_EINVAL, "mjb_compile: body_parentid[%d] must precede the body", b);
			return false;
		}
	return true;
}

// the dof tree (M_rowdof / M_coldof, dof_depth, maxdepth) checked against dof_Madr / nM, the actuators' transmissions (site_act), gravcomp_body,
// dof_jstart and the packed per-body / per-dof / per-joint records
bool build_tree_tables(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	int nM = 0;
	for (int i = 0; i < h.nv; i++) {
		if (h.dof_Madr[i] != nM) {  // (dof_parentid[i] < i: check_index_tables)
			fail(MJB_EINVAL, "mjb_compile: inconsistent dof_parentid / dof_Madr at dof %d", i);
			return false;
		}
		int depth = 0;
		for (int j = i; j >= 0; j = h.dof_parentid[j]) {
			M->M_rowdof.push_back(i);
			M->M_coldof.push_back(j);
			depth++;
		}
		M->dof_depth.push_back(depth);
		if (depth > M->maxdepth) M->maxdepth = depth;
		nM += depth;
	}
	if (nM != h.nM) {
		fail(MJB_EINVAL, "mjb_compile: nM = %d does not match the dof tree (%d)", h.nM, nM);
		return false;
	}
	for (int i = 0; i < h.nu; i++) {
		int j = h.actuator_trnid[2 * i];
		const int r = h.actuator_trnid[2 * i + 1];
		const bool okj = h.actuator_trntype[i] == MJB_TRN_JOINT && j >= 0 && j < h.njnt && h.jnt_type[j] >= MJB_JNT_SLIDE;
		const bool okt = h.actuator_trntype[i] == MJB_TRN_TENDON && j >= 0 && j < h.ntendon;
		// site transmission: the site, and no refsite (-1) or another site
		const bool oks = h.actuator_trntype[i] == MJB_TRN_SITE && j >= 0 && j < h.nsite && (r == -1 || (r >= 0 && r < h.nsite && r != j));
		if (!okj && !okt && !oks) {
			fail(MJB_EUNSUPPORTED, "mjb_compile: actuator %d: joint transmission on hinge / slide joints, fixed-tendon and site transmissions "
			                       "(refsite -1 or another site) are supported", i);
			return false;
		}
		if (oks) M->site_act.push_back(i);
	}
	// gravity compensation: any finite coefficient (above 1 and below 0 too); the bodies that have one
	for (int b = 0; b < h.nbody; b++) {
		if (!std::isfinite(h.body_gravcomp[b])) {
			fail(MJB_EINVAL, "mjb_compile: body_gravcomp[%d] is not finite", b);
			return false;
		}
		if (b > 0 && h.body_gravcomp[b] != 0) M->gravcomp_body.push_back(b);
	}
	// velocity-group start of each dof (hinge/slide: itself; ball: first of 3; free: first of each triple)
	M->dof_jstart.resize(h.nv);
	for (int dd = 0; dd < h.nv; dd++) {
		int j = h.dof_jntid[dd], t = h.jnt_type[j], da = h.jnt_dofadr[j];
		if (t == MJB_JNT_HINGE || t == MJB_JNT_SLIDE) M->dof_jstart[dd] = dd;
		else if (t == MJB_JNT_BALL) M->dof_jstart[dd] = da;
		else M->dof_jstart[dd] = (dd - da < 3) ? da : da + 3;
	}
	// packed per-body / per-dof / per-joint records
	for (int b = 0; b < h.nbody; b++) {
		int rec[4] = { h.body_parentid[b], h.body_dofadr[b], h.body_dofnum[b], h.body_rootid[b] };
		int rec2[4] = { h.body_jntadr[b], h.body_jntnum[b], h.body_sameframe[b], h.body_weldid[b] };
		M->body_rec.insert(M->body_rec.end(), rec, rec + 4);
		M->body_rec2.insert(M->body_rec2.end(), rec2, rec2 + 4);
	}
	for (int dd = 0; dd < h.nv; dd++) {
		int rec[4] = { h.dof_Madr[dd], M->dof_depth[dd] - 1, h.dof_bodyid[dd], h.dof_parentid[dd] };
		M->dof_rec.insert(M->dof_rec.end(), rec, rec + 4);
	}
	// what the per-dof / per-joint phases of com_vel / com_pos look up, one 16-byte record each (the chains of dependent table reads --
	// dof -> joint -> type, joint -> body -> root -- cost a trip to L2 per link)
	for (int dd = 0; dd < h.nv; dd++) {
		const int j = h.dof_jntid[dd], bd = h.dof_bodyid[dd];
		int rec[4] = { (h.jnt_type[j] == MJB_JNT_FREE && dd - h.jnt_dofadr[j] < 3) ? 1 : 0, M->dof_jstart[dd] == h.body_dofadr[bd] ? 1 : 0,
			           h.body_parentid[bd], bd };
		M->dof_rec2.insert(M->dof_rec2.end(), rec, rec + 4);
	}
	for (int j = 0; j < h.njnt; j++) {
		const int bi = h.jnt_bodyid[j];
		int rec[4] = { bi, h.jnt_type[j], h.jnt_dofadr[j], h.body_rootid[bi] };
		M->jnt_rec.insert(M->jnt_rec.end(), rec, rec + 4);
	}
	if (M->dof_rec2.empty()) M->dof_rec2.assign(4, 0);
	if (M->jnt_rec.empty()) M->jnt_rec.assign(4, 0);
	return true;
}

// the L'DL factorisation of M as a micro-programme: pivot by pivot (fac_ops / fac_beg) and by levels of the elimination tree (flv_*)
void build_factor_programme(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	for (int k = 0; k < h.nv; k++) {
		M->fac_beg.push_back((int)M->fac_ops.size() / 4);
		const int kk = h.dof_Madr[k], na = M->dof_depth[k] - 1;
		for (int a = 0; a < na; a++) {
			const int i = M->M_coldof[kk + 1 + a];
			for (int bb = a; bb < na; bb++) {
				int op[4] = { h.dof_Madr[i] + (bb - a), kk + 1 + a, kk + 1 + bb, 0 };
				M->fac_ops.insert(M->fac_ops.end(), op, op + 4);
			}
		}
	}
	M->fac_beg.push_back((int)M->fac_ops.size() / 4);
	// the same updates scheduled by LEVELS of the elimination tree (= the dof tree): pivots of equal height touch disjoint rows of
	// their own and only meet in the entries of common ancestors, so a level runs in one round: one lane per contribution
	// LD[dst] -= LD[srcA] / D_pivot * LD[srcB], the contributions to one entry combined by its first lane in descending pivot order.
	// flv_hdr [level][4] = { slots, longest list of slot 0 / 1 / 2 };  flv_rec [level][3][64][4] (below).  flv_n == 0 (a level with
	// more than 192 contributions, a list longer than 6, more than 64 levels): the kernels keep the pivot-by-pivot factorisation
	{
		std::vector<int> hgt((size_t)(h.nv > 0 ? h.nv : 1), 0);
		int nlev = 0, nseg = 0;
		bool flv_ok = true;
		for (int k = h.nv - 1; k >= 0; k--) {
			const int pk = h.dof_parentid[k];
			if (pk >= 0 && hgt[pk] < hgt[k] + 1) hgt[pk] = hgt[k] + 1;
			if (hgt[k] + 1 > nlev) nlev = hgt[k] + 1;
		}
		for (int lev = 0; lev < nlev; lev++) {
			std::vector<int> dsts;
			std::vector<std::vector<int>> lists;
			for (int k = h.nv - 1; k >= 0; k--) {
				if (hgt[k] != lev) continue;
				const int kk = h.dof_Madr[k], na = M->dof_depth[k] - 1;
				for (int a = 0; a < na; a++) {
					const int i = M->M_coldof[kk + 1 + a];
					for (int bb = a; bb < na; bb++) {
						const int dst = h.dof_Madr[i] + (bb - a);
						size_t at = 0;
						while (at < dsts.size() && dsts[at] != dst) at++;
						if (at == dsts.size()) {
							dsts.push_back(dst);
							lists.emplace_back();
						}
						lists[at].push_back(kk + 1 + a);
						lists[at].push_back(kk + 1 + bb);
						lists[at].push_back(k);
					}
				}
			}
			// a level's CONTRIBUTIONS at fixed places, one 16-byte word per lane in up to three slots: { dst | (row + 1 of a diagonal
			// dst) << 16, valid | owner << 1 | list length << 8, srcA | srcB << 16, pivot }.  The contributions to one entry sit in
			// consecutive lanes of one 16-lane row, the entry's owner first: it collects the others' products by DPP row shifts.
			// The lists go first (they must not straddle a row), the single contributions fill up.
			if (dsts.empty()) continue;
			std::vector<int> W;
			int tm[3] = { 0, 0, 0 };
			auto put = [&](size_t it) {
				const int d = dsts[it], n = (int)lists[it].size() / 3;
				const int drow1 = M->M_rowdof[d] == M->M_coldof[d] ? M->M_rowdof[d] + 1 : 0;
				while ((int)(W.size() / 4) % 16 + n > 16) W.insert(W.end(), 4, 0);
				for (int t = 0; t < n; t++) {
					const int slot = (int)(W.size() / 4) / 64;
					if (slot < 3 && n > tm[slot]) tm[slot] = n;
					int r[4] = { d | (drow1 << 16), 1 | (t == 0 ? 2 : 0) | (n << 8), lists[it][3 * t] | (lists[it][3 * t + 1] << 16), lists[it][3 * t + 2] };
					W.insert(W.end(), r, r + 4);
				}
			};
			for (size_t it = 0; it < dsts.size(); it++) {
				if (lists[it].size() / 3 > 6) flv_ok = false;
				else if (lists[it].size() / 3 > 1) put(it);
			}
			for (size_t it = 0; it < dsts.size(); it++)
				if (lists[it].size() / 3 == 1) put(it);
			const int nslot = ((int)(W.size() / 4) + 63) / 64;
			if (nslot > 3) flv_ok = false;
			W.resize((size_t)3 * 64 * 4, 0);
			int hdr[4] = { nslot, tm[0], tm[1], tm[2] };
			M->flv_hdr.insert(M->flv_hdr.end(), hdr, hdr + 4);
			M->flv_rec.insert(M->flv_rec.end(), W.begin(), W.end());
			nseg++;
		}
		if (h.nM >= 65536 || nseg > 64) flv_ok = false;
		if (!flv_ok) {
			nseg = 0;
			M->flv_hdr.clear();
			M->flv_rec.clear();
		}
		// (three empty levels behind the last: the kernel's look-ahead fetches need no bounds test)
		M->flv_rec.insert(M->flv_rec.end(), (size_t)3 * (3 * 64 * 4), 0);
		M->flv_n = nseg;
		// per qM entry: its row, and whether it is the diagonal one (the first and the last round of factor_levels)
		M->flv_ent.assign((size_t)((h.nM + 255) / 256 * 256 + 256), 0);
		for (int en = 0; en < h.nM; en++) M->flv_ent[en] = M->M_rowdof[en] | (M->M_rowdof[en] == M->M_coldof[en] ? 0x10000 : 0);
		if (M->flv_hdr.empty()) M->flv_hdr.assign(4, 0);
		if (M->flv_rec.empty()) M->flv_rec.assign(4, 0);
	}
}

// bit masks and ancestor tables of the tree stages: body_dofmask, M_dense, M_sym, body_anc / kin_rounds, body_dofanc, body_submask, sub_S, dof_bodymask
void build_masks(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	// ancestor-dof bit masks per body (contact Jacobians)
	M->body_dofmask.assign((size_t)2 * h.nbody, 0);
	for (int b = 1; b < h.nbody; b++) {
			int bb = b;
			while (bb > 0 && h.body_dofnum[bb] == 0) bb = h.body_parentid[bb];
			if (bb == 0) continue;
			for (int i = h.body_dofadr[bb] + h.body_dofnum[bb] - 1; i >= 0; i = h.dof_parentid[i])
				M->body_dofmask[2 * b + (i >> 5)] |= (int)(1u << (i & 31));
		}
	// dense address map of the joint-space inertia for the register-resident factor / solve (nv <= 16)
	M->M_dense.assign(256, -1);
	if (h.nv <= 16)
		for (int en = 0; en < h.nM; en++) M->M_dense[16 * M->M_rowdof[en] + M->M_coldof[en]] = en;
	// symmetric dense address map (nv <= 32): qM address of entry (i, j) = (j, i), -1 where the tree leaves a zero.  The primal
	// solvers keep row `lane` of M in registers (fwd_constraint_newton) instead of a dense nv x nv copy in the frame.
	M->M_sym.assign(1024, -1);
	if (h.nv <= 32)
		for (int en = 0; en < h.nM; en++) {
			M->M_sym[32 * M->M_rowdof[en] + M->M_coldof[en]] = en;
			M->M_sym[32 * M->M_coldof[en] + M->M_rowdof[en]] = en;
		}
	// ancestors at distance 2^r for the pointer-jumping kinematics (0 = world or beyond the root)
	{
		int maxd = 0;
		std::vector<int> depth((size_t)h.nbody, 0);
		for (int b = 1; b < h.nbody; b++) {
			depth[b] = depth[h.body_parentid[b]] + 1;
			if (depth[b] > maxd) maxd = depth[b];
		}
		M->kin_rounds = 0;
		while ((1 << M->kin_rounds) < maxd) M->kin_rounds++;
		M->body_anc.assign((size_t)(M->kin_rounds + 2) * h.nbody, 0);
		for (int b = 1; b < h.nbody; b++) M->body_anc[b] = h.body_parentid[b];
		for (int r = 1; r < M->kin_rounds + 2; r++)
			for (int b = 1; b < h.nbody; b++) {
				const int a = M->body_anc[(size_t)(r - 1) * h.nbody + b];
				M->body_anc[(size_t)r * h.nbody + b] = a ? M->body_anc[(size_t)(r - 1) * h.nbody + a] : 0;
			}
	}
	// ancestor dof lists for the root-to-leaf sums
	{
		M->body_dofanc.assign((size_t)4 * h.nbody, -1);
		bool aok = h.nv <= 255 && h.nv > 0;
		int amax = 0;
		for (int b = 1; b < h.nbody && aok; b++) {
			int n = 0;
			for (int i = 0; i < h.nv && i < 64; i++)
				if ((M->body_dofmask[2 * b + (i >> 5)] >> (i & 31)) & 1) {
					if (n >= 16) { aok = false; break; }
					unsigned int w = (unsigned int)M->body_dofanc[4 * b + (n >> 2)];
					w = (w & ~(0xFFu << (8 * (n & 3)))) | ((unsigned int)i << (8 * (n & 3)));
					M->body_dofanc[4 * b + (n >> 2)] = (int)w;
					n++;
				}
			if (n > amax) amax = n;
		}
		if (h.nv > 64) aok = false;
		M->dofanc_max = aok ? amax : 0;
	}
	// subtree membership masks (subtree com, composite inertia)
	M->body_submask.assign((size_t)2 * h.nbody, 0);
	for (int b = 0; b < h.nbody && h.nbody <= 64; b++)
		for (int a = b;; a = h.body_parentid[a]) {
			M->body_submask[2 * a + (b >> 5)] |= (int)(1u << (b & 31));
			if (a == 0) break;
		}
	M->sub_nt = h.nbody <= 16 ? 1 : (h.nbody <= 32 ? 2 : 0);
	M->sub_S.assign((size_t)(M->sub_nt > 0 ? M->sub_nt * 4 * M->sub_nt * 64 : 1), 0.0);
	for (int t = 0; t < M->sub_nt; t++)
		for (int k = 0; k < 4 * M->sub_nt; k++)
			for (int l = 0; l < 64; l++) {
				const int a = 16 * t + (l & 15), b = 4 * k + (l >> 4);
				if (a < h.nbody && b < h.nbody && ((M->body_submask[2 * a + (b >> 5)] >> (b & 31)) & 1))
					M->sub_S[((size_t)t * 4 * M->sub_nt + k) * 64 + l] = 1.0;
			}
	M->dof_bodymask.assign((size_t)2 * (h.nv > 0 ? h.nv : 1), 0);
	for (int b = 1; b < h.nbody; b++)
		for (int i = 0; i < h.nv; i++)
			if ((M->body_dofmask[2 * b + (i >> 5)] >> (i & 31)) & 1) M->dof_bodymask[2 * i + (b >> 5)] |= (int)(1u << (b & 31));
}

// which of the special kernels take the model: the lane = env topology (le_topo), the split step's smooth topology (sm_topo), their tape
void classify_lane_env(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	const bool gravcomp = !M->gravcomp_body.empty();  // (such a model matches no compiled-in topology; the split step's smooth kernel has no such term and stands down)
	M->le_topo = mjb_lane_env_match(&h);
	if (M->le_topo < 0 && mjb_lane_env_eligible(&h)) M->le_topo = MJB_LE_TOPO_JIT;
	// the split step (smooth half in lane = env form, constraint half one env per wavefront): the constraint half is kernel variant 9's -- plain PGS,
	// pyramidal / frictionless contacts, nv <= 16, no stage that needs mj_rnePostConstraint
	M->sm_topo = -1;
	if (!gravcomp && h.nefcmax > 0 && h.solver == MJB_SOL_PGS && !(h.cone == MJB_CONE_ELLIPTIC && h.nconmax > 0) && h.nv <= 16 && !M->need_rnepost && h.nefcmax <= 128)
		M->sm_topo = mjb_smooth_match(&h);
	if (M->le_topo != MJB_LE_TOPO_NONE || M->sm_topo >= 0) {
		M->le_tape.assign(mjb_lane_env_tape_doubles(&h), 0.0);
		mjb_lane_env_tape(&h, M->le_tape.data());
	}
}

// damp_int / eulerdamp: what the integrator adds to M's diagonal; implicitfast refuses what is not a model constant on the diagonal
bool build_integrator_damping(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	M->eulerdamp = 0;
	M->damp_int.assign(h.dof_damping, h.dof_damping + h.nv);
	if (h.integrator == MJB_INT_IMPLICITFAST) {
		// mj_implicit, mjINT_IMPLICITFAST: qH = M - h D, D = mjd_passive_vel + mjd_actuator_vel; a model constant on the diagonal here
		for (int t = 0; t < h.ntendon; t++)
			if (h.tendon_damping[t] != 0) {
				fail(MJB_EUNSUPPORTED, "mjb_compile: integrator implicitfast with tendon damping is not supported");
				return false;
			}
		for (int i = 0; i < h.nv; i++) M->damp_int[i] = (h.disableflags & MJB_DSBL_PASSIVE) ? 0.0 : h.dof_damping[i];
		for (int i = 0; i < h.nu; i++) {
			if (h.actuator_gaintype[i] == MJB_GAIN_AFFINE && h.actuator_gainprm[3 * i + 2] != 0) {
				fail(MJB_EUNSUPPORTED, "mjb_compile: integrator implicitfast with a velocity term in an affine actuator gain is not supported");
				return false;
			}
			if (h.disableflags & MJB_DSBL_ACTUATION) continue;
			const double bv = h.actuator_biastype[i] == MJB_BIAS_AFFINE ? h.actuator_biasprm[3 * i + 2] : 0.0, g = h.actuator_gear[6 * i];
			if (h.actuator_trntype[i] == MJB_TRN_SITE) {
				if (bv != 0) {  // (moment' bv moment depends on the configuration and is not diagonal)
					fail(MJB_EUNSUPPORTED, "mjb_compile: integrator implicitfast with a velocity-dependent actuator on a site is not supported");
					return false;
				}
				continue;
			}
			if (h.actuator_trntype[i] == MJB_TRN_TENDON) {
				if (bv != 0) {  // (moment' bv moment couples the tendon's joints: not diagonal)
					fail(MJB_EUNSUPPORTED, "mjb_compile: integrator implicitfast with a velocity-dependent actuator on a tendon is not supported");
					return false;
				}
				continue;
			}
			M->damp_int[h.jnt_dofadr[h.actuator_trnid[2 * i]]] -= g * g * bv;
		}
		for (int i = 0; i < h.nv; i++)
			if (M->damp_int[i] != 0) M->eulerdamp = 1;
	} else if (!(h.disableflags & MJB_DSBL_EULERDAMP))
		for (int i = 0; i < h.nv; i++)
			if (h.dof_damping[i] > 0) M->eulerdamp = 1;
	return true;
}

// nfriction: the dofs and tendons that get a dry-friction row
void count_friction_rows(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	M->nfriction = 0;
	if (!(h.disableflags & MJB_DSBL_FRICTIONLOSS))
		for (int i = 0; i < h.nv; i++)
			if (h.dof_frictionloss[i] > 0) M->nfriction++;
	if (!(h.disableflags & MJB_DSBL_FRICTIONLOSS))
		for (int t = 0; t < h.ntendon; t++)
			if (h.tendon_frictionloss[t] > 0) M->nfriction++;
}

void build_pair_records(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	// per-pair records of the static candidate list: everything mj_collision / mj_contactParam derive from the two geoms'
	// constants, resolved once (friction stays per env: rule 0 = max of both geoms, 1 = geom1, 2 = geom2)
	M->pair_i.assign((size_t)8 * (h.ncollpair > 0 ? h.ncollpair : 1), 0);
	M->pair_d.assign((size_t)24 * (h.ncollpair > 0 ? h.ncollpair : 1), 0.0);
	for (int p = 0; p < h.ncollpair; p++) {
		const int g1 = h.collpair_geom[2 * p], g2 = h.collpair_geom[2 * p + 1];
		int *pi = M->pair_i.data() + 8 * p;
		double *pd = M->pair_d.data() + 24 * p;
		pi[0] = g1; pi[1] = g2; pi[2] = h.geom_type[g1]; pi[3] = h.geom_type[g2];
		pi[6] = MJB_COLFUNC_DEFAULT;  // collision-function override (mjb_register_collision patches the batch's copy)
		pi[7] = 0;
		for (int k = 0; k < 3; k++) {
			pd[k] = h.geom_size[3 * g1 + k];
			pd[3 + k] = h.geom_size[3 * g2 + k];
		}
		const double margin = std::max(h.geom_margin[g1], h.geom_margin[g2]), gap = std::max(h.geom_gap[g1], h.geom_gap[g2]);
		pd[6] = margin; pd[7] = gap; pd[8] = h.geom_rbound[g1]; pd[9] = h.geom_rbound[g2];
		double *solref = pd + 10, *solimp = pd + 12;
		const int pr1 = h.geom_priority[g1], pr2 = h.geom_priority[g2];
		if (pr1 != pr2) {  // mj_contactParam: the geom with the higher priority decides
			const int g = pr1 > pr2 ? g1 : g2;
			pi[4] = h.geom_condim[g];
			pi[5] = pr1 > pr2 ? 1 : 2;
			for (int k = 0; k < 2; k++) solref[k] = h.geom_solref[2 * g + k];
			for (int k = 0; k < 5; k++) solimp[k] = h.geom_solimp[5 * g + k];
		} else {
			pi[4] = std::max(h.geom_condim[g1], h.geom_condim[g2]);
			pi[5] = 0;
			const double s1 = h.geom_solmix[g1], s2 = h.geom_solmix[g2];
			double mix;
			if (s1 >= 1e-15 && s2 >= 1e-15) mix = s1 / (s1 + s2);
			else if (s1 < 1e-15 && s2 < 1e-15) mix = 0.5;
			else if (s1 < 1e-15) mix = 0.0;
			else mix = 1.0;
			const double r10 = h.geom_solref[2 * g1], r20 = h.geom_solref[2 * g2];
			for (int k = 0; k < 2; k++) {
				const double a = h.geom_solref[2 * g1 + k], b = h.geom_solref[2 * g2 + k];
				solref[k] = (r10 > 0 && r20 > 0) ? mix * a + (1 - mix) * b : std::min(a, b);
			}
			for (int k = 0; k < 5; k++) solimp[k] = mix * h.geom_solimp[5 * g1 + k] + (1 - mix) * h.geom_solimp[5 * g2 + k];
		}
		pd[17] = margin - gap;
		pd[21] = h.body_invweight0[2 * h.geom_bodyid[g1]] + h.body_invweight0[2 * h.geom_bodyid[g2]];
		for (int k = 0; k < 3; k++) {  // mj_contactParam's friction of the MODEL's geoms (per-env overrides are mixed on the device)
			const double a = h.geom_friction[3 * g1 + k], b = h.geom_friction[3 * g2 + k];
			pd[18 + k] = pi[5] == 0 ? std::max(a, b) : (pi[5] == 1 ? a : b);
		}
		if (h.collpair_explicit[p]) {
			// <contact><pair>: what the pair states goes on top of the geoms' mix (collpair_param: friction[5] solref[2] solimp[5] margin gap, NaN = not stated)
			const double *pp = h.collpair_param + 14 * p;
			if (h.collpair_condim[p] > 0) pi[4] = h.collpair_condim[p];
			if (!std::isnan(pp[5])) { solref[0] = pp[5]; solref[1] = pp[6]; }
			if (!std::isnan(pp[7])) for (int k = 0; k < 5; k++) solimp[k] = pp[7 + k];
			if (!std::isnan(pp[12])) pd[6] = pp[12];
			if (!std::isnan(pp[13])) pd[7] = pp[13];
			pd[17] = pd[6] - pd[7];
			if (!std::isnan(pp[0])) {  // the pair's five friction numbers: tangent 1, spin, roll 1 in the slots of the geoms' three; tangent 2, roll 2 in the pads
				pi[5] = 4;
				pd[18] = pp[0]; pd[19] = pp[2]; pd[20] = pp[3]; pd[22] = pp[1]; pd[23] = pp[4];
			}
		}
	}
}

void build_limit_records(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	{  // limit records (see mjb_dev.h)
		const int nl = h.njnt + h.ntendon;
		M->lim_d.assign((size_t)24 * (nl > 0 ? nl : 1), 0.0);
		M->lim_i.assign((size_t)4 * (nl > 0 ? nl : 1), 0);
		for (int j = 0; j < h.njnt; j++) {
			double *r = M->lim_d.data() + 24 * j;
			int *ri = M->lim_i.data() + 4 * j;
			ri[0] = !h.jnt_limited[j] ? 0 : (h.jnt_type[j] >= MJB_JNT_SLIDE ? 1 : (h.jnt_type[j] == MJB_JNT_BALL ? 2 : 0));  // (2: a ball joint's angle limit)
			ri[1] = h.jnt_qposadr[j];
			ri[2] = h.jnt_dofadr[j];
			r[0] = h.jnt_range[2 * j]; r[1] = h.jnt_range[2 * j + 1]; r[6] = h.jnt_margin[j];
			r[10] = h.jnt_solref[2 * j]; r[11] = h.jnt_solref[2 * j + 1];
			for (int k = 0; k < 5; k++) r[12 + k] = h.jnt_solimp[5 * j + k];
			r[21] = h.dof_invweight0[h.jnt_dofadr[j]];
		}
		for (int t = 0; t < h.ntendon; t++) {
			double *r = M->lim_d.data() + 24 * (h.njnt + t);
			int *ri = M->lim_i.data() + 4 * (h.njnt + t);
			ri[0] = h.tendon_limited[t] ? 1 : 0;
			ri[1] = t;
			r[0] = h.tendon_range[2 * t]; r[1] = h.tendon_range[2 * t + 1]; r[6] = h.tendon_margin[t];
			r[10] = h.tendon_solref_lim[2 * t]; r[11] = h.tendon_solref_lim[2 * t + 1];
			for (int k = 0; k < 5; k++) r[12 + k] = h.tendon_solimp_lim[5 * t + k];
			r[21] = h.tendon_invweight0[t];
		}
	}
}

// the full frame with the field sizes, then -- from its size -- whether the model runs the row-slot kernels, then the fused frames (which
// depend on that) and where each frame lives
void choose_layouts(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	M->L = compute_layout(*M, false);
	for (int i = 0; i < MJB_F_COUNT; i++) M->field_size[i] = field_elements(*M, i);
	const bool primal = h.nefcmax > 0 && (h.solver == MJB_SOL_NEWTON || h.solver == MJB_SOL_CG);
	M->slot = primal && (h.nefcmax > 256 || mjb_layout_bytes(M->L) > mjb_max_lds_bytes());
	const FusedLayouts f = choose_fused_layouts(*M);
	M->Lc = f.Lc;
	M->Lw = f.Lw;
	M->has_wide = f.has_wide;
	M->hbm_full = M->slot && mjb_layout_bytes(M->L) > mjb_max_lds_bytes();
	M->hbm_fused = M->slot && mjb_layout_bytes(M->Lc) > mjb_max_lds_bytes();
}

void build_actuator_lists(mjb_model *M)
{
	const mjb_model_desc &h = M->h;
	// actuators per dof (CSR, ascending actuator id)
	M->dof_act_adr.assign((size_t)h.nv + 1, 0);
	// (one entry per (dof, actuator) with the actuator's moment arm on that dof: gear for a joint transmission, gear * coefficient for every
	//  joint of a fixed tendon)
	M->act_tendon = 0;
	auto each_arm = [&](auto &&fn) {
		for (int i = 0; i < h.nu; i++) {
			if (h.actuator_trntype[i] == MJB_TRN_SITE) continue;  // (configuration-dependent: the kernels compute its moment, FrameLayout::act_mom)
			const int id = h.actuator_trnid[2 * i];
			if (h.actuator_trntype[i] == MJB_TRN_TENDON) {
				M->act_tendon = 1;
				for (int w = h.tendon_adr[id]; w < h.tendon_adr[id] + h.tendon_num[id]; w++)
					fn(h.jnt_dofadr[h.wrap_objid[w]], i, h.actuator_gear[6 * i] * h.wrap_prm[w]);
			} else
				fn(h.jnt_dofadr[id], i, h.actuator_gear[6 * i]);
		}
	};
	each_arm([&](int dof, int, double) { M->dof_act_adr[dof + 1]++; });
	for (int dd = 0; dd < h.nv; dd++) M->dof_act_adr[dd + 1] += M->dof_act_adr[dd];
	M->dof_act_id.assign((size_t)M->dof_act_adr[h.nv], 0);
	M->dof_act_mom.assign((size_t)M->dof_act_adr[h.nv], 0.0);
	{
		std::vector<int> fill(M->dof_act_adr.begin(), M->dof_act_adr.end() - 1);
		each_arm([&](int dof, int i, double arm) {
			M->dof_act_id[fill[dof]] = i;
			M->dof_act_mom[fill[dof]++] = arm;
		});
	}
}

// a frame beyond one CU's LDS runs only under the row-slot kernels (from HBM)
bool check_frame_fits(const mjb_model *M)
{
	const int frame_bytes = mjb_layout_bytes(M->L);
	if (frame_bytes > mjb_max_lds_bytes() && !M->slot) {
		fail(MJB_EUNSUPPORTED, "mjb_compile: the per-env working set (%d bytes) exceeds one CU's LDS (%d bytes); "
		                       "lower nconmax / nefcmax", frame_bytes, mjb_max_lds_bytes());
		return false;
	}
	return true;
}

}  // namespace

extern "C" {

const char *mjb_last_error(void) { return g_err.c_str(); }

// mjb_compile: the stages above, in this order.  What each one reads of an earlier one's results (all of them read the host copy M->h that
// copy_description makes; nothing reads `desc` after it):
//   check_index_tables       nothing derived -- but every later stage follows the indices it has checked without looking again
//   build_tree_tables        writes M_rowdof / M_coldof / dof_depth / maxdepth, site_act, gravcomp_body, dof_jstart, the packed records
//   build_factor_programme   reads M_rowdof, M_coldof, dof_depth
//   build_masks              reads M_rowdof, M_coldof; its body_dofmask feeds body_dofanc and dof_bodymask inside the stage
//   need_rnepost             the description only; read by classify_lane_env and compute_layout
//   classify_lane_env        reads gravcomp_body, need_rnepost
//   build_integrator_damping, count_friction_rows, build_pair_records, build_limit_records      the description only
//   choose_layouts           compute_layout reads nfriction, need_rnepost, pair_i (largest contact dimension), site_act and -- the fused
//                            frames only -- slot, which the stage decides from the full frame between the two
//   build_sensor_tables      reads L, Lc, Lw
//   build_actuator_lists     the description only
//   check_frame_fits         reads L, slot
mjb_model *mjb_compile(const mjb_model_desc *desc)
{
	if (!desc) {
		fail(MJB_EINVAL, "mjb_compile: null desc");
		return nullptr;
	}
	if (!check_description(*desc)) return nullptr;
	std::unique_ptr<mjb_model> owner(new (std::nothrow) mjb_model);
	mjb_model *M = owner.get();
	if (!M) {
		fail(MJB_ENOMEM, "mjb_compile: out of memory");
		return nullptr;
	}
	copy_description(M, *desc);
	if (!check_index_tables(M->h)) return nullptr;
	if (!build_tree_tables(M)) return nullptr;
	build_factor_programme(M);
	build_masks(M);
	M->need_rnepost = needs_rnepost(M->h) ? 1 : 0;
	classify_lane_env(M);
	if (!build_integrator_damping(M)) return nullptr;
	count_friction_rows(M);
	build_pair_records(M);
	build_limit_records(M);
	choose_layouts(M);
	build_sensor_tables(M);
	build_actuator_lists(M);
	if (!check_frame_fits(M)) return nullptr;
	clear_error();
	return owner.release();
}

void mjb_free_model(mjb_model *m) { delete m; }

int mjb_field_size(const mjb_model *m, int field)
{
	if (!m || field < 0 || field >= MJB_F_COUNT) return fail(MJB_EINVAL, "mjb_field_size: bad argument");
	return m->field_size[field];
}
int mjb_field_is_int(int field) { return field >= 0 && field < MJB_F_COUNT && kFields[field].kind == 3; }
int mjb_field_is_state(int field) { return field >= 0 && field < MJB_F_COUNT && kFields[field].kind == 0; }
const char *mjb_field_name(int field) { return field >= 0 && field < MJB_F_COUNT ? kFields[field].name : ""; }
int mjb_frame_doubles(const mjb_model *m) { return m ? m->L.ndouble + m->L.nint / 2 : fail(MJB_EINVAL, "null model"); }
int mjb_frame_bytes(const mjb_model *m, int fused)
{
	if (!m) return fail(MJB_EINVAL, "null model");
	const FrameLayout &L = fused == 2 ? m->Lw : (fused ? m->Lc : m->L);  // (2: the wide fused frame of kernel variant 4, == 1 when the model has none)
	return mjb_layout_bytes(L);
}
int mjb_frame_offset(const mjb_model *m, int field, int fused)
{
	if (!m || field < 0 || field >= MJB_F_COUNT) return fail(MJB_EINVAL, "bad model / field");
	const FrameLayout &L = fused ? m->Lc : m->L;
	return field_slot(L, field);
}
int mjb_model_split_step(const mjb_model *m) { return m ? m->sm_topo : -1; }
int mjb_model_frame_info(const mjb_model *m, int *full_hbm, int *fused_hbm)
{
	if (full_hbm) *full_hbm = m && m->hbm_full ? 1 : 0;
	if (fused_hbm) *fused_hbm = m && m->hbm_fused ? 1 : 0;
	return m ? (m->slot ? 1 : 0) : fail(MJB_EINVAL, "null model");
}
int mjb_model_lane_env(const mjb_model *m) { return m ? m->le_topo : -1; }
int mjb_model_lane_env_tape(const mjb_model *m, double *out, int cap)
{
	if (!m || m->le_topo == MJB_LE_TOPO_NONE) return -1;
	const int n = (int)m->le_tape.size();
	if (out && cap >= n) memcpy(out, m->le_tape.data(), (size_t)n * sizeof(double));
	return n;
}
int mjb_model_lane_env_overlay(const mjb_model *m, double *out, int cap)
{
	if (!m || m->le_topo == MJB_LE_TOPO_NONE) return -1;
	const int n = mjb_lane_env_overlay_slots(&m->h);
	if (out && cap >= n) mjb_lane_env_overlay_row(&m->h, nullptr, nullptr, out);
	return n;
}
int mjb_env_mass_stride(const mjb_model *m)
{
	if (!m) return fail(MJB_EINVAL, "null model");
	return mjb_env_block_layout(m->h).mass_doubles;
}

int mjb_env_joint_stride(const mjb_model *m)
{
	if (!m) return fail(MJB_EINVAL, "null model");
	const EnvBlockLayout B = mjb_env_block_layout(m->h);
	return mjb_env_joint_packed(B, B.doubles);
}

// ---- mj_setConst for new body masses (callbacks.cpp:251-256, :582), host side, plain C++ ----
// What mj_setConst's set0 stage derives from the masses at qpos0: body_subtreemass, dof_invweight0 (diagonal of M^-1; joint-wise
// mean over the 3 dofs of a ball joint / each half of a free joint), body_invweight0 (mean translational / rotational diagonal of
// J M^-1 J' at the body's inertial frame; 0 for bodies welded to the world), tendon_invweight0 (J_t M^-1 J_t') and
// stat.meaninertia (mean diagonal of M).  M is assembled from body Jacobians (m Jp'Jp + Jr' R I R' Jr + armature), the same
// formulation as mujoco_ros_pkgs_amd/refdyn.py, which tests/test_setconst_cpp.py compares it with.
namespace {
struct SC {  // tiny dense helpers (row-major)
	static void quat2mat(const double *q, double *R)
	{
		const double w = q[0], x = q[1], y = q[2], z = q[3];
		R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
		R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
		R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
	}
	static void qmul(const double *a, const double *b, double *o)
	{
		const double r[4] = { a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
			                  a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0] };
		for (int k = 0; k < 4; k++) o[k] = r[k];
	}
	static void mv(const double *R, const double *v, double *o)
	{
		const double r[3] = { R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2] };
		for (int k = 0; k < 3; k++) o[k] = r[k];
	}
	static void cross(const double *a, const double *b, double *o)
	{
		const double r[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
		for (int k = 0; k < 3; k++) o[k] = r[k];
	}
};
}  // namespace

int mjb_derive_mass_params(const mjb_model *model, const double *body_mass, const double *body_inertia, double *out)
{
	if (!model || !body_mass || !out) return fail(MJB_EINVAL, "mjb_derive_mass_params: bad argument");
	return mjb_derive_mass_params_armature(model, body_mass, body_inertia, nullptr, out);
}

int mjb_derive_mass_params_armature(const mjb_model *model, const double *body_mass, const double *body_inertia, const double *dof_armature, double *out)
{
	if (!model || !body_mass || !out) return fail(MJB_EINVAL, "mjb_derive_mass_params_armature: bad argument");
	const mjb_model_desc &h = model->h;
	const double *armature = dof_armature ? dof_armature : h.dof_armature;
	const int nb = h.nbody, nv = h.nv, nj = h.njnt, nt = h.ntendon;
	const double *inertia = body_inertia ? body_inertia : h.body_inertia;
	const EnvBlockLayout B = mjb_env_block_layout(h);  // out: the mass section of an env's block
	for (int b = 0; b < nb; b++) {
		out[B.body_mass + b] = body_mass[b];
		out[B.body_subtreemass + b] = body_mass[b];
		for (int k = 0; k < 3; k++) out[B.body_inertia + 3 * b + k] = inertia[3 * b + k];
		out[B.body_invweight0 + 2 * b] = out[B.body_invweight0 + 2 * b + 1] = 0;
	}
	for (int b = nb - 1; b > 0; b--) out[B.body_subtreemass + h.body_parentid[b]] += out[B.body_subtreemass + b];
	for (int i = 0; i < nv; i++) out[B.dof_invweight0 + i] = 0;
	for (int t = 0; t < nt; t++) out[B.tendon_invweight0 + t] = 0;
	out[B.meaninertia] = 1.0;
	if (nv == 0) return MJB_OK;
	// kinematics at qpos0
	std::vector<double> xpos(3 * nb, 0.0), xquat(4 * nb, 0.0), xmat(9 * nb, 0.0), xipos(3 * nb, 0.0), ximat(9 * nb, 0.0), xanchor(3 * std::max(1, nj), 0.0),
	    xaxis(3 * std::max(1, nj), 0.0);
	xquat[0] = 1;
	SC::quat2mat(&xquat[0], &xmat[0]);
	for (int b = 1; b < nb; b++) {
		const int p = h.body_parentid[b], ja = h.body_jntadr[b], jn = h.body_jntnum[b];
		double pos[3], q[4];
		if (jn == 1 && h.jnt_type[ja] == MJB_JNT_FREE) {
			const int qa = h.jnt_qposadr[ja];
			double nrm = 0;
			for (int k = 0; k < 4; k++) nrm += h.qpos0[qa + 3 + k] * h.qpos0[qa + 3 + k];
			nrm = std::sqrt(nrm);
			for (int k = 0; k < 3; k++) pos[k] = h.qpos0[qa + k];
			for (int k = 0; k < 4; k++) q[k] = h.qpos0[qa + 3 + k] / nrm;
			for (int k = 0; k < 3; k++) { xanchor[3 * ja + k] = pos[k]; xaxis[3 * ja + k] = h.jnt_axis[3 * ja + k]; }
		} else {
			double v[3];
			SC::mv(&xmat[9 * p], &h.body_pos[3 * b], v);
			for (int k = 0; k < 3; k++) pos[k] = xpos[3 * p + k] + v[k];
			SC::qmul(&xquat[4 * p], &h.body_quat[4 * b], q);
			for (int j = ja; j < ja + jn; j++) {
				double R[9], w[3];
				SC::quat2mat(q, R);
				SC::mv(R, &h.jnt_axis[3 * j], &xaxis[3 * j]);
				SC::mv(R, &h.jnt_pos[3 * j], w);
				for (int k = 0; k < 3; k++) xanchor[3 * j + k] = pos[k] + w[k];
				if (h.jnt_type[j] == MJB_JNT_BALL) {  // (hinge / slide sit at qpos0: no motion)
					const int qa = h.jnt_qposadr[j];
					double ql[4], nrm = 0;
					for (int k = 0; k < 4; k++) nrm += h.qpos0[qa + k] * h.qpos0[qa + k];
					nrm = std::sqrt(nrm);
					for (int k = 0; k < 4; k++) ql[k] = h.qpos0[qa + k] / nrm;
					SC::qmul(q, ql, q);
					SC::quat2mat(q, R);
					SC::mv(R, &h.jnt_pos[3 * j], w);
					for (int k = 0; k < 3; k++) pos[k] = xanchor[3 * j + k] - w[k];
				}
			}
		}
		double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
		for (int k = 0; k < 3; k++) xpos[3 * b + k] = pos[k];
		for (int k = 0; k < 4; k++) xquat[4 * b + k] = q[k] / nrm;
		SC::quat2mat(&xquat[4 * b], &xmat[9 * b]);
	}
	for (int b = 0; b < nb; b++) {
		double v[3], Ri[9];
		SC::mv(&xmat[9 * b], &h.body_ipos[3 * b], v);
		for (int k = 0; k < 3; k++) xipos[3 * b + k] = xpos[3 * b + k] + v[k];
		SC::quat2mat(&h.body_iquat[4 * b], Ri);
		for (int r = 0; r < 3; r++)
			for (int c = 0; c < 3; c++) {
				double a = 0;
				for (int k = 0; k < 3; k++) a += xmat[9 * b + 3 * r + k] * Ri[3 * k + c];
				ximat[9 * b + 3 * r + c] = a;
			}
	}
	// Jacobians of a point fixed to `body` (3 x nv each)
	auto jac = [&](int body, const double *point, std::vector<double> &jp, std::vector<double> &jr) {
		std::fill(jp.begin(), jp.end(), 0.0);
		std::fill(jr.begin(), jr.end(), 0.0);
		for (int b = body; b > 0; b = h.body_parentid[b])
			for (int j = h.body_jntadr[b]; j < h.body_jntadr[b] + h.body_jntnum[b]; j++) {
				const int d = h.jnt_dofadr[j], t = h.jnt_type[j];
				auto rot_dof = [&](int dof, const double *ax, const double *about) {
					const double off[3] = { point[0] - about[0], point[1] - about[1], point[2] - about[2] };
					double c[3];
					SC::cross(ax, off, c);
					for (int k = 0; k < 3; k++) { jr[(size_t)k * nv + dof] = ax[k]; jp[(size_t)k * nv + dof] = c[k]; }
				};
				if (t == MJB_JNT_HINGE) rot_dof(d, &xaxis[3 * j], &xanchor[3 * j]);
				else if (t == MJB_JNT_SLIDE) for (int k = 0; k < 3; k++) jp[(size_t)k * nv + d] = xaxis[3 * j + k];
				else {
					const int r0 = t == MJB_JNT_FREE ? d + 3 : d;
					if (t == MJB_JNT_FREE) for (int k = 0; k < 3; k++) jp[(size_t)k * nv + d + k] = 1.0;
					for (int k = 0; k < 3; k++) {
						const double ax[3] = { xmat[9 * b + k], xmat[9 * b + 3 + k], xmat[9 * b + 6 + k] };
						rot_dof(r0 + k, ax, t == MJB_JNT_FREE ? &xpos[3 * b] : &xanchor[3 * j]);
					}
				}
			}
	};
	std::vector<double> M((size_t)nv * nv, 0.0), jp((size_t)3 * nv), jr((size_t)3 * nv);
	for (int i = 0; i < nv; i++) M[(size_t)i * nv + i] = armature[i];
	for (int b = 1; b < nb; b++) {
		const double mb = body_mass[b], *I = inertia + 3 * b;
		if (mb == 0 && I[0] == 0 && I[1] == 0 && I[2] == 0) continue;
		jac(b, &xipos[3 * b], jp, jr);
		double Iw[9];  // R diag(I) R'
		for (int r = 0; r < 3; r++)
			for (int c = 0; c < 3; c++) {
				double a = 0;
				for (int k = 0; k < 3; k++) a += ximat[9 * b + 3 * r + k] * I[k] * ximat[9 * b + 3 * c + k];
				Iw[3 * r + c] = a;
			}
		for (int i = 0; i < nv; i++)
			for (int j = 0; j < nv; j++) {
				double a = 0;
				for (int k = 0; k < 3; k++) a += mb * jp[(size_t)k * nv + i] * jp[(size_t)k * nv + j];
				for (int r = 0; r < 3; r++) {
					double t = 0;
					for (int c = 0; c < 3; c++) t += Iw[3 * r + c] * jr[(size_t)c * nv + j];
					a += jr[(size_t)r * nv + i] * t;
				}
				M[(size_t)i * nv + j] += a;
			}
	}
	double mean = 0;
	for (int i = 0; i < nv; i++) mean += M[(size_t)i * nv + i];
	out[B.meaninertia] = mean / nv;
	// M^-1 by Gauss-Jordan with partial pivoting (nv <= 64)
	std::vector<double> A(M), Minv((size_t)nv * nv, 0.0);
	for (int i = 0; i < nv; i++) Minv[(size_t)i * nv + i] = 1.0;
	for (int c = 0; c < nv; c++) {
		int piv = c;
		for (int r = c + 1; r < nv; r++)
			if (std::fabs(A[(size_t)r * nv + c]) > std::fabs(A[(size_t)piv * nv + c])) piv = r;
		if (std::fabs(A[(size_t)piv * nv + c]) < 1e-300) return fail(MJB_EINVAL, "mjb_derive_mass_params: singular joint-space inertia (dof %d)", c);
		if (piv != c)
			for (int k = 0; k < nv; k++) { std::swap(A[(size_t)piv * nv + k], A[(size_t)c * nv + k]); std::swap(Minv[(size_t)piv * nv + k], Minv[(size_t)c * nv + k]); }
		const double d = 1.0 / A[(size_t)c * nv + c];
		for (int k = 0; k < nv; k++) { A[(size_t)c * nv + k] *= d; Minv[(size_t)c * nv + k] *= d; }
		for (int r = 0; r < nv; r++) {
			if (r == c) continue;
			const double f = A[(size_t)r * nv + c];
			if (f == 0) continue;
			for (int k = 0; k < nv; k++) { A[(size_t)r * nv + k] -= f * A[(size_t)c * nv + k]; Minv[(size_t)r * nv + k] -= f * Minv[(size_t)c * nv + k]; }
		}
	}
	auto quad = [&](const double *ja, const double *jb) {  // ja' M^-1 jb for two nv-vectors
		double a = 0;
		for (int i = 0; i < nv; i++) {
			if (ja[i] == 0) continue;
			double t = 0;
			for (int j = 0; j < nv; j++) t += Minv[(size_t)i * nv + j] * jb[j];
			a += ja[i] * t;
		}
		return a;
	};
	for (int b = 1; b < nb; b++) {
		if (h.body_weldid[b] == 0) continue;
		jac(b, &xipos[3 * b], jp, jr);
		double tr = 0, ro = 0;
		for (int k = 0; k < 3; k++) { tr += quad(&jp[(size_t)k * nv], &jp[(size_t)k * nv]); ro += quad(&jr[(size_t)k * nv], &jr[(size_t)k * nv]); }
		out[B.body_invweight0 + 2 * b] = tr / 3;
		out[B.body_invweight0 + 2 * b + 1] = ro / 3;
	}
	for (int j = 0; j < nj; j++) {
		const int d = h.jnt_dofadr[j], t = h.jnt_type[j];
		auto tr3 = [&](int a) { return (Minv[(size_t)a * nv + a] + Minv[(size_t)(a + 1) * nv + a + 1] + Minv[(size_t)(a + 2) * nv + a + 2]) / 3; };
		double *w = out + B.dof_invweight0 + d;  // the joint's dofs
		if (t == MJB_JNT_HINGE || t == MJB_JNT_SLIDE) w[0] = Minv[(size_t)d * nv + d];
		else {
			w[0] = w[1] = w[2] = tr3(d);
			if (t != MJB_JNT_BALL) w[3] = w[4] = w[5] = tr3(d + 3);  // (free joint: its rotational half)
		}
	}
	std::vector<double> jt((size_t)nv);
	for (int t = 0; t < nt; t++) {
		std::fill(jt.begin(), jt.end(), 0.0);
		for (int w = h.tendon_adr[t]; w < h.tendon_adr[t] + h.tendon_num[t]; w++) jt[h.jnt_dofadr[h.wrap_objid[w]]] += h.wrap_prm[w];
		out[B.tendon_invweight0 + t] = quad(jt.data(), jt.data());
	}
	return MJB_OK;
}

}  // extern "C"

// ---- the device model blob: [ints | doubles].  The arrays of the description come first in each part (hint / hdbl, where ioff / doff put them);
// behind them the derived tables, each named ONCE below, in blob order: the image's size, the copies, the offsets in the DevModel, the rebase onto the
// device address and mjb_debug_blob_digest all walk these two lists.
namespace {
struct IntTable {
	std::vector<int> mjb_model::*src;
	mjb_ciptr DevModel::*dst;
};
struct DblTable {
	std::vector<double> mjb_model::*src;
	mjb_cdptr DevModel::*dst;
	bool tape;  // starts on a 64-byte boundary of the blob (wide scalar loads off one base); a null pointer when empty
};
#define T(src, dst) { &mjb_model::src, &DevModel::dst }
const IntTable kIntTables[] = {  // each on a 16-byte boundary (wide scalar loads)
	T(M_rowdof, M_rowdof), T(M_coldof, M_coldof), T(dof_depth, dof_depth), T(dof_jstart, dof_jstart), T(body_rec, body_rec), T(body_rec2, body_rec2),
	T(dof_rec, dof_rec), T(fac_ops, fac_ops), T(fac_beg, fac_beg), T(body_dofmask, body_dofmask), T(body_submask, body_submask), T(M_dense, M_dense),
	T(M_sym, M_sym), T(body_anc, body_anc), T(dof_bodymask, dof_bodymask), T(sens_copy, sens_copy), T(sens_slow, sens_slow), T(dof_act_adr, dof_act_adr),
	T(dof_act_id, dof_act_id), T(pair_i, pair_i), T(lim_i, lim_i), T(body_dofanc, body_dofanc), T(dof_rec2, dof_rec2), T(jnt_rec, jnt_rec),
	T(flv_hdr, flv_hdr), T(flv_rec, flv_rec), T(flv_ent, flv_ent), T(site_act, site_act), T(gravcomp_body, gravcomp_body),
};
#undef T
const DblTable kDblTables[] = {
	{ &mjb_model::pair_d, &DevModel::pair_d, false },    { &mjb_model::lim_d, &DevModel::lim_d, false },
	{ &mjb_model::sub_S, &DevModel::sub_S, false },      { &mjb_model::damp_int, &DevModel::dof_damping_int, false },
	{ &mjb_model::dof_act_mom, &DevModel::dof_act_mom, false }, { &mjb_model::le_tape, &DevModel::le_tape, true },
};
// The double part has always started this many ints behind the int tables' unpadded sizes (once a bound on their alignment padding).  Kept as a
// constant of the layout: the offsets of the double tables, and with them the tape's position, stay the ones every measurement was taken on.
const size_t kIntPartSlack = 112;
static_assert(3 * (sizeof kIntTables / sizeof kIntTables[0]) <= kIntPartSlack, "the int tables' alignment padding (at most 3 ints each) must fit the gap");
const size_t kTailBytes = 16;  // behind the last table, as ever: a 16-byte load that starts inside it ends inside the allocation
const uintptr_t kNullOffset = ~(uintptr_t)0;

// f(pointer member, elements of its table, the alignment in bytes the layout promises it) for every pointer member of a DevModel: the description's
// arrays, then the two lists
template <typename DM, typename F> void each_blob_pointer(const mjb_model &M, DM &dm, F f)
{
	const mjb_model_desc &h = M.h;
#define MJB_SIZE(name)
#define MJB_OPT_I(name)
#define MJB_OPT_D(name, n)
#define MJB_ARR_I(name, rows, cols) f(dm.name, (size_t)h.rows * (cols), sizeof(int));
#define MJB_ARR_D(name, rows, cols) f(dm.name, (size_t)h.rows * (cols), sizeof(double));
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	for (const IntTable &t : kIntTables) f(dm.*t.dst, (M.*t.src).size(), (size_t)16);
	for (const DblTable &t : kDblTables) f(dm.*t.dst, (M.*t.src).size(), t.tape ? (size_t)64 : sizeof(double));
}
template <typename P> void set_offset(P &p, uintptr_t off) { p = (P)off; }
}  // namespace

ModelBlob build_model_blob(const mjb_model &M)
{
	ModelBlob B;
	const mjb_model_desc &h = M.h;
	const size_t ni = M.hint.size(), nd = M.hdbl.size();
	// where everything goes (ints from the image's start, doubles from the double part's)
	size_t it = ni, unpadded = ni;
	std::vector<size_t> iat, dat;
	for (const IntTable &t : kIntTables) {
		it = (it + 3) & ~size_t(3);
		iat.push_back(it);
		it += (M.*t.src).size();
		unpadded += (M.*t.src).size();
	}
	B.dbl_offset = ((unpadded + kIntPartSlack) * sizeof(int) + 15) & ~size_t(15);
	size_t dt = nd;
	for (const DblTable &t : kDblTables) {
		const size_t n = (M.*t.src).size();
		while (t.tape && n && (B.dbl_offset + dt * sizeof(double)) % 64) dt++;
		dat.push_back(dt);
		dt += n;
	}
	B.image.assign(B.dbl_offset + dt * sizeof(double) + kTailBytes, 0);
	int *hi = reinterpret_cast<int *>(B.image.data());
	double *hd = reinterpret_cast<double *>(B.image.data() + B.dbl_offset);
	if (ni) memcpy(hi, M.hint.data(), ni * sizeof(int));
	if (nd) memcpy(hd, M.hdbl.data(), nd * sizeof(double));
	DevModel &dm = B.dm;
	{
		size_t ii = 0, dj = 0;
#define MJB_SIZE(name) dm.name = h.name;
#define MJB_OPT_I(name) dm.name = h.name;
#define MJB_OPT_D(name, n) for (int k = 0; k < n; k++) dm.name[k] = h.name[k];
#define MJB_ARR_I(name, rows, cols) set_offset(dm.name, M.ioff[ii++] * sizeof(int));
#define MJB_ARR_D(name, rows, cols) set_offset(dm.name, B.dbl_offset + M.doff[dj++] * sizeof(double));
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	}
	for (size_t k = 0; k < iat.size(); k++) {
		const std::vector<int> &v = M.*kIntTables[k].src;
		if (!v.empty()) memcpy(hi + iat[k], v.data(), v.size() * sizeof(int));
		set_offset(dm.*kIntTables[k].dst, iat[k] * sizeof(int));
	}
	for (size_t k = 0; k < dat.size(); k++) {
		const std::vector<double> &v = M.*kDblTables[k].src;
		if (!v.empty()) memcpy(hd + dat[k], v.data(), v.size() * sizeof(double));
		set_offset(dm.*kDblTables[k].dst, kDblTables[k].tape && v.empty() ? kNullOffset : B.dbl_offset + dat[k] * sizeof(double));
	}
	B.pair_i_offset = (uintptr_t)dm.pair_i;
	dm.kin_rounds = M.kin_rounds;
	dm.dofanc_max = M.dofanc_max;
	dm.flv_n = M.flv_n;
	dm.need_rnepost = M.need_rnepost;
	dm.act_tendon = M.act_tendon;
	dm.nsite_act = (int)M.site_act.size();
	dm.ngravcomp = (int)M.gravcomp_body.size();
	dm.sub_nt = M.sub_nt;
	for (int k = 0; k < 3; k++) {
		dm.sens_ncopy[k] = M.sens_ncopy[k];
		dm.sens_nslow[k] = M.sens_nslow[k];
	}
	dm.sens_ncopy_max = M.sens_ncopy_max ? M.sens_ncopy_max : 1;
	dm.eulerdamp = M.eulerdamp;
	dm.nfriction = M.nfriction;
	dm.maxdepth = M.maxdepth;
	return B;
}

void rebase_model_blob(const mjb_model &M, DevModel &dm, const void *base)
{
	each_blob_pointer(M, dm, [base](auto &p, size_t, size_t) {
		typedef std::remove_reference_t<decltype(p)> P;
		const uintptr_t off = (uintptr_t)p;
		p = off == kNullOffset ? (P) nullptr : (P)(static_cast<const unsigned char *>(base) + off);
	});
}

// ---- mjb_debug_model_digest: 64-bit FNV-1a over the members of a compiled model, in declaration order (never over raw struct bytes) ----
namespace {
struct Fnv {
	unsigned long long h = 14695981039346656037ull;
	void bytes(const void *p, size_t n)
	{
		const unsigned char *c = static_cast<const unsigned char *>(p);
		for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 1099511628211ull;
	}
	void operator()(int v) { bytes(&v, sizeof v); }
	void operator()(bool v) { (*this)(v ? 1 : 0); }
	void operator()(double v) { bytes(&v, sizeof v); }  // (the bit pattern: NaN marks "not stated" in collpair_param)
	void operator()(size_t v) { const unsigned long long w = v; bytes(&w, sizeof w); }
	template <typename T> void operator()(const std::vector<T> &v)
	{
		(*this)(v.size());
		for (const T &x : v) (*this)(x);
	}
	void operator()(const FrameLayout &L)
	{
		static_assert(std::has_unique_object_representations_v<FrameLayout>, "FrameLayout is hashed bytewise: ints only, no padding");
		bytes(&L, sizeof L);
	}
};
}  // namespace

extern "C" int mjb_debug_model_digest(const mjb_model *m, unsigned long long out[4])
{
	if (!m || !out) return fail(MJB_EINVAL, "mjb_debug_model_digest: bad argument");
	Fnv d0, d1, d2, d3;
	// [0] the copied description: sizes and options, then the arrays and where each one starts
#define MJB_SIZE(name) d0(m->h.name);
#define MJB_OPT_I(name) d0(m->h.name);
#define MJB_OPT_D(name, n) for (int k = 0; k < (n); k++) d0(m->h.name[k]);
#define MJB_ARR_I(name, rows, cols)
#define MJB_ARR_D(name, rows, cols)
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	d0(m->hint); d0(m->hdbl); d0(m->ioff); d0(m->doff);
	// [1] every derived table and scalar
	d1(m->M_rowdof); d1(m->M_coldof); d1(m->dof_depth); d1(m->dof_jstart); d1(m->body_rec); d1(m->body_rec2); d1(m->dof_rec); d1(m->fac_ops);
	d1(m->fac_beg); d1(m->body_dofmask); d1(m->body_submask); d1(m->M_dense); d1(m->body_anc); d1(m->dof_bodymask); d1(m->M_sym); d1(m->body_dofanc);
	d1(m->dof_rec2); d1(m->jnt_rec); d1(m->flv_hdr); d1(m->flv_rec); d1(m->flv_ent);
	d1(m->sens_copy); d1(m->sens_slow); d1(m->dof_act_adr); d1(m->dof_act_id);
	d1(m->pair_i); d1(m->pair_d); d1(m->sub_S); d1(m->lim_d); d1(m->dof_act_mom); d1(m->act_tendon); d1(m->site_act); d1(m->gravcomp_body);
	d1(m->damp_int); d1(m->lim_i);
	d1(m->eulerdamp); d1(m->maxdepth); d1(m->kin_rounds); d1(m->need_rnepost); d1(m->nfriction); d1(m->sub_nt); d1(m->dofanc_max); d1(m->flv_n);
	// [2] the layouts and what is decided with them
	d2(m->L); d2(m->Lc); d2(m->Lw);
	for (int v : m->field_size) d2(v);
	d2(m->has_wide); d2(m->slot); d2(m->hbm_full); d2(m->hbm_fused);
	for (int st = 0; st < 3; st++) d2(m->sens_ncopy[st]);
	for (int st = 0; st < 3; st++) d2(m->sens_nslow[st]);
	d2(m->sens_ncopy_max);
	// [3] the lane = env / split-step classification
	d3(m->le_topo); d3(m->sm_topo); d3(m->le_tape);
	out[0] = d0.h; out[1] = d1.h; out[2] = d2.h; out[3] = d3.h;
	return MJB_OK;
}

// ---- mjb_debug_blob_digest: the device model blob as build_model_blob lays it out.  [0] where every pointer member of the DevModel points, as an
// offset from the blob's base, in declaration order (a null pointer: ~0); [1] what each table holds, read through those offsets over the table's
// length (never the raw image: padding and slack stay out); [2] every other member of the DevModel, in declaration order ----
extern "C" int mjb_debug_blob_digest(const mjb_model *m, unsigned long long out[3])
{
	if (!m || !out) return fail(MJB_EINVAL, "mjb_debug_blob_digest: bad argument");
	const ModelBlob B = build_model_blob(*m);
	const DevModel &dm = B.dm;
	struct Entry { size_t member, offset, bytes, align; };  // (member: where the pointer sits inside the DevModel)
	std::vector<Entry> tab;
	each_blob_pointer(*m, dm, [&](const auto &p, size_t n, size_t align) {
		tab.push_back({ (size_t)(reinterpret_cast<const char *>(&p) - reinterpret_cast<const char *>(&dm)), (size_t)(uintptr_t)p, n * sizeof(*p), align });
	});
	// the layout's promises, checked on the way: alignment (16 bytes for the int tables, 64 for the tape), no table overlaps the next, all inside the image
	std::sort(tab.begin(), tab.end(), [](const Entry &a, const Entry &b) { return a.offset != b.offset ? a.offset < b.offset : a.bytes < b.bytes; });  // (an empty table may share its offset with the next)
	size_t end = 0;
	for (const Entry &e : tab) {
		if (e.offset == kNullOffset) continue;
		if (e.offset % e.align) return fail(MJB_EINVAL, "mjb_debug_blob_digest: the table at byte %zu is not on a %zu-byte boundary", e.offset, e.align);
		if (e.offset < end) return fail(MJB_EINVAL, "mjb_debug_blob_digest: the table at byte %zu overlaps the one before it", e.offset);
		end = e.offset + e.bytes;
	}
	if (end > B.image.size()) return fail(MJB_EINVAL, "mjb_debug_blob_digest: the last table ends outside the image");
	std::sort(tab.begin(), tab.end(), [](const Entry &a, const Entry &b) { return a.member < b.member; });
	Fnv d0, d1, d2;
	for (const Entry &e : tab) {
		const bool null = e.offset == kNullOffset;
		d0(null ? ~(size_t)0 : e.offset);
		d1(null ? (size_t)0 : e.bytes);
		if (!null) d1.bytes(B.image.data() + e.offset, e.bytes);
	}
#define MJB_SIZE(name) d2(dm.name);
#define MJB_OPT_I(name) d2(dm.name);
#define MJB_OPT_D(name, n) for (int k = 0; k < (n); k++) d2(dm.name[k]);
#define MJB_ARR_I(name, rows, cols)
#define MJB_ARR_D(name, rows, cols)
#include "../../include/mjb_model_fields.def"
#undef MJB_SIZE
#undef MJB_OPT_I
#undef MJB_OPT_D
#undef MJB_ARR_I
#undef MJB_ARR_D
	d2(dm.flv_n); d2(dm.act_tendon);
	for (int k = 0; k < 3; k++) d2(dm.sens_ncopy[k]);
	for (int k = 0; k < 3; k++) d2(dm.sens_nslow[k]);
	d2(dm.sens_ncopy_max); d2(dm.eulerdamp); d2(dm.nfriction); d2(dm.need_rnepost); d2(dm.kin_rounds); d2(dm.maxdepth); d2(dm.sub_nt); d2(dm.dofanc_max);
	d2(dm.nsite_act); d2(dm.ngravcomp);
	out[0] = d0.h; out[1] = d1.h; out[2] = d2.h;
	return MJB_OK;
}
