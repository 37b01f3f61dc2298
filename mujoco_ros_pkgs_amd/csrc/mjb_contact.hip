// mjb_contact.hip -- batched contact wrenches (mjb_contact_*): mj_contactForce of every contact and the net force, torque, normal force, count and
// smallest distance between the two geom sets of every configured query, for every env in one launch, fp64.
//
// The kernel is bound by memory: a frame is tens of KB per env and a live contact needs a few hundred bytes of it.  A block of 256 lanes takes `epb`
// whole envs with all their queries, or -- a query list too long for that -- a tile of one env's queries (mjb_contact_shape), and walks the envs'
// contacts in tiles of `ct`.  The phases of a tile, a barrier between any two:
//   1  Stage.  The first ncon records of contact_geom / dim / efc_address / frame / pos / dist / friction go into the contacts' LDS slots element by
//      element, consecutive lanes reading consecutive addresses; then, the ints being there, the rows of efc_force those contacts address.  (Once per
//      block, ahead of the tiles: the queries' masks as bit words, xpos of their reference bodies, ncon of the envs.)
//   2  Decode.  One lane per (env, contact): lf (mj_contactForce), F = frame' lf[0:3], T = frame' lf[3:6], written over the slot's inputs.  CONTACTS
//      goes out from there, one element per lane.
//   3  Sum.  One lane per (env, query) walks the env's contacts of the tile in ascending c, tests the membership bits of the two geoms and adds
//      sign (F, T + (pos - r_q) x F), lf[0], 1 and min(dist) to accumulators it keeps in registers across the tiles.
// Behind the tiles the wrenches pass through LDS and every output goes out one element per lane.
// Every value is computed by one lane, in ascending c, from operands that do not depend on the block's shape: no result depends on the launch.  The
// signed term is formed unsigned and then added or subtracted, so (B, A) is the negation of (A, B) to the bit (an exact zero is +0.0 in both).
//
// contact_lf below restates contact_force of mjb_step.hip (mj_contactForce) on operands staged in LDS: that one reads the frame through the step
// kernels' CModel / CLayout views, and sharing it would have put a new header under every step kernel's code object.
#include <hip/hip_runtime.h>

#include "mjb_contact.h"
#include "mjb_dev.h"
#include "mjb_math.h"

namespace {

// rows of efc_force a contact of dimension dim owns
DEVI int contact_rows(int dim, bool elliptic) { return dim == 1 ? 1 : (elliptic ? dim : 2 * (dim - 1)); }

// mj_contactForce from the contact's rows of efc_force (fr[MJB_CON_ROWS]) and its friction coefficients: normal first; the arithmetic of contact_force (mjb_step.hip)
DEVI void contact_lf(int dim, bool elliptic, const double *fr, const double *friction, double *res)
{
	for (int k = 0; k < 6; k++) res[k] = 0;
	if (dim == 1) {
		res[0] = fr[0];
	} else if (elliptic) {
		for (int k = 0; k < 6; k++)
			if (k < dim) res[k] = fr[k];
	} else {
		for (int k = 0; k < MJB_CON_ROWS; k++)
			if (k < 2 * (dim - 1)) res[0] += fr[k];
		for (int k = 0; k < 5; k++)
			if (k < dim - 1) res[1 + k] = (fr[2 * k] - fr[2 * k + 1]) * friction[k];
	}
}

DEVI bool mask_bit(const unsigned int *w, int g) { return (w[g >> 5] >> (g & 31)) & 1u; }

__global__ void __launch_bounds__(MJB_CON_BLOCK) mjb_contact_kernel(const KernelParams MJB_AS4 *__restrict__ P, const unsigned int *__restrict__ tab, int nquery, int epb, int qpb, int ct,
                                                                    int nwords, int query_blocks, double *__restrict__ out_wrench, double *__restrict__ out_normal,
                                                                    int *__restrict__ out_count, double *__restrict__ out_dist, double *__restrict__ out_contacts)
{
	extern __shared__ __attribute__((aligned(16))) double lds[];
	const DevModel MJB_AS4 &m = P->m;
	const DevState MJB_AS4 &s = P->s;
	const FrameLayout MJB_AS4 &L = P->L;
	const int nenv = s.nenv, nconmax = m.nconmax, ngeom = m.ngeom, nefcmax = m.nefcmax;
	const bool elliptic = m.cone == MJB_CONE_ELLIPTIC;
	const int env_block = (int)(blockIdx.x / (unsigned int)query_blocks), qblock = (int)(blockIdx.x % (unsigned int)query_blocks);
	const int env0 = env_block * epb, q0 = qblock * qpb;
	const int nq = min(qpb, nquery - q0);  // queries of this block
	const int t = (int)threadIdx.x, NT = (int)blockDim.x;
	const unsigned int *__restrict__ gmask = tab + (size_t)q0 * 2 * nwords;
	const int *__restrict__ refbody = reinterpret_cast<const int *>(tab + (size_t)nquery * 2 * nwords) + q0;
	// the LDS plan (mjb_contact.h)
	double *slots = lds, *rq = slots + (size_t)epb * ct * MJB_CON_SLOT, *wout = rq + (size_t)epb * qpb * 3;
	unsigned int *masks = reinterpret_cast<unsigned int *>(wout + (size_t)epb * qpb * 6);
	int *nconv = reinterpret_cast<int *>(masks + (size_t)qpb * 2 * nwords);

	// ---- once per block: masks, reference points, ncon
	for (int k = t; k < nq * 2 * nwords; k += NT) masks[k] = gmask[k];
	for (int le = t; le < epb; le += NT) {
		const int env = env0 + le;
		int n = 0;
		if (env < nenv) n = reinterpret_cast<const int *>(s.frame_ws + (size_t)env * s.frame_stride + L.ndouble)[L.ncon];
		nconv[le] = n < 0 ? 0 : (n > nconmax ? nconmax : n);
	}
	for (int idx = t; idx < epb * nq * 3; idx += NT) {
		const int le = idx / (nq * 3), rem = idx - le * nq * 3, ql = rem / 3, k = rem - ql * 3, env = env0 + le;
		const int rb = refbody[ql];
		rq[(le * qpb + ql) * 3 + k] = (env < nenv && rb >= 0 && rb < m.nbody) ? s.frame_ws[(size_t)env * s.frame_stride + L.xpos + 3 * rb + k] : 0.0;
	}
	__syncthreads();
	int maxn = 0;
	for (int le = 0; le < epb; le++) maxn = max(maxn, nconv[le]);

	// this lane's (env, query) of the sum phase
	const int le_s = t / qpb, ql_s = t - le_s * qpb;
	const bool live = le_s < epb && ql_s < nq && env0 + le_s < nenv;
	const unsigned int *mA = masks + (size_t)(live ? ql_s : 0) * 2 * nwords, *mB = mA + nwords;
	double rqs[3] = { 0, 0, 0 };
	if (live) ld3(rqs, rq + (le_s * qpb + ql_s) * 3);
	double acc[6] = { 0, 0, 0, 0, 0, 0 }, normal = 0, dmin = __builtin_inf();
	int count = 0;

	for (int c0 = 0; c0 < maxn; c0 += ct) {
		// ---- 1: stage the tile's records, element by element.  field(base offset in the frame, width, offset in the slot)
		auto stage = [&](int off, int width, int so) {
			for (int idx = t; idx < epb * ct * width; idx += NT) {
				const int le = idx / (ct * width), k = idx - le * ct * width, cl = k / width, j = k - cl * width;
				if (c0 + cl < nconv[le]) slots[(size_t)(le * ct + cl) * MJB_CON_SLOT + so + j] = s.frame_ws[(size_t)(env0 + le) * s.frame_stride + off + width * c0 + k];
			}
		};
		auto stage_int = [&](int off, int width, int so) {
			for (int idx = t; idx < epb * ct * width; idx += NT) {
				const int le = idx / (ct * width), k = idx - le * ct * width, cl = k / width, j = k - cl * width;
				if (c0 + cl < nconv[le])
					reinterpret_cast<int *>(slots + (size_t)(le * ct + cl) * MJB_CON_SLOT + MJB_CON_S_INTS)[so + j] =
						reinterpret_cast<const int *>(s.frame_ws + (size_t)(env0 + le) * s.frame_stride + L.ndouble)[off + width * c0 + k];
			}
		};
		stage_int(L.contact_geom, 2, 0);
		stage_int(L.contact_dim, 1, 2);
		stage_int(L.contact_efc_address, 1, 3);
		stage(L.contact_frame, 9, MJB_CON_S_FRAME);
		stage(L.contact_pos, 3, MJB_CON_S_POS);
		stage(L.contact_dist, 1, MJB_CON_S_DIST);
		stage(L.contact_friction, 5, MJB_CON_S_FRICTION);
		__syncthreads();
		// ... and the rows of efc_force they address (a contact whose rows do not lie inside the frame's row arrays counts as one without rows)
		for (int idx = t; idx < epb * ct * MJB_CON_ROWS; idx += NT) {
			const int le = idx / (ct * MJB_CON_ROWS), k = idx - le * ct * MJB_CON_ROWS, cl = k / MJB_CON_ROWS, j = k - cl * MJB_CON_ROWS;
			if (c0 + cl >= nconv[le]) continue;
			double *sl = slots + (size_t)(le * ct + cl) * MJB_CON_SLOT;
			const int *si = reinterpret_cast<const int *>(sl + MJB_CON_S_INTS);
			const int dim = si[2], adr = si[3];
			if (adr < 0 || dim < 1 || dim > 6) continue;
			const int rows = contact_rows(dim, elliptic);
			if (adr + rows <= nefcmax && j < rows) sl[MJB_CON_S_FORCE + j] = s.frame_ws[(size_t)(env0 + le) * s.frame_stride + L.efc_force + adr + j];
		}
		__syncthreads();

		// ---- 2: decode, in place
		for (int idx = t; idx < epb * ct; idx += NT) {
			const int le = idx / ct, cl = idx - le * ct;
			if (c0 + cl >= nconv[le]) continue;
			double *sl = slots + (size_t)idx * MJB_CON_SLOT;
			int *si = reinterpret_cast<int *>(sl + MJB_CON_S_INTS);
			const int dim = si[2], adr = si[3];
			const bool rows_ok = adr >= 0 && dim >= 1 && dim <= 6 && adr + contact_rows(dim, elliptic) <= nefcmax;
			double lf[6] = { 0, 0, 0, 0, 0, 0 }, F[3] = { 0, 0, 0 }, T[3] = { 0, 0, 0 };
			if (rows_ok) {
				double fr[MJB_CON_ROWS], mu[5], R[9];
				for (int k = 0; k < MJB_CON_ROWS; k++) fr[k] = k < contact_rows(dim, elliptic) ? sl[MJB_CON_S_FORCE + k] : 0.0;
				for (int k = 0; k < 5; k++) mu[k] = sl[MJB_CON_S_FRICTION + k];
				ld9(R, sl + MJB_CON_S_FRAME);
				contact_lf(dim, elliptic, fr, mu, lf);
				matTvec3(F, R, lf);
				matTvec3(T, R, lf + 3);
			} else {
				si[3] = -1;  // (the sum phase skips it)
			}
			st6(sl + MJB_CON_S_LF, lf);
			st3(sl + MJB_CON_S_F, F);
			st3(sl + MJB_CON_S_T, T);
		}
		__syncthreads();
		if (out_contacts && qblock == 0) {
			for (int idx = t; idx < epb * ct * 6; idx += NT) {
				const int le = idx / (ct * 6), k = idx - le * ct * 6, cl = k / 6, j = k - cl * 6;
				if (c0 + cl < nconv[le]) out_contacts[((size_t)(env0 + le) * nconmax + c0) * 6 + k] = slots[(size_t)(le * ct + cl) * MJB_CON_SLOT + MJB_CON_S_LF + j];
			}
		}

		// ---- 3: sum, ascending c
		if (live) {
			const int n_here = min(ct, nconv[le_s] - c0);
			for (int cl = 0; cl < n_here; cl++) {
				const double *sl = slots + (size_t)(le_s * ct + cl) * MJB_CON_SLOT;
				const int *si = reinterpret_cast<const int *>(sl + MJB_CON_S_INTS);
				const int g1 = si[0], g2 = si[1];
				if (si[3] < 0 || g1 < 0 || g2 < 0 || g1 >= ngeom || g2 >= ngeom) continue;
				const bool plus = mask_bit(mA, g2) && mask_bit(mB, g1), minus = mask_bit(mA, g1) && mask_bit(mB, g2);
				if (!plus && !minus) continue;  // (A and B are disjoint: never both)
				const double d[3] = { sl[MJB_CON_S_POS] - rqs[0], sl[MJB_CON_S_POS + 1] - rqs[1], sl[MJB_CON_S_POS + 2] - rqs[2] };
				double term[6], cr[3];
				ld3(term, sl + MJB_CON_S_F);
				cross3(cr, d, term);
				for (int k = 0; k < 3; k++) term[3 + k] = sl[MJB_CON_S_T + k] + cr[k];
				for (int k = 0; k < 6; k++) acc[k] = plus ? acc[k] + term[k] : acc[k] - term[k];
				normal += sl[MJB_CON_S_LF];
				count++;
				dmin = fmin(dmin, sl[MJB_CON_S_DIST]);
			}
		}
		__syncthreads();  // (the next tile's staging rewrites the slots)
	}

	// ---- the outputs, one element per lane
	if (out_contacts && qblock == 0) {
		for (int idx = t; idx < epb * nconmax * 6; idx += NT) {
			const int le = idx / (nconmax * 6), k = idx - le * nconmax * 6;
			if (env0 + le < nenv && k / 6 >= nconv[le]) out_contacts[(size_t)(env0 + le) * nconmax * 6 + k] = 0.0;
		}
	}
	if (live) {
		const size_t o = (size_t)(env0 + le_s) * nquery + q0 + ql_s;
		if (out_normal) out_normal[o] = normal;
		if (out_count) out_count[o] = count;
		if (out_dist) out_dist[o] = dmin;
		st6(wout + (le_s * qpb + ql_s) * 6, acc);
	}
	if (!out_wrench) return;  // (the same for every lane of the block)
	__syncthreads();
	for (int idx = t; idx < epb * nq * 6; idx += NT) {
		const int le = idx / (nq * 6), k = idx - le * nq * 6, ql = k / 6, j = k - ql * 6;
		if (env0 + le < nenv) out_wrench[((size_t)(env0 + le) * nquery + q0) * 6 + k] = wout[(le * qpb + ql) * 6 + j];
	}
}

}  // namespace

int mjb_launch_contact(const KernelParams *Pdev, const unsigned int *tab, int nenv, int nquery, int ngeom, int nconmax, double *out_wrench, double *out_normal, int *out_count,
                       double *out_dist, double *out_contacts, void *stream)
{
	const ConShape sh = mjb_contact_shape(ngeom, nconmax, nquery);
	const long long query_blocks = (nquery + sh.qpb - 1) / sh.qpb, env_blocks = (nenv + sh.epb - 1) / sh.epb;
	if (query_blocks * env_blocks > 0x7fffffffLL || sh.epb * sh.qpb > MJB_CON_BLOCK || sh.epb * sh.ct > MJB_CON_BLOCK || sh.lds_bytes > MJB_CON_LDS_LIMIT)
		return (int)hipErrorInvalidConfiguration;
	hipLaunchKernelGGL(mjb_contact_kernel, dim3((unsigned int)(query_blocks * env_blocks)), dim3(MJB_CON_BLOCK), (size_t)sh.lds_bytes, (hipStream_t)stream,
	                   (const KernelParams MJB_AS4 *)Pdev, tab, nquery, sh.epb, sh.qpb, sh.ct, sh.nwords, (int)query_blocks, out_wrench, out_normal, out_count, out_dist, out_contacts);
	return (int)hipGetLastError();
}
