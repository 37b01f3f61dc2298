// mjb_jac.hip -- batched Jacobians (mjb_jac_*): mj_jacSite / mj_jacBody / mj_jacBodyCom / mj_jacGeom, mj_solveM on their rows and J M^-1 J' for the
// configured points of every env in one launch, fp64.
//
// A block of 256 lanes takes `epb` whole envs with all their points, or -- a point set too long for the block's 40 KiB of LDS -- a tile of one env's
// points (mjb_jac_shape).  Per env it stages cdof, qvel, the points' world positions with the subtree_com of their trees' roots and, for a solve, qLD and
// qLDiagInv through LDS once, next to the dof tree (M_coldof, dof_Madr, dof_depth) as ints; after that no lane loads from global memory.  The phases, a
// barrier between any two:
//   1  J.  One lane per (env, point, dof) computes the column (jac_column, the arithmetic of the step kernel's point_jac) and writes its six entries
//      into the block's rows, which live in LDS dof-major across the rows ([nv][rows]): lane s = ((env, point), row) owns column s of that array.
//   2  J goes out with one element per lane, consecutive lanes to consecutive addresses -- a lane reads other lanes' columns here, as in the MINVJT
//      output of phase 4 --; VEL is row . qvel, one row per lane, ascending dofs.
//   3  y = L^-T J[r]', the first half of mj_solveM, in place: one lane per row.  The loops over the dofs and over a dof's ancestors are the same for
//      every lane (the tree is the model's); a lane takes part in pivot i when dof i moves its point's body.  The support of a row is that set of
//      ancestor dofs and this half never leaves it, so a wavefront skips the pivots none of its bodies has.
//      AINV[r][c] = sum_d (y_r[d] y_c[d]) / D[d] in ascending d: the same sequence of roundings for (r, c) and (c, r), symmetric to the bit.
//   4  MINVJT = L^-1 D^-1 y, the second half: it fills in every dof of the tree (M^-1 J' is dense there), so it runs over all dofs, for every lane
//      alike.  The rows go out as J did.
// Every value is computed by one lane from operands that do not depend on the block's shape: no result depends on the launch.
#include <hip/hip_runtime.h>

#include "mjb_dev.h"
#include "mjb_jac.h"
#include "mjb_math.h"

namespace {

__global__ void __launch_bounds__(MJB_JAC_BLOCK) mjb_jac_kernel(const KernelParams MJB_AS4 *__restrict__ P, const double *__restrict__ tab, int npoint, int epb, int ppb, int env_doubles,
                                                                int rows_pad, int point_blocks, double *__restrict__ out_J, double *__restrict__ out_MinvJT,
                                                                double *__restrict__ out_Ainv, double *__restrict__ out_vel)
{
	extern __shared__ double lds[];
	const DevModel MJB_AS4 &m = P->m;
	const DevState MJB_AS4 &s = P->s;
	const FrameLayout MJB_AS4 &L = P->L;
	const int nenv = s.nenv, nv = m.nv, nM = m.nM;
	const bool solve = out_MinvJT != nullptr || out_Ainv != nullptr;
	const JacPoint *__restrict__ rec = reinterpret_cast<const JacPoint *>(tab + (size_t)3 * npoint);
	const int env_block = (int)(blockIdx.x / (unsigned int)point_blocks), pblock = (int)(blockIdx.x % (unsigned int)point_blocks);
	const int env0 = env_block * epb, p0 = pblock * ppb;
	const int np = min(ppb, npoint - p0);  // points of this block
	const int t = (int)threadIdx.x, NT = (int)blockDim.x;
	// the LDS plan (mjb_jac.h): per env cdof[6 nv] | qvel[nv] | p[3 ppb] | rc[3 ppb] | qLD[nM] | qLDiagInv[nv], the rows, the dof tree
	const int o_qvel = 6 * nv, o_p = 7 * nv, o_rc = 7 * nv + 3 * ppb, o_LD = 7 * nv + 6 * ppb, o_di = o_LD + nM;
	double *rows = lds + (size_t)epb * env_doubles;
	int *coldof = reinterpret_cast<int *>(rows + (size_t)nv * rows_pad), *madr = coldof + nM, *depth = madr + nv;

	// ---- staging
	for (int idx = t; idx < epb * 7 * nv; idx += NT) {
		const int le = idx / (7 * nv), k = idx - le * 7 * nv, env = env0 + le;
		double v = 0;
		if (env < nenv) v = k < 6 * nv ? s.frame_ws[(size_t)env * s.frame_stride + L.cdof + k] : s.qvel[(size_t)env * nv + (k - 6 * nv)];
		lds[le * env_doubles + k] = v;
	}
	for (int idx = t; idx < epb * np; idx += NT) {
		const int le = idx / np, pl = idx - le * np, env = env0 + le;
		double p[3] = { 0, 0, 0 }, rc[3] = { 0, 0, 0 };
		if (env < nenv) {
			const JacPoint r = rec[p0 + pl];
			const double *f = s.frame_ws + (size_t)env * s.frame_stride;
			const int opos = r.type == MJB_JAC_SITE ? L.site_xpos : (r.type == MJB_JAC_BODY ? L.xpos : (r.type == MJB_JAC_BODYCOM ? L.xipos : L.geom_xpos));
			const int omat = r.type == MJB_JAC_SITE ? L.site_xmat : (r.type == MJB_JAC_BODY ? L.xmat : (r.type == MJB_JAC_BODYCOM ? L.ximat : L.geom_xmat));
			double R[9], o[3], rp[3];
			const double pnt[3] = { tab[3 * (p0 + pl)], tab[3 * (p0 + pl) + 1], tab[3 * (p0 + pl) + 2] };
			ld9(R, f + omat + 9 * r.id);
			ld3(o, f + opos + 3 * r.id);
			matvec3(rp, R, pnt);
			for (int k = 0; k < 3; k++) p[k] = o[k] + rp[k];
			ld3(rc, f + L.subtree_com + 3 * r.root);
		}
		st3(lds + le * env_doubles + o_p + 3 * pl, p);
		st3(lds + le * env_doubles + o_rc + 3 * pl, rc);
	}
	if (solve) {
		for (int idx = t; idx < epb * (nM + nv); idx += NT) {
			const int le = idx / (nM + nv), k = idx - le * (nM + nv), env = env0 + le;
			double v = 0;
			if (env < nenv) {
				const double *f = s.frame_ws + (size_t)env * s.frame_stride;
				v = k < nM ? f[L.qLD + k] : f[L.qLDiagInv + (k - nM)];
			}
			lds[le * env_doubles + o_LD + k] = v;
		}
		for (int k = t; k < nM; k += NT) coldof[k] = m.M_coldof[k];
		for (int k = t; k < nv; k += NT) {
			madr[k] = m.dof_Madr[k];
			depth[k] = m.dof_depth[k];
		}
	}
	__syncthreads();

	// ---- 1: the columns, into the rows
	for (int idx = t; idx < epb * np * nv; idx += NT) {
		const int q = idx / nv, d = idx - q * nv, le = q / np, pl = q - le * np;
		const JacPoint r = rec[p0 + pl];
		const double *eb = lds + le * env_doubles;
		double cd[6], jp[3], jr[3];
		ld6(cd, eb + 6 * d);
		jac_column(env0 + le < nenv && (((d < 32 ? r.mask[0] : r.mask[1]) >> (d & 31)) & 1u), cd, eb + o_rc + 3 * pl, eb + o_p + 3 * pl, jp, jr);
		double *col = rows + (size_t)d * rows_pad + (le * ppb + pl) * 6;
		for (int k = 0; k < 3; k++) {
			col[k] = jp[k];
			col[3 + k] = jr[k];
		}
	}
	__syncthreads();

	// ---- 2: J and VEL
	if (out_J) {
		const int per_env = np * 6 * nv;
		for (int idx = t; idx < epb * per_env; idx += NT) {
			const int le = idx / per_env, rem = idx - le * per_env, q = rem / nv, d = rem - q * nv, env = env0 + le;
			if (env < nenv) out_J[(((size_t)env * npoint + p0) * 6 + q) * nv + d] = rows[(size_t)d * rows_pad + le * ppb * 6 + q];
		}
	}
	// this lane's row: s_row = ((le, pl), r), column s_row of the rows
	const int le = t / (ppb * 6), q = t - le * ppb * 6, pl = q / 6, r = q - pl * 6, env = env0 + le;
	const bool live = le < epb && env < nenv && pl < np;
	const int s_row = t;  // (= (le * ppb + pl) * 6 + r; below rows_pad for a live lane)
	const double *eb = lds + (live ? le : 0) * env_doubles;
	unsigned int mask0 = 0, mask1 = 0;
	if (live) {
		mask0 = rec[p0 + pl].mask[0];
		mask1 = rec[p0 + pl].mask[1];
	}
	const size_t orow = live ? ((size_t)env * npoint + p0 + pl) * 6 + r : 0;
	if (out_vel && live) {
		double acc = 0;
		for (int d = 0; d < nv; d++) acc = fma(rows[(size_t)d * rows_pad + s_row], eb[o_qvel + d], acc);
		out_vel[orow] = acc;
	}
	if (!solve) return;  // (the same for every lane of the block)
	__syncthreads();     // (the J output has read every column, VEL its own: phase 3 rewrites them in place)

	// ---- 3: y = L^-T J[r]' in place, then AINV
	for (int i = nv - 1; i > 0; i--) {
		const int dep = depth[i];
		if (dep < 2) continue;
		if (live && (((i < 32 ? mask0 : mask1) >> (i & 31)) & 1u)) {
			const int adr = madr[i];
			const double xi = rows[(size_t)i * rows_pad + s_row];
			for (int k = 1; k < dep; k++) {
				double *x = rows + (size_t)coldof[adr + k] * rows_pad + s_row;
				*x = fma(-eb[o_LD + adr + k], xi, *x);
			}
		}
	}
	__syncthreads();
	if (out_Ainv && live) {
		double acc[6] = { 0, 0, 0, 0, 0, 0 };
		const int s_pt = s_row - r;  // row 0 of this lane's point
		for (int d = 0; d < nv; d++) {
			if (!(((d < 32 ? mask0 : mask1) >> (d & 31)) & 1u)) continue;  // (the rows of one point share the mask: both orders skip the same terms)
			const double di = eb[o_di + d], yr = rows[(size_t)d * rows_pad + s_row];
			for (int c = 0; c < 6; c++) acc[c] = __fma_rn(__dmul_rn(yr, rows[(size_t)d * rows_pad + s_pt + c]), di, acc[c]);
		}
		for (int c = 0; c < 6; c++) out_Ainv[orow * 6 + c] = acc[c];
	}
	if (!out_MinvJT) return;
	__syncthreads();  // (AINV has read the other rows of the point)

	// ---- 4: MINVJT = L^-1 D^-1 y
	if (live) {
		for (int d = 0; d < nv; d++) rows[(size_t)d * rows_pad + s_row] *= eb[o_di + d];
		for (int i = 1; i < nv; i++) {
			const int dep = depth[i];
			if (dep < 2) continue;
			const int adr = madr[i];
			double acc = rows[(size_t)i * rows_pad + s_row];
			for (int k = 1; k < dep; k++) acc = fma(-eb[o_LD + adr + k], rows[(size_t)coldof[adr + k] * rows_pad + s_row], acc);
			rows[(size_t)i * rows_pad + s_row] = acc;
		}
	}
	__syncthreads();
	const int per_env = np * 6 * nv;
	for (int idx = t; idx < epb * per_env; idx += NT) {
		const int le2 = idx / per_env, rem = idx - le2 * per_env, q2 = rem / nv, d = rem - q2 * nv, env2 = env0 + le2;
		if (env2 < nenv) out_MinvJT[(((size_t)env2 * npoint + p0) * 6 + q2) * nv + d] = rows[(size_t)d * rows_pad + le2 * ppb * 6 + q2];
	}
}

}  // namespace

int mjb_launch_jac(const KernelParams *Pdev, const double *tab, int nenv, int npoint, int nv, int nM, double *out_J, double *out_MinvJT, double *out_Ainv, double *out_vel, void *stream)
{
	const JacShape sh = mjb_jac_shape(nv, nM, npoint, out_MinvJT != nullptr || out_Ainv != nullptr);
	const long long point_blocks = (npoint + sh.ppb - 1) / sh.ppb, env_blocks = (nenv + sh.epb - 1) / sh.epb;
	if (point_blocks * env_blocks > 0x7fffffffLL || sh.epb * sh.ppb * 6 > MJB_JAC_BLOCK || sh.lds_bytes > MJB_JAC_LDS_BYTES) return (int)hipErrorInvalidConfiguration;
	hipLaunchKernelGGL(mjb_jac_kernel, dim3((unsigned int)(point_blocks * env_blocks)), dim3(MJB_JAC_BLOCK), (size_t)sh.lds_bytes, (hipStream_t)stream, (const KernelParams MJB_AS4 *)Pdev, tab,
	                   npoint, sh.epb, sh.ppb, sh.env_doubles, sh.rows_pad, (int)point_blocks, out_J, out_MinvJT, out_Ainv, out_vel);
	return (int)hipGetLastError();
}
