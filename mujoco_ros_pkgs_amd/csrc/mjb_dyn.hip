// mjb_dyn.hip -- batched joint-space dynamics (mjb_dyn_*): mj_fullM, mj_mulM, mj_solveM and the inverse dynamics on a block of vectors V the caller owns, and
// the bias acceleration Jdot qvel of configured points, for every env in one launch, fp64.
//
// A block of 256 lanes takes `epb` whole envs with all their vectors and points, or -- a set too long for the block's 40 KiB of LDS -- one env with a tile
// of its vectors and points (mjb_dyn_shape).  Everything is read from the frame workspace a forward pass left behind.  Per env the block has ONE LDS region
// that the phases fill one after the other, and the block's vectors as columns, dof-major across them ([nv][columns]).  The phases, a barrier between any two:
//   A  qM into the region, V into the columns.  M: one lane per element, a gather through full_adr (a structural zero is a literal +0.0).  MV / ID: one lane
//      per (env, vector, row), the row's entries in ascending j with __fma_rn, structural zeros skipped; ID = (MV + qfrc_bias) - qfrc_passive, rounded in
//      that order.  Both leave one element per lane at consecutive addresses.
//   B  qLD | qLDiagInv into the region, the dof tree (M_coldof, dof_Madr, dof_depth) beside it as ints.  MINVV: one lane per column, in place: L^-T, D^-1,
//      L^-1 -- the walk of mjb_jac.hip's phases 3 and 4 on a dense right-hand side, restated here --, then the columns go out one element per lane.
//   C  cdof_dot | qvel into the region.  JDOTV: one lane per (env, point, row); the six lanes of a point repeat the same arithmetic and each stores its row.
// Every value is computed by one lane from operands that do not depend on the block's shape: no result depends on the launch.
#include <hip/hip_runtime.h>

#include "mjb_dev.h"
#include "mjb_dyn.h"
#include "mjb_math.h"

namespace {

__global__ void __launch_bounds__(MJB_DYN_BLOCK) mjb_dyn_kernel(const KernelParams MJB_AS4 *__restrict__ P, const int *__restrict__ full_adr, const double *__restrict__ tab,
                                                                const double *__restrict__ V, int nvec, int npoint, int epb, int vpb, int ppb, int tiles, int env_doubles, int cols_pad,
                                                                int unintegrate, double *__restrict__ out_M, double *__restrict__ out_MV, double *__restrict__ out_MinvV,
                                                                double *__restrict__ out_ID, double *__restrict__ out_Jdotv)
{
	extern __shared__ double lds[];
	const DevModel MJB_AS4 &m = P->m;
	const DevState MJB_AS4 &s = P->s;
	const FrameLayout MJB_AS4 &L = P->L;
	const int nenv = s.nenv, nv = m.nv, nM = m.nM;
	const int env_block = (int)(blockIdx.x / (unsigned int)tiles), tile = (int)(blockIdx.x % (unsigned int)tiles);
	const int env0 = env_block * epb, k0 = tile * vpb, p0 = tile * ppb;
	const int t = (int)threadIdx.x, NT = (int)blockDim.x;
	// what this block has to do (the same for every lane of it)
	const bool vecs = out_MV != nullptr || out_MinvV != nullptr || out_ID != nullptr;
	const int nvk = vecs ? max(0, min(vpb, nvec - k0)) : 0;           // vectors of this block
	const int np = out_Jdotv ? max(0, min(ppb, npoint - p0)) : 0;     // points of this block
	const bool do_M = out_M != nullptr && tile == 0, do_MV = (out_MV != nullptr || out_ID != nullptr) && nvk > 0, do_solve = out_MinvV != nullptr && nvk > 0;
	double *cols = lds + (size_t)epb * env_doubles;
	int *coldof = reinterpret_cast<int *>(cols + (size_t)nv * cols_pad), *madr = coldof + nM, *depth = madr + nv;

	// ---- A: qM and the vectors
	if (do_M || do_MV) {
		for (int idx = t; idx < epb * nM; idx += NT) {
			const int le = idx / nM, k = idx - le * nM, env = env0 + le;
			lds[le * env_doubles + k] = env < nenv ? s.frame_ws[(size_t)env * s.frame_stride + L.qM + k] : 0.0;
		}
	}
	for (int idx = t; idx < epb * nvk * nv; idx += NT) {
		const int le = idx / (nvk * nv), rem = idx - le * nvk * nv, k = rem / nv, j = rem - k * nv, env = env0 + le;
		cols[(size_t)j * cols_pad + le * vpb + k] = env < nenv ? V[((size_t)env * nvec + k0 + k) * nv + j] : 0.0;
	}
	__syncthreads();
	if (do_M) {
		for (int idx = t; idx < epb * nv * nv; idx += NT) {
			const int le = idx / (nv * nv), ij = idx - le * nv * nv, env = env0 + le;
			if (env >= nenv) continue;
			const int adr = full_adr[ij];
			out_M[(size_t)env * nv * nv + ij] = adr >= 0 ? lds[le * env_doubles + adr] : 0.0;
		}
	}
	if (do_MV) {
		for (int idx = t; idx < epb * nvk * nv; idx += NT) {
			const int le = idx / (nvk * nv), rem = idx - le * nvk * nv, k = rem / nv, i = rem - k * nv, env = env0 + le;
			if (env >= nenv) continue;
			const double *qM = lds + le * env_doubles, *col = cols + le * vpb + k;
			double acc = 0;
			for (int j = 0; j < nv; j++) {
				const int adr = full_adr[j * nv + i];  // (= full_adr[i * nv + j]: consecutive lanes read consecutive words)
				if (adr >= 0) acc = __fma_rn(qM[adr], col[(size_t)j * cols_pad], acc);
			}
			const size_t o = ((size_t)env * nvec + k0 + k) * nv + i;
			if (out_MV) out_MV[o] = acc;
			if (out_ID) {
				const double *f = s.frame_ws + (size_t)env * s.frame_stride;
				out_ID[o] = __dsub_rn(__dadd_rn(acc, f[L.qfrc_bias + i]), f[L.qfrc_passive + i]);
			}
		}
	}

	// ---- B: M^-1 V on the frame's factor
	if (do_solve) {
		__syncthreads();  // (the products have read qM: the region is rewritten)
		for (int idx = t; idx < epb * (nM + nv); idx += NT) {
			const int le = idx / (nM + nv), k = idx - le * (nM + nv), env = env0 + le;
			double v = 0;
			if (env < nenv) {
				const double *f = s.frame_ws + (size_t)env * s.frame_stride;
				v = k < nM ? f[L.qLD + k] : f[L.qLDiagInv + (k - nM)];
			}
			lds[le * env_doubles + k] = v;
		}
		for (int k = t; k < nM; k += NT) coldof[k] = m.M_coldof[k];
		for (int k = t; k < nv; k += NT) {
			madr[k] = m.dof_Madr[k];
			depth[k] = m.dof_depth[k];
		}
		__syncthreads();
		// this lane's column: c = (le, k)
		const int le = t / vpb, k = t - le * vpb;
		if (le < epb && k < nvk && env0 + le < nenv) {
			const double *LD = lds + le * env_doubles, *di = LD + nM;
			double *x = cols + t;  // (t = le * vpb + k, below cols_pad)
			for (int i = nv - 1; i > 0; i--) {  // y = L^-T v
				const int dep = depth[i];
				if (dep < 2) continue;
				const int adr = madr[i];
				const double xi = x[(size_t)i * cols_pad];
				for (int a = 1; a < dep; a++) {
					double *xa = x + (size_t)coldof[adr + a] * cols_pad;
					*xa = fma(-LD[adr + a], xi, *xa);
				}
			}
			for (int d = 0; d < nv; d++) x[(size_t)d * cols_pad] *= di[d];  // D^-1
			for (int i = 1; i < nv; i++) {  // L^-1
				const int dep = depth[i];
				if (dep < 2) continue;
				const int adr = madr[i];
				double acc = x[(size_t)i * cols_pad];
				for (int a = 1; a < dep; a++) acc = fma(-LD[adr + a], x[(size_t)coldof[adr + a] * cols_pad], acc);
				x[(size_t)i * cols_pad] = acc;
			}
		}
		__syncthreads();
		for (int idx = t; idx < epb * nvk * nv; idx += NT) {
			const int le2 = idx / (nvk * nv), rem = idx - le2 * nvk * nv, k2 = rem / nv, i = rem - k2 * nv, env = env0 + le2;
			if (env < nenv) out_MinvV[((size_t)env * nvec + k0 + k2) * nv + i] = cols[(size_t)i * cols_pad + le2 * vpb + k2];
		}
	}

	// ---- C: Jdot qvel of the points
	if (np > 0) {
		const JacPoint *__restrict__ rec = reinterpret_cast<const JacPoint *>(tab + (size_t)3 * npoint);
		const double h = m.timestep[0];
		__syncthreads();  // (the region is rewritten)
		for (int idx = t; idx < epb * 7 * nv; idx += NT) {
			const int le = idx / (7 * nv), k = idx - le * 7 * nv, env = env0 + le;
			double v = 0;
			if (env < nenv) {
				const double *f = s.frame_ws + (size_t)env * s.frame_stride;
				if (k < 6 * nv) v = f[L.cdof_dot + k];
				else {
					// the velocities the frame's cvel and cdof_dot belong to: qvel, or -- behind a step's second half -- qvel before its update
					// qvel += timestep * eulerx (mjb_step.hip, euler)
					v = s.qvel[(size_t)env * nv + (k - 6 * nv)];
					if (unintegrate) v = __fma_rn(-h, f[L.eulerx + (k - 6 * nv)], v);
				}
			}
			lds[le * env_doubles + k] = v;
		}
		__syncthreads();
		for (int idx = t; idx < epb * np * 6; idx += NT) {
			const int le = idx / (np * 6), rem = idx - le * np * 6, pl = rem / 6, r = rem - pl * 6, env = env0 + le;
			if (env >= nenv) continue;
			const JacPoint pt = rec[p0 + pl];
			double lin[3] = { 0, 0, 0 }, ang[3] = { 0, 0, 0 };
			if (pt.body > 0) {
				const double *f = s.frame_ws + (size_t)env * s.frame_stride, *eb = lds + le * env_doubles;
				const int opos = pt.type == MJB_JAC_SITE ? L.site_xpos : (pt.type == MJB_JAC_BODY ? L.xpos : (pt.type == MJB_JAC_BODYCOM ? L.xipos : L.geom_xpos));
				const int omat = pt.type == MJB_JAC_SITE ? L.site_xmat : (pt.type == MJB_JAC_BODY ? L.xmat : (pt.type == MJB_JAC_BODYCOM ? L.ximat : L.geom_xmat));
				double R[9], o[3], rp[3], rc[3], cv[6];
				const double pnt[3] = { tab[3 * (p0 + pl)], tab[3 * (p0 + pl) + 1], tab[3 * (p0 + pl) + 2] };
				ld9(R, f + omat + 9 * pt.id);
				ld3(o, f + opos + 3 * pt.id);
				matvec3(rp, R, pnt);
				ld3(rc, f + L.subtree_com + 3 * pt.root);
				ld6(cv, f + L.cvel + 6 * pt.body);
				// A = sum of cdof_dot[d] qvel[d] over the dofs that move the body, ascending
				double A[6] = { 0, 0, 0, 0, 0, 0 };
				for (int d = 0; d < nv; d++) {
					if (!(((d < 32 ? pt.mask[0] : pt.mask[1]) >> (d & 31)) & 1u)) continue;
					const double qv = eb[6 * nv + d];
					for (int c = 0; c < 6; c++) A[c] = __fma_rn(eb[6 * d + c], qv, A[c]);
				}
				// r = p - subtree_com[root]; v_p = v + w x r; linear = A_lin + A_ang x r + w x v_p, angular = A_ang
				double off[3], wr[3], vp[3], ar[3], wv[3];
				for (int c = 0; c < 3; c++) off[c] = (o[c] + rp[c]) - rc[c];
				cross3(wr, cv, off);
				for (int c = 0; c < 3; c++) vp[c] = cv[3 + c] + wr[c];
				cross3(ar, A, off);
				cross3(wv, cv, vp);
				for (int c = 0; c < 3; c++) {
					lin[c] = (A[3 + c] + ar[c]) + wv[c];
					ang[c] = A[c];
				}
			}
			out_Jdotv[((size_t)env * npoint + p0 + pl) * 6 + r] = r == 0 ? lin[0] : (r == 1 ? lin[1] : (r == 2 ? lin[2] : (r == 3 ? ang[0] : (r == 4 ? ang[1] : ang[2]))));
		}
	}
}

}  // namespace

int mjb_launch_dyn(const KernelParams *Pdev, const int *full_adr, const double *tab, const double *V, int nenv, int nvec, int npoint, int nv, int nM, int unintegrate, double *out_M,
                   double *out_MV, double *out_MinvV, double *out_ID, double *out_Jdotv, void *stream)
{
	const int outputs = (out_M ? MJB_DYN_OUT_M : 0) | (out_MV ? MJB_DYN_OUT_MV : 0) | (out_MinvV ? MJB_DYN_OUT_MINVV : 0) | (out_ID ? MJB_DYN_OUT_ID : 0) | (out_Jdotv ? MJB_DYN_OUT_JDOTV : 0);
	const bool vecs = (outputs & (MJB_DYN_OUT_MV | MJB_DYN_OUT_MINVV | MJB_DYN_OUT_ID)) != 0;
	if (outputs == 0 || nenv < 1 || nv < 1 || !full_adr || (vecs && (nvec < 1 || !V)) || (out_Jdotv && (npoint < 1 || !tab))) return (int)hipErrorInvalidValue;
	const DynShape sh = mjb_dyn_shape(nv, nM, nvec, npoint, outputs);
	const long long blocks = (long long)((nenv + sh.epb - 1) / sh.epb) * sh.tiles;
	if (blocks > 0x7fffffffLL || sh.epb * sh.vpb > MJB_DYN_BLOCK || sh.epb * sh.ppb * 6 > MJB_DYN_BLOCK || sh.lds_bytes > MJB_DYN_LDS_BYTES || (vecs && sh.vpb < 1) || (out_Jdotv && sh.ppb < 1))
		return (int)hipErrorInvalidConfiguration;
	hipLaunchKernelGGL(mjb_dyn_kernel, dim3((unsigned int)blocks), dim3(MJB_DYN_BLOCK), (size_t)sh.lds_bytes, (hipStream_t)stream, (const KernelParams MJB_AS4 *)Pdev, full_adr, tab, V, nvec,
	                   npoint, sh.epb, sh.vpb, sh.ppb, sh.tiles, sh.env_doubles, sh.cols_pad, unintegrate, out_M, out_MV, out_MinvV, out_ID, out_Jdotv);
	return (int)hipGetLastError();
}
