// mjb_dyn.h — what the batched joint-space dynamics kernel (mjb_dyn.hip) shares with the batch side of the C-ABI (mjb_api.hip, mjb_dyn_*): the dense
// index table of qM and the shape of a launch.  The points of the JDOTV output use the Jacobian kernel's table (mjb_jac.h: pnt[npoint][3], then one
// JacPoint per point).
#pragma once

#include "../../include/mjb.h"
#include "mjb_dev.h"
#include "mjb_jac.h"

// full_adr[nv][nv], a model constant built once by mjb_dyn_configure: the index into qM of entry (i, j) when one dof is the other's ancestor-or-self
// along dof_parentid, -1 otherwise.  Symmetric.  qM stores row i as its diagonal, then the ancestors walking up, from dof_Madr[i] (M_coldof's order).
inline void mjb_dyn_full_adr(int nv, const int *dof_Madr, const int *dof_parentid, int *full_adr)
{
	for (int k = 0; k < nv * nv; k++) full_adr[k] = -1;
	for (int i = 0; i < nv; i++) {
		int adr = dof_Madr[i];
		for (int j = i; j >= 0; j = dof_parentid[j], adr++) full_adr[i * nv + j] = full_adr[j * nv + i] = adr;
	}
}

// The shape of a launch: a block of MJB_DYN_BLOCK lanes takes `epb` whole envs with all their vectors and points, or -- a set too long for that -- one
// env with a tile of `vpb` of its vectors and `ppb` of its points (tile t: vectors [t vpb, ..) and points [t ppb, ..); tile 0 also writes M).
// LDS, in doubles: per env ONE region the phases use one after the other -- qM[nM] (M, MV, ID), then qLD[nM] | qLDiagInv[nv] (MINVV), then
// cdof_dot[6 nv] | qvel[nv] (JDOTV) -- of the largest size asked for, made odd; then the block's vectors as columns, dof-major across them
// ([nv][columns, padded to an odd count], when MV, ID or MINVV is asked for); then the dof tree as ints (M_coldof[nM] | dof_Madr[nv] | dof_depth[nv],
// for MINVV).
#define MJB_DYN_BLOCK 256
#define MJB_DYN_LDS_BYTES (40 * 1024)  // a block's budget: four blocks per CU
#define MJB_DYN_MAX_EPB 32             // whole envs per block at most (a request for M alone has no lane count that would limit them)
struct DynShape {
	int epb, vpb, ppb;  // envs, vectors and points per block (vpb / ppb 0: none asked for)
	int tiles;          // blocks per group of epb envs
	int env_doubles;    // doubles of an env's region
	int cols_pad;       // columns of the vector block: epb * vpb, made odd (0: no vectors)
	int lds_bytes;
};
inline DynShape mjb_dyn_shape(int nv, int nM, int nvec, int npoint, int outputs)
{
	const bool needM = (outputs & (MJB_DYN_OUT_M | MJB_DYN_OUT_MV | MJB_DYN_OUT_ID)) != 0, solve = (outputs & MJB_DYN_OUT_MINVV) != 0;
	const bool vecs = (outputs & (MJB_DYN_OUT_MV | MJB_DYN_OUT_MINVV | MJB_DYN_OUT_ID)) != 0, jdot = (outputs & MJB_DYN_OUT_JDOTV) != 0;
	int region = 1;
	if (needM && nM > region) region = nM;
	if (solve && nM + nv > region) region = nM + nv;
	if (jdot && 7 * nv > region) region = 7 * nv;
	auto bytes = [&](int epb, int vpb, DynShape *out) {
		DynShape s{};
		s.epb = epb;
		s.vpb = vpb;
		s.env_doubles = region | 1;  // (odd: the same field of neighbouring envs falls on different banks)
		s.cols_pad = vpb ? ((epb * vpb) | 1) : 0;
		const int ints = solve ? nM + 2 * nv : 0;
		s.lds_bytes = 8 * (epb * s.env_doubles + nv * s.cols_pad + (ints + 1) / 2);
		if (out) *out = s;
		return s.lds_bytes;
	};
	const int nvk = vecs ? nvec : 0, npt = jdot ? npoint : 0;
	int vpb = nvk < MJB_DYN_BLOCK ? nvk : MJB_DYN_BLOCK;
	while (vpb > 1 && bytes(1, vpb, nullptr) > MJB_DYN_LDS_BYTES) vpb--;  // (one vector of one env fits for every model mjb_compile takes: nv <= 64, at most 26 KiB)
	const int ppb = npt < MJB_DYN_BLOCK / 6 ? npt : MJB_DYN_BLOCK / 6;
	int epb = 1;
	if (vpb == nvk && ppb == npt)
		while (epb < MJB_DYN_MAX_EPB && (epb + 1) * vpb <= MJB_DYN_BLOCK && (epb + 1) * ppb * 6 <= MJB_DYN_BLOCK && bytes(epb + 1, vpb, nullptr) <= MJB_DYN_LDS_BYTES) epb++;
	DynShape s;
	bytes(epb, vpb, &s);
	s.ppb = ppb;
	const int vt = vpb ? (nvk + vpb - 1) / vpb : 1, pt = ppb ? (npt + ppb - 1) / ppb : 1;
	s.tiles = vt > pt ? vt : pt;
	return s;
}

// every configured output of every env, from DevState::frame_ws; out_* are NULL for the outputs that were not asked for.  V [nenv][nvec][nv] is the
// batch's input block (NULL with nvec == 0), tab the point table (NULL with npoint == 0).  unintegrate != 0: the launch that left the frame also
// advanced qvel by timestep * eulerx (a step's second half), and JDOTV takes that update back to get the velocities the frame belongs to.
// (implemented in mjb_dyn.hip; returns hipError_t as int)
int mjb_launch_dyn(const KernelParams *Pdev, const int *full_adr, const double *tab, const double *V, int nenv, int nvec, int npoint, int nv, int nM, int unintegrate, double *out_M,
                   double *out_MV, double *out_MinvV, double *out_ID, double *out_Jdotv, void *stream);
