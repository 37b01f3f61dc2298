// mjb_jac.h — what the batched Jacobian kernel (mjb_jac.hip) shares with the batch side of the C-ABI (mjb_api.hip, mjb_jac_*): the point table,
// the shape of a launch, and the Jacobian column.
#pragma once

#include "../../include/mjb.h"
#include "mjb_dev.h"

// The point table of mjb_launch_jac: pnt[npoint][3] as doubles, then one JacPoint per point.  mjb_jac_configure resolves what does not depend on
// the env: the body the point is fixed to, that body's tree root (whose subtree_com the tree's cdof are taken about) and its row of body_dofmask.
struct JacPoint {
	int type, id;      // MJB_JAC_*, and the object's id
	int body, root;    // the object's body, body_rootid of it
	unsigned int mask[2];  // DevModel::body_dofmask of the body: bit d set, dof d moves the point
	int pad[2];
};
static_assert(sizeof(JacPoint) == 32, "point records of the Jacobian kernel");

// The shape of a launch: a block of MJB_JAC_BLOCK lanes takes `epb` whole envs and all their points (a short point set), or -- a set too long for
// that -- a tile of `ppb` points of one env.  LDS, in doubles: per env cdof | qvel | the points' positions and reference points | qLD | qLDiagInv
// (the last two when a solve is asked for), then the rows J[r] of every (env, point), dof-major across the rows ([nv][rows, padded to an odd count]),
// then the dof tree as ints (coldof[nM] | Madr[nv] | depth[nv], when a solve is asked for).
#define MJB_JAC_BLOCK 256
#define MJB_JAC_LDS_BYTES (40 * 1024)  // a block's budget: four blocks per CU
struct JacShape {
	int epb, ppb;       // envs per block, points per block
	int env_doubles;    // doubles per env ahead of the rows
	int rows_pad;       // lanes of the row block: epb * ppb * 6, made odd
	int lds_bytes;
};
inline JacShape mjb_jac_shape(int nv, int nM, int npoint, bool solve)
{
	auto bytes = [&](int epb, int ppb, JacShape *out) {
		JacShape s;
		s.epb = epb;
		s.ppb = ppb;
		s.env_doubles = (7 * nv + 6 * ppb + (solve ? nM + nv : 0)) | 1;  // (odd: the same field of neighbouring envs falls on different banks)
		s.rows_pad = (epb * ppb * 6) | 1;
		const int ints = solve ? nM + 2 * nv : 0;
		s.lds_bytes = 8 * (epb * s.env_doubles + nv * s.rows_pad + (ints + 1) / 2);
		if (out) *out = s;
		return s.lds_bytes;
	};
	JacShape s;
	int ppb = npoint < MJB_JAC_BLOCK / 6 ? npoint : MJB_JAC_BLOCK / 6;
	while (ppb > 1 && bytes(1, ppb, nullptr) > MJB_JAC_LDS_BYTES) ppb--;  // (one point of one env fits for every model mjb_compile takes: nv <= 64, at most 34 KiB)
	int epb = 1;
	if (ppb == npoint)
		while ((epb + 1) * ppb * 6 <= MJB_JAC_BLOCK && bytes(epb + 1, ppb, nullptr) <= MJB_JAC_LDS_BYTES) epb++;
	bytes(epb, ppb, &s);
	return s;
}

#if defined(__HIPCC__)
#include "mjb_math.h"
// column d of the Jacobian of point p fixed to a body: (cdof_ang x (p - subtree_com[root]) + cdof_lin, cdof_ang), zero when dof d does not move the
// body.  The arithmetic of point_jac (mjb_step.hip: site transmissions, gravity compensation), on operands the caller has staged: cd = cdof of dof d,
// rc = subtree_com of the body's root, moves = the dof's bit of the body's row of body_dofmask.
DEVI void jac_column(bool moves, const double *cd, const double *rc, const double *p, double *jp, double *jr)
{
	if (!moves) {
		jp[0] = jp[1] = jp[2] = jr[0] = jr[1] = jr[2] = 0;
		return;
	}
	const double off[3] = { p[0] - rc[0], p[1] - rc[1], p[2] - rc[2] };
	cross3(jp, cd, off);
	jp[0] += cd[3]; jp[1] += cd[4]; jp[2] += cd[5];
	jr[0] = cd[0]; jr[1] = cd[1]; jr[2] = cd[2];
}
#endif

// every configured point of every env, from DevState::frame_ws; out_* are NULL for the outputs that were not asked for (implemented in mjb_jac.hip; returns hipError_t as int)
int mjb_launch_jac(const KernelParams *Pdev, const double *tab, int nenv, int npoint, int nv, int nM, double *out_J, double *out_MinvJT, double *out_Ainv, double *out_vel,
                   void *stream);
