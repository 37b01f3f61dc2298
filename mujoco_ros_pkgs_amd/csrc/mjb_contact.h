// mjb_contact.h — what the batched contact-wrench kernel (mjb_contact.hip) shares with the batch side of the C-ABI (mjb_api.hip, mjb_contact_*): the
// query table and the shape of a launch.
#pragma once

#include "../../include/mjb.h"
#include "mjb_dev.h"

// The query table of mjb_launch_contact, as 32-bit words: the geom sets as bit words, mask[nquery][2][nwords] (A, then B; bit g & 31 of word g >> 5 set:
// geom g is a member), then ref_body[nquery] (-1: the world origin).  mjb_contact_configure builds it.
inline int mjb_contact_mask_words(int ngeom) { return (ngeom + 31) / 32; }
inline size_t mjb_contact_table_words(int ngeom, int nquery) { return (size_t)nquery * 2 * mjb_contact_mask_words(ngeom) + (size_t)nquery; }

// The shape of a launch: a block of MJB_CON_BLOCK lanes takes `epb` whole envs and all their queries (a short query list), or -- a list too long for
// that -- a tile of `qpb` queries of one env.  It walks its envs' contacts in tiles of `ct` contacts per env; the sums are carried in registers across
// the tiles, so no result depends on ct.  LDS, in doubles: one slot of MJB_CON_SLOT doubles per (env, contact of the tile) | the reference points
// r_q [epb][qpb][3] | the wrenches on their way out [epb][qpb][6]; then as 32-bit words the block's masks [qpb][2][nwords] | ncon [epb].
// A slot: contact_frame[9] | contact_pos[3] | contact_dist | contact_friction[5] | the contact's rows of efc_force[10] | geom1, geom2, dim, efc_address as
// ints | one double of padding (an odd stride: the same field of neighbouring contacts falls on different banks).  The decode phase rewrites the slot
// in place: lf[6] | F[3] over the frame, T[3] over the first rows of efc_force.
#define MJB_CON_BLOCK 256
#define MJB_CON_LDS_BYTES (40 * 1024)      // a block's budget: four blocks per CU
#define MJB_CON_LDS_LIMIT (64 * 1024)      // what a launch may ask for; only the masks of a model with some 100 000 geoms take a block beyond the budget
#define MJB_CON_SLOT 31
#define MJB_CON_ROWS 10                    // rows of a contact at most: pyramidal, condim 6
enum { MJB_CON_S_FRAME = 0, MJB_CON_S_POS = 9, MJB_CON_S_DIST = 12, MJB_CON_S_FRICTION = 13, MJB_CON_S_FORCE = 18, MJB_CON_S_INTS = 28,
       MJB_CON_S_LF = 0, MJB_CON_S_F = 6, MJB_CON_S_T = 18 };
struct ConShape {
	int epb, qpb, ct;  // envs per block, queries per block, contacts per env and tile
	int nwords;        // words of one geom set
	int lds_bytes;
};
inline ConShape mjb_contact_shape(int ngeom, int nconmax, int nquery)
{
	ConShape s;
	s.nwords = mjb_contact_mask_words(ngeom);
	auto bytes = [&](int epb, int qpb, int ct) { return 8 * (epb * ct * MJB_CON_SLOT + epb * qpb * 9) + 4 * (qpb * 2 * s.nwords + epb); };
	int qpb = nquery < MJB_CON_BLOCK ? nquery : MJB_CON_BLOCK;
	while (qpb > 1 && (long long)qpb * 2 * s.nwords * 4 > MJB_CON_LDS_BYTES / 4) qpb--;  // (the masks take a quarter of the budget at most; one query's always go in)
	const int goal = nconmax < 8 ? (nconmax < 1 ? 1 : nconmax) : 8;  // contacts of a tile the envs per block are sized for: the arm's envs hold fewer, the hand's take two tiles
	int epb = 1;
	if (qpb == nquery) {
		epb = MJB_CON_BLOCK / qpb;
		if (epb > MJB_CON_BLOCK / 2 / goal) epb = MJB_CON_BLOCK / 2 / goal;
		if (epb < 1) epb = 1;
	}
	int ct = MJB_CON_BLOCK / 2 / epb;
	if (ct > nconmax) ct = nconmax;
	if (ct < 1) ct = 1;
	while (ct > 1 && bytes(epb, qpb, ct) > MJB_CON_LDS_BYTES) ct--;
	while (epb > 1 && bytes(epb, qpb, ct) > MJB_CON_LDS_BYTES) epb--;
	s.epb = epb;
	s.qpb = qpb;
	s.ct = ct;
	s.lds_bytes = (bytes(epb, qpb, ct) + 15) & ~15;
	return s;
}

// every configured query of every env, from DevState::frame_ws; out_* are NULL for the outputs that were not asked for (implemented in mjb_contact.hip;
// returns hipError_t as int)
int mjb_launch_contact(const KernelParams *Pdev, const unsigned int *tab, int nenv, int nquery, int ngeom, int nconmax, double *out_wrench, double *out_normal, int *out_count,
                       double *out_dist, double *out_contacts, void *stream);
