// mjb_model.h — the compiled model (mjb_model) and what the model compiler (mjb_model.hip) shares with the batch side of the C-ABI (mjb_api.hip):
// the error helper and the tables of the data fields.  Host only.
#pragma once

#include <vector>

#include "mjb_dev.h"

#pragma GCC visibility push(hidden)  // (shared by the library's own translation units, not part of its ABI)

// records the message mjb_last_error returns (per thread) and hands `code` back: `return fail(MJB_EINVAL, "...")`.  Defined in mjb_model.hip.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

struct FieldInfo {
	const char *name;
	const char *rows;
	const char *cols;  // literal or size name (DD2)
	int kind;          // 0 state, 1 derived double, 2 derived double (2 size names), 3 int
};
extern const FieldInfo kFields[MJB_F_COUNT];  // include/mjb_data_fields.def, in the order of enum mjb_field

// the FrameLayout member that holds data field i's offset (MJB_F_*)
int &field_slot(FrameLayout &L, int i);
int field_slot(const FrameLayout &L, int i);

// the value of a size of the description by its name in the .def tables ("one": 1, a literal: itself)
int size_by_name(const mjb_model_desc &d, const char *n);

// The device model blob, built on the host (mjb_model.hip, one list of tables): what mjb_make_batch uploads as it stands.
struct mjb_model;
struct ModelBlob {
	std::vector<unsigned char> image;  // [ints | doubles]
	size_t dbl_offset = 0;             // byte offset of the double part
	size_t pair_i_offset = 0;          // ... of the per-pair int records (mjb_register_collision patches them on the device)
	DevModel dm{};                     // sizes, options and derived scalars filled in; every pointer member holds its table's byte offset into the image (all ones: a null pointer, the absent tape)
};
ModelBlob build_model_blob(const mjb_model &M);
// ... and once the image sits at `base`: the pointer members of dm, from offsets to addresses
void rebase_model_blob(const mjb_model &M, DevModel &dm, const void *base);

#pragma GCC visibility pop

struct mjb_model {
	mjb_model_desc h{};               // host copy (pointers into hint / hdbl)
	std::vector<int> hint;            // all int arrays, concatenated
	std::vector<double> hdbl;         // all double arrays, concatenated
	std::vector<size_t> ioff, doff;   // offsets of each array inside hint / hdbl (declaration order)
	std::vector<int> M_rowdof, M_coldof, dof_depth, dof_jstart, body_rec, body_rec2, dof_rec, fac_ops, fac_beg, body_dofmask, body_submask, M_dense, body_anc, dof_bodymask, M_sym, body_dofanc, dof_rec2, jnt_rec, flv_hdr, flv_rec, flv_ent;
	std::vector<int> sens_copy, sens_slow, dof_act_adr, dof_act_id;
	std::vector<int> pair_i;       // [ncollpair][8]  per candidate pair: g1, g2, type1, type2, condim, friction rule, collision-function override, 0
	std::vector<double> pair_d;    // [ncollpair][24] size1[3] size2[3] margin gap rbound1 rbound2 solref[2] solimp[5] includemargin friction[3] tran pad[2]
	std::vector<double> sub_S;     // 0/1 subtree matrix as MFMA A operands (mjb_dev.h)
	std::vector<double> lim_d;     // [njnt + ntendon][24] limit items in pair_d's slots (mjb_dev.h)
	std::vector<double> dof_act_mom;  // moment arm of entry t of the per-dof actuator lists (dof_act_adr / dof_act_id)
	int act_tendon = 0;               // some actuator drives a tendon
	std::vector<int> site_act;        // actuators with a site transmission, in actuator order (DevModel::site_act)
	std::vector<int> gravcomp_body;   // bodies with body_gravcomp != 0, ascending (DevModel::gravcomp_body; its size is mjModel.ngravcomp)
	std::vector<double> damp_int;  // [nv] -diag(D) of the integrator's implicit matrix M + h diag(.): dof_damping (Euler) / implicitfast's constant velocity derivative
	std::vector<int> lim_i;        // [njnt + ntendon][4]
	int sens_ncopy[3] = { 0, 0, 0 }, sens_nslow[3] = { 0, 0, 0 }, sens_ncopy_max = 0;
	int eulerdamp = 0, maxdepth = 0, kin_rounds = 0, need_rnepost = 0, nfriction = 0, sub_nt = 0, dofanc_max = 0, flv_n = 0;
	int field_size[MJB_F_COUNT]{};
	FrameLayout L{}, Lc{};
	// kernel variant 4 (Newton, capacity > 128 rows): a second, WIDE fused frame that holds 128 rows of efc_J and of every per-row
	// array (two envs per CU instead of four).  A batch whose env-steps mostly exceed 64 rows runs its long launches on it: those steps
	// take the two-rows-per-lane solver on LDS instead of the four-rows-per-lane one on the env's block in HBM (launch(), wide policy).
	FrameLayout Lw{};
	bool has_wide = false;
	// the row-slot solver (kernel variants 10 - 13): Newton / CG models beyond the register-row kernels -- more than 256 rows of capacity, or
	// a full frame larger than one CU's LDS.  Their fused frame holds every row (no efc_Jg, no wide frame); a launch whose frame exceeds
	// the LDS budget runs it from the env's slot of DevState::frame_ws (variants 12 / 13)
	bool slot = false;
	bool hbm_full = false, hbm_fused = false;  // the full / fused frame lives in HBM
	int le_topo = -1;  // compiled-in topology of the lane = env kernel the model matches (mjb_lane_env.hip); -1: none; -2: eligible, built by hiprtc on first use
	std::vector<double> le_tape;  // its constant tape (mjb_dev.h), empty without a topology
	int sm_topo = -1;  // compiled-in topology of the split step's smooth kernel (mjb_smooth.hip) when the model's constraint half fits mjb_cstep_kernel too; -1: none
};
