// mjb_episode.hip -- device-side episode resets (mjb_episode_*): the done rule, the reset of the done envs to a row of the initial-state bank with
// seeded noise, and the episode counters, for every env in one launch on the batch's stream.  Nothing here synchronises or crosses the host.
//
// A block of 256 lanes takes a group of 64 consecutive envs (mjb_episode.h).  The state arrays are env-major, so every field of the group is one
// contiguous run of HBM.  The phases, a barrier between any two:
//   1  done.  Lane t of the first wavefront reads time and the mask of env t of the group (64 neighbouring addresses each); with a box, all lanes walk
//      the group's qpos run with one element per lane, consecutive lanes at consecutive addresses, and raise the env's flag in LDS where a coordinate
//      is outside (NaN included: the test is !(lo <= q <= hi)).
//   2  The first wavefront writes done[env], adds its ballot's population to ndone with one vector atomic, compacts the done envs into a list in
//      LDS, reads and increments their episode counters and draws their bank rows.  A block without a done env ends here.
//   3  reset.  For each state field the lanes spread over the flattened (done env, element) pairs, element fastest: the stores of neighbouring lanes
//      go to neighbouring addresses of one env, and the work is the done envs', not the group's.  qvel takes one lane per (env, dof), qpos one lane
//      per (env, joint) -- a ball or free joint's quaternion is one lane's -- and the mocap poses one lane per (env, body).  A Philox call is made
//      for a done env's dofs only, and only for the parts that have a range.
// Every value is computed by one lane from the env's global index, its episode and the dof: no result depends on the launch or the batch's shape.
#include <hip/hip_runtime.h>

#include "mjb_dev.h"
#include "mjb_episode.h"
#include "mjb_math.h"

namespace {

// u in (0, 1): the first output word of Philox-4x32-10 (the rounds and the counter layout of philox_normal, mjb_math.h), (w0 + 0.5) / 2^32
DEVI double episode_u(unsigned long long seed, unsigned long long genv, unsigned int episode, unsigned int idx)
{
	unsigned int c0 = (unsigned int)genv, c1 = (unsigned int)(genv >> 32), c2 = episode, c3 = MJB_EP_STREAM + idx;
	unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
	for (int r = 0; r < 10; r++) {
		unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
		unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
		unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned int)p1;
		unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned int)p0;
		c0 = n0; c1 = n1; c2 = n2; c3 = n3;
		k0 += 0x9E3779B9u;
		k1 += 0xBB67AE85u;
	}
	return ((double)c0 + 0.5) * (1.0 / 4294967296.0);
}

__global__ void __launch_bounds__(MJB_EP_BLOCK) mjb_episode_kernel(const KernelParams MJB_AS4 *__restrict__ P, const EpisodeArgs a)
{
	__shared__ int flag[MJB_EP_GROUP];          // done, by env of the group
	__shared__ int list[MJB_EP_GROUP];          // the done envs of the group, ascending
	__shared__ int pick[MJB_EP_GROUP];          // their bank rows ...
	__shared__ unsigned int epi[MJB_EP_GROUP];  // ... and the episodes of their draws (both by env of the group)
	__shared__ int ndone_lds;
	const DevModel MJB_AS4 &m = P->m;
	const DevState MJB_AS4 &s = P->s;
	const int nenv = s.nenv, nq = m.nq, nv = m.nv, na = m.na, nu = m.nu, nbody = m.nbody, njnt = m.njnt;
	const int t = (int)threadIdx.x, NT = (int)blockDim.x;
	const int env0 = (int)blockIdx.x * MJB_EP_GROUP;
	const int ne = min(MJB_EP_GROUP, nenv - env0);  // envs of this group (the grid covers nenv: at least one)

	// ---- 1: done
	if (t < MJB_EP_GROUP) {
		int d = 0;
		if (t < ne) {
			const size_t env = (size_t)(env0 + t);
			if (a.use_rule) {
				d = a.time_limit > 0 && s.time[env] >= a.time_limit;
				if (a.mask && a.mask[env]) d = 1;
			} else
				d = a.mask ? a.mask[env] != 0 : 1;
		}
		flag[t] = d;
	}
	__syncthreads();
	if (a.use_rule && a.box) {
		const double *__restrict__ q = s.qpos + (size_t)env0 * nq;
		for (int idx = t; idx < ne * nq; idx += NT) {
			const int le = idx / nq, k = idx - le * nq;
			const double v = q[idx];
			if (!(v >= a.box[k] && v <= a.box[nq + k])) atomicOr(&flag[le], 1);
		}
		__syncthreads();
	}

	// ---- 2: outputs, the list of done envs, their episodes and bank rows
	if (t < MJB_EP_GROUP) {  // (the first wavefront, whole)
		const int d = flag[t];
		const unsigned long long bal = __ballot(d != 0);
		if (t < ne) a.done[env0 + t] = (unsigned char)(d != 0);
		if (t == 0) {
			ndone_lds = __popcll(bal);
			if (bal) atomicAdd(a.ndone, (unsigned int)__popcll(bal));
		}
		if (d) {
			const size_t env = (size_t)(env0 + t);
			list[__popcll(bal & ((1ull << t) - 1))] = t;
			const unsigned int ep = a.episode[env];
			a.episode[env] = ep + 1;
			epi[t] = ep;
			int k = 0;
			if (a.ninit > 0) {
				const double u = episode_u(a.seed, (unsigned long long)(a.env_offset + (long long)env), ep, (unsigned int)(2 * nv));
				k = min(a.ninit - 1, (int)floor(u * (double)a.ninit));
			}
			pick[t] = k;
		}
	}
	__syncthreads();
	const int nd = ndone_lds;
	if (nd == 0) return;

	// ---- 3: reset of the done envs
	// a field of w doubles per env, zeroed
	auto zero = [&](double *__restrict__ field, int w) {
		for (int idx = t; idx < nd * w; idx += NT) {
			const int c = idx / w, k = idx - c * w;
			field[(size_t)(env0 + list[c]) * w + k] = 0;
		}
	};
	zero(s.ctrl, nu);
	zero(s.ctrlnoise, nu);
	zero(s.qacc_warmstart, nv);
	zero(s.qfrc_applied, nv);
	zero(s.qacc, nv);
	zero(s.xfrc_applied, 6 * nbody);
	zero(s.sensordata, m.nsensordata);
	zero(s.time, 1);
	zero(s.energy, 2);

	const double *__restrict__ bank_qpos = a.bank, *__restrict__ bank_qvel = a.bank + (size_t)a.ninit * nq, *__restrict__ bank_act = bank_qvel + (size_t)a.ninit * nv;
	const bool bank = a.ninit > 0;
	for (int idx = t; idx < nd * na; idx += NT) {
		const int c = idx / na, k = idx - c * na, le = list[c];
		s.act[(size_t)(env0 + le) * na + k] = bank ? bank_act[(size_t)pick[le] * na + k] : 0.0;
	}
	for (int idx = t; idx < nd * nv; idx += NT) {  // qvel = bank + dv
		const int c = idx / nv, d = idx - c * nv, le = list[c];
		const size_t env = (size_t)(env0 + le);
		double v = bank ? bank_qvel[(size_t)pick[le] * nv + d] : 0.0;
		if (a.vrange) {
			const double lo = a.vrange[d], hi = a.vrange[nv + d];
			v += lo + (hi - lo) * episode_u(a.seed, (unsigned long long)(a.env_offset + (long long)env), epi[le], (unsigned int)(nv + d));
		}
		s.qvel[env * nv + d] = v;
	}
	for (int idx = t; idx < nd * njnt; idx += NT) {  // qpos = integrate_pos(bank, dq, 1), joint by joint
		const int c = idx / njnt, j = idx - c * njnt, le = list[c];
		const size_t env = (size_t)(env0 + le);
		const unsigned long long genv = (unsigned long long)(a.env_offset + (long long)env);
		const unsigned int ep = epi[le];
		const int jt = m.jnt_type[j], qa = m.jnt_qposadr[j], da = m.jnt_dofadr[j];
		const double *__restrict__ row = bank_qpos + (size_t)pick[le] * nq;
		double *__restrict__ out = s.qpos + env * nq;
		auto src = [&](int k) { return bank ? row[k] : m.qpos0[k]; };
		auto dq = [&](int d) {
			const double lo = a.qrange[d], hi = a.qrange[nv + d];
			return lo + (hi - lo) * episode_u(a.seed, genv, ep, (unsigned int)d);
		};
		if (jt == MJB_JNT_HINGE || jt == MJB_JNT_SLIDE) {
			double q = src(qa);
			if (a.qrange) q += dq(da);
			if (a.clamp && m.jnt_limited[j]) q = fmin(fmax(q, m.jnt_range[2 * j]), m.jnt_range[2 * j + 1]);
			out[qa] = q;
		} else {
			int pa = qa, va = da;
			if (jt == MJB_JNT_FREE) {
				for (int k = 0; k < 3; k++) out[pa + k] = a.qrange ? src(pa + k) + dq(va + k) : src(pa + k);
				pa += 3;
				va += 3;
			}
			double q[4] = { src(pa), src(pa + 1), src(pa + 2), src(pa + 3) };
			if (a.qrange) {
				const double w[3] = { dq(va), dq(va + 1), dq(va + 2) };
				quat_integrate(q, w, 1.0);
			}
			st4(out + pa, q);
		}
	}
	if (m.nmocap > 0)
		for (int idx = t; idx < nd * nbody; idx += NT) {  // mocap poses back to the model's
			const int c = idx / nbody, b = idx - c * nbody;
			const int mid = m.body_mocapid[b];
			if (mid < 0) continue;
			const size_t e = (size_t)(env0 + list[c]);
			for (int k = 0; k < 3; k++) s.mocap_pos[(e * m.nmocap + mid) * 3 + k] = m.body_pos[3 * b + k];
			for (int k = 0; k < 4; k++) s.mocap_quat[(e * m.nmocap + mid) * 4 + k] = m.body_quat[4 * b + k];
		}
}

}  // namespace

int mjb_launch_episode(const KernelParams *Pdev, const EpisodeArgs &a, int nenv, void *stream)
{
	if (nenv < 1) return (int)hipSuccess;
	hipError_t err = hipMemsetAsync(a.ndone, 0, sizeof(unsigned int), (hipStream_t)stream);
	if (err != hipSuccess) return (int)err;
	const int blocks = (nenv + MJB_EP_GROUP - 1) / MJB_EP_GROUP;
	hipLaunchKernelGGL(mjb_episode_kernel, dim3(blocks), dim3(MJB_EP_BLOCK), 0, (hipStream_t)stream, (const KernelParams MJB_AS4 *)Pdev, a);
	return (int)hipGetLastError();
}
