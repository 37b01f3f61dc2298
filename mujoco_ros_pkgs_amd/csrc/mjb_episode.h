// mjb_episode.h — what the episode kernel (mjb_episode.hip) shares with the batch side of the C-ABI (mjb_api.hip, mjb_episode_*): the shape of a
// launch and its argument block.
#pragma once

#include "../../include/mjb.h"
#include "mjb_dev.h"

// A block of MJB_EP_BLOCK lanes takes a group of MJB_EP_GROUP consecutive envs: one wavefront's worth, so that the group's done flags are one ballot.
#define MJB_EP_BLOCK 256
#define MJB_EP_GROUP 64

// The fourth Philox counter word of the episode stream is MJB_EP_STREAM + idx: the top bit keeps it apart from the control-noise and sensor-noise streams
// (philox_normal, small idx) under the same seed.  idx = d (position draw of dof d), nv + d (velocity draw), 2 nv (the bank pick).
#define MJB_EP_STREAM 0x80000000u

struct EpisodeArgs {
	// done: mjb_episode_step (use_rule = 1) = the rule OR mask; mjb_episode_reset (use_rule = 0) = mask alone, NULL = every env
	const unsigned char *mask;  // [nenv], device, or NULL
	int use_rule;
	int ninit;                  // rows of the bank (0: qpos0, zero, zero)
	double time_limit;          // <= 0: no time rule
	const double *box;          // lo[nq] | hi[nq] (+-inf: no bound), or NULL: no box
	const double *bank;         // qpos[ninit][nq] | qvel[ninit][nv] | act[ninit][na], or NULL with ninit == 0
	const double *qrange;       // lo[nv] | hi[nv] of the position draw in tangent space, or NULL: the bank row's qpos as it stands
	const double *vrange;       // lo[nv] | hi[nv] of the velocity draw, or NULL
	int clamp, pad;
	unsigned long long seed;
	long long env_offset;
	unsigned char *done;        // [nenv] 1 / 0, every env
	unsigned int *episode;      // [nenv] resets so far: the draw's episode, then incremented
	unsigned int *ndone;        // one word, zero when the kernel starts (the launcher clears it on the stream ahead of the kernel)
};

// one launch for every env of the batch, asynchronous on `stream` (implemented in mjb_episode.hip; returns hipError_t as int)
int mjb_launch_episode(const KernelParams *Pdev, const EpisodeArgs &a, int nenv, void *stream);
