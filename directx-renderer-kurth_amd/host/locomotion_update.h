// locomotion_update.h — the host interface of the PPO gradient step (locomotion_update.hip), called by the batch's C-ABI
// (locomotion_batch.hip: updatePhysicsBatchPPODevice, gradientsPhysicsBatchPPODevice).  Everything is enqueued on the given stream;
// nothing here synchronises.
//
// The flat parameter order, used by the gradient, by Adam's m and v and by gradientsPhysicsBatchPPODevice, is the order of the device's
// master copy:  actor W1T [66][H], b1 [H], W2T [H][H], b2 [H], W3T [H][27], b3 [27];  critic W1T [66][Hv], b1 [Hv], W2T [Hv][Hv], b2 [Hv],
// w3 [Hv], b3 [1];  logStd [27].  ppoTotal(H, Hv) floats.
#pragma once
#include <hip/hip_runtime.h>

#include "locomotion_policy.h"

enum { PPO_MAX_GROUPS = 128, PPO_STATS = 5, PPO_GROUP_STATS = 4, PPO_BLOCK = 256 };

// The master copy: the two device networks and dScales (std [27], logStd [27], ...) of the batch.
struct ppo_parameters { float* policy; float* valueNet; float* scales; uint32_t hidden, valueHidden; };
// rows x {66, 27, 1, 1, 1} device buffers, as collect and gae leave them.
struct ppo_rows { uint32_t rows; const float* obs; const float* actions; const float* oldLogProbs; const float* advantages; const float* returns; };
struct ppo_loss { float clipRange, vfCoef, entCoef; int normalizeAdvantage; };
// slab: ppoGroups(largest minibatch) x ppoTotal floats; partial: ppoBlocks floats; groupStats: PPO_MAX_GROUPS x PPO_GROUP_STATS floats.
struct ppo_scratch { float* slab; float* partial; float* groupStats; };
// torch.optim.Adam's step t: stepSize = lr / (1 - beta1^t), correction2Sqrt = sqrt(1 - beta2^t), both evaluated in double by the caller.
struct ppo_adam { float beta1, beta2, eps, stepSize, correction2Sqrt, maxGradNorm; };

inline size_t ppoTotal(uint32_t hidden, uint32_t valueHidden) { return policyFloats(hidden) + valueFloats(valueHidden) + ACTION_SIZE; }
inline uint32_t ppoTiles(uint32_t count) { return (count + 3) / 4; }
inline uint32_t ppoGroups(uint32_t count) { const uint32_t t = ppoTiles(count); return t < PPO_MAX_GROUPS ? t : PPO_MAX_GROUPS; }
inline uint32_t ppoBlocks(size_t total) { return (uint32_t)((total + PPO_BLOCK - 1) / PPO_BLOCK); }

// The unclipped gradient of ppo_loss on the minibatch order[0 .. count) (row indices into `data`; null: rows 0 .. count-1) into grad
// [ppoTotal], the sums of squares of its blocks of PPO_BLOCK into scratch.partial.  ratios (may be null) [count]: exp(logp - old) per
// minibatch row.  stats (may be null): {loss, policy loss, value loss, clip fraction} into stats[0 .. 3].  Two launches.
__attribute__((visibility("hidden"))) int ppoGradients(hipStream_t stream, const ppo_parameters& p, const ppo_rows& data, const uint32_t* order, uint32_t count, const ppo_loss& loss,
	const ppo_scratch& scratch, float* grad, float* ratios, float* stats);
// clip_grad_norm_ and one Adam step on the master copy, from grad and scratch.partial of ppoGradients; std follows logStd.  stats (may
// be null): the gradient's norm before clipping into stats[4].  One launch.
__attribute__((visibility("hidden"))) int ppoAdam(hipStream_t stream, const ppo_parameters& p, const ppo_scratch& scratch, const float* grad, float* m, float* v, const ppo_adam& adam, float* stats);
