// locomotion_update.hip — the PPO gradient step of training.py (PPOTrainer.iterate's inner loop) on the device: three launches per
// minibatch, all float32, no atomics, no host synchronisation.
//
//   k_loco_ppo_backward   a group (workgroup) takes tiles of POLICY_TILE minibatch rows: gathers them by index, runs the actor and the
//                         critic forward with forwardActorCritic (what collect ran), forms ppo_loss's per-row terms, backpropagates, and
//                         stores the tile's weight gradients to its own row of a slab [groups][parameters].  A group that takes more than
//                         one tile (more than PPO_MAX_GROUPS tiles in the minibatch) adds them into its row in tile order.  Every group
//                         recomputes the minibatch's advantage mean and std itself, in one fixed order.
//   k_loco_ppo_reduce     one lane per parameter adds the slab's rows in ascending group order (+ the entropy term of logStd), and every
//                         block stores the sum of the squares of its PPO_BLOCK gradients.
//   k_loco_ppo_adam       every block adds those sums in one fixed order: the global norm; then clip_grad_norm_'s scale and
//                         torch.optim.Adam's step on the master copy (the two networks and dScales), and std = exp(logStd) beside it.
//
// Every sum has one order that depends only on the shapes, so a step is bit-reproducible.  The tile's four rows are added as
// fma(r3, fma(r2, fma(r1, r0))), the slab's rows one by one.
#include <hip/hip_runtime.h>
#include <cstdio>

#include "locomotion_layers.h"
#include "locomotion_update.h"

namespace
{
	__device__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
	__device__ float sum4(float4 a) { return ((a.x + a.y) + a.z) + a.w; }
	__device__ float4 fma4(float w, float4 d, float4 s) { return make_float4(fmaf(w, d.x, s.x), fmaf(w, d.y, s.y), fmaf(w, d.z, s.z), fmaf(w, d.w, s.w)); }
	__device__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
	// d tanh: 1 - a^2 per row
	__device__ float4 tanhSlope(float4 a) { return make_float4(1.f - a.x * a.x, 1.f - a.y * a.y, 1.f - a.z * a.z, 1.f - a.w * a.w); }
	__device__ void put(float* p, float v, bool first) { *p = first ? v : *p + v; }

	// The sum of v over the block, the same in every thread: each lane of wave 0 adds its column of `scratch` in ascending order, then
	// the wave halves itself five times.  blockDim.x is a multiple of 64, at most PPO_BLOCK; scratch holds PPO_BLOCK + 1 floats.
	__device__ float blockSum(float v, float* scratch)
	{
		const uint32_t t = threadIdx.x;
		__syncthreads();
		scratch[t] = v;
		__syncthreads();
		if (t < 64)
		{
			float s = scratch[t];
			for (uint32_t k = t + 64; k < blockDim.x; k += 64) s += scratch[k];
			for (int offset = 32; offset > 0; offset >>= 1) s += __shfl_down(s, offset, 64);
			if (t == 0) scratch[PPO_BLOCK] = s;
		}
		__syncthreads();
		return scratch[PPO_BLOCK];
	}

	// Backpropagation through one layer for one input unit: sum_k W[unit][k] * d[k] over the layer's outputs in ascending k, the tile's
	// four rows side by side.  `row` is the unit's line of the [in][out] weights; with outputs a multiple of 4 it is read 16 bytes at a time.
	__device__ float4 backLayer(const float* __restrict__ row, uint32_t outputs, const float4* d)
	{
		float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
		if ((outputs & 3) == 0 && (((size_t)row) & 15) == 0)
			for (uint32_t k = 0; k < outputs; k += 4)
			{
				const float4 w = *(const float4*)(row + k);
				s = fma4(w.x, d[k], s); s = fma4(w.y, d[k + 1], s); s = fma4(w.z, d[k + 2], s); s = fma4(w.w, d[k + 3], s);
			}
		else
			for (uint32_t k = 0; k < outputs; ++k) s = fma4(row[k], d[k], s);
		return s;
	}

	// The gradients of the two hidden layers of one network for the tile, into the group's slab row `g` (the network's part of it, in
	// the network's own layout).  dz2 [hidden] is in LDS (`back`, written before a barrier) and, for this lane's unit, in `mine`; a1 is the
	// first tanh vector, a1Mine this lane's entry of it.
	__device__ void backHidden(const locomotion_policy& n, const float* base, uint32_t hidden, float* g, const float4* input, const float4* a1, float4 a1Mine, const float4* back, float4 mine, bool first)
	{
		const uint32_t t = threadIdx.x;
		if (t >= hidden) return;
		float* w2 = g + (n.w[1] - base);
		for (uint32_t i = 0; i < hidden; ++i) put(w2 + (size_t)i * hidden + t, dot4(a1[i], mine), first);
		put(g + (n.b[1] - base) + t, sum4(mine), first);
		const float4 dz1 = mul4(backLayer(n.w[1] + (size_t)t * hidden, hidden, back), tanhSlope(a1Mine));
		float* w1 = g + (n.w[0] - base);
		for (uint32_t x = 0; x < STATE_SIZE; ++x) put(w1 + (size_t)x * hidden + t, dot4(input[x], dz1), first);
		put(g + (n.b[0] - base) + t, sum4(dz1), first);
	}

	__global__ void __launch_bounds__(POLICY_MAX_HIDDEN) k_loco_ppo_backward(uint32_t count, uint32_t rows, const uint32_t* __restrict__ order,
		const float* __restrict__ obs, const float* __restrict__ actions, const float* __restrict__ oldLogProbs, const float* __restrict__ advantages, const float* __restrict__ returns,
		const float* __restrict__ policy, const float* __restrict__ valueNet, const float* __restrict__ scales, uint32_t hidden, uint32_t valueHidden,
		float clipRange, float vfCoef, int normalize, float* __restrict__ slab, size_t total, float* __restrict__ groupStats, float* __restrict__ ratios)
	{
		__shared__ float4 input[STATE_SIZE], hiddenA[POLICY_MAX_HIDDEN], hiddenB[POLICY_MAX_HIDDEN], valueA[POLICY_MAX_HIDDEN], valueB[POLICY_MAX_HIDDEN];
		__shared__ float4 back[POLICY_MAX_HIDDEN], valueBack[POLICY_MAX_HIDDEN];
		__shared__ float4 terms[ACTION_SIZE], zs[ACTION_SIZE], dMean[ACTION_SIZE], valueOut, dLogProb, dValue;
		__shared__ float invStd[ACTION_SIZE], sums[PPO_BLOCK + 1], rowStats[POLICY_TILE][3];
		__shared__ uint32_t rowOf[POLICY_TILE];
		const uint32_t t = threadIdx.x;
		const locomotion_policy p = networkOf(policy, hidden, ACTION_SIZE), v = networkOf(valueNet, valueHidden, 1);
		const float* logStd = scales + ACTION_SIZE;
		auto rowAt = [&](uint32_t i) { const uint32_t r = order ? order[i] : i; return r < rows ? r : rows - 1; }; // a bad index reads the last row, never past it

		// training.normalize_advantages over the minibatch: mean, then the std with Bessel's correction
		float mean = 0.f, spread = 1.f;
		if (normalize && count > 1)
		{
			float s = 0.f;
			for (uint32_t i = t; i < count; i += blockDim.x) s += advantages[rowAt(i)];
			mean = blockSum(s, sums) / (float)count;
			float q = 0.f;
			for (uint32_t i = t; i < count; i += blockDim.x) { const float d = advantages[rowAt(i)] - mean; q += d * d; }
			spread = sqrtf(blockSum(q, sums) / (float)(count - 1)) + 1e-8f;
		}
		if (t < ACTION_SIZE) invStd[t] = (float)exp(-(double)logStd[t]);
		float surrogate = 0.f, valueError = 0.f, clipped = 0.f; // lanes 0..3: this row's share of the statistics, over the group's tiles

		float* g = slab + (size_t)blockIdx.x * total;
		float* gPolicy = g; float* gValue = g + policyFloats(hidden); float* gLogStd = gValue + valueFloats(valueHidden);
		const uint32_t tiles = (count + POLICY_TILE - 1) / POLICY_TILE;
		bool first = true;
		for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, first = false)
		{
			const uint32_t firstRow = tile * POLICY_TILE;
			__syncthreads(); // the previous tile's LDS is done with
			loadTile(input, obs, nullptr, firstRow, count, rowAt);
			if (t < POLICY_TILE) rowOf[t] = firstRow + t < count ? rowAt(firstRow + t) : ~0u;
			__syncthreads();
			const forward_pair f = forwardActorCritic(p, v, input, hiddenA, hiddenB, valueA, valueB);
			if (t == criticLane()) valueOut = f.value;
			if (t < ACTION_SIZE) // z = (action - mean) / std and noiseLogProb's term per action
			{
				const float mu[POLICY_TILE] = { f.out.x, f.out.y, f.out.z, f.out.w };
				float z[POLICY_TILE], term[POLICY_TILE];
				#pragma unroll
				for (uint32_t r = 0; r < POLICY_TILE; ++r)
				{
					const float action = rowOf[r] != ~0u ? actions[(size_t)ACTION_SIZE * rowOf[r] + t] : mu[r];
					z[r] = (action - mu[r]) * invStd[t];
					const float square = z[r] * z[r]; const float half = -0.5f * square;
					term[r] = half - logStd[t];
				}
				zs[t] = make_float4(z[0], z[1], z[2], z[3]); terms[t] = make_float4(term[0], term[1], term[2], term[3]);
			}
			__syncthreads();
			if (t < POLICY_TILE) // one row per lane: ppo_loss's terms and their derivatives to the log-probability and the value
			{
				float dlp = 0.f, dv = 0.f;
				if (rowOf[t] != ~0u)
				{
					const uint32_t row = rowOf[t];
					float sum = 0.f;
					for (int j = 0; j < ACTION_SIZE; ++j) sum += ((const float*)&terms[j])[t];
					const float logProb = sum - 24.811340396526162f;
					const float ratio = expf(logProb - oldLogProbs[row]);
					const float advantage = normalize && count > 1 ? (advantages[row] - mean) / spread : advantages[row];
					const float low = 1.f - clipRange, high = 1.f + clipRange;
					const float plain = advantage * ratio, bounded = advantage * fminf(fmaxf(ratio, low), high);
					surrogate += -fminf(plain, bounded);
					if (plain <= bounded) dlp = -plain / (float)count; // d/dlogp of -min(A r, A clamp(r)) / count; the clamped branch is flat
					const float error = ((const float*)&valueOut)[t] - returns[row];
					valueError += error * error;
					dv = vfCoef * (2.f * error) / (float)count;
					clipped += fabsf(ratio - 1.f) > clipRange ? 1.f : 0.f;
					if (ratios) ratios[firstRow + t] = ratio;
				}
				((float*)&dLogProb)[t] = dlp; ((float*)&dValue)[t] = dv;
			}
			__syncthreads();
			const float4 dlp = dLogProb, dv = dValue;
			if (t < ACTION_SIZE) // d logp / d mean = z / std;  d logp / d logStd = z^2 - 1
			{
				const float4 z = zs[t];
				const float s = invStd[t];
				dMean[t] = make_float4(dlp.x * (z.x * s), dlp.y * (z.y * s), dlp.z * (z.z * s), dlp.w * (z.w * s));
				put(gLogStd + t, dot4(dlp, make_float4(z.x * z.x - 1.f, z.y * z.y - 1.f, z.z * z.z - 1.f, z.w * z.w - 1.f)), first);
			}
			__syncthreads();
			// the last layers: the weights' gradients, and dz2 = (W3^T d) * (1 - b^2) into LDS
			for (uint32_t e = t; e < hidden * ACTION_SIZE; e += blockDim.x) put(gPolicy + (p.w[2] - policy) + e, dot4(hiddenB[e / ACTION_SIZE], dMean[e % ACTION_SIZE]), first);
			if (t < ACTION_SIZE) put(gPolicy + (p.b[2] - policy) + t, sum4(dMean[t]), first);
			float4 dz2 = make_float4(0.f, 0.f, 0.f, 0.f), dvz2 = dz2;
			if (t < hidden) { dz2 = mul4(backLayer(p.w[2] + (size_t)t * ACTION_SIZE, ACTION_SIZE, dMean), tanhSlope(f.b)); back[t] = dz2; }
			if (t < valueHidden)
			{
				put(gValue + (v.w[2] - valueNet) + t, dot4(f.vb, dv), first);
				const float w = v.w[2][t];
				dvz2 = mul4(make_float4(w * dv.x, w * dv.y, w * dv.z, w * dv.w), tanhSlope(f.vb)); valueBack[t] = dvz2;
			}
			if (t == 0) put(gValue + (v.b[2] - valueNet), sum4(dv), first);
			__syncthreads();
			backHidden(p, policy, hidden, gPolicy, input, hiddenA, f.a, back, dz2, first);
			backHidden(v, valueNet, valueHidden, gValue, input, valueA, f.va, valueBack, dvz2, first);
		}
		if (t < POLICY_TILE) { rowStats[t][0] = surrogate; rowStats[t][1] = valueError; rowStats[t][2] = clipped; }
		__syncthreads();
		if (t < 3) groupStats[PPO_GROUP_STATS * blockIdx.x + t] = ((rowStats[0][t] + rowStats[1][t]) + rowStats[2][t]) + rowStats[3][t];
	}

	// One lane per parameter: the slab's rows in ascending order.  Block 0 also closes the statistics that need no norm.
	__global__ void __launch_bounds__(PPO_BLOCK) k_loco_ppo_reduce(const float* __restrict__ slab, size_t total, uint32_t groups, size_t logStdAt, uint32_t count,
		float vfCoef, float entCoef, const float* __restrict__ scales, const float* __restrict__ groupStats, float* __restrict__ grad, float* __restrict__ partial, float* __restrict__ stats)
	{
		__shared__ float sums[PPO_BLOCK + 1];
		const size_t i = (size_t)blockIdx.x * PPO_BLOCK + threadIdx.x;
		float g = 0.f;
		if (i < total)
		{
			for (uint32_t w = 0; w < groups; ++w) g += slab[(size_t)w * total + i];
			if (i >= logStdAt) g -= entCoef; // -ent_coef * mean(entropy), entropy = sum_j(logStd_j + const)
			grad[i] = g;
		}
		const float squares = blockSum(g * g, sums);
		if (threadIdx.x == 0) partial[blockIdx.x] = squares;
		if (stats && blockIdx.x == 0 && threadIdx.x == 0)
		{
			float s[3] = { 0.f, 0.f, 0.f };
			for (uint32_t w = 0; w < groups; ++w) for (int k = 0; k < 3; ++k) s[k] += groupStats[PPO_GROUP_STATS * w + k];
			float entropy = 0.f;
			for (int j = 0; j < ACTION_SIZE; ++j) entropy += 1.4189385332046727f + scales[ACTION_SIZE + j]; // 0.5 + 0.5 log(2 pi)
			const float policyLoss = s[0] / (float)count, valueLoss = s[1] / (float)count;
			stats[0] = policyLoss + vfCoef * valueLoss - entCoef * entropy; stats[1] = policyLoss; stats[2] = valueLoss; stats[3] = s[2] / (float)count;
		}
	}

	// clip_grad_norm_ (scale = min(1, max / (norm + 1e-6))) and torch.optim.Adam's step, one lane per parameter.
	__global__ void __launch_bounds__(PPO_BLOCK) k_loco_ppo_adam(size_t total, size_t policyCount, size_t valueCount, float* __restrict__ policy, float* __restrict__ valueNet, float* __restrict__ scales,
		const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ partial, uint32_t blocks, ppo_adam adam, float* __restrict__ stats)
	{
		__shared__ float sums[PPO_BLOCK + 1];
		float s = 0.f;
		for (uint32_t i = threadIdx.x; i < blocks; i += PPO_BLOCK) s += partial[i];
		const float norm = sqrtf(blockSum(s, sums));
		if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[4] = norm;
		const float scale = fminf(1.f, adam.maxGradNorm / (norm + 1e-6f));
		const size_t i = (size_t)blockIdx.x * PPO_BLOCK + threadIdx.x;
		if (i >= total) return;
		float* parameter = i < policyCount ? policy + i : i < policyCount + valueCount ? valueNet + (i - policyCount) : scales + ACTION_SIZE + (i - policyCount - valueCount);
		const float g = grad[i] * scale;
		const float average = m[i] + (g - m[i]) * (1.f - adam.beta1);
		const float square = v[i] * adam.beta2 + (1.f - adam.beta2) * (g * g);
		m[i] = average; v[i] = square;
		const float denominator = sqrtf(square) / adam.correction2Sqrt + adam.eps;
		const float next = *parameter - adam.stepSize * (average / denominator);
		*parameter = next;
		if (i >= policyCount + valueCount) scales[i - policyCount - valueCount] = (float)exp((double)next); // set_log_std's statement
	}

	bool launched(const char* what)
	{
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) { fprintf(stderr, "locomotion update: %s: %s\n", what, hipGetErrorString(e)); return false; }
		return true;
	}
}

int ppoGradients(hipStream_t stream, const ppo_parameters& p, const ppo_rows& data, const uint32_t* order, uint32_t count, const ppo_loss& loss,
	const ppo_scratch& scratch, float* grad, float* ratios, float* stats)
{
	const size_t total = ppoTotal(p.hidden, p.valueHidden);
	const uint32_t groups = ppoGroups(count), widest = p.hidden > p.valueHidden ? p.hidden : p.valueHidden;
	hipLaunchKernelGGL(k_loco_ppo_backward, dim3(groups), dim3(64 * ((widest + 63) / 64)), 0, stream, count, data.rows, order, data.obs, data.actions, data.oldLogProbs, data.advantages,
		data.returns, (const float*)p.policy, (const float*)p.valueNet, (const float*)p.scales, p.hidden, p.valueHidden, loss.clipRange, loss.vfCoef, loss.normalizeAdvantage,
		scratch.slab, total, scratch.groupStats, ratios);
	if (!launched("backward kernel")) return MI_ERR_HIP;
	hipLaunchKernelGGL(k_loco_ppo_reduce, dim3(ppoBlocks(total)), dim3(PPO_BLOCK), 0, stream, (const float*)scratch.slab, total, groups, total - ACTION_SIZE, count, loss.vfCoef, loss.entCoef,
		(const float*)p.scales, (const float*)scratch.groupStats, grad, scratch.partial, stats);
	return launched("reduce kernel") ? 0 : MI_ERR_HIP;
}

int ppoAdam(hipStream_t stream, const ppo_parameters& p, const ppo_scratch& scratch, const float* grad, float* m, float* v, const ppo_adam& adam, float* stats)
{
	const size_t total = ppoTotal(p.hidden, p.valueHidden);
	hipLaunchKernelGGL(k_loco_ppo_adam, dim3(ppoBlocks(total)), dim3(PPO_BLOCK), 0, stream, total, policyFloats(p.hidden), valueFloats(p.valueHidden), p.policy, p.valueNet, p.scales,
		grad, m, v, (const float*)scratch.partial, ppoBlocks(total), adam, stats);
	return launched("adam kernel") ? 0 : MI_ERR_HIP;
}
