// locomotion_layers.h — the device-side forward pass of the learned controller, stated once for every kernel that runs the networks:
// inference and collection (locomotion_batch.hip) and the PPO gradient step (locomotion_update.hip).  The tile loader, the layer sums
// and the barrier choreography of one network and of actor and critic side by side are here and nowhere else, so the log-probabilities
// the update recomputes are those of the networks the rollout ran.  The networks lie in the device layout: locomotion_policy.h's six
// arrays with every weight matrix transposed to [in][out] (networkOf gives the pointers).
#pragma once
#include <hip/hip_runtime.h>

#include "locomotion_policy.h"

namespace
{
	constexpr uint32_t POLICY_TILE = 4; // rows per pass of policyLayer, all four in the registers of every lane

	// One layer of applyLayer for POLICY_TILE environments: lane = output unit, weights transposed to [in][out] (one coalesced line per
	// input), the tile's inputs in LDS as [in][tile] (one broadcast read per input).  Per unit and environment the products are added
	// in ascending input order, product rounded, then added (-ffp-contract=off), then the bias: the sums of applyLayer, bit for bit.
	__device__ float4 policyLayer(const float* __restrict__ weightsT, const float* __restrict__ bias, uint32_t inputSize, uint32_t outputSize, const float4* from, uint32_t unit, bool activation)
	{
		float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
		if (unit >= outputSize) return sum;
		#pragma unroll 8
		for (uint32_t x = 0; x < inputSize; ++x)
		{
			const float w = weightsT[(size_t)x * outputSize + unit];
			const float4 f = from[x];
			sum.x += w * f.x; sum.y += w * f.y; sum.z += w * f.z; sum.w += w * f.w;
		}
		const float b = bias[unit];
		sum.x += b; sum.y += b; sum.z += b; sum.w += b;
		if (activation) { sum.x = tanhf(sum.x); sum.y = tanhf(sum.y); sum.z = tanhf(sum.z); sum.w = tanhf(sum.w); }
		return sum;
	}
	static_assert(POLICY_TILE == 4, "policyLayer carries the tile as one float4");

	// Rows first .. first + POLICY_TILE - 1 into LDS as [in][tile]; rows past count read as zeros.  Row i is row rowAt(i) of `states`
	// (the gradient step gathers through its permutation).  copy (may be null) receives the rows as they were read, row i at row i.
	// The caller's barrier follows.
	struct same_row { __device__ uint32_t operator()(uint32_t i) const { return i; } };
	template <class Map = same_row>
	__device__ __forceinline__ void loadTile(float4* input, const float* __restrict__ states, float* __restrict__ copy, uint32_t first, uint32_t count, Map rowAt = Map())
	{
		for (uint32_t i = threadIdx.x; i < POLICY_TILE * STATE_SIZE; i += blockDim.x)
		{
			const uint32_t r = i / STATE_SIZE, x = i % STATE_SIZE;
			const float v = first + r < count ? states[(size_t)STATE_SIZE * rowAt(first + r) + x] : 0.f;
			((float*)input)[POLICY_TILE * x + r] = v;
			if (copy && first + r < count) copy[(size_t)STATE_SIZE * (first + r) + x] = v;
		}
	}

	// One network over the tile in `input` (loaded, barrier passed): layer 1, its tanh vectors to hiddenA, barrier, layer 2, to hiddenB,
	// barrier, layer 3 on lanes 0 .. outputs - 1.  Lane t returns unit t's a = tanh(z1), b = tanh(z2) and out, one component per tile row
	// (zeros where it has no unit).  blockDim.x >= max(hidden, 64), a multiple of 64.
	struct forward_one { float4 a, b, out; };
	__device__ __forceinline__ forward_one forwardNetwork(const locomotion_policy& n, const float4* input, float4* hiddenA, float4* hiddenB)
	{
		const uint32_t t = threadIdx.x;
		forward_one f;
		f.a = policyLayer(n.w[0], n.b[0], STATE_SIZE, n.hidden, input, t, true);
		if (t < n.hidden) hiddenA[t] = f.a;
		__syncthreads();
		f.b = policyLayer(n.w[1], n.b[1], n.hidden, n.hidden, hiddenA, t, true);
		if (t < n.hidden) hiddenB[t] = f.b;
		__syncthreads();
		f.out = policyLayer(n.w[2], n.b[2], n.hidden, n.outputs, hiddenB, t, false);
		return f;
	}

	// Actor and critic over the same tile, layer by layer side by side, with the same three barriers.  The last layers run on different
	// waves where there are two: the actor's on lanes 0 .. 26, the critic's one unit on lane criticLane().  Afterwards hiddenA / hiddenB
	// hold the actor's tanh vectors and valueA / valueB the critic's.  blockDim.x >= max(p.hidden, v.hidden, 64), a multiple of 64.
	__device__ __forceinline__ uint32_t criticLane() { return blockDim.x > 64 ? 64 : 32; }
	struct forward_pair { float4 a, b, va, vb, out, value; };
	__device__ __forceinline__ forward_pair forwardActorCritic(const locomotion_policy& p, const locomotion_policy& v, const float4* input, float4* hiddenA, float4* hiddenB, float4* valueA, float4* valueB)
	{
		const uint32_t t = threadIdx.x;
		forward_pair f;
		f.a = policyLayer(p.w[0], p.b[0], STATE_SIZE, p.hidden, input, t, true);
		f.va = policyLayer(v.w[0], v.b[0], STATE_SIZE, v.hidden, input, t, true);
		if (t < p.hidden) hiddenA[t] = f.a;
		if (t < v.hidden) valueA[t] = f.va;
		__syncthreads();
		f.b = policyLayer(p.w[1], p.b[1], p.hidden, p.hidden, hiddenA, t, true);
		f.vb = policyLayer(v.w[1], v.b[1], v.hidden, v.hidden, valueA, t, true);
		if (t < p.hidden) hiddenB[t] = f.b;
		if (t < v.hidden) valueB[t] = f.vb;
		__syncthreads();
		f.out = policyLayer(p.w[2], p.b[2], p.hidden, p.outputs, hiddenB, t, false);
		f.value = policyLayer(v.w[2], v.b[2], v.hidden, v.outputs, valueB, t - criticLane(), false); // t < criticLane() wraps: no unit
		return f;
	}
}
