// locomotion_layers.h — the device-side layer arithmetic of the learned controller, shared by the kernels that run the networks:
// inference and collection (locomotion_batch.hip) and the PPO gradient step (locomotion_update.hip).  One statement of the sums, so
// that the log-probabilities the update recomputes are those of the networks the rollout ran.
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

	// A network in the device layout: W1T [66][H], b1 [H], W2T [H][H], b2 [H], W3T [H][outputs], b3 [outputs], back to back.
	struct network { const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3; };
	__device__ network networkOf(const float* __restrict__ p, uint32_t hidden, uint32_t outputs)
	{
		network n;
		n.w1 = p; n.b1 = n.w1 + (size_t)STATE_SIZE * hidden;
		n.w2 = n.b1 + hidden; n.b2 = n.w2 + (size_t)hidden * hidden;
		n.w3 = n.b2 + hidden; n.b3 = n.w3 + (size_t)hidden * outputs;
		return n;
	}
}
