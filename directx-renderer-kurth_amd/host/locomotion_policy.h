// locomotion_policy.h — the learned controller's network (learned_locomotion.cpp:11-27, 44-68): a 66 -> H -> H -> 27 MLP, tanh after
// the two hidden layers, none after the last.  A policy is six fp32 arrays in the layout of the reference's generated network.h,
// which is torch's named_parameters order (learning/convert_model_to_c++.py:8-46):
//     W1[H][66], b1[H], W2[H][H], b2[H], W3[27][H], b3[27]      row-major [out][in], one hidden size for both layers
// The reference fixes HIDDEN_LAYER_SIZE at 128; any 1 <= H <= POLICY_MAX_HIDDEN is accepted.  Shared like locomotion_shared.h: the
// single environment (g++) runs inferPolicy on the host, the batched one (hipcc) restates the same sums in k_loco_policy.
#pragma once
#include "locomotion_shared.h"

struct locomotion_policy { uint32_t hidden; const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3; };

namespace
{
	enum { POLICY_MAX_HIDDEN = 256 };

	LOCO_HD size_t policyFloats(uint32_t h) { return (size_t)h * STATE_SIZE + h + (size_t)h * h + h + (size_t)ACTION_SIZE * h + ACTION_SIZE; }

	// applyLayer (:11-26): per output the products are added in ascending input order, each product rounded before it is added (both
	// compilers run with -ffp-contract=off), then the bias, then tanh.
	LOCO_HD void applyLayer(const float* weights, const float* bias, uint32_t inputSize, uint32_t outputSize, const float* from, float* to, bool activation)
	{
		for (uint32_t y = 0; y < outputSize; ++y)
		{
			const float* row = weights + (size_t)y * inputSize;
			float sum = 0.f;
			for (uint32_t x = 0; x < inputSize; ++x) sum += row[x] * from[x];
			sum += bias[y];
			to[y] = activation ? tanhf(sum) : sum;
		}
	}

	// learned_locomotion::update (:52-64) up to applyAction: state -> a -> b -> action; a and b hold `hidden` floats each.
	LOCO_HD void inferPolicy(const locomotion_policy& p, const float* state, float* a, float* b, float* action)
	{
		applyLayer(p.w1, p.b1, STATE_SIZE, p.hidden, state, a, true);
		applyLayer(p.w2, p.b2, p.hidden, p.hidden, a, b, true);
		applyLayer(p.w3, p.b3, p.hidden, ACTION_SIZE, b, action, false);
	}
}

// The policy of setPhysicsPolicy (locomotion_env.cpp), for the batched environments: false while none is set.
__attribute__((visibility("hidden"))) bool locomotionPolicy(locomotion_policy* out);
// Uploads the current policy to the batch, if there is one (locomotion_batch.hip); called by setPhysicsPolicy.
__attribute__((visibility("hidden"))) int locomotionBatchPolicyChanged();
