// locomotion_policy.h — the learned controller's network (learned_locomotion.cpp:11-27, 44-68): a 66 -> H -> H -> 27 MLP, tanh after
// the two hidden layers, none after the last.  A policy is six fp32 arrays in the layout of the reference's generated network.h,
// which is torch's named_parameters order (learning/convert_model_to_c++.py:8-46):
//     W1[H][66], b1[H], W2[H][H], b2[H], W3[27][H], b3[27]      row-major [out][in], one hidden size for both layers
// The reference fixes HIDDEN_LAYER_SIZE at 128; any 1 <= H <= POLICY_MAX_HIDDEN is accepted.  Shared like locomotion_shared.h: the
// single environment (g++) runs inferPolicy on the host, the batched one (hipcc) restates the same sums in k_loco_policy.
// Also here, shared the same way: the critic of training, the exploration noise and the log-probability of a sampled action.
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

	// The critic of training (learning/learn_locomotion.py:71-107, vf=[128,128]): 66 -> Hv -> Hv -> 1, tanh after the two hidden layers,
	// carried in a locomotion_policy whose w3 is [1][Hv] and whose b3 is one float.
	LOCO_HD size_t valueFloats(uint32_t h) { return (size_t)h * STATE_SIZE + h + (size_t)h * h + h + h + 1; }
	LOCO_HD void inferValue(const locomotion_policy& p, const float* state, float* a, float* b, float* value)
	{
		applyLayer(p.w1, p.b1, STATE_SIZE, p.hidden, state, a, true);
		applyLayer(p.w2, p.b2, p.hidden, p.hidden, a, b, true);
		applyLayer(p.w3, p.b3, p.hidden, 1, b, value, false);
	}

	// The exploration noise of the sampled actions: a stateless function of (seed, environment, update counter, action index), so it
	// depends neither on the number of environments nor on any stored random state (the push draws of rng64 are left alone).
	// Integer stage, all in uint64 with wrap-around (splitmix64's finaliser, three times):
	//     mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
	//     h = mix(seed + 0x9E3779B97F4A7C15 * (env + 1));  h = mix(h ^ update);  h = mix(h + 0x9E3779B97F4A7C15 * (j + 1))
	//     k1 = h >> 40            (the top 24 bits)            u1 = (k1 + 1) * 2^-24  in (0, 1]
	//     k2 = (h >> 16) & 0xFFFFFF (the next 24 bits)          u2 = k2 * 2^-24        in [0, 1)
	// both uniforms exact in float32.  Then Box-Muller in float32, one normal per action index:
	//     eps = sqrtf(-2 * logf(u1)) * cosf(float32(2 pi) * u2)
	// each operation rounded to float32; logf, cosf and sqrtf are those of the compiling side (glibc on the host, OCML on the device).
	LOCO_HD uint64_t noiseMix(uint64_t z) { z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31; return z; }
	LOCO_HD void noiseUniforms(uint64_t seed, uint32_t env, uint64_t update, uint32_t j, float* u1, float* u2)
	{
		uint64_t h = noiseMix(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)env + 1));
		h = noiseMix(h ^ update);
		h = noiseMix(h + 0x9E3779B97F4A7C15ull * ((uint64_t)j + 1));
		*u1 = (float)((uint32_t)(h >> 40) + 1u) * 5.9604644775390625e-8f;
		*u2 = (float)((uint32_t)(h >> 16) & 0xFFFFFFu) * 5.9604644775390625e-8f;
	}
	LOCO_HD float noiseSample(uint64_t seed, uint32_t env, uint64_t update, uint32_t j)
	{
		float u1, u2;
		noiseUniforms(seed, env, update, j, &u1, &u2);
		const float l = logf(u1);
		const float r = sqrtf(-2.f * l);
		const float angle = 6.283185307179586f * u2;
		return r * cosf(angle);
	}

	// log N(a; mu, std) of one sampled action from its noise: sum_j(-eps_j^2 / 2 - logStd_j) - 13.5 log(2 pi), the terms added in
	// ascending j in float32, then the constant (the float32 nearest to the float64 value) subtracted.
	LOCO_HD float noiseLogProb(const float* eps, const float* logStd)
	{
		float sum = 0.f;
		for (int j = 0; j < ACTION_SIZE; ++j) { const float square = eps[j] * eps[j]; const float half = -0.5f * square; sum += half - logStd[j]; }
		return sum - 24.811340396526162f;
	}
}

// The policy of setPhysicsPolicy (locomotion_env.cpp), for the batched environments: false while none is set.
__attribute__((visibility("hidden"))) bool locomotionPolicy(locomotion_policy* out);
// Uploads the current policy to the batch, if there is one (locomotion_batch.hip); called by setPhysicsPolicy.
__attribute__((visibility("hidden"))) int locomotionBatchPolicyChanged();
// The critic of setPhysicsValueNetwork and the scales of setPhysicsActionStd (std[27], then logStd[27]): false / null while none is set.
__attribute__((visibility("hidden"))) bool locomotionValueNetwork(locomotion_policy* out);
__attribute__((visibility("hidden"))) const float* locomotionActionStd();
// Upload them to the batch, if there is one; called by the two setters.
__attribute__((visibility("hidden"))) int locomotionBatchValueChanged();
__attribute__((visibility("hidden"))) int locomotionBatchStdChanged();
