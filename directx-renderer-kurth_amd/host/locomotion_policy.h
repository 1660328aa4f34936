// locomotion_policy.h — the learned controller's networks (learned_locomotion.cpp:11-27, 44-68): the policy, a 66 -> H -> H -> 27 MLP,
// tanh after the two hidden layers, none after the last, and the critic of training (learning/learn_locomotion.py:71-107,
// vf=[128,128]), 66 -> Hv -> Hv -> 1 of the same form.  A network is six fp32 arrays in the layout of the reference's generated
// network.h, which is torch's named_parameters order (learning/convert_model_to_c++.py:8-46):
//     W1[H][66], b1[H], W2[H][H], b2[H], W3[outputs][H], b3[outputs]      row-major [out][in], one hidden size for both layers
// The reference fixes HIDDEN_LAYER_SIZE at 128; any 1 <= H <= POLICY_MAX_HIDDEN is accepted.  Shared like locomotion_shared.h: the
// single environment (g++) runs inferNetwork on the host; the batched one (hipcc) keeps the same six arrays with every weight matrix
// transposed to [in][out] and runs the same sums in locomotion_layers.h.  walkNetwork is the one statement of how the six arrays lie in
// a block; sizes, pointer views, packing and both transpositions come from it.
// Also here, shared the same way: the exploration noise and the log-probability of a sampled action.
#pragma once
#include "locomotion_shared.h"

// Layer l of a network: weights w[l], bias b[l].  outputs is 27 (the policy) or 1 (the critic).
template <class T> struct network_view { uint32_t hidden, outputs; T* w[3]; T* b[3]; };
typedef network_view<const float> locomotion_policy;

namespace
{
	enum { POLICY_MAX_HIDDEN = 256 };

	// The layout: layer l is inputs x units weights (in either orientation), then units biases; the three layers lie back to back.
	// each(l, inputs, units, weightsAt, biasAt), the two offsets in floats from the start.  Returns the floats of the whole network.
	template <class F> LOCO_HD size_t walkNetwork(uint32_t hidden, uint32_t outputs, F each)
	{
		size_t at = 0;
		for (int l = 0; l < 3; ++l)
		{
			const uint32_t inputs = l ? hidden : STATE_SIZE, units = l < 2 ? hidden : outputs;
			each(l, inputs, units, at, at + (size_t)inputs * units);
			at += (size_t)inputs * units + units;
		}
		return at;
	}

	LOCO_HD size_t networkFloats(uint32_t hidden, uint32_t outputs) { return walkNetwork(hidden, outputs, [](int, uint32_t, uint32_t, size_t, size_t) {}); }
	LOCO_HD size_t policyFloats(uint32_t h) { return networkFloats(h, ACTION_SIZE); }
	LOCO_HD size_t valueFloats(uint32_t h) { return networkFloats(h, 1); }

	// The six arrays of a network that lies in one block at p.
	template <class T> LOCO_HD network_view<T> networkOf(T* p, uint32_t hidden, uint32_t outputs)
	{
		network_view<T> n = { hidden, outputs, {}, {} };
		walkNetwork(hidden, outputs, [&](int l, uint32_t, uint32_t, size_t weightsAt, size_t biasAt) { n.w[l] = p + weightsAt; n.b[l] = p + biasAt; });
		return n;
	}

	// Copies a network array by array.  NETWORK_PLAIN: as it is (packing the setters' six pointers into a block).  NETWORK_TO_DEVICE:
	// `from` is [out][in] and `to` becomes [in][out], the upload.  NETWORK_TO_HOST: the way back, for readPhysicsBatch*.
	enum network_copy { NETWORK_PLAIN, NETWORK_TO_DEVICE, NETWORK_TO_HOST };
	inline void copyNetwork(const locomotion_policy& from, const network_view<float>& to, network_copy how)
	{
		walkNetwork(from.hidden, from.outputs, [&](int l, uint32_t inputs, uint32_t units, size_t, size_t)
		{
			if (how == NETWORK_PLAIN) memcpy(to.w[l], from.w[l], sizeof(float) * inputs * units);
			else for (uint32_t x = 0; x < inputs; ++x) for (uint32_t y = 0; y < units; ++y)
			{
				const size_t host = (size_t)y * inputs + x, device = (size_t)x * units + y;
				if (how == NETWORK_TO_DEVICE) to.w[l][device] = from.w[l][host]; else to.w[l][host] = from.w[l][device];
			}
			memcpy(to.b[l], from.b[l], sizeof(float) * units);
		});
	}

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

	// learned_locomotion::update (:52-64) up to applyAction, for either network in the [out][in] layout: state -> a -> b -> out; a and b
	// hold `hidden` floats each, out `outputs`.
	LOCO_HD void inferNetwork(const locomotion_policy& n, const float* state, float* a, float* b, float* out)
	{
		applyLayer(n.w[0], n.b[0], STATE_SIZE, n.hidden, state, a, true);
		applyLayer(n.w[1], n.b[1], n.hidden, n.hidden, a, b, true);
		applyLayer(n.w[2], n.b[2], n.hidden, n.outputs, b, out, false);
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

// The network of setPhysicsPolicy (outputs = 27) or setPhysicsValueNetwork (outputs = 1) as locomotion_env.cpp keeps it, for the
// batched environments: false while none is set.
__attribute__((visibility("hidden"))) bool locomotionNetwork(uint32_t outputs, locomotion_policy* out);
// The scales of setPhysicsActionStd (std[27], then logStd[27]): null while none is set.
__attribute__((visibility("hidden"))) const float* locomotionActionStd();
// Upload them to the batch, if there is one (locomotion_batch.hip); called by the three setters.
__attribute__((visibility("hidden"))) int locomotionBatchNetworkChanged(uint32_t outputs);
__attribute__((visibility("hidden"))) int locomotionBatchStdChanged();
