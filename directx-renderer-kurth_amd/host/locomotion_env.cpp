// locomotion_env.cpp — the reference's one application of the physics path, rebuilt over the C-ABI:
// the humanoid ragdoll (src/physics/ragdoll.cpp:10-158) and the reinforcement-learning environment that the reference exports from
// its Physics-Lib DLL (src/learning/learned_locomotion.cpp:395-489; state / action / reward: :73-357).  Built as libmi_locomotion.so
// with the SAME five exports, so learning/loco_env.py binds it by changing the library path:
//     int  getPhysicsStateSize();  int getPhysicsActionSize();
//     void getPhysicsRanges(float* stateMin, float* stateMax, float* actionMin, float* actionMax);
//     void resetPhysics(float* outState);
//     int  updatePhysics(float* action, float* outState, float* outReward);   // returns 1 when the ragdoll has fallen
// One addition: setPhysicsSeed(uint64) — the reference seeds its random pushes with time(0); here the seed is explicit (default
// fixed) so that runs are reproducible.  resetPhysics also fills outState (the reference leaves it untouched).
// The controller half (learned_locomotion::update, :44-68) is here too: setPhysicsPolicy keeps a network (locomotion_policy.h),
// inferPhysicsPolicy runs it on one state, updatePhysicsPolicy drives the single environment from it.
// For training (learning/learn_locomotion.py) the file keeps a critic in the same record (setPhysicsValueNetwork, inferPhysicsValue)
// and the Gaussian's scales (setPhysicsActionStd), and states the exploration noise on the host (samplePhysicsNoise); the batch
// collects with them.
// Everything physical happens in libmi_physics.so on the GPU; this file is host logic only, like the reference's.
//
// Build: directx_renderer_kurth_amd.build_locomotion() compiles this file with g++ and locomotion_batch.hip (the batched environments)
// with hipcc, and links both into ../libmi_locomotion.so against libmi_physics.so.
#include <cstdio>
#include <vector>

#include "locomotion_policy.h"

namespace
{
	struct environment
	{
		mi_world* world = nullptr;
		ragdoll doll;
		float lastSmoothedAction[ACTION_SIZE] = {};
		training train;
		float totalReward = 0.f;
		rng64 rng;
		// snapshot of the device state, refreshed after every step: transform_component (interpolated), velocities
		ragdoll_view view;

		void snapshot()
		{
			uint32_t n = mi_num_bodies(world);
			std::vector<float> t(7 * (size_t)n), v(6 * (size_t)n);
			mi_read_transforms(world, 0 /* transform_component: what the reference's getState reads */, t.data(), n);
			mi_read_velocities(world, v.data(), n);
			for (int i = 0; i < NUM_BODY_PARTS; ++i)
			{
				const float* p = &t[7 * (size_t)doll.body[i]]; const float* q = &v[6 * (size_t)doll.body[i]];
				view.transform[i] = { { p[3], p[4], p[5], p[6] }, { p[0], p[1], p[2] } };
				view.linearVelocity[i] = v3(q[0], q[1], q[2]); view.angularVelocity[i] = v3(q[3], q[4], q[5]);
			}
		}

		void applyAction(const float* action) // learned_locomotion.cpp:73-109
		{
			smoothAction(lastSmoothedAction, action);
			for (int i = 0; i < NUM_CONE_TWIST; ++i)
			{
				cone_twist_pod c; mi_constraint_get(world, MI_CONSTRAINT_CONE_TWIST, doll.coneTwist[i], &c);
				setConeTwistMotors(c, lastSmoothedAction, i);
				mi_constraint_set(world, MI_CONSTRAINT_CONE_TWIST, doll.coneTwist[i], &c);
			}
			for (int i = 0; i < NUM_HINGE; ++i)
			{
				hinge_pod c; mi_constraint_get(world, MI_CONSTRAINT_HINGE, doll.hinge[i], &c);
				setHingeMotors(c, lastSmoothedAction, i);
				mi_constraint_set(world, MI_CONSTRAINT_HINGE, doll.hinge[i], &c);
			}
		}
		void resetTraining() // training_locomotion::reset (:300-311) + learned_locomotion::reset (:36-44)
		{
			resetTargets(view, doll.boxMin, doll.boxMax, train);
			memset(lastSmoothedAction, 0, sizeof(lastSmoothedAction));
			float zero[ACTION_SIZE] = {};
			applyAction(zero);
		}
	};

	environment* env = nullptr;
	uint64_t seed = 0x9E3779B97F4A7C15ull;

	// A network as a setter left it: one block of networkFloats(hidden, outputs) floats, the six arrays back to back.
	struct stored_network
	{
		uint32_t outputs, hidden = 0; // hidden 0: none set
		std::vector<float> data;

		bool view(locomotion_policy* out) const { if (hidden) *out = networkOf(data.data(), hidden, outputs); return hidden != 0; }

		// A bad argument returns MI_ERR_INVALID_ARGUMENT and leaves the previous network active.
		int set(uint32_t h, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3)
		{
			if (!h || h > POLICY_MAX_HIDDEN || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return MI_ERR_INVALID_ARGUMENT;
			std::vector<float> packed(networkFloats(h, outputs));
			copyNetwork({ h, outputs, { w1, w2, w3 }, { b1, b2, b3 } }, networkOf(packed.data(), h, outputs), NETWORK_PLAIN);
			data.swap(packed);
			hidden = h;
			return locomotionBatchNetworkChanged(outputs);
		}

		// The network on one state, on the host.  ab (2 x hidden floats, may be NULL) receives tanh(z1), tanh(z2).
		int infer(const float* state, float* out, float* ab) const
		{
			locomotion_policy p;
			if (!view(&p)) return MI_ERR_INVALID_STATE;
			if (!state || !out) return MI_ERR_INVALID_ARGUMENT;
			float scratch[2 * POLICY_MAX_HIDDEN];
			inferNetwork(p, state, scratch, scratch + p.hidden, out);
			if (ab) memcpy(ab, scratch, sizeof(float) * 2 * p.hidden);
			return MI_OK;
		}
	};
	stored_network policy = { ACTION_SIZE }, critic = { 1 }; // setPhysicsPolicy's and setPhysicsValueNetwork's
	// The scales of setPhysicsActionStd.
	bool actionStdSet = false;
	float actionStd[2 * ACTION_SIZE] = {}; // std[27], logStd[27]

	// updatePhysics after its applyAction (:469-489): push draw, step, state, reward, fallen.
	int stepAfterAction(float* outState, float* outReward)
	{
		if (env->rng.f01() < 0.02f) // a random push every ~50 steps
		{
			uint32_t bodyPartIndex = env->rng.u32Between(0, NUM_BODY_PARTS - 1);
			vec3 part = env->view.transform[bodyPartIndex].position + v3(0.f, 0.2f, 0.f);
			float dx = env->rng.between(-1.f, 1.f), dz = env->rng.between(-1.f, 1.f);
			vec3 direction = normalize(v3(dx, 0.f, dz));
			vec3 origin = part - direction * 5.f;
			mi_test_physics_interaction(env->world, &origin.x, &direction.x, 1000.f);
		}
		mi_physics_settings s = { 1, 60, 4, 30, 0, 1, 0, 1, 1, 1 };
		float timer = 0.f;
		mi_step(env->world, &timer, &s, 1.f / 60.f);
		env->snapshot();
		getState(env->view, env->train, env->lastSmoothedAction, outState);
		bool failure = hasFallen(outState);
		*outReward = 0.f;
		if (!failure) { *outReward = getReward(env->view, env->train); env->totalReward += *outReward; }
		return failure ? 1 : 0;
	}
}

uint64_t locomotionSeed() { return seed; }

bool locomotionNetwork(uint32_t outputs, locomotion_policy* out) { return (outputs == 1 ? critic : policy).view(out); }

const float* locomotionActionStd() { return actionStdSet ? actionStd : nullptr; }

extern "C"
{
	int getPhysicsStateSize() { return STATE_SIZE; }   // learned_locomotion.cpp:401
	int getPhysicsActionSize() { return ACTION_SIZE; } // :402

	void setPhysicsSeed(unsigned long long s) { seed = s ? s : 0x9E3779B97F4A7C15ull; if (env) env->rng.state = seed; }

	void getPhysicsRanges(float* stateMin, float* stateMax, float* actionMin, float* actionMax) // :404-433
	{
		for (int i = 0; i < STATE_SIZE; ++i) { stateMin[i] = -FLT_MAX; stateMax[i] = FLT_MAX; }
		mi_world_desc d = { -1, 0, 0, 0 };
		mi_world* w = mi_world_create(&d);
		if (!w) { fprintf(stderr, "getPhysicsRanges: %s\n", mi_last_error(nullptr)); return; }
		ragdoll r = createRagdoll(w, v3(0.f, 0.f, 0.f), 0.f);
		fillRanges(w, r, actionMin, actionMax);
		mi_world_destroy(w);
	}

	void resetPhysics(float* outState) // :435-461
	{
		if (!env) { env = new environment; env->rng.state = seed; }
		if (env->world) mi_world_destroy(env->world);
		mi_world_desc d = { -1, 0, 0, 0 };
		env->world = mi_world_create(&d);
		if (!env->world) { fprintf(stderr, "resetPhysics: %s\n", mi_last_error(nullptr)); return; }
		env->totalReward = 0.f;
		addGround(env->world, 20.f);
		env->doll = createRagdoll(env->world, v3(0.f, 1.25f, 0.f), 0.f);
		std::vector<float> mp(13 * (size_t)mi_num_bodies(env->world));
		mi_read_mass_properties(env->world, mp.data(), mi_num_bodies(env->world));
		for (int i = 0; i < NUM_BODY_PARTS; ++i) { const float* m = &mp[13 * (size_t)env->doll.body[i]]; env->train.localCOG[i] = v3(m[0], m[1], m[2]); }
		env->snapshot();
		env->resetTraining();
		if (outState) getState(env->view, env->train, env->lastSmoothedAction, outState);
	}

	int updatePhysics(float* action, float* outState, float* outReward) // :463-489
	{
		if (!env || !env->world) { if (outReward) *outReward = 0.f; return 1; }
		env->applyAction(action);
		return stepAfterAction(outState, outReward);
	}

	// Replaces the policy (layout: locomotion_policy.h).  Kept for the single environment and uploaded to the batch, if one exists; may
	// be called before or after either reset.  A bad argument returns MI_ERR_INVALID_ARGUMENT and leaves the previous policy active.
	int setPhysicsPolicy(uint32_t hidden, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3)
	{
		return policy.set(hidden, w1, b1, w2, b2, w3, b3);
	}

	// The network on one state, on the host: needs no world and no GPU.  hidden (2 x H floats, may be NULL) receives tanh(z1), tanh(z2).
	int inferPhysicsPolicy(const float* state, float* action, float* hidden)
	{
		return policy.infer(state, action, hidden);
	}

	// learned_locomotion::update (:44-68) on the single environment: its state as it is -> network -> applyAction, then the rest of
	// updatePhysics.  Returns what updatePhysics returns, or -MI_ERR_INVALID_STATE without a policy.
	int updatePhysicsPolicy(float* outState, float* outReward)
	{
		locomotion_policy p;
		if (!policy.view(&p)) return -MI_ERR_INVALID_STATE;
		if (!env || !env->world) { if (outReward) *outReward = 0.f; return 1; }
		float state[STATE_SIZE], action[ACTION_SIZE], ab[2 * POLICY_MAX_HIDDEN];
		getState(env->view, env->train, env->lastSmoothedAction, state);
		inferNetwork(p, state, ab, ab + p.hidden, action);
		env->applyAction(action);
		return stepAfterAction(outState, outReward);
	}

	// The critic of training, 66 -> Hv -> Hv -> 1 with tanh on the hidden layers: w1 [Hv][66], b1, w2 [Hv][Hv], b2, w3 [1][Hv], b3 [1].
	// Independent of the policy's H; kept and uploaded like the policy.  A bad argument leaves the previous one active.
	int setPhysicsValueNetwork(uint32_t hidden, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3)
	{
		return critic.set(hidden, w1, b1, w2, b2, w3, b3);
	}

	// The critic on one state, on the host.  hidden (2 x Hv floats, may be NULL) receives tanh(z1), tanh(z2).
	int inferPhysicsValue(const float* state, float* outValue, float* hidden)
	{
		return critic.infer(state, outValue, hidden);
	}

	// The scale of the Gaussian around the policy's output, per action, and its logarithm: both given, so that the library evaluates
	// neither exp nor log of them.  Zeros are legal (the sample is then the mean).
	int setPhysicsActionStd(const float* std, const float* logStd)
	{
		if (!std || !logStd) return MI_ERR_INVALID_ARGUMENT;
		memcpy(actionStd, std, sizeof(float) * ACTION_SIZE); memcpy(actionStd + ACTION_SIZE, logStd, sizeof(float) * ACTION_SIZE);
		actionStdSet = true;
		return locomotionBatchStdChanged();
	}

	// The exploration noise of environment env at update counter `update` under `seed` (locomotion_policy.h: noiseSample), on the host:
	// out[27].  samplePhysicsNoiseUniforms gives the two uniforms behind every sample, which are exact: the integer stage made visible.
	int samplePhysicsNoise(unsigned long long seed, uint32_t env, unsigned long long update, float* out)
	{
		if (!out) return MI_ERR_INVALID_ARGUMENT;
		for (uint32_t j = 0; j < ACTION_SIZE; ++j) out[j] = noiseSample(seed, env, update, j);
		return MI_OK;
	}
	int samplePhysicsNoiseUniforms(unsigned long long seed, uint32_t env, unsigned long long update, float* outU1, float* outU2)
	{
		if (!outU1 || !outU2) return MI_ERR_INVALID_ARGUMENT;
		for (uint32_t j = 0; j < ACTION_SIZE; ++j) noiseUniforms(seed, env, update, j, outU1 + j, outU2 + j);
		return MI_OK;
	}
}
