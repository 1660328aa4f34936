// locomotion_batch.hip — N ragdoll environments of locomotion_env.cpp in ONE world, driven on the device: the motor targets go
// straight into the joint PODs (mi_joint_device_pods), the random pushes are one batched ray test (mi_test_physics_interaction_batch),
// and state, reward and fallen come out of one gather kernel.  Per update: one copy in, four kernels + mi_step, one copy out;
// no per-joint host call, no host ray test, no full-state copy.
//
// Environment e owns bodies 14e .. 14e+13 (its ragdoll, hips at (x_e, 1.25, z_e) on a square grid of pitch 8 m) over one ground box.
// Each environment restates the single one: the same builder, the same smoothing and motors, the same push draws from its own
// xorshift64 (seed ^ e * 0x9E3779B97F4A7C15; env 0 draws what the single environment draws), the same step settings, the same
// state and reward formulas (locomotion_shared.h), read from the interpolated pose as the single environment reads it.
//
// The controller (learned_locomotion::update, locomotion_policy.h) closes the loop on the device: k_loco_policy<27, true> reads the
// current states, runs the network (locomotion_layers.h), smooths and writes the motors, in place of k_loco_actions, so an update driven
// by the policy has the same launches as one driven by given actions.  The same kernel without the motors is the inference of either
// network: k_loco_policy<27, false> the policy's, k_loco_policy<1, false> the critic's.  dStates always holds the state of every environment as it is now (what
// observePhysicsBatch returns): every entry point that moves the environments refreshes it.  rolloutPhysicsBatchDevice enqueues
// whole trajectories, with the fallen environments reset from their flags on the device.
//
// Training data (learning/learn_locomotion.py:71-107, PPO) is collected the same way: collectPhysicsBatchDevice runs the rollout's
// updates with k_loco_sample in place of k_loco_policy<27, true>, which adds the critic, the exploration noise (locomotion_policy.h:
// noiseSample), the sampled action, its log-probability and the clamp to the action ranges in the same launch.  The advantages of
// gaePhysicsBatchDevice come from one lane per environment walking the rows backwards.
//
// The gradient step on that data is locomotion_update.hip's; its entry points are here (beginPhysicsBatchTraining ..
// readPhysicsBatchLogStd).  policy.data, critic.data and dScales are the master copy of the parameters while a training session is open: Adam
// writes them in place, and the kernels above read what it wrote.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#include "locomotion_layers.h"
#include "locomotion_update.h"

namespace
{
	constexpr uint32_t NUM_MOTOR_JOINTS = NUM_CONE_TWIST + NUM_HINGE;
	constexpr float GRID_PITCH = 8.f;

	// Per environment, fixed at resetPhysicsBatch: the spawn pose of every part (pose layout of the world: {pos, 0}, {quat}) and the
	// training targets of resetTraining.
	struct env_init { float4 spawn[2 * NUM_BODY_PARTS]; training train; };

	// A network on the device: locomotion_policy.h's six arrays, the weights transposed to [in][out], in one block.
	struct device_network { uint32_t outputs; float* data = nullptr; uint32_t hidden = 0; }; // hidden 0: none uploaded

	struct batch
	{
		mi_world* world = nullptr;
		hipStream_t stream = nullptr;
		uint32_t n = 0;
		struct mi_device_state ds = {};
		std::vector<ragdoll> dolls;
		// device
		env_init* dInit = nullptr;
		float* dSmoothed = nullptr;   // n x 27: lastSmoothedAction
		uint64_t* dRng = nullptr;     // n: xorshift64 states
		float* dRays = nullptr;       // n x 8: the push rays of the last update
		int32_t* dPushes = nullptr;   // n: 1 + pushed body, or 0
		uint32_t* dSlots = nullptr;   // n x 13: POD slot of each env's 7 cone-twist, then 6 hinge joints
		float* dActions = nullptr; float* dStates = nullptr; float* dRewards = nullptr; int32_t* dFallen = nullptr; uint32_t* dIds = nullptr;
		device_network policy = { ACTION_SIZE }, critic = { 1 };
		float* dScales = nullptr;     // 4 x 27: std, logStd, actionMin, actionMax
		bool stdSet = false, rangesSet = false;
		uint64_t noiseCounter = 0;    // collecting updates since resetPhysicsBatch
		void* pods[2] = { nullptr, nullptr }; // cone-twist, hinge
		// the training session of beginPhysicsBatchTraining: Adam's m, then v, in the flat parameter order of locomotion_update.h
		bool training = false;
		float lr = 0.f, beta1 = 0.f, beta2 = 0.f, adamEps = 0.f;
		uint64_t adamStep = 0;
		float* dMoments = nullptr;
		// scratch of the gradient step, grown on demand: the slab, the gradient, the blocks' sums of squares, the groups' statistics
		float* dSlab = nullptr; float* dGradient = nullptr; float* dPartial = nullptr; float* dGroupStats = nullptr;
		size_t slabFloats = 0, gradientFloats = 0;
		uint32_t generation[2] = { ~0u, ~0u };
	};
	batch* B = nullptr;

	bool ok(hipError_t e, const char* what) { if (e != hipSuccess) { fprintf(stderr, "locomotion batch: %s: %s\n", what, hipGetErrorString(e)); return false; } return true; }

	void release(batch* b)
	{
		if (!b) return;
		if (b->stream) (void)hipStreamSynchronize(b->stream);
		void* bufs[] = { b->dInit, b->dSmoothed, b->dRng, b->dRays, b->dPushes, b->dSlots, b->dActions, b->dStates, b->dRewards, b->dFallen, b->dIds, b->policy.data, b->critic.data, b->dScales, b->dMoments, b->dSlab, b->dGradient, b->dPartial, b->dGroupStats };
		for (void* p : bufs) if (p) (void)hipFree(p);
		if (b->world) mi_world_destroy(b->world);
		delete b;
	}

	__device__ void loadView(ragdoll_view& v, const float4* __restrict__ poseLerp, const float4* __restrict__ vel, uint32_t firstBody)
	{
		for (int i = 0; i < NUM_BODY_PARTS; ++i)
		{
			const float4 p = poseLerp[2 * (firstBody + i)], q = poseLerp[2 * (firstBody + i) + 1], l = vel[2 * (firstBody + i)], a = vel[2 * (firstBody + i) + 1];
			v.transform[i] = { { q.x, q.y, q.z, q.w }, { p.x, p.y, p.z } };
			v.linearVelocity[i] = v3(l.x, l.y, l.z); v.angularVelocity[i] = v3(a.x, a.y, a.z);
		}
	}

	// The motor targets of joint j of environment e (cone-twist joints first, then the hinges) from its smoothed action, into its POD.
	__device__ void writeMotor(uint32_t e, uint32_t j, const float* smoothed, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		const size_t slot = slots[NUM_MOTOR_JOINTS * e + j];
		if (j < NUM_CONE_TWIST) setConeTwistMotors(*(cone_twist_pod*)(conePods + slot * sizeof(cone_twist_pod)), smoothed, j);
		else setHingeMotors(*(hinge_pod*)(hingePods + slot * sizeof(hinge_pod)), smoothed, j - NUM_CONE_TWIST);
	}

	__device__ void writeMotors(uint32_t e, const float* smoothed, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		for (uint32_t j = 0; j < NUM_MOTOR_JOINTS; ++j) writeMotor(e, j, smoothed, slots, conePods, hingePods);
	}

	// Kernel A: applyAction for every environment.
	__global__ void __launch_bounds__(64) k_loco_actions(uint32_t n, const float* __restrict__ actions, float* __restrict__ smoothedAll, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
		if (e >= n) return;
		float smoothed[ACTION_SIZE];
		for (int i = 0; i < ACTION_SIZE; ++i) smoothed[i] = smoothedAll[ACTION_SIZE * e + i];
		smoothAction(smoothed, actions + (size_t)ACTION_SIZE * e);
		for (int i = 0; i < ACTION_SIZE; ++i) smoothedAll[ACTION_SIZE * e + i] = smoothed[i];
		writeMotors(e, smoothed, slots, conePods, hingePods);
	}

	// applyAction for a tile, by one wave: smoothAction of `applied` (this lane's action element of every tile row, lanes 0 .. 26), one
	// element per lane, through `smoothed` in LDS; barrier; then one joint per lane writes its POD.
	__device__ __forceinline__ void smoothAndDrive(const float (&applied)[POLICY_TILE], float (*smoothed)[ACTION_SIZE], uint32_t first, uint32_t count,
		float* __restrict__ smoothedAll, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		const uint32_t t = threadIdx.x;
		if (t < ACTION_SIZE)
		{
			#pragma unroll
			for (uint32_t r = 0; r < POLICY_TILE; ++r)
			{
				const uint32_t e = first + r;
				if (e >= count) continue;
				const float s = lerpf(smoothedAll[(size_t)ACTION_SIZE * e + t], applied[r], 0.1f);
				smoothedAll[(size_t)ACTION_SIZE * e + t] = s; smoothed[r][t] = s;
			}
		}
		__syncthreads();
		const uint32_t r = t / NUM_MOTOR_JOINTS, j = t % NUM_MOTOR_JOINTS, e = first + r;
		if (r < POLICY_TILE && e < count) writeMotor(e, j, smoothed[r], slots, conePods, hingePods);
	}
	static_assert(POLICY_TILE * NUM_MOTOR_JOINTS <= 64 && ACTION_SIZE <= 64, "one wave covers the tile's joints and actions");
	static_assert(POLICY_TILE * NUM_MOTOR_JOINTS + POLICY_TILE <= 64, "one wave covers the tile's joints and log-probabilities");

	// Kernel P: one network, 66 -> hidden -> hidden -> OUTPUTS, on a tile of POLICY_TILE rows per workgroup.  <27, true> is
	// learned_locomotion::update: the policy on the environments' states, then smoothAction and the motor PODs, i.e. everything
	// k_loco_actions does.  <27, false> and <1, false> are the policy and the critic alone on any rows.  blockDim.x >= max(hidden, 64), a
	// multiple of 64.  out (count x OUTPUTS, raw network outputs) and hiddenOut (count x 2 hidden: tanh(z1), tanh(z2)) may be null.
	template <uint32_t OUTPUTS, bool APPLY>
	__global__ void __launch_bounds__(POLICY_MAX_HIDDEN) k_loco_policy(uint32_t count, uint32_t hidden, const float* __restrict__ states, const float* __restrict__ net,
		float* __restrict__ out, float* __restrict__ hiddenOut, float* __restrict__ smoothedAll, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		static_assert(!APPLY || OUTPUTS == ACTION_SIZE, "only the policy drives the motors");
		__shared__ float4 input[STATE_SIZE], hiddenA[POLICY_MAX_HIDDEN], hiddenB[POLICY_MAX_HIDDEN];
		__shared__ float smoothed[POLICY_TILE][ACTION_SIZE];
		const uint32_t first = blockIdx.x * POLICY_TILE, t = threadIdx.x;
		loadTile(input, states, nullptr, first, count);
		__syncthreads();
		const forward_one f = forwardNetwork(networkOf(net, hidden, OUTPUTS), input, hiddenA, hiddenB);
		const float av[POLICY_TILE] = { f.a.x, f.a.y, f.a.z, f.a.w }, bv[POLICY_TILE] = { f.b.x, f.b.y, f.b.z, f.b.w }, ov[POLICY_TILE] = { f.out.x, f.out.y, f.out.z, f.out.w };
		#pragma unroll
		for (uint32_t r = 0; r < POLICY_TILE; ++r)
		{
			const uint32_t e = first + r;
			if (e >= count) continue;
			if (hiddenOut && t < hidden) { hiddenOut[(size_t)2 * hidden * e + t] = av[r]; hiddenOut[(size_t)2 * hidden * e + hidden + t] = bv[r]; }
			if (out && t < OUTPUTS) out[(size_t)OUTPUTS * e + t] = ov[r];
		}
		if (APPLY) smoothAndDrive(ov, smoothed, first, count, smoothedAll, slots, conePods, hingePods);
	}

	// Kernel S: the collecting update of a tile of POLICY_TILE environments, everything before the push in one launch: the actor and
	// the critic on the current states (forwardActorCritic), the noise, the sample a = mu + std * eps, its log-probability, the clamp to
	// the action ranges (clip != 0), smoothAction and the motor PODs.  blockDim.x >= max(hidden, valueHidden, 64), a multiple of 64.
	// Row outputs: obs (the states as read), actions (unclipped), eps (may be null), logProbs, values.
	__global__ void __launch_bounds__(POLICY_MAX_HIDDEN) k_loco_sample(uint32_t count, uint32_t hidden, uint32_t valueHidden, int clip, uint64_t seed, uint64_t update,
		const float* __restrict__ states, const float* __restrict__ policy, const float* __restrict__ valueNet, const float* __restrict__ scales,
		float* __restrict__ obsOut, float* __restrict__ actionsOut, float* __restrict__ epsOut, float* __restrict__ logProbsOut, float* __restrict__ valuesOut,
		float* __restrict__ smoothedAll, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		__shared__ float4 input[STATE_SIZE], hiddenA[POLICY_MAX_HIDDEN], hiddenB[POLICY_MAX_HIDDEN], valueA[POLICY_MAX_HIDDEN], valueB[POLICY_MAX_HIDDEN];
		__shared__ float smoothed[POLICY_TILE][ACTION_SIZE], eps[POLICY_TILE][ACTION_SIZE];
		const uint32_t first = blockIdx.x * POLICY_TILE, t = threadIdx.x;
		loadTile(input, states, obsOut, first, count);
		for (uint32_t i = t; i < POLICY_TILE * ACTION_SIZE; i += blockDim.x)
		{
			const uint32_t r = i / ACTION_SIZE, j = i % ACTION_SIZE;
			eps[r][j] = first + r < count ? noiseSample(seed, first + r, update, j) : 0.f;
		}
		__syncthreads();
		const forward_pair f = forwardActorCritic(networkOf(policy, hidden, ACTION_SIZE), networkOf(valueNet, valueHidden, 1), input, hiddenA, hiddenB, valueA, valueB);
		const float ov[POLICY_TILE] = { f.out.x, f.out.y, f.out.z, f.out.w }, vv[POLICY_TILE] = { f.value.x, f.value.y, f.value.z, f.value.w };
		float applied[POLICY_TILE] = {};
		#pragma unroll
		for (uint32_t r = 0; r < POLICY_TILE; ++r)
		{
			const uint32_t e = first + r;
			if (e >= count) continue;
			if (t == criticLane()) valuesOut[e] = vv[r];
			if (t < ACTION_SIZE)
			{
				const float noise = eps[r][t];
				const float scaled = scales[t] * noise;
				const float sample = ov[r] + scaled;
				actionsOut[(size_t)ACTION_SIZE * e + t] = sample;
				if (epsOut) epsOut[(size_t)ACTION_SIZE * e + t] = noise;
				applied[r] = clip ? clampf(sample, scales[2 * ACTION_SIZE + t], scales[3 * ACTION_SIZE + t]) : sample;
			}
		}
		smoothAndDrive(applied, smoothed, first, count, smoothedAll, slots, conePods, hingePods);
		const uint32_t q = t - POLICY_TILE * NUM_MOTOR_JOINTS; // the log-probabilities on the lanes after the joints'
		if (q < POLICY_TILE && first + q < count) logProbsOut[first + q] = noiseLogProb(eps[q], scales + ACTION_SIZE);
	}

	// Generalised advantage estimation, one lane per environment walking its column of [steps][n] backwards (the lanes run along n:
	// every load is one coalesced line).  All float32, in this order: delta = (r + (gamma * next) * nd) - V;
	// A = delta + ((gamma * lambda) * nd) * A_next;  return = A + V, with nd = done ? 0 : 1 and next = V[t + 1], or last[e] in the last row.
	__global__ void __launch_bounds__(64) k_loco_gae(uint32_t steps, uint32_t n, float gamma, float lambda, const float* __restrict__ rewards, const float* __restrict__ values,
		const int32_t* __restrict__ dones, const float* __restrict__ lastValues, float* __restrict__ advantages, float* __restrict__ returns)
	{
		const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
		if (e >= n) return;
		const float gl = gamma * lambda;
		float next = lastValues[e], advantage = 0.f;
		for (uint32_t t = steps; t-- > 0;)
		{
			const size_t i = (size_t)n * t + e;
			const float nd = dones[i] ? 0.f : 1.f, value = values[i];
			const float discounted = gamma * next;
			const float delta = (rewards[i] + discounted * nd) - value;
			const float carry = gl * nd;
			advantage = delta + carry * advantage;
			advantages[i] = advantage; returns[i] = advantage + value;
			next = value;
		}
	}

	// The noise alone: out[u][e][j] = noiseSample(seed, e, firstUpdate + u, j).
	__global__ void __launch_bounds__(256) k_loco_noise(uint64_t seed, uint64_t firstUpdate, uint32_t n, size_t total, float* __restrict__ out)
	{
		const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= total) return;
		const uint32_t j = (uint32_t)(i % ACTION_SIZE), e = (uint32_t)(i / ACTION_SIZE % n);
		out[i] = noiseSample(seed, e, firstUpdate + i / ((size_t)ACTION_SIZE * n), j);
	}

	// Kernel B: the random push of updatePhysics (:322-330), drawn in its order, as a ray for mi_test_physics_interaction_batch.
	__global__ void __launch_bounds__(64) k_loco_push_rays(uint32_t n, uint64_t* __restrict__ rngAll, const float4* __restrict__ poseLerp, float4* __restrict__ rays)
	{
		const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
		if (e >= n) return;
		rng64 rng; rng.state = rngAll[e];
		float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f);
		if (rng.f01() < 0.02f) // a random push every ~50 steps
		{
			uint32_t bodyPartIndex = rng.u32Between(0, NUM_BODY_PARTS - 1);
			const float4 p = poseLerp[2 * (NUM_BODY_PARTS * e + bodyPartIndex)];
			vec3 part = v3(p.x, p.y, p.z) + v3(0.f, 0.2f, 0.f);
			float dx = rng.between(-1.f, 1.f), dz = rng.between(-1.f, 1.f);
			vec3 direction = normalize(v3(dx, 0.f, dz));
			vec3 origin = part - direction * 5.f;
			r0 = make_float4(origin.x, origin.y, origin.z, 1000.f); r1 = make_float4(direction.x, direction.y, direction.z, 1.f);
		}
		rngAll[e] = rng.state;
		rays[2 * e] = r0; rays[2 * e + 1] = r1;
	}

	// Kernel C: getState, hasFallen and getReward of every listed environment (all when ids is null), into row e of the outputs.
	// With a mask only the environments whose mask word is set; mirror (may be null) receives a second copy of the state rows.
	__global__ void __launch_bounds__(64) k_loco_gather(uint32_t count, const uint32_t* __restrict__ ids, const int32_t* __restrict__ mask, const env_init* __restrict__ init,
		const float* __restrict__ smoothedAll, const float4* __restrict__ poseLerp, const float4* __restrict__ vel, float* __restrict__ states, float* __restrict__ mirror,
		float* __restrict__ rewards, int32_t* __restrict__ fallen)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= count) return;
		const uint32_t e = ids ? ids[i] : i;
		if (mask && !mask[e]) return;
		ragdoll_view v;
		loadView(v, poseLerp, vel, NUM_BODY_PARTS * e);
		const training& t = init[e].train;
		float* out = states + (size_t)STATE_SIZE * e;
		getState(v, t, smoothedAll + (size_t)ACTION_SIZE * e, out);
		const bool failure = hasFallen(out);
		rewards[e] = failure ? 0.f : getReward(v, t);
		fallen[e] = failure ? 1 : 0;
		if (mirror) for (int k = 0; k < STATE_SIZE; ++k) mirror[(size_t)STATE_SIZE * e + k] = out[k];
	}

	// Reset of the listed environments (with a mask instead of ids: of every environment whose mask word is set): spawn pose into the three pose copies, velocities and accumulators zeroed (vel.w = invMass
	// kept), smoothed action zeroed and applied (resetTraining's applyAction(zero)).
	__global__ void __launch_bounds__(64) k_loco_reset(uint32_t count, const uint32_t* __restrict__ ids, const int32_t* __restrict__ mask, const env_init* __restrict__ init, float* __restrict__ smoothedAll,
		const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods, float4* pose, float4* pose0, float4* poseLerp, float4* vel, float4* force)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= count) return;
		const uint32_t e = ids ? ids[i] : i;
		if (mask && !mask[e]) return;
		for (int k = 0; k < 2 * NUM_BODY_PARTS; ++k)
		{
			const size_t j = 2 * (size_t)NUM_BODY_PARTS * e + k;
			pose[j] = init[e].spawn[k]; pose0[j] = init[e].spawn[k]; poseLerp[j] = init[e].spawn[k];
			vel[j] = make_float4(0.f, 0.f, 0.f, (k & 1) ? 0.f : vel[j].w);
			force[j] = make_float4(0.f, 0.f, 0.f, 0.f);
		}
		float smoothed[ACTION_SIZE];
		for (int k = 0; k < ACTION_SIZE; ++k) { smoothed[k] = 0.f; smoothedAll[ACTION_SIZE * e + k] = 0.f; }
		writeMotors(e, smoothed, slots, conePods, hingePods);
	}

	// The joint PODs of the world may move (any joint add / delete / set): refetch the pointers and slots when the generation changed.
	int refreshPods(batch& b)
	{
		const uint32_t types[2] = { MI_CONSTRAINT_CONE_TWIST, MI_CONSTRAINT_HINGE };
		bool changed = false;
		for (int k = 0; k < 2; ++k)
		{
			uint32_t gen = 0; void* p = nullptr;
			if (int e = mi_joint_device_pods(b.world, types[k], &p, nullptr, 0, &gen)) return e;
			changed |= gen != b.generation[k] || p != b.pods[k];
		}
		if (!changed) return 0;
		std::vector<uint32_t> slots((size_t)NUM_MOTOR_JOINTS * b.n);
		for (int k = 0; k < 2; ++k)
		{
			const uint32_t numIds = (k == 0 ? NUM_CONE_TWIST : NUM_HINGE) * b.n;
			std::vector<uint32_t> slotOf(numIds);
			if (int e = mi_joint_device_pods(b.world, types[k], &b.pods[k], slotOf.data(), numIds, &b.generation[k])) return e;
			for (uint32_t env = 0; env < b.n; ++env)
				for (int i = 0; i < (k == 0 ? NUM_CONE_TWIST : NUM_HINGE); ++i)
				{
					const uint32_t id = k == 0 ? b.dolls[env].coneTwist[i] : b.dolls[env].hinge[i];
					const uint32_t s = id < numIds ? slotOf[id] : ~0u;
					if (s == ~0u) { fprintf(stderr, "locomotion batch: a ragdoll joint was deleted\n"); return MI_ERR_INVALID_STATE; }
					slots[(size_t)NUM_MOTOR_JOINTS * env + (k == 0 ? 0 : NUM_CONE_TWIST) + i] = s;
				}
		}
		if (!ok(hipMemcpyAsync(b.dSlots, slots.data(), sizeof(uint32_t) * slots.size(), hipMemcpyHostToDevice, b.stream), "slots")) return MI_ERR_HIP;
		if (!ok(hipStreamSynchronize(b.stream), "slots")) return MI_ERR_HIP;
		return 0;
	}

	dim3 blocks(uint32_t n) { return dim3((n + 63) / 64); }

	int launchReset(batch& b, const uint32_t* dIds, const int32_t* dMask, uint32_t count)
	{
		if (int e = refreshPods(b)) return e;
		hipLaunchKernelGGL(k_loco_reset, blocks(count), dim3(64), 0, b.stream, count, dIds, dMask, b.dInit, b.dSmoothed, b.dSlots, (uint8_t*)b.pods[0], (uint8_t*)b.pods[1],
			(float4*)b.ds.pose, (float4*)b.ds.pose0, (float4*)b.ds.poseLerp, (float4*)b.ds.vel, (float4*)b.ds.force);
		return ok(hipGetLastError(), "reset kernel") ? 0 : MI_ERR_HIP;
	}

	// The rows go to dStates; when that is not the batch's own current-state buffer (or is null), b.dStates receives them too.
	int launchGather(batch& b, const uint32_t* dIds, const int32_t* dMask, uint32_t count, float* dStates, float* dRewards, int32_t* dFallen)
	{
		float* primary = dStates ? dStates : b.dStates;
		hipLaunchKernelGGL(k_loco_gather, blocks(count), dim3(64), 0, b.stream, count, dIds, dMask, b.dInit, b.dSmoothed, (const float4*)b.ds.poseLerp, (const float4*)b.ds.vel,
			primary, primary == b.dStates ? nullptr : b.dStates, dRewards, dFallen);
		return ok(hipGetLastError(), "gather kernel") ? 0 : MI_ERR_HIP;
	}

	dim3 networkBlock(uint32_t hidden) { return dim3(64 * ((hidden + 63) / 64)); }

	// A network on count rows of dStatesIn, on the world's stream.  With apply (the policy only): rows are the environments, smoothed and
	// motors written.
	int launchNetwork(batch& b, const device_network& net, bool apply, uint32_t count, const float* dStatesIn, float* dOut, float* dHiddenOut)
	{
		const auto kernel = net.outputs == 1 ? k_loco_policy<1, false> : apply ? k_loco_policy<ACTION_SIZE, true> : k_loco_policy<ACTION_SIZE, false>;
		hipLaunchKernelGGL(kernel, dim3((count + POLICY_TILE - 1) / POLICY_TILE), networkBlock(net.hidden), 0, b.stream, count, net.hidden, dStatesIn, (const float*)net.data, dOut, dHiddenOut,
			apply ? b.dSmoothed : nullptr, apply ? (const uint32_t*)b.dSlots : nullptr, apply ? (uint8_t*)b.pods[0] : nullptr, apply ? (uint8_t*)b.pods[1] : nullptr);
		return ok(hipGetLastError(), "network kernel") ? 0 : MI_ERR_HIP;
	}

	// Replaces *p by a new buffer of `floats` floats; *p stays null, and *recorded (may be null) 0, where that fails.  The caller has made
	// sure that nothing in flight uses the old one.
	int reallocate(float** p, size_t floats, size_t* recorded = nullptr)
	{
		if (*p) (void)hipFree(*p);
		*p = nullptr; if (recorded) *recorded = 0;
		if (!ok(hipMalloc(p, sizeof(float) * floats), "alloc")) return MI_ERR_HIP;
		if (recorded) *recorded = floats;
		return 0;
	}

	// The network that the host keeps for `net` (setPhysicsPolicy or setPhysicsValueNetwork), if any, transposed to [in][out] once, here.
	int uploadNetwork(batch& b, device_network& net)
	{
		locomotion_policy p;
		if (!locomotionNetwork(net.outputs, &p)) return 0;
		std::vector<float> t(networkFloats(p.hidden, p.outputs));
		copyNetwork(p, networkOf(t.data(), p.hidden, p.outputs), NETWORK_TO_DEVICE);
		if (!ok(hipStreamSynchronize(b.stream), "network")) return MI_ERR_HIP; // nothing in flight reads the old one
		net.hidden = 0;
		if (int e = reallocate(&net.data, t.size())) return e;
		if (!ok(hipMemcpyAsync(net.data, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, b.stream), "network") || !ok(hipStreamSynchronize(b.stream), "network")) return MI_ERR_HIP;
		net.hidden = p.hidden;
		return 0;
	}

	// std and logStd of setPhysicsActionStd into the first half of dScales.
	int uploadActionStd(batch& b)
	{
		const float* scales = locomotionActionStd();
		if (!scales) return 0;
		if (!ok(hipMemcpyAsync(b.dScales, scales, sizeof(float) * 2 * ACTION_SIZE, hipMemcpyHostToDevice, b.stream), "std") || !ok(hipStreamSynchronize(b.stream), "std")) return MI_ERR_HIP;
		b.stdSet = true;
		return 0;
	}

	// The action ranges of getPhysicsRanges into the second half of dScales, once per batch; they are those of any ragdoll, read from one
	// in a world of its own so that the batch's world is not touched.
	int uploadRanges(batch& b)
	{
		if (b.rangesSet) return 0;
		static bool known = false;
		static float ranges[2 * ACTION_SIZE];
		if (!known)
		{
			mi_world_desc d = { -1, 0, 0, 0 };
			mi_world* w = mi_world_create(&d);
			if (!w) return MI_ERR_NO_DEVICE;
			ragdoll r = createRagdoll(w, v3(0.f, 0.f, 0.f), 0.f);
			fillRanges(w, r, ranges, ranges + ACTION_SIZE);
			mi_world_destroy(w);
			known = true;
		}
		if (!ok(hipMemcpyAsync(b.dScales + 2 * ACTION_SIZE, ranges, sizeof(ranges), hipMemcpyHostToDevice, b.stream), "ranges") || !ok(hipStreamSynchronize(b.stream), "ranges")) return MI_ERR_HIP;
		b.rangesSet = true;
		return 0;
	}

	// One update of every environment, all on the world's stream, writing the three outputs (device pointers; dStates may be null, the
	// batch's current-state buffer receives the states in any case).  With dActions: applyAction of these.  Without: the policy on the
	// current states, its raw outputs to dActionsOut (may be null).
	int launchAfterAction(batch& b, float* dStates, float* dRewards, int32_t* dFallen);
	int launchUpdate(batch& b, const float* dActions, float* dActionsOut, float* dStates, float* dRewards, int32_t* dFallen)
	{
		if (int e = refreshPods(b)) return e;
		if (dActions) hipLaunchKernelGGL(k_loco_actions, blocks(b.n), dim3(64), 0, b.stream, b.n, dActions, b.dSmoothed, b.dSlots, (uint8_t*)b.pods[0], (uint8_t*)b.pods[1]);
		else if (int e = launchNetwork(b, b.policy, true, b.n, b.dStates, dActionsOut, nullptr)) return e;
		return launchAfterAction(b, dStates, dRewards, dFallen);
	}

	// The rest of an update once the motors are written: push, step, gather.
	int launchAfterAction(batch& b, float* dStates, float* dRewards, int32_t* dFallen)
	{
		hipLaunchKernelGGL(k_loco_push_rays, blocks(b.n), dim3(64), 0, b.stream, b.n, b.dRng, (const float4*)b.ds.poseLerp, (float4*)b.dRays);
		if (!ok(hipGetLastError(), "action / push kernels")) return MI_ERR_HIP;
		if (int e = mi_test_physics_interaction_batch(b.world, b.n, 0, NUM_BODY_PARTS, b.dRays, b.dPushes)) return e;
		mi_physics_settings s = { 1, 60, 4, 30, 0, 1, 0, 1, 1, 1 };
		float timer = 0.f;
		if (int e = mi_step(b.world, &timer, &s, 1.f / 60.f)) return e;
		return launchGather(b, nullptr, nullptr, b.n, dStates, dRewards, dFallen);
	}

	// Ends the training session, if one is open: the optimiser state goes, the parameters stay as they are.
	int endTraining(batch& b)
	{
		if (!b.training) return 0;
		b.training = false; b.adamStep = 0;
		if (!ok(hipStreamSynchronize(b.stream), "end training")) return MI_ERR_HIP;
		if (b.dMoments) (void)hipFree(b.dMoments);
		b.dMoments = nullptr;
		return 0;
	}

	ppo_parameters parametersOf(batch& b) { return { b.policy.data, b.critic.data, b.dScales, b.policy.hidden, b.critic.hidden }; }
	ppo_scratch scratchOf(batch& b) { return { b.dSlab, b.dPartial, b.dGroupStats }; }

	// The scratch of the gradient step for minibatches of up to `count` rows with the networks as they are.
	int ensureScratch(batch& b, uint32_t count)
	{
		const size_t total = ppoTotal(b.policy.hidden, b.critic.hidden), slab = total * ppoGroups(count);
		if (slab <= b.slabFloats && total <= b.gradientFloats) return 0;
		if (!ok(hipStreamSynchronize(b.stream), "scratch")) return MI_ERR_HIP; // nothing in flight uses the old buffers
		if (slab > b.slabFloats && reallocate(&b.dSlab, slab, &b.slabFloats)) return MI_ERR_HIP;
		if (total > b.gradientFloats)
		{
			b.gradientFloats = 0;
			if (reallocate(&b.dGradient, total) || reallocate(&b.dPartial, ppoBlocks(total)) || reallocate(&b.dGroupStats, PPO_MAX_GROUPS * PPO_GROUP_STATS)) return MI_ERR_HIP;
			b.gradientFloats = total;
		}
		return 0;
	}

	// A network of the master copy back into the [out][in] arrays the setters take (host pointers).
	int readNetwork(batch& b, const device_network& net, float* w1, float* b1, float* w2, float* b2, float* w3, float* b3)
	{
		std::vector<float> t(networkFloats(net.hidden, net.outputs));
		if (!ok(hipMemcpyAsync(t.data(), net.data, sizeof(float) * t.size(), hipMemcpyDeviceToHost, b.stream), "read network") || !ok(hipStreamSynchronize(b.stream), "read network")) return MI_ERR_HIP;
		copyNetwork(networkOf((const float*)t.data(), net.hidden, net.outputs), { net.hidden, net.outputs, { w1, w2, w3 }, { b1, b2, b3 } }, NETWORK_TO_HOST);
		return 0;
	}

	int copyOut(batch& b, float* outStates, float* outRewards, int32_t* outFallen)
	{
		if (outStates && !ok(hipMemcpyAsync(outStates, b.dStates, sizeof(float) * STATE_SIZE * b.n, hipMemcpyDeviceToHost, b.stream), "states")) return MI_ERR_HIP;
		if (outRewards && !ok(hipMemcpyAsync(outRewards, b.dRewards, sizeof(float) * b.n, hipMemcpyDeviceToHost, b.stream), "rewards")) return MI_ERR_HIP;
		if (outFallen && !ok(hipMemcpyAsync(outFallen, b.dFallen, sizeof(int32_t) * b.n, hipMemcpyDeviceToHost, b.stream), "fallen")) return MI_ERR_HIP;
		return ok(hipStreamSynchronize(b.stream), "copy out") ? 0 : MI_ERR_HIP;
	}

	// The tail of an update from the host: copyOut, then the number of fallen environments (negative: an error code).
	int copyOutFallen(batch& b, float* outStates, float* outRewards, int32_t* outFallen)
	{
		std::vector<int32_t> fallen(b.n);
		if (int e = copyOut(b, outStates, outRewards, fallen.data())) return -e;
		int count = 0;
		for (uint32_t i = 0; i < b.n; ++i) count += fallen[i] != 0;
		if (outFallen) memcpy(outFallen, fallen.data(), sizeof(int32_t) * b.n);
		return count;
	}
}

extern "C"
{
	// Builds the world of numEnvs environments and resets all of them; outStates (host, numEnvs x 66) may be NULL.
	int resetPhysicsBatch(uint32_t numEnvs, float* outStates)
	{
		release(B); B = nullptr;
		if (!numEnvs) return MI_ERR_INVALID_ARGUMENT;
		batch* b = new batch;
		b->n = numEnvs;
		mi_world_desc d = { -1, NUM_BODY_PARTS * numEnvs, 0, 0 };
		b->world = mi_world_create(&d);
		if (!b->world) { fprintf(stderr, "resetPhysicsBatch: %s\n", mi_last_error(nullptr)); delete b; return MI_ERR_NO_DEVICE; }
		uint32_t side = 1;
		while (side * side < numEnvs) ++side;
		const float half = 0.5f * GRID_PITCH * (float)(side - 1);
		addGround(b->world, half + 20.f); // the single environment's ±20 m around every ragdoll
		for (uint32_t e = 0; e < numEnvs; ++e)
		{
			vec3 hip = v3(GRID_PITCH * (float)(e % side) - half, 1.25f, GRID_PITCH * (float)(e / side) - half);
			b->dolls.push_back(createRagdoll(b->world, hip, 0.f));
			if (b->dolls.back().body[0] != NUM_BODY_PARTS * e) { fprintf(stderr, "resetPhysicsBatch: unexpected body ids\n"); release(b); return MI_ERR_INVALID_STATE; }
		}
		// the single environment's snapshot + resetTraining, per environment, on the host
		const uint32_t nb = mi_num_bodies(b->world);
		std::vector<float> t(7 * (size_t)nb), v(6 * (size_t)nb), mp(13 * (size_t)nb);
		mi_read_transforms(b->world, 0, t.data(), nb); mi_read_velocities(b->world, v.data(), nb); mi_read_mass_properties(b->world, mp.data(), nb);
		std::vector<env_init> init(numEnvs);
		for (uint32_t e = 0; e < numEnvs; ++e)
		{
			ragdoll_view view;
			env_init& in = init[e];
			for (int i = 0; i < NUM_BODY_PARTS; ++i)
			{
				const size_t body = b->dolls[e].body[i];
				const float* p = &t[7 * body]; const float* q = &v[6 * body]; const float* m = &mp[13 * body];
				view.transform[i] = { { p[3], p[4], p[5], p[6] }, { p[0], p[1], p[2] } };
				view.linearVelocity[i] = v3(q[0], q[1], q[2]); view.angularVelocity[i] = v3(q[3], q[4], q[5]);
				in.train.localCOG[i] = v3(m[0], m[1], m[2]);
				in.spawn[2 * i] = make_float4(p[0], p[1], p[2], 0.f); in.spawn[2 * i + 1] = make_float4(p[3], p[4], p[5], p[6]);
			}
			resetTargets(view, b->dolls[e].boxMin, b->dolls[e].boxMax, in.train);
		}
		std::vector<uint64_t> rng(numEnvs);
		std::vector<uint32_t> ids(numEnvs);
		const uint64_t seed = locomotionSeed();
		for (uint32_t e = 0; e < numEnvs; ++e) { uint64_t s = seed ^ ((uint64_t)e * 0x9E3779B97F4A7C15ull); rng[e] = s ? s : 0x9E3779B97F4A7C15ull; ids[e] = e; }
		bool good = mi_device_state(b->world, &b->ds) == MI_OK;
		b->stream = (hipStream_t)b->ds.stream;
		const size_t n = numEnvs;
		good = good && ok(hipMalloc(&b->dInit, sizeof(env_init) * n), "alloc") && ok(hipMalloc(&b->dSmoothed, sizeof(float) * ACTION_SIZE * n), "alloc")
			&& ok(hipMalloc(&b->dRng, sizeof(uint64_t) * n), "alloc") && ok(hipMalloc(&b->dRays, sizeof(float) * 8 * n), "alloc")
			&& ok(hipMalloc(&b->dPushes, sizeof(int32_t) * n), "alloc") && ok(hipMalloc(&b->dSlots, sizeof(uint32_t) * NUM_MOTOR_JOINTS * n), "alloc")
			&& ok(hipMalloc(&b->dActions, sizeof(float) * ACTION_SIZE * n), "alloc") && ok(hipMalloc(&b->dStates, sizeof(float) * STATE_SIZE * n), "alloc")
			&& ok(hipMalloc(&b->dRewards, sizeof(float) * n), "alloc") && ok(hipMalloc(&b->dFallen, sizeof(int32_t) * n), "alloc")
			&& ok(hipMalloc(&b->dIds, sizeof(uint32_t) * n), "alloc") && ok(hipMalloc(&b->dScales, sizeof(float) * 4 * ACTION_SIZE), "alloc");
		good = good && ok(hipMemcpyAsync(b->dInit, init.data(), sizeof(env_init) * n, hipMemcpyHostToDevice, b->stream), "init")
			&& ok(hipMemcpyAsync(b->dRng, rng.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, b->stream), "rng")
			&& ok(hipMemcpyAsync(b->dIds, ids.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, b->stream), "ids")
			&& ok(hipMemsetAsync(b->dPushes, 0, sizeof(int32_t) * n, b->stream), "pushes");
		if (!good) { release(b); return MI_ERR_HIP; }
		B = b;
		int e = launchReset(*b, b->dIds, nullptr, numEnvs);
		if (!e) e = launchGather(*b, nullptr, nullptr, numEnvs, b->dStates, b->dRewards, b->dFallen);
		if (!e) e = uploadNetwork(*b, b->policy);
		if (!e) e = uploadNetwork(*b, b->critic);
		if (!e) e = uploadActionStd(*b);
		if (!e) e = copyOut(*b, outStates, nullptr, nullptr);
		return e;
	}

	// One step of every environment from host buffers: actions numEnvs x 27 in, states numEnvs x 66, rewards, fallen out.
	// Returns the number of fallen environments (negative: an error code).
	int updatePhysicsBatch(const float* actions, float* outStates, float* outRewards, int32_t* outFallen)
	{
		if (!B || !actions) return -MI_ERR_INVALID_STATE;
		batch& b = *B;
		if (!ok(hipMemcpyAsync(b.dActions, actions, sizeof(float) * ACTION_SIZE * b.n, hipMemcpyHostToDevice, b.stream), "actions")) return -MI_ERR_HIP;
		if (int e = launchUpdate(b, b.dActions, nullptr, b.dStates, b.dRewards, b.dFallen)) return -e;
		return copyOutFallen(b, outStates, outRewards, outFallen);
	}

	// The same from device buffers, enqueued on the world's stream (getPhysicsBatchStream) without a host synchronisation.
	int updatePhysicsBatchDevice(const float* dActions, float* dStates, float* dRewards, int32_t* dFallen)
	{
		if (!B || !dActions || !dStates || !dRewards || !dFallen) return MI_ERR_INVALID_STATE;
		return launchUpdate(*B, dActions, nullptr, dStates, dRewards, dFallen);
	}

	// Resets the listed environments (host ids) and writes their rows of outStates (host, numEnvs x 66); other rows are untouched.
	int resetPhysicsBatchEnvs(const uint32_t* envIds, uint32_t count, float* outStates)
	{
		if (!B) return MI_ERR_INVALID_STATE;
		batch& b = *B;
		if (!count) return 0;
		if (!envIds || count > b.n) return MI_ERR_INVALID_ARGUMENT;
		for (uint32_t i = 0; i < count; ++i) if (envIds[i] >= b.n) return MI_ERR_INVALID_ARGUMENT;
		uint32_t* dList = nullptr;
		if (!ok(hipMalloc(&dList, sizeof(uint32_t) * count), "alloc")) return MI_ERR_HIP;
		int e = ok(hipMemcpyAsync(dList, envIds, sizeof(uint32_t) * count, hipMemcpyHostToDevice, b.stream), "ids") ? 0 : MI_ERR_HIP;
		if (!e) e = launchReset(b, dList, nullptr, count);
		if (!e) e = launchGather(b, dList, nullptr, count, b.dStates, b.dRewards, b.dFallen);
		std::vector<float> states((size_t)STATE_SIZE * b.n);
		if (!e) e = copyOut(b, states.data(), nullptr, nullptr);
		(void)hipFree(dList);
		if (!e && outStates) for (uint32_t i = 0; i < count; ++i) memcpy(outStates + (size_t)STATE_SIZE * envIds[i], states.data() + (size_t)STATE_SIZE * envIds[i], sizeof(float) * STATE_SIZE);
		return e;
	}

	// State, reward and fallen of every environment as they are now, without stepping (host buffers, any may be NULL).
	int observePhysicsBatch(float* outStates, float* outRewards, int32_t* outFallen)
	{
		if (!B) return MI_ERR_INVALID_STATE;
		if (int e = launchGather(*B, nullptr, nullptr, B->n, B->dStates, B->dRewards, B->dFallen)) return e;
		return copyOut(*B, outStates, outRewards, outFallen);
	}

	void* getPhysicsBatchWorld(void) { return B ? (void*)B->world : nullptr; }
	void* getPhysicsBatchStream(void) { return B ? (void*)B->stream : nullptr; }

	// The pushes of the last update: outBodies[e] = 1 + the pushed body (a body of env e), or 0.  Returns how many envs were pushed.
	int getPhysicsBatchPushes(int32_t* outBodies)
	{
		if (!B || !outBodies) return -MI_ERR_INVALID_STATE;
		if (!ok(hipMemcpyAsync(outBodies, B->dPushes, sizeof(int32_t) * B->n, hipMemcpyDeviceToHost, B->stream), "pushes") || !ok(hipStreamSynchronize(B->stream), "pushes")) return -MI_ERR_HIP;
		int count = 0;
		for (uint32_t i = 0; i < B->n; ++i) count += outBodies[i] != 0;
		return count;
	}

	// The network alone on count rows of dStates (device, count x 66) into dActions (count x 27), on the world's stream; dHidden (may be
	// NULL, count x 2H) receives tanh(z1), tanh(z2) of every row: a parity facility.  Touches no environment.
	int inferPhysicsBatchDevice(uint32_t count, const float* dStates, float* dActions, float* dHidden)
	{
		if (!B || !B->policy.hidden) return MI_ERR_INVALID_STATE;
		if (!count || !dStates || !dActions) return MI_ERR_INVALID_ARGUMENT;
		return launchNetwork(*B, B->policy, false, count, dStates, dActions, dHidden);
	}

	// One closed-loop update of every environment, host buffers out (any may be NULL).  Returns what updatePhysicsBatch returns.
	int updatePhysicsBatchPolicy(float* outStates, float* outRewards, int32_t* outFallen)
	{
		if (!B || !B->policy.hidden) return -MI_ERR_INVALID_STATE;
		batch& b = *B;
		if (int e = launchUpdate(b, nullptr, nullptr, b.dStates, b.dRewards, b.dFallen)) return -e;
		return copyOutFallen(b, outStates, outRewards, outFallen);
	}

	// The same into device buffers, enqueued on the world's stream without a host synchronisation; dActions (may be NULL, n x 27)
	// receives the raw, unsmoothed network outputs.
	int updatePhysicsBatchPolicyDevice(float* dStates, float* dRewards, int32_t* dFallen, float* dActions)
	{
		if (!B || !B->policy.hidden || !dStates || !dRewards || !dFallen) return MI_ERR_INVALID_STATE;
		return launchUpdate(*B, nullptr, dActions, dStates, dRewards, dFallen);
	}

	// `steps` closed-loop updates enqueued back to back: row t of dStates [steps][n][66] (may be NULL), dActions [steps][n][27] (may be
	// NULL), dRewards [steps][n], dFallen [steps][n] holds the action taken at update t and the state, reward and fallen after it.
	// With autoReset every environment whose fallen is 1 after an update (the last one included) is reset on the device before the
	// next: spawn pose, zero velocities, zero smoothed action, motors rewritten, its random stream left alone; row t keeps the
	// terminal state, and the policy's next input is the reset state.  No host synchronisation beyond those of mi_step.
	int rolloutPhysicsBatchDevice(uint32_t steps, int autoReset, float* dStates, float* dActions, float* dRewards, int32_t* dFallen)
	{
		if (!B || !B->policy.hidden || !dRewards || !dFallen) return MI_ERR_INVALID_STATE;
		batch& b = *B;
		const size_t n = b.n;
		for (uint32_t t = 0; t < steps; ++t)
		{
			int32_t* fallen = dFallen + n * t;
			if (int e = launchUpdate(b, nullptr, dActions ? dActions + ACTION_SIZE * n * t : nullptr, dStates ? dStates + STATE_SIZE * n * t : nullptr, dRewards + n * t, fallen)) return e;
			if (!autoReset) continue;
			if (int e = launchReset(b, nullptr, fallen, b.n)) return e;
			if (int e = launchGather(b, nullptr, fallen, b.n, b.dStates, b.dRewards, b.dFallen)) return e;
		}
		return 0;
	}

	// The critic alone on count rows of dStates (device, count x 66) into dValues (count), on the world's stream; dHidden (may be NULL,
	// count x 2Hv) receives tanh(z1), tanh(z2) of every row.  Touches no environment.
	int inferPhysicsBatchValueDevice(uint32_t count, const float* dStates, float* dValues, float* dHidden)
	{
		if (!B || !B->critic.hidden) return MI_ERR_INVALID_STATE;
		if (!count || !dStates || !dValues) return MI_ERR_INVALID_ARGUMENT;
		return launchNetwork(*B, B->critic, false, count, dStates, dValues, dHidden);
	}

	// The exploration noise of updates firstUpdate .. firstUpdate + numUpdates - 1 of every environment into dEps [numUpdates][n][27], on
	// the world's stream: what collectPhysicsBatchDevice draws at those counters.  Moves neither the counter nor any random state.
	int samplePhysicsBatchNoiseDevice(unsigned long long firstUpdate, uint32_t numUpdates, float* dEps)
	{
		if (!B) return MI_ERR_INVALID_STATE;
		if (!numUpdates || !dEps) return MI_ERR_INVALID_ARGUMENT;
		const size_t total = (size_t)numUpdates * B->n * ACTION_SIZE;
		hipLaunchKernelGGL(k_loco_noise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, B->stream, (uint64_t)locomotionSeed(), (uint64_t)firstUpdate, B->n, total, dEps);
		return ok(hipGetLastError(), "noise kernel") ? 0 : MI_ERR_HIP;
	}

	// Collecting updates since resetPhysicsBatch: the counter the next collectPhysicsBatchDevice starts at (0 without a batch).
	unsigned long long getPhysicsBatchNoiseCounter(void) { return B ? B->noiseCounter : 0; }

	// `steps` closed-loop updates with sampled actions, enqueued back to back, always with the device-side reset of the fallen.  Row t:
	// dObs [steps][n][66] the states the networks saw at update t (after a fall: the reset state); dActions [steps][n][27] the sample
	// a = mu + std * eps, unclipped; dEps [steps][n][27] (may be NULL) the noise; dLogProbs [steps][n] log N(a; mu, std); dValues
	// [steps][n] the critic on dObs[t]; dRewards, dDones [steps][n] reward and fallen after the update.  The environment receives a,
	// with clip != 0 a clamped to the action ranges of getPhysicsRanges.  dLastValues [n]: the critic on the states after the last
	// update's reset.  Needs a policy, a critic and a std.
	int collectPhysicsBatchDevice(uint32_t steps, int clip, float* dObs, float* dActions, float* dEps, float* dLogProbs, float* dValues, float* dRewards, int32_t* dDones, float* dLastValues)
	{
		if (!B || !B->policy.hidden || !B->critic.hidden || !B->stdSet) return MI_ERR_INVALID_STATE;
		if (!steps || !dObs || !dActions || !dLogProbs || !dValues || !dRewards || !dDones || !dLastValues) return MI_ERR_INVALID_ARGUMENT;
		batch& b = *B;
		if (int e = uploadRanges(b)) return e;
		const size_t n = b.n;
		const uint64_t seed = locomotionSeed();
		const dim3 grid((b.n + POLICY_TILE - 1) / POLICY_TILE), block = networkBlock(b.policy.hidden > b.critic.hidden ? b.policy.hidden : b.critic.hidden);
		for (uint32_t t = 0; t < steps; ++t)
		{
			int32_t* fallen = dDones + n * t;
			if (int e = refreshPods(b)) return e;
			hipLaunchKernelGGL(k_loco_sample, grid, block, 0, b.stream, b.n, b.policy.hidden, b.critic.hidden, clip, seed, b.noiseCounter, (const float*)b.dStates, (const float*)b.policy.data,
				(const float*)b.critic.data, (const float*)b.dScales, dObs + STATE_SIZE * n * t, dActions + ACTION_SIZE * n * t, dEps ? dEps + ACTION_SIZE * n * t : nullptr,
				dLogProbs + n * t, dValues + n * t, b.dSmoothed, (const uint32_t*)b.dSlots, (uint8_t*)b.pods[0], (uint8_t*)b.pods[1]);
			if (!ok(hipGetLastError(), "sample kernel")) return MI_ERR_HIP;
			++b.noiseCounter;
			if (int e = launchAfterAction(b, nullptr, dRewards + n * t, fallen)) return e;
			if (int e = launchReset(b, nullptr, fallen, b.n)) return e;
			if (int e = launchGather(b, nullptr, fallen, b.n, b.dStates, b.dRewards, b.dFallen)) return e;
		}
		return launchNetwork(b, b.critic, false, b.n, b.dStates, dLastValues, nullptr);
	}

	// Generalised advantage estimation over [steps][n] device buffers (k_loco_gae), on the batch's stream.  Episodes end by falling only:
	// a done row bootstraps nothing, every other row bootstraps from the next value (the last row from dLastValues).
	int gaePhysicsBatchDevice(uint32_t steps, uint32_t n, float gamma, float lambda, const float* dRewards, const float* dValues, const int32_t* dDones, const float* dLastValues,
		float* dAdvantages, float* dReturns)
	{
		if (!B) return MI_ERR_INVALID_STATE;
		if (!steps || !n || !dRewards || !dValues || !dDones || !dLastValues || !dAdvantages || !dReturns) return MI_ERR_INVALID_ARGUMENT;
		hipLaunchKernelGGL(k_loco_gae, blocks(n), dim3(64), 0, B->stream, steps, n, gamma, lambda, dRewards, dValues, dDones, dLastValues, dAdvantages, dReturns);
		return ok(hipGetLastError(), "gae kernel") ? 0 : MI_ERR_HIP;
	}

	// Opens a training session on the batch's networks: Adam (torch.optim.Adam: lr, betas, eps) with m, v and the step count at zero.
	// From here on the device buffers the kernels read are the master copy of the parameters: updatePhysicsBatchPPODevice moves them in
	// place, readPhysicsBatch* return them, and the library's host copies (what the setters received) fall behind.  setPhysicsPolicy,
	// setPhysicsValueNetwork and setPhysicsActionStd end the session and drop the optimiser state; so does resetPhysicsBatch, which
	// builds a new batch from the host copies.  Needs a policy, a critic and a std.
	int beginPhysicsBatchTraining(float lr, float beta1, float beta2, float adamEps)
	{
		if (!B || !B->policy.hidden || !B->critic.hidden || !B->stdSet) return MI_ERR_INVALID_STATE;
		if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(adamEps >= 0.f)) return MI_ERR_INVALID_ARGUMENT;
		batch& b = *B;
		if (int e = endTraining(b)) return e;
		const size_t total = ppoTotal(b.policy.hidden, b.critic.hidden);
		if (int e = reallocate(&b.dMoments, 2 * total)) return e;
		if (!ok(hipMemsetAsync(b.dMoments, 0, sizeof(float) * 2 * total, b.stream), "moments")) return MI_ERR_HIP;
		b.lr = lr; b.beta1 = beta1; b.beta2 = beta2; b.adamEps = adamEps; b.adamStep = 0; b.training = true;
		return 0;
	}

	int endPhysicsBatchTraining(void) { return B ? endTraining(*B) : MI_ERR_INVALID_STATE; }

	// PPO's epochs over `rows` collected rows (device buffers: dObs [rows][66], dActions [rows][27], dOldLogProbs, dAdvantages, dReturns
	// [rows]), enqueued on the world's stream, three launches per minibatch, no host synchronisation.  dOrder [epochs][rows] (uint32 row
	// indices, one permutation per epoch; an index >= rows reads the last row) is cut into ceil(rows / batchSize) minibatches per epoch,
	// the last one short.  Each minibatch is one optimiser step of training.py's loop: ppo_loss (clipRange, vfCoef, entCoef, advantages
	// normalised per minibatch of more than one row with normalizeAdvantage), clip_grad_norm_(maxGradNorm), Adam.  dStats (may be NULL)
	// [epochs * minibatches][5] receives per step {loss, policy loss, value loss, clip fraction, gradient norm before clipping}.
	int updatePhysicsBatchPPODevice(uint32_t rows, const float* dObs, const float* dActions, const float* dOldLogProbs, const float* dAdvantages, const float* dReturns,
		uint32_t epochs, const uint32_t* dOrder, uint32_t batchSize, float clipRange, float vfCoef, float entCoef, float maxGradNorm, int normalizeAdvantage, float* dStats)
	{
		if (!B || !B->training) return MI_ERR_INVALID_STATE;
		if (!rows || !epochs || !batchSize || !dObs || !dActions || !dOldLogProbs || !dAdvantages || !dReturns || !dOrder) return MI_ERR_INVALID_ARGUMENT;
		batch& b = *B;
		if (int e = ensureScratch(b, batchSize < rows ? batchSize : rows)) return e;
		const ppo_parameters p = parametersOf(b);
		const ppo_scratch scratch = scratchOf(b);
		const ppo_rows data = { rows, dObs, dActions, dOldLogProbs, dAdvantages, dReturns };
		const ppo_loss loss = { clipRange, vfCoef, entCoef, normalizeAdvantage };
		const size_t total = ppoTotal(b.policy.hidden, b.critic.hidden);
		for (uint32_t epoch = 0; epoch < epochs; ++epoch)
			for (uint32_t start = 0; start < rows; start += batchSize)
			{
				const uint32_t count = rows - start < batchSize ? rows - start : batchSize;
				float* stats = dStats; if (dStats) dStats += PPO_STATS;
				if (int e = ppoGradients(b.stream, p, data, dOrder + (size_t)rows * epoch + start, count, loss, scratch, b.dGradient, nullptr, stats)) return e;
				const double t = (double)++b.adamStep;
				const ppo_adam adam = { b.beta1, b.beta2, b.adamEps, (float)((double)b.lr / (1.0 - pow((double)b.beta1, t))), (float)sqrt(1.0 - pow((double)b.beta2, t)), maxGradNorm };
				if (int e = ppoAdam(b.stream, p, scratch, b.dGradient, b.dMoments, b.dMoments + total, adam, stats)) return e;
			}
		return 0;
	}

	// The parity facility of the gradient step: the unclipped gradient of ppo_loss on one minibatch, dIndices [count] (uint32 rows of the
	// buffers; NULL: rows 0 .. count-1), into dGradient in the flat parameter order of locomotion_update.h (the device's [in][out]
	// layouts: actor, critic, logStd), the per-row ratio exp(logp - old) into dRatios [count] (may be NULL), and {loss, policy loss, value
	// loss, clip fraction} into dStats [4] (may be NULL).  Touches neither the parameters nor the optimiser state; needs no session.
	int gradientsPhysicsBatchPPODevice(uint32_t rows, const float* dObs, const float* dActions, const float* dOldLogProbs, const float* dAdvantages, const float* dReturns,
		uint32_t count, const uint32_t* dIndices, float clipRange, float vfCoef, float entCoef, int normalizeAdvantage, float* dGradient, float* dRatios, float* dStats)
	{
		if (!B || !B->policy.hidden || !B->critic.hidden || !B->stdSet) return MI_ERR_INVALID_STATE;
		if (!rows || !count || (!dIndices && count > rows) || !dObs || !dActions || !dOldLogProbs || !dAdvantages || !dReturns || !dGradient) return MI_ERR_INVALID_ARGUMENT;
		batch& b = *B;
		if (int e = ensureScratch(b, count)) return e;
		const ppo_rows data = { rows, dObs, dActions, dOldLogProbs, dAdvantages, dReturns };
		const ppo_loss loss = { clipRange, vfCoef, entCoef, normalizeAdvantage };
		return ppoGradients(b.stream, parametersOf(b), data, dIndices, count, loss, scratchOf(b), dGradient, dRatios, dStats);
	}

	// The parameters as they are on the device, after everything enqueued so far, in the layouts the setters take (host pointers).
	int readPhysicsBatchPolicy(float* w1, float* b1, float* w2, float* b2, float* w3, float* b3)
	{
		if (!B || !B->policy.hidden) return MI_ERR_INVALID_STATE;
		if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3) return MI_ERR_INVALID_ARGUMENT;
		return readNetwork(*B, B->policy, w1, b1, w2, b2, w3, b3);
	}
	int readPhysicsBatchValueNetwork(float* w1, float* b1, float* w2, float* b2, float* w3, float* b3)
	{
		if (!B || !B->critic.hidden) return MI_ERR_INVALID_STATE;
		if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3) return MI_ERR_INVALID_ARGUMENT;
		return readNetwork(*B, B->critic, w1, b1, w2, b2, w3, b3);
	}
	// std [27] (may be NULL) and logStd [27].
	int readPhysicsBatchLogStd(float* std, float* logStd)
	{
		if (!B || !B->stdSet) return MI_ERR_INVALID_STATE;
		if (!logStd) return MI_ERR_INVALID_ARGUMENT;
		float scales[2 * ACTION_SIZE];
		if (!ok(hipMemcpyAsync(scales, B->dScales, sizeof(scales), hipMemcpyDeviceToHost, B->stream), "read std") || !ok(hipStreamSynchronize(B->stream), "read std")) return MI_ERR_HIP;
		if (std) memcpy(std, scales, sizeof(float) * ACTION_SIZE);
		memcpy(logStd, scales + ACTION_SIZE, sizeof(float) * ACTION_SIZE);
		return 0;
	}
}

// A new network or std from the host replaces the master copy: an open training session ends with it.
int locomotionBatchNetworkChanged(uint32_t outputs) { if (!B) return 0; if (int e = endTraining(*B)) return e; return uploadNetwork(*B, outputs == 1 ? B->critic : B->policy); }
int locomotionBatchStdChanged() { if (!B) return 0; if (int e = endTraining(*B)) return e; return uploadActionStd(*B); }
