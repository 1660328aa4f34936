// locomotion_batch.hip — N ragdoll environments of locomotion_env.cpp in ONE world, driven on the device: the motor targets go
// straight into the joint PODs (mi_joint_device_pods), the random pushes are one batched ray test (mi_test_physics_interaction_batch),
// and state, reward and fallen come out of one gather kernel.  Per update: one copy in, four kernels + mi_step, one copy out;
// no per-joint host call, no host ray test, no full-state copy.
//
// Environment e owns bodies 14e .. 14e+13 (its ragdoll, hips at (x_e, 1.25, z_e) on a square grid of pitch 8 m) over one ground box.
// Each environment restates the single one: the same builder, the same smoothing and motors, the same push draws from its own
// xorshift64 (seed ^ e * 0x9E3779B97F4A7C15; env 0 draws what the single environment draws), the same step settings, the same
// state and reward formulas (locomotion_shared.h), read from the interpolated pose as the single environment reads it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#include "locomotion_shared.h"

namespace
{
	constexpr uint32_t NUM_MOTOR_JOINTS = NUM_CONE_TWIST + NUM_HINGE;
	constexpr float GRID_PITCH = 8.f;

	// Per environment, fixed at resetPhysicsBatch: the spawn pose of every part (pose layout of the world: {pos, 0}, {quat}) and the
	// training targets of resetTraining.
	struct env_init { float4 spawn[2 * NUM_BODY_PARTS]; training train; };

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
		void* pods[2] = { nullptr, nullptr }; // cone-twist, hinge
		uint32_t generation[2] = { ~0u, ~0u };
	};
	batch* B = nullptr;

	bool ok(hipError_t e, const char* what) { if (e != hipSuccess) { fprintf(stderr, "locomotion batch: %s: %s\n", what, hipGetErrorString(e)); return false; } return true; }

	void release(batch* b)
	{
		if (!b) return;
		if (b->stream) (void)hipStreamSynchronize(b->stream);
		void* bufs[] = { b->dInit, b->dSmoothed, b->dRng, b->dRays, b->dPushes, b->dSlots, b->dActions, b->dStates, b->dRewards, b->dFallen, b->dIds };
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

	__device__ void writeMotors(uint32_t e, const float* smoothed, const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods)
	{
		for (int i = 0; i < NUM_CONE_TWIST; ++i) setConeTwistMotors(*(cone_twist_pod*)(conePods + (size_t)slots[NUM_MOTOR_JOINTS * e + i] * sizeof(cone_twist_pod)), smoothed, i);
		for (int i = 0; i < NUM_HINGE; ++i) setHingeMotors(*(hinge_pod*)(hingePods + (size_t)slots[NUM_MOTOR_JOINTS * e + NUM_CONE_TWIST + i] * sizeof(hinge_pod)), smoothed, i);
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
	__global__ void __launch_bounds__(64) k_loco_gather(uint32_t count, const uint32_t* __restrict__ ids, const env_init* __restrict__ init, const float* __restrict__ smoothedAll,
		const float4* __restrict__ poseLerp, const float4* __restrict__ vel, float* __restrict__ states, float* __restrict__ rewards, int32_t* __restrict__ fallen)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= count) return;
		const uint32_t e = ids ? ids[i] : i;
		ragdoll_view v;
		loadView(v, poseLerp, vel, NUM_BODY_PARTS * e);
		const training& t = init[e].train;
		float* out = states + (size_t)STATE_SIZE * e;
		getState(v, t, smoothedAll + (size_t)ACTION_SIZE * e, out);
		const bool failure = hasFallen(out);
		rewards[e] = failure ? 0.f : getReward(v, t);
		fallen[e] = failure ? 1 : 0;
	}

	// Reset of the listed environments: spawn pose into the three pose copies, velocities and accumulators zeroed (vel.w = invMass
	// kept), smoothed action zeroed and applied (resetTraining's applyAction(zero)).
	__global__ void __launch_bounds__(64) k_loco_reset(uint32_t count, const uint32_t* __restrict__ ids, const env_init* __restrict__ init, float* __restrict__ smoothedAll,
		const uint32_t* __restrict__ slots, uint8_t* conePods, uint8_t* hingePods, float4* pose, float4* pose0, float4* poseLerp, float4* vel, float4* force)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= count) return;
		const uint32_t e = ids[i];
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

	int launchReset(batch& b, const uint32_t* dIds, uint32_t count)
	{
		if (int e = refreshPods(b)) return e;
		hipLaunchKernelGGL(k_loco_reset, blocks(count), dim3(64), 0, b.stream, count, dIds, b.dInit, b.dSmoothed, b.dSlots, (uint8_t*)b.pods[0], (uint8_t*)b.pods[1],
			(float4*)b.ds.pose, (float4*)b.ds.pose0, (float4*)b.ds.poseLerp, (float4*)b.ds.vel, (float4*)b.ds.force);
		return ok(hipGetLastError(), "reset kernel") ? 0 : MI_ERR_HIP;
	}

	int launchGather(batch& b, const uint32_t* dIds, uint32_t count, float* dStates, float* dRewards, int32_t* dFallen)
	{
		hipLaunchKernelGGL(k_loco_gather, blocks(count), dim3(64), 0, b.stream, count, dIds, b.dInit, b.dSmoothed, (const float4*)b.ds.poseLerp, (const float4*)b.ds.vel, dStates, dRewards, dFallen);
		return ok(hipGetLastError(), "gather kernel") ? 0 : MI_ERR_HIP;
	}

	// One update of every environment, reading dActions, writing the three outputs (device pointers), all on the world's stream.
	int launchUpdate(batch& b, const float* dActions, float* dStates, float* dRewards, int32_t* dFallen)
	{
		if (int e = refreshPods(b)) return e;
		hipLaunchKernelGGL(k_loco_actions, blocks(b.n), dim3(64), 0, b.stream, b.n, dActions, b.dSmoothed, b.dSlots, (uint8_t*)b.pods[0], (uint8_t*)b.pods[1]);
		hipLaunchKernelGGL(k_loco_push_rays, blocks(b.n), dim3(64), 0, b.stream, b.n, b.dRng, (const float4*)b.ds.poseLerp, (float4*)b.dRays);
		if (!ok(hipGetLastError(), "action / push kernels")) return MI_ERR_HIP;
		if (int e = mi_test_physics_interaction_batch(b.world, b.n, 0, NUM_BODY_PARTS, b.dRays, b.dPushes)) return e;
		mi_physics_settings s = { 1, 60, 4, 30, 0, 1, 0, 1, 1, 1 };
		float timer = 0.f;
		if (int e = mi_step(b.world, &timer, &s, 1.f / 60.f)) return e;
		return launchGather(b, nullptr, b.n, dStates, dRewards, dFallen);
	}

	int copyOut(batch& b, float* outStates, float* outRewards, int32_t* outFallen)
	{
		if (outStates && !ok(hipMemcpyAsync(outStates, b.dStates, sizeof(float) * STATE_SIZE * b.n, hipMemcpyDeviceToHost, b.stream), "states")) return MI_ERR_HIP;
		if (outRewards && !ok(hipMemcpyAsync(outRewards, b.dRewards, sizeof(float) * b.n, hipMemcpyDeviceToHost, b.stream), "rewards")) return MI_ERR_HIP;
		if (outFallen && !ok(hipMemcpyAsync(outFallen, b.dFallen, sizeof(int32_t) * b.n, hipMemcpyDeviceToHost, b.stream), "fallen")) return MI_ERR_HIP;
		return ok(hipStreamSynchronize(b.stream), "copy out") ? 0 : MI_ERR_HIP;
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
			&& ok(hipMalloc(&b->dIds, sizeof(uint32_t) * n), "alloc");
		good = good && ok(hipMemcpyAsync(b->dInit, init.data(), sizeof(env_init) * n, hipMemcpyHostToDevice, b->stream), "init")
			&& ok(hipMemcpyAsync(b->dRng, rng.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, b->stream), "rng")
			&& ok(hipMemcpyAsync(b->dIds, ids.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, b->stream), "ids")
			&& ok(hipMemsetAsync(b->dPushes, 0, sizeof(int32_t) * n, b->stream), "pushes");
		if (!good) { release(b); return MI_ERR_HIP; }
		B = b;
		int e = launchReset(*b, b->dIds, numEnvs);
		if (!e) e = launchGather(*b, nullptr, numEnvs, b->dStates, b->dRewards, b->dFallen);
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
		if (int e = launchUpdate(b, b.dActions, b.dStates, b.dRewards, b.dFallen)) return -e;
		std::vector<int32_t> fallen(b.n);
		if (int e = copyOut(b, outStates, outRewards, fallen.data())) return -e;
		int count = 0;
		for (uint32_t i = 0; i < b.n; ++i) count += fallen[i] != 0;
		if (outFallen) memcpy(outFallen, fallen.data(), sizeof(int32_t) * b.n);
		return count;
	}

	// The same from device buffers, enqueued on the world's stream (getPhysicsBatchStream) without a host synchronisation.
	int updatePhysicsBatchDevice(const float* dActions, float* dStates, float* dRewards, int32_t* dFallen)
	{
		if (!B || !dActions || !dStates || !dRewards || !dFallen) return MI_ERR_INVALID_STATE;
		return launchUpdate(*B, dActions, dStates, dRewards, dFallen);
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
		if (!e) e = launchReset(b, dList, count);
		if (!e) e = launchGather(b, dList, count, b.dStates, b.dRewards, b.dFallen);
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
		if (int e = launchGather(*B, nullptr, B->n, B->dStates, B->dRewards, B->dFallen)) return e;
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
}
