// locomotion_shared.h — the ragdoll RL environment's model, shared by the single environment (locomotion_env.cpp, g++) and the
// batched one (locomotion_batch.hip, hipcc): the ragdoll builder (ragdoll.cpp:10-158), the action limits (learned_locomotion.cpp:
// 365-385), the random numbers (core/random.h), and the formulas of resetTraining / getState / getReward (:36-44, 135-152,
// 300-357).  The formulas are LOCO_HD: host + device under hipcc, host only under g++, so both paths evaluate the same source.
// Everything sits in an unnamed namespace: each translation unit keeps its own copy, compiled by its own compiler.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "mi_physics.h"

#ifdef __HIPCC__
#define LOCO_HD __host__ __device__ inline
#else
#define LOCO_HD inline
#endif

namespace
{
	struct vec3 { float x, y, z; };
	struct quat { float x, y, z, w; };
	LOCO_HD vec3 v3(float x, float y, float z) { return { x, y, z }; }
	LOCO_HD vec3 operator+(vec3 a, vec3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
	LOCO_HD vec3 operator-(vec3 a, vec3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
	LOCO_HD vec3 operator*(vec3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
	LOCO_HD vec3 operator*(float s, vec3 a) { return a * s; }
	LOCO_HD float dot(vec3 a, vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
	LOCO_HD vec3 cross(vec3 a, vec3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
	LOCO_HD float length(vec3 a) { return sqrtf(dot(a, a)); }
	LOCO_HD vec3 normalize(vec3 a) { return a * (1.f / length(a)); }
	LOCO_HD quat conjugate(quat q) { return { -q.x, -q.y, -q.z, q.w }; }
	LOCO_HD quat operator*(quat a, quat b) // core/math.cpp quat product
	{
		return { a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
			a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z };
	}
	LOCO_HD vec3 operator*(quat q, vec3 v) { quat p = { v.x, v.y, v.z, 0.f }; quat r = q * p * conjugate(q); return { r.x, r.y, r.z }; }
	inline quat axisAngle(vec3 axis, float angle) { float h = angle * 0.5f, s = sinf(h); return { axis.x * s, axis.y * s, axis.z * s, cosf(h) }; }
	inline float deg2rad(float d) { return d * (3.14159265358979323846f / 180.f); }
	LOCO_HD float lerpf(float a, float b, float t) { return a + t * (b - a); }
	LOCO_HD float clampf(float v, float l, float u) { return fminf(u, fmaxf(l, v)); }
	constexpr float PI = 3.14159265358979323846f;

	struct trs { quat rotation; vec3 position; };
	LOCO_HD vec3 transformPosition(const trs& m, vec3 p) { return m.rotation * p + m.position; }

	enum { NUM_BODY_PARTS = 14, NUM_CONE_TWIST = 7, NUM_HINGE = 6, ACTION_SIZE = NUM_CONE_TWIST * 3 + NUM_HINGE, STATE_SIZE = 13 * 3 + ACTION_SIZE };
	enum part { torso, head, leftUpperArm, leftLowerArm, rightUpperArm, rightLowerArm, leftUpperLeg, leftLowerLeg, leftFoot, leftToes, rightUpperLeg, rightLowerLeg, rightFoot, rightToes };
	constexpr int NO_PARENT = -1;
	LOCO_HD int parentOf(int i) // ragdoll.cpp:155-168
	{
		const int p[NUM_BODY_PARTS] = { NO_PARENT, torso, torso, leftUpperArm, torso, rightUpperArm, torso, leftUpperLeg, leftLowerLeg, leftFoot, torso, rightUpperLeg, rightLowerLeg, rightFoot };
		return p[i];
	}

	// byte-identical PODs (constraints.h:229-257, 346-380)
	struct hinge_pod { float a[12]; float minRotationLimit, maxRotationLimit, maxMotorTorque; uint32_t motorType; float motorTargetAngle; float t[9]; };
	struct cone_twist_pod { float a[21]; float swingLimit, twistLimit; uint32_t swingMotorType; float swingMotorTargetAngle, maxSwingMotorTorque, swingMotorAxis; uint32_t twistMotorType; float twistMotorTargetAngle, maxTwistMotorTorque; };
	static_assert(sizeof(hinge_pod) == 104 && sizeof(cone_twist_pod) == 120, "POD layout");
	static_assert(offsetof(hinge_pod, maxMotorTorque) == 14 * 4 && offsetof(cone_twist_pod, swingMotorType) == 23 * 4 && offsetof(cone_twist_pod, maxTwistMotorTorque) == 29 * 4, "motor words");

	struct rng64 // core/random.h:5-49
	{
		uint64_t state = 0x9E3779B97F4A7C15ull;
		LOCO_HD uint64_t u64() { uint64_t x = state; x ^= x << 13; x ^= x >> 7; x ^= x << 17; state = x; return x; }
		LOCO_HD uint32_t u32() { return (uint32_t)u64(); }
		LOCO_HD float f01() { return u32() / (float)UINT32_MAX; }
		LOCO_HD float between(float lo, float hi) { return lo + f01() * (hi - lo); }
		LOCO_HD uint32_t u32Between(uint32_t lo, uint32_t hi) { return u32() % (hi - lo) + lo; }
	};

	// applyAction (learned_locomotion.cpp:73-109): the action is smoothed (lerp, beta 0.1), the motors become position motors with
	// 200 N m and targets from the smoothed action: (twist, swing, swing axis) per cone-twist joint, then one angle per hinge.
	LOCO_HD void smoothAction(float* smoothed, const float* action) { for (int i = 0; i < ACTION_SIZE; ++i) smoothed[i] = lerpf(smoothed[i], action[i], 0.1f); }
	LOCO_HD void setConeTwistMotors(cone_twist_pod& c, const float* smoothed, int i)
	{
		c.maxSwingMotorTorque = 200.f; c.maxTwistMotorTorque = 200.f; c.swingMotorType = MI_MOTOR_POSITION; c.twistMotorType = MI_MOTOR_POSITION;
		c.twistMotorTargetAngle = smoothed[3 * i]; c.swingMotorTargetAngle = smoothed[3 * i + 1]; c.swingMotorAxis = smoothed[3 * i + 2];
	}
	LOCO_HD void setHingeMotors(hinge_pod& c, const float* smoothed, int i)
	{
		c.maxMotorTorque = 200.f; c.motorType = MI_MOTOR_POSITION; c.motorTargetAngle = smoothed[3 * NUM_CONE_TWIST + i];
	}

	// What getState / getReward read of one ragdoll: transform_component (the interpolated pose) and the velocities of its parts.
	struct ragdoll_view
	{
		trs transform[NUM_BODY_PARTS]; vec3 linearVelocity[NUM_BODY_PARTS], angularVelocity[NUM_BODY_PARTS];
	};
	struct target { vec3 positions[6], velocities[6]; quat localRotation; };
	// What resetTraining fixes for an episode.
	struct training
	{
		vec3 localPositions[NUM_BODY_PARTS][6];
		target targets[NUM_BODY_PARTS];
		vec3 localCOG[NUM_BODY_PARTS];
		float headTargetHeight;
		vec3 torsoVelocityTarget;
	};

	LOCO_HD vec3 globalCOG(const ragdoll_view& v, const training& t, int i) { return v.transform[i].position + v.transform[i].rotation * t.localCOG[i]; } // rigid_body.cpp:83-86
	LOCO_HD vec3 pointVelocity(const ragdoll_view& v, const training& t, int i, vec3 localP) { return v.linearVelocity[i] + cross(v.angularVelocity[i], transformPosition(v.transform[i], localP) - globalCOG(v, t, i)); } // :88-93
	LOCO_HD quat localRotation(const ragdoll_view& v, int i) { quat parentRotation = parentOf(i) == NO_PARENT ? quat{ 0.f, 0.f, 0.f, 1.f } : v.transform[parentOf(i)].rotation; return v.transform[i].rotation * conjugate(parentRotation); }
	LOCO_HD vec3 frameOrigin(const ragdoll_view& v, const training& t) { vec3 c = globalCOG(v, t, torso); c.y = 0.f; return c; } // getCoordinateSystem (:111-122): torso COG on the ground, identity rotation

	// training_locomotion::reset (:300-311) + learned_locomotion::reset (:36-44), except the zero action, which the caller applies.
	// boxMin / boxMax: the local AABB of each part's colliders (:199-246).  t.localCOG must be filled.
	LOCO_HD void resetTargets(const ragdoll_view& v, const vec3* boxMin, const vec3* boxMax, training& t)
	{
		for (int i = 0; i < NUM_BODY_PARTS; ++i)
		{
			vec3 c = (boxMin[i] + boxMax[i]) * 0.5f, r = (boxMax[i] - boxMin[i]) * 0.5f;
			vec3* p = t.localPositions[i];
			p[0] = c - v3(r.x, 0.f, 0.f); p[1] = c - v3(0.f, r.y, 0.f); p[2] = c - v3(0.f, 0.f, r.z); p[3] = c + v3(r.x, 0.f, 0.f); p[4] = c + v3(0.f, r.y, 0.f); p[5] = c + v3(0.f, 0.f, r.z);
			for (int k = 0; k < 6; ++k) { t.targets[i].positions[k] = transformPosition(v.transform[i], p[k]); t.targets[i].velocities[k] = pointVelocity(v, t, i, p[k]); }
			t.targets[i].localRotation = localRotation(v, i);
		}
		t.headTargetHeight = v.transform[head].position.y;
		t.torsoVelocityTarget = v3(0.f, 0.f, 0.f);
	}

	LOCO_HD void getState(const ragdoll_view& v, const training& t, const float* smoothed, float* out) // :135-152; field order of learning_state (learned_locomotion.h:42-68)
	{
		vec3 o = frameOrigin(v, t);
		auto put = [&](int slot, vec3 a) { out[3 * slot] = a.x; out[3 * slot + 1] = a.y; out[3 * slot + 2] = a.z; };
		put(0, v.linearVelocity[torso]);
		put(1, globalCOG(v, t, leftToes) - o); put(2, v.linearVelocity[leftToes]);
		put(3, globalCOG(v, t, rightToes) - o); put(4, v.linearVelocity[rightToes]);
		put(5, globalCOG(v, t, torso) - o); put(6, v.linearVelocity[torso]);
		put(7, globalCOG(v, t, head) - o); put(8, v.linearVelocity[head]);
		put(9, globalCOG(v, t, leftLowerArm) - o); put(10, v.linearVelocity[leftLowerArm]);
		put(11, globalCOG(v, t, rightLowerArm) - o); put(12, v.linearVelocity[rightLowerArm]);
		for (int i = 0; i < ACTION_SIZE; ++i) out[39 + i] = smoothed[i];
	}
	LOCO_HD bool hasFallen(const float* state) { return state[3 * 7 + 1] < 1.f; } // headPosition.y < 1 (:154-157)

	LOCO_HD float getReward(const ragdoll_view& v, const training& t) // :325-357
	{
		float positionError = 0.f, velocityError = 0.f, rotationError = 0.f;
		for (int i = 0; i < NUM_BODY_PARTS; ++i)
		{
			for (int k = 0; k < 6; ++k)
			{
				positionError += length(transformPosition(v.transform[i], t.localPositions[i][k]) - t.targets[i].positions[k]);
				velocityError += length(pointVelocity(v, t, i, t.localPositions[i][k]) - t.targets[i].velocities[k]);
			}
			quat d = t.targets[i].localRotation * conjugate(localRotation(v, i));
			rotationError += 2.f * acosf(clampf(d.w, -1.f, 1.f));
		}
		float vcmError = length(v.linearVelocity[torso] - t.torsoVelocityTarget);
		float rp = expf(-10.f / NUM_BODY_PARTS * positionError), rv = expf(-1.f / NUM_BODY_PARTS * velocityError);
		float rlocal = expf(-10.f / NUM_BODY_PARTS * rotationError), rvcm = expf(-vcmError);
		float fall = clampf(1.3f - 1.4f * (t.headTargetHeight - v.transform[head].position.y), 0.f, 1.f);
		return fall * (rp + rv + rlocal + rvcm);
	}

	struct ragdoll
	{
		uint32_t body[NUM_BODY_PARTS];
		uint32_t coneTwist[NUM_CONE_TWIST], hinge[NUM_HINGE];
		vec3 boxMin[NUM_BODY_PARTS], boxMax[NUM_BODY_PARTS]; // local AABB of each part's colliders (learned_locomotion.cpp:199-246)
	};

	inline void grow(vec3& mn, vec3& mx, vec3 p) { mn = { fminf(mn.x, p.x), fminf(mn.y, p.y), fminf(mn.z, p.z) }; mx = { fmaxf(mx.x, p.x), fmaxf(mx.y, p.y), fmaxf(mx.z, p.z) }; }

	// humanoid_ragdoll::initialize — ragdoll.cpp:10-133.  Bodies are created in the un-placed pose, the joints from global points
	// in that pose (local anchors do not care about the later placement), then every part is rotated about the hip and moved.
	inline ragdoll createRagdoll(mi_world* w, vec3 hip, float initialRotation)
	{
		const float scale = 0.42f;
		mi_material material = { 0.2f, 1.f, 985.f };
		const vec3 Z = v3(0.f, 0.f, 1.f);
		const quat I = { 0.f, 0.f, 0.f, 1.f };
		trs t[NUM_BODY_PARTS] = {
			{ I, scale * v3(0.f, 0.f, 0.f) }, { I, scale * v3(0.f, 1.45f, 0.f) },
			{ axisAngle(Z, deg2rad(-30.f)), scale * v3(-0.6f, 0.75f, 0.f) }, { axisAngle(Z, deg2rad(-20.f)), scale * v3(-0.884f, 0.044f, -0.043f) },
			{ axisAngle(Z, deg2rad(30.f)), scale * v3(0.6f, 0.75f, 0.f) }, { axisAngle(Z, deg2rad(20.f)), scale * v3(0.884f, 0.044f, -0.043f) },
			{ axisAngle(Z, deg2rad(-10.f)), scale * v3(-0.371f, -0.812f, 0.f) }, { axisAngle(Z, deg2rad(-3.5f)), scale * v3(-0.452f, -1.955f, 0.f) },
			{ I, scale * v3(-0.498f, -2.585f, -0.18f) }, { I, scale * v3(-0.498f, -2.585f, -0.637f) },
			{ axisAngle(Z, deg2rad(10.f)), scale * v3(0.371f, -0.812f, 0.f) }, { axisAngle(Z, deg2rad(3.5f)), scale * v3(0.452f, -1.955f, 0.f) },
			{ I, scale * v3(0.498f, -2.585f, -0.18f) }, { I, scale * v3(0.498f, -2.585f, -0.637f) } };
		ragdoll r;
		for (int i = 0; i < NUM_BODY_PARTS; ++i)
		{
			r.body[i] = mi_add_body(w, 0, 1.f, 0.4f, 0.4f, &t[i].position.x, &t[i].rotation.x);
			r.boxMin[i] = v3(FLT_MAX, FLT_MAX, FLT_MAX); r.boxMax[i] = v3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
		}
		auto capsule = [&](int p, vec3 a, vec3 b, float radius)
		{
			float s[7] = { scale * a.x, scale * a.y, scale * a.z, scale * b.x, scale * b.y, scale * b.z, scale * radius };
			mi_add_collider(w, r.body[p], MI_COLLIDER_CAPSULE, s, &material);
			vec3 r3 = v3(s[6], s[6], s[6]), A = v3(s[0], s[1], s[2]), B = v3(s[3], s[4], s[5]);
			grow(r.boxMin[p], r.boxMax[p], A + r3); grow(r.boxMin[p], r.boxMax[p], A - r3); grow(r.boxMin[p], r.boxMax[p], B + r3); grow(r.boxMin[p], r.boxMax[p], B - r3);
		};
		auto box = [&](int p, vec3 radius)
		{
			float s[6] = { -scale * radius.x, -scale * radius.y, -scale * radius.z, scale * radius.x, scale * radius.y, scale * radius.z };
			mi_add_collider(w, r.body[p], MI_COLLIDER_AABB, s, &material);
			grow(r.boxMin[p], r.boxMax[p], v3(s[0], s[1], s[2])); grow(r.boxMin[p], r.boxMax[p], v3(s[3], s[4], s[5]));
		};
		capsule(torso, v3(-0.2f, 0.f, 0.f), v3(0.2f, 0.f, 0.f), 0.25f); capsule(torso, v3(-0.16f, 0.32f, 0.f), v3(0.16f, 0.32f, 0.f), 0.2f);
		capsule(torso, v3(-0.14f, 0.62f, 0.f), v3(0.14f, 0.62f, 0.f), 0.22f); capsule(torso, v3(-0.14f, 0.92f, 0.f), v3(0.14f, 0.92f, 0.f), 0.2f);
		capsule(head, v3(0.f, -0.075f, 0.f), v3(0.f, 0.075f, 0.f), 0.25f);
		for (int p : { leftUpperArm, leftLowerArm, rightUpperArm, rightLowerArm }) capsule(p, v3(0.f, -0.2f, 0.f), v3(0.f, 0.2f, 0.f), 0.15f);
		capsule(leftUpperLeg, v3(0.f, -0.3f, 0.f), v3(0.f, 0.3f, 0.f), 0.25f); capsule(leftLowerLeg, v3(0.f, -0.3f, 0.f), v3(0.f, 0.3f, 0.f), 0.18f);
		box(leftFoot, v3(0.1587f, 0.1f, 0.3424f)); capsule(leftToes, v3(-0.0587f, 0.f, 0.f), v3(0.0587f, 0.f, 0.f), 0.1f);
		capsule(rightUpperLeg, v3(0.f, -0.3f, 0.f), v3(0.f, 0.3f, 0.f), 0.25f); capsule(rightLowerLeg, v3(0.f, -0.3f, 0.f), v3(0.f, 0.3f, 0.f), 0.18f);
		box(rightFoot, v3(0.1587f, 0.1f, 0.3424f)); capsule(rightToes, v3(-0.0587f, 0.f, 0.f), v3(0.0587f, 0.f, 0.f), 0.1f);

		auto tp = [&](int p, vec3 local) { return transformPosition(t[p], scale * local); };
		auto td = [&](int p, vec3 d) { return t[p].rotation * d; };
		auto coneTwistJ = [&](int a, int b, vec3 anchor, vec3 axis, float swing, float twist) { return mi_add_cone_twist_constraint_global(w, r.body[a], r.body[b], &anchor.x, &axis.x, swing, twist); };
		auto hingeJ = [&](int a, int b, vec3 anchor, vec3 axis, float mn, float mx) { return mi_add_hinge_constraint_global(w, r.body[a], r.body[b], &anchor.x, &axis.x, mn, mx); };
		// per-type ids follow the add order; the reference's handle arrays (ragdoll.h:60-83) are in exactly this order
		uint32_t neck = coneTwistJ(torso, head, tp(torso, v3(0.f, 1.2f, 0.f)), v3(0.f, 1.f, 0.f), deg2rad(50.f), deg2rad(90.f));
		uint32_t lShoulder = coneTwistJ(torso, leftUpperArm, tp(torso, v3(-0.4f, 1.f, 0.f)), v3(-1.f, 0.f, 0.f), deg2rad(130.f), deg2rad(90.f));
		uint32_t lElbow = hingeJ(leftUpperArm, leftLowerArm, tp(leftUpperArm, v3(0.f, -0.42f, 0.f)), normalize(v3(1.f, 0.f, 1.f)), deg2rad(-5.f), deg2rad(85.f));
		uint32_t rShoulder = coneTwistJ(torso, rightUpperArm, tp(torso, v3(0.4f, 1.f, 0.f)), v3(1.f, 0.f, 0.f), deg2rad(130.f), deg2rad(90.f));
		uint32_t rElbow = hingeJ(rightUpperArm, rightLowerArm, tp(rightUpperArm, v3(0.f, -0.42f, 0.f)), normalize(v3(1.f, 0.f, -1.f)), deg2rad(-5.f), deg2rad(85.f));
		uint32_t lHip = coneTwistJ(torso, leftUpperLeg, tp(torso, v3(-0.3f, -0.25f, 0.f)), td(leftUpperLeg, v3(0.f, -1.f, 0.f)), -1.f, deg2rad(30.f));
		uint32_t lKnee = hingeJ(leftUpperLeg, leftLowerLeg, tp(leftUpperLeg, v3(0.f, -0.6f, 0.f)), v3(1.f, 0.f, 0.f), deg2rad(-90.f), deg2rad(5.f));
		uint32_t lAnkle = coneTwistJ(leftLowerLeg, leftFoot, tp(leftLowerLeg, v3(0.f, -0.52f, 0.f)), td(leftLowerLeg, v3(0.f, -1.f, 0.f)), deg2rad(75.f), deg2rad(20.f));
		uint32_t lToes = hingeJ(leftFoot, leftToes, tp(leftFoot, v3(0.f, 0.f, -0.36f)), v3(1.f, 0.f, 0.f), deg2rad(-45.f), deg2rad(45.f));
		uint32_t rHip = coneTwistJ(torso, rightUpperLeg, tp(torso, v3(0.3f, -0.25f, 0.f)), td(rightUpperLeg, v3(0.f, -1.f, 0.f)), -1.f, deg2rad(30.f));
		uint32_t rKnee = hingeJ(rightUpperLeg, rightLowerLeg, tp(rightUpperLeg, v3(0.f, -0.6f, 0.f)), v3(1.f, 0.f, 0.f), deg2rad(-90.f), deg2rad(5.f));
		uint32_t rAnkle = coneTwistJ(rightLowerLeg, rightFoot, tp(rightLowerLeg, v3(0.f, -0.52f, 0.f)), td(rightLowerLeg, v3(0.f, -1.f, 0.f)), deg2rad(75.f), deg2rad(20.f));
		uint32_t rToes = hingeJ(rightFoot, rightToes, tp(rightFoot, v3(0.f, 0.f, -0.36f)), v3(1.f, 0.f, 0.f), deg2rad(-45.f), deg2rad(45.f));
		const uint32_t ct[NUM_CONE_TWIST] = { neck, lShoulder, rShoulder, lHip, lAnkle, rHip, rAnkle };
		const uint32_t hg[NUM_HINGE] = { lElbow, rElbow, lKnee, lToes, rKnee, rToes };
		memcpy(r.coneTwist, ct, sizeof(ct)); memcpy(r.hinge, hg, sizeof(hg));

		quat rotation = axisAngle(v3(0.f, 1.f, 0.f), initialRotation);
		for (int i = 0; i < NUM_BODY_PARTS; ++i) // ragdoll.cpp:125-133
		{
			quat q = rotation * t[i].rotation;
			vec3 p = rotation * t[i].position + hip;
			mi_set_transform(w, r.body[i], &p.x, &q.x);
		}
		return r;
	}

	inline void fillRanges(mi_world* w, const ragdoll& r, float* actionMin, float* actionMax) // getLimits (:365-385)
	{
		int k = 0;
		for (int i = 0; i < NUM_CONE_TWIST; ++i)
		{
			cone_twist_pod c; mi_constraint_get(w, MI_CONSTRAINT_CONE_TWIST, r.coneTwist[i], &c);
			actionMin[k] = c.twistLimit >= 0.f ? -c.twistLimit : -PI; actionMax[k++] = c.twistLimit >= 0.f ? c.twistLimit : PI;
			actionMin[k] = c.swingLimit >= 0.f ? -c.swingLimit : -PI; actionMax[k++] = c.swingLimit >= 0.f ? c.swingLimit : PI;
			actionMin[k] = -PI; actionMax[k++] = PI;
		}
		for (int i = 0; i < NUM_HINGE; ++i)
		{
			hinge_pod c; mi_constraint_get(w, MI_CONSTRAINT_HINGE, r.hinge[i], &c);
			actionMin[k] = c.minRotationLimit <= 0.f ? c.minRotationLimit : -PI; actionMax[k++] = c.maxRotationLimit >= 0.f ? c.maxRotationLimit : PI;
		}
	}

	// The ground of resetPhysics (learned_locomotion.cpp:435-461): a static box with its top at y = 0, ±halfExtent in x and z.
	inline void addGround(mi_world* w, float halfExtent)
	{
		mi_material ground = { 0.1f, 1.f, 4.f };
		float box[6] = { -halfExtent, -4.f, -halfExtent, halfExtent, 4.f, halfExtent }, pos[3] = { 0.f, -4.f, 0.f }, rot[4] = { 0.f, 0.f, 0.f, 1.f };
		mi_add_static_collider(w, MI_COLLIDER_AABB, box, &ground, pos, rot);
	}
}

__attribute__((visibility("hidden"))) uint64_t locomotionSeed(); // the seed of setPhysicsSeed (locomotion_env.cpp), for the batched environments
