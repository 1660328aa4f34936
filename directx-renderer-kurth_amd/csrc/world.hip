// World: life cycle, HBM buffer management, mass properties, and the upload / download of bodies, colliders and joints.
// The step is in step.hip, the snapshot in snapshot.hip, the C-ABI of include/mi_physics.h in api.hip / api_scene.hip; the host
// halves of cloth, force fields and events sit next to their kernels (k_cloth.hip, k_events.hip).
#include "world.h"
#include <cstdio>
#include <cstring>
#include <atomic>

thread_local std::string g_createError;
thread_local World* g_currentWorld = nullptr;

void mi_set_error(hipError_t e, const char* file, int line)
{
	char buf[512];
	snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
	if (g_currentWorld) { if (!g_currentWorld->lastError) { g_currentWorld->lastError = MI_ERR_HIP; g_currentWorld->lastErrorText = buf; } }
	else g_createError = buf;
}

template <typename T> void DevBuf<T>::ensure(size_t n, hipStream_t s, bool keep)
{
	if (n <= cap) return;
	size_t newCap = std::max(n, cap + cap / 2);
	T* np = nullptr;
	MI_CHECK(hipMalloc((void**)&np, newCap * sizeof(T)));
	if (!np) return; // allocation failed: the world's error is set (MI_CHECK), the old buffer and capacity stay as they were
	if (keep && p && cap) { MI_CHECK(hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s)); MI_CHECK(hipStreamSynchronize(s)); }
	if (p) MI_CHECK(hipFree(p));
	p = np; cap = newCap;
}

template struct DevBuf<float4>; template struct DevBuf<float2>; template struct DevBuf<uint2>; template struct DevBuf<uint4>; template struct DevBuf<u32>;
template struct DevBuf<double>; template struct DevBuf<u64>; template struct DevBuf<uint8_t>; template struct DevBuf<uint16_t>; template struct DevBuf<float>; template struct DevBuf<ColliderRec>; template struct DevBuf<ManifoldRec>;

World::World(int dev) : device(dev)
{
	g_currentWorld = this;
	MI_CHECK(hipSetDevice(dev));
	MI_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	if (const char* e = getenv("MI_NARROW_SIDE_STREAM")) narrowSideStream = atoi(e) != 0; // 0: the narrowphase's pair kernels stay on `stream`
	if (narrowSideStream)
	{
		MI_CHECK(hipStreamCreateWithFlags(&narrowStream, hipStreamNonBlocking));
		// (device-scope, like the stage events: both streams are this device's, nothing of the host's is ordered by them)
		MI_CHECK(hipEventCreateWithFlags(&narrowFork, hipEventDisableTiming | hipEventDisableSystemFence));
		MI_CHECK(hipEventCreateWithFlags(&narrowJoin, hipEventDisableTiming | hipEventDisableSystemFence));
		if (!narrowStream || !narrowFork || !narrowJoin) narrowSideStream = false; // (the world's error is set)
	}
	MI_CHECK(hipHostMalloc((void**)&hCounters, CTR_WORDS * sizeof(u32), hipHostMallocDefault));
	if (hCounters) memset(hCounters, 0, CTR_WORDS * sizeof(u32));
	dCounters.ensure(CTR_WORDS, stream);
	if (dCounters.p) MI_CHECK(hipMemsetAsync(dCounters.p, 0, CTR_WORDS * sizeof(u32), stream));
	timing.stageEvents.resize(STAGE_RING * 6);
	// (device-scope events: a stage's time stamp needs no system-scope fence, and the host reads the counters from pinned memory behind an event it waits for)
	for (auto& e : timing.stageEvents) MI_CHECK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
	MI_CHECK(hipEventCreateWithFlags(&countersEvent, hipEventDisableTiming));
	validate = getenv("MI_PHYSICS_VALIDATE") != nullptr;
	cluster.enabled = getenv("MI_PHYSICS_NO_CLUSTER") == nullptr;
	cluster.jointsEnabled = getenv("MI_CLUSTER_NO_JOINTS") == nullptr; // LDS cluster contact sweep (one launch) vs global colouring + one launch per colour
	if (const char* e = getenv("MI_FLOW_TEST_ABORT")) cluster.flowTestAbortStep = (u32)atoi(e); // tests: make the cluster sweep of that internal step give up
	if (const char* e = getenv("MI_CLUSTER_TASK")) { cluster.taskWeight = 64u * (u32)std::max(16, atoi(e)); cluster.taskWeightLater = std::min(cluster.taskWeight, cluster.taskWeightLater); cluster.taskWeightComp = std::min(cluster.taskWeight, cluster.taskWeightComp); }  // manifolds per task
	if (getenv("MI_PHYSICS_REPLAY")) replay.referenceOrder = true;
	if (const char* e = getenv("MI_CLUSTER_BLOCKS")) cluster.blocksLimit = (u32)std::max(1, atoi(e));
	if (const char* e = getenv("MI_CLUSTER_REG_CONTACTS")) cluster.regContactsCap = (u32)std::max(0, atoi(e)); // tests: rows beyond it live in LDS / the scratch
	if (const char* e = getenv("MI_CLUSTER_LDS_ROWS")) cluster.ldsRowsCap = (u32)std::max(0, atoi(e)); // tests: a workgroup's rows beyond it live in the scratch
	if (const char* e = getenv("MI_CLUSTER_TASK_LATER")) cluster.taskWeightLater = 64u * (u32)std::max(16, atoi(e)); // ... of the phases after the first
	if (const char* e = getenv("MI_CLUSTER_TASK_COMP")) cluster.taskWeightComp = 64u * (u32)std::min(1 << 20, std::max(16, atoi(e))); // ... of the component phase (dealing its components otherwise changes no result)
	if (const char* e = getenv("MI_CLUSTER_COLOR_NARROW_MAX")) cluster.colorNarrowMax = (u32)std::max(0, atoi(e)); // tasks of more items are coloured by the wide instance (0: all of them)
	if (const char* e = getenv("MI_CLUSTER_COLOR_BLOCKS")) cluster.colorBlocksLimit = (u32)std::max(1, atoi(e)); // tests: a small narrow launch, whose workgroups colour several tasks in turn
	if (dCounters.p)
	{
		u32 box[6] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u }; // empty bounding box (k_cl_bbox accumulates, k_cl_offsets resets)
		MI_CHECK(hipMemcpyAsync(dCounters.p + CTR_CL_BBOX, box, sizeof(box), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipStreamSynchronize(stream));
	}
}

World::~World()
{
	g_currentWorld = this;
	if (narrowStream) (void)hipStreamSynchronize(narrowStream);
	if (stream) (void)hipStreamSynchronize(stream);
	for (auto& e : timing.stageEvents) if (e) (void)hipEventDestroy(e);
	if (countersEvent) (void)hipEventDestroy(countersEvent);
	if (hCounters) (void)hipHostFree(hCounters);
	if (narrowFork) (void)hipEventDestroy(narrowFork);
	if (narrowJoin) (void)hipEventDestroy(narrowJoin);
	if (narrowStream) (void)hipStreamDestroy(narrowStream);
	if (stream) (void)hipStreamDestroy(stream);
	g_currentWorld = nullptr;
}

void World::fail(int code, const std::string& what) { if (!lastError) { lastError = code; lastErrorText = what; } }

// ---------------------------------------------------------------------------------------------------------------
// Mass properties on the host at add time — reference physics.cpp:1416-1519 (per collider) + rigid_body.cpp:29-81 (combine).
// ---------------------------------------------------------------------------------------------------------------
struct MassProps { M3 inertia; V3 cog; float mass; };

static M3 mzero() { M3 r; memset(&r, 0, sizeof(r)); return r; }
static M3 mscaleH(const M3& a, float s) { M3 r; const float* p = &a.m00; float* q = &r.m00; for (int i = 0; i < 9; ++i) q[i] = p[i] * s; return r; }
static M3 msub(const M3& a, const M3& b) { M3 r; const float* p = &a.m00; const float* q = &b.m00; float* o = &r.m00; for (int i = 0; i < 9; ++i) o[i] = p[i] - q[i]; return r; }
static M3 mouter(V3 a, V3 b) // outerProduct, math.cpp:778-795
{
	V3 c0 = a * b.x, c1 = a * b.y, c2 = a * b.z;
	M3 r; r.m00 = c0.x; r.m10 = c0.y; r.m20 = c0.z; r.m01 = c1.x; r.m11 = c1.y; r.m21 = c1.z; r.m02 = c2.x; r.m12 = c2.y; r.m22 = c2.z;
	return r;
}
static M3 minvert(const M3& m) // math.cpp:276-306
{
	M3 inv;
	inv.m00 = m.m11 * m.m22 - m.m21 * m.m12; inv.m01 = m.m02 * m.m21 - m.m22 * m.m01; inv.m02 = m.m01 * m.m12 - m.m11 * m.m02;
	inv.m10 = m.m12 * m.m20 - m.m22 * m.m10; inv.m11 = m.m00 * m.m22 - m.m20 * m.m02; inv.m12 = m.m02 * m.m10 - m.m12 * m.m00;
	inv.m20 = m.m10 * m.m21 - m.m20 * m.m11; inv.m21 = m.m01 * m.m20 - m.m21 * m.m00; inv.m22 = m.m00 * m.m11 - m.m10 * m.m01;
	float det = m.m00 * (m.m11 * m.m22 - m.m21 * m.m12) - m.m01 * (m.m10 * m.m22 - m.m20 * m.m12) + m.m02 * (m.m10 * m.m21 - m.m20 * m.m11);
	if (det == 0.f) return mzero();
	return mscaleH(inv, 1.f / det);
}

static MassProps colliderMassProps(const World::HCollider& c, const World& w)
{
	MassProps r; r.inertia = mzero(); r.cog = v3s(0.f); r.mass = 0.f;
	const float* s = c.shape;
	switch (c.type)
	{
		case MI_HULL: // physics.cpp:1520-1580: signed tetrahedra (origin, face) with the covariance of the unit tetrahedron
		{
			Q4 rot = q4(s[0], s[1], s[2], s[3]); V3 pos = v3(s[4], s[5], s[6]);
			const World::HHull& g = w.hulls[(u32)s[7]];
			const float s60 = 1.f / 60.f, s120 = 1.f / 120.f;
			M3 C; C.m00 = s60; C.m01 = s120; C.m02 = s120; C.m10 = s120; C.m11 = s60; C.m12 = s120; C.m20 = s120; C.m21 = s120; C.m22 = s60;
			float totalMass = 0.f; M3 totalCov = mzero(); V3 totalCOG = v3s(0.f);
			for (size_t f = 0; f + 2 < g.triangles.size(); f += 3)
			{
				const float* pa = &g.vertices[3 * g.triangles[f]]; const float* pb = &g.vertices[3 * g.triangles[f + 1]]; const float* pc = &g.vertices[3 * g.triangles[f + 2]];
				V3 w1 = pos + rot * v3(pa[0], pa[1], pa[2]), w2 = pos + rot * v3(pb[0], pb[1], pb[2]), w3 = pos + rot * v3(pc[0], pc[1], pc[2]);
				M3 A; A.m00 = w1.x; A.m01 = w2.x; A.m02 = w3.x; A.m10 = w1.y; A.m11 = w2.y; A.m12 = w3.y; A.m20 = w1.z; A.m21 = w2.z; A.m22 = w3.z;
				float detA = A.m00 * (A.m11 * A.m22 - A.m21 * A.m12) - A.m01 * (A.m10 * A.m22 - A.m20 * A.m12) + A.m02 * (A.m10 * A.m21 - A.m20 * A.m11);
				M3 cov = (mscaleH(A, detA) * C) * mtranspose(A);
				float volume = 1.f / 6.f * detA;
				V3 cg = (w1 + w2 + w3) * 0.25f;
				totalMass += volume;
				totalCov = madd(totalCov, cov);
				totalCOG += cg * volume;
			}
			totalCOG = totalCOG / totalMass;
			M3 Cp = msub(totalCov, mscaleH(mouter(totalCOG, totalCOG), totalMass));
			r.cog = totalCOG;
			r.mass = totalMass * c.density;
			r.inertia = mscaleH(msub(mscaleH(midentity(), Cp.m00 + Cp.m11 + Cp.m22), Cp), c.density);
		} break;
		case MI_SPHERE:
		{
			float radius = s[3];
			float sqRadiusPI = MI_PI * (radius * radius);
			r.mass = (4.f / 3.f * sqRadiusPI * radius) * c.density;
			r.cog = v3(s[0], s[1], s[2]);
			r.inertia = mscaleH(midentity(), 2.f / 5.f * r.mass * radius * radius);
		} break;
		case MI_CAPSULE:
		{
			V3 pA = v3(s[0], s[1], s[2]), pB = v3(s[3], s[4], s[5]); float radius = s[6];
			V3 axis = pA - pB;
			if (axis.y < 0.f) axis *= -1.f;
			float height = length(axis);
			axis *= (1.f / height);
			M3 rot = quaternionToMat3(rotateFromTo(v3(0.f, 1.f, 0.f), axis));
			float sqRadius = radius * radius;
			float sqRadiusPI = MI_PI * sqRadius;
			float volume = 4.f / 3.f * sqRadiusPI * radius + sqRadiusPI * length(pA - pB);
			r.mass = volume * c.density;
			r.cog = (pA + pB) * 0.5f;
			float cylinderMass = c.density * sqRadiusPI * height;
			float hemiSphereMass = c.density * 2.f / 3.f * sqRadiusPI * radius;
			float sqCapsuleHeight = height * height;
			M3 I = mzero();
			I.m11 = sqRadius * cylinderMass * 0.5f;
			I.m00 = I.m22 = I.m11 * 0.5f + cylinderMass * sqCapsuleHeight / 12.f;
			float temp0 = hemiSphereMass * 2.f * sqRadius / 5.f;
			I.m11 += temp0 * 2.f;
			float temp1 = height * 0.5f;
			float temp2 = temp0 + hemiSphereMass * (temp1 * temp1 + 3.f / 8.f * sqCapsuleHeight);
			I.m00 += temp2 * 2.f;
			I.m22 += temp2 * 2.f;
			r.inertia = mtranspose(rot) * I * rot;
		} break;
		case MI_CYLINDER: // physics.cpp:1466-1494
		{
			V3 pA = v3(s[0], s[1], s[2]), pB = v3(s[3], s[4], s[5]); float radius = s[6];
			V3 axis = pA - pB;
			if (axis.y < 0.f) axis *= -1.f;
			float height = length(axis);
			axis *= (1.f / height);
			M3 rot = quaternionToMat3(rotateFromTo(v3(0.f, 1.f, 0.f), axis));
			float sqRadiusPI = MI_PI * radius * radius;
			r.mass = (sqRadiusPI * length(pA - pB)) * c.density;
			r.cog = (pA + pB) * 0.5f;
			float sqRadius = radius * radius;
			float sqHeight = height * height;
			M3 I = mzero();
			I.m11 = sqRadius * r.mass * 0.5f;
			I.m00 = I.m22 = 1.f / 12.f * r.mass * (3.f * sqRadius + sqHeight);
			r.inertia = mtranspose(rot) * I * rot;
		} break;
		case MI_AABB:
		{
			V3 lo = v3(s[0], s[1], s[2]), hi = v3(s[3], s[4], s[5]);
			V3 d0 = hi - lo;
			r.mass = (d0.x * d0.y * d0.z) * c.density;
			r.cog = (lo + hi) * 0.5f;
			V3 d = ((hi - lo) * 0.5f) * 2.f;
			r.inertia.m00 = 1.f / 12.f * r.mass * (d.y * d.y + d.z * d.z);
			r.inertia.m11 = 1.f / 12.f * r.mass * (d.x * d.x + d.z * d.z);
			r.inertia.m22 = 1.f / 12.f * r.mass * (d.x * d.x + d.y * d.y);
		} break;
		case MI_OBB:
		{
			Q4 q = q4(s[0], s[1], s[2], s[3]); V3 radius = v3(s[7], s[8], s[9]);
			V3 d = radius * 2.f;
			r.mass = (d.x * d.y * d.z) * c.density;
			r.cog = v3(s[4], s[5], s[6]);
			M3 I = mzero();
			I.m00 = 1.f / 12.f * r.mass * (d.y * d.y + d.z * d.z);
			I.m11 = 1.f / 12.f * r.mass * (d.x * d.x + d.z * d.z);
			I.m22 = 1.f / 12.f * r.mass * (d.x * d.x + d.y * d.y);
			M3 rot = quaternionToMat3(q);
			r.inertia = mtranspose(rot) * I * rot;
		} break;
		default: break;
	}
	return r;
}

void recalculateProperties(World& w, World::HBody& rb) // rigid_body.cpp:29-81
{
	if (rb.invMass == 0.f) return;
	u32 n = (u32)rb.colliders.size();
	if (!n) return;
	std::vector<MassProps> props(n);
	for (u32 i = 0; i < n; ++i) props[i] = colliderMassProps(w.colliders[rb.colliders[n - 1 - i]], w); // newest first (scene.h:56-58)
	M3 inertia = mzero(); V3 cog = v3s(0.f); float mass = 0.f;
	for (u32 i = 0; i < n; ++i) { mass += props[i].mass; cog += props[i].cog * props[i].mass; }
	rb.invMass = 1.f / mass;
	cog = cog * rb.invMass;
	rb.localCOG[0] = cog.x; rb.localCOG[1] = cog.y; rb.localCOG[2] = cog.z;
	for (u32 i = 0; i < n; ++i)
	{
		V3 r = props[i].cog - cog;
		inertia = madd(inertia, madd(props[i].inertia, mscaleH(msub(mscaleH(midentity(), dot(r, r)), mouter(r, r)), props[i].mass)));
	}
	M3 inv = minvert(inertia);
	memcpy(rb.invInertia, &inv.m00, 36);
}

// ---------------------------------------------------------------------------------------------------------------
// Upload / download
// ---------------------------------------------------------------------------------------------------------------
void World::downloadState()
{
	if (!stateOnDevice || !nb) return;
	resolvePendingFlow();
	std::vector<float4> hp(2 * (size_t)nb), hv(2 * (size_t)nb), hf(2 * (size_t)nb);
	MI_CHECK(hipMemcpyAsync(hp.data(), pose.p, sizeof(float4) * hp.size(), hipMemcpyDeviceToHost, stream));
	MI_CHECK(hipMemcpyAsync(hv.data(), vel.p, sizeof(float4) * hv.size(), hipMemcpyDeviceToHost, stream));
	MI_CHECK(hipMemcpyAsync(hf.data(), force.p, sizeof(float4) * hf.size(), hipMemcpyDeviceToHost, stream));
	MI_CHECK(hipStreamSynchronize(stream));
	for (u32 i = 0; i < nb; ++i)
	{
		HBody& b = bodies[i];
		b.pos[0] = hp[2 * i].x; b.pos[1] = hp[2 * i].y; b.pos[2] = hp[2 * i].z;
		b.rot[0] = hp[2 * i + 1].x; b.rot[1] = hp[2 * i + 1].y; b.rot[2] = hp[2 * i + 1].z; b.rot[3] = hp[2 * i + 1].w;
		b.v[0] = hv[2 * i].x; b.v[1] = hv[2 * i].y; b.v[2] = hv[2 * i].z;
		b.w[0] = hv[2 * i + 1].x; b.w[1] = hv[2 * i + 1].y; b.w[2] = hv[2 * i + 1].z;
		b.force[0] = hf[2 * i].x; b.force[1] = hf[2 * i].y; b.force[2] = hf[2 * i].z;
		b.torque[0] = hf[2 * i + 1].x; b.torque[1] = hf[2 * i + 1].y; b.torque[2] = hf[2 * i + 1].z;
	}
}

void World::upload()
{
	if (!topologyDirty) return;
	pullJointPods();            // device-written motors survive the joint re-upload this forces
	queries.interactTablesValid = false;
	if (stateOnDevice) downloadState(); // bodies added mid-simulation: pull the live state first
	u32 newNb = (u32)bodies.size(), newNc = (u32)colliders.size();
	std::vector<float4> hp(2 * (size_t)newNb), hv(2 * ((size_t)newNb + 1)), hprops(5 * (size_t)newNb), hf(2 * (size_t)newNb);
	for (u32 i = 0; i < newNb; ++i)
	{
		const HBody& b = bodies[i];
		hp[2 * i] = make_float4(b.pos[0], b.pos[1], b.pos[2], 0.f);
		hp[2 * i + 1] = make_float4(b.rot[0], b.rot[1], b.rot[2], b.rot[3]);
		hv[2 * i] = make_float4(b.v[0], b.v[1], b.v[2], b.invMass);
		hv[2 * i + 1] = make_float4(b.w[0], b.w[1], b.w[2], 0.f);
		hprops[5 * i] = make_float4(b.localCOG[0], b.localCOG[1], b.localCOG[2], b.invMass);
		hprops[5 * i + 1] = make_float4(b.invInertia[0], b.invInertia[1], b.invInertia[2], 0.f);
		hprops[5 * i + 2] = make_float4(b.invInertia[3], b.invInertia[4], b.invInertia[5], 0.f);
		hprops[5 * i + 3] = make_float4(b.invInertia[6], b.invInertia[7], b.invInertia[8], 0.f);
		hprops[5 * i + 4] = make_float4(b.gravityFactor, b.linDamp, b.angDamp, 0.f);
		hf[2 * i] = make_float4(b.force[0], b.force[1], b.force[2], 0.f);
		hf[2 * i + 1] = make_float4(b.torque[0], b.torque[1], b.torque[2], 0.f);
	}
	hv[2 * (size_t)newNb] = make_float4(0.f, 0.f, 0.f, 0.f); hv[2 * (size_t)newNb + 1] = make_float4(0.f, 0.f, 0.f, 0.f);

	std::vector<ColliderRec> hc(newNc); std::vector<float4> hsp(2 * (size_t)newNc);
	for (u32 i = 0; i < newNc; ++i)
	{
		const HCollider& c = colliders[i];
		ColliderRec r;
		r.a = make_float4(c.shape[0], c.shape[1], c.shape[2], c.shape[3]);
		r.b = make_float4(c.shape[4], c.shape[5], c.shape[6], c.shape[7]);
		r.c = make_float4(c.shape[8], c.shape[9], c.restitution, c.friction);
		u32 body = (c.body == MI_STATIC_BODY) ? newNb : c.body;
		r.d = make_float4(mi_u2f(c.type), mi_u2f(body), c.density, mi_u2f(c.zoneType | (c.zoneIndex << 8))); // flags: force-field / trigger collider
		hc[i] = r;
		hsp[2 * i] = make_float4(c.spos[0], c.spos[1], c.spos[2], 0.f);
		hsp[2 * i + 1] = make_float4(c.srot[0], c.srot[1], c.srot[2], c.srot[3]);
	}

	std::vector<float4> hhv, hhi; // hull vertex pool + per-geometry info
	for (const HHull& g : hulls)
	{
		u32 first = (u32)hhv.size(), count = (u32)(g.vertices.size() / 3);
		for (u32 v = 0; v < count; ++v) hhv.push_back(make_float4(g.vertices[3 * v], g.vertices[3 * v + 1], g.vertices[3 * v + 2], 0.f));
		hhi.push_back(make_float4(g.aabbMin[0], g.aabbMin[1], g.aabbMin[2], mi_u2f(first)));
		hhi.push_back(make_float4(g.aabbMax[0], g.aabbMax[1], g.aabbMax[2], mi_u2f(count)));
	}
	hullVerts.ensure(std::max<size_t>(hhv.size(), 1), stream); hullInfo.ensure(std::max<size_t>(hhi.size(), 2), stream);
	if (!hhv.empty())
	{
		MI_CHECK(hipMemcpyAsync(hullVerts.p, hhv.data(), sizeof(float4) * hhv.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(hullInfo.p, hhi.data(), sizeof(float4) * hhi.size(), hipMemcpyHostToDevice, stream));
	}

	nb = newNb; nc = newNc;
	size_t nb1 = (size_t)nb + 1;
	pose.ensure(2 * nb1, stream); pose0.ensure(2 * nb1, stream); poseLerp.ensure(2 * nb1, stream); vel.ensure(2 * nb1, stream);
	bprops.ensure(5 * nb1, stream); force.ensure(2 * nb1, stream); cog.ensure(nb1, stream); invIw.ensure(3 * nb1, stream);
	bodyMask.ensure(nb1, stream); claim.ensure(2 * nb1, stream);
	simMask.ensure(nb1, stream); aliveMask.ensure(nb1, stream);
	{
		std::vector<uint8_t> alive(nb1, 1);
		for (u32 i = 0; i < newNb; ++i) if (bodies[i].removed) alive[i] = 0;
		MI_CHECK(hipMemcpyAsync(aliveMask.p, alive.data(), nb1, hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(simMask.p, alive.data(), nb1, hipMemcpyHostToDevice, stream));
		MI_CHECK(hipStreamSynchronize(stream)); // `alive` goes out of scope
	}
	zones.fieldsDirty = true; // (re)sizes the per-body field bits
	size_t ncap = std::max<size_t>(nc, 1);
	colLocal.ensure(ncap, stream); colWorld.ensure(ncap, stream); colStaticPose.ensure(2 * ncap, stream); aabbMin.ensure(ncap, stream); aabbMax.ensure(ncap, stream);
	hashKey.ensure(ncap, stream); sortIdx.ensure(ncap, stream);
	sBox.ensure(2 * ncap, stream); pairCount.ensure(ncap + 1, stream); pairOffset.ensure(ncap + 1, stream);
	hashTableSize = std::max(1024u, nextPow2(2 * nc));
	cellStart.ensure(2 * (size_t)hashTableSize, stream); cellCount.ensure(hashTableSize + 4, stream); cellBase.ensure(hashTableSize + 4, stream);

	if (nb)
	{
		MI_CHECK(hipMemcpyAsync(pose.p, hp.data(), sizeof(float4) * hp.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(pose0.p, hp.data(), sizeof(float4) * hp.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(poseLerp.p, hp.data(), sizeof(float4) * hp.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(bprops.p, hprops.data(), sizeof(float4) * hprops.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(force.p, hf.data(), sizeof(float4) * hf.size(), hipMemcpyHostToDevice, stream));
	}
	MI_CHECK(hipMemcpyAsync(vel.p, hv.data(), sizeof(float4) * hv.size(), hipMemcpyHostToDevice, stream));
	std::vector<u32> hcb(newNc);
	for (u32 i = 0; i < newNc; ++i) hcb[i] = (colliders[i].body == MI_STATIC_BODY) ? newNb : colliders[i].body;
	colBody.ensure(ncap, stream);
	if (nc)
	{
		MI_CHECK(hipMemcpyAsync(colLocal.p, hc.data(), sizeof(ColliderRec) * hc.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(colStaticPose.p, hsp.data(), sizeof(float4) * hsp.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(colBody.p, hcb.data(), sizeof(u32) * hcb.size(), hipMemcpyHostToDevice, stream));
	}
	activeDirty = true; estActiveBodies = nb; estActiveCols = nc; // (the lists are rebuilt at the next step; until the host has seen their lengths the launches are sized for everything)
	MI_CHECK(hipStreamSynchronize(stream));
	topologyDirty = false; stateOnDevice = true;
	jointsChanged(); // the static dummy index (= nb) moved
}

// Joint generations are drawn from one counter for all worlds, so a restored world never repeats a generation of its source.
static std::atomic<u32> g_jointGeneration{ 0 };
void World::jointsChanged() { jointsDirty = true; jointGeneration = ++g_jointGeneration; }

// Device copy -> host copy of every joint POD (mi_joint_device_pods).  Nothing to do while the joints are dirty: the last pull
// happened when they became dirty, and the host copy has changed since.
void World::pullJointPods()
{
	if (!jointPodsOnDevice || jointsDirty) return;
	for (u32 t = 0; t < MI_JOINT_TYPES; ++t)
	{
		JointSet& js = joints[t];
		const u32 m = (u32)js.order.size(), podSize = MI_JOINT_POD_SIZE[t];
		if (!m || !js.dPods.p) continue;
		std::vector<uint8_t> hp((size_t)m * podSize);
		MI_CHECK(hipMemcpyAsync(hp.data(), js.dPods.p, hp.size(), hipMemcpyDeviceToHost, stream));
		MI_CHECK(hipStreamSynchronize(stream));
		for (u32 slot = 0; slot < m; ++slot) memcpy(js.pods.data() + (size_t)js.order[slot] * podSize, hp.data() + (size_t)slot * podSize, podSize);
	}
}

// Greedy colouring of each joint type on the host (joints change rarely): joint i gets the lowest colour free at both bodies.
void World::uploadJoints()
{
	if (!jointsDirty) return;
	// Colours ACROSS the types: a joint's colour ("level") is the lowest one above every colour already given to a joint of either of its
	// bodies, the joints taken in the reference's solve order (type after type, constraints.cpp:3748-3772; inside a type in storage
	// order).  Joints of one level share no body, and along every body the levels rise in that solve order, so "level by level" is
	// the reference's sequence with commuting solves swapped — and joints of DIFFERENT types that share no body get the same level
	// (a ragdoll: 5 levels instead of 1 hinge + 5 cone-twist colours = 6 dependent steps per iteration).
	std::vector<u32> nextLevel(bodies.size() + 1, 0u);
	u32 numLevels = 0;
	for (u32 t = 0; t < MI_JOINT_TYPES; ++t)
	{
		JointSet& js = joints[t];
		u32 n = js.count(), podSize = MI_JOINT_POD_SIZE[t];
		std::vector<u32> color(n, 0xFFFFFFFFu);
		u32 numColors = 0;
		for (u32 i = 0; i < n; ++i)
		{
			if (!js.alive[i]) continue;
			const u32 a = std::min<u32>(js.a[i], (u32)bodies.size()), b = std::min<u32>(js.b[i], (u32)bodies.size());
			const u32 c = std::max(a < bodies.size() ? nextLevel[a] : 0u, b < bodies.size() ? nextLevel[b] : 0u);
			if (a < bodies.size()) nextLevel[a] = c + 1;
			if (b < bodies.size()) nextLevel[b] = c + 1;
			color[i] = c; numColors = std::max(numColors, c + 1);
		}
		numLevels = std::max(numLevels, numColors);
		js.order.clear(); js.colorStart.assign(1, 0);
		for (u32 c = 0; c < numColors; ++c)
		{
			for (u32 i = 0; i < n; ++i) if (color[i] == c) js.order.push_back(i);
			js.colorStart.push_back((u32)js.order.size());
		}
		u32 m = (u32)js.order.size();
		if (!m) continue;
		std::vector<uint8_t> hp((size_t)m * podSize); std::vector<uint2> hpr(m);
		for (u32 s = 0; s < m; ++s)
		{
			u32 i = js.order[s];
			memcpy(hp.data() + (size_t)s * podSize, js.pods.data() + (size_t)i * podSize, podSize);
			hpr[s] = make_uint2(js.a[i], js.b[i]);
		}
		js.dPods.ensure(hp.size(), stream); js.dPairs.ensure(m, stream); js.dUpdate.ensure((size_t)m * MI_JOINT_UPDATE_FLOATS[t], stream);
		MI_CHECK(hipMemcpyAsync(js.dPods.p, hp.data(), hp.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipMemcpyAsync(js.dPairs.p, hpr.data(), sizeof(uint2) * m, hipMemcpyHostToDevice, stream));
		MI_CHECK(hipStreamSynchronize(stream));
	}
	// Joints inside the cluster sweep: bodies connected by joints form an island that must live in ONE task (a joint is solved out of
	// the task's LDS like a contact, and joints come before contacts in every iteration: constraints.cpp:3748-3772), so every body
	// gets its island's representative (lowest body index), and the joints are listed once in (type, colour) order.
	{
		const u32 n = (u32)bodies.size();
		std::vector<u32> rep(n + 1);
		for (u32 i = 0; i <= n; ++i) rep[i] = i;
		auto find = [&](u32 x) { while (rep[x] != x) { rep[x] = rep[rep[x]]; x = rep[x]; } return x; };
		std::vector<uint4> table;
		const u32 numClasses = numLevels; // class = level: the sweep runs the levels one after the other, whatever the types of their joints
		for (u32 t = 0; t < MI_JOINT_TYPES; ++t)
		{
			JointSet& js = joints[t];
			for (size_t c = 0; c + 1 < js.colorStart.size(); ++c)
				for (u32 sidx = js.colorStart[c]; sidx < js.colorStart[c + 1]; ++sidx)
				{
					u32 i = js.order[sidx], a = js.a[i], b = js.b[i];
					table.push_back(make_uint4(t | ((u32)c << 8), sidx, a, b));
					u32 ra = find(a), rb = find(b);
					if (ra != rb) { if (ra < rb) rep[rb] = ra; else rep[ra] = rb; }
				}
		}
		for (u32 i = 0; i < n; ++i) rep[i] = find(i);
		cluster.numJoints = (u32)table.size(); cluster.numJointClasses = numClasses;
		cluster.jointsInCluster = cluster.numJoints > 0 && numClasses <= CL_MAX_JOINT_CLASSES;
		if (getenv("MI_CLUSTER_DEBUG")) fprintf(stderr, "[mi_physics] joints: %u in %u levels -> %s\n", cluster.numJoints, numClasses, cluster.jointsInCluster ? "inside the cluster sweep" : "own launches");
		std::vector<u32> jointBody(n + 1, 0u);
		for (const uint4& e : table) { if (e.z < n) jointBody[e.z] = 1u; if (e.w < n) jointBody[e.w] = 1u; }
		cluster.jointBodyMask.ensure(n + 1, stream); cluster.jointListsValid = false;
		MI_CHECK(hipMemcpyAsync(cluster.jointBodyMask.p, jointBody.data(), sizeof(u32) * (n + 1), hipMemcpyHostToDevice, stream));
		cluster.rep.ensure(n + 1, stream); cluster.jointTable.ensure(std::max<size_t>(table.size(), 1), stream);
		MI_CHECK(hipMemcpyAsync(cluster.rep.p, rep.data(), sizeof(u32) * (n + 1), hipMemcpyHostToDevice, stream));
		if (!table.empty()) MI_CHECK(hipMemcpyAsync(cluster.jointTable.p, table.data(), sizeof(uint4) * table.size(), hipMemcpyHostToDevice, stream));
		MI_CHECK(hipStreamSynchronize(stream));
	}
	jointsDirty = false; jointVersion++;
}
