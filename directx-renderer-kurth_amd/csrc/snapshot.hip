// Snapshot / restore: the blob format, its writer and reader, mi_snapshot_size / mi_snapshot_save / mi_world_restore.
#include "api.h"
#include <cstring>
#include <algorithm>

namespace
{
	const uint32_t SNAPSHOT_MAGIC = 0x4850494Du, SNAPSHOT_VERSION = 6;
	struct BlobWriter
	{
		std::vector<uint8_t> bytes;
		void put(const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; bytes.insert(bytes.end(), b, b + n); }
		template <typename T> void pod(const T& v) { put(&v, sizeof(T)); }
		template <typename T> void vec(const std::vector<T>& v) { uint64_t n = v.size(); pod(n); if (n) put(v.data(), n * sizeof(T)); }
	};
	struct BlobReader
	{
		const uint8_t* p; size_t left; bool ok = true;
		void get(void* dst, size_t n) { if (n > left) { ok = false; return; } memcpy(dst, p, n); p += n; left -= n; }
		template <typename T> void pod(T& v) { get(&v, sizeof(T)); }
		template <typename T> void vec(std::vector<T>& v) { uint64_t n = 0; pod(n); if (!ok || n * sizeof(T) > left) { ok = false; return; } v.resize((size_t)n); if (n) get(v.data(), (size_t)n * sizeof(T)); }
	};
	std::vector<u64> previousKeys(World& w, DevBuf<u64>* tables, u32 size, u32 cur) // keys of the set the next step diffs against
	{
		std::vector<u64> keys;
		if (!size) return keys;
		std::vector<u64> image(size);
		w.resolvePendingFlow();
		MI_CHECK(hipMemcpyAsync(image.data(), tables[cur ^ 1].p, sizeof(u64) * size, hipMemcpyDeviceToHost, w.stream));
		MI_CHECK(hipStreamSynchronize(w.stream));
		for (u64 k : image) if (k != ~0ull) keys.push_back(k);
		std::sort(keys.begin(), keys.end());
		return keys;
	}
	struct BodyPod { float pos[3], rot[4], localCOG[3], invMass, invInertia[9], gravityFactor, linDamp, angDamp, v[3], w[3], force[3], torque[3]; uint32_t removed; };
	void serialize(World& w, BlobWriter& out)
	{
		w.forceFullColoring = true; // the image has no colour history: this world and the restored one both colour from scratch next step
		w.pullJointPods();
		w.upload();
		if (w.stateOnDevice) w.downloadState();
		out.pod(SNAPSHOT_MAGIC); out.pod(SNAPSHOT_VERSION);
		uint64_t nb = w.bodies.size(), nc = w.colliders.size(), nh = w.hulls.size();
		out.pod(nb); out.pod(nc); out.pod(nh);
		for (const World::HBody& b : w.bodies)
		{
			BodyPod p{};
			memcpy(p.pos, b.pos, 12); memcpy(p.rot, b.rot, 16); memcpy(p.localCOG, b.localCOG, 12); p.invMass = b.invMass; memcpy(p.invInertia, b.invInertia, 36);
			p.gravityFactor = b.gravityFactor; p.linDamp = b.linDamp; p.angDamp = b.angDamp;
			memcpy(p.v, b.v, 12); memcpy(p.w, b.w, 12); memcpy(p.force, b.force, 12); memcpy(p.torque, b.torque, 12); p.removed = b.removed ? 1u : 0u;
			out.pod(p); out.vec(b.colliders);
		}
		for (const World::HCollider& c : w.colliders) out.pod(c);
		for (const World::HHull& h : w.hulls) { out.vec(h.vertices); out.vec(h.triangles); out.put(h.aabbMin, 12); out.put(h.aabbMax, 12); }
		for (const JointSet& js : w.joints) { out.vec(js.pods); out.vec(js.a); out.vec(js.b); out.vec(js.alive); }
		// the sweep's sorting axis of the next step (the reference keeps it in its sap_context, collision_broad.cpp:20-24): it orients equal-type pairs
		{
			uint32_t axis = 0;
			if (w.dCounters.p) { MI_CHECK(hipMemcpyAsync(&axis, w.dCounters.p + CTR_SAP_AXIS + (w.stats.numInternalSteps & 1u), sizeof(u32), hipMemcpyDeviceToHost, w.stream)); MI_CHECK(hipStreamSynchronize(w.stream)); }
			out.pod(axis);
		}
		// force fields, triggers, and the previous step's overlap / collision sets (so that the next step raises the same events)
		out.vec(w.zones.fields); out.vec(w.zones.triggers);
		uint32_t flags = (w.zones.collisionBeginEvents ? 1u : 0u) | (w.zones.collisionEndEvents ? 2u : 0u); out.pod(flags);
		out.vec(previousKeys(w, w.zones.triggerSet, w.zones.triggerSetSize, w.zones.triggerCur)); out.vec(previousKeys(w, w.zones.collisionSet, w.zones.collisionSetSize, w.zones.collisionCur));
		// heightmap terrain
		out.pod(w.terrain.chunksPerDim); out.pod(w.terrain.chunkSize); out.pod(w.terrain.amplitude); out.put(w.terrain.minCorner, 12); out.put(w.terrain.material, 12);
		out.vec(w.terrain.hHeights); out.vec(w.terrain.hValid);
		// cloths: parameters, particle state, constraints
		w.downloadCloths();
		uint64_t ncl = w.cloth.cloths.size(); out.pod(ncl); out.put(w.cloth.iterations, sizeof(w.cloth.iterations));
		for (const World::HCloth& c : w.cloth.cloths)
		{
			float params[8] = { c.width, c.height, c.totalMass, c.stiffness, c.damping, c.gravityFactor, c.oldTotalMass, c.oldStiffness };
			out.put(params, sizeof(params)); out.pod(c.gridX); out.pod(c.gridY);
			out.vec(c.pos); out.vec(c.prev); out.vec(c.vel); out.vec(c.invMass); out.vec(c.constraints);
			uint32_t collide = c.collide ? 1u : 0u; out.pod(collide); out.pod(c.collision); // the settings of the projection pass; the contact plane does not travel
		}
	}
}

extern "C" {

// ---- snapshot / restore (row N3 of SURVEY §8f: checkpoint + resume; the engine's own scene files, serialization_yaml.cpp /
// serialization_binary.cpp, are asset formats and stay out of scope).  The blob holds everything the add API and the steps have put
// into the world: bodies with their current pose / velocity / accumulators and mass properties, colliders, hull geometries, joints.
// A world restored from it continues bit-identically (tests/test_gpu_snapshot.py).  Layout: 'MIPH', version, six counts, then the
// records in the order below, plain little-endian PODs.
uint64_t mi_snapshot_size(mi_world* world) { CHECK_WORLD(0); BlobWriter out; serialize(*W, out); return out.bytes.size(); }
int mi_snapshot_save(mi_world* world, void* buffer, uint64_t capacity)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	BlobWriter out; serialize(*W, out);
	if (W->lastError) return W->lastError;
	W->refreshCounters();     // the last step is counted now, not at the next step:
	W->cluster.sortDue = true; // the restored world orders its bodies at its first step: so does this one at its next ...
	W->cluster.compIdle = false;      // ... and runs the component phase in it, as a world without a last step does (the step has been counted above)
	W->cluster.cooldown = 0; W->cluster.failStreak = 0; // ... with the cluster sweep on
	if (!buffer || capacity < out.bytes.size()) { W->fail(MI_ERR_CAPACITY, "mi_snapshot_save: buffer too small (ask mi_snapshot_size)"); return MI_ERR_CAPACITY; }
	memcpy(buffer, out.bytes.data(), out.bytes.size());
	return MI_OK;
}
mi_world* mi_world_restore(const mi_world_desc* desc, const void* buffer, uint64_t size)
{
	mi_world* world = mi_world_create(desc);
	if (!world) return nullptr;
	World& w = world->w;
	BlobReader in{ (const uint8_t*)buffer, (size_t)size };
	uint32_t magic = 0, version = 0; uint64_t nb = 0, nc = 0, nh = 0;
	in.pod(magic); in.pod(version); in.pod(nb); in.pod(nc); in.pod(nh);
	if (!in.ok || magic != SNAPSHOT_MAGIC || version != SNAPSHOT_VERSION) { g_createError = "mi_world_restore: not a snapshot of this library version"; delete world; return nullptr; }
	for (uint64_t i = 0; in.ok && i < nb; ++i)
	{
		BodyPod p; in.pod(p);
		World::HBody b{};
		memcpy(b.pos, p.pos, 12); memcpy(b.rot, p.rot, 16); memcpy(b.localCOG, p.localCOG, 12); b.invMass = p.invMass; memcpy(b.invInertia, p.invInertia, 36);
		b.gravityFactor = p.gravityFactor; b.linDamp = p.linDamp; b.angDamp = p.angDamp;
		memcpy(b.v, p.v, 12); memcpy(b.w, p.w, 12); memcpy(b.force, p.force, 12); memcpy(b.torque, p.torque, 12); b.removed = p.removed != 0;
		in.vec(b.colliders);
		w.bodies.push_back(b);
	}
	for (uint64_t i = 0; in.ok && i < nc; ++i) { World::HCollider c; in.pod(c); w.colliders.push_back(c); }
	for (uint64_t i = 0; in.ok && i < nh; ++i) { World::HHull h; in.vec(h.vertices); in.vec(h.triangles); in.get(h.aabbMin, 12); in.get(h.aabbMax, 12); w.hulls.push_back(h); }
	for (JointSet& js : w.joints) { in.vec(js.pods); in.vec(js.a); in.vec(js.b); in.vec(js.alive); }
	{
		uint32_t axis = 0; in.pod(axis);
		if (in.ok && axis < 3u && w.dCounters.p) { MI_CHECK(hipMemcpyAsync(w.dCounters.p + CTR_SAP_AXIS, &axis, sizeof(u32), hipMemcpyHostToDevice, w.stream)); MI_CHECK(hipStreamSynchronize(w.stream)); } // the restored world's step 0 reads word 0
	}
	std::vector<u64> triggerKeys, collisionKeys; uint32_t flags = 0;
	in.vec(w.zones.fields); in.vec(w.zones.triggers); in.pod(flags); in.vec(triggerKeys); in.vec(collisionKeys);
	in.pod(w.terrain.chunksPerDim); in.pod(w.terrain.chunkSize); in.pod(w.terrain.amplitude); in.get(w.terrain.minCorner, 12); in.get(w.terrain.material, 12);
	in.vec(w.terrain.hHeights); in.vec(w.terrain.hValid);
	w.queries.terrainTableValid = false;
	if (in.ok && w.terrain.chunksPerDim)
	{
		size_t chunks = (size_t)w.terrain.chunksPerDim * w.terrain.chunksPerDim;
		if (w.terrain.hValid.size() != chunks || w.terrain.hHeights.size() != chunks * 129 * 129) in.ok = false;
		else
		{
			w.terrain.heights.ensure(w.terrain.hHeights.size(), w.stream); w.terrain.valid.ensure(chunks, w.stream);
			MI_CHECK(hipMemcpyAsync(w.terrain.heights.p, w.terrain.hHeights.data(), sizeof(uint16_t) * w.terrain.hHeights.size(), hipMemcpyHostToDevice, w.stream));
			MI_CHECK(hipMemcpyAsync(w.terrain.valid.p, w.terrain.hValid.data(), sizeof(u32) * chunks, hipMemcpyHostToDevice, w.stream));
			MI_CHECK(hipStreamSynchronize(w.stream));
		}
	}
	uint64_t ncl = 0; in.pod(ncl); in.get(w.cloth.iterations, sizeof(w.cloth.iterations));
	for (uint64_t i = 0; in.ok && i < ncl; ++i)
	{
		World::HCloth c; float params[8] = {};
		in.get(params, sizeof(params)); in.pod(c.gridX); in.pod(c.gridY);
		c.width = params[0]; c.height = params[1]; c.totalMass = params[2]; c.stiffness = params[3]; c.damping = params[4]; c.gravityFactor = params[5]; c.oldTotalMass = params[6]; c.oldStiffness = params[7];
		in.vec(c.pos); in.vec(c.prev); in.vec(c.vel); in.vec(c.invMass); in.vec(c.constraints);
		uint32_t collide = 0; in.pod(collide); in.pod(c.collision); c.collide = collide != 0;
		if (c.collide) w.cloth.numColliding++;
		if (in.ok && (c.pos.size() != 3 * (size_t)c.gridX * c.gridY || c.vel.size() != c.pos.size() || c.prev.size() != c.pos.size() || c.invMass.size() * 3 != c.pos.size())) in.ok = false;
		w.cloth.cloths.push_back(std::move(c));
	}
	if (!in.ok) { g_createError = "mi_world_restore: truncated snapshot"; delete world; return nullptr; }
	{ // every index the kernels will follow must point inside this world
		bool valid = true;
		const size_t numBodies = w.bodies.size(), numColliders = w.colliders.size(), numHulls = w.hulls.size();
		for (const World::HBody& b : w.bodies) for (u32 c : b.colliders) if (c >= numColliders) valid = false;
		for (const World::HCollider& c : w.colliders)
		{
			if (c.body != MI_STATIC_BODY && c.body >= numBodies) valid = false;
			if (c.type > MI_HULL) valid = false;
			if (c.type == MI_HULL && !(c.shape[7] >= 0.f && (size_t)c.shape[7] < numHulls)) valid = false;
			if (c.zoneType == 2 && c.zoneIndex >= w.zones.fields.size()) valid = false;
			if (c.zoneType == 3 && c.zoneIndex >= w.zones.triggers.size()) valid = false;
		}
		for (const World::HHull& h : w.hulls) { if (h.vertices.size() % 3 || h.triangles.size() % 3) valid = false; for (u32 t : h.triangles) if ((size_t)t * 3 + 2 >= h.vertices.size()) valid = false; }
		for (u32 t = 0; t < MI_JOINT_TYPES; ++t)
		{
			const JointSet& js = w.joints[t];
			size_t n = js.a.size();
			if (js.b.size() != n || js.alive.size() != n || js.pods.size() != n * MI_JOINT_POD_SIZE[t]) { valid = false; continue; }
			for (size_t i = 0; i < n; ++i) if (js.alive[i] && (js.a[i] >= numBodies || js.b[i] >= numBodies)) valid = false;
		}
		if (!valid) { g_createError = "mi_world_restore: snapshot holds an index outside the world"; delete world; return nullptr; }
	}
	w.cloth.dirty = true;
	w.zones.collisionBeginEvents = (flags & 1u) != 0; w.zones.collisionEndEvents = (flags & 2u) != 0;
	w.topologyDirty = true; w.jointsChanged(); w.zones.fieldsDirty = true;
	w.zones.restoredTriggerKeys = triggerKeys; w.zones.restoredCollisionKeys = collisionKeys; // entered into the sets when the first step sizes them
	return world;
}

} // extern "C"
