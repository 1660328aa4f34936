// Force fields, trigger events, collision begin/end events (row N2 of SURVEY §8f) — reference physics.cpp:759-787, 952-1178.
// None of this is launched for a world without force fields / triggers / enabled collision events.
#include "events.h"
#include "narrow.h" // KEY_ZONE: the pair manifolds end where its bucket starts
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------------------
// Force fields -> force accumulators, before the force integration (physics.cpp:963-967 localized, :1273 global).
// A body's localized forces are added in ascending field id (deterministic; the reference adds them in the order of its pair list),
// then the sum of the global fields.  Consumes and clears the per-body field bits set by k_zone_overlap.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_apply_fields(u32 nb, float4* __restrict__ force, u32* __restrict__ fieldMask, u32 fieldWords, const float4* __restrict__ fieldForce,
	float gx, float gy, float gz, u32 anyGlobal, const uint8_t* __restrict__ simMask)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nb) return;
	float4 F = force[2 * i];
	bool changed = false;
	for (u32 wd = 0; wd < fieldWords; ++wd)
	{
		u32 bits = fieldMask[(size_t)i * fieldWords + wd];
		if (!bits) continue;
		fieldMask[(size_t)i * fieldWords + wd] = 0u;
		while (bits)
		{
			u32 f = wd * 32u + (u32)__builtin_ctz(bits);
			bits &= bits - 1u;
			float4 ff = fieldForce[f];
			F.x += ff.x; F.y += ff.y; F.z += ff.z;
			changed = true;
		}
	}
	if (!simMask[i]) return;
	if (anyGlobal) { F.x += gx; F.y += gy; F.z += gz; changed = true; }
	if (changed) force[2 * i] = F;
}

void launch_apply_fields(World& w)
{
	if (w.zones.fields.empty() || !w.nb) return;
	w.uploadFields();
	if (!w.zones.fieldWords && !w.zones.anyGlobalForce) return;
	hipLaunchKernelGGL(k_apply_fields, dim3((w.nb + 255) / 256), dim3(256), 0, w.stream, w.nb, w.force.p, w.zones.fieldMask.p, w.zones.fieldWords, w.zones.fieldForce.p,
		w.zones.globalForce[0], w.zones.globalForce[1], w.zones.globalForce[2], w.zones.anyGlobalForce ? 1u : 0u, w.simMask.p);
}

// ---------------------------------------------------------------------------------------------------------------
// Leave / end events: every key of the previous step's set that this step's set does not hold; the slot is emptied for the
// table's next turn as "this step".
// ---------------------------------------------------------------------------------------------------------------
template <bool COLLISIONS>
__global__ void __launch_bounds__(256) k_scan_previous_set(PairSetView set, EventSink sink, const ColliderRec* __restrict__ colWorld, u32 nb, u32 emit)
{
	u32 s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s > set.mask) return;
	u64 key = set.prev[s];
	if (key == PAIRSET_EMPTY) return;
	set.prev[s] = PAIRSET_EMPTY;
	if (!emit || pairSetContains(set.cur, set.mask, set.shift, key)) return;
	u32 a = (u32)(key >> 32), b = (u32)key;
	if (COLLISIONS)
	{
		u32 bodyA = colBody(colWorld[a]), bodyB = colBody(colWorld[b]);
		if (eventIsMine(sink, bodyA, bodyB, nb)) eventWritePlain(sink, EVENT_COLLISION_END, a, b, bodyA < nb ? bodyA : 0xFFFFFFFFu, bodyB < nb ? bodyB : 0xFFFFFFFFu);
	}
	else if (eventIsMine(sink, b, b, nb)) eventWritePlain(sink, EVENT_TRIGGER_LEAVE, a, b, 0xFFFFFFFFu, b);
}

static PairSetView viewOf(DevBuf<u64>* tables, u32 size, u32 cur)
{
	PairSetView v; v.cur = tables[cur].p; v.prev = tables[cur ^ 1].p; v.mask = size - 1; v.shift = 64u - (u32)__builtin_ctz(size);
	return v;
}
EventSink sinkOf(World& w) { EventSink s = { (EventRec*)w.zones.eventRing.p, w.dCounters.p, w.zones.eventCap, w.stats.numInternalSteps, w.slab.size > 1 ? w.slab.code.p : nullptr }; return s; }

void launch_trigger_events(World& w)
{
	if (w.zones.triggers.empty() || !w.zones.triggerSetSize) return;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_previous_set<false>), dim3((w.zones.triggerSetSize + 255) / 256), dim3(256), 0, w.stream, viewOf(w.zones.triggerSet, w.zones.triggerSetSize, w.zones.triggerCur), sinkOf(w), w.colWorld.p, w.nb, 1u);
	w.zones.triggerCur ^= 1u;
}

// ---------------------------------------------------------------------------------------------------------------
// Begin events: one lane per manifold slot; a slot with contacts enters its collider pair into this step's set, a pair the previous
// step's set does not hold raises the event — mean contact point and normal, relative velocity of the two bodies at that point from
// the velocities after the force integration (physics.cpp:1075-1115).
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_collision_begin(u32* __restrict__ counters, const u64* __restrict__ pairSorted, const ManifoldRec* __restrict__ manifolds,
	const float4* __restrict__ vel, const float4* __restrict__ cog, u32 nb, PairSetView set, EventSink sink, u32 emit)
{
	u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= counters[CTR_BUCKET_START + KEY_ZONE]) return; // pair manifolds only: terrain contacts raise no events (physics.cpp:1049: colliderB < numColliders)
	uint4 ids = manifolds[slot].ids;
	u32 count = ids.z;
	if (!count) return;
	u64 packed = pairSorted[slot];
	u32 a = (u32)packed, b = (u32)(packed >> 32);
	u64 key = ((u64)a << 32) | b;
	if (!pairSetInsert(set.cur, set.mask, set.shift, key, counters)) return;
	if (!emit || pairSetContains(set.prev, set.mask, set.shift, key)) return;
	if (!eventIsMine(sink, ids.x, ids.y, nb)) return;
	EventRec* e = eventAppend(sink);
	if (!e) return;
	ManifoldRec m = manifolds[slot];
	float norm = 1.f / (float)count;
	V3 point = v3s(0.f), normal = v3s(0.f), n = v3(m.nf.x, m.nf.y, m.nf.z);
	for (u32 k = 0; k < count; ++k) { point += v3f4(m.p[k]); normal += n; }
	point = point * norm; normal = normal * norm;
	u32 bodyA = ids.x, bodyB = ids.y; // nb = the static dummy: zero velocity at the origin (physics.cpp:1279)
	V3 velA = v3f4(vel[2 * bodyA]) + cross(v3f4(vel[2 * bodyA + 1]), point - v3f4(cog[bodyA]));
	V3 velB = v3f4(vel[2 * bodyB]) + cross(v3f4(vel[2 * bodyB + 1]), point - v3f4(cog[bodyB]));
	V3 rel = velB - velA;
	EventRec r; r.kind = EVENT_COLLISION_BEGIN; r.step = sink.step; r.a = a; r.b = b; r.bodyA = bodyA < nb ? bodyA : 0xFFFFFFFFu; r.bodyB = bodyB < nb ? bodyB : 0xFFFFFFFFu;
	r.position[0] = point.x; r.position[1] = point.y; r.position[2] = point.z;
	r.normal[0] = normal.x; r.normal[1] = normal.y; r.normal[2] = normal.z;
	r.relativeVelocity[0] = rel.x; r.relativeVelocity[1] = rel.y; r.relativeVelocity[2] = rel.z;
	*e = r;
}

void launch_collision_events(World& w, u32 numPairs)
{
	if (!(w.zones.collisionBeginEvents || w.zones.collisionEndEvents) || !w.zones.collisionSetSize) return;
	PairSetView v = viewOf(w.zones.collisionSet, w.zones.collisionSetSize, w.zones.collisionCur);
	if (numPairs)
		hipLaunchKernelGGL(k_collision_begin, dim3((numPairs + 255) / 256), dim3(256), 0, w.stream, w.dCounters.p, (const u64*)w.pairsSorted.p, w.manifolds.p, w.vel.p, w.cog.p, w.nb, v, sinkOf(w), w.zones.collisionBeginEvents ? 1u : 0u);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_previous_set<true>), dim3((w.zones.collisionSetSize + 255) / 256), dim3(256), 0, w.stream, v, sinkOf(w), w.colWorld.p, w.nb, w.zones.collisionEndEvents ? 1u : 0u);
	w.zones.collisionCur ^= 1u;
}

// ---- force fields / events: host side ------------------------------------------------------------------------------
static V3 fieldForceWorld(const World::HField& f) // physics.cpp:767-771
{
	V3 force = v3(f.force[0], f.force[1], f.force[2]);
	return f.hasTransform ? (q4(f.rot[0], f.rot[1], f.rot[2], f.rot[3]) * force) : force;
}
void World::uploadFields()
{
	if (!zones.fieldsDirty) return;
	zones.fieldsDirty = false;
	std::vector<float4> hf(std::max<size_t>(zones.fields.size(), 1), make_float4(0.f, 0.f, 0.f, 0.f));
	V3 sum = v3s(0.f); zones.anyGlobalForce = false; bool anyLocal = false;
	for (size_t i = zones.fields.size(); i-- > 0;) // getForceFieldStates (physics.cpp:759-787): EnTT walks newest first
	{
		V3 f = fieldForceWorld(zones.fields[i]);
		if (zones.fields[i].numColliders) { hf[i] = make_float4(f.x, f.y, f.z, 0.f); anyLocal = true; }
		else { sum = sum + f; zones.anyGlobalForce = true; }
	}
	zones.globalForce[0] = sum.x; zones.globalForce[1] = sum.y; zones.globalForce[2] = sum.z;
	u32 words = anyLocal ? ((u32)zones.fields.size() + 31u) / 32u : 0u;
	zones.fieldForce.ensure(hf.size(), stream);
	MI_CHECK(hipMemcpyAsync(zones.fieldForce.p, hf.data(), sizeof(float4) * hf.size(), hipMemcpyHostToDevice, stream));
	size_t maskWords = std::max<size_t>((size_t)words * ((size_t)nb + 1), 1);
	if (words != zones.fieldWords || maskWords > zones.fieldMask.cap)
	{
		zones.fieldWords = words;
		zones.fieldMask.ensure(maskWords, stream);
		MI_CHECK(hipMemsetAsync(zones.fieldMask.p, 0, sizeof(u32) * maskWords, stream)); // bits are set by k_zone_overlap and cleared by k_apply_fields
	}
	MI_CHECK(hipStreamSynchronize(stream)); // `hf` goes out of scope
}

// Gives both tables of a pair set `newSize` slots; the previous step's keys (tables[cur ^ 1]) move over.
static void resizePairSet(World& w, DevBuf<u64>* tables, u32& size, u32 cur, u32 newSize, std::vector<u64>* seed = nullptr)
{
	const u32 shift = 64u - (u32)__builtin_ctz(newSize);
	std::vector<u64> image(newSize, ~0ull);
	if (seed)
	{
		for (u64 key : *seed) { u32 h = pairSetHash(key, shift); while (image[h] != ~0ull) h = (h + 1) & (newSize - 1); image[h] = key; }
		seed->clear();
	}
	if (size)
	{
		std::vector<u64> old(size);
		MI_CHECK(hipMemcpyAsync(old.data(), tables[cur ^ 1].p, sizeof(u64) * size, hipMemcpyDeviceToHost, w.stream));
		MI_CHECK(hipStreamSynchronize(w.stream));
		for (u64 key : old)
		{
			if (key == ~0ull) continue;
			u32 h = pairSetHash(key, shift);
			while (image[h] != ~0ull) h = (h + 1) & (newSize - 1);
			image[h] = key;
		}
	}
	tables[0].ensure(newSize, w.stream); tables[1].ensure(newSize, w.stream);
	MI_CHECK(hipMemsetAsync(tables[cur].p, 0xFF, sizeof(u64) * newSize, w.stream));
	MI_CHECK(hipMemcpyAsync(tables[cur ^ 1].p, image.data(), sizeof(u64) * newSize, hipMemcpyHostToDevice, w.stream));
	MI_CHECK(hipStreamSynchronize(w.stream));
	size = newSize;
}
void World::ensureEventBuffers(u32 numPairs)
{
	bool collisions = zones.collisionBeginEvents || zones.collisionEndEvents;
	if (zones.triggers.empty() && !collisions && zones.fields.empty()) return;
	if (!zones.fields.empty()) uploadFields(); // the narrowphase's overlap kernel needs the per-body field bits
	if (!zones.eventRing.p)
	{
		if (const char* e = getenv("MI_EVENT_CAPACITY")) zones.eventCap = std::max(16, atoi(e));
		zones.eventRing.ensure((size_t)zones.eventCap * sizeof(mi_event), stream);
	}
	if (!zones.triggers.empty())
	{
		// One key per overlapping (trigger, body): any number of triggers may hold one body, so the bodies do not bound the keys.  This
		// step's pair count does (every key comes from a pair of the zone bucket) and is on the host: the table is at most half full.
		u32 want = std::max(4096u, nextPow2(4u * std::max(nb, 1u)));
		want = std::max(want, nextPow2(2u * std::min(numPairs, 1u << 29)));
		want = std::max(want, nextPow2(4u * (u32)zones.restoredTriggerKeys.size()));
		if (want > zones.triggerSetSize) resizePairSet(*this, zones.triggerSet, zones.triggerSetSize, zones.triggerCur, want, &zones.restoredTriggerKeys);
	}
	if (collisions)
	{
		u32 want = std::max(4096u, nextPow2(2u * std::max(numPairs, lastNumManifolds * 2u)));
		want = std::max(want, nextPow2(4u * (u32)zones.restoredCollisionKeys.size()));
		if (want > zones.collisionSetSize) resizePairSet(*this, zones.collisionSet, zones.collisionSetSize, zones.collisionCur, want, &zones.restoredCollisionKeys);
	}
}
