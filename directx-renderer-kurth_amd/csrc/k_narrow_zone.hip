// ---------------------------------------------------------------------------------------------------------------
// Non-collision interactions: rigid body vs force-field / trigger collider — overlapCheck, collision_narrow.cpp:1593-1689, over the
// boolean tests of bounding_volumes.h:301-363 and bounding_volumes.cpp:704-835, 1079-1244.  One lane per pair of the KEY_ZONE bucket.
// A hit sets the body's bit of the field (k_apply_fields adds the forces in ascending field id) or enters the
// (trigger, body) pair into this step's overlap set (enter event if the previous step's set does not hold it).
// ---------------------------------------------------------------------------------------------------------------
#include "narrow_gjk.h"
#include "zone_overlap.h"
#include "events.h"

__global__ void __launch_bounds__(64) k_zone_overlap(u32* __restrict__ counters, const u64* __restrict__ pairSorted, const ColliderRec* __restrict__ colWorld,
	const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts, u32 nb, u32* __restrict__ fieldMask, u32 fieldWords, PairSetView triggers, EventSink sink)
{
	u32 slot = counters[CTR_BUCKET_START + KEY_ZONE] + blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= counters[CTR_BUCKET_START + KEY_INVALID]) return;
	u64 packed = pairSorted[slot];
	ColliderRec A = colWorld[(u32)packed], B = colWorld[(u32)(packed >> 32)];
	if (!overlapColliders(pairKey(colType(A), colType(B)), A, B, hullInfo, hullVerts)) return;
	bool zoneIsA = (__float_as_uint(A.d.w) & 0xFFu) != 0;
	u32 flags = __float_as_uint(zoneIsA ? A.d.w : B.d.w);
	u32 body = colBody(zoneIsA ? B : A), zoneType = flags & 0xFFu, zoneIndex = flags >> 8;
	if (body >= nb) return;
	if (zoneType == 2u) { if (fieldWords) atomicOr(&fieldMask[(size_t)body * fieldWords + (zoneIndex >> 5)], 1u << (zoneIndex & 31u)); }
	else if (triggers.cur)
	{
		u64 key = ((u64)zoneIndex << 32) | body;
		if (pairSetInsert(triggers.cur, triggers.mask, triggers.shift, key, counters) && !pairSetContains(triggers.prev, triggers.mask, triggers.shift, key) && eventIsMine(sink, body, body, nb))
			eventWritePlain(sink, EVENT_TRIGGER_ENTER, zoneIndex, body, 0xFFFFFFFFu, body);
	}
}

// Force fields and triggers: boolean overlap tests on the pairs behind the collision buckets (collision_narrow.cpp:2573-2593).  Not
// part of launch_narrowphase: it enters pairs into the trigger set and raises events, so it must run exactly once per step.
void launch_zone_overlap(World& w, u32 numPairs)
{
	if (!numPairs || (w.zones.fields.empty() && w.zones.triggers.empty())) return;
	const u64* sortedPairs = (const u64*)w.pairsSorted.p;
	PairSetView tv = { w.zones.triggers.empty() ? nullptr : w.zones.triggerSet[w.zones.triggerCur].p, w.zones.triggers.empty() ? nullptr : w.zones.triggerSet[w.zones.triggerCur ^ 1].p, w.zones.triggerSetSize - 1, 64u - (u32)__builtin_ctz(w.zones.triggerSetSize ? w.zones.triggerSetSize : 2u) };
	EventSink sink = sinkOf(w);
	hipLaunchKernelGGL(k_zone_overlap, dim3((numPairs + 63) / 64), dim3(64), 0, w.stream, w.dCounters.p, sortedPairs, w.colWorld.p, w.hullInfo.p, w.hullVerts.p, w.nb,
		w.zones.fieldMask.p, w.zones.fieldWords, tv, sink);
}
