// Narrowphase, first stage: prune, classify and bucket the broadphase pairs (reference collision_narrow.cpp:2346-2453), and
// launch_narrowphase, the sequence of all stages.  narrow.h has the overview and the pair keys.
#include "narrow.h"

MI_DEV bool typeSupported(u32 t) { return t <= MI_HULL; }

// ---------------------------------------------------------------------------------------------------------------
// K5: prune + classify.  Reads the 16-B tag quarter of both colliders.
// ---------------------------------------------------------------------------------------------------------------
// Equal types: the reference's sweep reports a pair as (collider whose start endpoint comes later on the sorting axis, the one already
// active) (collision_broad.cpp:127) and the narrowphase swaps equal-type pairs (collision_narrow.cpp:2374), so A = the collider
// whose box STARTS FIRST on this step's sorting axis.  Equal starts: the reference's order is that of its endpoint array (a stable
// insertion sort carried over from earlier frames); here the lower collider index comes first.
__global__ void __launch_bounds__(256) k_classify(const u32* __restrict__ counters, u32 nb, const uint2* __restrict__ pairs, const ColliderRec* __restrict__ colWorld, const float4* __restrict__ aabbMin, u32 stepParity,
	u32* __restrict__ pairKey, u64* __restrict__ pairPacked, u32 numLaunched)
{
	u32 p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= numLaunched) return;
	if (p >= counters[CTR_NUM_PAIRS]) { pairKey[p] = KEY_INVALID; pairPacked[p] = 0ull; return; } // (the launch is sized before the host knows the pair count: the surplus sorts behind everything)
	uint2 pr = pairs[p];
	float4 da = colWorld[pr.x].d, db = colWorld[pr.y].d;
	u32 tA = __float_as_uint(da.x), tB = __float_as_uint(db.x), bA = __float_as_uint(da.y), bB = __float_as_uint(db.y);
	u32 key = KEY_INVALID;
	bool rbA = bA < nb, rbB = bB < nb;
	if ((rbA || rbB) && !(rbA && rbB && bA == bB) && typeSupported(tA) && typeSupported(tB)) // :2358-2369
	{
		bool swap = tA > tB; // :2374: A = the lower type
		if (tA == tB)
		{
			const u32 axis = counters[CTR_SAP_AXIS + stepParity];
			float4 ma = aabbMin[pr.x], mb = aabbMin[pr.y];
			float sa = axis == 0u ? ma.x : (axis == 1u ? ma.y : ma.z), sb = axis == 0u ? mb.x : (axis == 1u ? mb.y : mb.z);
			swap = sb < sa || (sb == sa && pr.y < pr.x);
		}
		if (swap) { u32 t = pr.x; pr.x = pr.y; pr.y = t; t = tA; tA = tB; tB = t; }
		u32 zone = (__float_as_uint(da.w) | __float_as_uint(db.w)) & 0xFFu; // a force-field / trigger collider is in the pair
		key = zone ? KEY_ZONE : ::pairKey(tA, tB);
	}
	pairKey[p] = key;
	pairPacked[p] = ((u64)pr.y << 32) | pr.x;
}

__global__ void k_bucket_offsets(u32* __restrict__ counters, const u32* __restrict__ keySorted)
{
	u32 b = threadIdx.x; // bucket key 0..63
	u32 n = counters[CTR_NUM_PAIRS];
	u32 lo = 0, hi = n;
	while (lo < hi) { u32 mid = (lo + hi) >> 1; if (keySorted[mid] < b) lo = mid + 1; else hi = mid; }
	counters[CTR_BUCKET_START + b] = lo; // collision keys are <= KEY_HULL_HULL; KEY_ZONE (overlap checks) and KEY_INVALID sort last: manifold slots end where KEY_ZONE starts
	if (b == KEY_ZONE) { counters[CTR_NUM_VALID] = lo; counters[CTR_EPA_COUNT] = 0; counters[CTR_EPA_COUNT_HULL] = 0; counters[CTR_NUM_ACTIVE] = 0; counters[CTR_NUM_CONTACTS] = 0; }
}

static void launch_bucket_offsets(World& w) { hipLaunchKernelGGL(k_bucket_offsets, dim3(1), dim3(64), 0, w.stream, w.dCounters.p, w.pairKeySorted.p); }

void launch_narrowphase(World& w, u32 numPairs, u32 stepParity, bool deferSide)
{
	w.narrowSidePairs = 0; // (a side chain still owed to an earlier launch is void: this launch replaces that one)
	if (!numPairs)
	{
		if (w.terrain.chunksPerDim) launch_bucket_offsets(w); // no pairs: all buckets empty, the terrain contacts start at slot 0
		return;
	}
	hipLaunchKernelGGL(k_classify, dim3((numPairs + 255) / 256), dim3(256), 0, w.stream, w.dCounters.p, w.nb, w.pairs.p, w.colWorld.p, w.aabbMin.p, stepParity, w.pairKey.p, (u64*)w.pairsSorted.p + numPairs, numPairs);
	// sort (bucket key, packed pair): unsorted packed pairs live in the upper half of pairsSorted, sorted ones in the lower half
	csort_pairs_u64(w, w.pairKey.p, w.pairKeySorted.p, (const u64*)w.pairsSorted.p + numPairs, (u64*)w.pairsSorted.p, numPairs, 64);
	launch_bucket_offsets(w);
	// Two chains that share no data (narrow.h): GJK -> EPA on w.stream, closed forms + box-box on the side stream.
	if (!w.narrowSideStream)
	{
		launch_gjk(w, numPairs);
		launch_pair_kernels(w, numPairs, w.stream);
		launch_epa(w, numPairs);
		return;
	}
	MI_CHECK(hipEventRecord(w.narrowFork, w.stream));
	launch_gjk(w, numPairs);
	launch_epa(w, numPairs);
	w.narrowSidePairs = numPairs;
	if (!deferSide) launch_narrow_side(w);
}

// The side chain of the last launch_narrowphase, and the join: w.stream waits for it here, so whatever is launched next (and every
// buffer ensure before the next narrowphase) is behind both chains.  The side stream's wait for the fork event is a packet at the
// head of its queue from its submission until the main stream gets to the fork, and as long as one is there every kernel launch of
// the main stream is about 0.7 us slower (measured: profiles/narrow_overlap.txt).  The step launches its narrowphase a step's length
// ahead of the device, before its one host synchronisation; the side chain of that launch is submitted behind the synchronisation,
// when the device is about 0.1 ms short of the fork.
void launch_narrow_side(World& w)
{
	const u32 numPairs = w.narrowSidePairs;
	if (!numPairs) return;
	w.narrowSidePairs = 0;
	MI_CHECK(hipStreamWaitEvent(w.narrowStream, w.narrowFork, 0));
	launch_pair_kernels(w, numPairs, w.narrowStream);
	MI_CHECK(hipEventRecord(w.narrowJoin, w.narrowStream));
	MI_CHECK(hipStreamWaitEvent(w.stream, w.narrowJoin, 0));
}
