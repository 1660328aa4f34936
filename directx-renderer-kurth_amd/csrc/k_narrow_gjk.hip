// Narrowphase, GJK + EPA: the tube family (capsule / cylinder vs box, cylinder vs cylinder — reference collision_narrow.cpp:705-790,
// :821-1043) and the hull family (anything vs convex hull, one contact — :496-520, 792-818, 1045-1071, 1150-1176, 1529-1584), each in
// two phases: k_gjk, the boolean test over the family's slots, appends its hits to a work list; k_epa expands the polytopes of
// the hits with dense waves.  narrow.h has the overview and the pair keys, narrow_gjk.h the support functions and the simplex walk.
// (cylinderCylinderParallel, epaWave, capsuleBoxFinish and the simplex record: narrow_epa.h, shared with k_contact_query.hip)
#include "narrow_epa.h"
#include <algorithm>

// Phase 1: the GJK boolean test over the family's contiguous slot range (narrow.h: the tube family's range holds the tubeKey
// buckets and capsule-hull, a hull pair; its other keys cannot occur with typeA <= typeB).  Parallel cylinder pairs finish here in closed form.  Misses write
// their empty manifold; hits append (slot, simplex) to the EPA work list so that phase 2 runs with dense waves — the
// expanding polytope needs ~3.7 KB of private scratch per lane and 20 serial iterations, which must not idle behind misses.
template <int FAMILY>
__global__ void __launch_bounds__(256) k_gjk(u32* __restrict__ counters, const u32* __restrict__ keySorted, const u64* __restrict__ pairSorted,
	const ColliderRec* __restrict__ colWorld, ManifoldRec* __restrict__ manifolds, u32* __restrict__ epaList, float4* __restrict__ gjkSimplex,
	const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts, u32 listCap)
{
	// family 0: the contiguous slot range of the tube keys (capsule-hull is skipped); family 1: the hull range, keys with typeB = hull
	u32 slot = counters[CTR_BUCKET_START + (FAMILY == 0 ? KEY_TUBE_BEGIN : KEY_HULL_BEGIN)] + blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= counters[CTR_BUCKET_START + (FAMILY == 0 ? KEY_TUBE_END : KEY_HULL_END)]) return;
	u32 key = keySorted[slot];
	if (FAMILY == 0 ? hullKey(key) : !hullKey(key)) return;
	u64 packed = pairSorted[slot];
	ColliderRec A = colWorld[(u32)packed], B = colWorld[(u32)(packed >> 32)];
	SupShapes sh; Obb o;
	gjkOperands<FAMILY>(key, A, B, hullInfo, hullVerts, sh, o);
	if (key == KEY_CYLINDER_CYLINDER)
	{
		Man m = emptyManifold();
		int r = cylinderCylinderParallel(sh.tubeA, sh.tubeB, m);
		if (r != 2) { writeManifold(manifolds, slot, m, r == 1, A, B, slot); return; }
	}
	GjkSimplex sx;
	u32 iters;
	const bool gjkHit = gjkPair<FAMILY, true>(sh, sx, &iters);
	if (iters > counters[CTR_NARROW_LIMITS]) atomicMax(&counters[CTR_NARROW_LIMITS], iters); // (read first: once the mark has settled, no lane issues the same-address atomic)
	if (!gjkHit)
	{
		Man m = emptyManifold();
		writeManifold(manifolds, slot, m, false, A, B, slot);
		return;
	}
	u32 j = atomicAdd(&counters[FAMILY == 0 ? CTR_EPA_COUNT : CTR_EPA_COUNT_HULL], 1u); // order of the work list does not affect any result
	if (FAMILY == 1) j = listCap - 1u - j; // the hull pairs fill the list from its end
	epaList[j] = slot;
	storeSimplex(gjkSimplex + (size_t)j * 9, sx);
}

// Phase 2: EPA (EPA_GROUP lanes per hit = two hits per wave, polytopes in LDS) + face clipping (the group's first lane) for every GJK
// hit.  Groups stride over the work list.
template <int FAMILY>
__global__ void __launch_bounds__(64 * EPA_WAVES_PER_BLOCK) __attribute__((amdgpu_waves_per_eu(FAMILY == 0 ? 3 : 2, FAMILY == 0 ? 3 : 3))) k_epa(u32* __restrict__ counters, const u32* __restrict__ keySorted, const u64* __restrict__ pairSorted,
	const ColliderRec* __restrict__ colWorld, ManifoldRec* __restrict__ manifolds, const u32* __restrict__ epaList, const float4* __restrict__ gjkSimplex,
	const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts, u32 listCap)
{
	__shared__ EpaWave shared[EPA_WAVES_PER_BLOCK * EPA_PER_WAVE];
	const u32 wave = threadIdx.x >> 6, group = (threadIdx.x & 63u) / EPA_GROUP, lane = threadIdx.x & (EPA_GROUP - 1u);
	EpaWave& e = shared[wave * EPA_PER_WAVE + group];
	u32 numHits = counters[FAMILY == 0 ? CTR_EPA_COUNT : CTR_EPA_COUNT_HULL];
	u32 stride = gridDim.x * EPA_WAVES_PER_BLOCK * EPA_PER_WAVE;
	for (u32 jj = (blockIdx.x * EPA_WAVES_PER_BLOCK + wave) * EPA_PER_WAVE + group; jj < numHits; jj += stride)
	{
		u32 j = (FAMILY == 0) ? jj : listCap - 1u - jj;
		u32 slot = epaList[j];
		u32 key = keySorted[slot];
		u64 packed = pairSorted[slot];
		ColliderRec A = colWorld[(u32)packed], B = colWorld[(u32)(packed >> 32)];
		SupShapes sh; Obb o;
		gjkOperands<FAMILY>(key, A, B, hullInfo, hullVerts, sh, o);
		GjkSimplex sx;
		loadSimplex(gjkSimplex + (size_t)j * 9, sx);
		V3 point, normal; float depth;
		epaWave<FAMILY>(e, lane, group * EPA_GROUP, sx, sh, point, normal, depth, counters);
		if (lane == 0)
		{
			Man m = emptyManifold();
			if (FAMILY == 1 || key == KEY_CYLINDER_CYLINDER) { m.n = normal; m.count = 1; m.p[0] = make_float4(point.x, point.y, point.z, depth); } // :905-950; hull pairs
			else
			{
				const PolyStore store = { (float4*)e.tnx, (float4*)e.tnx + 16, 1u }; // the finished polytope's triangle arrays (2 KB, 16-byte aligned) hold the two 16-point clipping polygons: LDS, not scratch
				capsuleBoxFinish(point, normal, depth, sh.tubeA, sh.box, m, store);
			}
			if (key == KEY_CAPSULE_OBB || key == KEY_CYLINDER_OBB) // back to world space (:779-787, :1032-1040)
			{
				m.n = o.q * m.n;
#pragma unroll
				for (u32 i = 0; i < 4; ++i)
				{
					if (i >= m.count) break;
					V3 pt = o.q * (v3f4(m.p[i]) - o.c) + o.c;
					m.p[i] = make_float4(pt.x, pt.y, pt.z, m.p[i].w);
				}
			}
			writeManifold(manifolds, slot, m, true, A, B, slot);
		}
	}
}

// The four launches take the same arguments.
template <typename Kernel>
static void launch_family(World& w, Kernel kernel, dim3 grid, dim3 block)
{
	hipLaunchKernelGGL(kernel, grid, block, 0, w.stream, w.dCounters.p, w.pairKeySorted.p, (const u64*)w.pairsSorted.p, w.colWorld.p, w.manifolds.p, w.epaList.p, w.gjkSimplex.p, w.hullInfo.p, w.hullVerts.p, (u32)w.pairCap);
}

void launch_gjk(World& w, u32 numPairs)
{
	dim3 grid((numPairs + 255) / 256), block(256);
	launch_family(w, k_gjk<0>, grid, block);
	if (!w.hulls.empty()) launch_family(w, k_gjk<1>, grid, block);
}

void launch_epa(World& w, u32 numPairs)
{
	// The waves stride over the hit list: launch exactly as many workgroups as are resident at once (registers allow 3 per CU, the 38.5 KB
	// of LDS would allow 4), or the last quarter of a 4-per-CU grid runs as a second, mostly empty round.
	static int epaPerCU[2] = { 0, 0 }; static int numCUs = 0;
	if (!numCUs)
	{
		hipDeviceProp_t prop; MI_CHECK(hipGetDeviceProperties(&prop, w.device)); numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
		MI_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&epaPerCU[0], k_epa<0>, 64 * EPA_WAVES_PER_BLOCK, 0));
		MI_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&epaPerCU[1], k_epa<1>, 64 * EPA_WAVES_PER_BLOCK, 0));
		for (int& v : epaPerCU) if (v < 1) v = 3;
	}
	const u32 wanted = (numPairs + EPA_WAVES_PER_BLOCK - 1) / EPA_WAVES_PER_BLOCK;
	launch_family(w, k_epa<0>, dim3(std::min<u32>(wanted, (u32)(numCUs * epaPerCU[0]))), dim3(64 * EPA_WAVES_PER_BLOCK));
	if (!w.hulls.empty()) launch_family(w, k_epa<1>, dim3(std::min<u32>(wanted, (u32)(numCUs * epaPerCU[1]))), dim3(64 * EPA_WAVES_PER_BLOCK));
}
