// mi_contact_query_batch: many volumes, each against every candidate collider of the world: the manifold the step's narrowphase would build
// for a collider of that shape at that pose ("Contact queries"; the rule is stated in include/mi_physics.h).  "A collider you
// ask once": overlap's volume, candidates and box test (overlap_volume.h), then the step's own per-pair functions (narrow_pairs.h,
// narrow_gjk.h, narrow_epa.h) on the two world records, in the step's structure but on scratch and counters of the query's own
// (World::queries.cq*): the step's pair list, manifolds, EPA lists and dCounters are neither read nor written.
//   (launch_raycast_build)     leaves, keys, sort, tree, fit; with MI_CONTACT_QUERY_BRUTE_FORCE the leaves alone
//   k_cq_candidates<.., false> one lane per query: the volume (ovVolume), then rcWalk counting the leaves whose exact box meets the volume's;
//                              the query takes a segment of the pair list (one atomicAdd per query: where a segment lies depends on the
//                              order of the atomics, what it holds and what is reported from it do not)
//   (the host reads the 4-byte total and grows the scratch to it: no pair can be lost, whatever the world holds)
//   k_cq_candidates<.., true>  the same walk again, writing per pair {query, collider, body, key | who is operand A} and the two world
//                              records in operand order (A: the lower type, of equal types the volume)
//   k_cq_narrow<closed / box>  k_narrow's body over the list; box-box with the PolyStore columns in LDS, [i * 64 + lane]
//   k_cq_gjk<family>           k_gjk's body: misses and parallel cylinders finish here, hits go to the dense EPA work list
//   k_cq_epa<family>           k_epa's body: EPA_GROUP lanes per hit, polytopes in LDS, groups stride over the work list
//   k_cq_gather                one lane per query: its pairs with count > 0, the maxHits lowest collider indices ascending (kept by
//                              insertion in the segment's own slice of cqSort), the sign rule, the summary and the deepest contact
// Every pair writes its manifold to its own slot, so the work lists' order never reaches a result: two calls give the same bytes, and
// the tree and brute force differ only in the order of a segment, which the gather pass sorts away.
#include "world.h"
#include "collider_world.h"
#include "raycast_shared.h"
#include "overlap_volume.h"
#include "narrow_pairs.h"
#include "narrow_epa.h"
#include <algorithm>

// Words of the query's own counter block (World::queries.cqCounters, CTR_WORDS words, zeroed at every call).  The per-pair functions
// name the step's offsets (epaWave: CTR_NARROW_LIMITS), so the block has the step's layout; it uses these entries of it:
//   CTR_NUM_PAIRS        pairs (candidates whose box meets their volume's), the append cursor of the segments
//   CTR_EPA_COUNT(_HULL) GJK hits of the two families
//   CTR_NARROW_LIMITS    the GJK / EPA marks of this call
#define CQ_KEY_MASK 0xFFu
#define CQ_COLLIDER_IS_A 0x100u // in the key word of a pair: the candidate is operand A, the reported normal is flipped

template <bool FILL>
struct CqVisitor
{
	const OvQuery& q; const RcScene& sc; const float4* hullInfo;
	u32 query, base, room; uint4* pairs; ColliderRec* cols; u32 n;
	MI_DEV bool box(const float* b, float& key) const { key = 0.f; return ovBoxesMeet(q.mn, q.mx, v3(b[0], b[1], b[2]), v3(b[3], b[4], b[5])); } // (a NaN visits)
	MI_DEV void leaf(u32 c)
	{
		RcCollider col;
		if (!rcFetch(sc, c, q.ex, col)) return;
		ColliderRec o; V3 mn, mx;
		worldCollider(sc.cols[c], col.rot, col.pos, hullInfo, o, mn, mx);
		if (!ovBoxesMeet(q.mn, q.mx, mn, mx)) return;
		if (FILL && n < room) // (n < room always: both passes read the same world)
		{
			const u32 type = colType(o);
			const bool queryIsA = q.type <= type; // operand A: the lower type, of equal types the volume
			const ColliderRec A = ovPick(queryIsA, q.rec, o), B = ovPick(queryIsA, o, q.rec);
			const size_t j = (size_t)base + n;
			pairs[j] = make_uint4(query, c, col.reported, queryIsA ? pairKey(q.type, type) : (pairKey(type, q.type) | CQ_COLLIDER_IS_A));
			cols[2 * j] = A; cols[2 * j + 1] = B;
		}
		n++;
	}
};

// seg: per query {first pair, pairs, not switched off, 0}.  FILL == false writes it (and the world shapes), FILL == true reads it.
template <bool BRUTE, bool FILL>
__global__ void __launch_bounds__(64) k_cq_candidates(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ worldShapes, u32 built, RcScene sc,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, const float4* __restrict__ hullInfo, u32 numHulls,
	u32* __restrict__ counters, uint4* __restrict__ seg, uint4* __restrict__ pairs, ColliderRec* __restrict__ cols)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	uint4 s = make_uint4(0u, 0u, 0u, 0u);
	if (FILL) { s = seg[i]; if (!s.y) return; }
	OvQuery q;
	const bool on = ovVolume(i, queries, FILL ? nullptr : worldShapes, sc, alive, simMask, hullInfo, numHulls, q);
	if (!on) { if (!FILL) seg[i] = s; return; }
	CqVisitor<FILL> v{ q, sc, hullInfo, i, s.x, s.y, pairs, cols, 0u };
	const u32 n = built ? sc.hdr[RC_N] : 0u;
	if (n != 0u)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
	}
	if (!FILL) seg[i] = make_uint4(v.n ? atomicAdd(&counters[CTR_NUM_PAIRS], v.n) : 0u, v.n, 1u, 0u);
}

// ---- the pair passes: the bodies of k_narrow, k_gjk and k_epa (k_narrow_pairs.hip, k_narrow_gjk.hip) over the query's list ----
enum { CQ_CLOSED = 0, CQ_BOX = 1 };
template <int GROUP>
__global__ void __launch_bounds__(GROUP == CQ_CLOSED ? 256 : 64) k_cq_narrow(const u32* __restrict__ counters, const uint4* __restrict__ pairs, const ColliderRec* __restrict__ cols, ManifoldRec* __restrict__ manifolds)
{
	// the box kernel's clipping polygons: two per lane, 16 points each, point i of lane l at [i * 64 + l] (conflict-free 16-byte accesses)
	__shared__ float4 sPoly[GROUP == CQ_BOX ? 2 * 16 * 64 : 1];
	const PolyStore store = { sPoly + (GROUP == CQ_BOX ? threadIdx.x : 0u), sPoly + (GROUP == CQ_BOX ? 16u * 64u + threadIdx.x : 0u), 64u };
	const u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= counters[CTR_NUM_PAIRS]) return;
	const u32 key = pairs[slot].w & CQ_KEY_MASK;
	if (!(GROUP == CQ_CLOSED ? closedFormKey(key) : boxKey(key))) return;
	ColliderRec A = cols[2 * (size_t)slot], B = cols[2 * (size_t)slot + 1];
	Man m = emptyManifold();
	bool hit = false;
	if (GROUP == CQ_CLOSED)
	{
		switch (key)
		{
			case KEY_SPHERE_SPHERE: hit = sphereSphere(asSphere(A), asSphere(B), m); break;
			case KEY_SPHERE_CAPSULE: hit = sphereCapsule(asSphere(A), asCapsule(B), m); break;
			case KEY_SPHERE_CYLINDER: hit = sphereCylinder(asSphere(A), asCapsule(B), m); break;
			case KEY_SPHERE_AABB: hit = sphereBox(asSphere(A), asBox(B), m); break;
			case KEY_SPHERE_OBB: hit = sphereObb(asSphere(A), asObb(B), m); break;
			case KEY_CAPSULE_CAPSULE: hit = capsuleCapsule(asCapsule(A), asCapsule(B), m); break;
			case KEY_CAPSULE_CYLINDER: hit = capsuleCylinder(asCapsule(A), asCapsule(B), m); break;
			case KEY_AABB_AABB: hit = boxBoxAxisAligned(asBox(A), asBox(B), m); break;
		}
	}
	else
	{
		Obb oa;
		if (key == KEY_AABB_OBB) { Box b = asBox(A); oa.q = q4(0.f, 0.f, 0.f, 1.f); oa.c = boxCenter(b); oa.r = boxRadius(b); } // aabb -> obb
		else oa = asObb(A);
		hit = obbObb(oa, asObb(B), m, store);
	}
	writeManifold(manifolds, slot, m, hit, A, B, slot);
}

// listCap: the capacity of epaList (>= the pairs): the tube hits fill it from its start, the hull hits from its end, as in the step.
template <int FAMILY>
__global__ void __launch_bounds__(256) k_cq_gjk(u32* __restrict__ counters, const uint4* __restrict__ pairs, const ColliderRec* __restrict__ cols, ManifoldRec* __restrict__ manifolds,
	u32* __restrict__ epaList, float4* __restrict__ gjkSimplex, const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts, u32 listCap)
{
	const u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= counters[CTR_NUM_PAIRS]) return;
	const u32 key = pairs[slot].w & CQ_KEY_MASK;
	if (FAMILY == 0 ? !tubeKey(key) : !(hullKey(key) && key < KEY_HULL_END)) return;
	ColliderRec A = cols[2 * (size_t)slot], B = cols[2 * (size_t)slot + 1];
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
	if (iters > counters[CTR_NARROW_LIMITS]) atomicMax(&counters[CTR_NARROW_LIMITS], iters);
	if (!gjkHit)
	{
		Man m = emptyManifold();
		writeManifold(manifolds, slot, m, false, A, B, slot);
		return;
	}
	u32 j = atomicAdd(&counters[FAMILY == 0 ? CTR_EPA_COUNT : CTR_EPA_COUNT_HULL], 1u); // order of the work list does not affect any result
	if (FAMILY == 1) j = listCap - 1u - j;
	epaList[j] = slot;
	storeSimplex(gjkSimplex + (size_t)j * 9, sx);
}

template <int FAMILY>
__global__ void __launch_bounds__(64 * EPA_WAVES_PER_BLOCK) __attribute__((amdgpu_waves_per_eu(FAMILY == 0 ? 3 : 2, FAMILY == 0 ? 3 : 3))) k_cq_epa(u32* __restrict__ counters, const uint4* __restrict__ pairs,
	const ColliderRec* __restrict__ cols, ManifoldRec* __restrict__ manifolds, const u32* __restrict__ epaList, const float4* __restrict__ gjkSimplex,
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
		u32 key = pairs[slot].w & CQ_KEY_MASK;
		ColliderRec A = cols[2 * (size_t)slot], B = cols[2 * (size_t)slot + 1];
		SupShapes sh; Obb o;
		gjkOperands<FAMILY>(key, A, B, hullInfo, hullVerts, sh, o);
		GjkSimplex sx;
		loadSimplex(gjkSimplex + (size_t)j * 9, sx);
		V3 point, normal; float depth;
		epaWave<FAMILY>(e, lane, group * EPA_GROUP, sx, sh, point, normal, depth, counters);
		if (lane == 0)
		{
			Man m = emptyManifold();
			if (FAMILY == 1 || key == KEY_CYLINDER_CYLINDER) { m.n = normal; m.count = 1; m.p[0] = make_float4(point.x, point.y, point.z, depth); }
			else
			{
				const PolyStore store = { (float4*)e.tnx, (float4*)e.tnx + 16, 1u }; // the finished polytope's triangle arrays hold the two clipping polygons: LDS, not scratch
				capsuleBoxFinish(point, normal, depth, sh.tubeA, sh.box, m, store);
			}
			if (key == KEY_CAPSULE_OBB || key == KEY_CYLINDER_OBB) // back to world space
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

// ---- the gather pass ----
// out: per query 8 + 24 * maxHits words (zeroed by the launcher): {numContacts, numWritten, valid, 0, deepestCollider, deepestBody,
// deepestDepth, 0}, then maxHits x {collider, body, count, 0} {normal xyz, largest |depth|} 4 x {point xyz, depth}.  sorted: one uint2 per
// pair; a query keeps {collider, pair} of the maxHits lowest contacts so far in the first entries of its own segment, ascending.
__global__ void __launch_bounds__(64) k_cq_gather(u32 numQueries, u32 maxHits, const uint4* __restrict__ seg, const uint4* __restrict__ pairs, const ManifoldRec* __restrict__ manifolds,
	uint2* __restrict__ sorted, u32* __restrict__ out)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const uint4 s = seg[i];
	if (!s.z) return; // switched off: all zero
	u32* block = out + (size_t)i * (8u + 24u * (size_t)maxHits);
	uint2* list = sorted + s.x;
	u32 numContacts = 0u, numWritten = 0u, deepCollider = 0xFFFFFFFFu, deepBody = 0xFFFFFFFFu; float deepest = 0.f;
	for (u32 k = 0; k < s.y; ++k)
	{
		const u32 j = s.x + k;
		const u32 count = manifolds[j].ids.z;
		if (!count) continue;
		const uint4 p = pairs[j];
		float d = 0.f;
		for (u32 t = 0; t < 4u; ++t) if (t < count) d = fmaxf(d, fabsf(manifolds[j].p[t].w));
		if (d > deepest || (d == deepest && p.y < deepCollider)) { deepest = d; deepCollider = p.y; deepBody = p.z; }
		numContacts++;
		u32 at = numWritten;
		if (at == maxHits)
		{
			if (at == 0u || p.y > list[at - 1u].x) continue;
			at--; // the last one is displaced
		}
		else numWritten++;
		for (; at > 0u && list[at - 1u].x > p.y; --at) list[at] = list[at - 1u];
		list[at] = make_uint2(p.y, j);
	}
	for (u32 k = 0; k < numWritten; ++k)
	{
		const u32 j = list[k].y;
		const uint4 p = pairs[j];
		const ManifoldRec m = manifolds[j];
		const u32 flip = (p.w & CQ_COLLIDER_IS_A) ? 0x80000000u : 0u; // reported as if the volume were operand A: the sign bits of the normal and nothing else
		float d = 0.f;
		for (u32 t = 0; t < 4u; ++t) if (t < m.ids.z) d = fmaxf(d, fabsf(m.p[t].w));
		uint4* rec = (uint4*)(block + 8u + 24u * (size_t)k);
		rec[0] = make_uint4(p.y, p.z, m.ids.z, 0u);
		rec[1] = make_uint4(mi_f2u(m.nf.x) ^ flip, mi_f2u(m.nf.y) ^ flip, mi_f2u(m.nf.z) ^ flip, mi_f2u(d));
		for (u32 t = 0; t < 4u; ++t) rec[2 + t] = make_uint4(mi_f2u(m.p[t].x), mi_f2u(m.p[t].y), mi_f2u(m.p[t].z), mi_f2u(m.p[t].w));
	}
	block[0] = numContacts; block[1] = numWritten; block[2] = 1u; block[3] = 0u;
	block[4] = deepCollider; block[5] = deepBody; block[6] = mi_f2u(deepest); block[7] = 0u;
}

void launch_contact_query(World& w, u32 n, const mi_overlap_query* dQueries, u32 maxHits, u32 flags, void* dOut, float* dOutWorldShapes)
{
	World::Queries& Q = w.queries;
	const bool brute = (flags & MI_CONTACT_QUERY_BRUTE_FORCE) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_CONTACT_QUERY_STATIC) != 0, brute);
	if (built == RC_BUILD_FAILED) return;
	const u32 have = built == RC_BUILD_DONE ? 1u : 0u; // (no candidate collider: the kernels still form the world shapes and answer empty blocks)
	Q.cqCounters.ensure(CTR_WORDS, w.stream); Q.cqSeg.ensure(n, w.stream);
	if (w.lastError) return;
	MI_CHECK(hipMemsetAsync(Q.cqCounters.p, 0, sizeof(u32) * CTR_WORDS, w.stream));
	MI_CHECK(hipMemsetAsync(dOut, 0, (size_t)n * (32u + 96u * (size_t)maxHits), w.stream));
	const dim3 qGrid((n + 63) / 64), qBlock(64);
	const u32 numHulls = (u32)w.hulls.size();
	hipLaunchKernelGGL(HIP_KERNEL_NAME(brute ? k_cq_candidates<true, false> : k_cq_candidates<false, false>), qGrid, qBlock, 0, w.stream, n, (const float4*)dQueries, (float4*)dOutWorldShapes, have, rcScene(w),
		w.aliveMask.p, w.simMask.p, w.hullInfo.p, numHulls, Q.cqCounters.p, Q.cqSeg.p, (uint4*)nullptr, (ColliderRec*)nullptr);
	// the one read-back of a call: 4 bytes, the number of pairs, which sizes the scratch and the grids of the pair passes
	u32 total = 0;
	MI_CHECK(hipMemcpyAsync(&total, Q.cqCounters.p + CTR_NUM_PAIRS, sizeof(u32), hipMemcpyDeviceToHost, w.stream));
	MI_CHECK(hipStreamSynchronize(w.stream));
	if (w.lastError) return;
	if (total)
	{
		Q.cqPairs.ensure(total, w.stream); Q.cqCols.ensure(2 * (size_t)total, w.stream); Q.cqManifolds.ensure(total, w.stream);
		Q.cqEpaList.ensure(total, w.stream); Q.cqSimplex.ensure(9 * (size_t)total, w.stream); Q.cqSorted.ensure(total, w.stream);
		if (w.lastError) return;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(brute ? k_cq_candidates<true, true> : k_cq_candidates<false, true>), qGrid, qBlock, 0, w.stream, n, (const float4*)dQueries, (float4*)nullptr, have, rcScene(w),
			w.aliveMask.p, w.simMask.p, w.hullInfo.p, numHulls, Q.cqCounters.p, Q.cqSeg.p, Q.cqPairs.p, Q.cqCols.p);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cq_narrow<CQ_CLOSED>), dim3((total + 255) / 256), dim3(256), 0, w.stream, Q.cqCounters.p, Q.cqPairs.p, Q.cqCols.p, Q.cqManifolds.p);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cq_narrow<CQ_BOX>), dim3((total + 63) / 64), dim3(64), 0, w.stream, Q.cqCounters.p, Q.cqPairs.p, Q.cqCols.p, Q.cqManifolds.p);
		static int numCUs = 0;
		if (!numCUs) { hipDeviceProp_t prop; MI_CHECK(hipGetDeviceProperties(&prop, w.device)); numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }
		// (the EPA groups stride over the hit list: no more workgroups than are resident at once, 3 per CU by their registers, as in launch_epa)
		const dim3 gjkGrid((total + 255) / 256), epaGrid(std::min<u32>((total + EPA_WAVES_PER_BLOCK * EPA_PER_WAVE - 1) / (EPA_WAVES_PER_BLOCK * EPA_PER_WAVE), (u32)numCUs * 3u));
		const u32 listCap = (u32)std::min(Q.cqEpaList.cap, Q.cqSimplex.cap / 9); // (>= total: both were grown to it)
		for (int family = 0; family < (numHulls ? 2 : 1); ++family)
		{
			hipLaunchKernelGGL(HIP_KERNEL_NAME(family == 0 ? k_cq_gjk<0> : k_cq_gjk<1>), gjkGrid, dim3(256), 0, w.stream, Q.cqCounters.p, Q.cqPairs.p, Q.cqCols.p, Q.cqManifolds.p,
				Q.cqEpaList.p, Q.cqSimplex.p, w.hullInfo.p, w.hullVerts.p, listCap);
			hipLaunchKernelGGL(HIP_KERNEL_NAME(family == 0 ? k_cq_epa<0> : k_cq_epa<1>), epaGrid, dim3(64 * EPA_WAVES_PER_BLOCK), 0, w.stream, Q.cqCounters.p, Q.cqPairs.p, Q.cqCols.p, Q.cqManifolds.p,
				Q.cqEpaList.p, Q.cqSimplex.p, w.hullInfo.p, w.hullVerts.p, listCap);
		}
	}
	hipLaunchKernelGGL(k_cq_gather, qGrid, qBlock, 0, w.stream, n, maxHits, Q.cqSeg.p, Q.cqPairs.p, Q.cqManifolds.p, Q.cqSorted.p, (u32*)dOut);
}
