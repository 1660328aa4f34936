// mi_overlap_batch: many volumes, each against every candidate collider of the world: which colliders does the volume touch (DESIGN.md,
// "Overlap queries"; the rule is stated in include/mi_physics.h).  "A trigger you ask once": the verdict per candidate is the step's own
// two-stage decision for a trigger collider of that shape at that pose: the world boxes meet inclusively (the broadphase's comparison)
// and overlapColliders (zone_overlap.h) answers true on the two world records.  Both records and both boxes are built by worldCollider
// (collider_world.h), the function the step builds its colliders with, from the pose array the call itself reads.
//   (launch_raycast_build)  leaves, keys, sort, tree, fit; with MI_OVERLAP_BRUTE_FORCE the leaves alone
//   k_overlap               one lane per query: the volume's world pose from the mount's current pose (rcMount), its world record and box,
//                           then rcWalk with OvVisitor: a node is visited iff the volume's box meets its padded box; a leaf builds the
//                           candidate's world record and box, repeats the box test on the exact box and asks overlapColliders.  With
//                           MI_OVERLAP_BRUTE_FORCE the same leaf on every candidate flag of queries.leafBox.
// The padded leaf boxes only say which colliders need not be asked (DESIGN.md shows that they contain the step's boxes): the verdict is the
// leaf's alone, so the tree and brute force agree in every byte.  The hit list of a query is its row of dOut in global memory, kept
// ascending by insertion: the walk meets the candidates in tree order, and no per-lane array lands in scratch.
// (the volume itself, its world record and box, and the box test: overlap_volume.h, shared with k_contact_query.hip)
#include "world.h"
#include "collider_world.h"
#include "zone_overlap.h"
#include "raycast_shared.h"
#include "overlap_volume.h"

// The row of one query: {numOverlaps, numWritten, valid, reserved} and maxHits x {collider, body}, ascending in the collider index.
struct OvRow { u32* hits; u32 maxHits, numOverlaps, numWritten; };

// Collider c overlaps: count it, and keep it if it is among the maxHits lowest so far.
MI_DEV void ovInsert(OvRow& row, u32 c, u32 body)
{
	row.numOverlaps++;
	u32 k = row.numWritten;
	if (k == row.maxHits)
	{
		if (k == 0u || c > row.hits[2 * (k - 1u)]) return;
		k--; // the last one is displaced
	}
	else row.numWritten++;
	for (; k > 0u && row.hits[2 * (k - 1u)] > c; --k) { row.hits[2 * k] = row.hits[2 * (k - 1u)]; row.hits[2 * k + 1] = row.hits[2 * (k - 1u) + 1]; }
	row.hits[2 * k] = c; row.hits[2 * k + 1] = body;
}

// rcWalk's visitor of a volume.  Every node whose box the volume's box meets is visited: the order does not matter, the key is constant.
struct OvVisitor
{
	const OvQuery& q; const RcScene& sc; const float4* hullInfo; OvRow& row;
	MI_DEV bool box(const float* b, float& key) const { key = 0.f; return ovBoxesMeet(q.mn, q.mx, v3(b[0], b[1], b[2]), v3(b[3], b[4], b[5])); } // (a NaN visits)
	MI_DEV void leaf(u32 c)
	{
		RcCollider col;
		if (!rcFetch(sc, c, q.ex, col)) return;
		ColliderRec o; V3 mn, mx;
		worldCollider(sc.cols[c], col.rot, col.pos, hullInfo, o, mn, mx);
		if (!ovBoxesMeet(q.mn, q.mx, mn, mx)) return;
		const u32 type = colType(o);
		const bool queryIsA = q.type <= type; // operand A: the lower type, of equal types the volume
		const ColliderRec A = ovPick(queryIsA, q.rec, o), B = ovPick(queryIsA, o, q.rec); // (one instance of the test)
		if (overlapColliders(queryIsA ? pairKey(q.type, type) : pairKey(type, q.type), A, B, hullInfo, sc.hulls.verts)) ovInsert(row, c, col.reported);
	}
};

// queries: 6 x float4 per query = mi_overlap_query {shape[0..3]}, {shape[4..7]}, {shape[8], shape[9], type, enabled}, {pos.xyz, mount},
// {rot}, {excludeFirst, excludeCount, 0, 0} (integers as bits); out: per query 4 + 2 * maxHits words; worldShapes: NULL or 5 x float4.
// built == 0: no tree, nothing overlaps.
template <bool BRUTE>
__global__ void __launch_bounds__(64) k_overlap(u32 numQueries, const float4* __restrict__ queries, u32 maxHits, u32* __restrict__ out, float4* __restrict__ worldShapes, u32 built, RcScene sc,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, const float4* __restrict__ hullInfo, u32 numHulls)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	u32* block = out + (size_t)i * (4u + 2u * maxHits);
	for (u32 k = 0; k < 4u + 2u * maxHits; ++k) block[k] = 0u;

	OvQuery q;
	if (!ovVolume(i, queries, worldShapes, sc, alive, simMask, hullInfo, numHulls, q)) return;

	OvRow row{ block + 4, maxHits, 0u, 0u };
	OvVisitor v{ q, sc, hullInfo, row };
	const u32 n = built ? sc.hdr[RC_N] : 0u;
	if (n != 0u)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
	}
	block[0] = row.numOverlaps; block[1] = row.numWritten; block[2] = 1u;
}

void launch_overlap(World& w, u32 n, const mi_overlap_query* dQueries, u32 maxHits, u32 flags, void* dOut, float* dOutWorldShapes)
{
	const bool brute = (flags & MI_OVERLAP_BRUTE_FORCE) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_OVERLAP_STATIC) != 0, brute);
	if (built == RC_BUILD_FAILED) return;
	const u32 have = built == RC_BUILD_DONE ? 1u : 0u; // (no candidate collider: the kernel still forms the world shapes and answers empty lists)
	hipLaunchKernelGGL(brute ? k_overlap<true> : k_overlap<false>, dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, maxHits, (u32*)dOut, (float4*)dOutWorldShapes, have, rcScene(w),
		w.aliveMask.p, w.simMask.p, w.hullInfo.p, (u32)w.hulls.size());
}
