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
#include "world.h"
#include "collider_world.h"
#include "zone_overlap.h"
#include "raycast_shared.h"

struct OvQuery { ColliderRec rec; V3 mn, mx; u32 type; RcExclude ex; };
// The row of one query: {numOverlaps, numWritten, valid, reserved} and maxHits x {collider, body}, ascending in the collider index.
struct OvRow { u32* hits; u32 maxHits, numOverlaps, numWritten; };

// Shape words mi_add_collider takes for a type: the rest of the record is zero, as it is for a collider of the world.
MI_DEV u32 ovShapeWords(u32 type) { return type == MI_SPHERE ? 4u : ((type == MI_CAPSULE || type == MI_CYLINDER) ? 7u : (type == MI_AABB ? 6u : (type == MI_HULL ? 8u : 10u))); }

// The broadphase's comparison (k_broad.hip, aabbOverlap; reference aabbVsAABB): inclusive.
MI_DEV bool ovBoxesMeet(V3 amin, V3 amax, V3 bmin, V3 bmax)
{
	if (amax.x < bmin.x || amin.x > bmax.x) return false;
	if (amax.y < bmin.y || amin.y > bmax.y) return false;
	if (amax.z < bmin.z || amin.z > bmax.z) return false;
	return true;
}

// a or b, word by word.  (Not `c ? a : b` on the records themselves: a conditional between two lvalues selects an address, and a record whose
// address is taken stays in scratch.)
MI_DEV float4 ovPick(bool c, float4 a, float4 b) { return make_float4(c ? +a.x : +b.x, c ? +a.y : +b.y, c ? +a.z : +b.z, c ? +a.w : +b.w); }
MI_DEV ColliderRec ovPick(bool c, const ColliderRec& a, const ColliderRec& b) { ColliderRec r; r.a = ovPick(c, a.a, b.a); r.b = ovPick(c, a.b, b.b); r.c = ovPick(c, a.c, b.c); r.d = ovPick(c, a.d, b.d); return r; }

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
	const float4* Q = queries + 6 * (size_t)i;
	const float4 q0 = Q[0], q1 = Q[1], q2 = Q[2], q3 = Q[3], q4r = Q[4], q5 = Q[5];
	u32* block = out + (size_t)i * (4u + 2u * maxHits);
	for (u32 k = 0; k < 4u + 2u * maxHits; ++k) block[k] = 0u;

	OvQuery q; q.ex = RcExclude{ mi_f2u(q5.x), mi_f2u(q5.y) };
	const u32 type = mi_f2u(q2.z);
	bool on = mi_f2u(q2.w) != 0u && type < (u32)MI_TYPE_COUNT;
	if (on && type == MI_HULL) on = q1.w >= 0.f && q1.w < (float)numHulls && (u32)q1.w < numHulls; // (a NaN index fails the first comparison)
	V3 pos = v3(q3.x, q3.y, q3.z); Q4 rot = q4f4(q4r);
	if (on)
	{
		Q4 mrot; V3 mpos;
		const RcMount m = rcMount(mi_f2u(q3.w), sc.nb, sc.pose, alive, simMask, mrot, mpos);
		on = m != RC_MOUNT_OFF;
		if (m == RC_MOUNT_BODY) { pos = mrot * pos + mpos; rot = mrot * rot; }
	}
	q.mn = v3s(0.f); q.mx = v3s(0.f); q.type = 0u;
	if (on)
	{
		const float s[10] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y };
		const u32 n = ovShapeWords(type);
		float z[10];
		#pragma unroll
		for (u32 k = 0; k < 10u; ++k) z[k] = k < n ? s[k] : 0.f;
		ColliderRec local;
		local.a = make_float4(z[0], z[1], z[2], z[3]); local.b = make_float4(z[4], z[5], z[6], z[7]); local.c = make_float4(z[8], z[9], 0.f, 0.f);
		local.d = make_float4(mi_u2f(type), mi_u2f(MI_STATIC_BODY), 0.f, 0.f);
		worldCollider(local, rot, pos, hullInfo, q.rec, q.mn, q.mx);
		q.type = colType(q.rec);
		// (a NaN among the 8 corners of a box is dropped by fminf / fmaxf: what is left of such a box is finite but may be empty, min > max)
		on = isfinite(q.mn.x) && isfinite(q.mn.y) && isfinite(q.mn.z) && isfinite(q.mx.x) && isfinite(q.mx.y) && isfinite(q.mx.z) && q.mn.x <= q.mx.x && q.mn.y <= q.mx.y && q.mn.z <= q.mx.z;
	}
	if (worldShapes)
	{
		float4* W = worldShapes + 5 * (size_t)i;
		const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
		W[0] = ovPick(on, q.rec.a, zero); W[1] = ovPick(on, q.rec.b, zero);
		W[2] = ovPick(on, make_float4(q.rec.c.x, q.rec.c.y, mi_u2f(q.type), 0.f), zero);
		W[3] = ovPick(on, make_float4(q.mn.x, q.mn.y, q.mn.z, 0.f), zero); W[4] = ovPick(on, make_float4(q.mx.x, q.mx.y, q.mx.z, 0.f), zero);
	}
	if (!on) return;

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
