// What the query kernels share (k_raycast.hip, k_raycast_sensors.hip, k_proximity.hip, k_spherecast.hip, k_interact.hip):
//   RcHulls     the hull geometry tables as the Hull argument of rayBodyCollider / pointBodyCollider
//   RcScene     what a walk over the world's colliders reads, as one kernel argument
//   rcFetch     collider c of the scene in its current frame, and whether a query's exclusion range hides it
//   rcMount     a query's mount index: off, world space, or the frame of a body
//   rcWalk      the walk over the tree k_raycast.hip builds in World::queries (its layout is declared here too), nearer child first
//   rcBoxTest   the slab test of a ray (RcRay, rcPrepareRay) against a node's box: the ray cast's and the sphere cast's box visitor
#pragma once
#include "world.h"
#include "ray_tests.h"

struct RcHulls
{
	const float4* verts; const uint4* tris; const uint2* range;
	MI_DEV u32 numTriangles(u32 g) const { return range[g].y; }
	MI_DEV V3 vertex(u32 g, u32 f, u32 k) const { uint4 t = tris[range[g].x + f]; return v3f4(verts[k == 0 ? t.x : (k == 1 ? t.y : t.z)]); }
};
inline RcHulls rcHulls(const World& w) { return RcHulls{ w.hullVerts.p, w.queries.hullTris.p, w.queries.hullTriRange.p }; } // (hullTris, hullTriRange: World::buildInteractTables)

// ---- header words of World::queries.count (zeroed before every build; every accumulated word has 0 as its neutral element) ----
enum
{
	RC_N = 0,        // candidates
	RC_NEG_MIN = 1,  // 3 words: max of rcOrdered(-centre): the lower bound of the box centres
	RC_MAX = 4,      // 3 words: max of rcOrdered(centre)
	RC_DIAG = 7,     // float bits: largest diagonal of a padded leaf box
	RC_ABS = 8,      // float bits: largest |coordinate| of a padded leaf box
	RC_HEADER = 16,  // the arrival counters of the internal nodes follow
};
#define RC_LEAF 0x80000000u
#define RC_NO_PARENT 0xFFFFFFFFu
#define RC_NOT_A_CANDIDATE (1u << 30)
#define RC_KEY_BITS 30
// Depth of the tree = length of the longest chain of internal nodes.  Going down, the length of the common prefix of a node's range
// grows strictly; the prefix is counted over the 30 key bits and then, for equal keys, over the 32 bits of the sorted position.  The
// root's range has a prefix of >= 0 key bits and a node with two different leaves one of <= 61, so a chain has <= 62 nodes, and
// the stack, which holds one pending sibling per node of the chain, <= 62 entries.
#define RC_STACK 64
static_assert(RC_KEY_BITS + 32 <= RC_STACK, "rcWalk's stack holds one entry per level of the tree: key bits + position bits");
#define RC_EPS 1.1920929e-7f
#define RC_NODE_WORDS 16u // one internal node: 64 bytes (k_raycast.hip describes the record)

// The bodies and colliders of the world at their current poses, and the tree over the candidates (hdr, nodes, vals, leafBox = World::queries.count,
// queries.nodes, queries.valsSorted, queries.leafBox: valid after launch_raycast_build).  Passed to the kernels by value.
struct RcScene
{
	u32 nb, nc;
	const float4* pose; const float4* colStaticPose; const ColliderRec* cols; RcHulls hulls;
	const u32* hdr; const float4* nodes; const u32* vals; const float4* leafBox;
};
inline RcScene rcScene(const World& w)
{
	return RcScene{ w.nb, w.nc, w.pose.p, w.colStaticPose.p, w.colLocal.p, rcHulls(w), w.queries.count.p, (const float4*)w.queries.nodes.p, w.queries.valsSorted.p, w.queries.leafBox.p };
}

// The shape words of a collider record in the order rayBodyCollider and pointBodyCollider read them.
MI_DEV void rcShape(const ColliderRec& rec, float* s)
{
	s[0] = rec.a.x; s[1] = rec.a.y; s[2] = rec.a.z; s[3] = rec.a.w; s[4] = rec.b.x; s[5] = rec.b.y; s[6] = rec.b.z; s[7] = rec.b.w; s[8] = rec.c.x; s[9] = rec.c.y;
}
// Collider c in its current frame: its body's pose, or its own if it is static.  reported: the body a hit names (MI_STATIC_BODY for a static collider).
struct RcCollider { u32 body, reported, type; Q4 rot; V3 pos; float s[10]; };
// The bodies b with b - first < count (unsigned) are no candidates of a query: the exclusion range of the sensors.
struct RcExclude { u32 first, count; };
// false: c belongs to a body of the range, nothing but col.body is loaded.  A static collider is never excluded.
MI_DEV bool rcFetch(const RcScene& sc, u32 c, RcExclude ex, RcCollider& col)
{
	const ColliderRec rec = sc.cols[c];
	col.body = colBody(rec);
	const bool dynamic = col.body < sc.nb;
	if (dynamic && col.body - ex.first < ex.count) return false;
	const float4* P = dynamic ? (sc.pose + 2 * col.body) : (sc.colStaticPose + 2 * c);
	col.rot = q4f4(P[1]); col.pos = v3f4(P[0]);
	col.reported = dynamic ? col.body : MI_STATIC_BODY; col.type = colType(rec);
	rcShape(rec, col.s);
	return true;
}

// Where a query given relative to `mount` lives.  RC_MOUNT_WORLD (MI_STATIC_BODY): in world space already, the caller passes every bit
// on as it came.  RC_MOUNT_OFF: the mount is no body, a deleted one or one simulated elsewhere.  RC_MOUNT_BODY: x -> rot * x + pos.
enum RcMount { RC_MOUNT_OFF, RC_MOUNT_WORLD, RC_MOUNT_BODY };
MI_DEV RcMount rcMount(u32 mount, u32 nb, const float4* __restrict__ pose, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, Q4& rot, V3& pos)
{
	if (mount == MI_STATIC_BODY) return RC_MOUNT_WORLD;
	if (!(mount < nb && alive[mount] && simMask[mount])) return RC_MOUNT_OFF;
	pos = v3f4(pose[2 * mount]); rot = q4f4(pose[2 * mount + 1]);
	return RC_MOUNT_BODY;
}

// Depth-first over the n >= 1 candidates of the scene's tree.  The visitor v brings
//   bool box(const float* b, float& key)   may the box b = {min xyz, max xyz} still matter, held against whatever bound v keeps?  Of two
//                                          children that do, the smaller key goes first, the left one on a tie
//   void leaf(u32 c)                       collider c is a candidate
// stack[k * stride]: the caller's RC_STACK entries.
template <class Visitor>
MI_DEV void rcWalk(Visitor& v, const RcScene& sc, u32 n, u32* stack, u32 stride)
{
	u32 node = n == 1u ? (RC_LEAF | sc.vals[0]) : 0u, sp = 0u;
	for (;;)
	{
		if (node & RC_LEAF) v.leaf(node & ~RC_LEAF);
		else
		{
			const float4 w0 = sc.nodes[4 * node], w1 = sc.nodes[4 * node + 1], w2 = sc.nodes[4 * node + 2], w3 = sc.nodes[4 * node + 3];
			const float bl[6] = { w0.x, w0.y, w0.z, w0.w, w1.x, w1.y }, br[6] = { w1.z, w1.w, w2.x, w2.y, w2.z, w2.w };
			const u32 idL = mi_f2u(w3.x), idR = mi_f2u(w3.y);
			float keyL, keyR;
			const bool visitL = v.box(bl, keyL), visitR = v.box(br, keyR);
			if (visitL && visitR)
			{
				const bool leftFirst = keyL <= keyR;
				if (sp < RC_STACK) stack[stride * sp++] = leftFirst ? idR : idL; // (sp < RC_STACK always: see RC_STACK)
				node = leftFirst ? idL : idR;
				continue;
			}
			if (visitL || visitR) { node = visitL ? idL : idR; continue; }
		}
		if (sp == 0u) break;
		node = stack[stride * --sp];
	}
}

// ---- the slab test of a ray against a node's box (k_raycast.hip, k_spherecast.hip) ----
// Slack of the slab test: RC_SLACK_ULPS ulps of (|origin| + largest |coordinate| of the scene) in space, RC_SLACK_REL of the distance
// in t.  DESIGN.md derives them.
#define RC_SLACK_ULPS 16.f
#define RC_SLACK_REL (1.f / 256.f)

struct RcRay
{
	HRay r; float maxT;
	V3 inv; bool par[3];        // 1 / direction; axes the ray does not move along are tested by containment
	float space, absT, relT;    // slack of the slab test: in space, in t, and the share of the largest leaf in the relative part
};
// May the ray hit something in this padded box at a distance in [0, tmax]?  Conservative: the interval is widened by the slack, a box
// entered exactly at tmax is visited (a lower collider index may win the tie), and a comparison with a NaN visits.  tEnter orders the visit.
MI_DEV bool rcBoxTest(const RcRay& q, const float* b, float tmax, float& tEnter)
{
	float tE = -MI_FLT_MAX, tX = MI_FLT_MAX; bool outside = false;
	const float o[3] = { q.r.origin.x, q.r.origin.y, q.r.origin.z }, inv[3] = { q.inv.x, q.inv.y, q.inv.z };
	#pragma unroll
	for (u32 a = 0; a < 3; ++a)
	{
		if (q.par[a]) outside = outside || o[a] < b[a] - q.space || o[a] > b[3 + a] + q.space;
		else { const float t1 = (b[a] - o[a]) * inv[a], t2 = (b[3 + a] - o[a]) * inv[a]; tE = fmaxf(tE, fminf(t1, t2)); tX = fminf(tX, fmaxf(t1, t2)); }
	}
	const float lo = tE - q.absT - RC_SLACK_REL * (fmaxf(tE, 0.f) + q.relT), hi = tX + q.absT + RC_SLACK_REL * (fabsf(tX) + q.relT);
	tEnter = tE;
	return !(outside || lo > tmax || hi < 0.f || lo > hi);
}

// The slack of the slab test for this ray (RcRay::inv ... relT); scene = largest |coordinate|, diag = largest diagonal of the leaf boxes.
MI_DEV void rcPrepareRay(RcRay& q, float scene, float diag)
{
	const V3 ad = vabs(q.r.direction), ao = vabs(q.r.origin);
	const float dMax = fmaxf(fmaxf(ad.x, ad.y), ad.z);
	q.par[0] = !(ad.x > 1e-12f * dMax); q.par[1] = !(ad.y > 1e-12f * dMax); q.par[2] = !(ad.z > 1e-12f * dMax);
	q.inv = v3(q.par[0] ? 0.f : 1.f / q.r.direction.x, q.par[1] ? 0.f : 1.f / q.r.direction.y, q.par[2] ? 0.f : 1.f / q.r.direction.z);
	q.space = RC_SLACK_ULPS * RC_EPS * (fmaxf(fmaxf(ao.x, ao.y), ao.z) + scene);
	q.absT = q.space * fmaxf(fmaxf(fabsf(q.inv.x), fabsf(q.inv.y)), fabsf(q.inv.z));
	q.relT = diag / length(q.r.direction);
}
