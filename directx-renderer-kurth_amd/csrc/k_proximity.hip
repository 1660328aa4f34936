// mi_proximity: many points, each against every candidate collider of the world: the nearest surface within a radius (signed distance,
// closest point, outward normal) and the number of colliders within it ("Proximity sensors"; the rule is stated in
// include/mi_physics.h, its float32 operation order in point_tests.h).  The candidates, their padded boxes and the tree over them are
// mi_raycast_batch's, rebuilt by launch_raycast_build (k_raycast.hip) in World::rc* at every call; only the walk differs: a range
// search pruned by the distance from the point to a node's box, not a ray walk pruned by slab intervals.
//   (launch_raycast_build)  leaves, keys, sort, tree, fit; with MI_PROX_BRUTE_FORCE the leaves alone
//   k_proximity             one lane per query: the world point from the mount's current pose (its head), then nearer child first with
//                           a fixed stack in LDS; with MI_PROX_BRUTE_FORCE the same body walks every candidate flag of rcLeafBox
// The boxes only say which colliders need not be asked: a distance is decided by pointBodyCollider on the collider's LOCAL record and
// pose alone, so the tree and brute force agree in every byte.
#include "world.h"
#include "point_tests.h"
#include "raycast_shared.h"

// Slack of the pruning test: a node is skipped only if the float32 distance from the point to its padded box exceeds
// bound + PX_SLACK_ULPS ulps of (|point| + largest |coordinate| of the scene + largest leaf diagonal) + PX_SLACK_REL * bound.  DESIGN.md derives them.
#define PX_SLACK_ULPS 32.f
#define PX_SLACK_REL (1.f / 65536.f)
#define PX_NONE 0xFFFFFFFFu

struct PxQuery { V3 p; float radius, slackAbs; u32 exFirst, exCount; };
struct PxBest { float d; u32 col, body, within; V3 c, n; };

// Distance from p to the box b = {min xyz, max xyz}: 0 inside.  A NaN coordinate gives 0 on its axis (fmaxf drops it): such a node is visited.
MI_DEV float pxBoxDistance(V3 p, const float* b)
{
	const float gx = fmaxf(fmaxf(b[0] - p.x, p.x - b[3]), 0.f), gy = fmaxf(fmaxf(b[1] - p.y, p.y - b[4]), 0.f), gz = fmaxf(fmaxf(b[2] - p.z, p.z - b[5]), 0.f);
	return sqrtf(gx * gx + gy * gy + gz * gz);
}
// What a node's box distance is held against.  COUNT: every candidate within the radius has to be met.  Otherwise only one that beats or
// ties the best so far (a lower collider index may win the tie); never below 0, the distance of a box that contains the point.
template <bool COUNT>
MI_DEV float pxLimit(const PxQuery& q, const PxBest& best)
{
	const float bound = COUNT ? q.radius : fmaxf(fminf(q.radius, best.d), 0.f);
	return bound + (q.slackAbs + PX_SLACK_REL * bound);
}

template <bool COUNT>
MI_DEV void pxTestCollider(u32 c, const PxQuery& q, u32 nb, const float4* __restrict__ pose, const float4* __restrict__ colStaticPose, const ColliderRec* __restrict__ cols, const RcHulls& hulls, PxBest& best)
{
	const ColliderRec rec = cols[c];
	const u32 body = colBody(rec);
	if (body < nb && body - q.exFirst < q.exCount) return; // (static colliders are never excluded)
	const float4* P = (body < nb) ? (pose + 2 * body) : (colStaticPose + 2 * c);
	const Q4 rot = q4f4(P[1]); const V3 pos = v3f4(P[0]);
	const float s[10] = { rec.a.x, rec.a.y, rec.a.z, rec.a.w, rec.b.x, rec.b.y, rec.b.z, rec.b.w, rec.c.x, rec.c.y };
	const PtHit h = pointBodyCollider(conjugate(rot) * (q.p - pos), colType(rec), s, hulls);
	if (!(h.d <= q.radius)) return;
	if (COUNT) best.within++;
	if (best.col == PX_NONE || h.d < best.d || (h.d == best.d && c < best.col))
	{
		best.d = h.d; best.col = c; best.body = body < nb ? body : MI_STATIC_BODY;
		best.c = rot * h.c + pos; best.n = rot * h.n;
	}
}

// The n >= 1 candidates of the tree.  stack[k * stride]: the caller's RC_STACK entries.
template <bool COUNT>
MI_DEV void pxTraverse(const PxQuery& q, u32 n, const float4* __restrict__ nodes, const u32* __restrict__ vals, u32* stack, u32 stride, u32 nb, const float4* __restrict__ pose,
	const float4* __restrict__ colStaticPose, const ColliderRec* __restrict__ cols, const RcHulls& hulls, PxBest& best)
{
	u32 node = n == 1u ? (RC_LEAF | vals[0]) : 0u, sp = 0u;
	for (;;)
	{
		if (node & RC_LEAF) pxTestCollider<COUNT>(node & ~RC_LEAF, q, nb, pose, colStaticPose, cols, hulls, best);
		else
		{
			const float4 w0 = nodes[4 * node], w1 = nodes[4 * node + 1], w2 = nodes[4 * node + 2], w3 = nodes[4 * node + 3];
			const float bl[6] = { w0.x, w0.y, w0.z, w0.w, w1.x, w1.y }, br[6] = { w1.z, w1.w, w2.x, w2.y, w2.z, w2.w };
			const u32 idL = mi_f2u(w3.x), idR = mi_f2u(w3.y);
			const float dL = pxBoxDistance(q.p, bl), dR = pxBoxDistance(q.p, br), limit = pxLimit<COUNT>(q, best);
			const bool visitL = !(dL > limit), visitR = !(dR > limit); // (a tie and a NaN visit)
			if (visitL && visitR)
			{
				const bool leftFirst = dL <= dR;
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

// queries: 2 x float4 per query = mi_proximity_query {point.xyz, radius}, {mount, excludeFirst, excludeCount, enabled} (bits);
// out: 3 x float4 = mi_proximity_reading; worldPoints: NULL or 1 x float4 = {world point.xyz, radius}.  built == 0: no tree, nothing within.
template <bool BRUTE, bool COUNT>
__global__ void __launch_bounds__(64) k_proximity(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ out, float4* __restrict__ worldPoints, u32 built, u32 nb, u32 nc,
	const float4* __restrict__ pose, const float4* __restrict__ colStaticPose, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, const ColliderRec* __restrict__ cols, RcHulls hulls,
	const u32* __restrict__ hdr, const float4* __restrict__ nodes, const u32* __restrict__ vals, const float4* __restrict__ leafBox)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const float4 q0 = queries[2 * i], q1 = queries[2 * i + 1];
	const u32 mount = mi_f2u(q1.x);
	PxQuery q; q.p = v3(q0.x, q0.y, q0.z); q.radius = q0.w; q.exFirst = mi_f2u(q1.y); q.exCount = mi_f2u(q1.z);
	bool on = mi_f2u(q1.w) != 0u; // a mount that is no body, a deleted one, one simulated elsewhere: the query is off
	if (on && mount != MI_STATIC_BODY) // (MI_STATIC_BODY: already in world space, every bit as it came)
	{
		on = mount < nb && alive[mount] && simMask[mount];
		if (on) q.p = q4f4(pose[2 * mount + 1]) * q.p + v3f4(pose[2 * mount]);
	}
	if (worldPoints) worldPoints[i] = on ? make_float4(q.p.x, q.p.y, q.p.z, q.radius) : make_float4(0.f, 0.f, 0.f, 0.f);
	PxBest best; best.d = __builtin_inff(); best.col = PX_NONE; best.body = 0u; best.within = 0u; best.c = v3s(0.f); best.n = v3s(0.f);
	const u32 n = built ? hdr[RC_N] : 0u;
	if (on && q.radius >= 0.f && n != 0u) // (a negative or NaN radius finds nothing)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < nc; ++c) if (leafBox[2 * c].w != 0.f) pxTestCollider<COUNT>(c, q, nb, pose, colStaticPose, cols, hulls, best);
		}
		else
		{
			const V3 ap = vabs(q.p);
			q.slackAbs = PX_SLACK_ULPS * RC_EPS * (fmaxf(fmaxf(ap.x, ap.y), ap.z) + mi_u2f(hdr[RC_ABS]) + mi_u2f(hdr[RC_DIAG]));
			pxTraverse<COUNT>(q, n, nodes, vals, &stack[0][threadIdx.x], 64u, nb, pose, colStaticPose, cols, hulls, best);
		}
	}
	const bool found = best.col != PX_NONE;
	out[3 * i] = found ? make_float4(best.d, mi_u2f(best.col), mi_u2f(best.body), mi_u2f(1u)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 1] = found ? make_float4(best.c.x, best.c.y, best.c.z, mi_u2f(best.within)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 2] = found ? make_float4(best.n.x, best.n.y, best.n.z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <bool BRUTE, bool COUNT>
static void pxLaunch(World& w, u32 n, const mi_proximity_query* dQueries, mi_proximity_reading* dOut, float* dOutWorldPoints, bool built)
{
	const RcHulls hulls{ w.hullVerts.p, w.hullTris.p, w.hullTriRange.p };
	hipLaunchKernelGGL((k_proximity<BRUTE, COUNT>), dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, (float4*)dOut, (float4*)dOutWorldPoints, built ? 1u : 0u, w.nb, w.nc,
		w.pose.p, w.colStaticPose.p, w.aliveMask.p, w.simMask.p, w.colLocal.p, hulls, w.rcCount.p, (const float4*)w.rcNodes.p, w.rcValsSorted.p, w.rcLeafBox.p);
}

void launch_proximity(World& w, u32 n, const mi_proximity_query* dQueries, u32 flags, mi_proximity_reading* dOut, float* dOutWorldPoints)
{
	const bool brute = (flags & MI_PROX_BRUTE_FORCE) != 0, count = (flags & MI_PROX_COUNT) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_PROX_STATIC) != 0, brute);
	if (built == RC_BUILD_FAILED) return;
	const bool have = built == RC_BUILD_DONE; // (no candidate collider: the kernel still forms the world points and zeroes the readings)
	if (brute) { if (count) pxLaunch<true, true>(w, n, dQueries, dOut, dOutWorldPoints, have); else pxLaunch<true, false>(w, n, dQueries, dOut, dOutWorldPoints, have); }
	else { if (count) pxLaunch<false, true>(w, n, dQueries, dOut, dOutWorldPoints, have); else pxLaunch<false, false>(w, n, dQueries, dOut, dOutWorldPoints, have); }
}
