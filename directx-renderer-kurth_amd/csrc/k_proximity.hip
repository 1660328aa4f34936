// mi_proximity: many points, each against every candidate collider of the world: the nearest surface within a radius (signed distance,
// closest point, outward normal) and the number of colliders within it ("Proximity sensors"; the rule is stated in
// include/mi_physics.h, its float32 operation order in point_tests.h).  The candidates, their padded boxes and the tree over them are
// mi_raycast_batch's, rebuilt by launch_raycast_build (k_raycast.hip) in World::queries at every call; only the walk differs: a range
// search pruned by the distance from the point to a node's box, not a ray walk pruned by slab intervals.
//   (launch_raycast_build)  leaves, keys, sort, tree, fit; with MI_PROX_BRUTE_FORCE the leaves alone
//   k_proximity             one lane per query: the world point from the mount's current pose (rcMount), then rcWalk with PxVisitor,
//                           the box distance and the leaf test of a point; with MI_PROX_BRUTE_FORCE the same leaf test on every
//                           candidate flag of queries.leafBox.  rcMount, rcWalk, rcFetch and the RcScene argument: raycast_shared.h
// The boxes only say which colliders need not be asked: a distance is decided by pointBodyCollider on the collider's LOCAL record and
// pose alone, so the tree and brute force agree in every byte.
#include "proximity_shared.h" // PxQuery, PxBest, PxVisitor, pxBoxDistance: shared with the cloth's projection pass (k_cloth_collide.hip)

// queries: 2 x float4 per query = mi_proximity_query {point.xyz, radius}, {mount, excludeFirst, excludeCount, enabled} (bits);
// out: 3 x float4 = mi_proximity_reading; worldPoints: NULL or 1 x float4 = {world point.xyz, radius}.  built == 0: no tree, nothing within.
template <bool BRUTE, bool COUNT>
__global__ void __launch_bounds__(64) k_proximity(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ out, float4* __restrict__ worldPoints, u32 built, RcScene sc,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const float4 q0 = queries[2 * i], q1 = queries[2 * i + 1];
	PxQuery q; q.p = v3(q0.x, q0.y, q0.z); q.radius = q0.w; q.exFirst = mi_f2u(q1.y); q.exCount = mi_f2u(q1.z);
	bool on = mi_f2u(q1.w) != 0u;
	if (on)
	{
		Q4 rot; V3 pos;
		const RcMount m = rcMount(mi_f2u(q1.x), sc.nb, sc.pose, alive, simMask, rot, pos);
		on = m != RC_MOUNT_OFF;
		if (m == RC_MOUNT_BODY) q.p = rot * q.p + pos;
	}
	if (worldPoints) worldPoints[i] = on ? make_float4(q.p.x, q.p.y, q.p.z, q.radius) : make_float4(0.f, 0.f, 0.f, 0.f);
	PxBest best = pxBestNone();
	PxVisitor<COUNT> v{ q, sc, best, true }; // (the tree holds the static colliders iff the call wants them)
	const u32 n = built ? sc.hdr[RC_N] : 0u;
	if (on && q.radius >= 0.f && n != 0u) // (a negative or NaN radius finds nothing)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else
		{
			q.slackAbs = pxSlackAbs(q.p, sc);
			rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
		}
	}
	const bool found = best.col != PX_NONE;
	out[3 * i] = found ? make_float4(best.d, mi_u2f(best.col), mi_u2f(best.body), mi_u2f(1u)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 1] = found ? make_float4(best.c.x, best.c.y, best.c.z, mi_u2f(best.within)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 2] = found ? make_float4(best.n.x, best.n.y, best.n.z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

void launch_proximity(World& w, u32 n, const mi_proximity_query* dQueries, u32 flags, mi_proximity_reading* dOut, float* dOutWorldPoints)
{
	const bool brute = (flags & MI_PROX_BRUTE_FORCE) != 0, count = (flags & MI_PROX_COUNT) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_PROX_STATIC) != 0, brute);
	if (built == RC_BUILD_FAILED) return;
	const u32 have = built == RC_BUILD_DONE ? 1u : 0u; // (no candidate collider: the kernel still forms the world points and zeroes the readings)
	const auto kernel = brute ? (count ? k_proximity<true, true> : k_proximity<true, false>) : (count ? k_proximity<false, true> : k_proximity<false, false>);
	hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, (float4*)dOut, (float4*)dOutWorldPoints, have, rcScene(w), w.aliveMask.p, w.simMask.p);
}
