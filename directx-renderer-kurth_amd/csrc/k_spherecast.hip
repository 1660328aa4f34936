// mi_sphere_cast_batch: many swept spheres ("thick rays"), each against every candidate collider of the world: how far the sphere
// travels before its gap to a collider is down to the tolerance, and where and on what it touches ("Sphere casts"; the rule
// is stated in include/mi_physics.h, its float32 operation order in sphere_cast.h).  The candidates, their padded boxes and the tree
// over them are mi_raycast_batch's, rebuilt by launch_raycast_build (k_raycast.hip) in World::queries at every call.
//   (launch_raycast_build)  leaves, keys, sort, tree, fit; with MI_SPHERE_BRUTE_FORCE the leaves alone
//   k_sphere_cast           one lane per query: the world cast from the mount's current pose (rcMount), then rcWalk with ScVisitor: the
//                           ray's slab test (rcBoxTest) on the node's box grown by radius + tolerance + slack, and the march of
//                           sphere_cast.h at a leaf; with MI_SPHERE_BRUTE_FORCE the same leaf test on every candidate flag of queries.leafBox
// The boxes only say which colliders need not be asked: a candidate's answer is decided by sphereCastCollider on the collider's LOCAL
// record, its pose and the query alone.  The best hit so far only ends a march that is strictly beyond it and therefore cannot win,
// so the tree and brute force agree in every byte.
#include "world.h"
#include "sphere_cast.h"
#include "raycast_shared.h"

// What a node's box is grown by: radius + SC_GAP + SC_SLACK_ULPS ulps of (|origin| + largest |coordinate| of the scene + largest leaf
// diagonal + the length of the path within the scene + radius).  DESIGN.md derives it from the tolerance's guard.
#define SC_SLACK_ULPS 128.f
#define SC_NONE 0xFFFFFFFFu

struct ScQuery { RcRay ray; float radius, L, grow; RcExclude ex; };
struct ScBest { float t, gap; u32 col, body, hit, iterations; V3 c, n; };

// rcWalk's visitor of a swept sphere: a grown box is held against the closest hit so far by the ray's slab test (a box entered exactly
// at the bound and a NaN visit), a leaf may become the closest hit.
struct ScVisitor
{
	const ScQuery& q; const RcScene& sc; ScBest& best;
	MI_DEV bool box(const float* b, float& tEnter) const
	{
		const float grown[6] = { b[0] - q.grow, b[1] - q.grow, b[2] - q.grow, b[3] + q.grow, b[4] + q.grow, b[5] + q.grow };
		return rcBoxTest(q.ray, grown, fminf(q.ray.maxT, best.t), tEnter);
	}
	MI_DEV void leaf(u32 c)
	{
		RcCollider col;
		if (!rcFetch(sc, c, q.ex, col)) return;
		const ScHit h = sphereCastCollider(conjugate(col.rot) * (q.ray.r.origin - col.pos), conjugate(col.rot) * q.ray.r.direction, q.L, q.radius, q.ray.maxT, best.t,
			col.type, col.s, sc.hulls);
		if (h.hit != SC_HIT && h.hit != SC_UNRESOLVED) return;
		if (best.col == SC_NONE || h.t < best.t || (h.t == best.t && c < best.col))
		{
			best.t = h.t; best.gap = h.gap; best.col = c; best.body = col.reported; best.hit = h.hit; best.iterations = h.iterations;
			best.c = col.rot * h.c + col.pos; best.n = col.rot * h.n;
		}
	}
};

// queries: 3 x float4 per query = mi_sphere_cast {origin.xyz, maxT}, {direction.xyz, radius}, {mount, excludeFirst, excludeCount, enabled} (bits);
// out: 3 x float4 = mi_sphere_hit; worldCasts: NULL or 2 x float4 = {world origin.xyz, maxT}, {world direction.xyz, radius}.
// built == 0: no tree, every cast misses.
template <bool BRUTE>
__global__ void __launch_bounds__(64) k_sphere_cast(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ out, float4* __restrict__ worldCasts, u32 built, RcScene sc,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const float4 q0 = queries[3 * i], q1 = queries[3 * i + 1], q2 = queries[3 * i + 2];
	ScQuery q; q.ray.r = HRay{ v3(q0.x, q0.y, q0.z), v3(q1.x, q1.y, q1.z) }; q.ray.maxT = q0.w; q.radius = q1.w; q.ex = RcExclude{ mi_f2u(q2.y), mi_f2u(q2.z) };
	bool on = mi_f2u(q2.w) != 0u;
	if (on)
	{
		Q4 rot; V3 pos;
		const RcMount m = rcMount(mi_f2u(q2.x), sc.nb, sc.pose, alive, simMask, rot, pos);
		on = m != RC_MOUNT_OFF;
		if (m == RC_MOUNT_BODY) { q.ray.r.origin = rot * q.ray.r.origin + pos; q.ray.r.direction = rot * q.ray.r.direction; }
	}
	if (worldCasts)
	{
		const V3 o = q.ray.r.origin, d = q.ray.r.direction;
		worldCasts[2 * i] = on ? make_float4(o.x, o.y, o.z, q.ray.maxT) : make_float4(0.f, 0.f, 0.f, 0.f);
		worldCasts[2 * i + 1] = on ? make_float4(d.x, d.y, d.z, q.radius) : make_float4(0.f, 0.f, 0.f, 0.f);
	}
	q.L = length(q.ray.r.direction);
	ScBest best; best.t = __builtin_inff(); best.gap = 0.f; best.col = SC_NONE; best.body = 0u; best.hit = 0u; best.iterations = 0u; best.c = v3s(0.f); best.n = v3s(0.f);
	ScVisitor v{ q, sc, best };
	const u32 n = built ? sc.hdr[RC_N] : 0u;
	if (on && q.radius >= 0.f && q.ray.maxT >= 0.f && n != 0u) // (a negative or NaN radius and a negative or NaN maxT find nothing)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else
		{
			const float scene = mi_u2f(sc.hdr[RC_ABS]), diag = mi_u2f(sc.hdr[RC_DIAG]);
			const V3 ao = vabs(q.ray.r.origin);
			const float oMax = fmaxf(fmaxf(ao.x, ao.y), ao.z);
			const float reach = fminf(q.ray.maxT * q.L, 2.f * ((oMax + scene) + q.radius) + 1.f); // (inf * 0 = NaN: fminf keeps the other)
			q.grow = q.radius + (SC_GAP + SC_SLACK_ULPS * RC_EPS * ((((oMax + scene) + diag) + reach) + q.radius));
			rcPrepareRay(q.ray, scene, diag);
			rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
		}
	}
	const bool found = best.col != SC_NONE;
	out[3 * i] = found ? make_float4(best.t, mi_u2f(best.col), mi_u2f(best.body), mi_u2f(best.hit)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 1] = found ? make_float4(best.c.x, best.c.y, best.c.z, best.gap) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[3 * i + 2] = found ? make_float4(best.n.x, best.n.y, best.n.z, mi_u2f(best.iterations)) : make_float4(0.f, 0.f, 0.f, 0.f);
}

void launch_sphere_cast(World& w, u32 n, const mi_sphere_cast* dQueries, u32 flags, mi_sphere_hit* dOut, float* dOutWorldCasts)
{
	const bool brute = (flags & MI_SPHERE_BRUTE_FORCE) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_SPHERE_STATIC) != 0, brute);
	if (built == RC_BUILD_FAILED) return;
	const u32 have = built == RC_BUILD_DONE ? 1u : 0u; // (no candidate collider: the kernel still forms the world casts and zeroes the hits)
	hipLaunchKernelGGL(brute ? k_sphere_cast<true> : k_sphere_cast<false>, dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, (float4*)dOut, (float4*)dOutWorldCasts, have,
		rcScene(w), w.aliveMask.p, w.simMask.p);
}
