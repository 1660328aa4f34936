// The march of mi_sphere_cast_batch (include/mi_physics.h states the rule; the reference has none): how far a sphere of radius
// `radius` travels from o along v, in the collider's LOCAL frame, before its gap to the collider g(t) = pointBodyCollider(o + t v).d -
// radius has come down to the tolerance.  The signed distance to a convex shape is convex along a line and 1-Lipschitz; every step is
// the larger of the conservative advance g / L and the root of the chord through the last two samples, and neither passes the first
// contact in exact arithmetic ("Sphere casts").  This header is the one statement of the float32 operation order on top of
// point_tests.h: every expression below is evaluated as written, left to right, compiled with -ffp-contract=off on either side;
// tests/spherecast64.py restates it in numpy.
#pragma once
#include "point_tests.h"

#define SC_GAP 1e-4f        // a tenth of the solver's contact slop of 0.001 m
#define SC_GUARD_ULPS 16.f  // float32 guard of the tolerance, in ulps of |o| + t L + radius (derived in DESIGN.md)
#define SC_EPS 1.1920929e-7f
// The most samples one candidate took in tests/spherecast64.py's float32 restatement was 12 over its battery and 11 over 10 000 seeded
// random casts (spherecast64.measure_iterations): 12, doubled and rounded up to a power of two.
#define SC_MAX_ITER 32u

// hit of ScHit.  SC_BEATEN is no answer: the march went strictly beyond `beyond`, the t of a hit the caller already holds.
enum { SC_MISS = 0, SC_HIT = 1, SC_UNRESOLVED = 2, SC_BEATEN = 3 };
// t, gap = g(t) and the closest surface point c and outward normal n (local frame) at the last sample; iterations = samples taken.
struct ScHit { u32 hit; float t, gap; V3 c, n; u32 iterations; };

MI_DEV float scTol(float lenO, float t, float L, float radius) { return SC_GAP + (SC_GUARD_ULPS * SC_EPS) * ((lenO + t * L) + radius); }

// The march over any distance function dist(p) -> PtHit {d, c, n} that is convex along a line and 1-Lipschitz: a collider's signed
// distance (below) or the unsigned distance to one terrain triangle (terrain_point.h).
// L = |world direction|, formed once per query; maxT >= 0, radius >= 0 (the caller has sorted out the rest).
template <typename Dist>
MI_DEV ScHit sphereCastMarch(V3 o, V3 v, float L, float radius, float maxT, float beyond, const Dist& dist)
{
	ScHit h; h.hit = SC_MISS; h.t = 0.f; h.gap = 0.f; h.c = v3s(0.f); h.n = v3s(0.f); h.iterations = 0u;
	const float lenO = length(o);
	float t = 0.f, tPrev = 0.f, gPrev = 0.f;
	for (u32 it = 0; it < SC_MAX_ITER; ++it)
	{
		const PtHit p = dist(o + t * v);
		const float g = p.d - radius;
		h.t = t; h.gap = g; h.c = p.c; h.n = p.n; h.iterations = it + 1u;
		if (g <= scTol(lenO, t, L, radius)) { h.hit = SC_HIT; return h; } // (also an origin in touch or inside: t = 0, the gap negative)
		if (!(L > 0.f)) return h;                                           // a zero direction is an overlap test at the origin
		float step = g / L;                                                 // conservative advancement
		if (it > 0u)
		{
			const float slope = (g - gPrev) / (t - tPrev);
			if (slope >= 0.f) return h;                                     // receding: by convexity g does not come down again
			step = fmaxf(step, -g / slope);                                 // the chord's root
		}
		tPrev = t; gPrev = g;
		t = t + step;
		if (!(t <= maxT)) return h;
		if (t > beyond) { h.hit = SC_BEATEN; return h; }
	}
	h.hit = SC_UNRESOLVED;                                                  // free up to h.t, and the caller sees the flag
	return h;
}
// A collider (type, s = the 10 shape floats of its LOCAL record) in its own frame.
template <typename Hull>
MI_DEV ScHit sphereCastCollider(V3 o, V3 v, float L, float radius, float maxT, float beyond, u32 type, const float* s, const Hull& hull)
{
	return sphereCastMarch(o, v, L, radius, maxT, beyond, [&](V3 p) { return pointBodyCollider(p, type, s, hull); });
}
