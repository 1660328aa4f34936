// The point-to-shape tests of mi_proximity (include/mi_physics.h states the rule; the reference has none): the signed Euclidean
// distance d from a point to a collider (negative inside), the closest surface point c and the outward unit normal n there, in the
// collider's LOCAL frame; the caller rotates c and n back by the pose.  This header is the one statement of the float32 operation
// order: every expression below is evaluated as written, left to right, compiled with -ffp-contract=off on either side like
// ray_tests.h; tests/proximity64.py restates it in numpy.
#pragma once
#include "mi_common.h"

struct PtHit { float d; V3 c, n; };

// unit(v) = v / |v|, and zero where |v| is 0 (noz's 1e-8 threshold would zero the normal 1e-4 m from a surface).
MI_DEV V3 ptUnit(V3 v) { const float l = length(v); return l > 0.f ? v / l : v3s(0.f); }

MI_DEV PtHit pointSphere(V3 p, V3 ce, float r)
{
	const V3 v = p - ce;
	PtHit h; h.d = length(v) - r; h.n = ptUnit(v); h.c = ce + r * h.n;
	return h;
}
// s is the sensor normal rule's (ray_normals.h capsuleNormal): 0 where a == b.
MI_DEV PtHit pointCapsule(V3 p, V3 a, V3 b, float r)
{
	const V3 ab = b - a;
	const float den = dot(ab, ab);
	const float s = den > 0.f ? clamp01(dot(p - a, ab) / den) : 0.f;
	return pointSphere(p, a + s * ab, r);
}
MI_DEV PtHit pointCylinder(V3 p, V3 a, V3 b, float r)
{
	const V3 u = ptUnit(b - a);
	const float h = length(b - a), y = dot(p - a, u);
	const V3 rho = (p - a) - y * u;
	const float l = length(rho);
	const float dax = fabsf(y - h * 0.5f) - h * 0.5f, drad = l - r;
	PtHit o;
	if (dax <= 0.f && drad <= 0.f)
	{
		if (dax > drad) // the nearer cap; a tie goes to the side
		{
			const bool top = y > h * 0.5f;
			o.d = dax; o.n = top ? u : -u; o.c = top ? p + (h - y) * u : p - y * u;
		}
		else { o.d = drad; o.n = ptUnit(rho); o.c = (a + y * u) + r * o.n; }
		return o;
	}
	o.c = (a + clampf(y, 0.f, h) * u) + (l > r ? r * ptUnit(rho) : rho);
	const V3 v = p - o.c;
	o.d = length(v); o.n = ptUnit(v);
	return o;
}
MI_DEV PtHit pointBox(V3 p, V3 lo, V3 hi)
{
	const V3 ce = (lo + hi) * 0.5f, e = (hi - lo) * 0.5f, q = p - ce;
	const float wx = fabsf(q.x) - e.x, wy = fabsf(q.y) - e.y, wz = fabsf(q.z) - e.z;
	PtHit o;
	if (wx <= 0.f && wy <= 0.f && wz <= 0.f)
	{
		u32 k = 0; float best = wx;
		if (wy > best) { best = wy; k = 1; }
		if (wz > best) { best = wz; k = 2; }
		const float qk = k == 0 ? q.x : (k == 1 ? q.y : q.z), ek = k == 0 ? e.x : (k == 1 ? e.y : e.z), ck = k == 0 ? ce.x : (k == 1 ? ce.y : ce.z);
		const float s = qk < 0.f ? -1.f : 1.f, face = ck + s * ek; // (the sign of +0 and of -0 is positive)
		o.d = best;
		o.n = v3(k == 0 ? s : 0.f, k == 1 ? s : 0.f, k == 2 ? s : 0.f);
		o.c = v3(k == 0 ? face : p.x, k == 1 ? face : p.y, k == 2 ? face : p.z);
		return o;
	}
	o.c = ce + v3(clampf(q.x, -e.x, e.x), clampf(q.y, -e.y, e.y), clampf(q.z, -e.z, e.z));
	const V3 v = p - o.c;
	o.d = length(v); o.n = ptUnit(v);
	return o;
}
// Closest point of triangle (a, b, c) with unit normal n to p, by the regions of its vertices, edges and face (Ericson, Real-Time
// Collision Detection 5.1.5); in the face region the point is p moved along n onto the plane, not the barycentric sum.
MI_DEV V3 closestOnTriangle(V3 p, V3 a, V3 b, V3 c, V3 n)
{
	const V3 ab = b - a, ac = c - a, ap = p - a;
	const float d1 = dot(ab, ap), d2 = dot(ac, ap);
	if (d1 <= 0.f && d2 <= 0.f) return a;
	const V3 bp = p - b;
	const float d3 = dot(ab, bp), d4 = dot(ac, bp);
	if (d3 >= 0.f && d4 <= d3) return b;
	const float vc = d1 * d4 - d3 * d2;
	if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) return a + (d1 / (d1 - d3)) * ab;
	const V3 cp = p - c;
	const float d5 = dot(ab, cp), d6 = dot(ac, cp);
	if (d6 >= 0.f && d5 <= d6) return c;
	const float vb = d5 * d2 - d1 * d6;
	if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) return a + (d2 / (d2 - d6)) * ac;
	const float va = d3 * d6 - d5 * d4;
	if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b);
	return p - dot(ap, n) * n;
}
// Hull g in its own frame: inside or on it (the largest plane distance is <= 0) that plane, else the closest triangle; strict
// comparisons keep the lowest triangle index on a tie.  One pass over the triangles serves both.
template <typename Hull>
MI_DEV PtHit pointHull(V3 p, u32 g, const Hull& hull)
{
	float plane = -MI_FLT_MAX, dist = MI_FLT_MAX; V3 planeN = v3s(0.f), close = p;
	const u32 nt = hull.numTriangles(g);
	for (u32 f = 0; f < nt; ++f)
	{
		const V3 a = hull.vertex(g, f, 0), b = hull.vertex(g, f, 1), c = hull.vertex(g, f, 2);
		const V3 n = ptUnit(cross(b - a, c - a));
		const float pl = dot(p - a, n);
		if (pl > plane) { plane = pl; planeN = n; }
		const V3 cf = closestOnTriangle(p, a, b, c, n);
		const float df = length(p - cf);
		if (df < dist) { dist = df; close = cf; }
	}
	PtHit o;
	if (plane <= 0.f) { o.d = plane; o.n = planeN; o.c = p - plane * planeN; return o; }
	o.d = dist; o.c = close; o.n = ptUnit(p - close);
	return o;
}

// Collider (type, s = the 10 shape floats of its LOCAL record) against the point p in the body's frame.  An OBB and a hull are
// evaluated in the shape's own frame (p through the conjugate of the shape's quaternion) and c and n rotated back.
template <typename Hull>
MI_DEV PtHit pointBodyCollider(V3 p, u32 type, const float* s, const Hull& hull)
{
	switch (type)
	{
		case MI_SPHERE: return pointSphere(p, v3(s[0], s[1], s[2]), s[3]);
		case MI_CAPSULE: return pointCapsule(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6]);
		case MI_CYLINDER: return pointCylinder(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6]);
		case MI_AABB: return pointBox(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]));
		case MI_OBB:
		{
			const Q4 q = q4(s[0], s[1], s[2], s[3]); const V3 ce = v3(s[4], s[5], s[6]), ra = v3(s[7], s[8], s[9]);
			PtHit h = pointBox(conjugate(q) * (p - ce), v3s(0.f) - ra, ra);
			h.c = q * h.c + ce; h.n = q * h.n;
			return h;
		}
		case MI_HULL:
		{
			const Q4 q = q4(s[0], s[1], s[2], s[3]); const V3 hp = v3(s[4], s[5], s[6]);
			PtHit h = pointHull(conjugate(q) * (p - hp), (u32)s[7], hull);
			h.c = q * h.c + hp; h.n = q * h.n;
			return h;
		}
		default: { PtHit h; h.d = MI_FLT_MAX; h.c = p; h.n = v3s(0.f); return h; }
	}
}
