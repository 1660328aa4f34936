// GJK for the narrowphase: support functions, the operands of one instance by bucket key, the simplex walk.  What the GJK / EPA
// kernels (k_narrow_gjk.hip) and the boolean zone overlap test (k_narrow_zone.hip) share.
// GJK + EPA for a tube (capsule / cylinder) vs an axis-aligned box or a cylinder — collision_gjk.h:17-61,140-238;
// collision_gjk.cpp:6-212.
#pragma once
#include "narrow.h"

#define GJK_MAX_ITERATIONS 64

struct SupportPoint { V3 a, b, mk; };
struct GjkSimplex { SupportPoint a, b, c, d; u32 numPoints; };

MI_DEV V3 capsuleSupport(const Capsule& c, V3 dir)
{
	float distA = dot(dir, c.a), distB = dot(dir, c.b);
	V3 farther = distA > distB ? c.a : c.b;
	return normalize(dir) * c.r + farther;
}
MI_DEV V3 cylinderSupport(const Capsule& c, V3 dir) // collision_gjk.h:30-46
{
	float distA = dot(dir, c.a), distB = dot(dir, c.b);
	V3 farther = distA > distB ? c.a : c.b;
	V3 n = c.a - c.b;
	V3 projectedDir = noz(cross(cross(n, dir), n));
	return farther + projectedDir * c.r;
}
MI_DEV V3 boxSupport(const Box& b, V3 dir) { return v3((dir.x < 0.f) ? b.lo.x : b.hi.x, (dir.y < 0.f) ? b.lo.y : b.hi.y, (dir.z < 0.f) ? b.lo.z : b.hi.z); }
MI_DEV V3 hullSupport(const Hull& h, const float4* __restrict__ hullVerts, V3 dir) // collision_gjk.h:77-100: first vertex with the largest dot product
{
	dir = conjugate(h.q) * dir;
	V3 result = v3s(0.f);
	float maxDist = -MI_FLT_MAX;
	for (u32 i = 0; i < h.count; ++i)
	{
		V3 v = v3f4(hullVerts[h.first + i]);
		float d = dot(dir, v);
		if (d > maxDist) { maxDist = d; result = v; }
	}
	return h.pos + h.q * result;
}
// The two convex shapes of one GJK/EPA instance.  A: capsule, cylinder, sphere (tubeA.a = centre), axis-aligned box, OBB or hull;
// B: axis-aligned box, cylinder or hull.
enum { SUP_CAPSULE = 0, SUP_CYLINDER = 1, SUP_SPHERE = 2, SUP_BOX = 3, SUP_OBB = 4, SUP_HULL = 5 };
struct SupShapes { Capsule tubeA, tubeB; Box box, boxA; Obb obbA; Hull hullA, hullB; u32 kindA, kindB; const float4* hullVerts; };
// FAMILY 0: tube (capsule / cylinder) vs box or cylinder — the pairs of the BASELINE configs; FAMILY 1: anything vs hull.  Separate
// kernel instances: with the family fixed at compile time the unused shapes drop out of the registers (one build for everything
// needed 256 VGPRs and halved the occupancy of the tube pairs).
template <int FAMILY>
MI_DEV V3 supportA(const SupShapes& sh, V3 dir)
{
	if (FAMILY == 0) return (sh.kindA == SUP_CYLINDER) ? cylinderSupport(sh.tubeA, dir) : capsuleSupport(sh.tubeA, dir);
	switch (sh.kindA)
	{
		case SUP_CAPSULE: return capsuleSupport(sh.tubeA, dir);
		case SUP_CYLINDER: return cylinderSupport(sh.tubeA, dir);
		case SUP_SPHERE: return normalize(dir) * sh.tubeA.r + sh.tubeA.a; // collision_gjk.h:6-15
		case SUP_BOX: return boxSupport(sh.boxA, dir);
		case SUP_OBB: return obbSupport(sh.obbA, dir);
		default: return hullSupport(sh.hullA, sh.hullVerts, dir);
	}
}
template <int FAMILY>
MI_DEV SupportPoint supportPair(const SupShapes& sh, V3 dir)
{
	SupportPoint s;
	s.a = supportA<FAMILY>(sh, dir);
	if (FAMILY == 0) s.b = (sh.kindB == SUP_BOX) ? boxSupport(sh.box, -dir) : cylinderSupport(sh.tubeB, -dir);
	else s.b = hullSupport(sh.hullB, sh.hullVerts, -dir);
	s.mk = s.a - s.b;
	return s;
}
MI_DEV V3 crossABA(V3 a, V3 b) { return cross(cross(a, b), a); }

// returns 0 = stop, 1 = continue, 2 = error
MI_DEV int updateGJKSimplex(GjkSimplex& s, const SupportPoint& a, V3& dir)
{
	if (s.numPoints == 2)
	{
		V3 ao = -a.mk, ab = s.b.mk - a.mk, ac = s.c.mk - a.mk;
		V3 abc = cross(ab, ac);
		V3 abp = cross(ab, abc);
		if (dot(ao, abp) > 0.f) { s.c = a; dir = crossABA(ab, ao); return 1; }
		V3 acp = cross(abc, ac);
		if (dot(ao, acp) > 0.f) { s.b = a; dir = crossABA(ac, ao); return 1; }
		if (dot(ao, abc) >= 0.f) { s.d = s.b; s.b = a; s.numPoints = 3; dir = abc; return 1; }
		if (dot(ao, -abc) >= 0.f) { s.d = s.c; s.c = s.b; s.b = a; s.numPoints = 3; dir = -abc; return 1; }
		return 2;
	}
	if (s.numPoints == 3)
	{
		V3 ao = -a.mk, ab = s.b.mk - a.mk, ac = s.c.mk - a.mk, ad = s.d.mk - a.mk;
		V3 bcd = cross(s.c.mk - s.b.mk, s.d.mk - s.b.mk);
		if (dot(bcd, dir) > 0.00001f || dot(bcd, s.b.mk) < -0.00001f) return 2;
		V3 abc = cross(ac, ab), abd = cross(ab, ad), adc = cross(ad, ac);
		const int ABC = 1, ABD = 2, ADC = 4;
		int flags = 0;
		flags |= (dot(abc, ao) > 0.f) ? ABC : 0;
		flags |= (dot(abd, ao) > 0.f) ? ABD : 0;
		flags |= (dot(adc, ao) > 0.f) ? ADC : 0;
		if (flags == (ABC | ABD | ADC)) return 2;
		if (flags == 0) return 0;
		// The reference's goto web (collision_gjk.cpp:95-205) as a small state machine: entry = (face, first|second test).
		int face, second = 0;
		if (flags == ABC) { face = ABC; }
		else if (flags == ABD) { face = ABD; }
		else if (flags == ADC) { face = ADC; }
		else if (flags == (ABC | ABD)) { if (dot(cross(abc, ab), ao) > 0.f) { face = ABD; } else { face = ABC; second = 1; } }
		else if (flags == (ABD | ADC)) { if (dot(cross(abd, ad), ao) > 0.f) { face = ADC; } else { face = ABD; second = 1; } }
		else { if (dot(cross(adc, ac), ao) > 0.f) { face = ABC; } else { face = ADC; second = 1; } }
		if (face == ABC)
		{
			if (!second && dot(cross(abc, ab), ao) > 0.f) { s.c = a; s.numPoints = 2; dir = crossABA(ab, ao); return 1; }
			if (dot(cross(ac, abc), ao) > 0.f) { s.b = a; s.numPoints = 2; dir = crossABA(ac, ao); return 1; }
			s.d = a; dir = abc; return 1;
		}
		if (face == ABD)
		{
			if (!second && dot(cross(abd, ad), ao) > 0.f) { s.b = s.d; s.c = a; s.numPoints = 2; dir = crossABA(ad, ao); return 1; }
			if (dot(cross(ab, abd), ao) > 0.f) { s.c = a; s.numPoints = 2; dir = crossABA(ab, ao); return 1; }
			s.c = a; dir = abd; return 1;
		}
		{
			if (!second && dot(cross(adc, ac), ao) > 0.f) { s.b = a; s.numPoints = 2; dir = crossABA(ac, ao); return 1; }
			if (dot(cross(ad, adc), ao) > 0.f) { s.b = a; s.c = s.d; s.numPoints = 2; dir = crossABA(ad, ao); return 1; }
			s.b = a; dir = adc; return 1;
		}
	}
	return 2;
}

// COUNT: *iters = loop entries, counted as the oracle's g_gjkMaxItersSeen counts them (0 when a first support point already separates)
template <int FAMILY, bool COUNT = false>
MI_DEV bool gjkPair(const SupShapes& sh, GjkSimplex& sx, u32* iters = nullptr)
{
	if (COUNT) *iters = 0;
	V3 dir = v3(1.f, 0.1f, -0.2f);
	sx.c = supportPair<FAMILY>(sh, dir);
	if (dot(sx.c.mk, dir) < 0.f) return false;
	dir = -sx.c.mk;
	sx.b = supportPair<FAMILY>(sh, dir);
	if (dot(sx.b.mk, dir) < 0.f) return false;
	dir = crossABA(sx.c.mk - sx.b.mk, -sx.b.mk);
	sx.numPoints = 2;
	for (u32 it = 0; it < GJK_MAX_ITERATIONS; ++it)
	{
		if (COUNT) *iters = it + 1;
		if (sqlen(dir) < 0.0001f) return false;
		SupportPoint a = supportPair<FAMILY>(sh, dir);
		if (dot(a.mk, dir) < 0.f) return false;
		int res = updateGJKSimplex(sx, a, dir);
		if (res == 0) { sx.a = a; sx.numPoints = 4; return true; }
		if (res == 2) return false;
	}
	return false;
}

// Operands of one GJK/EPA instance by bucket key: capsule-aabb, capsule-obb, cylinder-cylinder, cylinder-aabb, cylinder-obb (the obb
// variants work in the box's frame, :771-790, :1024-1043), and x-hull for x = sphere, capsule, cylinder, aabb, obb, hull.
template <int FAMILY>
MI_DEV void gjkOperands(u32 key, const ColliderRec& A, const ColliderRec& B, const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts, SupShapes& sh, Obb& o)
{
	sh.hullVerts = hullVerts;
	sh.tubeA = asCapsule(A); sh.tubeB = sh.tubeA;
	sh.box.lo = v3s(0.f); sh.box.hi = v3s(0.f); sh.boxA = sh.box;
	sh.obbA.q = q4(0.f, 0.f, 0.f, 1.f); sh.obbA.c = v3s(0.f); sh.obbA.r = v3s(0.f);
	sh.hullA.q = sh.obbA.q; sh.hullA.pos = v3s(0.f); sh.hullA.first = 0; sh.hullA.count = 0; sh.hullB = sh.hullA;
	sh.kindA = (key >= KEY_CYLINDER_CYLINDER) ? SUP_CYLINDER : SUP_CAPSULE; sh.kindB = SUP_BOX; // (the tube family's keys from cylinder-cylinder on have typeA = cylinder)
	if (FAMILY == 1) // x vs hull
	{
		sh.kindB = SUP_HULL; sh.hullB = asHull(B, hullInfo);
		switch (key / 6) // typeA
		{
			case MI_SPHERE: { Sphere s = asSphere(A); sh.kindA = SUP_SPHERE; sh.tubeA.a = s.c; sh.tubeA.b = s.c; sh.tubeA.r = s.r; } break;
			case MI_CAPSULE: sh.kindA = SUP_CAPSULE; break;
			case MI_CYLINDER: sh.kindA = SUP_CYLINDER; break;
			case MI_AABB: sh.kindA = SUP_BOX; sh.boxA = asBox(A); break;
			case MI_OBB: sh.kindA = SUP_OBB; sh.obbA = asObb(A); break;
			default: sh.kindA = SUP_HULL; sh.hullA = asHull(A, hullInfo); break;
		}
		return;
	}
	if (key == KEY_CYLINDER_CYLINDER) { sh.kindB = SUP_CYLINDER; sh.tubeB = asCapsule(B); return; }
	if (key == KEY_CAPSULE_AABB || key == KEY_CYLINDER_AABB) { sh.box = asBox(B); return; }
	o = asObb(B);
	sh.box.lo = o.c - o.r; sh.box.hi = o.c + o.r;
	Capsule c_; c_.a = conjugate(o.q) * (sh.tubeA.a - o.c) + o.c; c_.b = conjugate(o.q) * (sh.tubeA.b - o.c) + o.c; c_.r = sh.tubeA.r;
	sh.tubeA = c_;
}
