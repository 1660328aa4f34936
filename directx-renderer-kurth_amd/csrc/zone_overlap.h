// The boolean overlap test of two world collider records, all 36 pairings: overlapCheck, collision_narrow.cpp:1593-1689, over the
// boolean tests of bounding_volumes.h:301-363 and bounding_volumes.cpp:704-835, 1079-1244.  What the step asks for a rigid body against
// a force-field / trigger collider (k_narrow_zone.hip) and what an overlap query asks for its volume against a candidate (k_overlap.hip).
// tests/zone64.py documents its properties in float64.
#pragma once
#include "narrow_gjk.h"

MI_DEV bool ovSphereSphere(V3 ca, float ra, V3 cb, float rb) { V3 d = ca - cb; float dist2 = dot(d, d); float radiusSum = ra + rb; return dist2 <= radiusSum * radiusSum; }
MI_DEV bool ovSphereCylinder(V3 sc, float sr, Capsule c) // bounding_volumes.cpp:704-724
{
	V3 ab = c.b - c.a;
	float t = dot(sc - c.a, ab) / sqlen(ab);
	if (t >= 0.f && t <= 1.f) return ovSphereSphere(sc, sr, lerp(c.a, c.b, t), c.r);
	V3 p = (t <= 0.f) ? c.a : c.b;
	V3 up = (t <= 0.f) ? -ab : ab;
	V3 projectedDirToCenter = normalize(cross(cross(up, sc - p), up));
	V3 endA = p + projectedDirToCenter * c.r;
	V3 endB = p - projectedDirToCenter * c.r;
	V3 closestToSphere = closestPointSegment(sc, endA, endB);
	float sqDistance = sqlen(closestToSphere - sc);
	return sqDistance <= sr; // sic (:723)
}
MI_DEV bool ovSphereBox(V3 sc, float sr, Box a) // bounding_volumes.h:320-326
{
	V3 p = v3(fminf(fmaxf(sc.x, a.lo.x), a.hi.x), fminf(fmaxf(sc.y, a.lo.y), a.hi.y), fminf(fmaxf(sc.z, a.lo.z), a.hi.z));
	V3 n = p - sc;
	return sqlen(n) <= sr * sr;
}
MI_DEV bool ovObbObb(const Obb& a, const Obb& b) // bounding_volumes.cpp:1079-1199
{
	V3 ax = a.q * v3(1.f, 0.f, 0.f), ay = a.q * v3(0.f, 1.f, 0.f), az = a.q * v3(0.f, 0.f, 1.f);
	V3 bx = b.q * v3(1.f, 0.f, 0.f), by = b.q * v3(0.f, 1.f, 0.f), bz = b.q * v3(0.f, 0.f, 1.f);
	M3 r;
	r.m00 = dot(ax, bx); r.m10 = dot(ay, bx); r.m20 = dot(az, bx);
	r.m01 = dot(ax, by); r.m11 = dot(ay, by); r.m21 = dot(az, by);
	r.m02 = dot(ax, bz); r.m12 = dot(ay, bz); r.m22 = dot(az, bz);
	V3 tw = b.c - a.c;
	V3 t = conjugate(a.q) * tw;
	M3 absR;
	absR.m00 = fabsf(r.m00) + MI_EPSILON; absR.m10 = fabsf(r.m10) + MI_EPSILON; absR.m20 = fabsf(r.m20) + MI_EPSILON;
	absR.m01 = fabsf(r.m01) + MI_EPSILON; absR.m11 = fabsf(r.m11) + MI_EPSILON; absR.m21 = fabsf(r.m21) + MI_EPSILON;
	absR.m02 = fabsf(r.m02) + MI_EPSILON; absR.m12 = fabsf(r.m12) + MI_EPSILON; absR.m22 = fabsf(r.m22) + MI_EPSILON;
	float ra, rb;
	for (u32 i = 0; i < 3; ++i) { ra = vget(a.r, i); rb = dot(mrow(absR, i), b.r); if (ra + rb - fabsf(vget(t, i)) < 0.f) return false; }
	for (u32 i = 0; i < 3; ++i) { ra = dot(mcol(absR, i), a.r); rb = vget(b.r, i); float d = dot(mcol(r, i), t); if (ra + rb - fabsf(d) < 0.f) return false; }
#define MI_OV_EDGE(RA, RB, DIST) ra = RA; rb = RB; if (ra + rb - fabsf(DIST) < 0.f) return false;
	MI_OV_EDGE(a.r.y * absR.m20 + a.r.z * absR.m10, b.r.y * absR.m02 + b.r.z * absR.m01, t.z * r.m10 - t.y * r.m20)
	MI_OV_EDGE(a.r.y * absR.m21 + a.r.z * absR.m11, b.r.x * absR.m02 + b.r.z * absR.m00, t.z * r.m11 - t.y * r.m21)
	MI_OV_EDGE(a.r.y * absR.m22 + a.r.z * absR.m12, b.r.x * absR.m01 + b.r.y * absR.m00, t.z * r.m12 - t.y * r.m22)
	MI_OV_EDGE(a.r.x * absR.m20 + a.r.z * absR.m00, b.r.y * absR.m12 + b.r.z * absR.m11, t.x * r.m20 - t.z * r.m00)
	MI_OV_EDGE(a.r.x * absR.m21 + a.r.z * absR.m01, b.r.x * absR.m12 + b.r.z * absR.m10, t.x * r.m21 - t.z * r.m01)
	MI_OV_EDGE(a.r.x * absR.m22 + a.r.z * absR.m02, b.r.x * absR.m11 + b.r.y * absR.m10, t.x * r.m22 - t.z * r.m02)
	MI_OV_EDGE(a.r.x * absR.m10 + a.r.y * absR.m00, b.r.y * absR.m22 + b.r.z * absR.m21, t.y * r.m00 - t.x * r.m10)
	MI_OV_EDGE(a.r.x * absR.m11 + a.r.y * absR.m01, b.r.x * absR.m22 + b.r.z * absR.m20, t.y * r.m01 - t.x * r.m11)
	MI_OV_EDGE(a.r.x * absR.m12 + a.r.y * absR.m02, b.r.x * absR.m21 + b.r.y * absR.m20, t.y * r.m02 - t.x * r.m12)
#undef MI_OV_EDGE
	return true;
}
MI_DEV bool overlapColliders(u32 key, const ColliderRec& A, const ColliderRec& B, const float4* __restrict__ hullInfo, const float4* __restrict__ hullVerts)
{
	switch (key)
	{
		case KEY_SPHERE_SPHERE: { Sphere a = asSphere(A), b = asSphere(B); return ovSphereSphere(a.c, a.r, b.c, b.r); }
		case KEY_SPHERE_CAPSULE: { Sphere s = asSphere(A); Capsule c = asCapsule(B); return ovSphereSphere(s.c, s.r, closestPointSegment(s.c, c.a, c.b), c.r); }
		case KEY_SPHERE_CYLINDER: { Sphere s = asSphere(A); return ovSphereCylinder(s.c, s.r, asCapsule(B)); }
		case KEY_SPHERE_AABB: { Sphere s = asSphere(A); return ovSphereBox(s.c, s.r, asBox(B)); }
		case KEY_SPHERE_OBB: { Sphere s = asSphere(A); Obb o = asObb(B); Box b; b.lo = o.c - o.r; b.hi = o.c + o.r; return ovSphereBox(conjugate(o.q) * (s.c - o.c) + o.c, s.r, b); }
		case KEY_CAPSULE_CAPSULE: { Capsule a = asCapsule(A), b = asCapsule(B); V3 c1, c2; closestSegmentSegment(a.a, a.b, b.a, b.b, c1, c2); return ovSphereSphere(c1, a.r, c2, b.r); }
		case KEY_CAPSULE_CYLINDER: { Capsule a = asCapsule(A), b = asCapsule(B); V3 c1, c2; closestSegmentSegment(a.a, a.b, b.a, b.b, c1, c2); return ovSphereCylinder(c1, a.r, b); }
		case KEY_AABB_AABB: { Box a = asBox(A), b = asBox(B); return !(a.hi.x < b.lo.x || a.lo.x > b.hi.x || a.hi.y < b.lo.y || a.lo.y > b.hi.y || a.hi.z < b.lo.z || a.lo.z > b.hi.z); }
		case KEY_AABB_OBB: { Box b = asBox(A); Obb oa; oa.q = q4(0.f, 0.f, 0.f, 1.f); oa.c = boxCenter(b); oa.r = boxRadius(b); return ovObbObb(oa, asObb(B)); }
		case KEY_OBB_OBB: return ovObbObb(asObb(A), asObb(B));
		default: break;
	}
	SupShapes sh; Obb o; GjkSimplex sx;
	if (hullKey(key)) { gjkOperands<1>(key, A, B, hullInfo, hullVerts, sh, o); return gjkPair<1>(sh, sx); } // x vs hull (trigger / force-field checks are not counted in CTR_NARROW_LIMITS)
	if (tubeKey(key)) { gjkOperands<0>(key, A, B, hullInfo, hullVerts, sh, o); return gjkPair<0>(sh, sx); } // no closed form for parallel cylinders here (:790-797)
	return false;
}
