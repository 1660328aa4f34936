// The per-pair functions of the pairs that need no GJK: closed forms (reference collision_narrow.cpp:374-612, :1074-1140) and box-box SAT +
// Sutherland-Hodgman clipping (:1179-1527).  What the step's pair kernels (k_narrow_pairs.hip) and the contact query's (k_contact_query.hip) run: one text.
#pragma once
#include "narrow_clip.h"

// ---------------------------------------------------------------------------------------------------------------
// Closed-form pair kernels
// ---------------------------------------------------------------------------------------------------------------
MI_DEV bool sphereSphere(Sphere s1, Sphere s2, Man& m) // collision_narrow.cpp:374-400
{
	V3 n = s2.c - s1.c;
	float radiusSum = s2.r + s1.r;
	float sq = sqlen(n);
	if (sq <= radiusSum * radiusSum)
	{
		float distance;
		if (sq == 0.f) { distance = 0.f; m.n = v3(0.f, 1.f, 0.f); }
		else { distance = sqrtf(sq); m.n = n / distance; }
		m.count = 1;
		V3 pt = 0.5f * (s1.c + s1.r * m.n + s2.c - s2.r * m.n);
		m.p[0] = make_float4(pt.x, pt.y, pt.z, radiusSum - distance);
		return true;
	}
	return false;
}
MI_DEV bool sphereCapsule(Sphere s, Capsule c, Man& m) // :402-406
{
	Sphere s2; s2.c = closestPointSegment(s.c, c.a, c.b); s2.r = c.r;
	return sphereSphere(s, s2, m);
}
MI_DEV bool sphereBox(Sphere s, Box a, Man& m) // :451-478
{
	V3 p = v3(fminf(fmaxf(s.c.x, a.lo.x), a.hi.x), fminf(fmaxf(s.c.y, a.lo.y), a.hi.y), fminf(fmaxf(s.c.z, a.lo.z), a.hi.z)); // closestPoint_PointAABB
	V3 n = p - s.c;
	float sq = sqlen(n);
	if (sq <= s.r * s.r)
	{
		float dist = 0.f;
		if (sq > 0.f) { dist = sqrtf(sq); n = n / dist; }
		else { n = v3(0.f, 1.f, 0.f); }
		m.count = 1;
		m.n = n;
		V3 pt = 0.5f * (p + s.c + n * s.r);
		m.p[0] = make_float4(pt.x, pt.y, pt.z, s.r - dist);
		return true;
	}
	return false;
}
MI_DEV bool sphereObb(Sphere s, Obb o, Man& m) // :480-494
{
	Box aabb; aabb.lo = o.c - o.r; aabb.hi = o.c + o.r;
	Sphere s_; s_.c = conjugate(o.q) * (s.c - o.c) + o.c; s_.r = s.r;
	if (sphereBox(s_, aabb, m))
	{
		m.n = o.q * m.n;
		V3 pt = o.q * (v3f4(m.p[0]) - o.c) + o.c;
		m.p[0] = make_float4(pt.x, pt.y, pt.z, m.p[0].w);
		return true;
	}
	return false;
}
MI_DEV bool sphereCylinder(Sphere s, Capsule c, Man& m) // :408-449 (a cylinder is stored as {A, B, r} like a capsule)
{
	V3 ab = c.b - c.a;
	float t = dot(s.c - c.a, ab) / sqlen(ab);
	if (t >= 0.f && t <= 1.f)
	{
		Sphere s2; s2.c = lerp(c.a, c.b, t); s2.r = c.r;
		return sphereSphere(s, s2, m);
	}
	V3 p = (t <= 0.f) ? c.a : c.b;
	V3 up = (t <= 0.f) ? -ab : ab;
	V3 projectedDirToCenter = normalize(cross(cross(up, s.c - p), up));
	V3 endA = p + projectedDirToCenter * c.r;
	V3 endB = p - projectedDirToCenter * c.r;
	V3 closestToSphere = closestPointSegment(s.c, endA, endB);
	V3 normal = closestToSphere - s.c;
	float sq = sqlen(normal);
	if (sq <= s.r * s.r)
	{
		float distance;
		if (sq == 0.f) { distance = 0.f; m.n = -normalize(up); }
		else { distance = sqrtf(sq); m.n = normal / distance; }
		m.count = 1;
		float depth = s.r - distance;
		V3 pt = closestToSphere + 0.5f * depth * normal; // scales the un-normalised normal, as :445 does
		m.p[0] = make_float4(pt.x, pt.y, pt.z, depth);
		return true;
	}
	return false;
}
// capsule vs capsule (:523-612) and capsule vs cylinder (:614-703): identical except for what the end-cap / general cases test against
template <bool B_IS_CYLINDER>
MI_DEV bool capsuleTube(Capsule a, Capsule b, Man& m)
{
	V3 aDir = a.b - a.a;
	V3 bDir = normalize(b.b - b.a);
	float aDirLength = length(aDir);
	aDir *= 1.f / aDirLength;
	float parallel = dot(aDir, bDir);
	if (fabsf(parallel) > 0.99f)
	{
		V3 pAa = a.a, pAb = a.b, pBa = b.a, pBb = b.b;
		if (parallel < 0.f) { V3 t = pBa; pBa = pBb; pBb = t; }
		V3 ref = a.a;
		float a0 = 0.f, a1 = aDirLength;
		float b0 = dot(aDir, pBa - ref), b1 = dot(aDir, pBb - ref);
		float left = fmaxf(a0, b0), right = fminf(a1, b1);
		if (right < left)
		{
			Sphere sa, sb; sa.r = a.r; sb.r = b.r;
			if (a0 > b1) { sa.c = pAa; sb.c = pBb; } else { sa.c = pAb; sb.c = pBa; }
			if (B_IS_CYLINDER) return sphereCylinder(sa, b, m);
			return sphereSphere(sa, sb, m);
		}
		V3 contactA0 = ref + left * aDir, contactA1 = ref + right * aDir;
		V3 contactB0 = closestPointSegment(contactA0, pBa, pBb);
		V3 contactB1 = contactB0 + (right - left) * aDir;
		V3 normal = contactB0 - contactA0;
		float d = length(normal);
		if (d < MI_EPSILON) { d = 0.f; normal = v3(0.f, 1.f, 0.f); } else { normal = normal / d; }
		float penetration = (a.r + b.r) - d;
		if (penetration < 0.f) return false;
		m.n = normal; m.count = 2;
		V3 p0 = (contactA0 + contactB0) * 0.5f, p1 = (contactA1 + contactB1) * 0.5f;
		m.p[0] = make_float4(p0.x, p0.y, p0.z, penetration);
		m.p[1] = make_float4(p1.x, p1.y, p1.z, penetration);
		return true;
	}
	V3 c1, c2;
	closestSegmentSegment(a.a, a.b, b.a, b.b, c1, c2);
	Sphere sa, sb; sa.c = c1; sa.r = a.r; sb.c = c2; sb.r = b.r;
	if (B_IS_CYLINDER) return sphereCylinder(sa, b, m);
	return sphereSphere(sa, sb, m);
}
MI_DEV bool capsuleCapsule(Capsule a, Capsule b, Man& m) { return capsuleTube<false>(a, b, m); }
MI_DEV bool capsuleCylinder(Capsule a, Capsule b, Man& m) { return capsuleTube<true>(a, b, m); }
MI_DEV bool boxBoxAxisAligned(Box a, Box b, Man& m) // :1074-1140
{
	V3 centerA = boxCenter(a), centerB = boxCenter(b), radiusA = boxRadius(a), radiusB = boxRadius(b);
	V3 d = centerB - centerA;
	V3 p = (radiusB + radiusA) - vabs(d);
	if (p.x < 0.f || p.y < 0.f || p.z < 0.f) return false;
	u32 minElement = (p.x < p.y) ? ((p.x < p.z) ? 0 : 2) : ((p.y < p.z) ? 1 : 2);
	float s = vget(d, minElement) < 0.f ? -1.f : 1.f;
	float penetration = vget(p, minElement) * s;
	V3 normal = v3s(0.f); vset(normal, minElement, s);
	m.n = normal; m.count = 4;
	u32 axis0 = (minElement + 1) % 3, axis1 = (minElement + 2) % 3;
	float min0 = fmaxf(vget(a.lo, axis0), vget(b.lo, axis0)), min1 = fmaxf(vget(a.lo, axis1), vget(b.lo, axis1));
	float max0 = fminf(vget(a.hi, axis0), vget(b.hi, axis0)), max1 = fminf(vget(a.hi, axis1), vget(b.hi, axis1));
	float depth = vget(centerA, minElement) + vget(radiusA, minElement) - penetration * 0.5f;
	for (u32 i = 0; i < 4; ++i)
	{
		V3 pt = v3s(0.f);
		vset(pt, axis0, (i < 2) ? min0 : max0);
		vset(pt, axis1, (i & 1) ? max1 : min1);
		vset(pt, minElement, depth);
		m.p[i] = make_float4(pt.x, pt.y, pt.z, penetration);
	}
	return true;
}

// OBB vs OBB — collision_narrow.cpp:1179-1527
MI_DEV bool obbObb(const Obb& a, const Obb& b, Man& m, const PolyStore& store)
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
	bool parallel = absR.m00 >= 0.99f || absR.m10 >= 0.99f || absR.m20 >= 0.99f || absR.m01 >= 0.99f || absR.m11 >= 0.99f || absR.m21 >= 0.99f
		|| absR.m02 >= 0.99f || absR.m12 >= 0.99f || absR.m22 >= 0.99f;

	float ra, rb;
	float minPenetration = MI_FLT_MAX;
	V3 normal = v3s(0.f);
	bool bFace = false;
	for (u32 i = 0; i < 3; ++i)
	{
		ra = vget(a.r, i);
		rb = dot(mrow(absR, i), b.r);
		float penetration = ra + rb - fabsf(vget(t, i));
		if (penetration < 0.f) return false;
		if (penetration < minPenetration) { minPenetration = penetration; normal = v3s(0.f); vset(normal, i, 1.f); }
	}
	for (u32 i = 0; i < 3; ++i)
	{
		ra = dot(mcol(absR, i), a.r);
		rb = vget(b.r, i);
		float d = dot(mcol(r, i), t);
		float penetration = ra + rb - fabsf(d);
		if (penetration < 0.f) return false;
		if (penetration < minPenetration) { minPenetration = penetration; normal = v3s(0.f); vset(normal, i, 1.f); bFace = true; }
	}
	bool edgeCollision = false;
	V3 edgeNormal = v3s(0.f);
	if (!parallel)
	{
		float penetration, l; V3 n;
#define MI_EDGE_TEST(RA, RB, DIST, NX, NY, NZ) \
		ra = RA; rb = RB; penetration = ra + rb - fabsf(DIST); \
		if (penetration < 0.f) return false; \
		n = v3(NX, NY, NZ); l = 1.f / length(n); penetration *= l; \
		if (penetration < minPenetration) { minPenetration = penetration; edgeNormal = n * l; edgeCollision = true; }
		MI_EDGE_TEST(a.r.y * absR.m20 + a.r.z * absR.m10, b.r.y * absR.m02 + b.r.z * absR.m01, t.z * r.m10 - t.y * r.m20, 0.f, -r.m20, r.m10)
		MI_EDGE_TEST(a.r.y * absR.m21 + a.r.z * absR.m11, b.r.x * absR.m02 + b.r.z * absR.m00, t.z * r.m11 - t.y * r.m21, 0.f, -r.m21, r.m11)
		MI_EDGE_TEST(a.r.y * absR.m22 + a.r.z * absR.m12, b.r.x * absR.m01 + b.r.y * absR.m00, t.z * r.m12 - t.y * r.m22, 0.f, -r.m22, r.m12)
		MI_EDGE_TEST(a.r.x * absR.m20 + a.r.z * absR.m00, b.r.y * absR.m12 + b.r.z * absR.m11, t.x * r.m20 - t.z * r.m00, r.m20, 0.f, -r.m00)
		MI_EDGE_TEST(a.r.x * absR.m21 + a.r.z * absR.m01, b.r.x * absR.m12 + b.r.z * absR.m10, t.x * r.m21 - t.z * r.m01, r.m21, 0.f, -r.m01)
		MI_EDGE_TEST(a.r.x * absR.m22 + a.r.z * absR.m02, b.r.x * absR.m11 + b.r.y * absR.m10, t.x * r.m22 - t.z * r.m02, r.m22, 0.f, -r.m02)
		MI_EDGE_TEST(a.r.x * absR.m10 + a.r.y * absR.m00, b.r.y * absR.m22 + b.r.z * absR.m21, t.y * r.m00 - t.x * r.m10, -r.m10, r.m00, 0.f)
		MI_EDGE_TEST(a.r.x * absR.m11 + a.r.y * absR.m01, b.r.x * absR.m22 + b.r.z * absR.m20, t.y * r.m01 - t.x * r.m11, -r.m11, r.m01, 0.f)
		MI_EDGE_TEST(a.r.x * absR.m12 + a.r.y * absR.m02, b.r.x * absR.m21 + b.r.y * absR.m20, t.y * r.m02 - t.x * r.m12, -r.m12, r.m02, 0.f)
#undef MI_EDGE_TEST
	}
	bool faceCollision = !edgeCollision;
	if (faceCollision) { if (bFace) normal = r * normal; }
	else normal = edgeNormal;
	normal = a.q * normal;
	if (dot(normal, tw) < 0.f) normal = -normal;
	m.n = normal;

	if (faceCollision)
	{
		V3 cpp[4], cpn[4], verts[4];
		Poly polygon; polygon.pts = store.a; polygon.stride = store.stride; polygon.n = 4;
		Poly clipped; clipped.pts = store.b; clipped.stride = store.stride;
		float4 plane;
		if (!bFace)
		{
			getAABBClippingPlanes(a.r, conjugate(a.q) * normal, cpp, cpn);
			getAABBIncidentVertices(b.r, conjugate(b.q) * normal, verts);
			for (u32 i = 0; i < 4; ++i) { cpp[i] = a.q * cpp[i] + a.c; cpn[i] = a.q * cpn[i]; verts[i] = b.q * verts[i] + b.c; }
			plane = createPlane(obbSupport(a, normal), normal);
		}
		else
		{
			getAABBClippingPlanes(b.r, conjugate(b.q) * -normal, cpp, cpn);
			getAABBIncidentVertices(a.r, conjugate(a.q) * -normal, verts);
			for (u32 i = 0; i < 4; ++i) { cpp[i] = b.q * cpp[i] + b.c; cpn[i] = b.q * cpn[i]; verts[i] = a.q * verts[i] + a.c; }
			plane = createPlane(obbSupport(b, -normal), -normal);
		}
		float4 clipPlanes[4];
		for (u32 i = 0; i < 4; ++i)
		{
			clipPlanes[i] = createPlane(cpp[i], cpn[i]);
			PP(polygon, i) = make_float4(verts[i].x, verts[i].y, verts[i].z, -signedDistanceToPlane(verts[i], plane));
		}
		if (!clipPointsAndBuildContact(polygon, clipped, clipPlanes, plane, m)) return false;
	}
	else
	{
		V3 a0, a1, b0, b1;
		getAABBIncidentEdge(a.r, conjugate(a.q) * normal, a0, a1);
		getAABBIncidentEdge(b.r, conjugate(b.q) * -normal, b0, b1);
		a0 = a.q * a0 + a.c; a1 = a.q * a1 + a.c; b0 = b.q * b0 + b.c; b1 = b.q * b1 + b.c;
		V3 pa, pb;
		float sq = closestSegmentSegment(a0, a1, b0, b1, pa, pb);
		V3 pt = (pa + pb) * 0.5f;
		m.count = 1;
		m.p[0] = make_float4(pt.x, pt.y, pt.z, sqrtf(sq));
	}
	return true;
}
