// Face clipping for the narrowphase: what box-box (obbObb, k_narrow_pairs.hip) and the capsule-vs-box finish behind EPA
// (capsuleBoxFinish, k_narrow_gjk.hip) share.
#pragma once
#include "narrow.h"

// ---------------------------------------------------------------------------------------------------------------
// Manifold helpers — collision_narrow.cpp:56-369.  Polygon vertices are float4 (xyz, penetrationDepth).
// ---------------------------------------------------------------------------------------------------------------
// A clipping polygon: up to 16 points (x, y, z, penetration) — collision_narrow.cpp:148-152 — kept OUTSIDE the registers (its points are
// indexed by loop counters): vertex i lives at pts[i * stride].  The box-box kernel gives every lane a column of an LDS array
// (stride 64: a lane's accesses are LDS round trips, not scratch-memory ones through the vector memory path — its waves spent
// 61 % of their cycles waiting for those); the lone lane that clips a capsule's segment behind EPA uses its finished polytope's LDS (stride 1).
struct Poly { float4* pts; u32 stride; u32 n; };
#define PP(P_, I_) (P_).pts[(I_) * (P_).stride]
struct PolyStore { float4* a; float4* b; u32 stride; };

MI_DEV float4 clipAgainstPlane(float4 a, float4 b, float aDist, float bDist) // :154-163
{
	aDist = fabsf(aDist); bDist = fabsf(bDist);
	float t = aDist / (aDist + bDist);
	return make_float4(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z), a.w + t * (b.w - a.w));
}
MI_DEV void sutherlandHodgman(Poly& input, const float4* clipPlanes, u32 numClipPlanes, Poly& output) // :166-222
{
	Poly* in = &input; Poly* out = &output;
	u32 clipIndex = 0;
	for (; clipIndex < numClipPlanes; ++clipIndex)
	{
		float4 plane = clipPlanes[clipIndex];
		out->n = 0;
		if (in->n == 0) break;
		float4 startPoint = PP(*in, in->n - 1);
		for (u32 i = 0; i < in->n; ++i)
		{
			float4 endPoint = PP(*in, i);
			float startDist = signedDistanceToPlane(v3f4(startPoint), plane);
			float endDist = signedDistanceToPlane(v3f4(endPoint), plane);
			bool startInside = startDist > 0.f, endInside = endDist > 0.f;
			if (startInside && endInside) { PP(*out, out->n++) = endPoint; }
			else if (startInside) { PP(*out, out->n++) = clipAgainstPlane(startPoint, endPoint, startDist, endDist); }
			else if (!startInside && endInside)
			{
				PP(*out, out->n++) = clipAgainstPlane(startPoint, endPoint, startDist, endDist);
				PP(*out, out->n++) = endPoint;
			}
			startPoint = endPoint;
		}
		Poly* tmp = in; in = out; out = tmp;
	}
	if (clipIndex % 2 == 0)
	{
		for (u32 i = 0; i < input.n; ++i) PP(output, i) = PP(input, i);
		output.n = input.n;
	}
}
MI_DEV void findStableContactManifold(const Poly& poly, V3 normal, Man& m) // :56-146
{
	const u32 nv = poly.n;
#define v(I_) PP(poly, I_)
	if (nv > 4)
	{
		V3 searchDir = getTangent(normal);
		float best = dot(searchDir, v3f4(v(0)));
		u32 ri = 0;
		for (u32 i = 1; i < nv; ++i) { float d = dot(searchDir, v3f4(v(i))); if (d > best) { ri = i; best = d; } }
		m.p[0] = v(ri);
		best = 0.f; ri = 0;
		for (u32 i = 0; i < nv; ++i) { float d = sqlen(v3f4(v(i)) - v3f4(m.p[0])); if (d > best) { ri = i; best = d; } }
		m.p[1] = v(ri);
		best = 0.f; ri = 0;
		for (u32 i = 0; i < nv; ++i)
		{
			V3 qa = v3f4(m.p[0]) - v3f4(v(i)), qb = v3f4(m.p[1]) - v3f4(v(i));
			float area = 0.5f * dot(cross(qa, qb), normal);
			if (area > best) { ri = i; best = area; }
		}
		m.p[2] = v(ri);
		best = 0.f; ri = 0;
		for (u32 i = 0; i < nv; ++i)
		{
			V3 qa = v3f4(m.p[0]) - v3f4(v(i)), qb = v3f4(m.p[1]) - v3f4(v(i)), qc = v3f4(m.p[2]) - v3f4(v(i));
			float area1 = 0.5f * dot(cross(qa, qb), normal);
			float area2 = 0.5f * dot(cross(qb, qc), normal);
			float area3 = 0.5f * dot(cross(qc, qa), normal);
			float area = fmaxf(fmaxf(area1, area2), area3);
			if (area > best) { ri = i; best = area; }
		}
		m.p[3] = v(ri);
		m.count = 4;
	}
	else
	{
		m.count = nv;
#pragma unroll
		for (u32 i = 0; i < 4; ++i) if (i < nv) m.p[i] = v(i); // (static indices: a manifold's four points stay in registers)
	}
#undef v
}
MI_DEV bool clipPointsAndBuildContact(Poly& polygon, Poly& clipped, const float4* clipPlanes, float4 referencePlane, Man& m) // :339-369 (clipped: the second polygon's storage)
{
	clipped.n = 0;
	sutherlandHodgman(polygon, clipPlanes, 4, clipped);
	if (clipped.n > 0)
	{
		for (u32 i = 0; i < clipped.n; ++i)
		{
			float4 pt = PP(clipped, i);
			if (pt.w < 0.f)
			{
				PP(clipped, i) = PP(clipped, clipped.n - 1);
				--clipped.n;
				--i;
			}
			else
			{
				float d = pt.w;
				pt.x += referencePlane.x * d; pt.y += referencePlane.y * d; pt.z += referencePlane.z * d;
				PP(clipped, i) = pt;
			}
		}
		if (clipped.n > 0) { findStableContactManifold(clipped, m.n, m); return true; }
	}
	return false;
}
MI_DEV void getAABBClippingPlanes(V3 radius, V3 normal, V3* pts, V3* nrm) // :225-254
{
	V3 p = vabs(normal);
	u32 maxElement = (p.x > p.y) ? ((p.x > p.z) ? 0 : 2) : ((p.y > p.z) ? 1 : 2);
	u32 axis0 = (maxElement + 1) % 3, axis1 = (maxElement + 2) % 3;
	V3 n;
	n = v3s(0.f); vset(n, axis0, 1.f); nrm[0] = n; pts[0] = -radius;
	n = v3s(0.f); vset(n, axis1, 1.f); nrm[1] = n; pts[1] = -radius;
	n = v3s(0.f); vset(n, axis0, -1.f); nrm[2] = n; pts[2] = radius;
	n = v3s(0.f); vset(n, axis1, -1.f); nrm[3] = n; pts[3] = radius;
}
MI_DEV void getAABBIncidentVertices(V3 radius, V3 normal, V3* verts) // :257-289
{
	V3 p = vabs(normal);
	u32 maxElement = (p.x > p.y) ? ((p.x > p.z) ? 0 : 2) : ((p.y > p.z) ? 1 : 2);
	float s = vget(normal, maxElement) < 0.f ? 1.f : -1.f;
	u32 axis0 = (maxElement + 1) % 3, axis1 = (maxElement + 2) % 3;
	float d = vget(radius, maxElement) * s;
	float min0 = -vget(radius, axis0), min1 = -vget(radius, axis1), max0 = vget(radius, axis0), max1 = vget(radius, axis1);
	for (u32 i = 0; i < 4; ++i)
	{
		V3 v = v3s(0.f);
		vset(v, maxElement, d);
		vset(v, axis0, (i == 1 || i == 2) ? max0 : min0);
		vset(v, axis1, (i >= 2) ? max1 : min1);
		verts[i] = v;
	}
}
MI_DEV void getAABBIncidentEdge(V3 radius, V3 normal, V3& outA, V3& outB) // :301-336
{
	V3 p = vabs(normal);
	outA = radius;
	if (p.x > p.y) { if (p.y > p.z) outB = v3(radius.x, radius.y, -radius.z); else outB = v3(radius.x, -radius.y, radius.z); }
	else { if (p.x > p.z) outB = v3(radius.x, radius.y, -radius.z); else outB = v3(-radius.x, radius.y, radius.z); }
	V3 sgn = v3(normal.x < 0.f ? -1.f : 1.f, normal.y < 0.f ? -1.f : 1.f, normal.z < 0.f ? -1.f : 1.f);
	outA = outA * sgn; outB = outB * sgn;
}
