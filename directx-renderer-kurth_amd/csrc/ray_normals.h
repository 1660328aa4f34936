// The hit normal of mi_raycast_sensors (include/mi_physics.h states the rule; the reference reports none): the surface's outward
// normal in the collider's LOCAL frame, from the local ray and t that rayBodyCollider returned, p = lr.origin + t * lr.direction: the
// same local hit the point is made from.  The caller rotates the result by the pose's rotation.  Compiled with -ffp-contract=off on
// either side, like ray_tests.h.
#pragma once
#include "ray_tests.h"

// AABB (lo, hi): the axis k with the largest |q_k| - e_k (q = p - centre, e = half extents), the lowest k on a tie; sign(q_k) on it.
MI_DEV V3 boxNormal(V3 p, V3 lo, V3 hi)
{
	const V3 q = p - (lo + hi) * 0.5f, e = (hi - lo) * 0.5f;
	const float dx = fabsf(q.x) - e.x, dy = fabsf(q.y) - e.y, dz = fabsf(q.z) - e.z;
	u32 k = 0; float best = dx;
	if (dy > best) { best = dy; k = 1; }
	if (dz > best) { best = dz; k = 2; }
	const float qk = vget(q, k), s = qk < 0.f ? -1.f : 1.f;
	return v3(k == 0 ? s : 0.f, k == 1 ? s : 0.f, k == 2 ? s : 0.f);
}
// Capsule (a, b, r): away from the closest point of the segment.  (a == b, where the quotient would be 0 / 0: the sphere about a)
MI_DEV V3 capsuleNormal(V3 p, V3 a, V3 b)
{
	const V3 ab = b - a;
	const float den = dot(ab, ab);
	const float s = den > 0.f ? clamp01(dot(p - a, ab) / den) : 0.f;
	return noz(p - (a + s * ab));
}
// Cylinder (a, b, r): the cap's normal where the point is less deep under a cap than under the side, else the side's; a tie goes to the side.
MI_DEV V3 cylinderNormal(V3 p, V3 a, V3 b, float r)
{
	const V3 u = noz(b - a);
	const float h = length(b - a), y = dot(p - a, u);
	const V3 rho = (p - a) - y * u;
	const float dc = refMin(y, h - y), ds = r - length(rho);
	if (dc < ds) return (y > h * 0.5f) ? u : -u;
	return noz(rho);
}
// Hull g: noz(cross(b - a, c - a)) of the triangle that supplied t in rayBodyCollider's loop (strict <: the lowest index on a tie), in
// the hull's frame; hr = the ray in that frame.  Zero if no triangle is hit.
template <typename Hull>
MI_DEV V3 hullNormal(const HRay& hr, u32 g, const Hull& hull)
{
	float best = MI_FLT_MAX; V3 n = v3s(0.f);
	const u32 nt = hull.numTriangles(g);
	for (u32 f = 0; f < nt; ++f)
	{
		const V3 a = hull.vertex(g, f, 0), b = hull.vertex(g, f, 1), c = hull.vertex(g, f, 2);
		float tt;
		if (rayTriangle(hr, a, b, c, tt) && tt < best) { best = tt; n = noz(cross(b - a, c - a)); }
	}
	return n;
}

// The normal of collider (type, s) in the body's frame for the local ray lr and the distance t of the hit.
template <typename Hull>
MI_DEV V3 rayBodyColliderNormal(const HRay& lr, float t, u32 type, const float* s, const Hull& hull)
{
	const V3 p = lr.origin + t * lr.direction;
	switch (type)
	{
		case MI_SPHERE: return noz(p - v3(s[0], s[1], s[2]));
		case MI_CAPSULE: return capsuleNormal(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]));
		case MI_CYLINDER: return cylinderNormal(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6]);
		case MI_AABB: return boxNormal(p, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]));
		case MI_OBB:
		{
			const Q4 q = q4(s[0], s[1], s[2], s[3]); const V3 ce = v3(s[4], s[5], s[6]), ra = v3(s[7], s[8], s[9]);
			const HRay br{ conjugate(q) * (lr.origin - ce), conjugate(q) * lr.direction };
			return q * boxNormal(br.origin + t * br.direction, v3s(0.f) - ra, ra);
		}
		case MI_HULL:
		{
			const Q4 q = q4(s[0], s[1], s[2], s[3]); const V3 hp = v3(s[4], s[5], s[6]);
			const HRay hr{ conjugate(q) * (lr.origin - hp), conjugate(q) * lr.direction };
			return q * hullNormal(hr, (u32)s[7], hull);
		}
		default: return v3s(0.f);
	}
}
