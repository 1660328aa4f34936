// testPhysicsInteraction's ray tests (bounding_volumes.cpp:197-394, 677-705; pointInTriangle: math.cpp:1273-1290) and the push
// it applies (physics.cpp:556-628), written once for the host entry point mi_test_physics_interaction (api.hip) and the batched
// kernel of mi_test_physics_interaction_batch (k_interact.hip).  Both translation units are compiled with -ffp-contract=off, so the
// same ray against the same pose gives the same bits on either side.
#pragma once
#include "mi_common.h"

struct HRay { V3 origin, direction; };
MI_DEV bool rayPlane(const HRay& r, V3 normal, float d, float& outT)
{
	float ndotd = dot(r.direction, normal);
	if (fabsf(ndotd) < 1e-6f) return false;
	outT = -(dot(r.origin, normal) + d) / ndotd;
	return true;
}
// the reference's own min / max (pch.h:57-67), not fminf / fmaxf: they differ in which operand a NaN replaces, and 0 * inf is a NaN here
// whenever the origin lies on a slab plane of an axis the ray does not move along
MI_DEV float refMin(float a, float b) { return (a < b) ? a : b; }
MI_DEV float refMax(float a, float b) { return (a < b) ? b : a; }
MI_DEV bool rayAABB(const HRay& r, V3 lo, V3 hi, float& outT)
{
	V3 invDir = v3(1.f / r.direction.x, 1.f / r.direction.y, 1.f / r.direction.z);
	float tx1 = (lo.x - r.origin.x) * invDir.x, tx2 = (hi.x - r.origin.x) * invDir.x;
	outT = refMin(tx1, tx2);
	float tmax = refMax(tx1, tx2);
	float ty1 = (lo.y - r.origin.y) * invDir.y, ty2 = (hi.y - r.origin.y) * invDir.y;
	outT = refMax(outT, refMin(ty1, ty2)); tmax = refMin(tmax, refMax(ty1, ty2));
	float tz1 = (lo.z - r.origin.z) * invDir.z, tz2 = (hi.z - r.origin.z) * invDir.z;
	outT = refMax(outT, refMin(tz1, tz2)); tmax = refMin(tmax, refMax(tz1, tz2));
	return tmax >= outT && outT > 0.f;
}
MI_DEV bool raySphere(const HRay& r, V3 center, float radius, float& outT)
{
	V3 m = r.origin - center;
	float b = dot(m, r.direction), c = dot(m, m) - radius * radius;
	if (c > 0.f && b > 0.f) return false;
	float discr = b * b - c;
	if (discr < 0.f) return false;
	outT = -b - sqrtf(discr);
	if (outT < 0.f) outT = 0.f;
	return true;
}
MI_DEV bool rayDisk(const HRay& r, V3 pos, V3 normal, float radius, float& outT)
{
	if (rayPlane(r, normal, -dot(normal, pos), outT)) return length(r.origin + outT * r.direction - pos) <= radius;
	return false;
}
MI_DEV bool rayCylinder(const HRay& r, V3 pa, V3 pb, float radius, float& outT)
{
	V3 axis = pb - pa;
	float height = length(axis);
	Q4 q = rotateFromTo(axis, v3(0.f, 1.f, 0.f));
	V3 o = q * (r.origin - pa), d = q * r.direction;
	const float epsilon = 1e-6f;
	float y = -1.f;
	if (o.x * o.x + o.z * o.z > radius * radius)
	{
		float a = d.x * d.x + d.z * d.z, b = d.x * o.x + d.z * o.z, c = o.x * o.x + o.z * o.z - radius * radius;
		float delta = b * b - a * c;
		if (delta < epsilon) return false;
		outT = (-b - sqrtf(delta)) / a;
		if (outT <= epsilon) return false;
		y = o.y + outT * d.y;
	}
	if (y > height + epsilon || y < -epsilon)
	{
		HRay lr{ o, d };
		float dist;
		if (d.y < 0.f && rayDisk(lr, v3(0.f, height, 0.f), v3(0.f, 1.f, 0.f), radius, dist)) outT = dist;
		if (d.y > 0.f && rayDisk(lr, v3(0.f, 0.f, 0.f), v3(0.f, -1.f, 0.f), radius, dist)) outT = dist;
		y = o.y + outT * d.y;
	}
	return y > -epsilon && y < height + epsilon;
}
MI_DEV bool rayCapsule(const HRay& r, V3 pa, V3 pb, float radius, float& outT)
{
	outT = MI_FLT_MAX;
	// t starts at 0: the reference declares it unwritten (bounding_volumes.cpp:366), and intersectCylinder reads it at :357 when the origin
	// is radially inside and no cap disk is taken (:346-355); on the device that is a register nobody wrote.  0 is what rayBodyCollider
	// hands the cylinder collider (physics.cpp:577).
	float t = 0.f; bool result = false;
	if (rayCylinder(r, pa, pb, radius, t)) { outT = t; result = true; }
	if (raySphere(r, pa, radius, t)) { outT = refMin(outT, t); result = true; }
	if (raySphere(r, pb, radius, t)) { outT = refMin(outT, t); result = true; }
	return result;
}
MI_DEV bool pointInTriangleH(V3 point, V3 a, V3 b, V3 c)
{
	V3 e10 = b - a, e20 = c - a;
	float aa = dot(e10, e10), bb = dot(e10, e20), cc = dot(e20, e20);
	float ac_bb = (aa * cc) - (bb * bb);
	V3 vp = point - a;
	float d = dot(vp, e10), e = dot(vp, e20);
	float x = (d * cc) - (e * bb), y = (e * aa) - (d * bb), z = x + y - ac_bb;
	u32 ux = mi_f2u(x), uy = mi_f2u(y), uz = mi_f2u(z);
	return ((uz & ~(ux | uy)) & 0x80000000u) != 0;
}
MI_DEV bool rayTriangle(const HRay& r, V3 a, V3 b, V3 c, float& outT)
{
	V3 normal = noz(cross(b - a, c - a));
	float d = -dot(normal, a);
	float nDotR = dot(r.direction, normal);
	if (fabsf(nDotR) <= 1e-6f) return false;
	outT = -(dot(r.origin, normal) + d) / nDotR;
	V3 q = r.origin + outT * r.direction;
	return outT >= 0.f && pointInTriangleH(q, a, b, c);
}

// One collider of a rigid body at (rot, pos) against the world-space ray r: the ray in the body's frame (lr) and the hit distance.
// shape = the collider's 10 local shape floats (ColliderRec a, b, c.xy); Hull provides numTriangles(g) and vertex(g, t, k) of hull g.
template <typename Hull>
MI_DEV bool rayBodyCollider(const HRay& r, Q4 rot, V3 pos, u32 type, const float* s, const Hull& hull, HRay& lr, float& t)
{
	lr = HRay{ conjugate(rot) * (r.origin - pos), conjugate(rot) * r.direction };
	t = 0.f;
	bool hit = false;
	switch (type)
	{
		case MI_SPHERE: hit = raySphere(lr, v3(s[0], s[1], s[2]), s[3], t); break;
		case MI_CAPSULE: hit = rayCapsule(lr, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], t); break;
		case MI_CYLINDER: hit = rayCylinder(lr, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], t); break;
		case MI_AABB: hit = rayAABB(lr, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), t); break;
		case MI_OBB:
		{
			Q4 q = q4(s[0], s[1], s[2], s[3]); V3 ce = v3(s[4], s[5], s[6]), ra = v3(s[7], s[8], s[9]);
			HRay br{ conjugate(q) * (lr.origin - ce), conjugate(q) * lr.direction };
			hit = rayAABB(br, v3s(0.f) - ra, ra, t);
		} break;
		case MI_HULL:
		{
			Q4 q = q4(s[0], s[1], s[2], s[3]); V3 hp = v3(s[4], s[5], s[6]);
			const u32 g = (u32)s[7];
			HRay hr{ conjugate(q) * (lr.origin - hp), conjugate(q) * lr.direction };
			float best = MI_FLT_MAX;
			const u32 nt = hull.numTriangles(g);
			for (u32 f = 0; f < nt; ++f)
			{
				float tt;
				if (rayTriangle(hr, hull.vertex(g, f, 0), hull.vertex(g, f, 1), hull.vertex(g, f, 2), tt) && tt < best) { best = tt; hit = true; }
			}
			t = best;
		} break;
		default: break;
	}
	return hit;
}

// The push of the closest hit: force = direction * strength at the hit point, torque about the body's centre of gravity
// (getGlobalCOGPosition, rigid_body.cpp:83-87).
MI_DEV void interactionPush(const HRay& r, const HRay& lr, float t, Q4 rot, V3 pos, V3 localCOG, float strength, V3& force, V3& torque)
{
	V3 localHit = lr.origin + t * lr.direction;
	V3 globalHit = rot * localHit + pos;                  // transformPosition (scale 1)
	V3 cogPosition = pos + rot * localCOG;
	force = r.direction * strength;
	torque = cross(globalHit - cogPosition, force);
}
