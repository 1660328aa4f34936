// A local collider record in world space with its world AABB (reference physics.cpp:631-756): what the step builds per collider
// (k_bodies.hip, buildCollider) and what an overlap query builds for its volume and for every candidate it asks (k_overlap.hip).
// One definition, so the two agree in every bit.
#pragma once
#include "mi_common.h"

MI_DEV void growBox(V3& mn, V3& mx, V3 o) { mn = vmin(mn, o); mx = vmax(mx, o); }

// bounding_box::transformToAABB (bounding_volumes.cpp:58-70): 8 corners in this order.
MI_DEV void boxToAABB(V3 lo, V3 hi, Q4 rot, V3 tr, V3& mn, V3& mx)
{
	mn = v3s(MI_FLT_MAX); mx = v3s(-MI_FLT_MAX);
	growBox(mn, mx, rot * lo + tr);
	growBox(mn, mx, rot * v3(hi.x, lo.y, lo.z) + tr);
	growBox(mn, mx, rot * v3(lo.x, hi.y, lo.z) + tr);
	growBox(mn, mx, rot * v3(hi.x, hi.y, lo.z) + tr);
	growBox(mn, mx, rot * v3(lo.x, lo.y, hi.z) + tr);
	growBox(mn, mx, rot * v3(hi.x, lo.y, hi.z) + tr);
	growBox(mn, mx, rot * v3(lo.x, hi.y, hi.z) + tr);
	growBox(mn, mx, rot * hi + tr);
}

// World record o and world box [mn, mx] of the local record c at the pose (trot, tpos) of its body (or of its own entity, if static).
// o starts as a copy of c: the words a shape does not use, the material and the ids carry over.
MI_DEV void worldCollider(const ColliderRec& c, Q4 trot, V3 tpos, const float4* __restrict__ hullInfo, ColliderRec& o, V3& mn, V3& mx)
{
	o = c;
	switch (colType(c))
	{
		case MI_SPHERE:
		{
			V3 center = tpos + trot * v3(c.a.x, c.a.y, c.a.z);
			float r = c.a.w;
			mn = center - v3s(r); mx = center + v3s(r);
			o.a = make_float4(center.x, center.y, center.z, r);
		} break;
		case MI_CYLINDER: // tight extents, physics.cpp:699-720
		{
			V3 posA = trot * v3(c.a.x, c.a.y, c.a.z) + tpos;
			V3 posB = trot * v3(c.a.w, c.b.x, c.b.y) + tpos;
			float r = c.b.z;
			V3 a = posB - posA;
			float aa = dot(a, a);
			float x = 1.f - a.x * a.x / aa, y = 1.f - a.y * a.y / aa, z = 1.f - a.z * a.z / aa;
			x = sqrtf(fmaxf(0.f, x)); y = sqrtf(fmaxf(0.f, y)); z = sqrtf(fmaxf(0.f, z));
			V3 e = r * v3(x, y, z);
			mn = vmin(posA - e, posB - e); mx = vmax(posA + e, posB + e);
			o.a = make_float4(posA.x, posA.y, posA.z, posB.x);
			o.b = make_float4(posB.y, posB.z, r, 0.f);
		} break;
		case MI_CAPSULE:
		{
			V3 posA = trot * v3(c.a.x, c.a.y, c.a.z) + tpos;
			V3 posB = trot * v3(c.a.w, c.b.x, c.b.y) + tpos;
			float r = c.b.z;
			V3 r3 = v3s(r);
			mn = v3s(MI_FLT_MAX); mx = v3s(-MI_FLT_MAX);
			growBox(mn, mx, posA + r3); growBox(mn, mx, posA - r3); growBox(mn, mx, posB + r3); growBox(mn, mx, posB - r3);
			o.a = make_float4(posA.x, posA.y, posA.z, posB.x);
			o.b = make_float4(posB.y, posB.z, r, 0.f);
		} break;
		case MI_AABB:
		{
			V3 lo = v3(c.a.x, c.a.y, c.a.z), hi = v3(c.a.w, c.b.x, c.b.y);
			boxToAABB(lo, hi, trot, tpos, mn, mx);
			if (trot.x == 0.f && trot.y == 0.f && trot.z == 0.f && trot.w == 1.f)
			{
				o.a = make_float4(mn.x, mn.y, mn.z, mx.x);
				o.b = make_float4(mx.y, mx.z, 0.f, 0.f);
			}
			else // a rotated AABB becomes an OBB (physics.cpp:725-733)
			{
				V3 center = trot * ((lo + hi) * 0.5f) + tpos;
				V3 radius = (hi - lo) * 0.5f;
				o.a = make_float4(trot.x, trot.y, trot.z, trot.w);
				o.b = make_float4(center.x, center.y, center.z, radius.x);
				o.c.x = radius.y; o.c.y = radius.z;
				o.d.x = __uint_as_float((u32)MI_OBB);
			}
		} break;
		case MI_OBB:
		{
			Q4 q = q4f4(c.a);
			V3 center = v3(c.b.x, c.b.y, c.b.z);
			V3 radius = v3(c.b.w, c.c.x, c.c.y);
			Q4 wq = trot * q;                         // bounding_oriented_box::transformToAABB/OBB (bounding_volumes.cpp:127-142)
			V3 wc = trot * center + tpos;
			boxToAABB(-radius, radius, wq, wc, mn, mx);
			o.a = make_float4(wq.x, wq.y, wq.z, wq.w);
			o.b = make_float4(wc.x, wc.y, wc.z, radius.x);
		} break;
		case MI_HULL: // physics.cpp:742-753: compose the transforms, AABB = the geometry's local box transformed
		{
			Q4 hq = q4f4(c.a);
			V3 hp = v3(c.b.x, c.b.y, c.b.z);
			u32 g = (u32)c.b.w;
			Q4 rotation = trot * hq;
			V3 position = trot * hp + tpos;
			float4 lo = hullInfo[2 * g], hi = hullInfo[2 * g + 1];
			boxToAABB(v3f4(lo), v3f4(hi), rotation, position, mn, mx);
			o.a = make_float4(rotation.x, rotation.y, rotation.z, rotation.w);
			o.b = make_float4(position.x, position.y, position.z, c.b.w);
		} break;
		default: mn = v3s(0.f); mx = v3s(0.f); break;
	}
}
