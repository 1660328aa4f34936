// The volume of an overlap query (k_overlap.hip) and of a contact query (k_contact_query.hip): one mi_overlap_query record becomes the
// world record and world box of a collider of that shape at that pose, by the rule in include/mi_physics.h (mount composition, the
// switched-off conditions, the world-shape output).  Both kernels ask their candidates with the same inclusive box test.
#pragma once
#include "world.h"
#include "collider_world.h"
#include "raycast_shared.h"

struct OvQuery { ColliderRec rec; V3 mn, mx; u32 type; RcExclude ex; };

// Shape words mi_add_collider takes for a type: the rest of the record is zero, as it is for a collider of the world.
MI_DEV u32 ovShapeWords(u32 type) { return type == MI_SPHERE ? 4u : ((type == MI_CAPSULE || type == MI_CYLINDER) ? 7u : (type == MI_AABB ? 6u : (type == MI_HULL ? 8u : 10u))); }

// The broadphase's comparison (k_broad.hip, aabbOverlap; reference aabbVsAABB): inclusive.
MI_DEV bool ovBoxesMeet(V3 amin, V3 amax, V3 bmin, V3 bmax)
{
	if (amax.x < bmin.x || amin.x > bmax.x) return false;
	if (amax.y < bmin.y || amin.y > bmax.y) return false;
	if (amax.z < bmin.z || amin.z > bmax.z) return false;
	return true;
}

// a or b, word by word.  (Not `c ? a : b` on the records themselves: a conditional between two lvalues selects an address, and a record whose
// address is taken stays in scratch.)
MI_DEV float4 ovPick(bool c, float4 a, float4 b) { return make_float4(c ? +a.x : +b.x, c ? +a.y : +b.y, c ? +a.z : +b.z, c ? +a.w : +b.w); }
MI_DEV ColliderRec ovPick(bool c, const ColliderRec& a, const ColliderRec& b) { ColliderRec r; r.a = ovPick(c, a.a, b.a); r.b = ovPick(c, a.b, b.b); r.c = ovPick(c, a.c, b.c); r.d = ovPick(c, a.d, b.d); return r; }

// Query i of `queries` (6 x float4 per query = mi_overlap_query {shape[0..3]}, {shape[4..7]}, {shape[8], shape[9], type, enabled},
// {pos.xyz, mount}, {rot}, {excludeFirst, excludeCount, 0, 0}, integers as bits) -> q; false: the query is switched off.  worldShapes:
// NULL or 5 x float4 per query, written here (zeros for a query that is switched off).
MI_DEV bool ovVolume(u32 i, const float4* __restrict__ queries, float4* __restrict__ worldShapes, const RcScene& sc, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask,
	const float4* __restrict__ hullInfo, u32 numHulls, OvQuery& q)
{
	const float4* Q = queries + 6 * (size_t)i;
	const float4 q0 = Q[0], q1 = Q[1], q2 = Q[2], q3 = Q[3], q4r = Q[4], q5 = Q[5];
	q.ex = RcExclude{ mi_f2u(q5.x), mi_f2u(q5.y) };
	const u32 type = mi_f2u(q2.z);
	bool on = mi_f2u(q2.w) != 0u && type < (u32)MI_TYPE_COUNT;
	if (on && type == MI_HULL) on = q1.w >= 0.f && q1.w < (float)numHulls && (u32)q1.w < numHulls; // (a NaN index fails the first comparison)
	V3 pos = v3(q3.x, q3.y, q3.z); Q4 rot = q4f4(q4r);
	if (on)
	{
		Q4 mrot; V3 mpos;
		const RcMount m = rcMount(mi_f2u(q3.w), sc.nb, sc.pose, alive, simMask, mrot, mpos);
		on = m != RC_MOUNT_OFF;
		if (m == RC_MOUNT_BODY) { pos = mrot * pos + mpos; rot = mrot * rot; }
	}
	q.mn = v3s(0.f); q.mx = v3s(0.f); q.type = 0u;
	if (on)
	{
		const float s[10] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y };
		const u32 n = ovShapeWords(type);
		float z[10];
		#pragma unroll
		for (u32 k = 0; k < 10u; ++k) z[k] = k < n ? s[k] : 0.f;
		ColliderRec local;
		local.a = make_float4(z[0], z[1], z[2], z[3]); local.b = make_float4(z[4], z[5], z[6], z[7]); local.c = make_float4(z[8], z[9], 0.f, 0.f);
		local.d = make_float4(mi_u2f(type), mi_u2f(MI_STATIC_BODY), 0.f, 0.f);
		worldCollider(local, rot, pos, hullInfo, q.rec, q.mn, q.mx);
		q.type = colType(q.rec);
		// (a NaN among the 8 corners of a box is dropped by fminf / fmaxf: what is left of such a box is finite but may be empty, min > max)
		on = isfinite(q.mn.x) && isfinite(q.mn.y) && isfinite(q.mn.z) && isfinite(q.mx.x) && isfinite(q.mx.y) && isfinite(q.mx.z) && q.mn.x <= q.mx.x && q.mn.y <= q.mx.y && q.mn.z <= q.mx.z;
	}
	if (worldShapes)
	{
		float4* W = worldShapes + 5 * (size_t)i;
		const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
		W[0] = ovPick(on, q.rec.a, zero); W[1] = ovPick(on, q.rec.b, zero);
		W[2] = ovPick(on, make_float4(q.rec.c.x, q.rec.c.y, mi_u2f(q.type), 0.f), zero);
		W[3] = ovPick(on, make_float4(q.mn.x, q.mn.y, q.mn.z, 0.f), zero); W[4] = ovPick(on, make_float4(q.mx.x, q.mx.y, q.mx.z, 0.f), zero);
	}
	return on;
}
