// Narrowphase: prune / classify / bucket (reference collision_narrow.cpp:2346-2453), then one branch-uniform kernel family per
// group of type pairs: closed forms (:374-612, :1074-1140), box-box SAT + Sutherland-Hodgman clipping (:1179-1527) and
// GJK + EPA for capsule / cylinder vs box and cylinder vs cylinder (:705-790, :821-1043, collision_gjk.{h,cpp}, collision_epa.{h,cpp}).
// One thread per candidate pair; every pair writes a 96-byte ManifoldRec (count 0 = no collision) so contact generation needs no
// atomics and keeps pair order.  Every pair with a convex hull is GJK + EPA with one contact (:496-520, 792-818, 1045-1071, 1150-1176,
// 1529-1584); the hull's support function walks its vertex list (collision_gjk.h:77-100).
//
// This header holds what every stage shares: the pair keys that name the buckets, the shape records and the manifold.  The stages,
// one translation unit each with its kernels and the host code that launches them: k_narrow_classify.hip (keys, sort, bucket
// offsets; launch_narrowphase), k_narrow_pairs.hip (closed forms and box-box), k_narrow_gjk.hip (GJK, then EPA on the hits) and
// k_narrow_zone.hip (boolean overlap tests for force fields and triggers).  narrow_clip.h and narrow_gjk.h hold what two of them use;
// narrow_pairs.h and narrow_epa.h hold the per-pair device functions of the pair and GJK / EPA stages, which the contact query
// (k_contact_query.hip) runs on its own pair list as well.
#pragma once
#include "world.h"

// ---------------------------------------------------------------------------------------------------------------
// Pair keys.  k_classify orders a pair so that typeA <= typeB and gives it the key typeA * 6 + typeB; the pairs are sorted by key
// and counters[CTR_BUCKET_START + key] is the first manifold slot of that key's bucket.  Every kernel below owns a set of keys.
// ---------------------------------------------------------------------------------------------------------------
#define KEY_INVALID 63u
#define KEY_ZONE 62u   // rigid body vs force-field / trigger collider: boolean overlap check only (collision_narrow.cpp:2378-2395)
MI_DEV constexpr u32 pairKey(u32 typeA, u32 typeB) { return typeA * 6 + typeB; }

constexpr u32 KEY_SPHERE_SPHERE = pairKey(MI_SPHERE, MI_SPHERE), KEY_SPHERE_CAPSULE = pairKey(MI_SPHERE, MI_CAPSULE), KEY_SPHERE_CYLINDER = pairKey(MI_SPHERE, MI_CYLINDER),
	KEY_SPHERE_AABB = pairKey(MI_SPHERE, MI_AABB), KEY_SPHERE_OBB = pairKey(MI_SPHERE, MI_OBB), KEY_SPHERE_HULL = pairKey(MI_SPHERE, MI_HULL),
	KEY_CAPSULE_CAPSULE = pairKey(MI_CAPSULE, MI_CAPSULE), KEY_CAPSULE_CYLINDER = pairKey(MI_CAPSULE, MI_CYLINDER), KEY_CAPSULE_AABB = pairKey(MI_CAPSULE, MI_AABB),
	KEY_CAPSULE_OBB = pairKey(MI_CAPSULE, MI_OBB), KEY_CAPSULE_HULL = pairKey(MI_CAPSULE, MI_HULL),
	KEY_CYLINDER_CYLINDER = pairKey(MI_CYLINDER, MI_CYLINDER), KEY_CYLINDER_AABB = pairKey(MI_CYLINDER, MI_AABB), KEY_CYLINDER_OBB = pairKey(MI_CYLINDER, MI_OBB),
	KEY_CYLINDER_HULL = pairKey(MI_CYLINDER, MI_HULL),
	KEY_AABB_AABB = pairKey(MI_AABB, MI_AABB), KEY_AABB_OBB = pairKey(MI_AABB, MI_OBB), KEY_AABB_HULL = pairKey(MI_AABB, MI_HULL),
	KEY_OBB_OBB = pairKey(MI_OBB, MI_OBB), KEY_OBB_HULL = pairKey(MI_OBB, MI_HULL), KEY_HULL_HULL = pairKey(MI_HULL, MI_HULL);

// k_narrow<GROUP_CLOSED>: closed forms; its buckets are scattered over the key space.
MI_DEV constexpr bool closedFormKey(u32 key)
{
	return key == KEY_SPHERE_SPHERE || key == KEY_SPHERE_CAPSULE || key == KEY_SPHERE_CYLINDER || key == KEY_SPHERE_AABB || key == KEY_SPHERE_OBB
		|| key == KEY_CAPSULE_CAPSULE || key == KEY_CAPSULE_CYLINDER || key == KEY_AABB_AABB;
}
// k_narrow<GROUP_BOX>: aabb-obb and obb-obb, inside the contiguous slot range [KEY_BOX_BEGIN, KEY_BOX_END) (aabb-hull lies in it and is skipped: GJK + EPA).
constexpr u32 KEY_BOX_BEGIN = KEY_AABB_OBB, KEY_BOX_END = KEY_OBB_HULL;
MI_DEV constexpr bool boxKey(u32 key) { return key == KEY_AABB_OBB || key == KEY_OBB_OBB; }
// k_gjk<0> / k_epa<0>, the tube family: capsule / cylinder vs box and cylinder vs cylinder, inside [KEY_TUBE_BEGIN, KEY_TUBE_END)
// (capsule-hull lies in it and is skipped; typeA * 6 + 0 and + 1 cannot occur there with typeA <= typeB).
constexpr u32 KEY_TUBE_BEGIN = KEY_CAPSULE_AABB, KEY_TUBE_END = KEY_CYLINDER_HULL;
MI_DEV constexpr bool tubeKey(u32 key) { return key == KEY_CAPSULE_AABB || key == KEY_CAPSULE_OBB || key == KEY_CYLINDER_CYLINDER || key == KEY_CYLINDER_AABB || key == KEY_CYLINDER_OBB; }
// k_gjk<1> / k_epa<1>, the hull family: anything vs hull, the keys with typeB = hull inside [KEY_HULL_BEGIN, KEY_HULL_END).
constexpr u32 KEY_HULL_BEGIN = KEY_SPHERE_HULL, KEY_HULL_END = KEY_HULL_HULL + 1;
MI_DEV constexpr bool hullKey(u32 key) { return key % 6 == MI_HULL; }
// Keys (typeA * 6 + typeB) that go through GJK + EPA.
MI_DEV constexpr bool gjkKey(u32 key) { return tubeKey(key) || (hullKey(key) && key < KEY_HULL_END); }

// The names above are a protocol between kernels (and CTR_BUCKET_START words that inspection tools read): each is pinned to its number.
constexpr bool keySetIs(bool (*in)(u32), u64 bits) { for (u32 k = 0; k < 64; ++k) if (in(k) != (((bits >> k) & 1ull) != 0)) return false; return true; }
constexpr u64 keyBits() { return 0ull; }
template <typename... T> constexpr u64 keyBits(u32 k, T... rest) { return (1ull << k) | keyBits(rest...); }
static_assert(MI_TYPE_COUNT == 6 && pairKey(MI_HULL, MI_HULL) < KEY_ZONE && KEY_ZONE == 62 && KEY_INVALID == 63, "collision keys sort before KEY_ZONE, KEY_INVALID last; k_bucket_offsets has one lane per key 0..63");
static_assert(KEY_SPHERE_SPHERE == 0 && KEY_SPHERE_CAPSULE == 1 && KEY_SPHERE_CYLINDER == 2 && KEY_SPHERE_AABB == 3 && KEY_SPHERE_OBB == 4 && KEY_SPHERE_HULL == 5, "pair keys: sphere vs x");
static_assert(KEY_CAPSULE_CAPSULE == 7 && KEY_CAPSULE_CYLINDER == 8 && KEY_CAPSULE_AABB == 9 && KEY_CAPSULE_OBB == 10 && KEY_CAPSULE_HULL == 11, "pair keys: capsule vs x");
static_assert(KEY_CYLINDER_CYLINDER == 14 && KEY_CYLINDER_AABB == 15 && KEY_CYLINDER_OBB == 16 && KEY_CYLINDER_HULL == 17, "pair keys: cylinder vs x");
static_assert(KEY_AABB_AABB == 21 && KEY_AABB_OBB == 22 && KEY_AABB_HULL == 23 && KEY_OBB_OBB == 28 && KEY_OBB_HULL == 29 && KEY_HULL_HULL == 35, "pair keys: box and hull vs x");
static_assert(keySetIs(closedFormKey, keyBits(0, 1, 2, 3, 4, 7, 8, 21)), "k_narrow<GROUP_CLOSED> owns keys 0, 1, 2, 3, 4, 7, 8, 21");
static_assert(keySetIs(boxKey, keyBits(22, 28)) && KEY_BOX_BEGIN == 22 && KEY_BOX_END == 29, "k_narrow<GROUP_BOX> owns keys 22 and 28 in slots [22, 29)");
static_assert(keySetIs(tubeKey, keyBits(9, 10, 14, 15, 16)) && KEY_TUBE_BEGIN == 9 && KEY_TUBE_END == 17, "the tube family owns keys 9, 10, 14, 15, 16 in slots [9, 17)");
static_assert(KEY_HULL_BEGIN == 5 && KEY_HULL_END == 36 && hullKey(5) && hullKey(35) && !hullKey(34), "the hull family owns the keys with key % 6 == 5 in slots [5, 36)");
static_assert(keySetIs(gjkKey, keyBits(5, 9, 10, 11, 14, 15, 16, 17, 23, 29, 35)), "GJK + EPA keys");

// ---------------------------------------------------------------------------------------------------------------
// Shape accessors
// ---------------------------------------------------------------------------------------------------------------
struct Sphere { V3 c; float r; };
struct Capsule { V3 a, b; float r; };
struct Box { V3 lo, hi; };
struct Obb { Q4 q; V3 c, r; };
struct Hull { Q4 q; V3 pos; u32 first, count; };
MI_DEV Sphere asSphere(const ColliderRec& c) { Sphere s; s.c = v3(c.a.x, c.a.y, c.a.z); s.r = c.a.w; return s; }
MI_DEV Capsule asCapsule(const ColliderRec& c) { Capsule s; s.a = v3(c.a.x, c.a.y, c.a.z); s.b = v3(c.a.w, c.b.x, c.b.y); s.r = c.b.z; return s; }
MI_DEV Box asBox(const ColliderRec& c) { Box s; s.lo = v3(c.a.x, c.a.y, c.a.z); s.hi = v3(c.a.w, c.b.x, c.b.y); return s; }
MI_DEV Obb asObb(const ColliderRec& c) { Obb s; s.q = q4f4(c.a); s.c = v3(c.b.x, c.b.y, c.b.z); s.r = v3(c.b.w, c.c.x, c.c.y); return s; }
MI_DEV Hull asHull(const ColliderRec& c, const float4* __restrict__ hullInfo)
{
	Hull h; h.q = q4f4(c.a); h.pos = v3(c.b.x, c.b.y, c.b.z);
	u32 g = (u32)c.b.w;
	h.first = __float_as_uint(hullInfo[2 * g].w); h.count = __float_as_uint(hullInfo[2 * g + 1].w);
	return h;
}
MI_DEV V3 boxCenter(const Box& b) { return (b.lo + b.hi) * 0.5f; }
MI_DEV V3 boxRadius(const Box& b) { return (b.hi - b.lo) * 0.5f; }
MI_DEV V3 obbSupport(const Obb& b, V3 dir) // collision_gjk.h:63-75 (the box-box reference plane and the GJK support of an OBB)
{
	dir = conjugate(b.q) * dir;
	V3 r = v3(dir.x < 0.f ? -b.r.x : b.r.x, dir.y < 0.f ? -b.r.y : b.r.y, dir.z < 0.f ? -b.r.z : b.r.z);
	return b.c + b.q * r;
}

MI_DEV V3 closestPointSegment(V3 q, V3 a, V3 b) // bounding_volumes.h:365-371
{
	V3 ab = b - a;
	float t = dot(q - a, ab) / sqlen(ab);
	t = clampf(t, 0.f, 1.f);
	return a + t * ab;
}
MI_DEV float closestSegmentSegment(V3 l1a, V3 l1b, V3 l2a, V3 l2b, V3& c1, V3& c2) // bounding_volumes.cpp:1251-1315
{
	float s, t;
	V3 d1 = l1b - l1a, d2 = l2b - l2a, r = l1a - l2a;
	float a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r);
	if (a <= MI_EPSILON && e <= MI_EPSILON) { c1 = l1a; c2 = l2a; return dot(c1 - c2, c1 - c2); }
	if (a <= MI_EPSILON) { s = 0.f; t = f / e; t = clampf(t, 0.f, 1.f); }
	else
	{
		float c = dot(d1, r);
		if (e <= MI_EPSILON) { t = 0.f; s = clampf(-c / a, 0.f, 1.f); }
		else
		{
			float b = dot(d1, d2);
			float denom = a * e - b * b;
			if (denom != 0.f) s = clampf((b * f - c * e) / denom, 0.f, 1.f); else s = 0.f;
			t = (b * s + f) / e;
			if (t < 0.f) { t = 0.f; s = clampf(-c / a, 0.f, 1.f); }
			else if (t > 1.f) { t = 1.f; s = clampf((b - c) / a, 0.f, 1.f); }
		}
	}
	c1 = l1a + d1 * s;
	c2 = l2a + d2 * t;
	return sqlen(c1 - c2);
}

// ---------------------------------------------------------------------------------------------------------------
// The manifold of one pair and its record (writeScalarContact, collision_narrow.cpp:2221-2253)
// ---------------------------------------------------------------------------------------------------------------
struct Man { V3 n; float4 p[4]; u32 count; };
MI_DEV Man emptyManifold() { Man m; m.count = 0; m.n = v3(0.f, 1.f, 0.f); return m; }

MI_DEV void writeManifold(ManifoldRec* __restrict__ out, u32 slot, const Man& m, bool hit, const ColliderRec& A, const ColliderRec& B, u32 pairIndexLo)
{
	ManifoldRec r;
	u32 count = hit ? m.count : 0;
	float friction = clamp01(sqrtf(colFriction(A) * colFriction(B)));
	float restitution = clamp01(fmaxf(colRestitution(A), colRestitution(B)));
	u32 fr = ((u32)(friction * 0xFFFF) << 16) | (u32)(restitution * 0xFFFF);
	for (u32 k = 0; k < 4; ++k) r.p[k] = (k < count) ? m.p[k] : make_float4(0.f, 0.f, 0.f, 0.f);
	r.nf = make_float4(m.n.x, m.n.y, m.n.z, __uint_as_float(fr));
	r.ids = make_uint4(colBody(A), colBody(B), count, pairIndexLo);
	out[slot] = r;
}

// The stages launch_narrowphase runs after classify / sort / bucket offsets; numPairs sizes the grids (the launch may be larger than
// the device's pair count: every kernel cuts itself to the bucket ranges in the counters).  They form two chains that share no data:
// each reads its own buckets of the sorted pair list and writes those buckets' manifold slots, the counters k_bucket_offsets wrote
// are read-only to both, and CTR_EPA_COUNT* / CTR_NARROW_LIMITS belong to GJK + EPA alone.  So behind k_bucket_offsets the pair
// kernels run on the world's side stream (World::narrowStream) while GJK -> EPA run on w.stream, and w.stream waits for the side
// stream before anything else is launched: in launch_narrowphase, or, for the launch a step makes ahead of its host
// synchronisation, in launch_narrow_side behind it (k_narrow_classify.hip says why).  With MI_NARROW_SIDE_STREAM=0 all of them
// run on w.stream: GJK, pair kernels, EPA.
void launch_gjk(World& w, u32 numPairs);           // k_narrow_gjk.hip: GJK on the tube family, and on the hull family if the world has hulls; fills the EPA work lists
void launch_pair_kernels(World& w, u32 numPairs, hipStream_t stream); // k_narrow_pairs.hip: closed forms, then box-box, on `stream`
void launch_epa(World& w, u32 numPairs);           // k_narrow_gjk.hip: EPA + face clipping on the GJK hits of both families
