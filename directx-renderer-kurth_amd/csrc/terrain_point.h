// The heightmap terrain as a candidate of mi_proximity (MI_PROX_TERRAIN) and of mi_sphere_cast_batch (MI_SPHERE_TERRAIN):
// include/mi_physics.h states the rule; this header is the one statement of its float32 operation order on top of point_tests.h and
// sphere_cast.h.  Every expression below is evaluated as written, left to right, compiled with -ffp-contract=off;
// tests/terrain_prox64.py and tests/terrain_spherecast64.py restate it in numpy.  Everything is in WORLD space: the terrain has no pose.
// The triangles are k_heightmap's and the ray cast's: (A, B, C) and (C, B, D) of terrainCellVertices, ids as in mi_ray_hit.
#pragma once
#include "point_tests.h"
#include "sphere_cast.h"
#include "terrain_shared.h"

#define TP_NO_TRIANGLE 0xFFFFFFFFu
#define TP_CELLS (TERRAIN_VERTS - 1u)

// One triangle against a point: the unit face normal, the closest point and the unsigned distance.
struct TpTri { V3 n, c; float d; };
MI_DEV TpTri tpTriangle(V3 p, V3 a, V3 b, V3 c)
{
	TpTri r;
	r.n = ptUnit(cross(b - a, c - a));
	r.c = closestOnTriangle(p, a, b, c, r.n);
	r.d = length(p - r.c);
	return r;
}
// Does triangle `which` of the cell [x0, x1] x [z0, z1] contain p's (x, z)?  The ray rule's closed containment with q = p.
MI_DEV bool tpOwns(V3 p, float x0, float x1, float z0, float z1, u32 which)
{
	const float u = (p.x - x0) / (x1 - x0), v = (p.z - z0) / (z1 - z0);
	if (!(u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f)) return false;
	return which == 0u ? u + v <= 1.f : u + v >= 1.f;
}

// ---- proximity ---------------------------------------------------------------------------------------------------------------------
// The nearest triangle so far (smallest d, of equal d the lowest id) and the triangle that decides the sign (the lowest id among
// those that own p's column).  Both updates are idempotent: a triangle may be met twice.
struct TpBest { float d; u32 id; V3 c, n; u32 signId; bool below; };
MI_DEV TpBest tpBestNone() { TpBest b; b.d = __builtin_inff(); b.id = TP_NO_TRIANGLE; b.c = v3s(0.f); b.n = v3s(0.f); b.signId = TP_NO_TRIANGLE; b.below = false; return b; }

MI_DEV void tpPointTriangle(V3 p, V3 a, V3 b, V3 c, float x0, float x1, float z0, float z1, u32 which, u32 id, TpBest& best)
{
	const TpTri r = tpTriangle(p, a, b, c);
	if (r.d < best.d || (r.d == best.d && id < best.id)) { best.d = r.d; best.id = id; best.c = r.c; best.n = r.n; }
	if (id < best.signId && tpOwns(p, x0, x1, z0, z1, which)) { best.signId = id; best.below = dot(p - a, r.n) < 0.f; }
}
// Both triangles of cell (cx, cz) of chunk `chunk`.  The walk and brute force share this body.
MI_DEV void tpPointCell(const TerrainParams& P, V3 chunkMin, u32 chunk, u32 cx, u32 cz, u32 ha, u32 hb, u32 hc, u32 hd, V3 p, TpBest& best)
{
	V3 A, B, C, D;
	terrainCellVertices(P, chunkMin, cx, cz, ha, hb, hc, hd, A, B, C, D);
	const u32 id = ((chunk * (TP_CELLS * TP_CELLS)) + cz * TP_CELLS + cx) * 2u;
	tpPointTriangle(p, A, B, C, A.x, D.x, A.z, D.z, 0u, id, best);
	tpPointTriangle(p, C, B, D, A.x, D.x, A.z, D.z, 1u, id + 1u, best);
}
// The reading of the terrain from the nearest triangle and the sign: d, point, normal.
struct TpReading { float d; V3 c, n; };
MI_DEV TpReading tpReading(V3 p, const TpBest& best)
{
	TpReading r;
	r.d = best.below ? -best.d : best.d;
	r.c = best.c;
	const V3 v = best.below ? best.c - p : p - best.c;
	r.n = length(v) > 0.f ? ptUnit(v) : best.n;
	return r;
}

// ---- sphere cast -------------------------------------------------------------------------------------------------------------------
// The unsigned distance to one triangle as the march's distance function: c = the closest point, n = unit(centre - c), the face
// normal where they coincide.
struct TpTriangleDistance
{
	V3 a, b, c;
	MI_DEV PtHit operator()(V3 p) const
	{
		const TpTri r = tpTriangle(p, a, b, c);
		PtHit h; h.d = r.d; h.c = r.c;
		const V3 v = p - r.c;
		h.n = length(v) > 0.f ? ptUnit(v) : r.n;
		return h;
	}
};
// The closest terrain hit so far: smallest t, of equal t the lowest id.  `beyond` of a march is best.t (the collider's t at first).
struct TpCast { float t, gap; u32 id, hit, iterations; V3 c, n; };
MI_DEV void tpCastTriangle(V3 o, V3 v, float L, float radius, float maxT, V3 a, V3 b, V3 c, u32 id, TpCast& best)
{
	const ScHit h = sphereCastMarch(o, v, L, radius, maxT, best.t, TpTriangleDistance{ a, b, c });
	if (h.hit != SC_HIT && h.hit != SC_UNRESOLVED) return;
	if (h.t < best.t || (best.id != TP_NO_TRIANGLE && h.t == best.t && id < best.id))
	{
		best.t = h.t; best.gap = h.gap; best.id = id; best.hit = h.hit; best.iterations = h.iterations; best.c = h.c; best.n = h.n;
	}
}
MI_DEV void tpCastCell(const TerrainParams& P, V3 chunkMin, u32 chunk, u32 cx, u32 cz, u32 ha, u32 hb, u32 hc, u32 hd, V3 o, V3 v, float L, float radius, float maxT, TpCast& best)
{
	V3 A, B, C, D;
	terrainCellVertices(P, chunkMin, cx, cz, ha, hb, hc, hd, A, B, C, D);
	const u32 id = ((chunk * (TP_CELLS * TP_CELLS)) + cz * TP_CELLS + cx) * 2u;
	tpCastTriangle(o, v, L, radius, maxT, A, B, C, id, best);
	tpCastTriangle(o, v, L, radius, maxT, C, B, D, id + 1u, best);
}
