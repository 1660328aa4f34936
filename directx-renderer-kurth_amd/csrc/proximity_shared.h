// What decides a proximity reading, shared by mi_proximity (k_proximity.hip, k_proximity_terrain.hip) and the cloth's projection pass
// (k_cloth_collide.hip), so that both decide with the same code:
//   PxQuery, PxBest, PxVisitor   rcWalk's visitor of a point: the box distance that prunes, the leaf test that decides (pointBodyCollider)
//   pxtSearch                    the heightmap terrain against a point: the column, then chunks -> tiles -> cells, or every cell
// The rule is stated in include/mi_physics.h, its float32 operation order in point_tests.h and terrain_point.h.
#pragma once
#include "world.h"
#include "point_tests.h"
#include "terrain_point.h"
#include "terrain_walk.h"
#include "raycast_shared.h"

// Slack of the pruning test: a node is skipped only if the float32 distance from the point to its padded box exceeds
// bound + PX_SLACK_ULPS ulps of (|point| + largest |coordinate| of the scene + largest leaf diagonal) + PX_SLACK_REL * bound.  DESIGN.md derives them.
#define PX_SLACK_ULPS 32.f
#define PX_SLACK_REL (1.f / 65536.f)
#define PX_NONE 0xFFFFFFFFu

struct PxQuery { V3 p; float radius, slackAbs; u32 exFirst, exCount; };
struct PxBest { float d; u32 col, body, within; V3 c, n; };
MI_DEV PxBest pxBestNone() { PxBest best; best.d = __builtin_inff(); best.col = PX_NONE; best.body = 0u; best.within = 0u; best.c = v3s(0.f); best.n = v3s(0.f); return best; }

// Distance from p to the box b = {min xyz, max xyz}: 0 inside.  A NaN coordinate gives 0 on its axis (fmaxf drops it): such a node is visited.
MI_DEV float pxBoxDistance(V3 p, const float* b)
{
	const float gx = fmaxf(fmaxf(b[0] - p.x, p.x - b[3]), 0.f), gy = fmaxf(fmaxf(b[1] - p.y, p.y - b[4]), 0.f), gz = fmaxf(fmaxf(b[2] - p.z, p.z - b[5]), 0.f);
	return sqrtf(gx * gx + gy * gy + gz * gz);
}
// What a node's box distance is held against.  COUNT: every candidate within the radius has to be met.  Otherwise only one that beats or
// ties the best so far (a lower collider index may win the tie); never below 0, the distance of a box that contains the point.
template <bool COUNT>
MI_DEV float pxLimit(const PxQuery& q, const PxBest& best)
{
	const float bound = COUNT ? q.radius : fmaxf(fminf(q.radius, best.d), 0.f);
	return bound + (q.slackAbs + PX_SLACK_REL * bound);
}
// The absolute part of the slack for the point of q in this scene (RC_ABS, RC_DIAG of the tree's header).
MI_DEV float pxSlackAbs(V3 p, const RcScene& sc)
{
	const V3 ap = vabs(p);
	return PX_SLACK_ULPS * RC_EPS * (fmaxf(fmaxf(ap.x, ap.y), ap.z) + mi_u2f(sc.hdr[RC_ABS]) + mi_u2f(sc.hdr[RC_DIAG]));
}

// rcWalk's visitor of a point: a box is held against pxLimit, a leaf within the radius is counted and may become the nearest.
// withStatic == false: a collider without a rigid body is no candidate (a tree built with them serves a query that does not want them).
template <bool COUNT>
struct PxVisitor
{
	const PxQuery& q; const RcScene& sc; PxBest& best; bool withStatic;
	MI_DEV bool box(const float* b, float& d) const { d = pxBoxDistance(q.p, b); return !(d > pxLimit<COUNT>(q, best)); } // (a tie and a NaN visit)
	MI_DEV void leaf(u32 c)
	{
		RcCollider col;
		if (!rcFetch(sc, c, RcExclude{ q.exFirst, q.exCount }, col)) return;
		if (!withStatic && col.reported == MI_STATIC_BODY) return;
		const PtHit h = pointBodyCollider(conjugate(col.rot) * (q.p - col.pos), col.type, col.s, sc.hulls);
		if (!(h.d <= q.radius)) return;
		if (COUNT) best.within++;
		if (best.col == PX_NONE || h.d < best.d || (h.d == best.d && c < best.col))
		{
			best.d = h.d; best.col = c; best.body = col.reported;
			best.c = col.rot * h.c + col.pos; best.n = col.rot * h.n;
		}
	}
};

// ---- the heightmap terrain (k_proximity_terrain.hip describes the column, the bound and the slack) ----
#define PXT_SLACK_ULPS 64.f
#define PXT_SLACK_REL (1.f / 65536.f)

struct PxtQuery { V3 p; float radius, slackCol, slackBase, invCell; };

// Distance from p to the box [x0, x1] x [heights lo .. hi] x [z0, z1]; 0 inside.
MI_DEV float pxtBoxDistance(const TerrainParams& P, V3 p, float x0, float x1, float z0, float z1, u32 lo, u32 hi)
{
	const float y0 = (float)lo * P.heightScale + P.minY, y1 = (float)hi * P.heightScale + P.minY;
	const float gx = fmaxf(fmaxf(x0 - p.x, p.x - x1), 0.f), gy = fmaxf(fmaxf(y0 - p.y, p.y - y1), 0.f), gz = fmaxf(fmaxf(z0 - p.z, p.z - z1), 0.f);
	return sqrtf(gx * gx + gy * gy + gz * gz);
}
// What a box distance is held against (a tie and a NaN visit).
MI_DEV float pxtLimit(const TerrainParams& P, const PxtQuery& q, const TpBest& best, u32 lo, u32 hi)
{
	const float bound = best.below ? best.d : fminf(q.radius, best.d);
	const float S = (float)(hi - lo) * P.heightScale * q.invCell;
	return bound + (q.slackBase * (1.f + S * S) + PXT_SLACK_REL * bound);
}
MI_DEV void pxtCell(const TerrainParams& P, const uint16_t* __restrict__ H, V3 chunkMin, u32 chunk, u32 cx, u32 cz, V3 p, TpBest& best)
{
	tpPointCell(P, chunkMin, chunk, cx, cz, H[TERRAIN_VERTS * cz + cx], H[TERRAIN_VERTS * (cz + 1u) + cx], H[TERRAIN_VERTS * cz + cx + 1u], H[TERRAIN_VERTS * (cz + 1u) + cx + 1u], p, best);
}

// The nearest triangle and the sign of the finite world point p with radius >= 0 (best.id == TP_NO_TRIANGLE: no triangle met).  BRUTE: the
// cell body over every cell of every valid chunk, no table (tiles, chunkRange are not read).
template <bool BRUTE>
MI_DEV TpBest pxtSearch(const TerrainParams& P, const uint16_t* __restrict__ heights, const u32* __restrict__ valid, const u32* __restrict__ tiles,
	const u32* __restrict__ chunkRange, V3 p, float radius, float pMax)
{
	PxtQuery q; q.p = p; q.radius = radius;
	const V3 corner = v3(P.minX, P.minY, P.minZ);
	const u32 cpd = P.chunksPerDim;
	TpBest best = tpBestNone();
	if (BRUTE)
	{
		for (u32 chunk = 0; chunk < cpd * cpd; ++chunk)
		{
			if (!valid[chunk]) continue;
			const V3 chunkMin = terrainChunkMin(P, corner, chunk % cpd, chunk / cpd);
			const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
			for (u32 cz = 0; cz < RT_CELLS; ++cz)
				for (u32 cx = 0; cx < RT_CELLS; ++cx) pxtCell(P, H, chunkMin, chunk, cx, cz, p, best);
		}
		return best;
	}
	const float span = P.chunkSize * (float)cpd, top = 65535.f * P.heightScale;
	const V3 am = vmax(vabs(corner), vabs(corner + v3(span, top, span)));
	const float M = pMax + fmaxf(fmaxf(am.x, am.y), am.z);
	q.slackCol = RT_SLACK_ULPS * RT_EPS * M; q.slackBase = PXT_SLACK_ULPS * RT_EPS * M; q.invCell = 1.f / P.chunkScale;
	const int last = (int)cpd - 1, lastCell = (int)RT_CELLS - 1;
	// the column: every cell whose widened extent holds (p.x, p.z); clamped indices only add real triangles
	{
		const int Xa = rtIndex((p.x - q.slackCol - P.minX) * P.invChunkSize, 0, last), Xb = rtIndex((p.x + q.slackCol - P.minX) * P.invChunkSize, 0, last);
		const int Za = rtIndex((p.z - q.slackCol - P.minZ) * P.invChunkSize, 0, last), Zb = rtIndex((p.z + q.slackCol - P.minZ) * P.invChunkSize, 0, last);
		for (int Z = Za; Z <= Zb; ++Z)
			for (int X = Xa; X <= Xb; ++X)
			{
				const u32 chunk = (u32)Z * cpd + (u32)X;
				if (!valid[chunk]) continue;
				const V3 chunkMin = terrainChunkMin(P, corner, (u32)X, (u32)Z);
				const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
				const int xa = rtIndex((p.x - q.slackCol - chunkMin.x) * q.invCell, 0, lastCell), xb = rtIndex((p.x + q.slackCol - chunkMin.x) * q.invCell, 0, lastCell);
				const int za = rtIndex((p.z - q.slackCol - chunkMin.z) * q.invCell, 0, lastCell), zb = rtIndex((p.z + q.slackCol - chunkMin.z) * q.invCell, 0, lastCell);
				for (int cz = za; cz <= zb; ++cz)
					for (int cx = xa; cx <= xb; ++cx) pxtCell(P, H, chunkMin, chunk, (u32)cx, (u32)cz, p, best);
			}
	}
	// the range search: chunks -> tiles -> cells.  The index ranges only spare box tests (they are cut by the same limit plus the
	// column's slack); the box test decides.
	const float tileSize = P.chunkScale * (float)RT_TILE, invTile = 1.f / tileSize;
	for (u32 chunk = 0; chunk < cpd * cpd; ++chunk)
	{
		if (!valid[chunk]) continue;
		const u32 cr = chunkRange[chunk];
		const V3 chunkMin = terrainChunkMin(P, corner, chunk % cpd, chunk / cpd);
		const float limC = pxtLimit(P, q, best, cr & 0xFFFFu, cr >> 16);
		if (pxtBoxDistance(P, p, chunkMin.x, chunkMin.x + P.chunkSize, chunkMin.z, chunkMin.z + P.chunkSize, cr & 0xFFFFu, cr >> 16) > limC) continue;
		const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
		const float wC = limC + q.slackCol;
		const int txa = rtIndex((p.x - wC - chunkMin.x) * invTile, 0, (int)RT_TILES - 1), txb = rtIndex((p.x + wC - chunkMin.x) * invTile, 0, (int)RT_TILES - 1);
		const int tza = rtIndex((p.z - wC - chunkMin.z) * invTile, 0, (int)RT_TILES - 1), tzb = rtIndex((p.z + wC - chunkMin.z) * invTile, 0, (int)RT_TILES - 1);
		for (int tz = tza; tz <= tzb; ++tz)
			for (int tx = txa; tx <= txb; ++tx)
			{
				const u32 tr = tiles[chunk * (RT_TILES * RT_TILES) + (u32)tz * RT_TILES + (u32)tx];
				const float tx0 = chunkMin.x + (float)tx * tileSize, tz0 = chunkMin.z + (float)tz * tileSize;
				const float limT = pxtLimit(P, q, best, tr & 0xFFFFu, tr >> 16);
				if (pxtBoxDistance(P, p, tx0, tx0 + tileSize, tz0, tz0 + tileSize, tr & 0xFFFFu, tr >> 16) > limT) continue;
				for (u32 cz = (u32)tz * RT_TILE; cz < (u32)tz * RT_TILE + RT_TILE; ++cz)
					for (u32 cx = (u32)tx * RT_TILE; cx < (u32)tx * RT_TILE + RT_TILE; ++cx)
					{
						const u32 ha = H[TERRAIN_VERTS * cz + cx], hb = H[TERRAIN_VERTS * (cz + 1u) + cx], hc = H[TERRAIN_VERTS * cz + cx + 1u], hd = H[TERRAIN_VERTS * (cz + 1u) + cx + 1u];
						const u32 lo = min(min(ha, hb), min(hc, hd)), hi = max(max(ha, hb), max(hc, hd));
						const float cx0 = chunkMin.x + (float)cx * P.chunkScale, cz0 = chunkMin.z + (float)cz * P.chunkScale;
						if (pxtBoxDistance(P, p, cx0, cx0 + P.chunkScale, cz0, cz0 + P.chunkScale, lo, hi) > pxtLimit(P, q, best, lo, hi)) continue;
						tpPointCell(P, chunkMin, chunk, cx, cz, ha, hb, hc, hd, p, best);
					}
			}
	}
	return best;
}
// Largest |coordinate| of p: a point that is not finite (the result exceeds MI_FLT_MAX or is NaN) has no nearest triangle.
MI_DEV float pxtPointMax(V3 p) { const V3 ap = vabs(p); return fmaxf(fmaxf(ap.x, ap.y), ap.z); }
