// MI_PROX_TERRAIN: the heightmap terrain as one more candidate of mi_proximity, the solid under the surface ("Proximity and
// sphere casts over the terrain"; the rule is stated in include/mi_physics.h, its float32 operation order in terrain_point.h).  Runs
// after k_proximity on the records it wrote (zeroed ones when no collider is a candidate) and replaces a record where the terrain's
// signed distance is strictly smaller than the collider's; with MI_PROX_COUNT it adds 1 to numWithin where the terrain is within.
//   (launch_terrain_tables) the min / max table of the heights per 8 x 8-cell tile and per chunk (terrain_walk.h), the ray cast's
//   k_px_terrain<false, *>  one lane per query: the world point again by rcMount (the same bytes k_proximity formed), the cells of the
//                           point's own column first (they decide the sign and seed the bound), then chunks -> tiles -> cells pruned by
//                           the distance from the point to each box
//   k_px_terrain<true, *>   MI_PROX_BRUTE_FORCE: the same cell body (tpPointCell) over every cell of every valid chunk, no table
// Only tpPointTriangle decides a reading; the boxes only say which cells need not be asked, so the walk and brute force agree in every byte.
//
// The column.  Which triangles own p's (x, z) is decided by tpOwns on the vertex coordinates; the walk finds them as the ray walk finds
// the cells of a vertical ray: every chunk and cell whose extent, widened by RT_SLACK_ULPS ulps of M (terrain_walk.h derives it),
// holds (p.x, p.z).  M = largest |coordinate| of p + largest |coordinate| of the terrain's box.
//
// The bound.  Above the surface, or over no chunk, only a triangle with d_f <= min(radius, best d_f so far) can change the record.  Below
// the surface the terrain is within for every radius, so the bound is the best d_f so far alone, never the radius; it starts at the d_f of
// the column's own triangles, which are candidates like any other (an upper bound of the nearest distance because it is one of them).
//
// The slack.  A box (x / z extent of a chunk, tile or cell, heights lo .. hi of the table) is skipped only if the float32 distance
// from p to it exceeds bound + slack(lo, hi) + PXT_SLACK_REL * bound, with slack = PXT_SLACK_ULPS eps M (1 + S^2),
// S = (hi - lo) * heightScale / cell size, the largest slope a triangle in the box can have.  What it has to cover: tpTriangle's d_f is
// |p - c_f| of the COMPUTED c_f, so d_f >= dist(p, box) - (how far c_f lies outside the box) - rounding.  A vertex is in the box up
// to the 3 eps M between vertex formula and grid line; an edge point a + s ab has s in [0, 1] by the signs its branch tested (the
// quotient of a non-negative number by a sum that contains it), so it is in the box up to 2 more roundings at M.  The face point
// p - dot(ap, n) n lies on the plane but may lie outside the triangle by e where a region test (vc, vb, va: differences of
// products of two dot products) was decided by its rounding: with vc = |ab| |cross(ab, ac)| e, |cross| >= cell^2, an error of
// <= 8 eps M |ab| |ac| |ap| in vc and |ap| <= (2 + e / cell) sqrt(1 + S^2) cell where the deficit matters (the point is close to the
// plane; far above it the deficit is e^2 / 2h, second order), e <= 16 eps M (1 + S^2), and the plane leaves the box's heights by at most
// sqrt(2) S e within that rim, which the next level's S, taken over the larger box, covers.  The box distance itself: 3 subtractions at
// M, then 5 relative roundings.  PXT_SLACK_ULPS = 64 is twice the sum, PXT_SLACK_REL = 2^-16 covers the relative roundings of both
// distances (k_proximity.hip's PX_SLACK_REL).
#include "world.h"
#include "terrain_point.h"
#include "terrain_walk.h"
#include "raycast_shared.h"

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

// queries, out: k_proximity's.  nb, pose, alive, simMask: rcMount's.
template <bool BRUTE, bool COUNT>
__global__ void __launch_bounds__(64) k_px_terrain(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ out, u32 nb, const float4* __restrict__ pose,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, TerrainParams P, const uint16_t* __restrict__ heights, const u32* __restrict__ valid,
	const u32* __restrict__ tiles, const u32* __restrict__ chunkRange)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const float4 q0 = queries[2 * i], q1 = queries[2 * i + 1];
	if (mi_f2u(q1.w) == 0u) return;
	PxtQuery q; q.p = v3(q0.x, q0.y, q0.z); q.radius = q0.w;
	{
		Q4 rot; V3 pos;
		const RcMount m = rcMount(mi_f2u(q1.x), nb, pose, alive, simMask, rot, pos);
		if (m == RC_MOUNT_OFF) return;
		if (m == RC_MOUNT_BODY) q.p = rot * q.p + pos;
	}
	if (!(q.radius >= 0.f)) return; // (a negative or NaN radius finds nothing)
	const V3 p = q.p, corner = v3(P.minX, P.minY, P.minZ);
	const u32 cpd = P.chunksPerDim;
	const V3 ap = vabs(p);
	const float pMax = fmaxf(fmaxf(ap.x, ap.y), ap.z);
	if (!(pMax <= MI_FLT_MAX)) return; // a point that is not finite has no nearest triangle (the walk and brute force alike)
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
	}
	else
	{
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
	}
	if (best.id == TP_NO_TRIANGLE) return;
	const TpReading r = tpReading(p, best);
	if (!(r.d <= q.radius)) return;
	const float4 rec0 = out[3 * i], rec1 = out[3 * i + 1];
	const bool colFound = mi_f2u(rec0.w) != 0u;
	const u32 within = COUNT ? mi_f2u(rec1.w) + 1u : 0u;
	if (!colFound || r.d < rec0.x) // (MI_TERRAIN_COLLIDER is the largest index: a tie stays with the collider)
	{
		out[3 * i] = make_float4(r.d, mi_u2f(MI_TERRAIN_COLLIDER), mi_u2f(MI_STATIC_BODY), mi_u2f(1u));
		out[3 * i + 1] = make_float4(r.c.x, r.c.y, r.c.z, mi_u2f(within));
		out[3 * i + 2] = make_float4(r.n.x, r.n.y, r.n.z, mi_u2f(best.id));
	}
	else if (COUNT) out[3 * i + 1] = make_float4(rec1.x, rec1.y, rec1.z, mi_u2f(within));
}

void launch_proximity_terrain(World& w, u32 n, const mi_proximity_query* dQueries, u32 flags, mi_proximity_reading* dOut)
{
	const u32 chunks = w.terrain.chunksPerDim * w.terrain.chunksPerDim;
	if (!chunks || !n) return;
	const bool brute = (flags & MI_PROX_BRUTE_FORCE) != 0, count = (flags & MI_PROX_COUNT) != 0;
	if (!brute && !launch_terrain_tables(w)) return;
	const TerrainParams P = terrainParams(w);
	const auto kernel = brute ? (count ? k_px_terrain<true, true> : k_px_terrain<true, false>) : (count ? k_px_terrain<false, true> : k_px_terrain<false, false>);
	hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, (float4*)dOut, w.nb, w.pose.p, w.aliveMask.p, w.simMask.p, P,
		w.terrain.heights.p, w.terrain.valid.p, brute ? (const u32*)nullptr : w.queries.terrainTiles.p, brute ? (const u32*)nullptr : w.queries.terrainChunkRange.p);
}
