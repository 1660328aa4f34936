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
#include "proximity_shared.h" // PxtQuery, pxtBoxDistance, pxtLimit, pxtSearch: shared with the cloth's projection pass (k_cloth_collide.hip)

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
	V3 p = v3(q0.x, q0.y, q0.z); const float radius = q0.w;
	{
		Q4 rot; V3 pos;
		const RcMount m = rcMount(mi_f2u(q1.x), nb, pose, alive, simMask, rot, pos);
		if (m == RC_MOUNT_OFF) return;
		if (m == RC_MOUNT_BODY) p = rot * p + pos;
	}
	if (!(radius >= 0.f)) return; // (a negative or NaN radius finds nothing)
	const float pMax = pxtPointMax(p);
	if (!(pMax <= MI_FLT_MAX)) return; // a point that is not finite has no nearest triangle (the walk and brute force alike)
	const TpBest best = pxtSearch<BRUTE>(P, heights, valid, tiles, chunkRange, p, radius, pMax);
	if (best.id == TP_NO_TRIANGLE) return;
	const TpReading r = tpReading(p, best);
	if (!(r.d <= radius)) return;
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
