// MI_RAY_TERRAIN: the heightmap terrain as a candidate of mi_raycast_batch ("Whole-world ray casts": the terrain).  Runs
// after k_raycast on the records it wrote (or on zeroed records when no collider is a candidate) and replaces a record where a terrain
// triangle is hit strictly before the collider.
//   k_rc_terrain_tiles   uint16 min / max of the heights per 8 x 8-cell tile (16 x 16 tiles per chunk) and per chunk; built when the
//                        heights changed (World::queries.terrainTableValid), on the world's stream, before the next terrain cast
//   k_rc_terrain<false>  one lane per ray: clip to the terrain's box, walk chunks -> tiles -> cells under the ray front to back
//   k_rc_terrain<true>   MI_RAY_BRUTE_FORCE: the same cell body (rtCell) over every cell of every valid chunk, no table
// The triangles are k_heightmap's: (A, B, C) and (C, B, D) of terrainCellVertices.  The hit rule is stated in include/mi_physics.h.
#include "world.h"
#include "terrain_shared.h"

#define RT_EPS 1.1920929e-7f
#define RT_NO_TRIANGLE 0xFFFFFFFFu
#define RT_CELLS (TERRAIN_VERTS - 1u)      // 128 cells per chunk and axis
#define RT_TILE 8u                         // cells per tile and axis
#define RT_TILES (RT_CELLS / RT_TILE)      // 16 tiles per chunk and axis
// Slack of the walk, in space: RT_SLACK_ULPS ulps of (largest |coordinate| of the origin + largest |coordinate| of the terrain's box).
// What it has to cover (M = that sum, eps = 2^-23): the triangle test accepts a hit by the rounded point q = fl(o + t d), which is
// within eps (|t d| + |q|) <= 3 eps M of the exact line; the vertex coordinates fl(chunkMin + fl(c * chunkScale)) differ from the
// walk's grid lines g + i * s by <= 3 eps M; the walk's own arithmetic (the position at an interval end, 2 roundings at <= 2 M; the
// distance to a grid line, (line - o) * (1 / d), 3 relative roundings on a product <= 2 M) adds <= 10 eps M.  16 eps M in all; the
// slack is twice that and is applied to both sides of every column and of every minor range.
// In height the hit point lies on the triangle's plane within the residual of t's formula, <= 20 eps M measured along the normal
// (6 roundings at |n| (|o| + |a|) in the numerator, 4 relative ones on t), i.e. <= 20 eps M / n.y vertically, plus the plane's slope
// times the 3 eps M the point may lie outside the cell.  With S = amplitude / cell size (the largest height difference over a cell
// side): slope <= sqrt(2) S and 1 / n.y <= 1 + 1.5 S, so 20 (1 + 1.5 S) + 5 S <= 32 (4 + 8 S) / 4: slackY = slack * (4 + 8 S).
#define RT_SLACK_ULPS 32.f

struct RtBest { float t; u32 id; V3 point; };

// One triangle (a, b, c) of the cell [x0, x1] x [z0, z1] (world coordinates of its vertices): ray::intersectTriangle's plane step
// (bounding_volumes.cpp:249-265), then containment by the cell-relative coordinates of q = o + t d, closed on all sides;
// triangle 0 owns u + v <= 1, triangle 1 owns u + v >= 1.  colT: the collider's hit (MI_FLT_MAX and colHit = false without one).
MI_DEV void rtTriangle(V3 o, V3 d, float maxT, bool colHit, float colT, V3 a, V3 b, V3 c, float x0, float x1, float z0, float z1, u32 which, u32 id, RtBest& best)
{
	const V3 n = noz(cross(b - a, c - a));
	const float nd = dot(d, n);
	if (fabsf(nd) <= 1e-6f) return;
	const float t = -(dot(o, n) - dot(n, a)) / nd;
	if (!(t >= 0.f && t <= maxT) || (colHit && !(t < colT))) return;
	const V3 q = o + t * d;
	const float u = (q.x - x0) / (x1 - x0), v = (q.z - z0) / (z1 - z0);
	if (!(u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f)) return;
	if (which == 0u ? !(u + v <= 1.f) : !(u + v >= 1.f)) return;
	if (t < best.t || (best.id != RT_NO_TRIANGLE && t == best.t && id < best.id)) { best.t = t; best.id = id; best.point = q; }
}
// Both triangles of cell (cx, cz) of chunk `chunk`.  The walk and brute force share this body.
MI_DEV void rtCell(const TerrainParams& P, V3 chunkMin, u32 chunk, u32 cx, u32 cz, u32 ha, u32 hb, u32 hc, u32 hd, V3 o, V3 d, float maxT, bool colHit, float colT, RtBest& best)
{
	V3 A, B, C, D;
	terrainCellVertices(P, chunkMin, cx, cz, ha, hb, hc, hd, A, B, C, D);
	const u32 id = ((chunk * (RT_CELLS * RT_CELLS)) + cz * RT_CELLS + cx) * 2u;
	rtTriangle(o, d, maxT, colHit, colT, A, B, C, A.x, D.x, A.z, D.z, 0u, id, best);
	rtTriangle(o, d, maxT, colHit, colT, C, B, D, A.x, D.x, A.z, D.z, 1u, id + 1u, best);
}

// ---- the tile table ----------------------------------------------------------------------------------------------------------------
// One workgroup per chunk, one lane per tile: (max << 16) | min over the 9 x 9 vertices of the tile's 8 x 8 cells, then the chunk's.
__global__ void __launch_bounds__(256) k_rc_terrain_tiles(const uint16_t* __restrict__ heights, u32* __restrict__ tiles, u32* __restrict__ chunkRange)
{
	__shared__ u32 sLo[4], sHi[4];
	const u32 chunk = blockIdx.x, tile = threadIdx.x, tx = tile % RT_TILES, tz = tile / RT_TILES;
	const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
	u32 lo = 0xFFFFu, hi = 0u;
	for (u32 z = 0; z <= RT_TILE; ++z)
		for (u32 x = 0; x <= RT_TILE; ++x) { const u32 h = H[TERRAIN_VERTS * (RT_TILE * tz + z) + RT_TILE * tx + x]; lo = min(lo, h); hi = max(hi, h); }
	tiles[chunk * (RT_TILES * RT_TILES) + tile] = (hi << 16) | lo;
	for (int k = 32; k > 0; k >>= 1) { lo = min(lo, (u32)__shfl_xor(lo, k)); hi = max(hi, (u32)__shfl_xor(hi, k)); }
	if ((threadIdx.x & 63u) == 0u) { sLo[threadIdx.x >> 6] = lo; sHi[threadIdx.x >> 6] = hi; }
	__syncthreads();
	if (threadIdx.x == 0u) chunkRange[chunk] = (max(max(sHi[0], sHi[1]), max(sHi[2], sHi[3])) << 16) | min(min(sLo[0], sLo[1]), min(sLo[2], sLo[3]));
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// The walk runs in its own parameter s = t * dmax (dmax = the direction's largest |component|), with the direction divided by dmax:
// the axis the ray moves fastest along has |component| 1, nothing overflows for a tiny or huge direction, and an axis whose component
// is below 1e-12 of the largest is treated as not moved along (over the terrain's extent it moves 1e-12 of that extent, far below
// the slack), so nothing divides by zero: a vertical ray covers one cell column, or up to four cells when its origin lies on grid lines.
struct RtRay
{
	V3 o, d; float dmax;             // d: direction / dmax
	bool parX, parY, parZ;
	float slack, slackY;
};
MI_DEV int rtIndex(float v, int lo, int hi) { return (int)fminf(fmaxf(floorf(v), (float)lo), (float)hi); } // (a NaN gives lo)

// The squares (ix, iz), ix0 <= ix <= ix1, iz0 <= iz <= iz1, of a grid with lines gx + ix * s, gz + iz * s whose slack-widened extent
// the ray touches within [sa, sb] (walk parameter), front to back along the axis the ray moves faster on: visit(ix, iz, a, b) with
// [a, b] the widened interval the ray spends in the square's column; visit returns true to end this sweep (nothing further along
// can be entered before the best hit).  Conservative: a square is left out only if the widened ray misses its widened column.
template <class F>
MI_DEV void rtSweep(const RtRay& q, float gx, float gz, float s, int ix0, int ix1, int iz0, int iz1, float sa, float sb, F&& visit)
{
	const float invS = 1.f / s;
	if (q.parX && q.parZ)
	{
		const int xa = rtIndex((q.o.x - q.slack - gx) * invS, ix0, ix1), xb = rtIndex((q.o.x + q.slack - gx) * invS, ix0, ix1);
		const int za = rtIndex((q.o.z - q.slack - gz) * invS, iz0, iz1), zb = rtIndex((q.o.z + q.slack - gz) * invS, iz0, iz1);
		for (int iz = za; iz <= zb; ++iz) for (int ix = xa; ix <= xb; ++ix) if (visit(ix, iz, sa, sb)) return;
		return;
	}
	const bool majorX = !q.parX && (q.parZ || fabsf(q.d.x) >= fabsf(q.d.z));
	const float om = majorX ? q.o.x : q.o.z, dm = majorX ? q.d.x : q.d.z, gm = majorX ? gx : gz;
	const float on = majorX ? q.o.z : q.o.x, dn = majorX ? q.d.z : q.d.x, gn = majorX ? gz : gx;
	const int m0 = majorX ? ix0 : iz0, m1 = majorX ? ix1 : iz1, n0 = majorX ? iz0 : ix0, n1 = majorX ? iz1 : ix1;
	const float invM = 1.f / dm, slackS = q.slack * fabsf(invM);
	const float pa = om + sa * dm, pb = om + sb * dm;
	const int ma = rtIndex((fminf(pa, pb) - q.slack - gm) * invS, m0, m1), mb = rtIndex((fmaxf(pa, pb) + q.slack - gm) * invS, m0, m1);
	for (int k = 0; k <= mb - ma; ++k)
	{
		const int im = dm > 0.f ? ma + k : mb - k;
		const float s0 = ((gm + (float)im * s - q.slack) - om) * invM, s1 = ((gm + (float)(im + 1) * s + q.slack) - om) * invM;
		const float a = fmaxf(fminf(s0, s1) - slackS, sa), b = fminf(fmaxf(s0, s1) + slackS, sb);
		if (a > b) continue;
		const float na = on + a * dn, nb = on + b * dn;
		const int ia = rtIndex((fminf(na, nb) - q.slack - gn) * invS, n0, n1), ib = rtIndex((fmaxf(na, nb) + q.slack - gn) * invS, n0, n1);
		for (int j = 0; j <= ib - ia; ++j)
		{
			const int in = dn >= 0.f ? ia + j : ib - j;
			if (visit(majorX ? im : in, majorX ? in : im, a, b)) return;
		}
	}
}
// Does the ray's height over [a, b], widened by slackY, miss the heights [lo, hi] (uint16)?  (A NaN does not miss.)
MI_DEV bool rtMissesHeights(const RtRay& q, const TerrainParams& P, float a, float b, u32 lo, u32 hi)
{
	const float ya = q.o.y + a * q.d.y, yb = q.o.y + b * q.d.y;
	return fminf(ya, yb) - q.slackY > (float)hi * P.heightScale + P.minY || fmaxf(ya, yb) + q.slackY < (float)lo * P.heightScale + P.minY;
}

// Ray i: reads the record k_raycast wrote, replaces it if a terrain triangle is hit strictly before the collider.
template <bool BRUTE>
MI_DEV void rtRay(u32 i, const float4* __restrict__ rays, float4* __restrict__ out, const TerrainParams& P, const uint16_t* __restrict__ heights,
	const u32* __restrict__ valid, const u32* __restrict__ tiles, const u32* __restrict__ chunkRange)
{
	const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
	if (r1.w == 0.f) return;
	const float4 rec = out[2 * i];
	const bool colHit = mi_f2u(rec.w) != 0u;
	const float colT = colHit ? rec.x : MI_FLT_MAX, maxT = r0.w;
	const V3 o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z), corner = v3(P.minX, P.minY, P.minZ);
	const int cpd = (int)P.chunksPerDim;
	RtBest best; best.t = MI_FLT_MAX; best.id = RT_NO_TRIANGLE; best.point = v3s(0.f);
	if (BRUTE)
	{
		for (u32 chunk = 0; chunk < P.chunksPerDim * P.chunksPerDim; ++chunk)
		{
			if (!valid[chunk]) continue;
			const V3 chunkMin = terrainChunkMin(P, corner, chunk % P.chunksPerDim, chunk / P.chunksPerDim);
			const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
			for (u32 cz = 0; cz < RT_CELLS; ++cz)
				for (u32 cx = 0; cx < RT_CELLS; ++cx)
					rtCell(P, chunkMin, chunk, cx, cz, H[TERRAIN_VERTS * cz + cx], H[TERRAIN_VERTS * (cz + 1) + cx], H[TERRAIN_VERTS * cz + cx + 1], H[TERRAIN_VERTS * (cz + 1) + cx + 1], o, d, maxT, colHit, colT, best);
		}
	}
	else
	{
		const V3 ad = vabs(d), ao = vabs(o);
		RtRay q; q.o = o; q.dmax = fmaxf(fmaxf(ad.x, ad.y), ad.z);
		const float oMax = fmaxf(fmaxf(ao.x, ao.y), ao.z);
		if (!(q.dmax > 0.f && q.dmax <= MI_FLT_MAX && oMax <= MI_FLT_MAX)) return; // a zero direction misses; so does every triangle test of a ray that is not finite
		q.d = v3(d.x / q.dmax, d.y / q.dmax, d.z / q.dmax);
		q.parX = !(ad.x > 1e-12f * q.dmax); q.parY = !(ad.y > 1e-12f * q.dmax); q.parZ = !(ad.z > 1e-12f * q.dmax);
		// the terrain's box, the slack, the clip
		const float span = P.chunkSize * (float)cpd, top = 65535.f * P.heightScale;
		const V3 bmin = corner, bmax = corner + v3(span, top, span);
		const V3 am = vmax(vabs(bmin), vabs(bmax));
		q.slack = RT_SLACK_ULPS * RT_EPS * (oMax + fmaxf(fmaxf(am.x, am.y), am.z));
		q.slackY = q.slack * (4.f + 8.f * fabsf(top) / P.chunkScale);
		float sa = 0.f, sb = fminf(maxT, colT) * q.dmax; // (+inf stays +inf until an axis the ray moves along clips it)
		bool outside = false;
		{
			const float oo[3] = { o.x, o.y, o.z }, dd[3] = { q.d.x, q.d.y, q.d.z }, lo[3] = { bmin.x - q.slack, fminf(bmin.y, bmax.y) - q.slackY, bmin.z - q.slack },
				hi[3] = { bmax.x + q.slack, fmaxf(bmin.y, bmax.y) + q.slackY, bmax.z + q.slack };
			const bool par[3] = { q.parX, q.parY, q.parZ };
			#pragma unroll
			for (u32 k = 0; k < 3; ++k)
			{
				if (par[k]) outside = outside || oo[k] < lo[k] || oo[k] > hi[k];
				else { const float inv = 1.f / dd[k], t1 = (lo[k] - oo[k]) * inv, t2 = (hi[k] - oo[k]) * inv, w = q.slack * fabsf(inv); sa = fmaxf(sa, fminf(t1, t2) - w); sb = fminf(sb, fmaxf(t1, t2) + w); }
			}
		}
		if (outside || sa > sb) return;
		rtSweep(q, P.minX, P.minZ, P.chunkSize, 0, cpd - 1, 0, cpd - 1, sa, sb, [&](int X, int Z, float a, float b) -> bool
		{
			if (a > best.t * q.dmax) return true;
			const u32 chunk = (u32)Z * P.chunksPerDim + (u32)X;
			if (!valid[chunk]) return false;
			const u32 cr = chunkRange[chunk];
			if (rtMissesHeights(q, P, a, b, cr & 0xFFFFu, cr >> 16)) return false;
			const V3 chunkMin = terrainChunkMin(P, corner, (u32)X, (u32)Z);
			const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
			rtSweep(q, chunkMin.x, chunkMin.z, P.chunkScale * (float)RT_TILE, 0, (int)RT_TILES - 1, 0, (int)RT_TILES - 1, a, b, [&](int tx, int tz, float ta, float tb) -> bool
			{
				if (ta > best.t * q.dmax) return true;
				const u32 tr = tiles[chunk * (RT_TILES * RT_TILES) + (u32)tz * RT_TILES + (u32)tx];
				if (rtMissesHeights(q, P, ta, tb, tr & 0xFFFFu, tr >> 16)) return false;
				rtSweep(q, chunkMin.x, chunkMin.z, P.chunkScale, tx * (int)RT_TILE, tx * (int)RT_TILE + (int)RT_TILE - 1, tz * (int)RT_TILE, tz * (int)RT_TILE + (int)RT_TILE - 1, ta, tb, [&](int cx, int cz, float ca, float cb) -> bool
				{
					if (ca > best.t * q.dmax) return true;
					const u32 ha = H[TERRAIN_VERTS * (u32)cz + (u32)cx], hb = H[TERRAIN_VERTS * ((u32)cz + 1u) + (u32)cx], hc = H[TERRAIN_VERTS * (u32)cz + (u32)cx + 1u], hd = H[TERRAIN_VERTS * ((u32)cz + 1u) + (u32)cx + 1u];
					if (rtMissesHeights(q, P, ca, cb, min(min(ha, hb), min(hc, hd)), max(max(ha, hb), max(hc, hd)))) return false;
					rtCell(P, chunkMin, chunk, (u32)cx, (u32)cz, ha, hb, hc, hd, o, d, maxT, colHit, colT, best);
					return false;
				});
				return false;
			});
			return false;
		});
	}
	if (best.id == RT_NO_TRIANGLE) return;
	out[2 * i] = make_float4(best.t, mi_u2f(MI_TERRAIN_COLLIDER), mi_u2f(MI_STATIC_BODY), mi_u2f(1u));
	out[2 * i + 1] = make_float4(best.point.x, best.point.y, best.point.z, mi_u2f(best.id));
}
template <bool BRUTE>
__global__ void __launch_bounds__(64) k_rc_terrain(u32 numRays, const float4* __restrict__ rays, float4* __restrict__ out, TerrainParams P, const uint16_t* __restrict__ heights,
	const u32* __restrict__ valid, const u32* __restrict__ tiles, const u32* __restrict__ chunkRange)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < numRays) rtRay<BRUTE>(i, rays, out, P, heights, valid, tiles, chunkRange);
}

void launch_raycast_terrain(World& w, u32 numRays, const float* dRays, u32 flags, mi_ray_hit* dOutHits)
{
	const u32 chunks = w.terrain.chunksPerDim * w.terrain.chunksPerDim;
	if (!chunks || !numRays) return;
	const TerrainParams P = terrainParams(w);
	if (flags & MI_RAY_BRUTE_FORCE)
	{
		hipLaunchKernelGGL(k_rc_terrain<true>, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, (const float4*)dRays, (float4*)dOutHits, P, w.terrain.heights.p, w.terrain.valid.p, (const u32*)nullptr, (const u32*)nullptr);
		return;
	}
	if (!w.queries.terrainTableValid)
	{
		w.queries.terrainTiles.ensure((size_t)chunks * RT_TILES * RT_TILES, w.stream); w.queries.terrainChunkRange.ensure(chunks, w.stream);
		if (w.lastError) return;
		hipLaunchKernelGGL(k_rc_terrain_tiles, dim3(chunks), dim3(256), 0, w.stream, w.terrain.heights.p, w.queries.terrainTiles.p, w.queries.terrainChunkRange.p);
		w.queries.terrainTableValid = true;
	}
	hipLaunchKernelGGL(k_rc_terrain<false>, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, (const float4*)dRays, (float4*)dOutHits, P, w.terrain.heights.p, w.terrain.valid.p, w.queries.terrainTiles.p, w.queries.terrainChunkRange.p);
}
