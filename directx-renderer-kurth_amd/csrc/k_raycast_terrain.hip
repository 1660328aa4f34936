// MI_RAY_TERRAIN: the heightmap terrain as a candidate of mi_raycast_batch ("Whole-world ray casts": the terrain).  Runs
// after k_raycast on the records it wrote (or on zeroed records when no collider is a candidate) and replaces a record where a terrain
// triangle is hit strictly before the collider.
//   k_rc_terrain_tiles   uint16 min / max of the heights per 8 x 8-cell tile (16 x 16 tiles per chunk) and per chunk; built when the
//                        heights changed (World::queries.terrainTableValid), on the world's stream, before the next terrain query
//                        (launch_terrain_tables: the proximity and sphere-cast terrain passes read the same table)
//   k_rc_terrain<false>  one lane per ray: clip to the terrain's box, walk chunks -> tiles -> cells under the ray front to back
//                        (the sweep, its slack and the table's constants: terrain_walk.h)
//   k_rc_terrain<true>   MI_RAY_BRUTE_FORCE: the same cell body (rtCell) over every cell of every valid chunk, no table
// The triangles are k_heightmap's: (A, B, C) and (C, B, D) of terrainCellVertices.  The hit rule is stated in include/mi_physics.h.
#include "world.h"
#include "terrain_walk.h"

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

// ---- the walk (RtRay, rtSweep, rtMissesHeights: terrain_walk.h) -------------------------------------------------------------------
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

bool launch_terrain_tables(World& w)
{
	const u32 chunks = w.terrain.chunksPerDim * w.terrain.chunksPerDim;
	if (w.queries.terrainTableValid || !chunks) return !w.lastError;
	w.queries.terrainTiles.ensure((size_t)chunks * RT_TILES * RT_TILES, w.stream); w.queries.terrainChunkRange.ensure(chunks, w.stream);
	if (w.lastError) return false;
	hipLaunchKernelGGL(k_rc_terrain_tiles, dim3(chunks), dim3(256), 0, w.stream, w.terrain.heights.p, w.queries.terrainTiles.p, w.queries.terrainChunkRange.p);
	w.queries.terrainTableValid = true;
	return true;
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
	if (!launch_terrain_tables(w)) return;
	hipLaunchKernelGGL(k_rc_terrain<false>, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, (const float4*)dRays, (float4*)dOutHits, P, w.terrain.heights.p, w.terrain.valid.p, w.queries.terrainTiles.p, w.queries.terrainChunkRange.p);
}
