// MI_SPHERE_TERRAIN: the heightmap terrain as candidates of mi_sphere_cast_batch, a two-sided sheet of triangles (DESIGN.md,
// "Proximity and sphere casts over the terrain"; the rule is stated in include/mi_physics.h, its float32 operation order in
// terrain_point.h on top of sphere_cast.h).  Runs after k_sphere_cast on the records it wrote (zeroed ones when no collider is a
// candidate) and replaces a record where a triangle is touched strictly before the collider.
//   (launch_terrain_tables) the min / max table of the heights per 8 x 8-cell tile and per chunk (terrain_walk.h), the ray cast's
//   k_sc_terrain<false>     one lane per query: the world cast again by rcMount (the same bytes k_sphere_cast formed), then rtSweep
//                           front to back over chunks -> tiles -> cells with the slack grown by the sphere, the march of both
//                           triangles in each cell (tpCastCell)
//   k_sc_terrain<true>      MI_SPHERE_BRUTE_FORCE: the same cell body over every cell of every valid chunk, no table
// A triangle's answer is decided by sphereCastMarch on its vertices and the query alone; the best t so far (the collider's at first)
// only ends a march that is strictly beyond it and cannot win, so the walk and brute force agree in every byte.
//
// The slack.  A march stops on a triangle at t only if its computed gap |centre - c_f| - radius <= tol(t), i.e. the computed c_f is within
// radius + tol(t) + rounding of the rounded centre fl(o + t v).  c_f lies in the triangle's box up to e (k_proximity_terrain.hip derives
// e <= 16 eps M (1 + S^2) with S the largest slope in the box), the rounded centre on the exact line up to 3 eps (|o| + t L), and
// tol(t) <= SC_GAP + 16 eps (|o| + reach + radius), with reach the length of the path on which a touch is possible at all (the sphere's
// centre is then within radius + tol of the terrain's box: k_spherecast.hip's `reach`).  So every touched triangle's box, widened in x, z
// and height by slack(S) = radius + SC_GAP + SCT_SLACK_ULPS eps (|o|max + terrain|max| + reach + radius) (1 + S^2), holds the
// centre's exact position at t: the 16 + 16 + 3 above plus the ray walk's own 16 (terrain_walk.h), doubled: SCT_SLACK_ULPS = 128, as
// SC_SLACK_ULPS.  Each level sweeps with the slack of the box above it (the whole terrain: S = amplitude / cell; a chunk and a tile:
// their ranges in the table), which is >= the slack of every box inside.
// Why a widened column entered after the best t cannot hold an earlier touch: at a touch the centre is inside the widened box of
// the touched triangle, hence inside the widened column of its cell, tile and chunk, so the column was entered at or before that t;
// the sweep is front to back in entry, so every column still to come is entered later too.
#include "world.h"
#include "terrain_point.h"
#include "terrain_walk.h"
#include "raycast_shared.h"

#define SCT_SLACK_ULPS 128.f

struct SctSlack { float grow, base, invCell; };
MI_DEV float sctSlack(const TerrainParams& P, const SctSlack& s, u32 lo, u32 hi)
{
	const float S = (float)(hi - lo) * P.heightScale * s.invCell;
	return s.grow + s.base * (1.f + S * S);
}

// queries, out: k_sphere_cast's.  nb, pose, alive, simMask: rcMount's.
template <bool BRUTE>
__global__ void __launch_bounds__(64) k_sc_terrain(u32 numQueries, const float4* __restrict__ queries, float4* __restrict__ out, u32 nb, const float4* __restrict__ pose,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, TerrainParams P, const uint16_t* __restrict__ heights, const u32* __restrict__ valid,
	const u32* __restrict__ tiles, const u32* __restrict__ chunkRange)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numQueries) return;
	const float4 q0 = queries[3 * i], q1 = queries[3 * i + 1], q2 = queries[3 * i + 2];
	if (mi_f2u(q2.w) == 0u) return;
	V3 o = v3(q0.x, q0.y, q0.z), d = v3(q1.x, q1.y, q1.z);
	const float maxT = q0.w, radius = q1.w;
	{
		Q4 rot; V3 pos;
		const RcMount m = rcMount(mi_f2u(q2.x), nb, pose, alive, simMask, rot, pos);
		if (m == RC_MOUNT_OFF) return;
		if (m == RC_MOUNT_BODY) { o = rot * o + pos; d = rot * d; }
	}
	if (!(radius >= 0.f && maxT >= 0.f)) return; // (a negative or NaN radius and a negative or NaN maxT find nothing)
	const V3 ad = vabs(d), ao = vabs(o);
	const float dmax = fmaxf(fmaxf(ad.x, ad.y), ad.z), oMax = fmaxf(fmaxf(ao.x, ao.y), ao.z);
	if (!(dmax <= MI_FLT_MAX && oMax <= MI_FLT_MAX && radius <= MI_FLT_MAX)) return; // a cast that is not finite does not meet the terrain (the walk and brute force alike)
	const float L = length(d);
	const float4 rec = out[3 * i];
	const float colT = mi_f2u(rec.w) != 0u ? rec.x : __builtin_inff();
	const V3 corner = v3(P.minX, P.minY, P.minZ);
	const u32 cpd = P.chunksPerDim;
	TpCast best; best.t = colT; best.gap = 0.f; best.id = TP_NO_TRIANGLE; best.hit = 0u; best.iterations = 0u; best.c = v3s(0.f); best.n = v3s(0.f);
	if (BRUTE)
	{
		for (u32 chunk = 0; chunk < cpd * cpd; ++chunk)
		{
			if (!valid[chunk]) continue;
			const V3 chunkMin = terrainChunkMin(P, corner, chunk % cpd, chunk / cpd);
			const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
			for (u32 cz = 0; cz < RT_CELLS; ++cz)
				for (u32 cx = 0; cx < RT_CELLS; ++cx)
					tpCastCell(P, chunkMin, chunk, cx, cz, H[TERRAIN_VERTS * cz + cx], H[TERRAIN_VERTS * (cz + 1) + cx], H[TERRAIN_VERTS * cz + cx + 1], H[TERRAIN_VERTS * (cz + 1) + cx + 1], o, d, L, radius, maxT, best);
		}
	}
	else
	{
		const bool still = !(dmax > 0.f);             // a zero direction is an overlap test at the origin: the cells around it
		RtRay q; q.o = o; q.dmax = still ? 1.f : dmax;
		q.d = still ? v3s(0.f) : v3(d.x / dmax, d.y / dmax, d.z / dmax);
		q.parX = still || !(ad.x > 1e-12f * dmax); q.parY = still || !(ad.y > 1e-12f * dmax); q.parZ = still || !(ad.z > 1e-12f * dmax);
		const float span = P.chunkSize * (float)cpd, top = 65535.f * P.heightScale;
		const V3 bmin = corner, bmax = corner + v3(span, top, span);
		const V3 am = vmax(vabs(bmin), vabs(bmax));
		const float scene = fmaxf(fmaxf(am.x, am.y), am.z);
		const float reach = fminf(maxT * L, 2.f * ((oMax + scene) + radius) + 1.f); // (inf * 0 = NaN: fminf keeps the other)
		SctSlack sl; sl.grow = radius + SC_GAP; sl.base = SCT_SLACK_ULPS * RT_EPS * (((oMax + scene) + reach) + radius); sl.invCell = 1.f / P.chunkScale;
		q.slack = q.slackY = sctSlack(P, sl, 0u, 65535u);
		float sa = 0.f, sb = fminf(maxT, colT) * q.dmax; // (+inf stays +inf until an axis the cast moves along clips it)
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
		rtSweep(q, P.minX, P.minZ, P.chunkSize, 0, (int)cpd - 1, 0, (int)cpd - 1, sa, sb, [&](int X, int Z, float a, float b) -> bool
		{
			if (a > best.t * q.dmax) return true;
			const u32 chunk = (u32)Z * cpd + (u32)X;
			if (!valid[chunk]) return false;
			const u32 cr = chunkRange[chunk];
			RtRay qc = q; qc.slack = qc.slackY = sctSlack(P, sl, cr & 0xFFFFu, cr >> 16);
			if (rtMissesHeights(qc, P, a, b, cr & 0xFFFFu, cr >> 16)) return false;
			const V3 chunkMin = terrainChunkMin(P, corner, (u32)X, (u32)Z);
			const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
			rtSweep(qc, chunkMin.x, chunkMin.z, P.chunkScale * (float)RT_TILE, 0, (int)RT_TILES - 1, 0, (int)RT_TILES - 1, a, b, [&](int tx, int tz, float ta, float tb) -> bool
			{
				if (ta > best.t * q.dmax) return true;
				const u32 tr = tiles[chunk * (RT_TILES * RT_TILES) + (u32)tz * RT_TILES + (u32)tx];
				RtRay qt = q; qt.slack = qt.slackY = sctSlack(P, sl, tr & 0xFFFFu, tr >> 16);
				if (rtMissesHeights(qt, P, ta, tb, tr & 0xFFFFu, tr >> 16)) return false;
				rtSweep(qt, chunkMin.x, chunkMin.z, P.chunkScale, tx * (int)RT_TILE, tx * (int)RT_TILE + (int)RT_TILE - 1, tz * (int)RT_TILE, tz * (int)RT_TILE + (int)RT_TILE - 1, ta, tb, [&](int cx, int cz, float ca, float cb) -> bool
				{
					if (ca > best.t * q.dmax) return true;
					const u32 ha = H[TERRAIN_VERTS * (u32)cz + (u32)cx], hb = H[TERRAIN_VERTS * ((u32)cz + 1u) + (u32)cx], hc = H[TERRAIN_VERTS * (u32)cz + (u32)cx + 1u], hd = H[TERRAIN_VERTS * ((u32)cz + 1u) + (u32)cx + 1u];
					if (rtMissesHeights(qt, P, ca, cb, min(min(ha, hb), min(hc, hd)), max(max(ha, hb), max(hc, hd)))) return false;
					tpCastCell(P, chunkMin, chunk, (u32)cx, (u32)cz, ha, hb, hc, hd, o, d, L, radius, maxT, best);
					return false;
				});
				return false;
			});
			return false;
		});
	}
	if (best.id == TP_NO_TRIANGLE) return;
	out[3 * i] = make_float4(best.t, mi_u2f(MI_TERRAIN_COLLIDER), mi_u2f(MI_STATIC_BODY), mi_u2f(best.hit));
	out[3 * i + 1] = make_float4(best.c.x, best.c.y, best.c.z, best.gap);
	out[3 * i + 2] = make_float4(best.n.x, best.n.y, best.n.z, mi_u2f(best.iterations));
}

void launch_sphere_cast_terrain(World& w, u32 n, const mi_sphere_cast* dQueries, u32 flags, mi_sphere_hit* dOut)
{
	const u32 chunks = w.terrain.chunksPerDim * w.terrain.chunksPerDim;
	if (!chunks || !n) return;
	const bool brute = (flags & MI_SPHERE_BRUTE_FORCE) != 0;
	if (!brute && !launch_terrain_tables(w)) return;
	const TerrainParams P = terrainParams(w);
	hipLaunchKernelGGL(brute ? k_sc_terrain<true> : k_sc_terrain<false>, dim3((n + 63) / 64), dim3(64), 0, w.stream, n, (const float4*)dQueries, (float4*)dOut, w.nb, w.pose.p,
		w.aliveMask.p, w.simMask.p, P, w.terrain.heights.p, w.terrain.valid.p, brute ? (const u32*)nullptr : w.queries.terrainTiles.p, brute ? (const u32*)nullptr : w.queries.terrainChunkRange.p);
}
