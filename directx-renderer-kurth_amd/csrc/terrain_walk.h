// What the terrain passes of the world queries share (k_raycast_terrain.hip, k_proximity_terrain.hip, k_spherecast_terrain.hip): the
// constants of the min/max tile table, the table's launch, and the front-to-back sweep of a ray over a square grid.
//   launch_terrain_tables   k_rc_terrain_tiles (k_raycast_terrain.hip) when World::queries.terrainTableValid says the heights changed
//   RtRay, rtIndex, rtSweep, rtMissesHeights   the ray walk's sweep; the sphere cast's walk runs it with a slack grown by its radius
#pragma once
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

// Builds World::queries.terrainTiles / terrainChunkRange on the world's stream if the heights changed since the last build
// (k_raycast_terrain.hip).  false: an allocation failed (World::lastError is set).
bool launch_terrain_tables(World& w);

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
