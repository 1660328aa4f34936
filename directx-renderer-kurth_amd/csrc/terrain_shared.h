// Heightmap terrain: what k_heightmap.hip (contacts) and k_raycast_terrain.hip (ray casts) share — the parameter block and the
// vertex formulas of a cell, so that a ray hits the triangles the bodies collide with (heightmap_collider.h:156-206).
#pragma once
#include "world.h"

#define TERRAIN_VERTS 129u

struct TerrainParams { u32 chunksPerDim; float chunkSize, invChunkSize, chunkScale, heightScale, invAmplitudeScale, minX, minY, minZ, friction, restitution; };

static inline TerrainParams terrainParams(const World& w)
{
	TerrainParams P;
	P.chunksPerDim = w.terrain.chunksPerDim; P.chunkSize = w.terrain.chunkSize; P.invChunkSize = 1.f / w.terrain.chunkSize; P.chunkScale = w.terrain.chunkSize / (TERRAIN_VERTS - 1);
	P.heightScale = w.terrain.amplitude / 65535; P.invAmplitudeScale = 1.f / w.terrain.amplitude;
	P.minX = w.terrain.minCorner[0]; P.minY = w.terrain.minCorner[1]; P.minZ = w.terrain.minCorner[2]; P.friction = w.terrain.material[1]; P.restitution = w.terrain.material[0];
	return P;
}

// Lower corner of chunk (x, z); `corner` = (P.minX, P.minY, P.minZ).
MI_DEV V3 terrainChunkMin(const TerrainParams& P, V3 corner, u32 x, u32 z) { return v3(x * P.chunkSize, 0.f, z * P.chunkSize) + corner; }
// The four vertices of cell (cx, cz) of a chunk from its four heights ha = H[cz][cx], hb = H[cz + 1][cx], hc = H[cz][cx + 1], hd = H[cz + 1][cx + 1].
// The cell's triangles are (A, B, C) and (C, B, D).
MI_DEV void terrainCellVertices(const TerrainParams& P, V3 chunkMin, u32 cx, u32 cz, u32 ha, u32 hb, u32 hc, u32 hd, V3& posA, V3& posB, V3& posC, V3& posD)
{
	float x0 = (float)cx * P.chunkScale, x1 = (float)(cx + 1) * P.chunkScale, z0 = (float)cz * P.chunkScale, z1 = (float)(cz + 1) * P.chunkScale;
	posA = v3(x0, ha * P.heightScale, z0) + chunkMin; posB = v3(x0, hb * P.heightScale, z1) + chunkMin;
	posC = v3(x1, hc * P.heightScale, z0) + chunkMin; posD = v3(x1, hd * P.heightScale, z1) + chunkMin;
}
