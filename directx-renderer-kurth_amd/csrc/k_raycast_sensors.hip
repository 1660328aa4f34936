// mi_raycast_sensors: rays given in the frame of a body, a body range per ray that is no candidate, and the hit normal (DESIGN.md,
// "Body-mounted ray sensors"; the rule is stated in include/mi_physics.h).  Around the one traversal of mi_raycast_batch:
//   k_rc_sensor_rays      one lane per ray: the world ray from the mount's current pose (rcMount, raycast_shared.h, on World::pose, the
//                         array the cast reads) into the caller's buffer or World::queries.sensorRays, and the exclusion range into
//                         World::queries.sensorExclude
//   (launch_raycast)      the BVH of k_raycast.hip, built once; k_raycast<.., EXCLUDE = true> writes 32-byte records into
//                         World::queries.sensorHits; with MI_RAY_TERRAIN k_rc_terrain runs on them unchanged
//   k_rc_sensor_normals   one lane per ray: the winning collider again (rcFetch), its local ray (the expression of rayBodyCollider), the normal
//                         rule of ray_normals.h, or the terrain triangle from its id; writes the 48-byte records
// The two passes are kernels of their own and not folded into k_raycast: that kernel sits at 75 VGPRs with its 16 KiB stack, and the
// normal of a hull repeats the hull's triangle loop, which inside the traversal would run for every leaf that improves the best hit.
#include "world.h"
#include "ray_normals.h"
#include "raycast_shared.h"
#include "terrain_shared.h"

#define RS_CELLS (TERRAIN_VERTS - 1u)

// in: 3 x float4 per ray = mi_sensor_ray {origin.xyz, maxT}, {direction.xyz, enabled}, {mount, excludeFirst, excludeCount, reserved} (bits).
__global__ void __launch_bounds__(256) k_rc_sensor_rays(u32 numRays, const float4* __restrict__ in, u32 nb, const float4* __restrict__ pose, const uint8_t* __restrict__ alive,
	const uint8_t* __restrict__ simMask, float4* __restrict__ worldRays, uint2* __restrict__ exclude)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numRays) return;
	const float4 r0 = in[3 * i], r1 = in[3 * i + 1], r2 = in[3 * i + 2];
	Q4 rot; V3 pos;
	const RcMount m = rcMount(mi_f2u(r2.x), nb, pose, alive, simMask, rot, pos);
	float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0; // off: the ray is disabled
	if (m == RC_MOUNT_WORLD) { w0 = r0; w1 = r1; }
	else if (m == RC_MOUNT_BODY)
	{
		const V3 o = rot * v3(r0.x, r0.y, r0.z) + pos, d = rot * v3(r1.x, r1.y, r1.z);
		w0 = make_float4(o.x, o.y, o.z, r0.w); w1 = make_float4(d.x, d.y, d.z, r1.w);
	}
	worldRays[2 * i] = w0; worldRays[2 * i + 1] = w1;
	exclude[i] = make_uint2(mi_f2u(r2.y), mi_f2u(r2.z));
}

// The triangle of a terrain hit from its id (include/mi_physics.h): noz(cross(b - a, c - a)) as rtTriangle forms it; no pose rotation.
MI_DEV V3 rsTerrainNormal(u32 id, const TerrainParams& P, const uint16_t* __restrict__ heights)
{
	const u32 which = id & 1u, cell = (id >> 1) % (RS_CELLS * RS_CELLS), chunk = (id >> 1) / (RS_CELLS * RS_CELLS), cx = cell % RS_CELLS, cz = cell / RS_CELLS;
	const uint16_t* H = heights + (size_t)chunk * TERRAIN_VERTS * TERRAIN_VERTS;
	const V3 chunkMin = terrainChunkMin(P, v3(P.minX, P.minY, P.minZ), chunk % P.chunksPerDim, chunk / P.chunksPerDim);
	V3 A, B, C, D;
	terrainCellVertices(P, chunkMin, cx, cz, H[TERRAIN_VERTS * cz + cx], H[TERRAIN_VERTS * (cz + 1) + cx], H[TERRAIN_VERTS * cz + cx + 1], H[TERRAIN_VERTS * (cz + 1) + cx + 1], A, B, C, D);
	return which == 0u ? noz(cross(B - A, C - A)) : noz(cross(B - C, D - C));
}

// hits: the 32-byte records of k_raycast / k_rc_terrain; out: 3 x float4 per ray = mi_sensor_hit.
__global__ void __launch_bounds__(64) k_rc_sensor_normals(u32 numRays, const float4* __restrict__ worldRays, const float4* __restrict__ hits, float4* __restrict__ out, RcScene sc,
	TerrainParams P, const uint16_t* __restrict__ heights)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numRays) return;
	const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
	V3 n = v3s(0.f);
	if (mi_f2u(h0.w) != 0u)
	{
		const u32 c = mi_f2u(h0.y);
		if (c == MI_TERRAIN_COLLIDER) n = rsTerrainNormal(mi_f2u(h1.w), P, heights);
		else
		{
			const float4 r0 = worldRays[2 * i], r1 = worldRays[2 * i + 1];
			RcCollider col;
			rcFetch(sc, c, RcExclude{ 0u, 0u }, col); // (the winner was no excluded one)
			const HRay lr{ conjugate(col.rot) * (v3(r0.x, r0.y, r0.z) - col.pos), conjugate(col.rot) * v3(r1.x, r1.y, r1.z) }; // rayBodyCollider's lr
			n = col.rot * rayBodyColliderNormal(lr, h0.x, col.type, col.s, sc.hulls);
		}
	}
	out[3 * i] = h0; out[3 * i + 1] = h1; out[3 * i + 2] = make_float4(n.x, n.y, n.z, 0.f);
}

void launch_raycast_sensors(World& w, u32 numRays, const mi_sensor_ray* dRays, u32 flags, bool terrain, mi_sensor_hit* dOutHits, float* dOutWorldRays)
{
	w.queries.sensorHits.ensure(2 * (size_t)numRays, w.stream); w.queries.sensorExclude.ensure(numRays, w.stream);
	if (!dOutWorldRays) w.queries.sensorRays.ensure(2 * (size_t)numRays, w.stream);
	if (w.lastError) return;
	float4* worldRays = dOutWorldRays ? (float4*)dOutWorldRays : w.queries.sensorRays.p;
	hipLaunchKernelGGL(k_rc_sensor_rays, dim3((numRays + 255) / 256), dim3(256), 0, w.stream, numRays, (const float4*)dRays, w.nb, w.pose.p, w.aliveMask.p, w.simMask.p, worldRays, w.queries.sensorExclude.p);
	launch_raycast(w, numRays, (const float*)worldRays, flags, (mi_ray_hit*)w.queries.sensorHits.p, w.queries.sensorExclude.p); // (no candidate collider: the records are zeroed)
	if (terrain && !w.lastError) launch_raycast_terrain(w, numRays, (const float*)worldRays, flags, (mi_ray_hit*)w.queries.sensorHits.p);
	if (w.lastError) return;
	hipLaunchKernelGGL(k_rc_sensor_normals, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, (const float4*)worldRays, (const float4*)w.queries.sensorHits.p, (float4*)dOutHits, rcScene(w),
		terrainParams(w), w.terrain.heights.p);
}
