// mi_test_physics_interaction_batch: testPhysicsInteraction (physics.cpp:556-628) for many rays, one lane per ray.  Ray i tests only
// the colliders of its own body range, so lanes never share a body: the push is a plain read-add-write of the accumulators, with no
// atomics, and the result does not depend on the schedule.  The ray tests are those of the host entry point (ray_tests.h); the hull
// table and the shape words of a collider record are the world queries' (RcHulls, rcShape: raycast_shared.h).
#include "world.h"
#include "ray_tests.h"
#include "raycast_shared.h"

__global__ void __launch_bounds__(64) k_interaction_batch(u32 numRays, u32 firstBody, u32 bodiesPerRay, const float4* __restrict__ rays, int32_t* __restrict__ outBody,
	const float4* __restrict__ pose, const float4* __restrict__ bprops, const uint8_t* __restrict__ alive, const ColliderRec* __restrict__ cols,
	const u32* __restrict__ colStart, const u32* __restrict__ colList, RcHulls hulls, float4* __restrict__ force)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numRays) return;
	const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
	if (r1.w == 0.f) { outBody[i] = 0; return; }
	const HRay r{ v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z) };
	float minT = MI_FLT_MAX; int minBody = -1; u32 minCol = 0xFFFFFFFFu; V3 f = v3s(0.f), tq = v3s(0.f);
	const u32 b0 = firstBody + i * bodiesPerRay;
	for (u32 b = b0; b < b0 + bodiesPerRay; ++b)
	{
		if (!alive[b]) continue;
		const float4 p = pose[2 * b], q = pose[2 * b + 1];
		const Q4 rot = q4f4(q); const V3 pos = v3(p.x, p.y, p.z);
		for (u32 k = colStart[b]; k < colStart[b + 1]; ++k)
		{
			const u32 c = colList[k];
			const ColliderRec rec = cols[c];
			float s[10]; HRay lr; float t;
			rcShape(rec, s);
			// the host walks all colliders in index order and keeps the first of equal distances: the same choice here
			if (rayBodyCollider(r, rot, pos, colType(rec), s, hulls, lr, t) && (t < minT || (minBody >= 0 && t == minT && c < minCol)))
			{
				minT = t; minBody = (int)b; minCol = c;
				interactionPush(r, lr, t, rot, pos, v3f4(bprops[5 * b]), r0.w, f, tq);
			}
		}
	}
	if (minBody < 0) { outBody[i] = 0; return; }
	float4 fa = force[2 * minBody], ta = force[2 * minBody + 1];
	fa.x += f.x; fa.y += f.y; fa.z += f.z; ta.x += tq.x; ta.y += tq.y; ta.z += tq.z;
	force[2 * minBody] = fa; force[2 * minBody + 1] = ta;
	outBody[i] = 1 + minBody;
}

void launch_interaction_batch(World& w, u32 numRays, u32 firstBody, u32 bodiesPerRay, const float* dRays, int32_t* dOutBody)
{
	hipLaunchKernelGGL(k_interaction_batch, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, firstBody, bodiesPerRay, (const float4*)dRays, dOutBody,
		w.pose.p, w.bprops.p, w.aliveMask.p, w.colLocal.p, w.queries.bodyColStart.p, w.queries.bodyColList.p, rcHulls(w), w.force.p);
}
