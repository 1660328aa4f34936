// Cloth collision (mi_cloth_set_collision; DESIGN.md, "Cloth collision"; the rule is stated in include/mi_physics.h): one projection
// pass per internal step over the particles of the cloths that have collision on, after k_cloth_simulate has written the step's
// positions and damped velocities, at the poses and velocities the step's velocity integration left.
//   (launch_raycast_build)  the queries' collider tree at the current poses (k_raycast.hip), with the static colliders if a colliding
//                           cloth wants them; in brute-force mode the leaves alone
//   (launch_terrain_tables) the terrain's min / max table, if a colliding cloth meets the terrain (terrain_walk.h)
//   k_cloth_collide         one lane per particle, read straight from the cloth planes, 64-lane workgroups that never span two cloths
//                           (a grid-ordered cloth makes a wave's particles neighbours: the walk stays coherent): the reading of
//                           mi_proximity for the particle (rcWalk with PxVisitor, then pxtSearch: proximity_shared.h, the code
//                           mi_proximity decides with), then the projection, fused: a lane reads and writes its own particle only
// Per-cloth differences (static flag, exclusion range, thickness) are applied in the leaf and in the projection, not in the tree.
// A cluster sweep that gave up: the kernel reads CTR_FLOW_STATUS and skips itself as k_integrate_velocities does; World::recoverFlow
// launches the pass again behind its own integration.
#include "proximity_shared.h"

#define CC_NONE 0xFFFFFFFFu
struct ClothCollideDesc { u32 firstParticle, numParticles, flags, exFirst, exCount; float thickness, friction; u32 pad; };
static_assert(sizeof(ClothCollideDesc) == 32, "one record per colliding cloth");

// descs, blocks: World::cloth.collideDescs, collideBlockList ({record, first particle of the workgroup within its cloth}).  planes: the
// cloth planes (position xyz, velocity xyz, previous position xyz, inverse mass) of `stride` floats.  built == 0: no tree, no collider found.
template <bool BRUTE, bool TERRAIN>
__global__ void __launch_bounds__(64) k_cloth_collide(const ClothCollideDesc* __restrict__ descs, const uint2* __restrict__ blocks, float* __restrict__ planes, size_t stride,
	u32* __restrict__ contacts, u32 built, RcScene sc, const float4* __restrict__ vel, const float4* __restrict__ bprops, const u32* __restrict__ flowStatus,
	TerrainParams P, const uint16_t* __restrict__ heights, const u32* __restrict__ valid, const u32* __restrict__ tiles, const u32* __restrict__ chunkRange)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	if (*flowStatus) return; // the cluster sweep gave up: poses and velocities are invalid, World::recoverFlow runs the pass after its integration
	const uint2 blk = blocks[blockIdx.x];
	const ClothCollideDesc d = descs[blk.x];
	const u32 k = blk.y + threadIdx.x;
	if (k >= d.numParticles) return;
	const size_t i = (size_t)d.firstParticle + k;
	if (!(planes[9 * stride + i] > 0.f)) { contacts[i] = CC_NONE; return; } // a fixed particle
	PxQuery q; q.p = v3(planes[i], planes[stride + i], planes[2 * stride + i]); q.radius = d.thickness; q.exFirst = d.exFirst; q.exCount = d.exCount; q.slackAbs = 0.f;

	// the reading: mi_proximity's, without MI_PROX_COUNT
	PxBest best = pxBestNone();
	PxVisitor<false> v{ q, sc, best, (d.flags & MI_CLOTH_COLLIDE_STATIC) != 0u };
	const u32 n = built ? sc.hdr[RC_N] : 0u;
	if (q.radius >= 0.f && n != 0u)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else
		{
			q.slackAbs = pxSlackAbs(q.p, sc);
			rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
		}
	}
	if (TERRAIN && (d.flags & MI_CLOTH_COLLIDE_TERRAIN) != 0u && q.radius >= 0.f)
	{
		const float pMax = pxtPointMax(q.p);
		if (pMax <= MI_FLT_MAX) // (a point that is not finite does not meet the terrain)
		{
			const TpBest tb = pxtSearch<BRUTE>(P, heights, valid, tiles, chunkRange, q.p, q.radius, pMax);
			if (tb.id != TP_NO_TRIANGLE)
			{
				const TpReading r = tpReading(q.p, tb);
				if (r.d <= q.radius && (best.col == PX_NONE || r.d < best.d)) // (a tie stays with the collider)
				{
					best.d = r.d; best.col = MI_TERRAIN_COLLIDER; best.body = MI_STATIC_BODY; best.c = r.c; best.n = r.n;
				}
			}
		}
	}
	if (best.col == PX_NONE || (best.n.x == 0.f && best.n.y == 0.f && best.n.z == 0.f)) { contacts[i] = CC_NONE; return; } // untouched, byte for byte

	// the projection
	const V3 nrm = best.n;
	const float push = d.thickness - best.d;
	const V3 p1 = q.p + nrm * push;
	V3 vs = v3s(0.f);
	if (best.body != MI_STATIC_BODY)
	{
		const u32 b = best.body;
		const V3 cogb = v3f4(sc.pose[2 * b]) + q4f4(sc.pose[2 * b + 1]) * v3f4(bprops[5 * b]); // (World::cog is one integration old here)
		vs = v3f4(vel[2 * b]) + cross(v3f4(vel[2 * b + 1]), best.c - cogb);
	}
	const V3 vp = v3(planes[3 * stride + i], planes[4 * stride + i], planes[5 * stride + i]);
	V3 u = vp - vs;
	const float un = dot(u, nrm);
	if (un < 0.f)
	{
		u = u - nrm * un;
		const float jn = -un, lt = length(u);
		if (d.friction > 0.f)
		{
			const float s = lt > d.friction * jn ? 1.f - (d.friction * jn) / lt : 0.f;
			u = u * s;
		}
		const V3 v1 = vs + u;
		planes[3 * stride + i] = v1.x; planes[4 * stride + i] = v1.y; planes[5 * stride + i] = v1.z;
	}
	planes[i] = p1.x; planes[stride + i] = p1.y; planes[2 * stride + i] = p1.z;
	contacts[i] = best.col;
}

// The pass's tables from the host's settings: written again when a setting or the particle layout changed.
static bool uploadCollideTables(World& w)
{
	World::Cloth& cl = w.cloth;
	std::vector<ClothCollideDesc> descs; std::vector<uint2> blocks;
	u32 first = 0, flags = 0;
	for (const World::HCloth& c : cl.cloths)
	{
		const u32 n = c.gridX * c.gridY;
		if (c.collide)
		{
			for (u32 k = 0; k < n; k += 64u) blocks.push_back(make_uint2((u32)descs.size(), k));
			descs.push_back(ClothCollideDesc{ first, n, c.collision.flags, c.collision.excludeFirst, c.collision.excludeCount, c.collision.thickness, c.collision.friction, 0u });
			flags |= c.collision.flags;
		}
		first += n;
	}
	cl.collideBlocks = (u32)blocks.size(); cl.collideFlags = flags;
	if (cl.contactsStride != cl.stride) // a new particle layout: nothing has been pushed off anything yet
	{
		cl.contacts.ensure(std::max<size_t>(cl.stride, 1), w.stream);
		if (w.lastError) return false;
		MI_CHECK(hipMemsetAsync(cl.contacts.p, 0xFF, sizeof(u32) * std::max<size_t>(cl.stride, 1), w.stream));
		cl.contactsStride = cl.stride;
	}
	cl.collideDescs.ensure(sizeof(ClothCollideDesc) * std::max<size_t>(descs.size(), 1), w.stream); cl.collideBlockList.ensure(std::max<size_t>(blocks.size(), 1), w.stream);
	if (w.lastError) return false;
	if (!descs.empty())
	{
		MI_CHECK(hipMemcpyAsync(cl.collideDescs.p, descs.data(), sizeof(ClothCollideDesc) * descs.size(), hipMemcpyHostToDevice, w.stream));
		MI_CHECK(hipMemcpyAsync(cl.collideBlockList.p, blocks.data(), sizeof(uint2) * blocks.size(), hipMemcpyHostToDevice, w.stream));
		MI_CHECK(hipStreamSynchronize(w.stream)); // (the host vectors go out of scope; only after a setting or the layout changed)
	}
	cl.collideDirty = false;
	return true;
}

void launch_cloth_collide(World& w)
{
	World::Cloth& cl = w.cloth;
	if (!cl.numColliding || !cl.stateOnDevice) return; // (not on the device: the state was read back since the step, which settled the step first)
	if (cl.collideDirty && !uploadCollideTables(w)) return;
	if (!cl.collideBlocks) return;
	const bool brute = cl.collideBrute;
	const u32 chunks = w.terrain.chunksPerDim * w.terrain.chunksPerDim;
	const bool terrain = (cl.collideFlags & MI_CLOTH_COLLIDE_TERRAIN) != 0u && chunks != 0u;
	if (terrain && chunks > 131071u) { w.fail(MI_ERR_INVALID_ARGUMENT, "cloth collision: a heightmap of more than 131071 chunks cannot be met (mi_proximity's limit)"); return; }
	if (!w.queries.interactTablesValid) w.buildInteractTables(); // the hull triangles of rcScene
	if (w.lastError) return;
	const RcBuild built = launch_raycast_build(w, (cl.collideFlags & MI_CLOTH_COLLIDE_STATIC) != 0u, brute);
	if (built == RC_BUILD_FAILED) return;
	if (built == RC_BUILD_NO_CANDIDATES && !terrain) { MI_CHECK(hipMemsetAsync(cl.contacts.p, 0xFF, sizeof(u32) * std::max<size_t>(cl.stride, 1), w.stream)); return; } // nothing to be pushed off
	if (terrain && !brute && !launch_terrain_tables(w)) return;
	const TerrainParams P = terrainParams(w);
	const auto kernel = brute ? (terrain ? k_cloth_collide<true, true> : k_cloth_collide<true, false>) : (terrain ? k_cloth_collide<false, true> : k_cloth_collide<false, false>);
	hipLaunchKernelGGL(kernel, dim3(cl.collideBlocks), dim3(64), 0, w.stream, (const ClothCollideDesc*)cl.collideDescs.p, cl.collideBlockList.p, cl.planes.p, (size_t)cl.stride, cl.contacts.p,
		built == RC_BUILD_DONE ? 1u : 0u, rcScene(w), w.vel.p, w.bprops.p, w.dCounters.p + CTR_FLOW_STATUS, P, w.terrain.heights.p, w.terrain.valid.p,
		terrain && !brute ? w.queries.terrainTiles.p : (const u32*)nullptr, terrain && !brute ? w.queries.terrainChunkRange.p : (const u32*)nullptr);
}
