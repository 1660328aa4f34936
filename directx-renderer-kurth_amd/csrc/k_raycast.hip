// mi_raycast_batch: many rays, each against every candidate collider of the world, closest hit with its point (DESIGN.md,
// "Whole-world ray casts").  A structure of its own, rebuilt at every call from the current poses and kept in buffers nothing else
// uses (World::queries): the step's AABBs, world colliders, sorted boxes, cell tables and counters belong to a step that may still be in
// flight and are neither read nor written here.
//   k_rc_leaves   candidate flag + padded world AABB per collider; count, bounds of the box centres, largest box diagonal
//   k_rc_keys     30-bit Morton key of every candidate's box centre (non-candidates: bit 30, so they sort behind the candidates)
//   (radix sort)  prim_sort_pairs_u32, 31 bits
//   k_rc_tree     internal nodes after Karras (2012), equal keys separated by their sorted position
//   k_rc_fit      node boxes bottom-up: the second child to arrive at a node merges and goes on
//   k_raycast     one lane per ray: rcWalk (raycast_shared.h: near child first, fixed stack in LDS) with RcRayVisitor, the slab test and
//                 the leaf test of a ray; with MI_RAY_BRUTE_FORCE the same leaf test on all colliders; <.., EXCLUDE = true>
//                 (mi_raycast_sensors, k_raycast_sensors.hip) skips the colliders of the ray's own body range
// A hit is decided by rayBodyCollider (ray_tests.h) on the collider's LOCAL record and pose alone (rcFetch), as in k_interaction_batch;
// the boxes only say which colliders need not be asked.  The kernel reads the world through one RcScene argument (raycast_shared.h).
#include "world.h"
#include "ray_tests.h"
#include "raycast_shared.h"

void prim_sort_pairs_u32(World& w, const u32* kin, u32* kout, const u32* vin, u32* vout, u32 n, u32 bits);


// Leaf pad, per axis: RC_PAD_ULPS ulps of (largest |coordinate| of the box + its diagonal) + RC_PAD_FLOOR.  DESIGN.md derives them.
// (The slack of the slab test, RC_SLACK_ULPS and RC_SLACK_REL: raycast_shared.h.)
#define RC_PAD_ULPS 8.f
#define RC_PAD_FLOOR 1e-5f

MI_DEV u32 rcOrdered(float f) { u32 u = mi_f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); } // order-preserving, never 0 for a finite f
MI_DEV float rcUnordered(u32 u) { return mi_u2f((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
MI_DEV void rcGrow(V3& mn, V3& mx, V3 p) { mn = vmin(mn, p); mx = vmax(mx, p); }
MI_DEV void rcCorners(V3 lo, V3 hi, Q4 rot, V3 tr, V3& mn, V3& mx)
{
	mn = v3s(MI_FLT_MAX); mx = v3s(-MI_FLT_MAX);
	for (u32 k = 0; k < 8; ++k) rcGrow(mn, mx, rot * v3((k & 1) ? hi.x : lo.x, (k & 2) ? hi.y : lo.y, (k & 4) ? hi.z : lo.z) + tr);
}
// World AABB of a local collider at (rot, pos), unpadded.  A cylinder gets its capsule's box.
MI_DEV void rcWorldBox(const ColliderRec& c, Q4 rot, V3 pos, const float4* __restrict__ hullInfo, V3& mn, V3& mx)
{
	switch (colType(c))
	{
		case MI_SPHERE: { V3 ce = rot * v3(c.a.x, c.a.y, c.a.z) + pos; mn = ce - v3s(c.a.w); mx = ce + v3s(c.a.w); } break;
		case MI_CAPSULE: case MI_CYLINDER:
		{
			V3 a = rot * v3(c.a.x, c.a.y, c.a.z) + pos, b = rot * v3(c.a.w, c.b.x, c.b.y) + pos;
			mn = vmin(a, b) - v3s(c.b.z); mx = vmax(a, b) + v3s(c.b.z);
		} break;
		case MI_AABB: rcCorners(v3(c.a.x, c.a.y, c.a.z), v3(c.a.w, c.b.x, c.b.y), rot, pos, mn, mx); break;
		case MI_OBB: { V3 ra = v3(c.b.w, c.c.x, c.c.y); rcCorners(-ra, ra, rot * q4f4(c.a), rot * v3(c.b.x, c.b.y, c.b.z) + pos, mn, mx); } break;
		case MI_HULL:
		{
			const u32 g = (u32)c.b.w;
			rcCorners(v3f4(hullInfo[2 * g]), v3f4(hullInfo[2 * g + 1]), rot * q4f4(c.a), rot * v3(c.b.x, c.b.y, c.b.z) + pos, mn, mx);
		} break;
		default: mn = pos; mx = pos; break;
	}
}

// Collider c: is it a candidate, and if so its padded box; acc = what the header accumulates (negMin xyz, max xyz, diagonal, |coordinate|).
MI_DEV bool rcLeaf(u32 c, u32 nb, u32 withStatic, const ColliderRec* __restrict__ cols, const float4* __restrict__ pose, const float4* __restrict__ colStaticPose,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, const float4* __restrict__ hullInfo, float4* __restrict__ leafBox, u32* acc)
{
	const ColliderRec rec = cols[c];
	const u32 body = colBody(rec), zone = mi_f2u(rec.d.w) & 0xFFu;
	const bool candidate = zone == 0u && (body < nb ? (alive[body] && simMask[body]) : withStatic != 0u);
	V3 mn = v3s(0.f), mx = v3s(0.f);
	if (candidate)
	{
		const float4* P = (body < nb) ? (pose + 2 * body) : (colStaticPose + 2 * c);
		rcWorldBox(rec, q4f4(P[1]), v3f4(P[0]), hullInfo, mn, mx);
		const float diag = length(mx - mn);
		const V3 pad = (vmax(vabs(mn), vabs(mx)) + v3s(diag)) * (RC_PAD_ULPS * RC_EPS) + v3s(RC_PAD_FLOOR);
		mn = mn - pad; mx = mx + pad;
		const V3 ce = (mn + mx) * 0.5f, am = vmax(vabs(mn), vabs(mx));
		const u32 v[8] = { rcOrdered(-ce.x), rcOrdered(-ce.y), rcOrdered(-ce.z), rcOrdered(ce.x), rcOrdered(ce.y), rcOrdered(ce.z),
			mi_f2u(length(mx - mn)), mi_f2u(fmaxf(fmaxf(am.x, am.y), am.z)) }; // (non-negative floats order like their bits)
		for (int k = 0; k < 8; ++k) acc[k] = acc[k] > v[k] ? acc[k] : v[k];
	}
	leafBox[2 * c] = make_float4(mn.x, mn.y, mn.z, candidate ? 1.f : 0.f);
	leafBox[2 * c + 1] = make_float4(mx.x, mx.y, mx.z, 0.f);
	return candidate;
}
__global__ void __launch_bounds__(256) k_rc_leaves(u32 nc, u32 nb, u32 withStatic, const ColliderRec* __restrict__ cols, const float4* __restrict__ pose, const float4* __restrict__ colStaticPose,
	const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask, const float4* __restrict__ hullInfo, float4* __restrict__ leafBox, u32* __restrict__ hdr)
{
	u32 count = 0, acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (u32 c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x)
		count += rcLeaf(c, nb, withStatic, cols, pose, colStaticPose, alive, simMask, hullInfo, leafBox, acc) ? 1u : 0u;
	// one atomic per word and workgroup (same-address atomics serialise)
	__shared__ u32 sAcc[4][9];
	for (int o = 32; o > 0; o >>= 1) { count += __shfl_xor(count, o); for (int k = 0; k < 8; ++k) acc[k] = max(acc[k], (u32)__shfl_xor(acc[k], o)); }
	if ((threadIdx.x & 63) == 0) { for (int k = 0; k < 8; ++k) sAcc[threadIdx.x >> 6][k] = acc[k]; sAcc[threadIdx.x >> 6][8] = count; }
	__syncthreads();
	if (threadIdx.x < 8) { const u32 m = max(max(sAcc[0][threadIdx.x], sAcc[1][threadIdx.x]), max(sAcc[2][threadIdx.x], sAcc[3][threadIdx.x])); if (m) atomicMax(&hdr[RC_NEG_MIN + threadIdx.x], m); }
	if (threadIdx.x == 8) { const u32 s = sAcc[0][8] + sAcc[1][8] + sAcc[2][8] + sAcc[3][8]; if (s) atomicAdd(&hdr[RC_N], s); }
}

MI_DEV u32 rcSpread(u32 v) { v = (v * 0x00010001u) & 0xFF0000FFu; v = (v * 0x00000101u) & 0x0F00F00Fu; v = (v * 0x00000011u) & 0xC30C30C3u; v = (v * 0x00000005u) & 0x49249249u; return v; }
// (an extent of 0 on an axis — centres coplanar, collinear or all the same — gives cell 0 on it: nothing is divided)
MI_DEV u32 rcCell(float v, float lo, float hi) { const float e = hi - lo; return e > 0.f ? min(1023u, (u32)fmaxf((v - lo) * (1024.f / e), 0.f)) : 0u; }

MI_DEV u32 rcKey(u32 c, const float4* __restrict__ leafBox, const u32* __restrict__ hdr)
{
	const float4 mn = leafBox[2 * c], mx = leafBox[2 * c + 1];
	if (mn.w == 0.f) return RC_NOT_A_CANDIDATE;
	const V3 lo = v3(-rcUnordered(hdr[RC_NEG_MIN]), -rcUnordered(hdr[RC_NEG_MIN + 1]), -rcUnordered(hdr[RC_NEG_MIN + 2]));
	const V3 hi = v3(rcUnordered(hdr[RC_MAX]), rcUnordered(hdr[RC_MAX + 1]), rcUnordered(hdr[RC_MAX + 2]));
	return (rcSpread(rcCell((mn.x + mx.x) * 0.5f, lo.x, hi.x)) << 2) | (rcSpread(rcCell((mn.y + mx.y) * 0.5f, lo.y, hi.y)) << 1) | rcSpread(rcCell((mn.z + mx.z) * 0.5f, lo.z, hi.z));
}
__global__ void __launch_bounds__(256) k_rc_keys(u32 nc, const float4* __restrict__ leafBox, const u32* __restrict__ hdr, u32* __restrict__ keys, u32* __restrict__ vals)
{
	const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= nc) return;
	keys[c] = rcKey(c, leafBox, hdr); vals[c] = c;
}

// One internal node: 64 bytes = the boxes of its two children {min xyz, max xyz} x 2 (written by k_rc_fit), their ids (a leaf: RC_LEAF |
// collider index) and two unused words.  Node 0 is the root.
// (RC_NODE_WORDS = 16: raycast_shared.h)
// Common prefix of the sorted keys i and j (Karras 2012, section 4): -1 outside the list; equal keys go on with their positions.
MI_DEV int rcDelta(const u32* __restrict__ keys, int n, int i, int j)
{
	if (j < 0 || j >= n) return -1;
	const u32 a = keys[i], b = keys[j];
	return a != b ? __builtin_clz(a ^ b) : 32 + __builtin_clz((u32)i ^ (u32)j);
}
MI_DEV void rcTreeNode(int i, int n, const u32* __restrict__ keys, const u32* __restrict__ vals, u32* __restrict__ nodes, u32* __restrict__ parentInt, u32* __restrict__ parentLeaf)
{
	const int d = rcDelta(keys, n, i, i + 1) > rcDelta(keys, n, i, i - 1) ? 1 : -1;
	const int dMin = rcDelta(keys, n, i, i - d);
	int lMax = 2;
	while (rcDelta(keys, n, i, i + lMax * d) > dMin) lMax <<= 1;
	int l = 0;
	for (int t = lMax >> 1; t > 0; t >>= 1) if (rcDelta(keys, n, i, i + (l + t) * d) > dMin) l += t;
	const int j = i + l * d, dNode = rcDelta(keys, n, i, j);
	int s = 0;
	for (int t = (l + 1) >> 1; ; t = (t + 1) >> 1) { if (rcDelta(keys, n, i, i + (s + t) * d) > dNode) s += t; if (t <= 1) break; }
	const int split = i + s * d + min(d, 0), first = min(i, j), last = max(i, j);
	const bool leafL = first == split, leafR = last == split + 1;
	nodes[RC_NODE_WORDS * (u32)i + 12] = leafL ? (RC_LEAF | vals[split]) : (u32)split;
	nodes[RC_NODE_WORDS * (u32)i + 13] = leafR ? (RC_LEAF | vals[split + 1]) : (u32)(split + 1);
	(leafL ? parentLeaf : parentInt)[split] = (u32)i << 1;
	(leafR ? parentLeaf : parentInt)[split + 1] = ((u32)i << 1) | 1u;
	if (i == 0) parentInt[0] = RC_NO_PARENT;
}
__global__ void __launch_bounds__(256) k_rc_tree(const u32* __restrict__ hdr, const u32* __restrict__ keys, const u32* __restrict__ vals, u32* __restrict__ nodes, u32* __restrict__ parentInt, u32* __restrict__ parentLeaf)
{
	const int n = (int)hdr[RC_N], i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n - 1) rcTreeNode(i, n, keys, vals, nodes, parentInt, parentLeaf); // (n < 2: no internal node)
}

// One lane per leaf climbs towards the root.  At every node it writes the box it carries into its slot of the node's record; the first
// child to arrive stops there, the second reads its sibling's box, merges and climbs on.  The box is published by a fence before the
// arrival counter's atomic and picked up behind a fence after it.  The root's own box is the scene's: nobody needs it.
MI_DEV void rcFitLeaf(u32 j, const u32* __restrict__ vals, const float4* __restrict__ leafBox, const u32* __restrict__ parentInt, const u32* __restrict__ parentLeaf, float* nodes, u32* arrivals)
{
	const u32 c = vals[j];
	V3 mn = v3f4(leafBox[2 * c]), mx = v3f4(leafBox[2 * c + 1]);
	u32 up = parentLeaf[j];
	for (u32 level = 0; level < RC_STACK && up != RC_NO_PARENT; ++level)
	{
		const u32 p = up >> 1, side = up & 1u;
		float* mine = nodes + RC_NODE_WORDS * p + 6u * side;
		mine[0] = mn.x; mine[1] = mn.y; mine[2] = mn.z; mine[3] = mx.x; mine[4] = mx.y; mine[5] = mx.z;
#if defined(__HIP_DEVICE_COMPILE__)
		__threadfence();
		if (atomicAdd(&arrivals[p], 1u) == 0u) return;
		__threadfence();
#else
		if (arrivals[p]++ == 0u) return; // (host build of this function: one leaf after the other)
#endif
		const float* other = nodes + RC_NODE_WORDS * p + 6u * (side ^ 1u);
		mn = vmin(mn, v3(other[0], other[1], other[2])); mx = vmax(mx, v3(other[3], other[4], other[5]));
		up = parentInt[p];
	}
}
__global__ void __launch_bounds__(256) k_rc_fit(const u32* __restrict__ hdr, const u32* __restrict__ vals, const float4* __restrict__ leafBox, const u32* __restrict__ parentInt, const u32* __restrict__ parentLeaf,
	float* nodes, u32* arrivals)
{
	const u32 n = hdr[RC_N], j = blockIdx.x * blockDim.x + threadIdx.x;
	if (n >= 2u && j < n) rcFitLeaf(j, vals, leafBox, parentInt, parentLeaf, nodes, arrivals);
}

// (RcRay, rcBoxTest, rcPrepareRay and the slack of the slab test: raycast_shared.h, shared with k_spherecast.hip)
struct RcBest { float t; u32 col, body; V3 point; }; // t starts at MI_FLT_MAX like the reference's minDistance: a test that reports FLT_MAX or +inf (a box whose slab interval is poisoned, rule R2a) has not hit
// rcWalk's visitor of a ray: a box is held against the closest hit so far, a leaf may become it.  ex: mi_raycast_sensors' exclusion range.
struct RcRayVisitor
{
	const RcRay& q; RcExclude ex; const RcScene& sc; RcBest& best;
	MI_DEV bool box(const float* b, float& tEnter) const { return rcBoxTest(q, b, fminf(q.maxT, best.t), tEnter); }
	MI_DEV void leaf(u32 c)
	{
		RcCollider col; HRay lr; float t;
		if (!rcFetch(sc, c, ex, col)) return;
		if (rayBodyCollider(q.r, col.rot, col.pos, col.type, col.s, sc.hulls, lr, t) && t >= 0.f && t <= q.maxT && (t < best.t || (best.col != 0xFFFFFFFFu && t == best.t && c < best.col)))
		{
			best.t = t; best.col = c; best.body = col.reported;
			best.point = col.rot * (lr.origin + t * lr.direction) + col.pos; // interactionPush's globalHit
		}
	}
};

// exclude: NULL, or one {first, count} body range per ray (EXCLUDE: it is read).
template <bool BRUTE, bool EXCLUDE>
__global__ void __launch_bounds__(64) k_raycast(u32 numRays, const float4* __restrict__ rays, float4* __restrict__ out, RcScene sc, const uint2* __restrict__ exclude)
{
	__shared__ u32 stack[BRUTE ? 1 : RC_STACK][64]; // [level][lane]: a wave's access is one row, conflict-free
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numRays) return;
	const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
	RcBest best; best.t = MI_FLT_MAX; best.col = 0xFFFFFFFFu; best.body = 0u; best.point = v3s(0.f);
	RcRay q; q.r = HRay{ v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z) }; q.maxT = r0.w;
	RcExclude ex{ 0u, 0u };
	if (EXCLUDE) { const uint2 e = exclude[i]; ex.first = e.x; ex.count = e.y; }
	RcRayVisitor v{ q, ex, sc, best };
	const u32 n = sc.hdr[RC_N];
	if (r1.w != 0.f && n != 0u)
	{
		if (BRUTE)
		{
			for (u32 c = 0; c < sc.nc; ++c) if (sc.leafBox[2 * c].w != 0.f) v.leaf(c);
		}
		else
		{
			rcPrepareRay(q, mi_u2f(sc.hdr[RC_ABS]), mi_u2f(sc.hdr[RC_DIAG]));
			rcWalk(v, sc, n, &stack[0][threadIdx.x], 64u);
		}
	}
	const bool hit = best.col != 0xFFFFFFFFu;
	out[2 * i] = hit ? make_float4(best.t, mi_u2f(best.col), mi_u2f(best.body), mi_u2f(1u)) : make_float4(0.f, 0.f, 0.f, 0.f);
	out[2 * i + 1] = hit ? make_float4(best.point.x, best.point.y, best.point.z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The tree over the current candidates in World::queries, enqueued on the world's stream: what mi_raycast_batch and mi_proximity both walk.
// brute: only the leaves (candidate flags, padded boxes, header words), which is all a brute-force walk reads.
RcBuild launch_raycast_build(World& w, bool withStatic, bool brute)
{
	// what the host knows of the candidates (a slab's simulate mask can only take some away): none = nothing is built
	u32 hostCandidates = 0;
	for (const World::HCollider& c : w.colliders) if (c.zoneType == 0u && (c.body == MI_STATIC_BODY ? withStatic : !w.bodies[c.body].removed)) hostCandidates++;
	if (!hostCandidates || !w.nc) return RC_BUILD_NO_CANDIDATES;
	const u32 nc = w.nc;
	w.queries.leafBox.ensure(2 * (size_t)nc, w.stream); w.queries.count.ensure(RC_HEADER + (size_t)nc, w.stream);
	w.queries.keys.ensure(nc, w.stream); w.queries.keysSorted.ensure(nc, w.stream); w.queries.vals.ensure(nc, w.stream); w.queries.valsSorted.ensure(nc, w.stream);
	w.queries.nodes.ensure(4 * (size_t)nc, w.stream); w.queries.parentInt.ensure(nc, w.stream); w.queries.parentLeaf.ensure(nc, w.stream);
	if (w.lastError) return RC_BUILD_FAILED;
	const u32 blocks = (nc + 255u) / 256u;
	MI_CHECK(hipMemsetAsync(w.queries.count.p, 0, sizeof(u32) * (brute ? (size_t)RC_HEADER : RC_HEADER + (size_t)nc), w.stream));
	hipLaunchKernelGGL(k_rc_leaves, dim3(std::min(blocks, 256u)), dim3(256), 0, w.stream, nc, w.nb, withStatic ? 1u : 0u, w.colLocal.p, w.pose.p, w.colStaticPose.p,
		w.aliveMask.p, w.simMask.p, w.hullInfo.p, w.queries.leafBox.p, w.queries.count.p);
	if (brute) return RC_BUILD_DONE;
	hipLaunchKernelGGL(k_rc_keys, dim3(blocks), dim3(256), 0, w.stream, nc, w.queries.leafBox.p, w.queries.count.p, w.queries.keys.p, w.queries.vals.p);
	prim_sort_pairs_u32(w, w.queries.keys.p, w.queries.keysSorted.p, w.queries.vals.p, w.queries.valsSorted.p, nc, RC_KEY_BITS + 1);
	if (hostCandidates > 1u)
	{
		const u32 treeBlocks = (hostCandidates + 255u) / 256u; // (the device's count is at most the host's)
		hipLaunchKernelGGL(k_rc_tree, dim3(treeBlocks), dim3(256), 0, w.stream, w.queries.count.p, w.queries.keysSorted.p, w.queries.valsSorted.p, (u32*)w.queries.nodes.p, w.queries.parentInt.p, w.queries.parentLeaf.p);
		hipLaunchKernelGGL(k_rc_fit, dim3(treeBlocks), dim3(256), 0, w.stream, w.queries.count.p, w.queries.valsSorted.p, w.queries.leafBox.p, w.queries.parentInt.p, w.queries.parentLeaf.p, (float*)w.queries.nodes.p, w.queries.count.p + RC_HEADER);
	}
	return RC_BUILD_DONE;
}

// dExclude: NULL, or one {first, count} body range per ray (mi_raycast_sensors): the colliders of those bodies are no candidates of that ray.
void launch_raycast(World& w, u32 numRays, const float* dRays, u32 flags, mi_ray_hit* dOutHits, const uint2* dExclude)
{
	const bool brute = (flags & MI_RAY_BRUTE_FORCE) != 0;
	const RcBuild built = launch_raycast_build(w, (flags & MI_RAY_STATIC) != 0, brute);
	if (built == RC_BUILD_NO_CANDIDATES) { MI_CHECK(hipMemsetAsync(dOutHits, 0, sizeof(mi_ray_hit) * (size_t)numRays, w.stream)); return; } // every ray misses
	if (built == RC_BUILD_FAILED) return;
	const auto kernel = brute ? (dExclude ? k_raycast<true, true> : k_raycast<true, false>) : (dExclude ? k_raycast<false, true> : k_raycast<false, false>);
	hipLaunchKernelGGL(kernel, dim3((numRays + 63) / 64), dim3(64), 0, w.stream, numRays, (const float4*)dRays, (float4*)dOutHits, rcScene(w), dExclude);
}
