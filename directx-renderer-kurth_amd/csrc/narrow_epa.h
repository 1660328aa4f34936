// GJK + EPA, the per-pair device functions: the parallel branch of cylinder vs cylinder, the wave-cooperative EPA, what follows EPA for a
// tube on a box, and the simplex record a GJK hit hands to EPA.  What the step's kernels (k_narrow_gjk.hip) and the contact query's
// (k_contact_query.hip) run: one text.
#pragma once
#include "narrow_gjk.h"
#include "narrow_clip.h"
#include <cstddef>

// cylinder vs cylinder, parallel branch (:821-903).  Returns 0 = no collision, 1 = manifold written, 2 = not parallel (GJK + EPA).
MI_DEV int cylinderCylinderParallel(Capsule a, Capsule b, Man& m)
{
	V3 aDir = a.b - a.a;
	V3 bDir = normalize(b.b - b.a);
	float aDirLength = length(aDir);
	aDir *= 1.f / aDirLength;
	float parallel = dot(aDir, bDir);
	if (!(fabsf(parallel) > 0.99f)) return 2;
	V3 pBa = b.a, pBb = b.b;
	if (parallel < 0.f) { V3 t = pBa; pBa = pBb; pBb = t; }
	V3 ref = a.a;
	float a0 = 0.f, a1 = aDirLength;
	float b0 = dot(aDir, pBa - ref), b1 = dot(aDir, pBb - ref);
	float left = fmaxf(a0, b0), right = fminf(a1, b1);
	if (right < left) return 0;
	V3 contactA0 = ref + left * aDir, contactA1 = ref + right * aDir;
	V3 contactB0 = closestPointSegment(contactA0, pBa, pBb);
	V3 contactB1 = contactB0 + (right - left) * aDir;
	V3 normal = contactB0 - contactA0;
	float d = length(normal);
	float penetration = (a.r + b.r) - d;
	if (penetration < 0.f) return 0;
	float capPenetration = right - left;
	if (capPenetration < penetration)
	{
		m.count = 1;
		V3 pt;
		if (b0 > a0) { m.n = aDir; pt = a.b - v3s(capPenetration * 0.5f); }   // vec3 - float broadcast, as :891/:897 do
		else { m.n = -aDir; pt = a.a + v3s(capPenetration * 0.5f); }
		m.p[0] = make_float4(pt.x, pt.y, pt.z, capPenetration);
	}
	else
	{
		if (d < MI_EPSILON) { d = 0.f; normal = v3(0.f, 1.f, 0.f); } else { normal = normal / d; }
		m.n = normal; m.count = 2;
		V3 p0 = (contactA0 + contactB0) * 0.5f, p1 = (contactA1 + contactB1) * 0.5f;
		m.p[0] = make_float4(p0.x, p0.y, p0.z, penetration);
		m.p[1] = make_float4(p1.x, p1.y, p1.z, penetration);
	}
	return 1;
}

// ---------------------------------------------------------------------------------------------------------------
// EPA — collision_epa.h:96-168; collision_epa.cpp:5-239.  Array sizes: the reference's 1024-entry arrays can
// hold at most 24 points after its 20 iterations; triangles/edges are sized above the measured high-water marks (98 / 100 over
// all test scenes, same caps in oracle/onarrow.h), and the reference's out-of-memory exits are kept.
// ---------------------------------------------------------------------------------------------------------------
#define EPA_MAX_POINTS 24
#define EPA_MAX_TRIANGLES 128
#define EPA_MAX_EDGES 160
#define EPA_MAX_BORDER 32

MI_DEV V3 barycentric(V3 a, V3 b, V3 c, V3 p) // math.cpp:1390-1408
{
	V3 v0 = b - a, v1 = c - a, v2 = p - a;
	float d00 = dot(v0, v0), d01 = dot(v0, v1), d11 = dot(v1, v1), d20 = dot(v2, v0), d21 = dot(v2, v1);
	float denom = d00 * d11 - d01 * d01;
	denom = (fabsf(denom) < MI_EPSILON) ? 1.f : denom;
	float v = (d11 * d20 - d01 * d21) / denom;
	float w = (d00 * d21 - d01 * d20) / denom;
	float u = 1.0f - v - w;
	return v3(u, v, w);
}

// ---------------------------------------------------------------------------------------------------------------
// Wave-cooperative EPA (collision_epa.h:96-168, collision_epa.cpp:5-239): ONE WAVE expands ONE polytope.  The polytope
// (points, triangles, edges) lives in LDS (7.6 KB per wave); the per-iteration scans the serial algorithm does over all
// triangles / edges are strided over the 64 lanes, the closest-triangle search is a shuffle min-reduction on (distance, index)
// — the same "first strictly smaller" winner as the serial scan — and border edges are compacted in index order with
// ballot + popcount, so indices, tie-breaks and therefore results are those of the serial reference algorithm.
// Support points are recomputed redundantly by every lane (wave-uniform values, no LDS traffic).
// ---------------------------------------------------------------------------------------------------------------
struct alignas(16) EpaWave
{
	float pa[EPA_MAX_POINTS][3], pb[EPA_MAX_POINTS][3];          // support points on A and B; minkowski = a - b (bit-identical to the stored one)
	float tnx[EPA_MAX_TRIANGLES], tny[EPA_MAX_TRIANGLES], tnz[EPA_MAX_TRIANGLES], tdist[EPA_MAX_TRIANGLES];
	// (indices are below 65535 = EPA_NONE32: 16 bits each keep a wave's polytope at 6.3 KB instead of 9.6, i.e. more resident workgroups)
	uint16_t ta[EPA_MAX_TRIANGLES], tb[EPA_MAX_TRIANGLES], tc[EPA_MAX_TRIANGLES], teA[EPA_MAX_TRIANGLES], teB[EPA_MAX_TRIANGLES], teC[EPA_MAX_TRIANGLES];
	uint8_t tactive[EPA_MAX_TRIANGLES];
	uint16_t ea[EPA_MAX_EDGES], eb[EPA_MAX_EDGES], etA[EPA_MAX_EDGES], etB[EPA_MAX_EDGES];
	u32 refs[EPA_MAX_EDGES];
	u32 border[EPA_MAX_BORDER], newEdgePerPoint[EPA_MAX_POINTS];
};
static_assert(offsetof(EpaWave, tnx) % 16 == 0 && sizeof(EpaWave) % 16 == 0 && 4 * sizeof(float) * EPA_MAX_TRIANGLES >= 2 * 16 * sizeof(float4), "the triangle arrays double as two 16-point clipping polygons (capsuleBoxFinish)");
#define EPA_NONE32 0xFFFFu
#define EPA_GROUP 32u                 // lanes per polytope (>= EPA_MAX_BORDER and EPA_MAX_POINTS: one lane per border edge / point)
#define EPA_GROUP_MASK 0xFFFFFFFFu
#define WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier()

__device__ __forceinline__ V3 epaMk(const EpaWave& e, u32 i) { return v3(e.pa[i][0], e.pa[i][1], e.pa[i][2]) - v3(e.pb[i][0], e.pb[i][1], e.pb[i][2]); }
__device__ __forceinline__ void epaSetPoint(EpaWave& e, u32 i, const SupportPoint& p)
{
	e.pa[i][0] = p.a.x; e.pa[i][1] = p.a.y; e.pa[i][2] = p.a.z; e.pb[i][0] = p.b.x; e.pb[i][1] = p.b.y; e.pb[i][2] = p.b.z;
}
__device__ __forceinline__ void epaSetTri(EpaWave& e, u32 t, u32 a, u32 b, u32 c, u32 eA, u32 eB, u32 eC, V3 mka, V3 mkb, V3 mkc)
{
	V3 n = normalize(cross(mkb - mka, mkc - mka)); // getTriangleInfo (collision_epa.cpp:5-11)
	e.tnx[t] = n.x; e.tny[t] = n.y; e.tnz[t] = n.z; e.tdist[t] = dot(n, mka);
	e.ta[t] = a; e.tb[t] = b; e.tc[t] = c; e.teA[t] = eA; e.teB[t] = eB; e.teC[t] = eC; e.tactive[t] = 1;
}

// Runs on a GROUP of EPA_GROUP lanes (two polytopes per wave: the scalar part of an iteration — support point, termination test, the
// bookkeeping — is issued once for both, and the kernel is bound by instruction issue); every lane of a group returns the same
// (point, normal, depth).  `lane` is the lane inside the group.  Counts and indices are uniform inside a group, not across the wave:
// the two groups' loops and exits diverge freely, every cross-lane operation (shuffles below EPA_GROUP, ballots cut to the group's
// bits) stays inside a group, and WAVE_SYNC orders a group's LDS traffic whatever the other group is doing.
template <int FAMILY>
__device__ void epaWave(EpaWave& e, u32 lane, u32 groupShift, const GjkSimplex& g, const SupShapes& sh, V3& outPoint, V3& outNormal, float& outDepth, u32* __restrict__ counters)
{
	u32 numTris = 4, numPoints = 4, numEdges = 6;
	u32 maxBorder = 0; bool outOfMemory = false; // for the high-water marks (CTR_NARROW_LIMITS), as the oracle records them
	if (lane == 0)
	{
		epaSetPoint(e, 0, g.a); epaSetPoint(e, 1, g.b); epaSetPoint(e, 2, g.c); epaSetPoint(e, 3, g.d);
		epaSetTri(e, 0, 0, 1, 3, 4, 3, 0, g.a.mk, g.b.mk, g.d.mk);
		epaSetTri(e, 1, 1, 2, 3, 5, 4, 1, g.b.mk, g.c.mk, g.d.mk);
		epaSetTri(e, 2, 2, 0, 3, 3, 5, 2, g.c.mk, g.a.mk, g.d.mk);
		epaSetTri(e, 3, 0, 2, 1, 1, 0, 2, g.a.mk, g.c.mk, g.b.mk);
		const u32 E[6][4] = { { 0, 1, 0, 3 }, { 1, 2, 1, 3 }, { 2, 0, 2, 3 }, { 0, 3, 2, 0 }, { 1, 3, 0, 1 }, { 2, 3, 1, 2 } };
		for (u32 i = 0; i < 6; ++i) { e.ea[i] = E[i][0]; e.eb[i] = E[i][1]; e.etA[i] = E[i][2]; e.etB[i] = E[i][3]; }
	}
	WAVE_SYNC();

	u32 closest = 0;
	for (u32 it = 0; it < 20; ++it)
	{
		// findTriangleClosestToOrigin (collision_epa.cpp:89-109): lowest index among the minimal distances
		float bd = MI_FLT_MAX; u32 bi = 0xFFFFFFFFu;
		for (u32 t = lane; t < numTris; t += EPA_GROUP) { if (e.tactive[t]) { float d = e.tdist[t]; if (d < bd) { bd = d; bi = t; } } }
		for (int o = EPA_GROUP / 2; o > 0; o >>= 1)
		{
			float od = __shfl_xor(bd, o); u32 oi = __shfl_xor(bi, o);
			if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
		}
		closest = bi;
		if (closest == 0xFFFFFFFFu) { closest = 0; break; }
		V3 tn = v3(e.tnx[closest], e.tny[closest], e.tnz[closest]);
		SupportPoint np = supportPair<FAMILY>(sh, tn);
		float dd = dot(np.mk, tn);
		if (dd - e.tdist[closest] < 0.01f) break;

		// addNewPointAndUpdate (collision_epa.cpp:111-239)
		for (u32 i = lane; i < numEdges; i += EPA_GROUP) e.refs[i] = 0;
		if (lane < EPA_MAX_POINTS) e.newEdgePerPoint[lane] = 0;
		WAVE_SYNC();
		for (u32 t = lane; t < numTris; t += EPA_GROUP)
		{
			if (e.tactive[t])
			{
				float d = dot(v3(e.tnx[t], e.tny[t], e.tnz[t]), np.mk - epaMk(e, e.ta[t]));
				if (d > 0.f) { atomicAdd(&e.refs[e.teA[t]], 1u); atomicAdd(&e.refs[e.teB[t]], 1u); atomicAdd(&e.refs[e.teC[t]], 1u); e.tactive[t] = 0; }
			}
		}
		WAVE_SYNC();
		u32 nBorder = 0;
		for (u32 base = 0; base < numEdges; base += EPA_GROUP) // border edges in edge-index order
		{
			u32 i = base + lane;
			bool flag = i < numEdges && e.refs[i] == 1;
			u32 mask = (u32)(__ballot(flag) >> groupShift) & EPA_GROUP_MASK; // (the other group's lanes, if they are in this loop at all, vote in their own bits)
			u32 pos = nBorder + __popc(mask & ((1u << lane) - 1u));
			if (flag && pos < EPA_MAX_BORDER) e.border[pos] = i;
			nBorder += __popc(mask);
		}
		if (nBorder > EPA_MAX_BORDER) { outOfMemory = true; break; }             // "out of memory" exits, as the serial code's pushes would hit them
		maxBorder = max(maxBorder, nBorder);
		if (numPoints >= EPA_MAX_POINTS) { outOfMemory = true; break; }
		if (numEdges + nBorder > EPA_MAX_EDGES || numTris + nBorder > EPA_MAX_TRIANGLES) { outOfMemory = true; break; }
		u32 newPoint = numPoints++;
		if (lane == 0) epaSetPoint(e, newPoint, np);
		WAVE_SYNC();
		u32 triOffset = numTris;
		if (lane < nBorder)
		{
			u32 ei = e.border[lane];
			u32 ea = e.ea[ei], eb = e.eb[ei], tA = e.etA[ei], tB = e.etB[ei];
			bool triAActive = e.tactive[tA] != 0, triBActive = e.tactive[tB] != 0;
			u32 ptc = triBActive ? ea : eb;
			u32 triIndex = numTris + lane, newEdge = numEdges + lane;
			e.ea[newEdge] = ptc; e.eb[newEdge] = newPoint; e.etA[newEdge] = EPA_NONE32; e.etB[newEdge] = triIndex;
			atomicMax(&e.newEdgePerPoint[ptc], newEdge);                      // serial code: last writer (= highest index) wins
			u32 bI = ptc, cI = triBActive ? eb : ea;
			epaSetTri(e, triIndex, newPoint, bI, cI, ei, EPA_NONE32, newEdge, np.mk, epaMk(e, bI), epaMk(e, cI));
			if (triAActive) e.etB[ei] = triIndex; else e.etA[ei] = triIndex;
		}
		numEdges += nBorder; numTris += nBorder;
		WAVE_SYNC();
		if (lane < nBorder) // fix up the indices left open above
		{
			u32 ei = e.border[lane];
			bool triBNew = e.etB[ei] >= triOffset;
			u32 ptc = triBNew ? e.ea[ei] : e.eb[ei];
			u32 other = e.newEdgePerPoint[ptc];
			u32 triIndex = lane + triOffset;
			e.teB[triIndex] = other;
			e.etA[other] = triIndex;
		}
		WAVE_SYNC();
	}
	V3 tn = v3(e.tnx[closest], e.tny[closest], e.tnz[closest]);
	float tdist = e.tdist[closest];
	u32 ia = e.ta[closest], ib = e.tb[closest], ic = e.tc[closest];
	V3 bary = barycentric(epaMk(e, ia), epaMk(e, ib), epaMk(e, ic), tn * tdist);
	V3 pointA = bary.x * v3(e.pa[ia][0], e.pa[ia][1], e.pa[ia][2]) + bary.y * v3(e.pa[ib][0], e.pa[ib][1], e.pa[ib][2]) + bary.z * v3(e.pa[ic][0], e.pa[ic][1], e.pa[ic][2]);
	V3 pointB = bary.x * v3(e.pb[ia][0], e.pb[ia][1], e.pb[ia][2]) + bary.y * v3(e.pb[ib][0], e.pb[ib][1], e.pb[ib][2]) + bary.z * v3(e.pb[ic][0], e.pb[ic][1], e.pb[ic][2]);
	outPoint = 0.5f * (pointA + pointB);
	outNormal = tn;
	outDepth = tdist;
	if (lane == 0) // one update per polytope: the counts only grow, so their final values are this polytope's maxima
	{
		// (read first: the marks settle within a step or two, after which no polytope issues the same-address atomics — unguarded,
		// they cost c3 0.86 ms per step)
		if (numTris > counters[CTR_NARROW_LIMITS + 1]) atomicMax(&counters[CTR_NARROW_LIMITS + 1], numTris);
		if (numEdges > counters[CTR_NARROW_LIMITS + 2]) atomicMax(&counters[CTR_NARROW_LIMITS + 2], numEdges);
		if (maxBorder > counters[CTR_NARROW_LIMITS + 3]) atomicMax(&counters[CTR_NARROW_LIMITS + 3], maxBorder);
		if (outOfMemory) atomicAdd(&counters[CTR_NARROW_LIMITS + 4], 1u);
	}
	WAVE_SYNC(); // the next instance reuses this LDS block
}

// Everything of intersection(capsule, aabb) after EPA — collision_narrow.cpp:723-768
MI_DEV void capsuleBoxFinish(V3 point, V3 normal, float depth, const Capsule& c, const Box& a, Man& m, const PolyStore& store)
{
	m.n = normal; m.count = 1;
	m.p[0] = make_float4(point.x, point.y, point.z, depth);
	if (fabsf(normal.x) > 0.99f || fabsf(normal.y) > 0.99f || fabsf(normal.z) > 0.99f)
	{
		V3 axis = normalize(c.b - c.a);
		if (fabsf(dot(normal, axis)) < 0.01f)
		{
			V3 cpp[4], cpn[4];
			float4 clipPlanes[4];
			V3 aabbNormal = -normal;
			V3 refPoint = v3((aabbNormal.x < 0.f) ? a.lo.x : a.hi.x, (aabbNormal.y < 0.f) ? a.lo.y : a.hi.y, (aabbNormal.z < 0.f) ? a.lo.z : a.hi.z); // getAABBReferencePlane :291-299
			float4 referencePlane = createPlane(refPoint, aabbNormal);
			Poly polygon; polygon.pts = store.a; polygon.stride = store.stride; polygon.n = 2;
			Poly clipped; clipped.pts = store.b; clipped.stride = store.stride;
			V3 pa = c.a + normal * c.r, pb = c.b + normal * c.r;
			PP(polygon, 0) = make_float4(pa.x, pa.y, pa.z, -signedDistanceToPlane(pa, referencePlane));
			PP(polygon, 1) = make_float4(pb.x, pb.y, pb.z, -signedDistanceToPlane(pb, referencePlane));
			V3 aCenter = boxCenter(a);
			getAABBClippingPlanes(boxRadius(a), aabbNormal, cpp, cpn);
			for (u32 i = 0; i < 4; ++i) clipPlanes[i] = createPlane(cpp[i] + aCenter, cpn[i]);
			clipPointsAndBuildContact(polygon, clipped, clipPlanes, referencePlane, m);
		}
	}
}

// The record a GJK hit hands to EPA: its simplex, 4 support points x 9 floats packed as 9 float4 at gjkSimplex + 9 * (position in the
// work list) (written out: an array of pointers to the four points goes through scratch memory).
__device__ __forceinline__ void storeSimplex(float4* S, const GjkSimplex& sx)
{
	const SupportPoint &p0 = sx.a, &p1 = sx.b, &p2 = sx.c, &p3 = sx.d;
	S[0] = make_float4(p0.a.x, p0.a.y, p0.a.z, p0.b.x); S[1] = make_float4(p0.b.y, p0.b.z, p0.mk.x, p0.mk.y); S[2] = make_float4(p0.mk.z, p1.a.x, p1.a.y, p1.a.z);
	S[3] = make_float4(p1.b.x, p1.b.y, p1.b.z, p1.mk.x); S[4] = make_float4(p1.mk.y, p1.mk.z, p2.a.x, p2.a.y); S[5] = make_float4(p2.a.z, p2.b.x, p2.b.y, p2.b.z);
	S[6] = make_float4(p2.mk.x, p2.mk.y, p2.mk.z, p3.a.x); S[7] = make_float4(p3.a.y, p3.a.z, p3.b.x, p3.b.y); S[8] = make_float4(p3.b.z, p3.mk.x, p3.mk.y, p3.mk.z);
}
__device__ __forceinline__ void loadSimplex(const float4* S, GjkSimplex& sx)
{
	const float4 s0 = S[0], s1 = S[1], s2 = S[2], s3 = S[3], s4 = S[4], s5 = S[5], s6 = S[6], s7 = S[7], s8 = S[8];
	sx.a.a = v3(s0.x, s0.y, s0.z); sx.a.b = v3(s0.w, s1.x, s1.y); sx.a.mk = v3(s1.z, s1.w, s2.x);
	sx.b.a = v3(s2.y, s2.z, s2.w); sx.b.b = v3(s3.x, s3.y, s3.z); sx.b.mk = v3(s3.w, s4.x, s4.y);
	sx.c.a = v3(s4.z, s4.w, s5.x); sx.c.b = v3(s5.y, s5.z, s5.w); sx.c.mk = v3(s6.x, s6.y, s6.z);
	sx.d.a = v3(s6.w, s7.x, s7.y); sx.d.b = v3(s7.z, s7.w, s8.x); sx.d.mk = v3(s8.y, s8.z, s8.w);
	sx.numPoints = 4;
}

// The shape of an EPA workgroup: EPA_GROUP lanes per hit, polytopes in LDS.
#define EPA_WAVES_PER_BLOCK 4
#define EPA_PER_WAVE (64 / EPA_GROUP)
