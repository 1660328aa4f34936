// Narrowphase, the pairs that need no GJK: closed forms (reference collision_narrow.cpp:374-612, :1074-1140) and box-box SAT +
// Sutherland-Hodgman clipping (:1179-1527).  One thread per candidate pair.  narrow.h has the overview and the pair keys.
// (the per-pair functions themselves: narrow_pairs.h, shared with k_contact_query.hip)
#include "narrow_pairs.h"

// ---------------------------------------------------------------------------------------------------------------
// K6/K7: pair kernels + contact emit (writeManifold)
// ---------------------------------------------------------------------------------------------------------------
enum { GROUP_CLOSED = 0, GROUP_BOX = 1 };

// GROUP_CLOSED scans all valid slots and skips foreign buckets (its buckets are scattered over the key space);
// GROUP_BOX covers the contiguous slot range [KEY_BOX_BEGIN, KEY_BOX_END) (aabb-obb, obb-obb; aabb-hull is skipped: GJK + EPA).
template <int GROUP>
__global__ void __launch_bounds__(GROUP == GROUP_CLOSED ? 256 : 64) k_narrow(const u32* __restrict__ counters, const u32* __restrict__ keySorted, const u64* __restrict__ pairSorted,
	const ColliderRec* __restrict__ colWorld, ManifoldRec* __restrict__ manifolds)
{
	// the box kernel's clipping polygons: two per lane, 16 points each, point i of lane l at [i * 64 + l] (conflict-free 16-byte accesses)
	__shared__ float4 sPoly[GROUP == GROUP_BOX ? 2 * 16 * 64 : 1];
	const PolyStore store = { sPoly + (GROUP == GROUP_BOX ? threadIdx.x : 0u), sPoly + (GROUP == GROUP_BOX ? 16u * 64u + threadIdx.x : 0u), 64u };
	u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (GROUP == GROUP_BOX) { slot += counters[CTR_BUCKET_START + KEY_BOX_BEGIN]; if (slot >= counters[CTR_BUCKET_START + KEY_BOX_END]) return; }
	if (slot >= counters[CTR_NUM_VALID]) return;
	u32 key = keySorted[slot];
	if (!(GROUP == GROUP_CLOSED ? closedFormKey(key) : boxKey(key))) return;
	u64 packed = pairSorted[slot];
	u32 ia = (u32)packed, ib = (u32)(packed >> 32);
	ColliderRec A = colWorld[ia], B = colWorld[ib];
	Man m = emptyManifold();
	bool hit = false;
	if (GROUP == GROUP_CLOSED)
	{
		switch (key)
		{
			case KEY_SPHERE_SPHERE: hit = sphereSphere(asSphere(A), asSphere(B), m); break;
			case KEY_SPHERE_CAPSULE: hit = sphereCapsule(asSphere(A), asCapsule(B), m); break;
			case KEY_SPHERE_CYLINDER: hit = sphereCylinder(asSphere(A), asCapsule(B), m); break;
			case KEY_SPHERE_AABB: hit = sphereBox(asSphere(A), asBox(B), m); break;
			case KEY_SPHERE_OBB: hit = sphereObb(asSphere(A), asObb(B), m); break;
			case KEY_CAPSULE_CAPSULE: hit = capsuleCapsule(asCapsule(A), asCapsule(B), m); break;
			case KEY_CAPSULE_CYLINDER: hit = capsuleCylinder(asCapsule(A), asCapsule(B), m); break;
			case KEY_AABB_AABB: hit = boxBoxAxisAligned(asBox(A), asBox(B), m); break;
		}
	}
	else
	{
		Obb oa;
		if (key == KEY_AABB_OBB) { Box b = asBox(A); oa.q = q4(0.f, 0.f, 0.f, 1.f); oa.c = boxCenter(b); oa.r = boxRadius(b); } // aabb -> obb (:1142-1148)
		else oa = asObb(A);
		hit = obbObb(oa, asObb(B), m, store);
	}
	writeManifold(manifolds, slot, m, hit, A, B, slot);
}

void launch_pair_kernels(World& w, u32 numPairs, hipStream_t stream)
{
	const u64* sortedPairs = (const u64*)w.pairsSorted.p;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_narrow<GROUP_CLOSED>), dim3((numPairs + 255) / 256), dim3(256), 0, stream, w.dCounters.p, w.pairKeySorted.p, sortedPairs, w.colWorld.p, w.manifolds.p);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_narrow<GROUP_BOX>), dim3((numPairs + 63) / 64), dim3(64), 0, stream, w.dCounters.p, w.pairKeySorted.p, sortedPairs, w.colWorld.p, w.manifolds.p);
}
