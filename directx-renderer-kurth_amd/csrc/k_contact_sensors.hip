// mi_contact_sensors: what the contacts of the last step did to a body, reduced on the device from the rows the sweep left behind
// ("Contact sensors"; the rule is stated in include/mi_physics.h).  The step's buffers are only read.  A reading adds its
// terms in ascending manifold slot, then contact index, whatever order the sweep ran in, so the work is a grouping of the schedule
// positions by body and an ordered walk:
//   k_cs_mark        one lane per sensor: its body is wanted (World::queries.csBody[b].x)
//   k_cs_count       one pass over the schedule positions: manifolds per wanted body, on either side (integer atomics: a count has no order)
//   k_cs_alloc       one lane per body: its segment of World::queries.csEntries, taken from one cursor (where a segment lies is of no
//                    consequence: every segment is sorted on its own); bodies with more than CS_SMALL manifolds go on a list
//   k_cs_fill        the second pass: (slot << 32 | position) into the segments, in whatever order the lanes arrive
//   k_cs_sort_small  one lane per body: insertion sort of a segment of 2 .. CS_SMALL keys (a body in a pile has 4 to 8)
//   k_cs_sort_large  one workgroup per listed body: bitonic network, in LDS up to CS_LDS_KEYS keys (a hub), in place beyond
//   k_cs_read        CS_GROUP lanes per sensor: each lane fetches one manifold of the segment (ids, filter, normal, the planes, the
//                    impulses) and forms its terms; the group then adds the terms of its CS_GROUP manifolds one after the other, every
//                    lane the same sum: the far-memory round trips run side by side, the additions in the one order the rule fixes
// O(bodies + manifolds + sensors); nothing is sensors x manifolds.  No floating-point atomics anywhere.
#include "world.h"

#define CS_SMALL 32u
#define CS_LDS_KEYS 4096u
#define CS_GROUP 8u

// csBody[b] = {wanted, manifolds, first entry, fill cursor}; meta = {entries handed out, bodies on the list}
MI_DEV u32 csPositions(const u32* __restrict__ counters, u32 bound) { const u32 n = counters[CTR_NUM_MANIFOLDS]; return n < bound ? n : bound; }

__global__ void __launch_bounds__(256) k_cs_mark(u32 numSensors, const uint4* __restrict__ sensors, u32 nb, uint4* __restrict__ csBody)
{
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numSensors) return;
	const u32 b = sensors[i].x;
	if (b < nb) csBody[b].x = 1u;
}

__global__ void __launch_bounds__(256) k_cs_count(const u32* __restrict__ counters, u32 bound, const uint4* __restrict__ rowIds, u32 nb, uint4* __restrict__ csBody)
{
	const u32 n = csPositions(counters, bound);
	for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x)
	{
		const uint4 ids = rowIds[s];
		if (ids.x < nb && csBody[ids.x].x) atomicAdd(&csBody[ids.x].y, 1u);
		if (ids.y < nb && csBody[ids.y].x) atomicAdd(&csBody[ids.y].y, 1u);
	}
}

__global__ void __launch_bounds__(256) k_cs_alloc(u32 nb, uint4* __restrict__ csBody, u32* __restrict__ meta, u32* __restrict__ large)
{
	const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= nb) return;
	const u32 c = csBody[b].y;
	if (!c) return;
	csBody[b].z = atomicAdd(&meta[0], c);
	if (c > CS_SMALL) large[atomicAdd(&meta[1], 1u)] = b;
}

__global__ void __launch_bounds__(256) k_cs_fill(const u32* __restrict__ counters, u32 bound, const uint4* __restrict__ rowIds, u32 nb, uint4* __restrict__ csBody, u64* __restrict__ entries, u32 entryCap)
{
	const u32 n = csPositions(counters, bound);
	for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x)
	{
		const uint4 ids = rowIds[s];
		const u64 key = ((u64)ids.w << 32) | s;
		if (ids.x < nb && csBody[ids.x].x) { const u32 p = csBody[ids.x].z + atomicAdd(&csBody[ids.x].w, 1u); if (p < entryCap) entries[p] = key; }
		if (ids.y < nb && csBody[ids.y].x) { const u32 p = csBody[ids.y].z + atomicAdd(&csBody[ids.y].w, 1u); if (p < entryCap) entries[p] = key; }
	}
}

__global__ void __launch_bounds__(256) k_cs_sort_small(u32 nb, const uint4* __restrict__ csBody, u64* __restrict__ entries)
{
	const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= nb) return;
	const uint4 bs = csBody[b];
	if (bs.y < 2u || bs.y > CS_SMALL) return;
	u64* e = entries + bs.z;
	for (u32 i = 1; i < bs.y; ++i)
	{
		const u64 key = e[i];
		u32 j = i;
		for (; j > 0u && e[j - 1u] > key; --j) e[j] = e[j - 1u];
		e[j] = key;
	}
}

// Bitonic network with every comparison ascending (the first step of a merge compares mirrored partners, the rest are half cleaners):
// keys past the end count as +infinity and never move, so any length sorts in place without padding.  One workgroup, keys in LDS or HBM.
MI_DEV void csCompareSwap(u64* keys, u32 a, u32 b, u32 len)
{
	if (b >= len) return;
	const u64 x = keys[a], y = keys[b];
	if (x > y) { keys[a] = y; keys[b] = x; }
}
__device__ void csBitonic(u64* keys, u32 len)
{
	u32 padded = 1u;
	while (padded < len) padded <<= 1;
	const u32 half = padded / 2u;
	for (u32 k = 2u; k <= padded; k <<= 1)
	{
		for (u32 i = threadIdx.x; i < half; i += blockDim.x) { const u32 h = k / 2u, block = i / h, off = i % h; csCompareSwap(keys, block * k + off, block * k + k - 1u - off, len); }
		__syncthreads();
		for (u32 j = k / 4u; j > 0u; j >>= 1)
		{
			for (u32 i = threadIdx.x; i < half; i += blockDim.x) { const u32 a = (i / j) * 2u * j + i % j; csCompareSwap(keys, a, a + j, len); }
			__syncthreads();
		}
	}
}

__global__ void __launch_bounds__(256) k_cs_sort_large(const u32* __restrict__ meta, const u32* __restrict__ large, const uint4* __restrict__ csBody, u64* __restrict__ entries)
{
	__shared__ u64 keys[CS_LDS_KEYS];
	const u32 numLarge = meta[1];
	for (u32 li = blockIdx.x; li < numLarge; li += gridDim.x)
	{
		const uint4 bs = csBody[large[li]];
		u64* e = entries + bs.z;
		if (bs.y <= CS_LDS_KEYS)
		{
			for (u32 i = threadIdx.x; i < bs.y; i += blockDim.x) keys[i] = e[i];
			__syncthreads();
			csBitonic(keys, bs.y);
			for (u32 i = threadIdx.x; i < bs.y; i += blockDim.x) e[i] = keys[i];
			__syncthreads(); // (the next body's load must not overtake this store's reads of the LDS)
		}
		else csBitonic(e, bs.y);
	}
}

// sensors: mi_contact_sensor {body, partners, excludeFirst, excludeCount}; out: 3 x float4 per sensor = mi_contact_reading
// {impulse.xyz, normalImpulse}, {angularImpulse.xyz, numContacts}, {numManifolds, strongestPartner, valid, 0} (the integers as bits).
__global__ void __launch_bounds__(256) k_cs_read(u32 numSensors, const uint4* __restrict__ sensors, u32 nb, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ simMask,
	const uint4* __restrict__ csBody, const u64* __restrict__ entries, size_t rowCap, const uint4* __restrict__ rowIds, const float4* __restrict__ rowShared,
	const float4* __restrict__ rowPlanes, const float2* __restrict__ rowLambda, float4* __restrict__ out)
{
	const u32 gid = blockIdx.x * blockDim.x + threadIdx.x, i = gid / CS_GROUP, lane = gid % CS_GROUP;
	if (i >= numSensors) return; // (a whole group leaves together: the shuffles below stay inside a group)
	const uint4 sn = sensors[i];
	const u32 body = sn.x;
	const bool valid = body < nb && alive[body] && simMask[body];
	V3 lin = v3s(0.f), ang = v3s(0.f);
	float normal = 0.f, best = 0.f;
	u32 numContacts = 0u, numManifolds = 0u, strongest = 0u;
	if (valid)
	{
		const uint4 bs = csBody[body];
		for (u32 base = 0u; base < bs.y; base += CS_GROUP)
		{
			// this lane's manifold of the batch: its terms, formed as fl(fl(ln * n) + fl(lt * t)) per component, negated for side A
			u32 count = 0u, partner = 0u;
			V3 tl[MI_MAX_CONTACTS_PER_MANIFOLD], ta[MI_MAX_CONTACTS_PER_MANIFOLD]; float ln[MI_MAX_CONTACTS_PER_MANIFOLD];
#pragma unroll
			for (u32 k = 0; k < MI_MAX_CONTACTS_PER_MANIFOLD; ++k) { tl[k] = v3s(0.f); ta[k] = v3s(0.f); ln[k] = 0.f; }
			if (base + lane < bs.y)
			{
				const u32 s = (u32)entries[bs.z + base + lane];
				const uint4 ids = s < rowCap ? rowIds[s] : make_uint4(nb, nb, 0u, 0u);
				const bool isB = ids.y == body;
				partner = isB ? ids.x : ids.y;
				const bool pass = partner == nb ? (sn.y & MI_CONTACT_STATIC) != 0u : ((sn.y & MI_CONTACT_DYNAMIC) != 0u && !(partner - sn.z < sn.w));
				if (pass)
				{
					count = ids.z < MI_MAX_CONTACTS_PER_MANIFOLD ? ids.z : MI_MAX_CONTACTS_PER_MANIFOLD;
					const V3 n = v3f4(rowShared[s]);
#pragma unroll
					for (u32 k = 0; k < MI_MAX_CONTACTS_PER_MANIFOLD; ++k)
					{
						if (k >= count) break;
						const float4* P = rowPlanes + (size_t)(k * MI_ROW_PLANES) * rowCap + s;
						const float4 p0 = P[0], p1 = P[rowCap], p2 = P[2 * rowCap], p3 = P[3 * rowCap];
						const float2 lam = rowLambda[(size_t)k * rowCap + s];
						const V3 t = v3(p0.x, p0.y, p0.z);
						const V3 ct = isB ? v3(p1.z, p1.w, p2.x) : v3(p0.w, p1.x, p1.y), cn = isB ? v3(p3.x, p3.y, p3.z) : v3(p2.y, p2.z, p2.w);
						const V3 l = lam.x * n + lam.y * t, a = lam.x * cn + lam.y * ct;
						tl[k] = isB ? l : -l; ta[k] = isB ? a : -a; ln[k] = lam.x;
					}
				}
			}
			// the batch in order: every lane of the group adds the same terms
			const u32 batch = bs.y - base < CS_GROUP ? bs.y - base : CS_GROUP;
			for (u32 j = 0u; j < batch; ++j)
			{
				const u32 cnt = __shfl(count, j, CS_GROUP), prt = __shfl(partner, j, CS_GROUP);
				float sum = 0.f;
#pragma unroll
				for (u32 k = 0; k < MI_MAX_CONTACTS_PER_MANIFOLD; ++k)
				{
					const float lx = __shfl(tl[k].x, j, CS_GROUP), ly = __shfl(tl[k].y, j, CS_GROUP), lz = __shfl(tl[k].z, j, CS_GROUP);
					const float ax = __shfl(ta[k].x, j, CS_GROUP), ay = __shfl(ta[k].y, j, CS_GROUP), az = __shfl(ta[k].z, j, CS_GROUP);
					const float nk = __shfl(ln[k], j, CS_GROUP);
					if (k < cnt)
					{
						lin = lin + v3(lx, ly, lz); ang = ang + v3(ax, ay, az);
						normal = normal + nk; sum = sum + nk;
					}
				}
				if (cnt)
				{
					if (!numManifolds || sum > best) { best = sum; strongest = prt == nb ? MI_STATIC_BODY : prt; } // ascending slots: a tie keeps the lower one
					numManifolds++; numContacts += cnt;
				}
			}
		}
	}
	if (lane) return;
	out[3 * (size_t)i] = make_float4(lin.x, lin.y, lin.z, normal);
	out[3 * (size_t)i + 1] = make_float4(ang.x, ang.y, ang.z, mi_u2f(numContacts));
	out[3 * (size_t)i + 2] = make_float4(mi_u2f(numManifolds), mi_u2f(strongest), mi_u2f(valid ? 1u : 0u), 0.f);
}

// withRows: the last step had rows at all (otherwise the device's manifold count is the step's before: every reading is empty)
void launch_contact_sensors(World& w, u32 numSensors, const mi_contact_sensor* dSensors, mi_contact_reading* dOut, bool withRows)
{
	const u32 nb = w.last.bodies; // the bodies of that step: its rows name the static dummy by this index
	const size_t bound = withRows ? std::min<size_t>(w.last.numPairs, w.rowCap) : 0;
	const size_t entryCap = std::max<size_t>(2 * bound, 1);
	w.queries.csBody.ensure((size_t)nb + 1, w.stream); w.queries.csLarge.ensure((size_t)nb + 1, w.stream); w.queries.csMeta.ensure(4, w.stream); w.queries.csEntries.ensure(entryCap, w.stream);
	if (w.lastError) return;
	const uint4* sensors = (const uint4*)dSensors;
	MI_CHECK(hipMemsetAsync(w.queries.csBody.p, 0, sizeof(uint4) * ((size_t)nb + 1), w.stream));
	if (bound)
	{
		MI_CHECK(hipMemsetAsync(w.queries.csMeta.p, 0, sizeof(u32) * 4, w.stream));
		const u32 rowGrid = (u32)std::min<size_t>((bound + 255) / 256, 4096), bodyGrid = (nb + 255) / 256;
		hipLaunchKernelGGL(k_cs_mark, dim3((numSensors + 255) / 256), dim3(256), 0, w.stream, numSensors, sensors, nb, w.queries.csBody.p);
		hipLaunchKernelGGL(k_cs_count, dim3(rowGrid), dim3(256), 0, w.stream, w.dCounters.p, (u32)bound, w.rowIds.p, nb, w.queries.csBody.p);
		hipLaunchKernelGGL(k_cs_alloc, dim3(bodyGrid), dim3(256), 0, w.stream, nb, w.queries.csBody.p, w.queries.csMeta.p, w.queries.csLarge.p);
		hipLaunchKernelGGL(k_cs_fill, dim3(rowGrid), dim3(256), 0, w.stream, w.dCounters.p, (u32)bound, w.rowIds.p, nb, w.queries.csBody.p, w.queries.csEntries.p, (u32)std::min<size_t>(entryCap, 0xFFFFFFFFu));
		hipLaunchKernelGGL(k_cs_sort_small, dim3(bodyGrid), dim3(256), 0, w.stream, nb, w.queries.csBody.p, w.queries.csEntries.p);
		hipLaunchKernelGGL(k_cs_sort_large, dim3(std::min(bodyGrid, 256u)), dim3(256), 0, w.stream, w.queries.csMeta.p, w.queries.csLarge.p, w.queries.csBody.p, w.queries.csEntries.p);
	}
	const u32 groupsPerBlock = 256u / CS_GROUP;
	hipLaunchKernelGGL(k_cs_read, dim3((numSensors + groupsPerBlock - 1) / groupsPerBlock), dim3(256), 0, w.stream, numSensors, sensors, nb, w.aliveMask.p, w.simMask.p,
		w.queries.csBody.p, w.queries.csEntries.p, w.rowCap, w.rowIds.p, w.rowShared.p, w.rowPlanes.p, w.rowLambda.p, (float4*)dOut);
}
