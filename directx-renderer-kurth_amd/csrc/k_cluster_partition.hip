// Cluster sweep, first stage: the partition.  Orders the bodies along the phases' Morton curves, cuts each curve into tasks by
// weight, deals every manifold (and joint) to the task it is interior to, sends what the curves leave over to the component phase,
// and lays the tasks' manifolds out for k_cluster_color.hip.  cluster.h explains why clusters exist and how the phases work.
#include "cluster.h"

void prim_sort_pairs_u32(World& w, const u32* kin, u32* kout, const u32* vin, u32* vout, u32 n, u32 bits);
void prim_exclusive_scan_u32(World& w, const u32* in, u32* out, u32 n);

MI_DEV u32 clOrderedBits(float f) { u32 b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
MI_DEV float clOrderedFloat(u32 o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
MI_DEV u32 clSpread10(u32 x) { x &= 0x3FFu; x = (x | (x << 16)) & 0x030000FFu; x = (x | (x << 8)) & 0x0300F00Fu; x = (x | (x << 4)) & 0x030C30C3u; x = (x | (x << 2)) & 0x09249249u; return x; }

// ---------------------------------------------------------------------------------------------------------------
// Body order: bounding box of the centres of gravity, Morton keys per phase, radix sort, ranks.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cl_bbox(u32 nb, const float4* __restrict__ cog, const uint8_t* __restrict__ simMask, u32* __restrict__ counters)
{
	float mn[3] = { MI_FLT_MAX, MI_FLT_MAX, MI_FLT_MAX }, mx[3] = { -MI_FLT_MAX, -MI_FLT_MAX, -MI_FLT_MAX };
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += gridDim.x * blockDim.x)
	{
		if (!simMask[i]) continue;
		float4 c = cog[i];
		if (!(c.x == c.x && c.y == c.y && c.z == c.z)) continue;
		mn[0] = fminf(mn[0], c.x); mn[1] = fminf(mn[1], c.y); mn[2] = fminf(mn[2], c.z);
		mx[0] = fmaxf(mx[0], c.x); mx[1] = fmaxf(mx[1], c.y); mx[2] = fmaxf(mx[2], c.z);
	}
	for (int k = 0; k < 3; ++k)
		for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
	__shared__ float sMn[4][3], sMx[4][3]; // one atomic pair per workgroup and axis: same-address atomics from all over the chip serialise
	if ((threadIdx.x & 63u) == 0u) for (int k = 0; k < 3; ++k) { sMn[threadIdx.x >> 6][k] = mn[k]; sMx[threadIdx.x >> 6][k] = mx[k]; }
	__syncthreads();
	if (threadIdx.x < 3u)
	{
		u32 k = threadIdx.x;
		float a = fminf(fminf(sMn[0][k], sMn[1][k]), fminf(sMn[2][k], sMn[3][k])), b = fmaxf(fmaxf(sMx[0][k], sMx[1][k]), fmaxf(sMx[2][k], sMx[3][k]));
		if (a <= b) { atomicMin(&counters[CTR_CL_BBOX + k], clOrderedBits(a)); atomicMax(&counters[CTR_CL_BBOX + 3 + k], clOrderedBits(b)); }
	}
}

struct ClShifts { u32 s[CL_MAX_PARTS][3]; };

__global__ void __launch_bounds__(256) k_cl_keys(u32 nb, u32 numParts, ClShifts shifts, u32 maxShift, const float4* __restrict__ cog, const uint8_t* __restrict__ simMask,
	const u32* __restrict__ counters, u32* __restrict__ keys, u32* __restrict__ vals)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nb) return;
	float lo[3], ext = 0.f;
	for (int k = 0; k < 3; ++k)
	{
		lo[k] = clOrderedFloat(counters[CTR_CL_BBOX + k]);
		float hi = clOrderedFloat(counters[CTR_CL_BBOX + 3 + k]);
		ext = fmaxf(ext, hi - lo[k]);
	}
	float scale = (ext > 0.f) ? (float)(1023u - maxShift) / ext : 0.f; // one cell size for the three axes
	float4 c = cog[i];
	bool sim = simMask[i] != 0 && c.x == c.x && c.y == c.y && c.z == c.z;
	int q[3] = { (int)((c.x - lo[0]) * scale), (int)((c.y - lo[1]) * scale), (int)((c.z - lo[2]) * scale) };
	for (int k = 0; k < 3; ++k) q[k] = q[k] < 0 ? 0 : (q[k] > (int)(1023u - maxShift) ? (int)(1023u - maxShift) : q[k]);
	for (u32 p = 0; p < numParts; ++p)
	{
		u32 key = clSpread10((u32)q[0] + shifts.s[p][0]) | (clSpread10((u32)q[1] + shifts.s[p][1]) << 1) | (clSpread10((u32)q[2] + shifts.s[p][2]) << 2);
		// bodies simulated elsewhere sort last; no manifold refers to them.  Bits 30-31: the curve, so that ONE sort orders all curves (clRefreshBodyOrder)
		keys[(size_t)p * nb + i] = (sim ? key : 0x3FFFFFFFu) | (p << 30);
		vals[(size_t)p * nb + i] = i;
	}
}

__global__ void __launch_bounds__(256) k_cl_ranks(u32 nb, u32 numParts, const u32* __restrict__ sortedBodies, u32* __restrict__ rank)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nb) return;
	for (u32 p = 0; p < numParts; ++p) rank[(size_t)p * (nb + 1) + sortedBodies[(size_t)p * nb + i]] = i;
	if (i == 0) for (u32 p = 0; p < numParts; ++p) rank[(size_t)p * (nb + 1) + nb] = 0xFFFFFFFFu; // the static dummy owns nothing
}

// ---------------------------------------------------------------------------------------------------------------
// Assignment.  wsum[r] = weight of the not-yet-assigned manifolds OWNED by the body of rank r (owner = the dynamic body of the
// manifold that comes first on this phase's curve); cum = exclusive scan; task of a body = cum / taskWeight; a manifold whose
// dynamic bodies agree on the task is interior to it.  Whatever a task holds is owned by its bodies, so a task's weight is below
// taskWeight + one body's weight.
// ---------------------------------------------------------------------------------------------------------------
// A phase may not have more tasks than the solve launch has workgroups (task t of a phase runs on workgroup (offset + t) % G, all
// of them resident): when the pile outgrows "G tasks of the configured weight", the chunks grow instead.  cum[nb] = total weight.
// And a world of jointed islands that would leave most workgroups without a first-phase task — 256 ragdolls — is spread over the
// launch in smaller tasks (fewer joints and colours per task; islands are never cut, so smaller tasks cost no extra hand-overs;
// config 4: 28 -> 165 tasks, 0.583 ms at 1000, 0.544 at 400, 0.516 at 150, 0.522 at 100), down to CL_WEIGHT_SPREAD_MIN.  Only the first
// phase (its weight argument carries CL_WEIGHT_ISLANDS).  Contact-only worlds keep their chunks: smaller ones cut more manifolds
// (config 2, 10 k spheres: no gain at 300, a fourth phase at 150).
#define CL_WEIGHT_ISLANDS 0x80000000u
#define CL_WEIGHT_REG_LIMIT (64u * 1250u)  // chunk weight up to which a task's INTERIOR contacts (70 - 85 % of what its bodies own) fit k_cl_solve's register sets, give or take what LDS holds
#define CL_WEIGHT_SPREAD_MIN (64u * 150u)
MI_DEV u32 clEffectiveWeight(u32 taskWeightArg, u32 totalWeight, u32 maxTasks)
{
	const u32 taskWeight = taskWeightArg & ~CL_WEIGHT_ISLANDS;
	u32 need = totalWeight / maxTasks + 1u;                                   // one task per workgroup ...
	if (need <= taskWeight)
	{
		if ((taskWeightArg & CL_WEIGHT_ISLANDS) && 2u * need <= taskWeight)
		{
			const u32 spread = need + need / 2u;
			return spread > CL_WEIGHT_SPREAD_MIN ? spread : min(CL_WEIGHT_SPREAD_MIN, taskWeight);
		}
		return taskWeight;
	}
	if (need <= CL_WEIGHT_REG_LIMIT) return need;                             // ... as long as such a task still fits the lanes' registers,
	u32 need2 = totalWeight / (CL_TASKS_PER_PHASE * maxTasks) + 1u;             // then up to CL_TASKS_PER_PHASE per workgroup (the later ones run from LDS)
	return need2 > CL_WEIGHT_REG_LIMIT ? need2 : CL_WEIGHT_REG_LIMIT;
}
#define CL_UNASSIGNED 0xFFFFFFFFu
#define CL_WEIGHT_MANIFOLD 64u            // weight of a manifold on the curve ...
#define CL_WEIGHT_EXTRA 64u               // ... plus this per contact beyond the first (the sweep's unit is the contact)
#define CL_REST_CAP 1024u                 // once no more than this many manifolds are unassigned, they all go to the rest task (it must fit k_cl_color's tables)
#define CL_REMAIN_SUBS 64u // the 'still unassigned after phase p' count is kept in 64 partial counters: ~2000 workgroups adding to ONE word queue up behind each other
// The cursors the assignment accumulates into (World::cluster.taskCount): CL_SUBCOUNTERS per task key, then CL_REMAIN_SUBS per word of CTR_CL_REMAIN.
constexpr u32 CL_TASK_CURSORS = CL_MAX_PHASES * CL_MAX_TASKS * CL_SUBCOUNTERS;
constexpr u32 CL_REMAIN_WORDS = ctrWords(CTR_CL_REMAIN);
constexpr u32 CL_REMAIN_CURSORS = CL_REMAIN_WORDS * CL_REMAIN_SUBS;
static_assert(CL_REMAIN_WORDS == CL_MAX_PHASES + 1u, "one 'still unassigned' count per phase and one behind the last");
// The counter ranges k_cl_clear zeroes besides, as CTR_LAYOUT has them.
constexpr u32 CL_LEFT_WORDS = ctrWords(CTR_CL_LEFT);
constexpr u32 CL_STATS_WORDS = ctrWords(CTR_CL_STATUS) + ctrWords(CTR_CL_SHARED) + ctrWords(CTR_CL_PHASE_COUNT); // status, shared bodies, manifolds per phase
static_assert(CTR_CL_SHARED == CTR_CL_STATUS + ctrWords(CTR_CL_STATUS) && CTR_CL_PHASE_COUNT == CTR_CL_SHARED + ctrWords(CTR_CL_SHARED), "cleared as one range from CTR_CL_STATUS on");

// The three appenders (k_cl_assign, k_cl_assign_cached, k_cl_comp_assign) pick one of a task's CL_SUBCOUNTERS cursors for manifold j,
// and k_cl_scatter reads the same one back: by the workgroup that handles j in the kernels launched one lane per manifold,
// block = j / CL_ASSIGN_LANES (their blockIdx.x; k_cl_comp_assign strides over a list and derives it from j).
#define CL_ASSIGN_LANES 256u
MI_DEV u32 clSubCounter(u32 block) { return block & (CL_SUBCOUNTERS - 1u); }
// Equal-key wave append: the active lanes of a wave each append one entry to the cursor of their key.  Groups of equal keys first
// (ballots only), then ALL the groups' leaders issue their atomics together: one round trip to the memory-side atomic unit per
// wave, not one per distinct key.  Returns the lane's position.  clAppendByCursor: the lanes name their cursor (a task key's
// sub-counter) themselves; clAppendByKey: one workgroup handles all the wave's manifolds (block, clSubCounter), so equal keys are equal cursors.
MI_DEV u32 clAppendByCursor(u32* taskCount, u32 cursor)
{
	u64 todo = __ballot(1), mine = 0;
	const u32 lane = threadIdx.x & 63u;
	while (todo)
	{
		u32 leader = (u32)__ffsll((long long)todo) - 1u;
		u32 c0 = __shfl(cursor, leader);
		u64 same = __ballot(cursor == c0) & todo;
		if (cursor == c0) mine = same;
		todo &= ~same;
	}
	const u32 myLeader = (u32)__ffsll((long long)mine) - 1u, cnt = (u32)__popcll(mine);
	u32 base = 0;
	if (lane == myLeader) base = atomicAdd(&taskCount[cursor], cnt);
	base = __shfl(base, myLeader);
	return base + (u32)__popcll(mine & ((1ull << lane) - 1ull));
}
MI_DEV u32 clAppendByKey(u32* taskCount, u32 key, u32 block) { return clAppendByCursor(taskCount, key * CL_SUBCOUNTERS + clSubCounter(block)); }
// Wave append to the left-over list (what the last curve phase leaves goes to the component phase), one atomic per wave.  Returns
// the position of the lane's entry; the list holds leftCap entries.
MI_DEV u32 clAppendLeft(u32* counters)
{
	const u64 m = __ballot(1);
	const u32 lane = threadIdx.x & 63u, leader = (u32)__ffsll((long long)m) - 1u;
	u32 base = 0;
	if (lane == leader) base = atomicAdd(&counters[CTR_CL_LEFT], (u32)__popcll(m));
	return __shfl(base, leader) + (u32)__popcll(m & ((1ull << lane) - 1ull));
}

// Everything the assignment accumulates into, cleared in one launch.
__global__ void __launch_bounds__(256) k_cl_clear(u32 nb1, u32* __restrict__ wsum, u32* __restrict__ phaseMask, u32* __restrict__ taskCount, u32* __restrict__ jointCount, u32* __restrict__ counters, u32* __restrict__ compLabel,
	const u32* __restrict__ jointBodyMask, u32 keepJointLists)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nb1) { compLabel[i] = i; compLabel[nb1 + i] = i; } // components of what the curve phases leave over: every body its own (both label buffers)
	if (i < CL_LEFT_WORDS) counters[CTR_CL_LEFT + i] = 0;
	if (i == 0u) counters[CTR_CL_SCRATCH] = 0;   // append cursor of the solve launch's row scratch
	if (i < CL_MAX_TASKS && !keepJointLists) jointCount[i] = 0; // (between two refreshes the joints' tasks do not change: their lists are kept, see launch_cluster_build)
	if (i < CL_MAX_PARTS * nb1) wsum[i] = 0;
	if (i < nb1) phaseMask[i] = (keepJointLists && jointBodyMask) ? jointBodyMask[i] : 0u; // (kept joint lists: their bodies' first-phase bit, which the joint assignment sets otherwise)
	if (i < CL_TASK_CURSORS + CL_REMAIN_CURSORS) taskCount[i] = 0; // (+ the split 'still unassigned' counters behind the task counters)
	if (i < CL_STATS_WORDS) counters[CTR_CL_STATUS + i] = 0;  // status, shared bodies, manifolds per phase
	if (i < CL_REMAIN_WORDS) counters[CTR_CL_REMAIN + i] = 0;
}

MI_DEV u32 clWeight(u32 count) { return CL_WEIGHT_MANIFOLD + (count - 1u) * CL_WEIGHT_EXTRA; }

// rep: island representative per body (bodies connected by joints share one; the body itself otherwise; the dummy maps to itself).
// In phase 0 a body counts where its representative is on the curve, so that an island is never cut.
#define CL_WEIGHT_JOINT (6u * CL_WEIGHT_MANIFOLD) // a joint's solve costs several contact rows: at most ~160 joints per task
__global__ void __launch_bounds__(256) k_cl_weights0(const u32* __restrict__ counters, u32 nb, const uint4* __restrict__ actIds, const u32* __restrict__ rank0, const u32* __restrict__ rep,
	u32* __restrict__ wsum, u32* __restrict__ taskKey)
{
	u32 j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= counters[CTR_NUM_ACTIVE]) return;
	uint4 ids = actIds[j];
	u32 ra = rank0[rep ? rep[ids.x] : ids.x], rb = rank0[rep ? rep[ids.y] : ids.y]; // the dummy's rank is 0xFFFFFFFF
	atomicAdd(&wsum[min(ra, rb)], clWeight(ids.z));
	taskKey[j] = CL_UNASSIGNED;
}
__global__ void __launch_bounds__(256) k_cl_joint_weights(u32 numJoints, const uint4* __restrict__ table, const u32* __restrict__ rank0, const u32* __restrict__ rep, u32* __restrict__ wsum)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numJoints) return;
	atomicAdd(&wsum[rank0[rep[table[i].z]]], CL_WEIGHT_JOINT);
}
// After phase 0's scan: every joint goes to the task of its island.
__global__ void __launch_bounds__(256) k_cl_joint_assign(u32 numJoints, u32 nb, u32 taskWeight, u32 maxTasks, const uint4* __restrict__ table, const u32* __restrict__ rank0, const u32* __restrict__ rep, const u32* __restrict__ cum,
	u32* __restrict__ jointTask, u32* __restrict__ jointPos, u32* __restrict__ jointCount, u32* __restrict__ phaseMask, u32* __restrict__ status)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numJoints) return;
	uint4 e = table[i];
	u32 t = cum[rank0[rep[e.z]]] / clEffectiveWeight(taskWeight, cum[nb], maxTasks);
	if (t >= CL_MAX_TASKS) { atomicOr(status, 1u); t = CL_MAX_TASKS - 1u; }
	jointTask[i] = t;
	jointPos[i] = atomicAdd(&jointCount[t], 1u);
	atomicOr(&phaseMask[e.z], 1u); atomicOr(&phaseMask[e.w], 1u);
}
__global__ void __launch_bounds__(256) k_cl_joint_scatter(u32 numJoints, const u32* __restrict__ jointTask, const u32* __restrict__ jointPos, const u32* __restrict__ jointStart, u32* __restrict__ jointList)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < numJoints) jointList[jointStart[jointTask[i]] + jointPos[i]] = i;
}

// Phase p: assign what is interior; what is left adds its weight to the next phase's curve, or (last partition) goes to the rest task.
__global__ void __launch_bounds__(CL_ASSIGN_LANES) k_cl_assign(u32* counters, u32 nb, u32 phase, u32 numParts, u32 taskWeight, u32 maxTasks, const uint4* __restrict__ actIds,
	const u32* __restrict__ rank, const u32* __restrict__ cum, const u32* __restrict__ rankNext, u32* __restrict__ wsumNext,
	u32* __restrict__ taskKey, u32* __restrict__ taskPos, u32* __restrict__ taskCount, u32* __restrict__ phaseMask, u32* __restrict__ status, const u32* __restrict__ rep, u32* __restrict__ leftList, u32 leftCap)
{
	u32 j = blockIdx.x * blockDim.x + threadIdx.x;
	taskWeight = clEffectiveWeight(taskWeight, cum[nb], maxTasks);
	u32* remainSub = taskCount + CL_TASK_CURSORS;
	__shared__ u32 sEntering;
	if (threadIdx.x < 64u)
	{
		u32 v = phase ? remainSub[phase * CL_REMAIN_SUBS + threadIdx.x] : 0u;
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		if (threadIdx.x == 0) sEntering = phase ? v : counters[CTR_NUM_ACTIVE];
	}
	__syncthreads();
	const u32 entering = sEntering;
	const bool dumpAll = entering <= CL_REST_CAP && !rep; // few enough left: one task takes them all, later partitions stay empty (with joints, phase 0 keeps the contacts of an island next to its joints)
	bool pending = j < counters[CTR_NUM_ACTIVE] && taskKey[j] == CL_UNASSIGNED;
	u32 key = CL_UNASSIGNED;
	uint4 ids = make_uint4(0, 0, 0, 0);
	bool da = false, db = false;
	if (pending)
	{
		ids = actIds[j];
		da = ids.x < nb; db = ids.y < nb;
		if (dumpAll) key = CL_MAX_PARTS * CL_MAX_TASKS;
		else
		{
			u32 ta = da ? cum[rank[rep ? rep[ids.x] : ids.x]] / taskWeight : 0u, tb = db ? cum[rank[rep ? rep[ids.y] : ids.y]] / taskWeight : 0u; // rep: phase 0 with joints only
			if (!da) ta = tb;
			if (!db) tb = ta;
			if (ta == tb)
			{
				if (ta >= CL_MAX_TASKS) { atomicOr(status, 1u); ta = CL_MAX_TASKS - 1u; }
				key = phase * CL_MAX_TASKS + ta;
			}
			else if (phase + 1u == numParts && !leftList) key = CL_MAX_PARTS * CL_MAX_TASKS; // the rest task
		}
	}
	// what the last curve phase leaves goes to the component phase (k_cl_components), through a list
	const bool toList = pending && key == CL_UNASSIGNED && phase + 1u == numParts && leftList;
	if (toList) { const u32 at = clAppendLeft(counters); if (at < leftCap) leftList[at] = j; }
	bool left = pending && key == CL_UNASSIGNED;
	u32 numLeft = (u32)__syncthreads_count(left); // one atomic per workgroup
	if (threadIdx.x == 0 && numLeft) atomicAdd(&remainSub[(phase + 1u) * CL_REMAIN_SUBS + (blockIdx.x & (CL_REMAIN_SUBS - 1u))], numLeft);
	if (!pending) return;
	if (key != CL_UNASSIGNED)
	{
		u32 ph = key / CL_MAX_TASKS;
		taskKey[j] = key;
		// append position: one atomic per (wave, task) instead of one per manifold.  The active list follows the narrowphase slots,
		// i.e. the broadphase's cell order, so a wave's manifolds belong to very few tasks; returning atomics on one address are
		// served one after the other (~0.2 us each), and a task used to get ~80 of them per sub-counter.
		taskPos[j] = clAppendByKey(taskCount, key, blockIdx.x);
		// (most bodies have the bit already from another manifold of theirs: look before the atomic)
		if (da && !(__hip_atomic_load(&phaseMask[ids.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (1u << ph))) atomicOr(&phaseMask[ids.x], 1u << ph);
		if (db && !(__hip_atomic_load(&phaseMask[ids.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (1u << ph))) atomicOr(&phaseMask[ids.y], 1u << ph);
	}
	else if (!toList)
	{
		u32 ra = rankNext[ids.x], rb = rankNext[ids.y];
		atomicAdd(&wsumNext[min(ra, rb)], clWeight(ids.z));
	}
}

// ---- the partition cached between re-sorts -------------------------------------------------------------------------------------
// Bodies move a fraction of their size per step and the pile's contacts change by well under a per cent per step, so the chunk
// boundaries of a phase (which chunk a body's curve position belongs to) are computed with the full pipeline — weights, scans,
// one assignment pass per phase — only on the steps that also re-sort the bodies along the curves; in between, the stored chunk of
// every body per phase decides where a manifold goes, in ONE pass without scans.  Any partition is valid; a stale one only lets the
// tasks' sizes drift by the few per cent the pile changes in those steps (the refresh chunks are cut 4 % short for that).
__global__ void __launch_bounds__(256) k_cl_store_chunks(u32 nb, u32 taskWeight, u32 maxTasks, const u32* __restrict__ rank, const u32* __restrict__ cum, const u32* __restrict__ rep, u32* __restrict__ chunk)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nb) return;
	u32 t = cum[rank[rep ? rep[i] : i]] / clEffectiveWeight(taskWeight, cum[nb], maxTasks);
	chunk[i] = min(t, CL_MAX_TASKS - 1u);
}
// numCached: the phases placed from the stored chunks (1: the first phase only — the later phases, a quarter of the manifolds, keep
// the per-step pipeline on what is left, which keeps their tasks at the size their fast path needs).  What the cached phases leave
// goes on to phase numCached (its weight onto that phase's curve), or to the rest task when there is none.
__global__ void __launch_bounds__(CL_ASSIGN_LANES) k_cl_assign_cached(u32* counters, u32 nb, u32 numParts, u32 numCached, u32 withJoints, const uint4* __restrict__ actIds, const u32* __restrict__ chunk,
	const u32* __restrict__ rankNext, u32* __restrict__ wsumNext, u32* __restrict__ taskKey, u32* __restrict__ taskPos, u32* __restrict__ taskCount, u32* __restrict__ phaseMask, u32* __restrict__ leftList, u32 leftCap)
{
	const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
	const u32 numActive = counters[CTR_NUM_ACTIVE];
	const bool live = j < numActive;
	const bool dumpAll = numActive <= CL_REST_CAP && !withJoints;
	u32* remainSub = taskCount + CL_TASK_CURSORS;
	u32 key = CL_MAX_PARTS * CL_MAX_TASKS, phase = numParts; // the rest task unless a phase takes it
	uint4 ids = make_uint4(0, 0, 0, 0);
	bool da = false, db = false;
	if (live)
	{
		ids = actIds[j];
		da = ids.x < nb; db = ids.y < nb;
		if (!dumpAll)
		{
			// (the first two phases' chunks are requested together: a manifold the first phase cuts does not wait a second round trip)
			const u32* c1 = chunk + (size_t)(nb + 1u);
			u32 ta = da ? chunk[ids.x] : 0u, tb = db ? chunk[ids.y] : 0u, ta1 = (da && numCached > 1u) ? c1[ids.x] : 0u, tb1 = (db && numCached > 1u) ? c1[ids.y] : 0u;
			for (u32 p = 0; p < numCached; ++p)
			{
				if (p == 1u) { ta = ta1; tb = tb1; }
				else if (p > 1u) { const u32* c = chunk + (size_t)p * (nb + 1u); ta = da ? c[ids.x] : 0u; tb = db ? c[ids.y] : 0u; }
				if (!da) ta = tb;
				if (!db) tb = ta;
				if (ta == tb) { key = p * CL_MAX_TASKS + ta; phase = p; break; }
			}
		}
	}
	// manifolds still unassigned when phase q + 1 starts (statistics)
	const bool goesOn = live && phase == numParts && numCached < numParts && !dumpAll; // left by the cached phases, with a pipeline phase to go to
	for (u32 q = 0; q < numCached; ++q)
	{
		u32 numLeft = (u32)__syncthreads_count(live && phase > q);
		if (threadIdx.x == 0 && numLeft) atomicAdd(&remainSub[(q + 1u) * CL_REMAIN_SUBS + (blockIdx.x & (CL_REMAIN_SUBS - 1u))], numLeft);
	}
	const bool toList = live && phase == numParts && numCached == numParts && !dumpAll && leftList; // left by ALL curve phases: the component phase takes it
	if (toList) { const u32 at = clAppendLeft(counters); if (at < leftCap) leftList[at] = j; taskKey[j] = CL_UNASSIGNED; }
	if (!live || toList) return;
	if (goesOn)
	{
		taskKey[j] = CL_UNASSIGNED;
		u32 ra = rankNext[ids.x], rb = rankNext[ids.y];
		atomicAdd(&wsumNext[min(ra, rb)], clWeight(ids.z));
		return;
	}
	taskKey[j] = key;
	taskPos[j] = clAppendByKey(taskCount, key, blockIdx.x);
	const u32 ph = key / CL_MAX_TASKS;
	if (da) atomicOr(&phaseMask[ids.x], 1u << ph); // (results unused: the wave does not wait for them; a load-then-or would)
	if (db) atomicOr(&phaseMask[ids.y], 1u << ph);
}
__global__ void __launch_bounds__(256) k_cl_joint_assign_cached(u32 numJoints, const uint4* __restrict__ table, const u32* __restrict__ chunk0, u32* __restrict__ jointTask, u32* __restrict__ jointPos,
	u32* __restrict__ jointCount, u32* __restrict__ phaseMask)
{
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= numJoints) return;
	uint4 e = table[i];
	u32 t = chunk0[e.z]; // (the chunk of the island's representative: k_cl_store_chunks)
	jointTask[i] = t;
	jointPos[i] = atomicAdd(&jointCount[t], 1u);
	atomicOr(&phaseMask[e.z], 1u); atomicOr(&phaseMask[e.w], 1u);
}

// ---- the component phase ---------------------------------------------------------------------------------------------------------
// What the curve phases leave over (a few per cent of the manifolds: those cut by every curve's chunk borders, in small clumps where
// the borders cross) is not cut again: its connected components (bodies joined by left-over manifolds) are found and whole components
// are dealt to the tasks of ONE more phase, so nothing is left for a further phase and the rest task stays empty (each phase costs a
// hand-over and its slowest task's colours in EVERY iteration).  Union-find on a global label array (label[b] = a body of b's
// component with a smaller or equal id; k_cl_clear set label[b] = b in both of its buffers), a fixed number of rounds, each reading
// the labels the previous round left and writing the next buffer (k_cl_comp_round), so that the labels after every round, and with
// them the schedule, do not depend on how the manifolds of a round interleave — a component that has not converged by then only
// sends the manifolds whose ends still disagree to the rest task.  Components are
// dealt to tasks by a hash of their label (the clumps are tens of manifolds against tasks of hundreds: the load evens out), a
// component too large for a task is sent to the rest task.
#define CL_COMP_ROUNDS 4u
#define CL_COMP_LABEL_BUFFERS 2u // World::cluster.compLabel: nb + 1 labels each; a round reads one and writes the other, k_cl_clear initialises both
static_assert(CL_COMP_ROUNDS % CL_COMP_LABEL_BUFFERS == 0u, "the last round must write the first label buffer: the weights and the assignment read it");
#define CL_COMP_MAX_WEIGHT (64u * 1400u) // a component heavier than this cannot be a task's (k_cl_color's tables): rest task
#define CL_COMP_BLOCKS 64u               // workgroups of the component kernels (they stride over the list: its length is only known on the device)
#define CL_LD(P_) __hip_atomic_load((P_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
MI_DEV u32 clFind(u32* label, u32 x) { u32 r = CL_LD(&label[x]); for (u32 h = 0; h < 16u; ++h) { u32 up = CL_LD(&label[r]); if (up == r) break; r = up; } return r; }
// One round: every left-over manifold hooks the larger of its ends' roots under the smaller one, and points both ends at the
// smaller root.  A round reads the labels of the previous round (labelIn, not written during the round) and lowers those of the next
// (labelOut) with atomicMin only, so what a round produces does not depend on how its manifolds interleave: the components, the
// weights and so the whole schedule repeat from run to run.  labelOut still holds the labels of two rounds ago, which are valid
// (a body of the same component, smaller or equal id) and never below what this round writes into them.
MI_DEV u32 clFindIn(const u32* __restrict__ label, u32 x) { u32 r = label[x]; for (u32 h = 0; h < 16u; ++h) { u32 up = label[r]; if (up == r) break; r = up; } return r; }
__global__ void __launch_bounds__(256) k_cl_comp_round(const u32* __restrict__ counters, u32 nb, u32 leftCap, const u32* __restrict__ leftList, const uint4* __restrict__ actIds,
	const u32* __restrict__ labelIn, u32* __restrict__ labelOut)
{
	const u32 n = min(counters[CTR_CL_LEFT], leftCap);
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
	{
		uint4 ids = actIds[leftList[i]];
		if (ids.x >= nb || ids.y >= nb) continue;
		const u32 ra = clFindIn(labelIn, ids.x), rb = clFindIn(labelIn, ids.y), lo = min(ra, rb);
		if (ra != rb) atomicMin(&labelOut[max(ra, rb)], lo);
		atomicMin(&labelOut[ids.x], lo);
		atomicMin(&labelOut[ids.y], lo);
	}
}
// Weight of every component (at its label) and of the lot (counters[CTR_CL_LEFT + 2], zeroed by k_cl_clear).
__global__ void __launch_bounds__(256) k_cl_comp_weights(u32* __restrict__ counters, u32 nb, u32 leftCap, const u32* __restrict__ leftList, const uint4* __restrict__ actIds, u32* label, u32* __restrict__ compWeight)
{
	const u32 n = min(counters[CTR_CL_LEFT], leftCap);
	u32 mine = 0;
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
	{
		uint4 ids = actIds[leftList[i]];
		u32 b = ids.x < nb ? ids.x : ids.y;
		u32 w = clWeight(ids.z);
		atomicAdd(&compWeight[clFind(label, b)], w);
		mine += w;
	}
	for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
	if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(&counters[CTR_CL_LEFT + 2], mine);
}
// Deal the manifolds: both ends in one component of fitting size -> that component's task (hash of its label); otherwise the rest task.
// The components share no body and a manifold's colour follows from its component alone, so the number of tasks they are dealt to
// changes no body's sequence of row solves: taskWeight (World::cluster.taskWeightComp) is chosen for where the tasks run, behind a
// first task whose bodies and rows already sit in the workgroup's LDS.  maxTasks: what the sweep's launch runs of one phase.
__global__ void __launch_bounds__(CL_ASSIGN_LANES) k_cl_comp_assign(u32* __restrict__ counters, u32 nb, u32 phase, u32 taskWeight, u32 maxTasks, u32 leftCap, const u32* __restrict__ leftList, const uint4* __restrict__ actIds, u32* label,
	const u32* __restrict__ compWeight, u32* __restrict__ taskKey, u32* __restrict__ taskPos, u32* __restrict__ taskCount, u32* __restrict__ phaseMask)
{
	const u32 n = min(counters[CTR_CL_LEFT], leftCap), total = counters[CTR_CL_LEFT + 2];
	const u32 numTasks = min(max(1u, (total + taskWeight - 1u) / taskWeight), maxTasks);
	if (blockIdx.x == 0 && threadIdx.x == 0) counters[CTR_CL_LEFT + 1] = numTasks;
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
	{
		const u32 j = leftList[i];
		uint4 ids = actIds[j];
		const bool da = ids.x < nb, db = ids.y < nb;
		u32 la = da ? clFind(label, ids.x) : 0u, lb = db ? clFind(label, ids.y) : 0u;
		if (!da) la = lb;
		if (!db) lb = la;
		u32 key = CL_MAX_PARTS * CL_MAX_TASKS;
		if (la == lb && compWeight[la] <= CL_COMP_MAX_WEIGHT) key = phase * CL_MAX_TASKS + clHash(la * 2654435761u) % numTasks;
		else if (la != lb) atomicAdd(&counters[CTR_CL_LEFT + 3], 1u); else atomicMax(&counters[CTR_CL_LEFT + 4], compWeight[la]); // (statistics: not converged / too large)
		taskKey[j] = key;
		// (the sub-counter k_cl_scatter derives from j's workgroup in ITS launch.  One atomic per wave and cursor: the phase has a dozen
		// tasks, and ~5 k returning atomics on their ~100 cursors, served one after the other, were most of this kernel's 12 us)
		taskPos[j] = clAppendByCursor(taskCount, key * CL_SUBCOUNTERS + clSubCounter(j / CL_ASSIGN_LANES));
		const u32 ph = key / CL_MAX_TASKS;
		if (da) atomicOr(&phaseMask[ids.x], 1u << ph);
		if (db) atomicOr(&phaseMask[ids.y], 1u << ph);
	}
}
#undef CL_LD

// One workgroup: exclusive scan of the per-task counts -> first slot of every task; tasks per phase; end of schedule.
// Inclusive prefix sum over the 1024 lanes of a workgroup: shuffles inside a wave, one LDS step across the 16 waves (two barriers; a
// Hillis-Steele ladder through LDS was 20).
MI_DEV u32 clBlockInclusive1024(u32 v, u32* waveTotals /* [16], LDS */)
{
	const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (u32 o = 1; o < 64u; o <<= 1) { u32 up = __shfl_up(v, o); if (lane >= o) v += up; }
	if (lane == 63u) waveTotals[wave] = v;
	__syncthreads();
	u32 before = 0;
	for (u32 k = 0; k < 16u; ++k) before += (k < wave) ? waveTotals[k] : 0u;
	__syncthreads(); // (waveTotals is reused by the next call)
	return v + before;
}
__global__ void __launch_bounds__(1024) k_cl_offsets(u32* __restrict__ counters, u32 numParts, u32 narrowLimit, const u32* __restrict__ taskCount, u32* __restrict__ taskStart, const u32* __restrict__ jointCount, u32* __restrict__ jointStart)
{
	__shared__ u32 part[16];
	__shared__ u32 lastTask[CL_MAX_PHASES], oversize;
	const u32 total = CL_TASK_CURSORS, per = (total + 1023u) / 1024u;
	u32 t = threadIdx.x;
	if (t < CL_MAX_PHASES) lastTask[t] = 0;
	if (t == 0) oversize = 0;
	__shared__ uint16_t cnt[CL_TASK_CURSORS]; // the counters, read once with neighbouring lanes on neighbouring words (a sub-counter holds < 64 k)
	for (u32 e = t; e < total; e += 1024u) cnt[e] = (uint16_t)min(taskCount[e], 0xFFFFu);
	__syncthreads(); // (cnt, lastTask)
	u32 sum = 0;
	for (u32 k = 0; k < per; ++k) if (t * per + k < total) sum += cnt[t * per + k];
	u32 run = clBlockInclusive1024(sum, part) - sum;
	// (a lane's 20 consecutive starts leave as five 16-byte stores: 20 word stores per lane, each wave's spread over 5 KB, were
	// ~13 k cache-line writes through ONE compute unit: 12.9 -> 7.1 us)
	static_assert(CL_TASK_CURSORS % (1024u * 4u) == 0u, "every lane scans the same number of cursors, in whole groups of four");
	for (u32 k = 0; k < per; k += 4u)
	{
		u32 v[4];
		for (u32 q = 0; q < 4u; ++q)
		{
			u32 e = t * per + k + q, c = cnt[e], key = e / CL_SUBCOUNTERS;
			v[q] = run; run += c;
			if (c) atomicMax(&lastTask[key / CL_MAX_TASKS], (key % CL_MAX_TASKS) + 1u);
		}
		*(uint4*)(taskStart + t * per + k) = make_uint4(v[0], v[1], v[2], v[3]);
	}
	if (t == 1023u) taskStart[total] = run;
	__syncthreads();
	// joints per phase-0 task (CL_MAX_TASKS <= 1024 entries: one per lane); a task may hold joints and no manifold
	{
		u32 jc = (jointCount && t < CL_MAX_TASKS) ? jointCount[t] : 0u;
		const u32 jIncl = jointCount ? clBlockInclusive1024(jc, part) : 0u; // (uniform branch)
		if (jointStart && t < CL_MAX_TASKS) { jointStart[t] = jIncl - jc; if (t == CL_MAX_TASKS - 1u) jointStart[CL_MAX_TASKS] = jIncl; }
		if (jc) atomicMax(&lastTask[0], t + 1u);
		// tasks of narrowLimit items (manifolds + joints) or more: k_cl_color's wide instance colours those, and only those
		u32 big = 0;
		for (u32 key = t; key < total / CL_SUBCOUNTERS; key += 1024u)
		{
			u32 items = key < CL_MAX_TASKS ? jc : 0u; // (key = t there)
			for (u32 k = 0; k < CL_SUBCOUNTERS; ++k) items += cnt[key * CL_SUBCOUNTERS + k];
			big += items >= narrowLimit ? 1u : 0u;
		}
		if (big) atomicAdd(&oversize, big);
		__syncthreads();
	}
	const u32 totalManifolds = taskStart[total];
	if (t < CL_MAX_PHASES) counters[CTR_CL_NUM_TASKS + t] = lastTask[t];
	if (t < CL_REMAIN_WORDS) { u32 v = 0; for (u32 k = 0; k < CL_REMAIN_SUBS; ++k) v += taskCount[total + t * CL_REMAIN_SUBS + k]; counters[CTR_CL_REMAIN + t] = v; } // for the host's statistics / phase-count adaptation
	if (t == 0)
	{
		counters[CTR_NUM_MANIFOLDS] = totalManifolds;
		counters[CTR_NUM_COLORS] = 0; // k_cl_color: atomicMax of the local colour counts
		counters[CTR_CL_COLOR_TASKS] = oversize; counters[CTR_CL_COLOR_TASKS + 1] = 0; counters[CTR_CL_COLOR_TASKS + 2] = 0; // ... and the tasks each instance coloured
		for (int k = 0; k < 3; ++k) { counters[CTR_CL_BBOX + k] = 0xFFFFFFFFu; counters[CTR_CL_BBOX + 3 + k] = 0u; } // consumed by k_cl_keys: ready for the next step
	}
}

__global__ void __launch_bounds__(CL_ASSIGN_LANES) k_cl_scatter(const u32* __restrict__ counters, const u32* __restrict__ taskKey, const u32* __restrict__ taskPos, const u32* __restrict__ taskStart, u32* __restrict__ pre)
{
	u32 j = blockIdx.x * blockDim.x + threadIdx.x; // same launch geometry as k_cl_assign: blockIdx selects the same sub-counter
	if (j >= counters[CTR_NUM_ACTIVE]) return;
	pre[taskStart[taskKey[j] * CL_SUBCOUNTERS + clSubCounter(blockIdx.x)] + taskPos[j]] = j;
}

// ---------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------
// Cell shifts of the phases' Morton curves (phase 0 unshifted).
static const ClShifts CL_SHIFTS = { { { 0, 0, 0 }, { 13, 9, 15 }, { 27, 21, 31 }, { 7, 29, 5 } } };
static const u32 CL_SORT_INTERVAL = 8;           // steps between re-sorts of the bodies along the curves (= refreshes of the cached chunks)
static const u32 CL_CHUNK_HEADROOM_PERCENT = 10; // the cached chunks are cut this much short: the pile may grow until the next refresh

static const dim3 CL_BLOCK(256);
static dim3 clGrid(u32 items) { return dim3((items + 255) / 256); }
static dim3 clManifoldGrid(u32 numPairs) { return dim3((numPairs + CL_ASSIGN_LANES - 1u) / CL_ASSIGN_LANES); } // one lane per manifold: k_cl_assign, k_cl_assign_cached, k_cl_scatter (clSubCounter)
// tasks per phase, with a margin for the chunks' rounding
static u32 clMaxTasks(const World& w) { return std::min<u32>(CL_MAX_TASKS / CL_TASKS_PER_PHASE, w.cluster.blocks) - std::min<u32>(8u, w.cluster.blocks / 8u); }

// The buffers sized by the bodies, the pair capacity and the task table.  false = an allocation failed.
static bool clSizeBuffers(World& w)
{
	const u32 nb = w.nb, P = CL_MAX_PARTS;
	const size_t nb1 = (size_t)nb + 1;
	w.cluster.keys.ensure((size_t)P * nb, w.stream); w.cluster.keysSorted.ensure((size_t)P * nb, w.stream); w.cluster.vals.ensure((size_t)P * nb, w.stream); w.cluster.sorted.ensure((size_t)P * nb, w.stream);
	w.cluster.rank.ensure((size_t)P * nb1, w.stream); w.cluster.sharedSlot.ensure((size_t)CL_MAX_PHASES * nb1, w.stream); w.cluster.wsum.ensure(P * nb1, w.stream); w.cluster.cum.ensure(nb1, w.stream); w.cluster.phaseMask.ensure(nb1, w.stream);
	w.cluster.taskKey.ensure(w.pairCap, w.stream); w.cluster.taskPos.ensure(w.pairCap, w.stream); w.cluster.pre.ensure(w.pairCap, w.stream); w.cluster.local.ensure(w.pairCap, w.stream); w.cluster.entry.ensure(4 * w.pairCap, w.stream);
	const u32 totalKeys = CL_MAX_PHASES * CL_MAX_TASKS;
	w.cluster.taskCount.ensure(CL_TASK_CURSORS + CL_REMAIN_CURSORS, w.stream); w.cluster.taskStart.ensure(CL_TASK_CURSORS + 1, w.stream);
	w.cluster.tasks.ensure((size_t)totalKeys * sizeof(ClTask), w.stream); w.cluster.bodyList.ensure((size_t)totalKeys * CL_BODY_STRIDE, w.stream);
	return !w.lastError;
}
// The joints' task lists (nj joints run inside the sweep), the component phase's labels and list, the cached chunks.
static bool clSizeListBuffers(World& w, u32 nj)
{
	const size_t nb1 = (size_t)w.nb + 1;
	w.cluster.jointCount.ensure(CL_MAX_TASKS, w.stream); w.cluster.jointStart.ensure(CL_MAX_TASKS + 1, w.stream);
	w.cluster.jointTask.ensure(std::max(nj, 1u), w.stream); w.cluster.jointPos.ensure(std::max(nj, 1u), w.stream); w.cluster.jointList.ensure(std::max(nj, 1u), w.stream); w.cluster.taskJoints.ensure(std::max(nj, 1u), w.stream);
	w.cluster.jointClassStart.ensure((size_t)CL_MAX_TASKS * (CL_MAX_JOINT_CLASSES + 2u), w.stream);
	if (w.lastError) return false;
	w.cluster.compLabel.ensure(CL_COMP_LABEL_BUFFERS * nb1, w.stream); w.cluster.leftList.ensure(w.pairCap, w.stream);
	if (w.lastError) return false;
	w.cluster.chunk.ensure((size_t)CL_MAX_PARTS * nb1, w.stream);
	return !w.lastError;
}

// Body order along the phases' curves.  Any order is correct, this one makes the clusters compact; bodies move a fraction of
// their size per step, so the order is refreshed every few steps only (one sort of all bodies along all curves), at once when bodies were
// added and after a snapshot was taken or restored (so that a restored world and its original keep making the same choices).
// Returns whether this step re-sorted (and so re-cuts the chunks); the steps in between reuse the stored chunks.
static bool clRefreshBodyOrder(World& w)
{
	const u32 nb = w.nb, P = CL_MAX_PARTS;
	const bool due = w.cluster.sortDue || w.cluster.sortAge >= CL_SORT_INTERVAL || w.cluster.sortBodies != nb;
	if (due)
	{
		// the curves in use and the one behind them (phase p attributes what it leaves over along curve p + 1) are sorted; all of them the first
		// time and when the body count changed, so that every rank array holds valid positions (each sort is ~80 us at 100 k bodies)
		const u32 sortParts = (w.cluster.sortBodies != nb) ? P : CL_CURVE_PARTS + 1u;
		u32 maxShift = 0;
		for (const auto& s : CL_SHIFTS.s) for (u32 v : s) maxShift = std::max(maxShift, v);
		hipLaunchKernelGGL(k_cl_bbox, dim3(std::min<u32>(clGrid(nb).x, 64u)), CL_BLOCK, 0, w.stream, nb, w.cog.p, w.simMask.p, w.dCounters.p);
		hipLaunchKernelGGL(k_cl_keys, clGrid(nb), CL_BLOCK, 0, w.stream, nb, P, CL_SHIFTS, maxShift, w.cog.p, w.simMask.p, w.dCounters.p, w.cluster.keys.p, w.cluster.vals.p);
		// The curves lie curve-major in cluster.keys / cluster.vals and carry their index in the keys' top bits: one stable sort of sortParts x nb
		// items leaves curve p's order in [p * nb, (p + 1) * nb), equal keys by ascending body, as one sort per curve did (at 100 k
		// bodies rocPRIM runs a block sort and 7 merge launches per curve; the 300 k items of three curves take one block sort and 18
		// merge launches: 146 -> 111 us of kernel time per refresh, profiles/cluster_build.txt).
		static_assert(CL_MAX_PARTS <= 4u, "the curve index has two key bits above the 30-bit Morton code");
		prim_sort_pairs_u32(w, w.cluster.keys.p, w.cluster.keysSorted.p, w.cluster.vals.p, w.cluster.sorted.p, sortParts * nb, 32);
		hipLaunchKernelGGL(k_cl_ranks, clGrid(nb), CL_BLOCK, 0, w.stream, nb, sortParts, w.cluster.sorted.p, w.cluster.rank.p);
		w.cluster.sortDue = false; w.cluster.sortAge = 0; w.cluster.sortBodies = nb;
	}
	w.cluster.sortAge++;
	return due;
}

// Everything the assignment accumulates into, cleared in one launch.
static void clClear(World& w, u32 nj, bool keepJointLists)
{
	const size_t nb1 = (size_t)w.nb + 1;
	const u32 clearItems = std::max<u32>((u32)(CL_MAX_PARTS * nb1), CL_TASK_CURSORS + CL_REMAIN_CURSORS);
	hipLaunchKernelGGL(k_cl_clear, clGrid(clearItems), CL_BLOCK, 0, w.stream, (u32)nb1, w.cluster.wsum.p, w.cluster.phaseMask.p, w.cluster.taskCount.p, w.cluster.jointCount.p, w.dCounters.p, w.cluster.compLabel.p,
		nj ? w.cluster.jointBodyMask.p : (const u32*)nullptr, keepJointLists ? 1u : 0u);
}

// A refresh step: the full pipeline per curve phase (weights, scan, assignment), which also stores every body's chunk for the cached pass.
// withJoints: joints run inside the sweep (islands are not cut); leftList: where the last phase's left-overs go (null: the rest task).
static void clAssignByPhase(World& w, u32 numPairs, u32 nj, bool withJoints, u32* leftList)
{
	const u32* rep = withJoints ? w.cluster.rep.p : nullptr;
	const u32 nb = w.nb, parts = CL_CURVE_PARTS, maxTasks = clMaxTasks(w), leftCap = (u32)w.pairCap;
	const size_t nb1 = (size_t)nb + 1;
	const u32 firstFlags = withJoints ? CL_WEIGHT_ISLANDS : 0u; // (goes with the first phase's weight)
	const u32 weight0 = w.cluster.taskWeight - (u32)((u64)w.cluster.taskWeight * CL_CHUNK_HEADROOM_PERCENT / 100u), weightLater = w.cluster.taskWeightLater - (u32)((u64)w.cluster.taskWeightLater * CL_CHUNK_HEADROOM_PERCENT / 100u);
	hipLaunchKernelGGL(k_cl_weights0, clGrid(numPairs), CL_BLOCK, 0, w.stream, w.dCounters.p, nb, w.actIds.p, w.cluster.rank.p, rep, w.cluster.wsum.p, w.cluster.taskKey.p);
	if (nj) hipLaunchKernelGGL(k_cl_joint_weights, clGrid(nj), CL_BLOCK, 0, w.stream, nj, w.cluster.jointTable.p, w.cluster.rank.p, rep, w.cluster.wsum.p);
	for (u32 p = 0; p < parts; ++p)
	{
		u32* wsum = w.cluster.wsum.p + (size_t)p * nb1; u32* wsumNext = w.cluster.wsum.p + (size_t)std::min(p + 1, CL_MAX_PARTS - 1) * nb1;
		prim_exclusive_scan_u32(w, wsum, w.cluster.cum.p, nb + 1);
		hipLaunchKernelGGL(k_cl_assign, clManifoldGrid(numPairs), dim3(CL_ASSIGN_LANES), 0, w.stream, w.dCounters.p, nb, p, parts, p ? weightLater : (weight0 | firstFlags), maxTasks, w.actIds.p, w.cluster.rank.p + (size_t)p * nb1, w.cluster.cum.p,
			w.cluster.rank.p + (size_t)std::min(p + 1, CL_MAX_PARTS - 1) * nb1, wsumNext, w.cluster.taskKey.p, w.cluster.taskPos.p, w.cluster.taskCount.p, w.cluster.phaseMask.p, w.dCounters.p + CTR_CL_STATUS, p == 0 ? rep : nullptr, leftList, leftCap);
		if (p == 0 && nj) // (cum still holds phase 0's scan)
			hipLaunchKernelGGL(k_cl_joint_assign, clGrid(nj), CL_BLOCK, 0, w.stream, nj, nb, weight0 | firstFlags, maxTasks, w.cluster.jointTable.p, w.cluster.rank.p, rep, w.cluster.cum.p, w.cluster.jointTask.p, w.cluster.jointPos.p, w.cluster.jointCount.p, w.cluster.phaseMask.p, w.dCounters.p + CTR_CL_STATUS);
		hipLaunchKernelGGL(k_cl_store_chunks, clGrid(nb), CL_BLOCK, 0, w.stream, nb, p ? weightLater : (weight0 | firstFlags), maxTasks, w.cluster.rank.p + (size_t)p * nb1, w.cluster.cum.p, p == 0 ? rep : nullptr, w.cluster.chunk.p + (size_t)p * nb1);
	}
}
// Between two refreshes: one pass over the manifolds with the stored chunks; the joints' lists are rebuilt unless they are kept.
static void clAssignCached(World& w, u32 numPairs, u32 nj, bool withJoints, bool keepJointLists, u32* leftList)
{
	const u32 nb = w.nb, parts = CL_CURVE_PARTS;
	const size_t nb1 = (size_t)nb + 1;
	hipLaunchKernelGGL(k_cl_assign_cached, clManifoldGrid(numPairs), dim3(CL_ASSIGN_LANES), 0, w.stream, w.dCounters.p, nb, parts, parts, withJoints ? 1u : 0u, w.actIds.p, w.cluster.chunk.p,
		w.cluster.rank.p + (size_t)parts * nb1, w.cluster.wsum.p + (size_t)parts * nb1, w.cluster.taskKey.p, w.cluster.taskPos.p, w.cluster.taskCount.p, w.cluster.phaseMask.p, leftList, (u32)w.pairCap);
	if (nj && !keepJointLists) hipLaunchKernelGGL(k_cl_joint_assign_cached, clGrid(nj), CL_BLOCK, 0, w.stream, nj, w.cluster.jointTable.p, w.cluster.chunk.p, w.cluster.jointTask.p, w.cluster.jointPos.p, w.cluster.jointCount.p, w.cluster.phaseMask.p);
}
// What the curve phases left over (World::cluster.leftList): whole connected components to the tasks of one more phase (index CL_CURVE_PARTS).
static void clAssignComponents(World& w)
{
	const u32 nb = w.nb, leftCap = (u32)w.pairCap;
	const size_t nb1 = (size_t)nb + 1;
	u32* compWeight = w.cluster.wsum.p + (size_t)(CL_MAX_PARTS - 1) * nb1; // (the last curve's weight sums are not in use: zeroed by k_cl_clear)
	for (u32 r = 0; r < CL_COMP_ROUNDS; ++r) // (the label buffers alternate: round r reads buffer r % 2 and writes the other)
		hipLaunchKernelGGL(k_cl_comp_round, dim3(CL_COMP_BLOCKS), CL_BLOCK, 0, w.stream, w.dCounters.p, nb, leftCap, w.cluster.leftList.p, w.actIds.p,
			(const u32*)(w.cluster.compLabel.p + (size_t)(r % CL_COMP_LABEL_BUFFERS) * nb1), w.cluster.compLabel.p + (size_t)((r + 1u) % CL_COMP_LABEL_BUFFERS) * nb1);
	hipLaunchKernelGGL(k_cl_comp_weights, dim3(CL_COMP_BLOCKS), CL_BLOCK, 0, w.stream, w.dCounters.p, nb, leftCap, w.cluster.leftList.p, w.actIds.p, w.cluster.compLabel.p, compWeight);
	const u32 maxTasks = std::min<u32>(CL_MAX_TASKS, CL_TASKS_PER_PHASE * std::max(1u, w.cluster.blocks)); // (beyond it k_cl_solve gives the step up: status 128)
	hipLaunchKernelGGL(k_cl_comp_assign, dim3(CL_COMP_BLOCKS), dim3(CL_ASSIGN_LANES), 0, w.stream, w.dCounters.p, nb, CL_CURVE_PARTS, w.cluster.taskWeightComp, maxTasks, leftCap, w.cluster.leftList.p, w.actIds.p, w.cluster.compLabel.p, compWeight,
		w.cluster.taskKey.p, w.cluster.taskPos.p, w.cluster.taskCount.p, w.cluster.phaseMask.p);
}
// First slot of every task, then every manifold (and, unless kept, joint) to its slot.
static void clOffsetsAndScatter(World& w, u32 numPairs, u32 nj, bool keepJointLists)
{
	hipLaunchKernelGGL(k_cl_offsets, dim3(1), dim3(1024), 0, w.stream, w.dCounters.p, CL_CURVE_PARTS, w.cluster.colorNarrowLimit, w.cluster.taskCount.p, w.cluster.taskStart.p, nj ? w.cluster.jointCount.p : (u32*)nullptr, nj ? w.cluster.jointStart.p : (u32*)nullptr);
	if (nj && !keepJointLists) hipLaunchKernelGGL(k_cl_joint_scatter, clGrid(nj), CL_BLOCK, 0, w.stream, nj, w.cluster.jointTask.p, w.cluster.jointPos.p, w.cluster.jointStart.p, w.cluster.jointList.p);
	w.cluster.jointListsValid = nj != 0u;
	hipLaunchKernelGGL(k_cl_scatter, clManifoldGrid(numPairs), dim3(CL_ASSIGN_LANES), 0, w.stream, w.dCounters.p, w.cluster.taskKey.p, w.cluster.taskPos.p, w.cluster.taskStart.p, w.cluster.pre.p);
}

// Everything between "manifolds exist" and "rows can be initialised": order of the bodies, tasks, local colouring, final slot order.
void launch_cluster_build(World& w, u32 numPairs)
{
	if (!numPairs) return;
	const bool withJoints = cluster_solves_joints(w);
	const u32 nj = withJoints ? w.cluster.numJoints : 0u;
	if (!clSizeBuffers(w)) return;
	launch_active_list(w, numPairs); // active manifolds (k_active_list of the colouring: also counts contacts); no warm colours, no global colour masks
	bool refresh = clRefreshBodyOrder(w);
	if (!clSizeListBuffers(w, nj)) return;
	// A world whose curve phases left nothing over in the last step (ragdolls standing apart: every island interior to its task) skips
	// the component phase's six launches; what the curves do leave over in this step then goes to the rest task, as without the
	// component phase, and the next step runs the components again (World::countPreviousStep).
	u32* leftList = !w.cluster.compIdle ? w.cluster.leftList.p : nullptr;
	if (w.cluster.chunkJointVersion != w.jointVersion || w.cluster.chunkWithJoints != withJoints) refresh = true; // (the stored chunks were cut for other joints)
	// The joints' tasks follow their islands' chunks, which change at a refresh only: in between, the task lists of the joints (task,
	// position, counts, the scattered list) are kept as the refresh step built them — two launches less per step for a ragdoll world.
	const bool keepJointLists = !refresh && nj != 0u && w.cluster.jointListsValid;
	clClear(w, nj, keepJointLists);
	if (refresh)
	{
		clAssignByPhase(w, numPairs, nj, withJoints, leftList);
		w.cluster.chunkJointVersion = w.jointVersion; w.cluster.chunkWithJoints = withJoints;
	}
	else clAssignCached(w, numPairs, nj, withJoints, keepJointLists, leftList);
	if (leftList) clAssignComponents(w);
	clOffsetsAndScatter(w, numPairs, nj, keepJointLists);
	cluster_color_launch(w, nj);
}
