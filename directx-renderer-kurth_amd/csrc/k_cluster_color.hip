// Cluster sweep, second stage: one workgroup per task builds the task's local body table, colours its contacts and writes the task
// header and the contact schedule the sweep (k_cluster_solve.hip) runs.  cluster.h explains the clusters, the phases and the hand-over.
#include "cluster.h"

#define CL_LANES 1024u                    // k_cl_color
#define CL_TASK_MAX_MANIFOLDS 2048u       // hard limits of k_cl_color's LDS tables (a task normally holds <= taskManifolds + one body's degree)
#define CL_TASK_MAX_BODIES 4095u
#define CL_HASH_SIZE 8192u                // largest body hash; a task uses clHashSize(manifolds + joints) slots of it
#define CL_KEY_HIST_WORDS 264u            // k_cl_color's histogram of the manifold keys colour * 4 + (4 - count): (CL_SERIAL_COLOR + 1) * 4 = 260 keys, in whole rows of 8 words
static_assert(CL_KEY_HIST_WORDS >= (CL_SERIAL_COLOR + 1u) * 4u && CL_KEY_HIST_WORDS % 8u == 0u, "one histogram word per (colour or serial tail, contact count)");
#define CL_TRACE_ROW_COLOR 14u            // developer timeline (mi_debug_flow_trace): the row of a task's CL_TRACE_ROWS that k_cl_color stamps (k_cl_solve documents the others)
static_assert(CL_TRACE_ROW_COLOR < CL_TRACE_ROWS, "k_cl_color's row lies inside the task's trace rows");

// Bid of a manifold for its bodies in a colouring round: lowest wins.  Manifolds with more contacts bid lower, so they are coloured
// first and gather in the low colours: a colour's sweep time is that of its longest manifold, and this keeps the 2-4-contact ones
// (20 % of a mixed pile) out of most colours.  Then a pseudo-random priority (hash of the narrowphase slot and the round), then
// the position inside the task, which makes the bid unique.
MI_DEV u32 clBid(u32 slot, u32 count, u32 round, u32 i) { return (((4u - count) & 3u) << 22) | ((clHash(slot * 2654435761u + round) & 0x3FFu) << 12) | (i & 0xFFFu); } // 24 bits

// Slots of a task's body hash: a power of two with at most every second slot taken (a manifold or joint brings two bodies at most), and
// whole waves in the sweeps over it.  A task of 450 bodies clears and sweeps 4096 slots instead of all 8192.
MI_DEV u32 clHashSize(u32 items) { u32 hs = 64u; while (hs < 4u * items && hs < CL_HASH_SIZE) hs <<= 1; return hs; }
static_assert(2u * (CL_TASK_MAX_MANIFOLDS + CL_TASK_MAX_JOINTS) < CL_HASH_SIZE, "the largest task's bodies leave free slots in the largest hash");
// Insert body g: whoever takes the slot fetches the body's phase mask and parks "shared" (touched in more than one phase) beside
// the key, so that the sweep that hands out the local indices reads LDS only.
MI_DEV void clHashInsert(u32* hKey, u32* hVal, u32 hashMask, u32 g, const u32* __restrict__ phaseMask)
{
	u32 h = clHash(g) & hashMask;
	for (;;)
	{
		u32 old = atomicCAS(&hKey[h], 0u, g + 1u);
		if (old == 0u) { hVal[h] = __popc(phaseMask[g]) > 1 ? 1u : 0u; break; }
		if (old == g + 1u) break;
		h = (h + 1u) & hashMask;
	}
}
MI_DEV u32 clHashFind(const u32* hKey, const u32* hVal, u32 hashMask, u32 g)
{
	u32 h = clHash(g) & hashMask;
	while (hKey[h] != g + 1u) h = (h + 1u) & hashMask;
	return hVal[h];
}

// ---------------------------------------------------------------------------------------------------------------
// Per task, one workgroup: local body table, local colouring, order by (colour, 4 - contacts), task header.
//   LDS: body hash (global id -> local index), per local body a 64-bit colour mask and a claim word, per manifold its two local
//   bodies, its key and its final position.
// Colouring = the rounds of k_color_round with LDS atomics: every uncoloured manifold bids for both bodies with a pseudo-random
// priority (deterministic: hash of its narrowphase slot and the round); who holds both takes the lowest colour free on both.
// Manifolds that find no colour below 64 form the task's serial tail (one per barrier).
// Local indices: bodies touched in more than one phase ("shared") first, then the task-private ones.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CL_LANES) k_cl_color(u32* __restrict__ counters, u32 nb, const u32* __restrict__ taskStart, u32* __restrict__ pre, const uint4* __restrict__ actIds,
	const u32* __restrict__ phaseMask, ClTask* __restrict__ tasks, u32* __restrict__ bodyList, u32* __restrict__ mOrder, u32* __restrict__ mKeySorted, u32* __restrict__ mLocal, u32* __restrict__ cEntry, u32* __restrict__ sharedSlot,
	const u32* __restrict__ jointStart, const u32* __restrict__ jointList, const uint4* __restrict__ jointTable, uint2* __restrict__ taskJoints, u32* __restrict__ jointClassStart, u64* __restrict__ trace)
{
	extern __shared__ u32 clds[];
	u32* hKey = clds;                                   // [CL_HASH_SIZE] global id + 1, 0 = empty; the task's first clHashSize() slots are in use
	u32* hVal = hKey + CL_HASH_SIZE;                    // [CL_HASH_SIZE] shared or not, then the local index
	u64* mask = (u64*)(hVal + CL_HASH_SIZE);            // [CL_TASK_MAX_BODIES + 1]
	u32* claim = (u32*)(mask + CL_TASK_MAX_BODIES + 1); // [CL_TASK_MAX_BODIES + 1]
	u32* mAB = claim + CL_TASK_MAX_BODIES + 1;          // [CL_TASK_MAX_MANIFOLDS] la | lb << 16
	u32* mKey = mAB + CL_TASK_MAX_MANIFOLDS;            // [..] colour * 4 + (4 - count); UNCOLORED while colouring
	u32* mPos = mKey + CL_TASK_MAX_MANIFOLDS;           // [..] final position
	u32* mCnt = mPos + CL_TASK_MAX_MANIFOLDS;           // [..] contact count by final position, then its exclusive scan of (count - 1)
	u32* mSlot = mCnt + CL_TASK_MAX_MANIFOLDS;          // [..] narrowphase slot | contacts << 28 (the colouring rounds' priorities hash it)
	u32* hist = mSlot + CL_TASK_MAX_MANIFOLDS;          // [CL_KEY_HIST_WORDS] per key, then cursors
	u32* jHist = hist + CL_KEY_HIST_WORDS;              // [CL_MAX_JOINT_CLASSES + 1] joints per (type, colour) class, then cursors
	u32* cHist = jHist + CL_MAX_JOINT_CLASSES + 1;      // [CL_SERIAL_COLOR + 2] contacts per colour (64 = the serial tail), then first positions, then cursors
	__shared__ u32 sNumShared, sNumPrivate, sMaxColor, sScan[16], sSharedBase;
	const u32 tid = threadIdx.x;
	// developer timeline (mi_debug_flow_trace): row CL_TRACE_ROW_COLOR of the task's CL_TRACE_ROWS rows = core-clock stamps of the stages below, [15] = colouring rounds
#define CL_STAMP(I_) if (trace && tid == 0 && key < CL_MAX_TASKS) trace[((size_t)key * CL_TRACE_ROWS + CL_TRACE_ROW_COLOR) * CL_TRACE_WORDS + (I_)] = clock64();

	// Task t of phase p is built by workgroup (tasks of the earlier phases + t) % G — the rotation the solve launch uses — so that
	// the later phases' tasks go to the workgroups the first phase left idle first, and nobody builds more than
	// ceil(tasks / G) + 1 of them (by key order workgroup 0 built one task of EVERY phase: 4 x 35 us on the kernel's critical path).
	for (u32 ph = 0; ph < CL_MAX_PHASES; ++ph)
	{
	const u32 tasksInPhase = counters[CTR_CL_NUM_TASKS + ph];
	const u32 tFirst = (blockIdx.x + gridDim.x - (clPhaseOffset(counters, ph) % gridDim.x)) % gridDim.x;
	for (u32 key = ph * CL_MAX_TASKS + tFirst; key < ph * CL_MAX_TASKS + min(tasksInPhase, CL_MAX_TASKS); key += gridDim.x)
	{
		u32 first = taskStart[key * CL_SUBCOUNTERS], n = taskStart[(key + 1u) * CL_SUBCOUNTERS] - first;
		ClTask* T = tasks + key;
		// joints of the task (phase 0 only: an island lives in one phase-0 task)
		const u32 jFirst = (jointStart && key < CL_MAX_TASKS) ? jointStart[key] : 0u, nj = (jointStart && key < CL_MAX_TASKS) ? jointStart[key + 1u] - jFirst : 0u;
		if (jointStart && key < CL_MAX_TASKS && tid <= CL_MAX_JOINT_CLASSES) jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + tid] = 0u; // (no joints: all classes empty)
		if (jointStart && key < CL_MAX_TASKS && tid == 0) jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + CL_MAX_JOINT_CLASSES + 1u] = jFirst;
		if (!n && !nj) { if (tid == 0) { T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } continue; }
		if (n > CL_TASK_MAX_MANIFOLDS || nj > CL_TASK_MAX_JOINTS) { if (tid == 0) { atomicOr(&counters[CTR_CL_STATUS], 2u); T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } continue; }
		u32 phase = key / CL_MAX_TASKS;
		const u32 hashSize = clHashSize(n + nj), hashMask = hashSize - 1u; // (this task's: the one before may have used more or fewer slots)
		for (u32 h = tid; h < hashSize; h += CL_LANES) hKey[h] = 0;
		for (u32 h = tid; h < CL_KEY_HIST_WORDS + CL_MAX_JOINT_CLASSES + 1u + CL_SERIAL_COLOR + 2u; h += CL_LANES) hist[h] = 0;
		if (tid == 0) { sNumShared = 0; sNumPrivate = 0; sMaxColor = 0; }
		__syncthreads();
		CL_STAMP(0)
		// 1. distinct dynamic bodies
		// (the manifold's ids are fetched once, through two dependent global loads, and parked in LDS for the sort and step 2)
		for (u32 i = tid; i < n; i += CL_LANES)
		{
			u32 pi = pre[first + i];
			uint4 ids = actIds[pi];
			mKey[i] = ids.x; mCnt[i] = ids.y; mAB[i] = pi; mSlot[i] = (ids.w & 0x0FFFFFFFu) | (ids.z << 28);
			for (u32 e = 0; e < 2; ++e)
			{
				u32 g = e ? ids.y : ids.x;
				if (g >= nb) continue;
				clHashInsert(hKey, hVal, hashMask, g, phaseMask);
			}
		}
		for (u32 i = tid; i < nj; i += CL_LANES) // the joints' bodies: a limb in the air has joints and no contact
		{
			uint4 e4 = jointTable[jointList[jFirst + i]];
			for (u32 e = 0; e < 2; ++e)
			{
				u32 g = e ? e4.w : e4.z;
				if (g >= nb) continue;
				clHashInsert(hKey, hVal, hashMask, g, phaseMask);
			}
		}
		__syncthreads();
		for (u32 h = tid; h < hashSize; h += CL_LANES) // (hashSize is a multiple of 64: the ballots below see whole waves)
		{
			// local index = running count of the shared / private bodies: one LDS atomic per wave, not per body (same-address LDS
			// atomics are served one lane at a time)
			const bool has = hKey[h] != 0u;
			const bool shared = has && hVal[h] != 0u;
			const u64 bs = __ballot(shared), bp = __ballot(has && !shared);
			const u32 lane = tid & 63u;
			u32 baseS = 0, baseP = 0;
			if (lane == 0u) { if (bs) baseS = atomicAdd(&sNumShared, (u32)__popcll(bs)); if (bp) baseP = atomicAdd(&sNumPrivate, (u32)__popcll(bp)); }
			baseS = __shfl(baseS, 0); baseP = __shfl(baseP, 0);
			const u64 below = (1ull << lane) - 1ull;
			if (has) hVal[h] = shared ? ((baseS + (u32)__popcll(bs & below)) | 0x80000000u) : baseP + (u32)__popcll(bp & below);
		}
		__syncthreads();
		const u32 numShared = sNumShared, numBodies = sNumShared + sNumPrivate;
		const bool tooMany = numBodies > CL_TASK_MAX_BODIES; // uniform
		if (tooMany) { if (tid == 0) { atomicOr(&counters[CTR_CL_STATUS], 2u); T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } __syncthreads(); continue; }
		// The task's shared bodies get a contiguous run of hand-over records (32 B each): its lanes publish them with coalesced stores, and
		// whoever uses a body next finds the record through sharedSlot[phase][body].  (The placement of the run depends on the order the
		// tasks get here; results do not.)
		if (tid == 0) sSharedBase = atomicAdd(&counters[CTR_CL_SHARED], numShared);
		__syncthreads();
		const u32 sharedBase = sSharedBase;
		for (u32 h = tid; h < hashSize; h += CL_LANES)
			if (hKey[h])
			{
				u32 v = hVal[h];
				u32 l = (v & 0x80000000u) ? (v & 0x7FFFFFFFu) : numShared + v;
				hVal[h] = l;
				bodyList[(size_t)key * CL_BODY_STRIDE + l] = hKey[h] - 1u;
				if (l < numShared) sharedSlot[(size_t)phase * (nb + 1u) + (hKey[h] - 1u)] = sharedBase + l;
			}
		for (u32 l = tid; l <= numBodies; l += CL_LANES) { mask[l] = 0ull; claim[l] = 0xFFFFFFFFu; }
		__syncthreads();
		CL_STAMP(1)
		// 1b. The task's manifolds arrive in the order their append atomics landed.  The colouring below breaks bid ties by position, so
		// the positions are made a function of the inputs first: bitonic sort by {contact count, narrowphase slot} (unique per
		// manifold).  With that the whole schedule, and so every result, repeats from run to run (snapshot / restore continue
		// bit-identically).  Stages that exchange inside 128 consecutive elements stay inside one wave and need no workgroup barrier.
		{
			u32 m = 128u; while (m < n) m <<= 1;
			// one 64-bit word per element {key, arrival index} (a stage is then one LDS round trip: two reads, compare, two writes);
			// the words live in the colour-mask table, which the rounds need zeroed only afterwards
			u64* sk = mask;
			static_assert(CL_TASK_MAX_BODIES + 1u >= CL_TASK_MAX_MANIFOLDS, "the colour masks double as the sort's scratch");
			for (u32 i = tid; i < m; i += CL_LANES) sk[i] = ((u64)(i < n ? mSlot[i] : 0xFFFFFFFFu) << 32) | i;
			__syncthreads();
			for (u32 k = 2u; k <= m; k <<= 1)
				for (u32 j = k >> 1, lj = 31u - (u32)__clz(k >> 1); j > 0u; j >>= 1, --lj) // j = 1 << lj (no integer division in the index arithmetic)
				{
					if (tid < (m >> 1))
					{
						u32 a = ((tid >> lj) << (lj + 1u)) + (tid & (j - 1u)), b = a + j;
						bool up = (a & k) == 0u;
						u64 ka = sk[a], kb = sk[b];
						if ((ka > kb) == up) { sk[a] = kb; sk[b] = ka; }
					}
					if (j > 64u || (j == 1u && k >= 128u)) __syncthreads(); // the next stage (j / 2, or the next k's first) crosses the waves' 128-element blocks
					else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				}
			__syncthreads();
			for (u32 i = tid; i < n; i += CL_LANES) { u64 e = sk[i]; mSlot[i] = (u32)(e >> 32); mPos[i] = (u32)e; }
			__syncthreads();
			for (u32 l = tid; l <= numBodies; l += CL_LANES) mask[l] = 0ull;
			for (u32 i = tid; i < m; i += CL_LANES) mask[i] = 0ull; // (the scratch may reach beyond the bodies)
		}
		CL_STAMP(2)
		// 2. local ids of every manifold, in the sorted order (n <= 2 * CL_LANES: two per lane, gathered before anything is overwritten)
		{
			static_assert(CL_TASK_MAX_MANIFOLDS <= 2u * CL_LANES, "two manifolds per lane");
			u32 gx[2], gy[2], gp[2];
			for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * CL_LANES; if (i < n) { u32 o = mPos[i]; gx[r] = mKey[o]; gy[r] = mCnt[o]; gp[r] = mAB[o]; } }
			__syncthreads();
			for (u32 r = 0; r < 2u; ++r)
			{
				u32 i = tid + r * CL_LANES;
				if (i >= n) continue;
				u32 loc[2];
				for (u32 e = 0; e < 2; ++e)
				{
					u32 g = e ? gy[r] : gx[r];
					loc[e] = CL_LOCAL_STATIC;
					if (g >= nb) continue;
					loc[e] = clHashFind(hKey, hVal, hashMask, g);
				}
				mAB[i] = loc[0] | (loc[1] << 16);
				mKey[i] = 0xFFFFFFFFu;
				pre[first + i] = gp[r]; // (read again when the final order is written out)
			}
		}
		__syncthreads();
		// 2b. the joints: local ids of their bodies, ordered by (type, colour) class (counting sort: class sizes, offsets, cursors)
		if (nj)
		{
			for (u32 i = tid; i < nj; i += CL_LANES) atomicAdd(&jHist[min(jointTable[jointList[jFirst + i]].x >> 8, CL_MAX_JOINT_CLASSES - 1u)], 1u);
			__syncthreads();
			if (tid == 0)
			{
				u32 run = 0;
				for (u32 c = 0; c < CL_MAX_JOINT_CLASSES; ++c) { u32 v = jHist[c]; jHist[c] = run; jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + c] = run; run += v; }
				jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + CL_MAX_JOINT_CLASSES] = run;
			}
			__syncthreads();
			for (u32 i = tid; i < nj; i += CL_LANES)
			{
				u32 ji = jointList[jFirst + i];
				uint4 e4 = jointTable[ji];
				u32 loc[2];
				for (u32 e = 0; e < 2; ++e)
				{
					u32 g = e ? e4.w : e4.z;
					loc[e] = CL_LOCAL_STATIC;
					if (g >= nb) continue;
					loc[e] = clHashFind(hKey, hVal, hashMask, g);
				}
				u32 p = atomicAdd(&jHist[min(e4.x >> 8, CL_MAX_JOINT_CLASSES - 1u)], 1u); // (order inside a class is free: its joints share no body)
				taskJoints[jFirst + p] = make_uint2(ji, loc[0] | (loc[1] << 16));
			}
			__syncthreads();
		}
		CL_STAMP(3)
		// 3. colouring rounds.  A claim word holds {round, inverted bid}: a later round's bid beats any earlier one under atomicMax, so
		// the claims need no clearing between rounds: two barriers per round (bid | decide; the second one also tells whether anybody
		// is left).  No shared counters inside the rounds: a same-address LDS atomic from every lane costs more than the round itself.
		for (u32 l = tid; l < numBodies; l += CL_LANES) claim[l] = 0u;
		__syncthreads();
		// (a lane keeps its two manifolds' slot word, local body ids and colour in registers over the rounds: what it reads from LDS
		// in a round is the claims and the colour masks only)
		u32 rSlot[2], rAB[2], rKey[2];
		for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * CL_LANES; rKey[r] = 0u; rSlot[r] = 0u; rAB[r] = 0u; if (i < n) { rSlot[r] = mSlot[i]; rAB[r] = mAB[i]; rKey[r] = 0xFFFFFFFFu; } }
		for (u32 round = 0; ; ++round)
		{
			const bool lastRound = round >= 254u; // (the round tag has 8 bits: whoever is still uncoloured then goes to the serial tail)
			u32 bid[2];
			for (u32 r = 0; r < 2u; ++r)
			{
				if (rKey[r] != 0xFFFFFFFFu) continue;
				u32 sc = rSlot[r];
				bid[r] = ((round + 1u) << 24) | (0xFFFFFFu - clBid(sc & 0x0FFFFFFFu, sc >> 28, round, tid + r * CL_LANES));
				u32 la = rAB[r] & 0xFFFFu, lb = rAB[r] >> 16;
				if (la != CL_LOCAL_STATIC) atomicMax(&claim[la], bid[r]);
				if (lb != CL_LOCAL_STATIC) atomicMax(&claim[lb], bid[r]);
			}
			__syncthreads();
			u32 left = 0;
			for (u32 r = 0; r < 2u; ++r)
			{
				if (rKey[r] != 0xFFFFFFFFu) continue;
				u32 cnt = rSlot[r] >> 28;
				u32 la = rAB[r] & 0xFFFFu, lb = rAB[r] >> 16;
				bool won = (la == CL_LOCAL_STATIC || claim[la] == bid[r]) && (lb == CL_LOCAL_STATIC || claim[lb] == bid[r]);
				if (!won && !lastRound) { ++left; continue; }
				// A manifold of cnt contacts takes cnt CONSECUTIVE colours [c, c + cnt) on both bodies (the sweep's step is one contact row:
				// its contacts run in colours c, c + 1, ...), the lowest such run free on both: manifolds that share a body get disjoint
				// runs, so "by first colour" is still a sequential order of whole manifolds (what the schedule export reports).
				u64 used = (la != CL_LOCAL_STATIC ? mask[la] : 0ull) | (lb != CL_LOCAL_STATIC ? mask[lb] : 0ull);
				u64 fr = ~used;
				if (cnt > 1u) fr &= fr >> 1;
				if (cnt > 2u) fr &= fr >> 1;
				if (cnt > 3u) fr &= fr >> 1; // bit c set = colours c .. c + cnt - 1 all free (the shifts bring zeros in at the top: a run never passes colour 63)
				u32 c = (won && fr) ? (u32)__ffsll((long long)fr) - 1u : CL_SERIAL_COLOR;
				if (c < CL_SERIAL_COLOR)
				{
					const u64 run = ((cnt >= 64u ? 0ull : (1ull << cnt)) - 1ull) << c;
					if (la != CL_LOCAL_STATIC) mask[la] |= run; // the only winner on this body in this round
					if (lb != CL_LOCAL_STATIC) mask[lb] |= run;
				}
				rKey[r] = c * 4u + (4u - cnt);
			}
			if (!__syncthreads_or((int)left)) { if (trace && tid == 0 && key < CL_MAX_TASKS) trace[((size_t)key * CL_TRACE_ROWS + CL_TRACE_ROW_COLOR) * CL_TRACE_WORDS + 15u] = round + 1u; break; }
		}
		for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * CL_LANES; if (i < n) mKey[i] = rKey[r]; }
		__syncthreads();
		CL_STAMP(4)
		// 4. manifold order by key = (first colour, contact count): histogram, scan by one wave, cursors.  This is the order the rows are
		// initialised in and the schedule export reports (manifold after manifold; manifolds that share a body have disjoint colour runs).
		for (u32 i = tid; i < n; i += CL_LANES)
		{
			const u32 k = mKey[i], c = k >> 2, cnt = 4u - (k & 3u);
			atomicAdd(&hist[k], 1u);
			// ... and the CONTACT histogram per colour (contact q of a manifold runs in colour c + q; the serial tail is class 64)
			if (c < CL_SERIAL_COLOR) { for (u32 q = 0; q < cnt; ++q) atomicAdd(&cHist[c + q], 1u); }
			else atomicAdd(&cHist[CL_SERIAL_COLOR], cnt);
		}
		__syncthreads();
		if (tid < 64u) // 260 keys, 5 per lane (65 colours x 4 counts): serial scan over 64 lanes
		{
			u32 base = tid * 5u, s = 0;
			u32 v[5];
			for (u32 k = 0; k < 5u; ++k) { v[k] = (base + k < 260u) ? hist[base + k] : 0u; s += v[k]; }
			u32 incl = s;
			for (int o = 1; o < 64; o <<= 1) { u32 up = __shfl_up(incl, o); if ((int)tid >= o) incl += up; }
			u32 run = incl - s;
			for (u32 k = 0; k < 5u; ++k) { if (base + k < 260u) hist[base + k] = run; run += v[k]; }
			// contacts per colour -> first contact position of every colour (lane = colour); number of colours in use
			const u32 cc = cHist[tid];
			u32 ci = cc;
			for (int o = 1; o < 64; o <<= 1) { u32 up = __shfl_up(ci, o); if ((int)tid >= o) ci += up; }
			const u32 coloured = (u32)__shfl(ci, 63), serial = cHist[CL_SERIAL_COLOR];
			u32 top = cc ? tid + 1u : 0u;
			for (int o = 32; o > 0; o >>= 1) top = max(top, (u32)__shfl_xor(top, o));
			cHist[tid] = ci - cc;
			if (tid == 0) { cHist[CL_SERIAL_COLOR] = coloured; cHist[CL_SERIAL_COLOR + 1u] = coloured + serial; sMaxColor = top; }
		}
		__syncthreads();
		const u32 numColors = sMaxColor, numContacts = cHist[CL_SERIAL_COLOR + 1u], serialStartC = cHist[CL_SERIAL_COLOR];
		if (tid <= CL_SERIAL_COLOR + 1u) T->colorStart[tid] = cHist[tid];
		if (tid == 0)
		{
			T->first = first; T->count = n; T->numBodies = numBodies; T->numShared = numShared; T->numColors = numColors; T->serialStart = serialStartC; T->numRows = numContacts;
			atomicMax(&counters[CTR_NUM_COLORS], numColors + (serialStartC < numContacts ? 1u : 0u));
			T->sharedBase = sharedBase;
			atomicAdd(&counters[CTR_CL_PHASE_COUNT + phase], n);
		}
		__syncthreads();
		// Positions inside a (colour, count) class: an atomic cursor (order inside a class is free, its manifolds share no body: the
		// RESULTS repeat from run to run, the memory order need not).
		// The serial tail IS order-dependent: its positions follow the (sorted) index.
		for (u32 i = tid; i < n; i += CL_LANES)
		{
			u32 k = mKey[i], p;
			if ((k >> 2) < CL_SERIAL_COLOR) p = atomicAdd(&hist[k], 1u);
			else { p = hist[k]; for (u32 j = 0; j < i; ++j) p += (mKey[j] == k) ? 1u : 0u; } // (rare: a body with more than 64 contacts in one task)
			mPos[i] = p;
		}
		__syncthreads();
		CL_STAMP(5)
		// 5. the contact schedule: contact q of a manifold of first colour c gets a position inside colour c + q (cursor: free order
		// inside a colour); the serial tail's contacts follow in manifold position order, a manifold's contacts in order.
		// Entry = manifold position inside the task | q << 12.
		for (u32 i = tid; i < n; i += CL_LANES)
		{
			const u32 k = mKey[i], c = k >> 2, cnt = 4u - (k & 3u), mp = mPos[i];
			if (c < CL_SERIAL_COLOR) { for (u32 q = 0; q < cnt; ++q) cEntry[(size_t)4u * first + atomicAdd(&cHist[c + q], 1u)] = mp | (q << 12); }
			else
			{
				u32 p = serialStartC;
				for (u32 j = 0; j < n; ++j) if ((mKey[j] >> 2) >= CL_SERIAL_COLOR && mPos[j] < mp) p += 4u - (mKey[j] & 3u);
				for (u32 q = 0; q < cnt; ++q) cEntry[(size_t)4u * first + p + q] = mp | (q << 12);
			}
		}
		CL_STAMP(6)
		for (u32 i = tid; i < n; i += CL_LANES)
		{
			u32 p = mPos[i];
			mOrder[first + p] = pre[first + i];
			mKeySorted[first + p] = mKey[i];
			mLocal[first + p] = mAB[i];
		}
		__syncthreads();
		CL_STAMP(7)
	}
	}
#undef CL_STAMP
}

// ---------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------
static size_t clColorLdsBytes()
{
	return sizeof(u32) * (2 * CL_HASH_SIZE + (CL_TASK_MAX_BODIES + 1) + 5 * CL_TASK_MAX_MANIFOLDS + CL_KEY_HIST_WORDS + CL_MAX_JOINT_CLASSES + 1 + CL_SERIAL_COLOR + 2) + sizeof(u64) * (CL_TASK_MAX_BODIES + 1);
}

bool cluster_color_setup()
{
	return hipFuncSetAttribute((const void*)k_cl_color, hipFuncAttributeMaxDynamicSharedMemorySize, (int)clColorLdsBytes()) == hipSuccess;
}

// Colours the tasks k_cl_offsets / k_cl_scatter laid out; one workgroup per workgroup of the solve launch (the same task rotation).
void cluster_color_launch(World& w, u32 nj)
{
	hipLaunchKernelGGL(k_cl_color, dim3(w.cluster.blocks), dim3(CL_LANES), clColorLdsBytes(), w.stream, w.dCounters.p, w.nb, w.cluster.taskStart.p, w.cluster.pre.p, w.actIds.p,
		w.cluster.phaseMask.p, (ClTask*)w.cluster.tasks.p, w.cluster.bodyList.p, w.mOrder.p, w.mKeySorted.p, w.cluster.local.p, w.cluster.entry.p, w.cluster.sharedSlot.p,
		nj ? w.cluster.jointStart.p : (const u32*)nullptr, w.cluster.jointList.p, w.cluster.jointTable.p, w.cluster.taskJoints.p, w.cluster.jointClassStart.p, w.cluster.flowTrace.p);
}
