// Cluster sweep, second stage: one workgroup per task builds the task's local body table, colours its contacts and writes the task
// header and the contact schedule the sweep (k_cluster_solve.hip) runs.  cluster.h explains the clusters, the phases and the hand-over.
#include "cluster.h"

#define CL_LANES 1024u                    // k_cl_color
#define CL_TASK_MAX_MANIFOLDS 2048u       // hard limits of k_cl_color's LDS tables (a task normally holds <= taskManifolds + one body's degree)
#define CL_TASK_MAX_BODIES 4095u
#define CL_HASH_SIZE 8192u                // largest body hash; a task uses clHashSize(manifolds + joints) slots of it
#define CL_KEY_HIST_WORDS 264u            // k_cl_color's histogram of the manifold keys colour * 4 + (4 - count): (CL_SERIAL_COLOR + 1) * 4 = 260 keys, in whole rows of 8 words
// The narrow instance (two workgroups per compute unit): tasks of at most CLN_MAX_ITEMS manifolds + joints
#define CLN_LANES 640u
#define CLN_MAX_ITEMS 1280u                 // (the first phase cuts tasks of ~1000 manifolds, which a growing pile overshoots between two re-cuts: profiles/color_tasks.txt)
#define CLN_MAX_MANIFOLDS CLN_MAX_ITEMS
#define CLN_MAX_BODIES (2u * CLN_MAX_ITEMS) // a manifold or joint brings two bodies at most
#define CLN_HASH_SIZE 4096u                 // up to 1024 items both instances pick the same hash size; beyond, this one fills its hash further (2560 bodies at the very most; ~0.8 per item in a pile).  Local indices reach no result.
static_assert(CLN_MAX_BODIES < CLN_HASH_SIZE, "the largest task's bodies leave free slots in the hash");
static_assert(CLN_HASH_SIZE <= CL_HASH_SIZE && CLN_MAX_MANIFOLDS <= CL_TASK_MAX_MANIFOLDS && CLN_MAX_BODIES <= CL_TASK_MAX_BODIES, "whatever the narrow instance takes the wide one could");
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
template<u32 HASH> MI_DEV u32 clHashSize(u32 items) { u32 hs = 64u; while (hs < 4u * items && hs < HASH) hs <<= 1; return hs; }
static_assert(2u * (CL_TASK_MAX_MANIFOLDS + CL_TASK_MAX_JOINTS) < CL_HASH_SIZE, "the largest task's bodies leave free slots in the largest hash");
// Insert body g: whoever takes the slot fetches the body's phase mask and parks "shared" (touched in more than one phase) beside
// the key, so that the sweep that hands out the local indices reads LDS only.
template<typename HV> MI_DEV void clHashInsert(u32* hKey, HV* hVal, u32 hashMask, u32 g, const u32* __restrict__ phaseMask)
{
	u32 h = clHash(g) & hashMask;
	for (;;)
	{
		u32 old = atomicCAS(&hKey[h], 0u, g + 1u);
		if (old == 0u) { hVal[h] = (HV)(__popc(phaseMask[g]) > 1 ? 1u : 0u); break; }
		if (old == g + 1u) break;
		h = (h + 1u) & hashMask;
	}
}
template<typename HV> MI_DEV u32 clHashFind(const u32* hKey, const HV* hVal, u32 hashMask, u32 g)
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
//
// The kernel is a template over its lane count and table sizes, with two instances.  The NARROW one (640 lanes, tables for tasks of at
// most CLN_MAX_ITEMS manifolds + joints, half the LDS) is launched with two workgroups resident per compute unit and gives every
// task a workgroup of its own, so the launch takes about as long as its slowest task however many tasks there are.  The WIDE one
// (1024 lanes, the largest tables) follows on the same stream with the solve launch's rotation and colours only the tasks the
// narrow tables cannot hold; with none (k_cl_offsets counts them) its workgroups read one word and leave.  Everything that reaches
// a result — sort keys, bids, colour runs, key order — is the same expression in both: where a task is coloured changes nothing.
// ---------------------------------------------------------------------------------------------------------------
struct ClColorArgs
{
	u32* counters; u32 nb, narrowLimit; const u32* taskStart; u32* pre; const uint4* actIds; const u32* phaseMask; ClTask* tasks; u32* bodyList; u32* mOrder; u32* mKeySorted; u32* mLocal; u32* cEntry; u32* sharedSlot;
	const u32* jointStart; const u32* jointList; const uint4* jointTable; uint2* taskJoints; u32* jointClassStart; u64* trace;
};

// HV: a hash slot's value (local body index, top bit = shared while the indices are handed out), MP: a manifold's position inside its task.
template<bool NARROW, u32 LANES, u32 HASH, u32 MAX_BODIES, u32 MAX_MANIFOLDS, typename HV, typename MP>
MI_DEV void clColorTask(const ClColorArgs& A, const u32 key)
{
	u32* const counters = A.counters; const u32 nb = A.nb; const u32* __restrict__ const taskStart = A.taskStart; u32* __restrict__ const pre = A.pre; const uint4* __restrict__ const actIds = A.actIds;
	const u32* __restrict__ const phaseMask = A.phaseMask; ClTask* __restrict__ const tasks = A.tasks; u32* __restrict__ const bodyList = A.bodyList; u32* __restrict__ const mOrder = A.mOrder; u32* __restrict__ const mKeySorted = A.mKeySorted;
	u32* __restrict__ const mLocal = A.mLocal; u32* __restrict__ const cEntry = A.cEntry; u32* __restrict__ const sharedSlot = A.sharedSlot; const u32* __restrict__ const jointStart = A.jointStart; const u32* __restrict__ const jointList = A.jointList;
	const uint4* __restrict__ const jointTable = A.jointTable; uint2* __restrict__ const taskJoints = A.taskJoints; u32* __restrict__ const jointClassStart = A.jointClassStart; u64* __restrict__ const trace = A.trace;
	extern __shared__ u32 clds[];
	u32* hKey = clds;                                   // [HASH] global id + 1, 0 = empty; the task's first clHashSize() slots are in use
	HV* hVal = (HV*)(hKey + HASH);                      // [HASH] shared or not, then the local index
	constexpr u32 HV_SHARED = 1u << (8u * (u32)sizeof(HV) - 1u);
	static_assert(MAX_BODIES < HV_SHARED && MAX_MANIFOLDS <= (1ull << (8u * sizeof(MP))) && (HASH * sizeof(HV)) % 8u == 0u, "local indices and positions fit their words; the colour masks stay 8-byte aligned");
	u64* mask = (u64*)(hVal + HASH);                    // [MAX_BODIES + 1]
	u32* claim = (u32*)(mask + MAX_BODIES + 1);         // [MAX_BODIES + 1]
	u32* mAB = claim + MAX_BODIES + 1;                  // [MAX_MANIFOLDS] la | lb << 16
	u32* mKey = mAB + MAX_MANIFOLDS;                    // [..] colour * 4 + (4 - count); UNCOLORED while colouring
	u32* mCnt = mKey + MAX_MANIFOLDS;                   // [..] contact count by final position, then its exclusive scan of (count - 1)
	u32* mSlot = mCnt + MAX_MANIFOLDS;                  // [..] narrowphase slot | contacts << 28 (the colouring rounds' priorities hash it)
	u32* hist = mSlot + MAX_MANIFOLDS;                  // [CL_KEY_HIST_WORDS] per key, then cursors
	u32* jHist = hist + CL_KEY_HIST_WORDS;              // [CL_MAX_JOINT_CLASSES + 1] joints per (type, colour) class, then cursors
	u32* cHist = jHist + CL_MAX_JOINT_CLASSES + 1;      // [CL_SERIAL_COLOR + 2] contacts per colour (64 = the serial tail), then first positions, then cursors
	MP* mPos = (MP*)(cHist + CL_SERIAL_COLOR + 2);      // [MAX_MANIFOLDS] arrival index by sorted index, then the final position
	__shared__ u32 sNumShared, sNumPrivate, sMaxColor, sScan[16], sSharedBase;
	const u32 tid = threadIdx.x;
	// developer timeline (mi_debug_flow_trace): row CL_TRACE_ROW_COLOR of the task's CL_TRACE_ROWS rows = core-clock stamps of the stages below, [15] = colouring rounds
#define CL_STAMP(I_) if (trace && tid == 0 && key < CL_MAX_TASKS) trace[((size_t)key * CL_TRACE_ROWS + CL_TRACE_ROW_COLOR) * CL_TRACE_WORDS + (I_)] = clock64();

	u32 first = taskStart[key * CL_SUBCOUNTERS], n = taskStart[(key + 1u) * CL_SUBCOUNTERS] - first;
	ClTask* T = tasks + key;
	// joints of the task (phase 0 only: an island lives in one phase-0 task)
	const u32 jFirst = (jointStart && key < CL_MAX_TASKS) ? jointStart[key] : 0u, nj = (jointStart && key < CL_MAX_TASKS) ? jointStart[key + 1u] - jFirst : 0u;
	// Which launch colours the task: the narrow instance those of fewer than narrowLimit items, the wide one the others (two launches per step, disjoint tasks).
	if (((n + nj) < A.narrowLimit) != NARROW) return;
	if (tid == 0) atomicAdd(&counters[CTR_CL_COLOR_TASKS + (NARROW ? 1u : 2u)], 1u); // (mi_debug_color_tasks)
	if (jointStart && key < CL_MAX_TASKS && tid <= CL_MAX_JOINT_CLASSES) jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + tid] = 0u; // (no joints: all classes empty)
	if (jointStart && key < CL_MAX_TASKS && tid == 0) jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + CL_MAX_JOINT_CLASSES + 1u] = jFirst;
	if (!n && !nj) { if (tid == 0) { T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } return; }
	if (n > MAX_MANIFOLDS || nj > CL_TASK_MAX_JOINTS) { if (tid == 0) { atomicOr(&counters[CTR_CL_STATUS], 2u); T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } return; }
	u32 phase = key / CL_MAX_TASKS;
	const u32 hashSize = clHashSize<HASH>(n + nj), hashMask = hashSize - 1u; // (this task's: the one before may have used more or fewer slots)
	for (u32 h = tid; h < hashSize; h += LANES) hKey[h] = 0;
	for (u32 h = tid; h < CL_KEY_HIST_WORDS + CL_MAX_JOINT_CLASSES + 1u + CL_SERIAL_COLOR + 2u; h += LANES) hist[h] = 0;
	if (tid == 0) { sNumShared = 0; sNumPrivate = 0; sMaxColor = 0; }
	__syncthreads();
	CL_STAMP(0)
	// 1. distinct dynamic bodies
	// (the manifold's ids are fetched once, through two dependent global loads, and parked in LDS for the sort and step 2)
	for (u32 i = tid; i < n; i += LANES)
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
	for (u32 i = tid; i < nj; i += LANES) // the joints' bodies: a limb in the air has joints and no contact
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
	for (u32 h = tid; h < hashSize; h += LANES) // (hashSize is a multiple of 64: the ballots below see whole waves)
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
		if (has) hVal[h] = (HV)(shared ? ((baseS + (u32)__popcll(bs & below)) | HV_SHARED) : baseP + (u32)__popcll(bp & below));
	}
	__syncthreads();
	const u32 numShared = sNumShared, numBodies = sNumShared + sNumPrivate;
	const bool tooMany = numBodies > MAX_BODIES; // uniform
	if (tooMany) { if (tid == 0) { atomicOr(&counters[CTR_CL_STATUS], 2u); T->first = first; T->count = 0; T->numBodies = 0; T->numShared = 0; T->numColors = 0; T->serialStart = 0; T->numRows = 0; } __syncthreads(); return; }
	// The task's shared bodies get a contiguous run of hand-over records (32 B each): its lanes publish them with coalesced stores, and
	// whoever uses a body next finds the record through sharedSlot[phase][body].  (The placement of the run depends on the order the
	// tasks get here; results do not.)
	if (tid == 0) sSharedBase = atomicAdd(&counters[CTR_CL_SHARED], numShared);
	__syncthreads();
	const u32 sharedBase = sSharedBase;
	for (u32 h = tid; h < hashSize; h += LANES)
		if (hKey[h])
		{
			u32 v = hVal[h];
			u32 l = (v & HV_SHARED) ? (v & (HV_SHARED - 1u)) : numShared + v;
			hVal[h] = (HV)l;
			bodyList[(size_t)key * CL_BODY_STRIDE + l] = hKey[h] - 1u;
			if (l < numShared) sharedSlot[(size_t)phase * (nb + 1u) + (hKey[h] - 1u)] = sharedBase + l;
		}
	for (u32 l = tid; l <= numBodies; l += LANES) { mask[l] = 0ull; claim[l] = 0xFFFFFFFFu; }
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
		static_assert(MAX_BODIES + 1u >= 2u * MAX_MANIFOLDS - 1u, "the colour masks double as the sort's scratch (m < 2 n words)");
		for (u32 i = tid; i < m; i += LANES) sk[i] = ((u64)(i < n ? mSlot[i] : 0xFFFFFFFFu) << 32) | i;
		__syncthreads();
		for (u32 k = 2u; k <= m; k <<= 1)
			for (u32 j = k >> 1, lj = 31u - (u32)__clz(k >> 1); j > 0u; j >>= 1, --lj) // j = 1 << lj (no integer division in the index arithmetic)
			{
				for (u32 t = tid; t < (m >> 1); t += LANES) // (one pass, or two where m / 2 exceeds the lanes: pair t belongs to the same wave in every stage)
				{
					u32 a = ((t >> lj) << (lj + 1u)) + (t & (j - 1u)), b = a + j;
					bool up = (a & k) == 0u;
					u64 ka = sk[a], kb = sk[b];
					if ((ka > kb) == up) { sk[a] = kb; sk[b] = ka; }
				}
				if (j > 64u || (j == 1u && k >= 128u)) __syncthreads(); // the next stage (j / 2, or the next k's first) crosses the waves' 128-element blocks
				else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			}
		__syncthreads();
		for (u32 i = tid; i < n; i += LANES) { u64 e = sk[i]; mSlot[i] = (u32)(e >> 32); mPos[i] = (MP)e; }
		__syncthreads();
		for (u32 l = tid; l <= numBodies; l += LANES) mask[l] = 0ull;
		for (u32 i = tid; i < m; i += LANES) mask[i] = 0ull; // (the scratch may reach beyond the bodies)
	}
	CL_STAMP(2)
	// 2. local ids of every manifold, in the sorted order (n <= 2 * LANES: two per lane, gathered before anything is overwritten)
	{
		static_assert(MAX_MANIFOLDS <= 2u * LANES, "two manifolds per lane");
		u32 gx[2], gy[2], gp[2];
		for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * LANES; if (i < n) { u32 o = mPos[i]; gx[r] = mKey[o]; gy[r] = mCnt[o]; gp[r] = mAB[o]; } }
		__syncthreads();
		for (u32 r = 0; r < 2u; ++r)
		{
			u32 i = tid + r * LANES;
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
		for (u32 i = tid; i < nj; i += LANES) atomicAdd(&jHist[min(jointTable[jointList[jFirst + i]].x >> 8, CL_MAX_JOINT_CLASSES - 1u)], 1u);
		__syncthreads();
		if (tid == 0)
		{
			u32 run = 0;
			for (u32 c = 0; c < CL_MAX_JOINT_CLASSES; ++c) { u32 v = jHist[c]; jHist[c] = run; jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + c] = run; run += v; }
			jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + CL_MAX_JOINT_CLASSES] = run;
		}
		__syncthreads();
		for (u32 i = tid; i < nj; i += LANES)
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
	for (u32 l = tid; l < numBodies; l += LANES) claim[l] = 0u;
	__syncthreads();
	// (a lane keeps its two manifolds' slot word, local body ids and colour in registers over the rounds: what it reads from LDS
	// in a round is the claims and the colour masks only)
	u32 rSlot[2], rAB[2], rKey[2];
	for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * LANES; rKey[r] = 0u; rSlot[r] = 0u; rAB[r] = 0u; if (i < n) { rSlot[r] = mSlot[i]; rAB[r] = mAB[i]; rKey[r] = 0xFFFFFFFFu; } }
	for (u32 round = 0; ; ++round)
	{
		const bool lastRound = round >= 254u; // (the round tag has 8 bits: whoever is still uncoloured then goes to the serial tail)
		u32 bid[2];
		for (u32 r = 0; r < 2u; ++r)
		{
			if (rKey[r] != 0xFFFFFFFFu) continue;
			u32 sc = rSlot[r];
			bid[r] = ((round + 1u) << 24) | (0xFFFFFFu - clBid(sc & 0x0FFFFFFFu, sc >> 28, round, tid + r * LANES /* the manifold's sorted index */));
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
	for (u32 r = 0; r < 2u; ++r) { u32 i = tid + r * LANES; if (i < n) mKey[i] = rKey[r]; }
	__syncthreads();
	CL_STAMP(4)
	// 4. manifold order by key = (first colour, contact count): histogram, scan by one wave, cursors.  This is the order the rows are
	// initialised in and the schedule export reports (manifold after manifold; manifolds that share a body have disjoint colour runs).
	for (u32 i = tid; i < n; i += LANES)
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
	for (u32 i = tid; i < n; i += LANES)
	{
		u32 k = mKey[i], p;
		if ((k >> 2) < CL_SERIAL_COLOR) p = atomicAdd(&hist[k], 1u);
		else { p = hist[k]; for (u32 j = 0; j < i; ++j) p += (mKey[j] == k) ? 1u : 0u; } // (rare: a body with more than 64 contacts in one task)
		mPos[i] = (MP)p;
	}
	__syncthreads();
	CL_STAMP(5)
	// 5. the contact schedule: contact q of a manifold of first colour c gets a position inside colour c + q (cursor: free order
	// inside a colour); the serial tail's contacts follow in manifold position order, a manifold's contacts in order.
	// Entry = manifold position inside the task | q << 12.
	for (u32 i = tid; i < n; i += LANES)
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
	for (u32 i = tid; i < n; i += LANES)
	{
		u32 p = mPos[i];
		mOrder[first + p] = pre[first + i];
		mKeySorted[first + p] = mKey[i];
		mLocal[first + p] = mAB[i];
	}
	__syncthreads();
	CL_STAMP(7)
#undef CL_STAMP
}

// Wide instance: workgroup b colours, of the tasks its tables alone can hold, those the solve launch's rotation gives it, one after the other.
__global__ void __launch_bounds__(CL_LANES) k_cl_color(const ClColorArgs A)
{
	if (A.counters[CTR_CL_COLOR_TASKS] == 0u) return; // (k_cl_offsets: no task has narrowLimit items or more)
	// Task t of phase p is built by workgroup (tasks of the earlier phases + t) % G — the rotation the solve launch uses — so that
	// the later phases' tasks go to the workgroups the first phase left idle first, and nobody builds more than
	// ceil(tasks / G) + 1 of them (by key order workgroup 0 built one task of EVERY phase: 4 x 35 us on the kernel's critical path).
	for (u32 ph = 0; ph < CL_MAX_PHASES; ++ph)
	{
		const u32 tasksInPhase = A.counters[CTR_CL_NUM_TASKS + ph];
		const u32 tFirst = (blockIdx.x + gridDim.x - (clPhaseOffset(A.counters, ph) % gridDim.x)) % gridDim.x;
		for (u32 key = ph * CL_MAX_TASKS + tFirst; key < ph * CL_MAX_TASKS + min(tasksInPhase, CL_MAX_TASKS); key += gridDim.x)
			clColorTask<false, CL_LANES, CL_HASH_SIZE, CL_TASK_MAX_BODIES, CL_TASK_MAX_MANIFOLDS, u32, u32>(A, key);
	}
}

// Narrow instance: the tasks of all phases in one phase-major sequence (the big first-phase tasks are dispatched first), workgroup b
// takes b, b + G, ...: with two workgroups resident per compute unit, one task each on this part's 256 compute units up to 512 tasks.
__global__ void __launch_bounds__(CLN_LANES, 6 /* waves per SIMD: two workgroups of 10 waves per compute unit, however they fall on its four SIMDs */) k_cl_color_narrow(const ClColorArgs A)
{
	u32 phaseEnd[CL_MAX_PHASES], total = 0;
	for (u32 ph = 0; ph < CL_MAX_PHASES; ++ph) { total += min(A.counters[CTR_CL_NUM_TASKS + ph], CL_MAX_TASKS); phaseEnd[ph] = total; }
	for (u32 flat = blockIdx.x; flat < total; flat += gridDim.x)
	{
		u32 ph = 0, before = 0;
		while (flat >= phaseEnd[ph]) before = phaseEnd[ph++]; // (flat < total = phaseEnd[CL_MAX_PHASES - 1]: ph stays inside the table)
		clColorTask<true, CLN_LANES, CLN_HASH_SIZE, CLN_MAX_BODIES, CLN_MAX_MANIFOLDS, uint16_t, uint16_t>(A, ph * CL_MAX_TASKS + (flat - before));
	}
}

// ---------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------
template<u32 HASH, u32 MAX_BODIES, u32 MAX_MANIFOLDS, typename HV, typename MP> constexpr size_t clColorLdsBytes() // clColorTask's tables
{
	return sizeof(u32) * (HASH + (MAX_BODIES + 1) + 4 * MAX_MANIFOLDS + CL_KEY_HIST_WORDS + CL_MAX_JOINT_CLASSES + 1 + CL_SERIAL_COLOR + 2) + sizeof(HV) * HASH + sizeof(MP) * MAX_MANIFOLDS + sizeof(u64) * (MAX_BODIES + 1);
}
static constexpr size_t CL_WIDE_LDS = clColorLdsBytes<CL_HASH_SIZE, CL_TASK_MAX_BODIES, CL_TASK_MAX_MANIFOLDS, u32, u32>(), CL_NARROW_LDS = clColorLdsBytes<CLN_HASH_SIZE, CLN_MAX_BODIES, CLN_MAX_MANIFOLDS, uint16_t, uint16_t>();
static_assert(2 * (CL_NARROW_LDS + 512) <= 160 * 1024, "two narrow workgroups share a compute unit's 160 KB of LDS");

// Sets both instances' dynamic-LDS attribute (false = the device refuses the wide one: no cluster sweep) and sizes the narrow launch:
// it is used only where two of its workgroups are resident per compute unit; otherwise every task goes through the wide kernel.
bool cluster_color_setup(World& w, u32 computeUnits)
{
	if (hipFuncSetAttribute((const void*)k_cl_color, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CL_WIDE_LDS) != hipSuccess) return false;
	int resident = 0;
	if (hipFuncSetAttribute((const void*)k_cl_color_narrow, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CL_NARROW_LDS) != hipSuccess
		|| hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, (const void*)k_cl_color_narrow, (int)CLN_LANES, CL_NARROW_LDS) != hipSuccess) { (void)hipGetLastError(); resident = 0; }
	w.cluster.colorResident = (u32)std::max(0, resident);
	w.cluster.colorNarrowBlocks = resident >= 2 ? (u32)resident * computeUnits : 0u;
	if (w.cluster.colorBlocksLimit) w.cluster.colorNarrowBlocks = std::min(w.cluster.colorNarrowBlocks, w.cluster.colorBlocksLimit); // MI_CLUSTER_COLOR_BLOCKS (tests: workgroups that stride over several tasks)
	w.cluster.colorNarrowLimit = w.cluster.colorNarrowBlocks ? std::min(w.cluster.colorNarrowMax, CLN_MAX_ITEMS) + 1u : 0u;
	if (w.cluster.colorNarrowLimit == 1u) w.cluster.colorNarrowLimit = 0u; // MI_CLUSTER_COLOR_NARROW_MAX=0: the wide kernel alone
	if (!w.cluster.colorNarrowLimit) w.cluster.colorNarrowBlocks = 0u;
	if (getenv("MI_CLUSTER_DEBUG")) fprintf(stderr, "[mi_physics] task colouring: narrow instance %u B LDS, %d resident per compute unit -> %u workgroups for tasks below %u items\n", (u32)CL_NARROW_LDS, resident, w.cluster.colorNarrowBlocks, w.cluster.colorNarrowLimit);
	return true;
}

// Colours the tasks k_cl_offsets / k_cl_scatter laid out: the narrow launch, a task per workgroup, then the wide one for the tasks beyond
// the narrow tables, one workgroup per workgroup of the solve launch (the same task rotation).  The wide launch is made every step:
// the host does not know the sizes of the tasks it is launching for.
void cluster_color_launch(World& w, u32 nj)
{
	ClColorArgs A;
	A.counters = w.dCounters.p; A.nb = w.nb; A.narrowLimit = w.cluster.colorNarrowLimit; A.taskStart = w.cluster.taskStart.p; A.pre = w.cluster.pre.p; A.actIds = w.actIds.p; A.phaseMask = w.cluster.phaseMask.p;
	A.tasks = (ClTask*)w.cluster.tasks.p; A.bodyList = w.cluster.bodyList.p; A.mOrder = w.mOrder.p; A.mKeySorted = w.mKeySorted.p; A.mLocal = w.cluster.local.p; A.cEntry = w.cluster.entry.p; A.sharedSlot = w.cluster.sharedSlot.p;
	A.jointStart = nj ? w.cluster.jointStart.p : (const u32*)nullptr; A.jointList = w.cluster.jointList.p; A.jointTable = w.cluster.jointTable.p; A.taskJoints = w.cluster.taskJoints.p; A.jointClassStart = w.cluster.jointClassStart.p; A.trace = w.cluster.flowTrace.p;
	if (w.cluster.colorNarrowBlocks) hipLaunchKernelGGL(k_cl_color_narrow, dim3(w.cluster.colorNarrowBlocks), dim3(CLN_LANES), CL_NARROW_LDS, w.stream, A);
	hipLaunchKernelGGL(k_cl_color, dim3(w.cluster.blocks), dim3(CL_LANES), CL_WIDE_LDS, w.stream, A);
}
