// Cluster sweep, third stage: the sweep itself.  One 512-lane workgroup per cluster runs its tasks in phase order, iteration after
// iteration, out of LDS and registers, and hands the bodies that more than one phase touches from task to task through tagged
// records.  cluster.h explains the clusters, the phases and the hand-over rule; k_cluster_color.hip builds what this stage reads.
#include "cluster.h"
#include "solver_rows.h"
#include "joint_solve.h"

#define CL_MAX_LOCAL_TASKS 8u              // tasks of all phases per workgroup
#define CLS_LANES 512u                    // k_cl_solve: 8 waves = 128 quads (four lanes work on one contact row) ...
#define CLQ_QUADS (CLS_LANES / 4u)
#define CLQ_SETS 7u                       // ... each keeping this many contact rows in registers (19 VGPRs per row and lane).  Eight sets reach the 256 VGPRs a launch of
                                          // 2 waves per SIMD allows only with 12-21 registers spilled into the colour loop: 7 sets (236 VGPRs, none spilled) solve 8 % faster
#define CLQ_REG_CONTACTS (CLQ_QUADS * CLQ_SETS) // contacts of a workgroup's first task that live in registers (worlds whose joints run inside the sweep: CLQ_SETS_JOINTS sets, the joint solves need the registers)
#define CLQ_SETS_JOINTS 4u
#define CL_SPIN_LIMIT (1u << 22)          // polls before a lane gives up: only reached when the workgroups are not all resident

// FOUR lanes (a quad) work on one contact row: lane q owns one of the row's four body vectors x (q = 0: vA, 1: wA, 2: vB, 3: wB — one
// float4 of the body's LDS record) and its pieces of the row: dT / dN = what x is dotted with in the tangent / normal row velocity
// (body A's negated), aT / aN = what an impulse adds to x (inverse mass and sign folded in).  A row velocity is the sum of the
// four lanes' 3-term dots — two DPP adds inside the quad, every lane gets the bit-identical total (p0 + p1) + (p2 + p3) — the
// impulse update is done by all four lanes redundantly, each then updates its vector: solver_rows.h's solveRow, lane for lane.
// Measured against one lane per manifold (tests/micro/colorstep.hip): a colour step is ONE LDS access each way and ~27 vector
// instructions per lane instead of four and ~66 — 344 cycles against 707, 450 against 1 880 when all eight waves have work — and a
// manifold of k contacts is k such steps (its contacts run in consecutive colours) instead of one step of 700 + 465 (k - 1) cycles.
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

struct QuadRow { V3 dT, aT, dN, aN; float mT, mN, bias, friction, lamN, lamT; }; // 18 floats per lane
#define CLQ_ZERO_FLOAT4S (2u * CLQ_QUADS + 4u)
#define CLQ_ROW_FLOAT4S 14u // a contact row outside the registers (LDS, or the global scratch beyond LDS): per lane q three float4 {dT, aT.x} {aT.yz, dN.xy} {dN.z, aN} at 3 q, then {mT, mN, bias, friction}, {lamN, lamT, addresses of lanes 0 | 1 << 16, 2 | 3 << 16}

struct ClLocal // a task of this workgroup, in LDS
{
	u32 first, count, numBodies, numShared, numColors, serialStart, numContacts, phase, key, sharedBase, numJoints;
	u32 bodyOff;     // float4 index of the task's bodies (2 float4 each)
	u32 infoOff;     // u32 index of per-body {global id, turn info, hand-over record}
	// Where a contact position's row lives, best tier at the CLOSING end: [0, spill) in the global scratch from scratchBase on, [spill,
	// regBase = numContacts - regContacts) in LDS (rowCap = regBase - spill rows from rowOff on), [regBase, numContacts) in the lanes'
	// register sets (the workgroup's first task only; set s of quad j holds position regBase + s * CLQ_QUADS + j)
	u32 regContacts, spill, rowOff, rowCap, scratchBase;
	u32 ldsColors;   // the task's first colours that end at or below regBase (a task with no contact in registers: all of them)
	u32 colorStart[68];
};

struct ClArgs
{
	u32* counters; const ClTask* tasks; const u32* bodyList; const u32* phaseMask; const u32* sharedSlot;
	const u32* mKeySorted; const u32* mLocal; const u32* cEntry;
	const float4* rowPlanes; const float4* rowShared; float2* rowLambda; float4* rowScratch; u32 scratchContacts;
	u32 regContactsCap; // MI_CLUSTER_REG_CONTACTS: most contacts a first task keeps in registers (tests; ~0u: as many as the sets hold)
	u32 ldsRowsCap;     // MI_CLUSTER_LDS_ROWS: most rows a workgroup keeps in LDS (tests; ~0u: as many as fit)
	u32 predictDiv, pollSleep; // pacing of the hand-over polls (CL_PREDICT_DIV / CL_POLL_SLEEP)
	float4* vel; u64* flow; u64* trace; // trace: developer timeline (mi_debug_flow_trace), normally null
	size_t rowCap; u32 nb, flowBytes, epoch, itBegin, itEnd, ldsFloat4s;
	// joints run by the sweep (null / 0 when the world has none or they keep their own launches): per phase-0 task the class offsets
	// [CL_MAX_JOINT_CLASSES + 2] (last two: joint count, first entry), the class-sorted entries {table index, la | lb << 16}, the table
	// {type | class << 8, index in the type's arrays, body a, body b}, the per-type update records, world inverse inertia
	const u32* jointClassStart; const uint2* taskJoints; const uint4* jointTable; float* jointUpd[MI_JOINT_TYPES]; const float4* invIw; u32 numJointClasses;
};

MI_DEV float clQuadSum(float p)
{
	float q = p + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0xB1, 0xF, 0xF, false)); // quad_perm [1, 0, 3, 2]: lin + ang of one body
	return q + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q), 0x4E, 0xF, 0xF, false));   // quad_perm [2, 3, 0, 1]: body A's + body B's
}
// One contact row (friction, then normal: constraints.cpp:3404-3442) on this lane's body vector x.
MI_DEV void clSolveQuad(QuadRow& r, V3& x)
{
	float vt = clQuadSum(rowDot3(x, r.dT));
	float maxFriction = r.friction * r.lamN;
	float newT = rowClampSym(__builtin_fmaf(-r.mT, vt, r.lamT), maxFriction);
	float d = newT - r.lamT; r.lamT = newT;
	x = rowFma(d, r.aT, x);
	float vn = clQuadSum(rowDot3(x, r.dN));
	float newN = fmaxf(__builtin_fmaf(-r.mN, vn - r.bias, r.lamN), 0.f);
	d = newN - r.lamN; r.lamN = newN;
	x = rowFma(d, r.aN, x);
}
// Lane q's view of contact position p of task L, from the global row planes: its pieces of the row and the LDS address of its body
// vector (a static body: the all-zero record; its apply vectors are zero, so what is written back is the zero that was read).
MI_DEV void clBuildQuadRow(QuadRow& r, u32& addr, const ClLocal& L, const ClArgs& A, const float4* lds, u32 p, u32 q, u32 zeroRec, u32& slotOut, u32& kOut)
{
	const u32 e = A.cEntry[(size_t)4u * L.first + p], mp = e & 0xFFFu, k = e >> 12, slot = L.first + mp;
	const u32 ab = A.mLocal[slot], local = q < 2u ? (ab & 0xFFFFu) : (ab >> 16);
	const float4 sh = A.rowShared[slot];
	ContactRow row; loadRow(row, k, slot, A.rowCap, A.rowPlanes, A.rowLambda);
	const bool isStatic = local == CL_LOCAL_STATIC;
	addr = (isStatic ? zeroRec : L.bodyOff + 2u * local) + (q & 1u);
	const float invMass = isStatic ? 0.f : lds[L.bodyOff + 2u * local].w; // (.w of a body's first float4 = its inverse mass, constant over the launch)
	const V3 t = v3(row.p0.x, row.p0.y, row.p0.z), n = v3(sh.x, sh.y, sh.z);
	if (q == 0u) { r.dT = -t; r.aT = -(invMass * t); r.dN = -n; r.aN = -(invMass * n); }
	else if (q == 1u) { r.dT = -v3(row.p0.w, row.p1.x, row.p1.y); r.aT = -v3(row.p3.w, row.p4.x, row.p4.y); r.dN = -v3(row.p2.y, row.p2.z, row.p2.w); r.aN = -v3(row.p5.y, row.p5.z, row.p5.w); }
	else if (q == 2u) { r.dT = t; r.aT = invMass * t; r.dN = n; r.aN = invMass * n; }
	else { r.dT = v3(row.p1.z, row.p1.w, row.p2.x); r.aT = v3(row.p4.z, row.p4.w, row.p5.x); r.dN = v3(row.p3.x, row.p3.y, row.p3.z); r.aN = v3(row.p6.x, row.p6.y, row.p6.z); }
	r.mT = row.p7.x; r.mN = row.p6.w; r.bias = row.p7.y; r.friction = sh.w; r.lamN = row.lam.x; r.lamT = row.lam.y;
	slotOut = slot; kOut = k;
}
// Row storage outside the registers (P = the contact's CLQ_ROW_FLOAT4S float4): every lane stores its vectors, lane 0 the scalars and lane
// 0 / 2 the packed addresses of their pair of lanes (the addresses of a quad: two bodies x {linear, angular} = base and base + 1).
template <typename T> MI_DEV T clLdsAt(const float4* lds, u32 byte) { return *(const T*)((const char*)lds + byte); }
template <typename PTR> MI_DEV void clStoreQuadRow(PTR P, u32 q, const QuadRow& r, u32 addr)
{
	P[3u * q] = make_float4(r.dT.x, r.dT.y, r.dT.z, r.aT.x); P[3u * q + 1u] = make_float4(r.aT.y, r.aT.z, r.dN.x, r.dN.y); P[3u * q + 2u] = make_float4(r.dN.z, r.aN.x, r.aN.y, r.aN.z);
	if (q == 0u) P[12] = make_float4(r.mT, r.mN, r.bias, r.friction);
	const u32 other = (u32)__builtin_amdgcn_update_dpp(0, (int)addr, 0xB1, 0xF, 0xF, false); // the partner lane's address (quad_perm [1, 0, 3, 2])
	const u32 otherPair = (u32)__builtin_amdgcn_update_dpp(0, (int)(addr | (other << 16)), 0x4E, 0xF, 0xF, false); // lanes 2 | 3 << 16 seen from lane 0
	if (q == 0u) P[13] = make_float4(r.lamN, r.lamT, __uint_as_float(addr | (other << 16)), __uint_as_float(otherPair));
}
MI_DEV u32 clPairAddr(u32 pair, u32 q) { return (q & 1u) ? (pair >> 16) : (pair & 0xFFFFu); } // a lane's address out of its pair's word
#define CLQ_PAIR_WORD(q) (54u + ((q) >> 1)) // u32 index of that word inside a row: P[13].z for lanes 0 and 1, P[13].w for lanes 2 and 3
template <typename PTR> MI_DEV void clLoadQuadRow(QuadRow& r, u32& addr, PTR P, u32 q)
{
	float4 a = P[3u * q], b = P[3u * q + 1u], c = P[3u * q + 2u], d = P[12], e = P[13];
	r.dT = v3f4(a); r.aT = v3(a.w, b.x, b.y); r.dN = v3(b.z, b.w, c.x); r.aN = v3(c.y, c.z, c.w);
	r.mT = d.x; r.mN = d.y; r.bias = d.z; r.friction = d.w; r.lamN = e.x; r.lamT = e.y;
	addr = clPairAddr(__float_as_uint(q < 2u ? e.z : e.w), q);
}

// JOINTS: the instantiation for worlds whose joints run inside the sweep (its extra registers and code stay out of the other one).
template <bool JOINTS> __global__ void __launch_bounds__(CLS_LANES) k_cl_solve(ClArgs A)
{
	extern __shared__ float4 lds[];
	__shared__ ClLocal sTask[CL_MAX_LOCAL_TASKS];
	__shared__ u32 sNumTasks, sAbort;
	__shared__ u32 sRegStart[CL_SERIAL_COLOR + 4u]; // the first task's colorStart counted from its regBase, as its register sets count (what lies below wraps and is never read)
	const u32 tid = threadIdx.x, G = gridDim.x, quad = tid >> 2, q = tid & 3u;
	constexpr u32 SETS = JOINTS ? CLQ_SETS_JOINTS : CLQ_SETS;
	u32* status = A.counters + CTR_FLOW_STATUS;
	__amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(A.flow, 0, A.flowBytes, 0x00020000);
	// The static body: an all-zero record.  Its apply vectors are zero, so a contact lane writes back the zero it read; every quad has its own copy
	// (CLQ_ZERO_FLOAT4S float4 at the end of LDS: a third of a pile's contacts touch the ground, and same-address writes of one wave
	// instruction are served one after the other).  The joints read a shared copy and write into a sink.
	const u32 zeroBase = A.ldsFloat4s - CLQ_ZERO_FLOAT4S, zeroRec = zeroBase + 2u * CLQ_QUADS, sinkRec = zeroRec + 2u;

	// ---- which tasks are mine, and where they live in LDS ----
	if (tid == 0)
	{
		if (A.trace) A.trace[(size_t)blockIdx.x * CL_TRACE_ROWS * CL_TRACE_WORDS + 15 * 32] = wall_clock64();
		u32 nT = 0, off = 0, used = 0; // used: float4s of LDS handed out
		bool bad = A.counters[CTR_CL_STATUS] != 0u;
		for (u32 p = 0; p < CL_MAX_PHASES; ++p)
		{
			u32 tasksInPhase = A.counters[CTR_CL_NUM_TASKS + p];
			if (tasksInPhase > CL_TASKS_PER_PHASE * G) { bad = true; atomicOr(status, 128u); }
			// task t of phase p runs on workgroup (clPhaseOffset + t) % G; a phase with more tasks than workgroups wraps around (its tasks
			// share no body, so a workgroup may run two of them one after the other)
			off = clPhaseOffset(A.counters, p);
			u32 t = (blockIdx.x + G - (off % G)) % G;
			for (; t < tasksInPhase && !bad; t += G)
			{
				u32 key = p * CL_MAX_TASKS + t;
				const ClTask* T = A.tasks + key;
				const u32 tj = (A.jointClassStart && p == 0u) ? A.jointClassStart[(size_t)key * (CL_MAX_JOINT_CLASSES + 2u) + CL_MAX_JOINT_CLASSES] : 0u; // joints of the task
				if (!T->count && !tj) continue;
				if (nT == CL_MAX_LOCAL_TASKS) { bad = true; atomicOr(status, 256u); break; }
				ClLocal& L = sTask[nT];
				L.first = T->first; L.count = T->count; L.numBodies = T->numBodies; L.numShared = T->numShared; L.numColors = T->numColors; L.serialStart = T->serialStart; L.numContacts = T->numRows;
				L.phase = p; L.key = key; L.sharedBase = T->sharedBase; L.numJoints = tj;
				if (tj > CLS_LANES || (tj && nT)) { bad = true; atomicOr(status, 2048u); } // one lane per joint; joints run with the workgroup's first task only
				for (u32 c = 0; c <= CL_SERIAL_COLOR + 1u; ++c) L.colorStart[c] = T->colorStart[c];
				L.colorStart[CL_SERIAL_COLOR + 2u] = L.colorStart[CL_SERIAL_COLOR + 1u]; L.colorStart[CL_SERIAL_COLOR + 3u] = L.colorStart[CL_SERIAL_COLOR + 1u]; // (the colour loop reads two entries ahead)
				L.bodyOff = used; used += 2u * L.numBodies;
				L.infoOff = used * 4u; used += (3u * L.numBodies + 3u) / 4u;
				L.regContacts = (nT == 0) ? min(L.numContacts, min(CLQ_QUADS * SETS, A.regContactsCap)) : 0u;
				L.rowOff = 0; L.rowCap = 0; L.spill = 0;
				const u32 regBase = L.numContacts - L.regContacts;
				// (The colour loop runs these while c < ldsColors, the rest while c < mainColors.  ldsColors <= mainColors for non-empty colours:
				// the one-wave tail's colours begin at or beyond regBase.  An EMPTY colour that sits at regBase and opens the tail is counted here
				// too: the LDS loop then takes one step without a row past mainColors and the tail runs the empty colour again, no row either way.
				// The scratch loop in front ends on csCur == spill whenever colours remain, whether it cut a colour there or not.)
				L.ldsColors = 0; while (L.ldsColors < L.numColors && L.colorStart[L.ldsColors + 1u] <= regBase) ++L.ldsColors;
				if (nT == 0) for (u32 c = 0; c < CL_SERIAL_COLOR + 4u; ++c) sRegStart[c] = L.colorStart[c] - regBase;
				++nT;
			}
		}
		if (used + CLQ_ZERO_FLOAT4S > A.ldsFloat4s) { bad = true; atomicOr(status, 512u); } // the bodies alone exceed LDS: cannot run this launch
		// rows outside the register sets: whatever LDS is left, in task order
		u32 ldsRowsLeft = A.ldsRowsCap;
		for (u32 k = 0; k < nT && !bad; ++k)
		{
			ClLocal& L = sTask[k];
			u32 want = L.numContacts - L.regContacts;
			u32 left = A.ldsFloat4s - used - CLQ_ZERO_FLOAT4S; // (the end of LDS holds the static body's all-zero records and the sink)
			u32 fit = min(left / CLQ_ROW_FLOAT4S, ldsRowsLeft);
			u32 cap = want < fit ? want : fit;              // what does not fit, the task's FIRST positions, goes to the global scratch (L2-resident, every step on such a row waits for it: the cluster build sizes the later phases' tasks so that this is rare)
			L.rowOff = used; L.rowCap = cap; used += CLQ_ROW_FLOAT4S * cap; ldsRowsLeft -= cap; L.scratchBase = 0; L.spill = want - cap;
			if (want > cap) { L.scratchBase = atomicAdd(&A.counters[CTR_CL_SCRATCH], want - cap); if (L.scratchBase + (want - cap) > A.scratchContacts) { bad = true; atomicOr(status, 1024u); break; } }
		}
		if (bad) atomicOr(status, 64u);
		sNumTasks = nT; sAbort = (bad || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 1u : 0u;
	}
	__syncthreads();
	if (sAbort) return; // uniform: the launch cannot run (or somebody has given up already); the host redoes the step
	const u32 numTasks = sNumTasks;
	if (!numTasks) return;

	// ---- prologue: bodies, then the rows ----
	for (u32 k = 0; k < numTasks; ++k)
	{
		const ClLocal& L = sTask[k];
		u32* info = (u32*)lds + L.infoOff;
		for (u32 l = tid; l < L.numBodies; l += CLS_LANES)
		{
			u32 g = A.bodyList[(size_t)L.key * CL_BODY_STRIDE + l];
			u32 pm = A.phaseMask[g];
			u32 deg = __popc(pm), rank = __popc(pm & ((1u << L.phase) - 1u));
			// where the body comes from: the record of the phase that used it last (the last phase of the previous iteration for this
			// iteration's first user)
			u32 below = pm & ((1u << L.phase) - 1u);
			u32 prev = below ? 31u - (u32)__clz(below) : 31u - (u32)__clz(pm);
			info[3 * l] = g; info[3 * l + 1] = deg | (rank << 8);
			info[3 * l + 2] = (l < L.numShared) ? A.sharedSlot[(size_t)prev * (A.nb + 1u) + g] : 0u;
			lds[L.bodyOff + 2 * l] = A.vel[2 * g]; lds[L.bodyOff + 2 * l + 1] = A.vel[2 * g + 1]; // shared ones too: .w = invMass stays, the rest is replaced at every acquire
		}
	}
	for (u32 i = tid; i < CLQ_ZERO_FLOAT4S; i += CLS_LANES) lds[zeroBase + i] = make_float4(0.f, 0.f, 0.f, 0.f);
	__syncthreads();
	// the first task's last regContacts contacts in registers: set s of this lane's quad holds contact position regBase + s * CLQ_QUADS + quad
	QuadRow rows[SETS]; u32 addr[SETS];
	{
		const ClLocal& L = sTask[0];
		const u32 regBase = L.numContacts - L.regContacts;
#pragma unroll
		for (u32 s = 0; s < SETS; ++s)
		{
			const u32 p = s * CLQ_QUADS + quad;
			rows[s].dT = rows[s].aT = rows[s].dN = rows[s].aN = v3(0.f, 0.f, 0.f); rows[s].mT = rows[s].mN = rows[s].bias = rows[s].friction = rows[s].lamN = rows[s].lamT = 0.f; addr[s] = sinkRec;
			if (p < L.regContacts) { u32 slot, kk; clBuildQuadRow(rows[s], addr[s], L, A, lds, regBase + p, q, zeroBase + 2u * quad, slot, kk); }
		}
	}
	// every other contact of the workgroup's tasks, the positions below regBase: its four lane rows in LDS, the first spill of them in the scratch
	for (u32 k = 0; k < numTasks; ++k)
	{
		const ClLocal& L = sTask[k];
		for (u32 p = quad; p < L.numContacts - L.regContacts; p += CLQ_QUADS)
		{
			QuadRow r; u32 a, slot, kk;
			clBuildQuadRow(r, a, L, A, lds, p, q, zeroBase + 2u * quad, slot, kk);
			if (p >= L.spill) clStoreQuadRow(lds + L.rowOff + (p - L.spill) * CLQ_ROW_FLOAT4S, q, r, a);
			else clStoreQuadRow(A.rowScratch + (size_t)(L.scratchBase + p) * CLQ_ROW_FLOAT4S, q, r, a);
		}
	}
	// The last colours of a task hold a handful of contacts (the busiest body's last rows).  Those of the first task that lie in the
	// registers and whose positions, counted from regBase, all fall into ONE block of 16 belong to one wave (16 quads of one register
	// set): that wave runs them back to back, in program order, without the workgroup barrier in between (LDS serves a wave's accesses
	// in order).  tailStart0 = first such colour, tailSet = their register set, myTail = this lane's colour among them (255: none).
	u32 tailStart0 = sTask[0].numColors, tailSet = 0, myTail = 255u;
	{
		const ClLocal& L = sTask[0];
		const u32 regBase = L.numContacts - L.regContacts, endPos = L.colorStart[L.numColors];
		if (L.numColors && endPos > regBase)
		{
			const u32 blk = (endPos - regBase - 1u) >> 4;
			while (tailStart0 > 0u && L.colorStart[tailStart0 - 1u] >= regBase && ((L.colorStart[tailStart0 - 1u] - regBase) >> 4) == blk) --tailStart0;
			if (L.numColors - tailStart0 < 2u) tailStart0 = L.numColors;
			else
			{
				tailSet = (L.colorStart[tailStart0] - regBase) / CLQ_QUADS;
				const u32 p = regBase + tailSet * CLQ_QUADS + quad;
				if (p >= L.colorStart[tailStart0] && p < endPos) { myTail = tailStart0; while (L.colorStart[myTail + 1u] <= p) ++myTail; }
			}
		}
		tailStart0 = __builtin_amdgcn_readfirstlane(tailStart0); tailSet = __builtin_amdgcn_readfirstlane(tailSet);
	}
	// this lane's joint (first task only, phase 0): class, update record, the two bodies as LDS addresses and as global ids (inverse inertia)
	const u32 bodyOff0 = sTask[0].bodyOff;
	u32 jClass = 0xFFFFFFFFu, jType = 0, jA = 0, jB = 0, jRdA = zeroRec, jWrA = sinkRec, jRdB = zeroRec, jWrB = sinkRec; float* jRec = nullptr;
	const u32 numJoints0 = (JOINTS && sTask[0].phase == 0u) ? sTask[0].numJoints : 0u;
	if (JOINTS && tid < numJoints0)
	{
		const u32* cs = A.jointClassStart + (size_t)sTask[0].key * (CL_MAX_JOINT_CLASSES + 2u);
		uint2 e = A.taskJoints[cs[CL_MAX_JOINT_CLASSES + 1u] + tid];
		uint4 t4 = A.jointTable[e.x];
		jType = t4.x & 0xFFu; jClass = t4.x >> 8; jA = t4.z; jB = t4.w;
		jRec = A.jointUpd[jType] + (size_t)t4.y * jointUpdateFloats(jType);
		u32 la = e.y & 0xFFFFu, lb = e.y >> 16;
		if (la != CL_LOCAL_STATIC) { jRdA = bodyOff0 + 2u * la; jWrA = jRdA; }
		if (lb != CL_LOCAL_STATIC) { jRdB = bodyOff0 + 2u * lb; jWrB = jRdB; }
	}
	__syncthreads();
	// developer timeline: 16 rows of 32 stamps per workgroup: row 3 k = "task k acquired its shared bodies" in iteration (column), row
	// 3 k + 1 = "task k's colours done"; rows 5-6: core-clock stamp after every colour of iteration 10 of the first task, rows 7-8: the
	// colours' sizes; row 15: [0] kernel start, [1] prologue done, [2 + 4 k ..] task k's size, colours, shared bodies, phase;
	// [22 + k] task k's rows in LDS | in registers << 32 (the rest of its contacts: in the global scratch); [27 + k] task k's rows in the
	// scratch (its positions below that) | colours run by the one-wave tail << 32
	u64* trace = A.trace ? A.trace + (size_t)blockIdx.x * CL_TRACE_ROWS * CL_TRACE_WORDS : nullptr;
	if (trace && tid == 0)
	{
		trace[15 * 32 + 1] = wall_clock64();
		for (u32 k = 0; k < numTasks && k < 5u; ++k) { trace[15 * 32 + 2 + 4 * k] = sTask[k].count; trace[15 * 32 + 3 + 4 * k] = sTask[k].numColors; trace[15 * 32 + 4 + 4 * k] = sTask[k].numShared; trace[15 * 32 + 5 + 4 * k] = sTask[k].phase | (sTask[k].numBodies << 8) | ((u64)sTask[k].numContacts << 32); trace[15 * 32 + 22 + k] = sTask[k].rowCap | ((u64)sTask[k].regContacts << 32); trace[15 * 32 + 27 + k] = sTask[k].spill | ((u64)(k == 0u ? sTask[0].numColors - tailStart0 : 0u) << 32); }
	}

	// One step = the contacts at positions [cs, end) of a task (one colour, or one contact of the serial tail).  A task's positions lie in
	// up to three tiers, the best at the closing end (ClLocal): [0, spill) rows in the global scratch, [spill, regBase) rows in LDS,
	// [regBase, numContacts) register set (position - regBase) / CLQ_QUADS of quad (position - regBase) % CLQ_QUADS.  The closing colours
	// are the many small ones (the busiest body's last rows), the opening ones the few large ones: a colour step costs the same whatever it
	// holds, so the cheap tier goes where the steps are, and the one-wave tail below is open to every first task.  The colour loop runs
	// tier by tier, and a colour that straddles spill or regBase is cut there (one more barrier): the scratch colours through the general
	// step CLQ_SOLVE_ROWS, the LDS colours through the short CLQ_SOLVE_ROWS_LDS (per colour, not per task: a task with rows in the scratch
	// pays for them in its opening colours only), then the register colours on positions counted from regBase, written SET BY SET (a
	// colour's positions are consecutive, so the colours that begin in set S are a run of the loop; one that reaches beyond set S + 1 is
	// cut into two steps), so that the code of a step names its one or two register sets statically: no dispatch, nothing of the other
	// sets passes through the loop, and no row step stands between the set loops.
#define CLQ_SOLVE_SET(S_, CS_, END_) if ((S_) < SETS) { const u32 pos = (S_) * CLQ_QUADS + quad; if (pos >= (CS_) && pos < (END_)) { float4 b = lds[addr[(S_) < SETS ? (S_) : 0u]]; V3 x = v3f4(b); clSolveQuad(rows[(S_) < SETS ? (S_) : 0u], x); lds[addr[(S_) < SETS ? (S_) : 0u]] = make_float4(x.x, x.y, x.z, b.w); } }
	// A row in LDS carries its body addresses in its last float4: read with the row, the body read would be a SECOND dependent LDS round
	// trip per step.  So a lane asks for the address word of the row it solves next one step early (pfW): a step's start is the end of
	// the step before it, the lane's first LDS row of the step that follows [CS_, END_) is max(END_, spill) + quad, and the scratch
	// steps in front of the first LDS step leave that at spill + quad, which the request made for the task's turn covers (CLQ_PREFETCH_TURN);
	// the register steps come last and ask for nothing.  The address words are written by the prologue alone (a step writes back its
	// row's two impulses, never the float2 beside them), so the word a lane holds across a barrier cannot be stale.  Further passes of a
	// step with more than CLQ_QUADS rows get their word from the pass before them.  Rows in the global scratch keep the two trips.
#define CLQ_PREFETCH(POS_) { const u32 in_ = max((POS_), spill) + quad - spill; if (in_ < rowCap) pfW = ((const u32*)(lds + rowOff + in_ * CLQ_ROW_FLOAT4S))[CLQ_PAIR_WORD(q)]; }
	// The general step: positions [CS_, END_) below regBase, wherever their rows live, in passes of CLQ_QUADS (the scratch colours, cut at
	// spill, and the serial tail's contacts outside the registers).  [CS_, END_) must lie on ONE side of spill: the word a lane brings
	// along (pfW) is that of LDS row max(CS_, spill) + quad - spill, its first row only if the step does not begin below spill and reach beyond it.
#define CLQ_SOLVE_ROWS(CS_, END_) \
	{ \
		u32 w = pfW; \
		CLQ_PREFETCH(END_) \
		for (u32 p = (CS_) + quad; p < (END_); p += CLQ_QUADS) \
		{ \
			const bool inLds = p >= spill; \
			QuadRow r; u32 a; float4 b; \
			float4* P = lds + rowOff + (inLds ? p - spill : 0u) * CLQ_ROW_FLOAT4S; \
			float4* S = A.rowScratch + (size_t)(scratchBase + (inLds ? 0u : p)) * CLQ_ROW_FLOAT4S; \
			u32 wn = 0u; if (p + CLQ_QUADS < (END_) && p + CLQ_QUADS >= spill) wn = ((const u32*)(lds + rowOff + (p + CLQ_QUADS - spill) * CLQ_ROW_FLOAT4S))[CLQ_PAIR_WORD(q)]; \
			if (inLds) { u32 unused; a = clPairAddr(w, q); b = lds[a]; clLoadQuadRow(r, unused, P, q); } else { clLoadQuadRow(r, a, S, q); b = lds[a]; } \
			V3 x = v3f4(b); clSolveQuad(r, x); lds[a] = make_float4(x.x, x.y, x.z, b.w); \
			if (q == 0u) { if (inLds) ((float2*)(P + 13))[0] = make_float2(r.lamN, r.lamT); else ((float2*)(S + 13))[0] = make_float2(r.lamN, r.lamT); } \
			w = wn; \
		} \
	}
	// The same step for positions whose rows are ALL in LDS, spill <= CS_ < END_ <= regBase: every task but a workgroup's first runs all
	// its colours here, but for the few whose first rows did not fit.  Measured, a row step cost 0.43 us against the register step's 0.28,
	// and what it costs is its instruction count far more than its LDS round trips (a wave gets through the ~45 instructions of a
	// register step in ~650 cycles).  So this form keeps it short: a step takes at most CLQ_QUADS rows (the loop cuts a larger colour
	// into several steps, as the set loops do at a set's end), so there is no loop over passes; no branch on where a row lives; row
	// addresses by one 24-bit multiply-add; and the request for the lane's next row is clamped to the task's last LDS row instead of
	// guarded (a lane without a next row reads a word it never uses).  Rows count from spill: i and endR are LDS row numbers, endR <=
	// rowCap, and a step that has a row has csCur < regBase, that is rowCap >= 1, so min(endR + quad, lastRow = rowCap - 1) names one of
	// the task's own rows [0, rowCap) whatever spill is (an empty colour of a task without LDS rows asks for the word at rowOff, inside
	// the workgroup's LDS in front of the zero records, and uses nothing).
#define CLQ_SOLVE_ROWS_LDS(CS_, END_) \
	{ \
		const u32 i = (CS_) - spill + quad, endR = (END_) - spill, w = pfW; \
		pfW = clLdsAt<u32>(lds, __umul24(min(endR + quad, lastRow), CLQ_ROW_FLOAT4S * 16u) + pairByte); \
		if (i < endR) \
		{ \
			const u32 a = clPairAddr(w, q), rowByte = __umul24(i, CLQ_ROW_FLOAT4S * 16u) + rowsByte, own = rowByte + q * 48u; \
			const float4 b = lds[a], r0 = clLdsAt<float4>(lds, own), r1 = clLdsAt<float4>(lds, own + 16u), r2 = clLdsAt<float4>(lds, own + 32u), r3 = clLdsAt<float4>(lds, rowByte + 192u); \
			const float2 lam = clLdsAt<float2>(lds, rowByte + 208u); \
			QuadRow r; r.dT = v3f4(r0); r.aT = v3(r0.w, r1.x, r1.y); r.dN = v3(r1.z, r1.w, r2.x); r.aN = v3(r2.y, r2.z, r2.w); \
			r.mT = r3.x; r.mN = r3.y; r.bias = r3.z; r.friction = r3.w; r.lamN = lam.x; r.lamT = lam.y; \
			V3 x = v3f4(b); clSolveQuad(r, x); lds[a] = make_float4(x.x, x.y, x.z, b.w); \
			if (q == 0u) *(float2*)((char*)lds + (rowByte + 208u)) = make_float2(r.lamN, r.lamT); \
		} \
	}
#define CLQ_ADVANCE(END_) \
	__syncthreads(); \
	if (stamp && c < 63u && (END_) == csNext) { trace[5 * 32 + 1 + c] = clock64(); trace[7 * 32 + c] = L.colorStart[c + 1u] - L.colorStart[c]; } \
	if ((END_) == csNext) { csCur = csNext; csNext = __builtin_amdgcn_readfirstlane(csAfter); ++c; } else csCur = (END_);
	// (in the set loops csCur, csNext and csAfter count from regBase, as the sets do: sRegStart; only a workgroup's first task gets here)
#define CLQ_SET_LOOP(S_) \
	if ((S_) < SETS) while (c < mainColors && csCur < min(regC, ((S_) + 1u) * CLQ_QUADS)) \
	{ \
		const u32 csAfter = sRegStart[c + 2u]; /* (requested now, needed at the next colour: the LDS round trip hides behind this step) */ \
		const u32 end = min(csNext, min(regC, ((S_) + 2u) * CLQ_QUADS)); /* (a colour that reaches beyond set S_ + 1 is cut there) */ \
		CLQ_SOLVE_SET(S_, csCur, end) \
		if (end > ((S_) + 1u) * CLQ_QUADS) { CLQ_SOLVE_SET((S_) + 1u, csCur, end) } \
		CLQ_ADVANCE(end) \
	}
	static_assert(CLQ_SETS <= 8u, "the colour loop below names eight sets");

	// ---- iterations ----
	bool aborted = false;
	// The first request of a task's turn reads the task record and then the row, two LDS round trips: it is made right after the turn
	// before it has published its bodies (and once in front of the loop), where it is in nobody's way, and returns while the workgroup waits for bodies.
#define CLQ_PREFETCH_TURN(K_) { const ClLocal& N = sTask[K_]; const u32 sp_ = N.spill, in_ = max(N.colorStart[0], sp_) + quad - sp_; if (in_ < N.rowCap) pfW = ((const u32*)(lds + N.rowOff + in_ * CLQ_ROW_FLOAT4S))[CLQ_PAIR_WORD(q)]; }
	u32 pfW = 0u; // the address word of this lane's next row outside the registers (CLQ_PREFETCH)
	CLQ_PREFETCH_TURN(0u)
	u64 lastPublish = 0; u32 lastWait = 0; // when this workgroup last handed its bodies on, and how long (10 ns ticks) the bodies of its first task then took to come back
	for (u32 it = A.itBegin; it < A.itEnd && !aborted; ++it)
	{
		for (u32 k = 0; k < numTasks; ++k)
		{
			const ClLocal& L = sTask[k];
			const u32* info = (const u32*)lds + L.infoOff;
			// acquire the bodies other phases also touch.  The sweep is periodic: a task's bodies come back about one iteration
			// period after they came back last time, so the workgroup sleeps through most of the previous wait before it polls (the
			// polls are uncached loads through the fabric: 50k lanes polling all the time slow every hand-over down); then every lane
			// polls the tagged halves of up to two bodies per pass, all loads in flight together, and fetches the second half
			// (stored before the first) once the tag has arrived.
			{
				if (k == 0 && lastWait > 64u && it > A.itBegin + 1u)
				{
					u64 until = lastPublish + (u64)(lastWait - lastWait / A.predictDiv);
					while (wall_clock64() < until) __builtin_amdgcn_s_sleep(8);
				}
				const u32 rel = it - A.itBegin;
				for (u32 base = 0; base < L.numShared; base += 2u * CLS_LANES)
				{
					u32 gid[2], want[2]; bool pend[2]; bool any = false;
#pragma unroll
					for (u32 qq = 0; qq < 2; ++qq)
					{
						u32 l = base + qq * CLS_LANES + tid;
						pend[qq] = false; gid[qq] = 0; want[qq] = 0;
						if (l >= L.numShared) continue;
						u32 ti = info[3 * l + 1], deg = ti & 0xFFu, rank = ti >> 8;
						if (rel == 0u && rank == 0u) continue; // first user of the launch: the prologue's copy of vel is current
						gid[qq] = info[3 * l + 2]; want[qq] = A.epoch + rel * deg + rank; pend[qq] = true; any = true;
					}
					u32 spins = 0;
					while (any)
					{
						u32x4 h0[2], h1[2];
						asm volatile("" ::: "memory");
#pragma unroll
						for (u32 qq = 0; qq < 2; ++qq)
							if (pend[qq]) { h0[qq] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, gid[qq] * 32u, 0, 16); h1[qq] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, gid[qq] * 32u + 16u, 0, 16); }
						any = false;
#pragma unroll
						for (u32 qq = 0; qq < 2; ++qq)
						{
							if (!pend[qq]) continue;
							if (h0[qq].w == want[qq] && h1[qq].w == want[qq]) // each half carries its own tag
							{
								u32 l = base + qq * CLS_LANES + tid;
								float invMass = lds[L.bodyOff + 2 * l].w; // constant over the launch
								lds[L.bodyOff + 2 * l] = make_float4(__uint_as_float(h0[qq].x), __uint_as_float(h0[qq].y), __uint_as_float(h0[qq].z), invMass);
								lds[L.bodyOff + 2 * l + 1] = make_float4(__uint_as_float(h1[qq].x), __uint_as_float(h1[qq].y), __uint_as_float(h1[qq].z), 0.f);
								pend[qq] = false;
							}
							any = any || pend[qq];
						}
						if (any)
						{
							if (++spins > CL_SPIN_LIMIT) { atomicOr(status, 1u); sAbort = 1u; break; }
							if ((spins & 63u) == 0u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { sAbort = 1u; break; }
							if (A.pollSleep == 1u) __builtin_amdgcn_s_sleep(1); else if (A.pollSleep >= 2u) __builtin_amdgcn_s_sleep(4);
						}
					}
				}
			}
			__syncthreads();
			if (sAbort) { aborted = true; break; }
			if (k == 0 && it > A.itBegin) lastWait = (u32)(wall_clock64() - lastPublish);
			if (trace && tid == 0 && it - A.itBegin < 32u && k < 5u) trace[(3 * k) * 32 + (it - A.itBegin)] = wall_clock64();
			// joints first (constraints.cpp:3748-3772: all joint types, then the contacts): one (type, colour) class per step
			if (JOINTS && k == 0 && numJoints0)
			{
				const u32* cs = A.jointClassStart + (size_t)L.key * (CL_MAX_JOINT_CLASSES + 2u);
				for (u32 c = 0; c < A.numJointClasses; ++c)
				{
					if (cs[c + 1u] == cs[c]) continue; // (uniform: the class has no joint in this task)
					if (jClass == c)
					{
						Vel v; float4 a0 = lds[jRdA], a1 = lds[jRdA + 1], b0 = lds[jRdB], b1 = lds[jRdB + 1];
						v.vA = v3f4(a0); v.wA = v3f4(a1); v.vB = v3f4(b0); v.wB = v3f4(b1); v.invMassA = a0.w; v.invMassB = b0.w;
						M3 IA = ldInvI(A.invIw, jA), IB = ldInvI(A.invIw, jB);
						jointSolve(jType, jRec, v, IA, IB);
						lds[jWrA] = make_float4(v.vA.x, v.vA.y, v.vA.z, v.invMassA); lds[jWrA + 1] = make_float4(v.wA.x, v.wA.y, v.wA.z, 0.f);
						lds[jWrB] = make_float4(v.vB.x, v.vB.y, v.vB.z, v.invMassB); lds[jWrB + 1] = make_float4(v.wB.x, v.wB.y, v.wB.z, 0.f);
					}
					__syncthreads();
				}
			}
			// the contacts, colour by colour (a colour = one row solve per quad), then the serial tail one contact per step
			{
				const u32 numColors = __builtin_amdgcn_readfirstlane(L.numColors), serialStart = __builtin_amdgcn_readfirstlane(L.serialStart), numContacts = __builtin_amdgcn_readfirstlane(L.numContacts);
				// (what a step needs of the task record, in scalar registers: read from LDS once per turn, not behind every barrier)
				const u32 regC = __builtin_amdgcn_readfirstlane(L.regContacts), rowOff = __builtin_amdgcn_readfirstlane(L.rowOff), rowCap = __builtin_amdgcn_readfirstlane(L.rowCap), scratchBase = __builtin_amdgcn_readfirstlane(L.scratchBase);
				const u32 spill = __builtin_amdgcn_readfirstlane(L.spill), ldsColors = __builtin_amdgcn_readfirstlane(L.ldsColors), regBase = numContacts - regC; // (the cut points: the same in every lane, in scalar registers)
				const bool stamp = trace && tid == 0 && it == A.itBegin + 10u && k == 0;
				if (stamp) trace[5 * 32] = clock64();
				const u32 mainColors = (k == 0u) ? tailStart0 : numColors;
				u32 c = 0, csCur = __builtin_amdgcn_readfirstlane(L.colorStart[0]), csNext = __builtin_amdgcn_readfirstlane(L.colorStart[1]);
				// (a first task that fits the register sets, every task of the sparse steps, falls straight through to the set loops: three loop
				// tests it had to branch over in front of them cost it 0.03 us per turn)
				if (__builtin_expect(regBase != 0u, 0))
				{
					// the opening colours whose rows did not fit LDS (rare: a later task behind large ones), cut at spill
					while (c < mainColors && csCur < spill)
					{
						const u32 csAfter = L.colorStart[c + 2u];
						const u32 end = min(csNext, spill);
						CLQ_SOLVE_ROWS(csCur, end)
						CLQ_ADVANCE(end)
					}
					// the colours in LDS rows (a task that is not the workgroup's first: all its other colours; a first task larger than the sets: its
					// opening ones).  Those that end at or below regBase run in a loop bounded by their number, which is all a later task needs (three
					// limits in one min() made the compiler take the step's end through a vector register); then the piece below regBase of a first
					// task's colour that straddles it.
					{
						const u32 rowsByte = rowOff * 16u, lastRow = max(rowCap, 1u) - 1u, pairByte = rowsByte + 4u * CLQ_PAIR_WORD(q);
						while (c < ldsColors)
						{
							const u32 csAfter = L.colorStart[c + 2u];
							const u32 end = min(csNext, csCur + CLQ_QUADS);
							CLQ_SOLVE_ROWS_LDS(csCur, end)
							CLQ_ADVANCE(end)
						}
						while (c < mainColors && csCur < regBase)
						{
							const u32 csAfter = L.colorStart[c + 2u];
							const u32 end = min(regBase, csCur + CLQ_QUADS); // (< csNext: the colour goes on in the registers)
							CLQ_SOLVE_ROWS_LDS(csCur, end)
							CLQ_ADVANCE(end)
						}
					}
					csCur -= regBase; csNext -= regBase;
				}
				// the colours in the register sets, on positions counted from regBase (a first task that fits the sets: regBase = 0, all of them)
				CLQ_SET_LOOP(0) CLQ_SET_LOOP(1) CLQ_SET_LOOP(2) CLQ_SET_LOOP(3) CLQ_SET_LOOP(4) CLQ_SET_LOOP(5) CLQ_SET_LOOP(6) CLQ_SET_LOOP(7)
				if (mainColors < numColors) // the first task's trailing colours: one wave, no workgroup barrier in between
				{
#define CLQ_TAIL(S_) case S_: if ((S_) < SETS && myTail != 255u) for (u32 ct = mainColors; ct < numColors; ++ct) { if (myTail == ct) { float4 b = lds[addr[(S_) < SETS ? (S_) : 0u]]; V3 x = v3f4(b); clSolveQuad(rows[(S_) < SETS ? (S_) : 0u], x); lds[addr[(S_) < SETS ? (S_) : 0u]] = make_float4(x.x, x.y, x.z, b.w); } __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); } break;
					switch (tailSet) { CLQ_TAIL(0) CLQ_TAIL(1) CLQ_TAIL(2) CLQ_TAIL(3) CLQ_TAIL(4) CLQ_TAIL(5) CLQ_TAIL(6) CLQ_TAIL(7) default: break; }
#undef CLQ_TAIL
					__syncthreads();
					if (stamp) for (u32 ct = mainColors; ct < numColors && ct < 63u; ++ct) { trace[5 * 32 + 1 + ct] = clock64(); trace[7 * 32 + ct] = L.colorStart[ct + 1u] - L.colorStart[ct]; }
				}
				if (serialStart < numContacts) CLQ_PREFETCH(serialStart) // (colorStart[numColors] = serialStart: the colours left this very word; asked for again so that the tail does not lean on it)
				for (u32 sp = serialStart; sp < numContacts; ++sp) // the serial tail (manifolds that found no colour run below 64): one contact per step
				{
					if (sp >= regBase)
					{
						const u32 rp = sp - regBase;
						switch (rp / CLQ_QUADS)
						{
							case 0: CLQ_SOLVE_SET(0u, rp, rp + 1u) break; case 1: CLQ_SOLVE_SET(1u, rp, rp + 1u) break; case 2: CLQ_SOLVE_SET(2u, rp, rp + 1u) break; case 3: CLQ_SOLVE_SET(3u, rp, rp + 1u) break;
							case 4: CLQ_SOLVE_SET(4u, rp, rp + 1u) break; case 5: CLQ_SOLVE_SET(5u, rp, rp + 1u) break; case 6: CLQ_SOLVE_SET(6u, rp, rp + 1u) break; default: CLQ_SOLVE_SET(7u, rp, rp + 1u) break;
						}
					}
					else { CLQ_SOLVE_ROWS(sp, sp + 1u) }
					__syncthreads();
				}
			}
			if (trace && tid == 0 && it - A.itBegin < 32u && k < 5u) trace[(3 * k + 1) * 32 + (it - A.itBegin)] = wall_clock64();
			// hand the shared bodies on
			for (u32 l = tid; l < L.numShared; l += CLS_LANES)
			{
				u32 g = info[3 * l], ti = info[3 * l + 1];
				u32 deg = ti & 0xFFu, rank = ti >> 8;
				u32 want = A.epoch + (it - A.itBegin) * deg + rank;
				u32 rec = (L.sharedBase + l) * 32u; // consecutive lanes, consecutive records: the write-through stores coalesce
				float4 b0 = lds[L.bodyOff + 2 * l], b1 = lds[L.bodyOff + 2 * l + 1];
				if (it + 1u == A.itEnd && rank + 1u == deg) { A.vel[2 * g] = b0; A.vel[2 * g + 1] = make_float4(b1.x, b1.y, b1.z, 0.f); } // last user of the launch
				else
				{
					u32x4 h1 = { __float_as_uint(b1.x), __float_as_uint(b1.y), __float_as_uint(b1.z), want + 1u };
					u32x4 h0 = { __float_as_uint(b0.x), __float_as_uint(b0.y), __float_as_uint(b0.z), want + 1u };
					__builtin_amdgcn_raw_buffer_store_b128(h1, rsrc, rec + 16u, 0, 16);
					__builtin_amdgcn_raw_buffer_store_b128(h0, rsrc, rec, 0, 16);
				}
			}
			if (k + 1u == numTasks) lastPublish = wall_clock64();
			CLQ_PREFETCH_TURN(k + 1u < numTasks ? k + 1u : 0u)
		}
	}
	if (aborted) return; // the host redoes the step (World::recoverSolve)

	// ---- epilogue: task-private bodies and the accumulated impulses go home ----
	for (u32 k = 0; k < numTasks; ++k)
	{
		const ClLocal& L = sTask[k];
		const u32* info = (const u32*)lds + L.infoOff;
		for (u32 l = L.numShared + tid; l < L.numBodies; l += CLS_LANES)
		{
			u32 g = info[3 * l];
			float4 b1 = lds[L.bodyOff + 2 * l + 1];
			A.vel[2 * g] = lds[L.bodyOff + 2 * l]; A.vel[2 * g + 1] = make_float4(b1.x, b1.y, b1.z, 0.f);
		}
		if (q == 0u) // (a quad's four lanes hold the same impulses)
		{
			if (k == 0)
			{
#pragma unroll
				for (u32 s = 0; s < SETS; ++s)
				{
					const u32 p = s * CLQ_QUADS + quad;
					if (p < L.regContacts) { const u32 e = A.cEntry[(size_t)4u * L.first + (L.numContacts - L.regContacts) + p]; A.rowLambda[(size_t)(e >> 12) * A.rowCap + L.first + (e & 0xFFFu)] = make_float2(rows[s].lamN, rows[s].lamT); }
				}
			}
			for (u32 p = quad; p < L.numContacts - L.regContacts; p += CLQ_QUADS)
			{
				const u32 e = A.cEntry[(size_t)4u * L.first + p];
				const float4 lam = p >= L.spill ? lds[L.rowOff + (p - L.spill) * CLQ_ROW_FLOAT4S + 13u] : A.rowScratch[(size_t)(L.scratchBase + p) * CLQ_ROW_FLOAT4S + 13u];
				A.rowLambda[(size_t)(e >> 12) * A.rowCap + L.first + (e & 0xFFFu)] = make_float2(lam.x, lam.y);
			}
		}
	}
#undef CLQ_SET_LOOP
#undef CLQ_ADVANCE
#undef CLQ_SOLVE_ROWS
#undef CLQ_SOLVE_ROWS_LDS
#undef CLQ_PREFETCH
#undef CLQ_PREFETCH_TURN
#undef CLQ_SOLVE_SET
}

// ---------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------
bool cluster_solves_joints(const World& w) { return w.cluster.jointsInCluster && w.cluster.jointsEnabled; }

// All of a workgroup's LDS beyond the kernel's static tables, less a margin, in whole float4s.
u32 cluster_solve_setup(const World& w)
{
	int maxLds = 0;
	MI_CHECK(hipDeviceGetAttribute(&maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, w.device));
	hipFuncAttributes fa = {};
	MI_CHECK(hipFuncGetAttributes(&fa, (const void*)k_cl_solve<true>));
	size_t dyn = (maxLds > 0 ? (size_t)maxLds : 65536) - fa.sharedSizeBytes - 256;
	dyn &= ~(size_t)15;
	if (hipFuncSetAttribute((const void*)k_cl_solve<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess
		|| hipFuncSetAttribute((const void*)k_cl_solve<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) return 0u;
	return (u32)dyn;
}

bool cluster_available(World& w)
{
	if (w.cluster.ldsBytes) return w.cluster.ldsBytes != ~0u;
	int cus = 0;
	MI_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, w.device));
	const u32 dyn = cluster_solve_setup(w);
	if (!dyn || !cluster_color_setup(w, (u32)std::max(1, cus)))
	{
		(void)hipGetLastError();
		w.cluster.ldsBytes = ~0u;
		return false;
	}
	w.cluster.ldsBytes = dyn; w.cluster.blocks = (u32)std::max(1, cus);
	if (w.cluster.blocksLimit) w.cluster.blocks = std::min(w.cluster.blocks, w.cluster.blocksLimit); // MI_CLUSTER_BLOCKS (tests: a small launch, so that phases wrap around)
	return true;
}

static const u32 CL_PREDICT_DIV = 4; // a lane sleeps through 1 - 1/CL_PREDICT_DIV of its previous wait for a hand-over before it polls
static const u32 CL_POLL_SLEEP = 1;  // pause between two polls (k_cl_solve: 0 none, 1 short, 2 long)

// Iterations [itBegin, itEnd) of the contact sweep in one launch.
void launch_cluster_solve(World& w, u32 itBegin, u32 itEnd)
{
	if (itBegin >= itEnd) return;
	size_t words = (size_t)(w.nb + 1) * CL_MAX_PHASES * 4; // one 32-byte hand-over record per (phase, body) at most
	if (w.cluster.flow.cap < words) { w.cluster.flow.ensure(words, w.stream); w.cluster.flowEpoch = 0; if (w.lastError) return; } // (a failed allocation leaves the old, smaller buffer: nothing may be launched over it)
	if (w.cluster.flowEpoch == 0 || w.cluster.flowEpoch >= 0xFFFEu) // first use or the turn counter about to wrap: no stale record may ever match
	{
		MI_CHECK(hipMemsetAsync(w.cluster.flow.p, 0, sizeof(u64) * words, w.stream));
		w.cluster.flowEpoch = 0;
	}
	w.cluster.flowEpoch++;
	if (w.cluster.flowTestAbortStep == w.stats.numInternalSteps) // tests: pretend a lane timed out; everybody drains without solving
	{
		u32 one = 16u;
		MI_CHECK(hipMemcpyAsync(w.dCounters.p + CTR_FLOW_STATUS, &one, sizeof(u32), hipMemcpyHostToDevice, w.stream));
		MI_CHECK(hipStreamSynchronize(w.stream));
	}
	const size_t scratchContacts = std::min<size_t>(2 * w.pairCap, 512u * 1024u); // rows that fit neither the registers nor LDS (224 B each)
	w.cluster.rowScratch.ensure(scratchContacts * CLQ_ROW_FLOAT4S, w.stream);
	if (w.lastError) return;
	if (itBegin) MI_CHECK(hipMemsetAsync(w.dCounters.p + CTR_CL_SCRATCH, 0, sizeof(u32), w.stream)); // (the step's first launch finds it cleared by k_cl_clear)
	ClArgs A;
	A.rowScratch = w.cluster.rowScratch.p; A.scratchContacts = (u32)scratchContacts; A.regContactsCap = w.cluster.regContactsCap; A.ldsRowsCap = w.cluster.ldsRowsCap;
	A.counters = w.dCounters.p; A.tasks = (const ClTask*)w.cluster.tasks.p; A.bodyList = w.cluster.bodyList.p; A.phaseMask = w.cluster.phaseMask.p; A.sharedSlot = w.cluster.sharedSlot.p;
	A.mKeySorted = w.mKeySorted.p; A.mLocal = w.cluster.local.p; A.cEntry = w.cluster.entry.p;
	A.rowPlanes = w.rowPlanes.p; A.rowShared = w.rowShared.p; A.rowLambda = w.rowLambda.p; A.vel = w.vel.p; A.flow = w.cluster.flow.p; A.trace = w.cluster.flowTrace.p; A.predictDiv = CL_PREDICT_DIV; A.pollSleep = CL_POLL_SLEEP;
	A.rowCap = w.rowCap; A.nb = w.nb; A.flowBytes = (u32)(words * sizeof(u64)); A.epoch = w.cluster.flowEpoch << 16; A.itBegin = itBegin; A.itEnd = itEnd;
	A.ldsFloat4s = w.cluster.ldsBytes / 16u;
	const bool withJoints = cluster_solves_joints(w);
	A.jointClassStart = withJoints ? w.cluster.jointClassStart.p : nullptr; A.taskJoints = w.cluster.taskJoints.p; A.jointTable = w.cluster.jointTable.p; A.invIw = w.invIw.p; A.numJointClasses = withJoints ? w.cluster.numJointClasses : 0u;
	for (u32 t = 0; t < MI_JOINT_TYPES; ++t) A.jointUpd[t] = w.joints[t].dUpdate.p;
	if (withJoints) hipLaunchKernelGGL(k_cl_solve<true>, dim3(w.cluster.blocks), dim3(CLS_LANES), w.cluster.ldsBytes, w.stream, A);
	else hipLaunchKernelGGL(k_cl_solve<false>, dim3(w.cluster.blocks), dim3(CLS_LANES), w.cluster.ldsBytes, w.stream, A);
}
