// The step: the launch sequence of one physicsStepInternal, what the host settles of the step before it, and physicsStep on top.
// Step order follows the reference's physicsStepInternal (physics.cpp:1180-1362) exactly: world-space colliders from the
// previous step's physics_transform1 -> broadphase -> narrowphase -> gravity/force integration -> constraint init (with
// post-gravity velocities) -> N solver iterations (joints by type, then contacts) -> velocity integration.
#include "world.h"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <algorithm>

void ensurePairBuffers(World& w, size_t numPairs)
{
	if (numPairs <= w.pairCap) return;
	size_t cap = std::max<size_t>(numPairs + numPairs / 2, 4096);
	w.pairs.ensure(cap, w.stream, true); w.pairsSorted.ensure(2 * cap, w.stream); w.pairKey.ensure(cap, w.stream); w.pairKeySorted.ensure(cap, w.stream);
	w.manifolds.ensure(cap, w.stream); w.actIds.ensure(cap, w.stream); w.epaList.ensure(cap, w.stream); w.gjkSimplex.ensure(9 * cap, w.stream); w.mColor.ensure(cap, w.stream); w.mKey.ensure(cap, w.stream); w.mKeySorted.ensure(cap, w.stream); w.mIdx.ensure(cap, w.stream); w.mOrder.ensure(cap, w.stream);
	w.rowPlanes.ensure((size_t)MI_MAX_CONTACTS_PER_MANIFOLD * MI_ROW_PLANES * cap, w.stream); w.rowShared.ensure(cap, w.stream);
	w.rowLambda.ensure((size_t)MI_MAX_CONTACTS_PER_MANIFOLD * cap, w.stream); w.rowIds.ensure(cap, w.stream);
	if (w.lastError) return; // an allocation failed: the capacities stay, the step returns the error
	w.pairCap = cap; w.rowCap = cap;
}

static void readCounters(World& w)
{
	MI_CHECK(hipMemcpyAsync(w.hCounters, w.dCounters.p, CTR_WORDS * sizeof(u32), hipMemcpyDeviceToHost, w.stream));
	MI_CHECK(hipStreamSynchronize(w.stream));
}

// This step's start (world-space colliders, pair count) ran on inputs that have changed since: run it again and read its counters.
// The early pair list + narrowphase, if any, were sized and fed by the stale start, so the step launches them anew.
static void restartStepStart(World& w, bool& early) { launch_build_colliders(w); launch_broadphase_count(w); readCounters(w); early = false; }

// The next colouring starts from scratch: no active list, no body masks, no claims, no colour history.
static void colorFromScratch(World& w)
{
	const size_t nb1 = (size_t)w.nb + 1;
	MI_CHECK(hipMemsetAsync(w.dCounters.p + CTR_NUM_ACTIVE, 0, 2 * sizeof(u32), w.stream)); // active-list cursor + contact count: the list is rebuilt
	MI_CHECK(hipMemsetAsync(w.bodyMask.p, 0, sizeof(u64) * nb1, w.stream));
	MI_CHECK(hipMemsetAsync(w.claim.p, 0xFF, sizeof(u64) * 2 * nb1, w.stream));
	w.forceFullColoring = true;
}

// A step without pairs has no schedule: what hCounters holds of one is the step's before.
static void clearSchedule(World& w)
{
	memset(w.hCounters + CTR_KEY_START, 0, sizeof(u32) * (MI_NUM_SCHEDULE_KEYS + 1));
	w.hCounters[CTR_NUM_MANIFOLDS] = 0; w.hCounters[CTR_NUM_VALID] = 0;
}

static const u32 TAIL_MAX_MANIFOLDS = 2048; // colours at the end of the schedule no larger than this go to the one-workgroup tail kernel

// The launch-per-colour sweep (the fallback of the cluster sweep and the reference it is tested against): solveOneIteration x N
// (constraints.cpp:3748-3772), per iteration all joint colours by type, then all contact colours.
static void runSolverSweep(World& w, u32 iters, u32 numColors)
{
	const u32* keyStart = w.hCounters + CTR_KEY_START;
	bool serial = numColors || w.hCounters[CTR_NUM_PAIRS] ? keyStart[4 * MI_SERIAL_COLOR + 4] > keyStart[4 * MI_SERIAL_COLOR] : false;
	u32 size[MI_MAX_COLORS] = {}, need[MI_MAX_COLORS] = {};
	for (u32 c = 0; c < numColors; ++c) { size[c] = keyStart[4 * c + 4] - keyStart[4 * c]; need[c] = (size[c] + 255) / 256; }
	// Small worlds only (every colour fits one workgroup pass or two): the whole contact sweep of an iteration is one launch of the
	// one-workgroup kernel.  On large worlds a colour step is bound by its dependent far-memory round trips (ids -> bodies -> store,
	// ~4.7 us), not by the launch, and a single workgroup sweeping the small tail colours measured SLOWER than separate launches.
	bool allSmall = numColors >= 2;
	for (u32 c = 0; c < numColors; ++c) if (size[c] > TAIL_MAX_MANIFOLDS) allSmall = false;
	const u32 firstTail = allSmall ? 0u : numColors;
	if (!numColors && !serial && !w.numJointKernels()) return;
	for (u32 it = 0; it < iters; ++it)
	{
		launch_joint_solve_iteration(w);
		if (numColors || serial) launch_solve_contacts_iteration(w, need, numColors, firstTail, serial);
	}
}

// The reference's greedy batch scheduler for W-wide SIMD solves (scheduleConstraintsSIMD, constraints.cpp:51-184), restated for the
// replay facility: constraints are dealt round-robin to four buckets; inside its bucket a constraint goes to the first open batch
// none of whose lanes shares a body with it (a static body conflicts with nothing: it is replaced by the constraint's other body
// for the test), into that batch's lowest free lane; a batch that fills up is emitted at once, the partly filled ones follow bucket
// by bucket at the end.  Contacts are enumerated the way the reference emits them: manifold by manifold in narrowphase order, a
// manifold's contacts in order.  ids = the schedule's id quads {body a, body b, contacts, narrowphase slot} by schedule position.
// Result: replay.host = entries (position | contact << 28, 0xFFFFFFFF = empty lane), MI_REPLAY_WIDTH per batch.
u32 World::scheduleReferenceBatches(const std::vector<uint4>& ids, u32 numPositions)
{
	const u32 W = MI_REPLAY_WIDTH, NONE = 0xFFFFFFFFu, numBuckets = 4, dummy = nb;
	std::vector<u32> bySlot(numPositions);
	for (u32 i = 0; i < numPositions; ++i) bySlot[i] = i;
	std::sort(bySlot.begin(), bySlot.end(), [&](u32 x, u32 y) { return ids[x].w < ids[y].w; });
	struct Batch { u32 a[MI_REPLAY_WIDTH], b[MI_REPLAY_WIDTH], entry[MI_REPLAY_WIDTH]; };
	auto emptyBatch = [&]() { Batch e; for (u32 l = 0; l < W; ++l) { e.a[l] = e.b[l] = NONE; e.entry[l] = NONE; } return e; };
	std::vector<Batch> open[numBuckets];
	u32 count[numBuckets] = { 0, 0, 0, 0 };
	for (u32 q = 0; q < numBuckets; ++q) open[q].push_back(emptyBatch()); // the always-accepting batch behind the last open one
	replay.host.clear();
	auto emit = [&](const Batch& e) { for (u32 l = 0; l < W; ++l) replay.host.push_back(e.entry[l]); };
	u32 index = 0;
	for (u32 p : bySlot)
		for (u32 k = 0; k < ids[p].z; ++k, ++index)
		{
			const u32 bodyA = ids[p].x, bodyB = ids[p].y;
			const u32 testA = bodyA == dummy ? bodyB : bodyA, testB = bodyB == dummy ? bodyA : bodyB;
			std::vector<Batch>& es = open[index % numBuckets];
			u32 j = 0;
			for (;; ++j)
			{
				const Batch& e = es[j];
				bool conflict = false;
				for (u32 l = 0; l < W && !conflict; ++l) conflict = e.a[l] == testA || e.b[l] == testA || e.a[l] == testB || e.b[l] == testB;
				if (!conflict) break;
			}
			Batch& e = es[j];
			u32 lane = 0;
			while (!(e.a[lane] == NONE && e.b[lane] == NONE)) ++lane;
			e.entry[lane] = p | (k << 28); e.a[lane] = bodyA; e.b[lane] = bodyB;
			u32& c = count[index % numBuckets];
			if (j == c) { ++c; if (es.size() <= c) es.push_back(emptyBatch()); else es[c] = emptyBatch(); }
			else if (lane == W - 1) { Batch full = e; --c; es[j] = es[c]; emit(full); es[c] = emptyBatch(); }
		}
	for (u32 q = 0; q < numBuckets; ++q) for (u32 i = 0; i < count[q]; ++i) emit(open[q][i]);
	return (u32)(replay.host.size() / W);
}

// Global colouring + rows + the launch sweep: the whole solver stage of a step on the fallback path.
static void solveWithLaunchSweep(World& w, u32 numPairs, float dt, u32 iters)
{
	u32 numColors = 0;
	if (numPairs)
	{
		for (u32 attempt = 0; ; ++attempt)
		{
			launch_coloring(w, numPairs);
			readCounters(w);                               // sync #2: colour boundaries of the contact schedule
			// Manifolds the round budget left uncoloured sit in a serial bucket that ONE wave sweeps (correct, and fine for a handful).
			// A colouring from scratch on a short budget can leave thousands there (measured: 4 ms per iteration on config 3): colour
			// again from scratch with four times the rounds instead (a round is one 5 us launch).
			if (w.hCounters[CTR_OVERFLOW] <= 64u || attempt >= 3u) break;
			w.coloringRounds = std::min(1024u, std::max(w.coloringRounds, 16u) * 4u);
			colorFromScratch(w);
		}
		numColors = w.hCounters[CTR_NUM_COLORS];
		w.lastNumManifolds = w.hCounters[CTR_NUM_MANIFOLDS];
		// adaptive colouring budget: last round that made progress + margin; grow quickly on overflow
		u32 lastUseful = w.hCounters[CTR_LAST_ROUND];
		w.coloringRounds = w.hCounters[CTR_OVERFLOW] ? std::min(1024u, w.coloringRounds * 2) : std::max(12u, lastUseful + 6);
	}
	else { clearSchedule(w); w.lastNumManifolds = 0; }
	launch_contact_init(w, numPairs, dt);
	launch_joint_init(w, dt);
	if (w.replay.referenceOrder) // the reference's batch order instead of the colour schedule (debug facility: one workgroup sweeps all contacts)
	{
		const u32 numPositions = numPairs ? w.hCounters[CTR_NUM_MANIFOLDS] : 0u;
		std::vector<uint4> ids(numPositions);
		if (numPositions) { MI_CHECK(hipMemcpyAsync(ids.data(), w.rowIds.p, sizeof(uint4) * numPositions, hipMemcpyDeviceToHost, w.stream)); MI_CHECK(hipStreamSynchronize(w.stream)); }
		w.replay.batches = w.scheduleReferenceBatches(ids, numPositions);
		w.replay.entries.ensure(std::max<size_t>(w.replay.host.size(), 1), w.stream);
		if (w.lastError) return;
		if (!w.replay.host.empty()) MI_CHECK(hipMemcpyAsync(w.replay.entries.p, w.replay.host.data(), sizeof(u32) * w.replay.host.size(), hipMemcpyHostToDevice, w.stream));
		for (u32 it = 0; it < iters; ++it) { launch_joint_solve_iteration(w); launch_solve_replay(w, w.replay.batches); } // joints before contacts (constraints.cpp:3748-3772)
		return;
	}
	runSolverSweep(w, iters, numColors);
}

// The cluster sweep of the last step gave up (CTR_FLOW_STATUS != 0: a task did not fit its tables or LDS, more tasks than
// workgroups, or — only when the GPU is shared with another persistent kernel — a lane timed out waiting for a body): its
// velocities are garbage and k_integrate_velocities skipped itself.  The manifolds of that step are in place (when the give-up is
// noticed at the next step's first synchronisation, stepInternal has just launched that step's narrowphase again, with that step's
// sorting axis): restore the pre-solve velocities, colour globally, rebuild the rows in that order, run joints + contacts as
// launches, integrate.  The cluster sweep then stays off for a while.
void World::recoverFlow()
{
	stats.numFlowRecoveries++;
	// why: bit 6 = the cluster build did not fit (too many tasks in a phase, a task beyond the colouring tables or LDS): try again soon;
	// anything else = a lane timed out (GPU shared with another persistent kernel): stay away for a while
	u32 why = hCounters[CTR_FLOW_STATUS];
	if (getenv("MI_CLUSTER_DEBUG"))
	{
		// (a fresh copy: hCounters is one step old when the give-up is noticed outside a step, and nothing of the next step's setup has run yet)
		std::vector<u32> c(CTR_WORDS);
		(void)hipMemcpyAsync(c.data(), dCounters.p, CTR_WORDS * sizeof(u32), hipMemcpyDeviceToHost, stream);
		(void)hipStreamSynchronize(stream);
		fprintf(stderr, "[mi_physics] step %u: cluster sweep gave up: status %u, build status %u, parts %u, tasks %u %u %u %u %u, manifolds %u %u %u %u %u (active %u), remain %u %u %u %u %u; components: listed %u tasks %u weight %u ends disagree %u largest too-big %u; scratch rows %u\n", stats.numInternalSteps, c[CTR_FLOW_STATUS] | why,
			c[CTR_CL_STATUS], CL_CURVE_PARTS, c[CTR_CL_NUM_TASKS], c[CTR_CL_NUM_TASKS + 1], c[CTR_CL_NUM_TASKS + 2], c[CTR_CL_NUM_TASKS + 3], c[CTR_CL_NUM_TASKS + 4],
			c[CTR_CL_PHASE_COUNT], c[CTR_CL_PHASE_COUNT + 1], c[CTR_CL_PHASE_COUNT + 2], c[CTR_CL_PHASE_COUNT + 3], c[CTR_CL_PHASE_COUNT + 4], c[CTR_NUM_ACTIVE],
			c[CTR_CL_REMAIN + 1], c[CTR_CL_REMAIN + 2], c[CTR_CL_REMAIN + 3], c[CTR_CL_REMAIN + 4], c[CTR_CL_REMAIN + 5],
			c[CTR_CL_LEFT], c[CTR_CL_LEFT + 1], c[CTR_CL_LEFT + 2], c[CTR_CL_LEFT + 3], c[CTR_CL_LEFT + 4], c[CTR_CL_SCRATCH]);
	}
	// (a world that keeps not fitting backs off: 4, 8, ... 256 steps of launch sweep between attempts)
	if ((why & 64u) && !(why & 1u)) { cluster.cooldown = std::min(256u, 4u << std::min(cluster.failStreak, 6u)); ++cluster.failStreak; }
	else cluster.cooldown = 256;
	coloringRounds = 64;
	MI_CHECK(hipMemsetAsync(dCounters.p + CTR_FLOW_STATUS, 0, sizeof(u32), stream));
	launch_restore_velocities(*this); // (the simulated bodies': the backup holds nothing of the others)
	colorFromScratch(*this);
	solveWithLaunchSweep(*this, last.numPairs, last.dt, last.iters);
	launch_integrate_velocities(*this, last.dt);
	launch_cloth_collide(*this);      // the step's own pass skipped itself on the status word, as the integration did (it runs before the next step's cloth kernel either way)
	last.cluster = false;
	if (last.jointPath != MI_JOINT_PATH_NONE) last.jointPath = MI_JOINT_PATH_LAUNCH_SWEEP;
}

// Before the host looks at results: has the last step's cluster sweep completed?  (One extra 4-byte read, only after a cluster step.)
int World::resolvePendingFlow()
{
	if (!last.unsettled) return lastError;
	last.unsettled = false;
	u32 status = 0;
	MI_CHECK(hipMemcpyAsync(&status, dCounters.p + CTR_FLOW_STATUS, sizeof(u32), hipMemcpyDeviceToHost, stream));
	MI_CHECK(hipStreamSynchronize(stream));
	if (status)
	{
		hCounters[CTR_FLOW_STATUS] = status;
		recoverFlow();
		MI_CHECK(hipStreamSynchronize(stream));
	}
	return lastError;
}

void World::harvestTiming()
{
	if (!timing.ringPending) return;
	MI_CHECK(hipStreamSynchronize(stream));
	for (u32 k = 0; k < timing.ringPending; ++k)
	{
		u32 slot = (timing.ringHead + STAGE_RING - timing.ringPending + k) % STAGE_RING;
		for (int i = 0; i < 5; ++i) { float ms = 0.f; (void)hipEventElapsedTime(&ms, timing.stageEvents[slot * 6 + i], timing.stageEvents[slot * 6 + i + 1]); timing.accMs[i] += ms; }
		timing.accTimed++;
	}
	timing.ringPending = 0;
}

// hCounters holds the colour / manifold / contact counts of the step before the current one whenever the host has just read the
// counters at a step's first synchronisation: add them to the running sums once.
void World::countPreviousStep()
{
	if (last.counted) return;
	last.counted = true;
	const bool had = last.numPairs != 0, hadCluster = had && last.cluster;
	stats.numCollisions = had ? hCounters[CTR_NUM_MANIFOLDS] : 0; stats.numContacts = had ? hCounters[CTR_NUM_CONTACTS] : 0;
	stats.numColors = had ? hCounters[CTR_NUM_COLORS] : 0; stats.flowProbes = hCounters[CTR_FLOW_PROBES];
	stats.numBroadphaseOverlaps = last.truePairs;
	lastNumManifolds = stats.numCollisions;
	for (u32 p = 0; p < 5; ++p)
	{
		stats.clusterTasks[p] = hadCluster ? hCounters[CTR_CL_NUM_TASKS + p] : 0;
		stats.clusterManifolds[p] = hadCluster ? hCounters[CTR_CL_PHASE_COUNT + p] : 0;
	}
	stats.clusterSharedBodies = hadCluster ? hCounters[CTR_CL_SHARED] : 0; stats.clusterParts = last.cluster ? CL_CURVE_PARTS : 0;
	if (hadCluster) cluster.failStreak = 0; // (a give-up never gets here: recoverFlow clears last.cluster)
	cluster.compIdle = hadCluster && hCounters[CTR_CL_LEFT] == 0u && hCounters[CTR_CL_PHASE_COUNT + CL_MAX_PARTS] == 0u;
	if (hadCluster && (stats.numInternalSteps % 50u) == 0u && getenv("MI_CLUSTER_DEBUG"))
		fprintf(stderr, "[mi_physics] step %u: component phase: %u manifolds left by the curve phases, %u tasks, weight %u, %u with ends in different components after the rounds, largest component sent to the rest task %u\n", stats.numInternalSteps,
			hCounters[CTR_CL_LEFT], hCounters[CTR_CL_LEFT + 1], hCounters[CTR_CL_LEFT + 2], hCounters[CTR_CL_LEFT + 3], hCounters[CTR_CL_LEFT + 4]);
	timing.sumContacts += stats.numContacts; timing.sumManifolds += stats.numCollisions; timing.sumColors += stats.numColors; timing.sumPairs += last.truePairs; timing.sumProbes += stats.flowProbes; timing.sumSteps++;
}

// Bring hCounters (and the statistics) up to date with the device: needed by whoever looks at the last step's schedule or counts
// when the step did not read the colour table back itself.
void World::refreshCounters()
{
	if (last.counted) return;
	resolvePendingFlow();
	readCounters(*this);
	if (!last.numPairs) { clearSchedule(*this); hCounters[CTR_NUM_COLORS] = 0; }
	hCounters[CTR_NUM_PAIRS] = last.truePairs; // (the pair count of the finished step; the device word is the same until the next broadphase)
	if (hCounters[CTR_VALIDATE]) fail(MI_ERR_INVALID_STATE, "non-finite values in the last step (debug guard): " + std::to_string(hCounters[CTR_VALIDATE]) + " elements, first code " + std::to_string(hCounters[CTR_VALIDATE + 1]));
	countPreviousStep();
}

// ---- the phases of World::stepInternal, in stream order ---------------------------------------------------------------
// Stage timing: this step's six events of the ring, the first one recorded; nullptr while timing is off.
static hipEvent_t* beginStageTiming(World& w)
{
	if (!w.timing.timeStages) return nullptr;
	if (w.timing.ringPending == World::STAGE_RING) w.harvestTiming();
	hipEvent_t* ev = &w.timing.stageEvents[w.timing.ringHead * 6];
	w.timing.ringHead = (w.timing.ringHead + 1) % World::STAGE_RING; w.timing.ringPending++;
	MI_CHECK(hipEventRecord(ev[0], w.stream));
	return ev;
}
static void stamp(World& w, hipEvent_t* ev, u32 stage) { if (ev) MI_CHECK(hipEventRecord(ev[stage], w.stream)); }

// Colliders, pair count, and the step's one host read: the pair count (it sizes buffers and launches), with it the previous step's
// counts and status words.  The copy is asynchronous; while it is on its way the device is given work that does not need the host's
// knowledge of the count: the pair list and the narrowphase, launched for the previous step's count plus a margin (their kernels
// take the real count from the device and ignore the surplus).  If the count turns out larger than that, or a collider outgrew its
// pair slab this step, both are launched again with the right size — a repeated narrowphase in the rare step where the pile jumps.
// Returns whether that early launch was made, `guess` = the count it was made for.
static bool launchStepStart(World& w, hipEvent_t* ev, u32& guess)
{
	launch_build_colliders(w);
	launch_validate(w, 0, 0);
	launch_broadphase_count(w);
	MI_CHECK(hipMemcpyAsync(w.hCounters, w.dCounters.p, CTR_WORDS * sizeof(u32), hipMemcpyDeviceToHost, w.stream));
	MI_CHECK(hipEventRecord(w.countersEvent, w.stream));
	if (!w.last.truePairs || w.validate) return false;
	guess = w.last.truePairs + w.last.truePairs / 8u + 4096u;
	if ((size_t)guess + w.terrain.slotCap((u32)w.colliders.size()) > w.pairCap) return false;
	launch_broadphase_write(w, guess, w.last.slabOverflow);
	stamp(w, ev, 1);
	launch_narrowphase(w, guess, w.stats.numInternalSteps & 1u, true); // (its side chain: launchCollisionStages, if this launch stands)
	return true;
}

// The counters are on the host: settle the previous step with them (a give-up of its cluster sweep, its counts) and see whether
// this step's start has to be run again.  False: the world has failed.
static bool settlePreviousStep(World& w, bool& early)
{
	const u32* hc = w.hCounters;
	w.last.unsettled = false;
	if (hc[CTR_FLOW_STATUS])                               // the cluster sweep of the previous step gave up
	{
		if (early)
		{
			// The early pair list + narrowphase just launched overwrote the previous step's pairs and manifolds.  The poses have not
			// moved since (that step's integration skipped itself), so the broadphase in the buffers is the previous step's: write its
			// pair list and run its narrowphase again, with ITS sorting axis.  This step's pair count has put the axis of step + 1 into
			// the word of the previous step's parity; the previous step's own axis is put back from the host (the word is written
			// again when this step's start is run again below).
			const u32 prevParity = (w.stats.numInternalSteps - 1u) & 1u;
			MI_CHECK(hipMemsetD32Async((hipDeviceptr_t)(w.dCounters.p + CTR_SAP_AXIS + prevParity), (int)w.last.axis, 1, w.stream));
			launch_broadphase_write(w, w.last.truePairs, w.last.slabOverflow);
			launch_narrowphase(w, w.last.truePairs, prevParity);
		}
		w.recoverFlow();                                   // redo the previous step's solve + integration with the launch sweep (synchronises)
		restartStepStart(w, early);                        // ... which moved the poses this step's start had read
	}
	w.estActiveBodies = hc[CTR_ACTIVE_BODIES]; w.estActiveCols = hc[CTR_ACTIVE_COLS]; // lengths of the active lists: size the next launches
	// More active colliders than the pair kernels were laid out for (the lists grew by more than 12 % in one step).  The first count
	// consumed the cell size and the bucket sizes: rebuild them (the lists are current) and count with the right bound.
	if (hc[CTR_ACTIVE_OVERFLOW]) restartStepStart(w, early);
	if (hc[CTR_VALIDATE])                                  // the debug guard found NaN / Inf in the previous step (or in this step's colliders)
	{
		static const char* stageName[4] = { "world-space colliders / boxes", "contacts", "body update records (centre of gravity, inverse inertia, velocities)", "poses / velocities after the step" };
		u32 first = hc[CTR_VALIDATE + 1];
		w.fail(MI_ERR_INVALID_STATE, "non-finite values in " + std::string(stageName[(first >> 28) & 3u]) + ": " + std::to_string(hc[CTR_VALIDATE]) + " elements, first at index " + std::to_string(first & 0x0FFFFFFFu));
		return false;
	}
	w.countPreviousStep();                                 // the counters just read hold the previous step's colour / contact counts
	if (hc[CTR_TERRAIN_OVERFLOW]) { w.fail(MI_ERR_CAPACITY, "more terrain contacts than manifold slots: contacts were dropped (raise MI_TERRAIN_SLOTS_PER_COLLIDER)"); return false; }
	if (hc[CTR_EVENT_OVERFLOW] & 2u) { w.fail(MI_ERR_CAPACITY, "a trigger / collision overlap set was full: events of the last step were lost"); return false; }
	return true;
}

// Buffers for this step's pair count, then the pair list + narrowphase unless the early launch stands, and the stages that hang on
// the narrowphase.  False: an allocation failed, and nothing of this step may touch the pair buffers.
static bool launchCollisionStages(World& w, hipEvent_t* ev, const StepRecord& cur, bool early, u32 guess)
{
	ensurePairBuffers(w, cur.numPairs);
	w.ensureEventBuffers(cur.numPairs);
	if (w.lastError) return false;
	if (!early)
	{
		launch_broadphase_write(w, cur.truePairs, cur.slabOverflow);
		stamp(w, ev, 1);
		launch_narrowphase(w, cur.truePairs, w.stats.numInternalSteps & 1u);
	}
	else launch_narrow_side(w);                            // the early launch stands: its side-stream chain and the join
	launch_zone_overlap(w, early ? guess : cur.truePairs);
	launch_heightmap(w, cur.truePairs, cur.numPairs);      // physics.cpp:1236-1249
	launch_trigger_events(w);                              // physics.cpp:1255 (handleNonCollisionInteractions)
	launch_validate(w, 1, cur.numPairs);
	stamp(w, ev, 2);
	return true;
}

// Force fields and force integration up to the solve.  False: an allocation failed.
static bool launchForceStages(World& w, const StepRecord& cur)
{
	launch_apply_fields(w);                                // :963-967, :1273
	if (cur.cluster) { w.cluster.velBackup.ensure(2 * ((size_t)w.nb + 1), w.stream); if (w.lastError) return false; } // (a failed allocation leaves the old, smaller buffer)
	launch_integrate_forces(w, cur.dt, cur.cluster);       // a cluster step keeps its pre-solve velocities, in case it has to be redone (World::recoverFlow)
	launch_validate(w, 2, 0);
	launch_collision_events(w, cur.numPairs);              // :1284 (handleCollisionCallbacks: after the force integration)
	return true;
}

// Contact + joint solver of the step: the LDS cluster sweep (one persistent launch, no host synchronisation: everything is sized on
// the device), or global colouring + one launch per colour.
static void launchSolve(World& w, hipEvent_t* ev, const StepRecord& cur)
{
	if (!cur.cluster)
	{
		solveWithLaunchSweep(w, cur.numPairs, cur.dt, cur.iters);
		stamp(w, ev, 3); // (the launch sweep is enqueued behind its own synchronisation: setup and solve are not separated here)
		return;
	}
	launch_cluster_build(w, cur.numPairs);
	launch_contact_init(w, cur.numPairs, cur.dt);
	launch_joint_init(w, cur.dt);
	stamp(w, ev, 3);
	w.forceFullColoring = true;
	if (!w.numJointKernels() || cluster_solves_joints(w)) launch_cluster_solve(w, 0, cur.iters);
	else for (u32 it = 0; it < cur.iters; ++it) { launch_joint_solve_iteration(w); launch_cluster_solve(w, it, it + 1); } // joints before contacts in every iteration (constraints.cpp:3748-3772)
}

int World::stepInternal(float dt, u32 iters)
{
	g_currentWorld = this;
	if (lastError) return lastError;
	upload(); uploadJoints();
	if (lastError) return lastError;
	if (!nb) return MI_OK;
	iterations = iters;
	hipEvent_t* ev = beginStageTiming(*this);

	u32 guess = 0;
	bool early = launchStepStart(*this, ev, guess);
	MI_CHECK(hipEventSynchronize(countersEvent));          // sync #1: number of overlapping pairs
	if (!settlePreviousStep(*this, early)) return lastError;

	StepRecord cur;                                        // this step; it becomes `last` below
	cur.dt = dt; cur.iters = iters; cur.bodies = nb;
	cur.axis = hCounters[CTR_SAP_AXIS + (stats.numInternalSteps & 1u)]; // (written by the previous step's broadphase: kept for a recovery at the next step)
	cur.truePairs = hCounters[CTR_NUM_PAIRS];
	cur.slabOverflow = hCounters[CTR_PAIR_OVERFLOW] != 0u;
	cur.numPairs = cur.truePairs + terrain.slotCap((u32)colliders.size());
	if (early && (cur.truePairs > guess || (cur.slabOverflow && !last.slabOverflow))) { early = false; stats.numNarrowphaseRedone++; }
	if (!launchCollisionStages(*this, ev, cur, early, guess)) return lastError;

	if (cluster.cooldown) --cluster.cooldown;
	// (the launch sweep when the cluster sweep is switched off, recovering, or cannot hold the turn counters)
	cur.cluster = cluster.enabled && !replay.referenceOrder && !cluster.cooldown && cur.numPairs && iters && iters < 4096u && cluster_available(*this);
	cur.unsettled = cur.cluster;
	cur.jointPath = !numSortedJoints() ? MI_JOINT_PATH_NONE : !cur.cluster ? MI_JOINT_PATH_LAUNCH_SWEEP : (cluster_solves_joints(*this) ? MI_JOINT_PATH_CLUSTER : MI_JOINT_PATH_INTERLEAVED);
	cur.counted = false;
	if (!launchForceStages(*this, cur)) return lastError;
	launchSolve(*this, ev, cur);
	stamp(*this, ev, 4);
	last = cur;                                            // the one place the record is written: from here on "the last step" is this one

	launch_integrate_velocities(*this, dt);
	launch_validate(*this, 3, 0);
	launch_cloth(*this, dt);                               // physics.cpp:1354-1358
	launch_cloth_collide(*this);                           // mi_cloth_set_collision: nothing unless a cloth has it on
	stamp(*this, ev, 5);

	stats.numRigidBodies = nb; stats.numColliders = nc; stats.numJoints = numSortedJoints(); stats.coloringRounds = coloringRounds;
	stats.numInternalSteps++;
	if (!last.cluster) countPreviousStep(); // this step's counts are on the host already (hCounters comes from its own second read)
	return lastError;
}

// physicsStep — reference physics.cpp:1364-1413
int World::step(float* timer, const mi_physics_settings* s, float dt)
{
	g_currentWorld = this;
	upload(); uploadJoints();
	if (lastError) return lastError;
	cloth.iterations[0] = s->numClothVelocityIterations; cloth.iterations[1] = s->numClothPositionIterations; cloth.iterations[2] = s->numClothDriftIterations;
	if (s->fixedFrameRate)
	{
		const float fixedDt = 1.f / (float)s->frameRate;
		*timer += dt;
		u32 physicsIterations = 0;
		if (*timer >= fixedDt)
		{
			launch_copy_pose0(*this);
			while (*timer >= fixedDt && physicsIterations++ < s->maxPhysicsIterationsPerFrame)
			{
				int e = stepInternal(fixedDt, s->numRigidSolverIterations);
				if (e) return e;
				*timer -= fixedDt;
			}
		}
		if (*timer >= fixedDt) *timer = fmodf(*timer, fixedDt);
		resolvePendingFlow(); // the interpolation reads the final poses
		launch_lerp_pose(*this, *timer / fixedDt);
	}
	else
	{
		int e = stepInternal(dt, s->numRigidSolverIterations);
		if (e) return e;
		if (nb) MI_CHECK(hipMemcpyAsync(poseLerp.p, pose.p, sizeof(float4) * 2 * nb, hipMemcpyDeviceToDevice, stream));
	}
	return lastError;
}
