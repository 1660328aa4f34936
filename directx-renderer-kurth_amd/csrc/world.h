// Host-side World of the MI355X rigid-body stepper: owns the SoA device buffers (HBM layout in DESIGN.md), one HIP
// stream (plus a side stream that only the narrowphase forks to and joins from), and the per-step launch sequence.  The C-ABI in include/mi_physics.h is a thin shell over this class.
#pragma once
#include "mi_common.h"
#include "../../include/mi_physics.h"
#include <vector>
#include <string>
#include <algorithm>
#include <type_traits>

// ---- persistent joint PODs: byte-for-byte the reference's structs (constraints.h:73-80,129-135,175-183,229-257,346-380,497-520)
struct mi_distance_constraint { float localAnchorA[3], localAnchorB[3], globalLength; };
struct mi_ball_constraint { float localAnchorA[3], localAnchorB[3]; };
struct mi_fixed_constraint { float initialInvRotationDifference[4], localAnchorA[3], localAnchorB[3]; };
struct mi_hinge_constraint
{
	float localAnchorA[3], localAnchorB[3], localHingeAxisA[3], localHingeAxisB[3];
	float minRotationLimit, maxRotationLimit, maxMotorTorque; u32 motorType; float motorVelocity;
	float localHingeTangentA[3], localHingeBitangentA[3], localHingeTangentB[3];
};
struct mi_cone_twist_constraint
{
	float localAnchorA[3], localAnchorB[3], localLimitAxisA[3], localLimitAxisB[3];
	float localLimitTangentA[3], localLimitBitangentA[3], localLimitTangentB[3];
	float swingLimit, twistLimit; u32 swingMotorType; float swingMotorVelocity, maxSwingMotorTorque, swingMotorAxis;
	u32 twistMotorType; float twistMotorVelocity, maxTwistMotorTorque;
};
struct mi_slider_constraint
{
	float initialInvRotationDifference[4], localAnchorA[3], localAnchorB[3], localAxisA[3];
	float negDistanceLimit, posDistanceLimit, maxMotorForce; u32 motorType; float motorVelocity;
};
static_assert(sizeof(mi_distance_constraint) == 28 && sizeof(mi_ball_constraint) == 24 && sizeof(mi_fixed_constraint) == 40, "POD layout");
static_assert(sizeof(mi_hinge_constraint) == 104 && sizeof(mi_cone_twist_constraint) == 120 && sizeof(mi_slider_constraint) == 72, "POD layout");

static const u32 MI_JOINT_TYPES = 6;
static const u32 MI_JOINT_POD_SIZE[MI_JOINT_TYPES] = { 28, 24, 40, 104, 120, 72 };
// Per-joint solver scratch ("update" record) in floats, by type; laid out by the kernels in k_joints.hip.
static const u32 MI_JOINT_UPDATE_FLOATS[MI_JOINT_TYPES] = { 20, 20, 36, 56, 80, 72 };

// A device buffer and its owner: freed when it goes out of scope (after the World's destructor body has drained both streams), so a
// buffer is a member and nothing else; never copied.
template <typename T> struct DevBuf
{
	T* p = nullptr; size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { if (p) (void)hipFree(p); }
	void ensure(size_t n, hipStream_t s, bool keep = false);
	void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } } // (the status is ignored: nothing can be done about it)
};
static_assert(!std::is_copy_constructible<DevBuf<u32>>::value && !std::is_copy_assignable<DevBuf<u32>>::value, "DevBuf owns its memory");

struct JointSet
{
	std::vector<uint8_t> pods;            // host, add order
	std::vector<u32> a, b;                // body ids
	std::vector<uint8_t> alive;
	// colour-sorted device view
	DevBuf<uint8_t> dPods; DevBuf<uint2> dPairs; DevBuf<float> dUpdate;
	std::vector<u32> order;               // sorted slot -> joint id
	std::vector<u32> colorStart;          // size numColors+1
	u32 count() const { return (u32)a.size(); }
	u32 numColors() const { return colorStart.empty() ? 0u : (u32)colorStart.size() - 1u; } // = kernels per solver iteration
};

// Device-side step counters (u32 words of World::dCounters), copied to pinned host memory twice per step.  The offsets are part of
// the snapshot / inspection contract (and of the compiled kernels): a new entry takes a free word, nothing moves.  CTR_LAYOUT below
// holds every entry's extent and is checked at compile time.
enum
{
	CTR_NUM_PAIRS = 0,      // broadphase overlaps
	CTR_NUM_VALID = 1,      // candidate pairs that survive prune/classify (= manifold slots)
	CTR_NUM_MANIFOLDS = 2,  // slots with >= 1 contact
	CTR_EPA_COUNT = 3,      // GJK hits waiting for EPA
	CTR_NUM_COLORS = 4,
	CTR_FIRST_LARGE = 5,    // sorted position of the first "large" collider
	CTR_LAST_ROUND = 6,     // last colouring round that coloured anything
	CTR_OVERFLOW = 7,       // manifolds sent to the serial bucket because the round budget ran out
	CTR_CELL_SIZE = 8,      // float bits: largest extent of a collider riding on a rigid body
	CTR_NUM_ACTIVE = 9,     // append cursor of the active-manifold list
	CTR_NUM_CONTACTS = 10,  // sum of contact counts over the active manifolds
	CTR_PAIR_OVERFLOW = 11, // some collider has more broadphase partners than its slab holds
	CTR_FIRST_INACTIVE = 12,// sorted position of the first collider whose body is simulated by another GPU
	CTR_FLOW_STATUS = 13,   // cluster sweep: non-zero = the launch could not run or a lane gave up waiting (result invalid): the host redoes the step
	CTR_FLOW_PROBES = 14,   // always 0: no kernel counts probes any more; the word stays because mi_stats.flowProbes reports it (ABI)
	CTR_EPA_COUNT_HULL = 15,// GJK hits among the hull pairs (their EPA work list grows from the end of epaList)
	CTR_BUCKET_START = 16,  // 65 words: first slot of narrowphase bucket key b (narrow.h: pairKey, KEY_ZONE, KEY_INVALID); [64] unused
	CTR_KEY_START = 96,     // (MI_MAX_COLORS+1)*4 + 1 words: first schedule slot of key colour*4 + (4-count); last = numManifolds
	CTR_COLOR_BARRIER = 360,// 4 words: grid barrier of the fused colouring kernel (arrivals, 3 x manifolds left)
	CTR_SAP_AXIS = 368,     // 2 words: the reference sweep's sorting axis (collision_broad.cpp:443-444) for internal step k at [k & 1]: written by step k - 1 from its AABB centres, read by k_classify
	CTR_CL_SCRATCH = 371,   // cluster sweep: append cursor of the global row scratch (contacts that fit neither registers nor LDS), reset before every launch
	CTR_CL_LEFT = 372,      // 5 words: cluster build: manifolds left over by the curve phases (cursor of the list the component phase works on); statistics of the component phase: tasks, total weight, manifolds whose ends disagree, weight of the largest component sent to the rest task
	CTR_ACTIVE_BODIES = 377, // simulated bodies / their colliders + the static ones (lengths of the active lists, k_active_scan); more of the latter than the broadphase was launched for
	CTR_ACTIVE_COLS = 378,
	CTR_ACTIVE_OVERFLOW = 379,
	CTR_CELL_SIZE_USED = 380, // float bits: the cell size the current sorted order was built with (CTR_CELL_SIZE is reset for the next step's atomicMax before the last pair kernel runs)
	CTR_EVENT_COUNT = 416,  // append cursor of the event ring (trigger enter/leave, collision begin/end), reset by mi_drain_events
	CTR_EVENT_OVERFLOW = 417,// bit 0: the event ring was full, events were dropped; bit 1: a pair-set table was full
	CTR_TERRAIN_BASE = 418, // first manifold slot of the terrain contacts (= number of pair manifold slots)
	CTR_TERRAIN_OVERFLOW = 419,// more terrain contacts than slots: contacts were dropped (the host fails the world)
	CTR_CL_NUM_TASKS = 424, // 5 words: cluster sweep: tasks of phase p (positions up to the last non-empty one)
	CTR_CL_STATUS = 429,    // cluster build: bit 0 = more tasks in a phase than the table holds, bit 1 = a task exceeds k_cl_color's tables
	CTR_CL_SHARED = 430,    // statistics: bodies handed between tasks (summed over tasks)
	CTR_CL_PHASE_COUNT = 431,// 5 words: statistics: manifolds per phase
	CTR_CL_BBOX = 436,      // 6 words: min xyz, max xyz of the simulated bodies' centres of gravity (order-preserving integer encoding)
	CTR_CL_REMAIN = 442,    // 6 words: manifolds still unassigned when partition phase p starts ([0] unused: all active ones)
	CTR_VALIDATE = 448,     // 2 words: non-finite values found by the debug guard (MI_PHYSICS_VALIDATE=1), first offender (stage << 28 | index)
	CTR_NARROW_LIMITS = 450,// 5 words: high-water marks of the GJK / EPA caps since the world was created (k_gjk, k_epa): GJK iterations, EPA triangles, edges, border edges; EPA runs that left through an out-of-memory exit (mi_debug_narrow_limits)
	CTR_CL_COLOR_TASKS = 456,// 3 words: task colouring of the last step: tasks too large for the narrow instance (k_cl_offsets; the wide launch leaves at once on 0), tasks the narrow / the wide instance coloured (mi_debug_color_tasks)
	CTR_WORDS = 512,
};
struct CtrRange { u32 first, words; };
static constexpr CtrRange CTR_LAYOUT[] = // every entry of the enum, ascending
{
	{ CTR_NUM_PAIRS, 1 }, { CTR_NUM_VALID, 1 }, { CTR_NUM_MANIFOLDS, 1 }, { CTR_EPA_COUNT, 1 }, { CTR_NUM_COLORS, 1 }, { CTR_FIRST_LARGE, 1 }, { CTR_LAST_ROUND, 1 }, { CTR_OVERFLOW, 1 },
	{ CTR_CELL_SIZE, 1 }, { CTR_NUM_ACTIVE, 1 }, { CTR_NUM_CONTACTS, 1 }, { CTR_PAIR_OVERFLOW, 1 }, { CTR_FIRST_INACTIVE, 1 }, { CTR_FLOW_STATUS, 1 }, { CTR_FLOW_PROBES, 1 }, { CTR_EPA_COUNT_HULL, 1 },
	{ CTR_BUCKET_START, 65 }, { CTR_KEY_START, (MI_MAX_COLORS + 1) * 4 + 1 }, { CTR_COLOR_BARRIER, 4 }, { CTR_SAP_AXIS, 2 }, { CTR_CL_SCRATCH, 1 }, { CTR_CL_LEFT, 5 },
	{ CTR_ACTIVE_BODIES, 1 }, { CTR_ACTIVE_COLS, 1 }, { CTR_ACTIVE_OVERFLOW, 1 }, { CTR_CELL_SIZE_USED, 1 }, { CTR_EVENT_COUNT, 1 }, { CTR_EVENT_OVERFLOW, 1 }, { CTR_TERRAIN_BASE, 1 }, { CTR_TERRAIN_OVERFLOW, 1 },
	{ CTR_CL_NUM_TASKS, 5 }, { CTR_CL_STATUS, 1 }, { CTR_CL_SHARED, 1 }, { CTR_CL_PHASE_COUNT, 5 }, { CTR_CL_BBOX, 6 }, { CTR_CL_REMAIN, 6 }, { CTR_VALIDATE, 2 }, { CTR_NARROW_LIMITS, 5 }, { CTR_CL_COLOR_TASKS, 3 },
};
constexpr bool ctrLayoutDisjoint() { u32 end = 0; for (const CtrRange& r : CTR_LAYOUT) { if (r.first < end) return false; end = r.first + r.words; } return end <= CTR_WORDS; }
constexpr u32 ctrWords(u32 first) { for (const CtrRange& r : CTR_LAYOUT) if (r.first == first) return r.words; return 0; } // extent of the entry that begins at `first`
static_assert(ctrLayoutDisjoint(), "CTR_*: an entry reaches into the next one (or past CTR_WORDS), or CTR_LAYOUT is not in ascending order");
// Cluster sweep (cluster.h, k_cluster_*.hip): up to CL_MAX_PARTS partition phases + the rest phase; task key = phase * CL_MAX_TASKS + task.
#define MI_REPLAY_WIDTH 8u // lanes of the reference's SIMD batches (constraints.cpp: CONSTRAINT_SIMD_WIDTH with AVX)
#define CL_MAX_PARTS 4u
#define CL_CURVE_PARTS 2u // curve phases a step uses; the component phase comes on top (phase index CL_CURVE_PARTS)
#define CL_MAX_PHASES (CL_MAX_PARTS + 1u)
#define CL_MAX_TASKS 512u
#define CL_BODY_STRIDE 4096u
#define CL_MAX_JOINT_CLASSES 64u   // (type, colour) classes of joints the cluster sweep can run
#define CL_TASK_MAX_JOINTS 512u    // joints per task (one lane each)
#define CL_TRACE_ROWS 16u          // developer timeline (mi_debug_flow_trace): rows per task of k_cl_color and per workgroup of k_cl_solve (at most CL_MAX_TASKS of either) ...
#define CL_TRACE_WORDS 32u         // ... of this many u64 stamps each
#define MI_NUM_SCHEDULE_KEYS ((MI_MAX_COLORS + 1) * 4)

// What the host knows about the last internal step.  The step after it is launched before the host has seen how it ended, so this
// is what that step (and every entry point that synchronises in between) settles, counts or redoes it from.  Written as a whole
// by World::stepInternal once the step's solve is enqueued; afterwards only `unsettled` and `counted` are ticked off, and a
// recovery (World::recoverFlow) corrects `cluster` and `jointPath` to what finally solved the step.
struct StepRecord
{
	u32 numPairs = 0, truePairs = 0;   // bound on its manifold slots (pair slots + room for the terrain contacts) / its broadphase overlaps
	bool slabOverflow = false;         // its CTR_PAIR_OVERFLOW
	u32 axis = 0;                      // its sorting axis (CTR_SAP_AXIS of its parity): its narrowphase is run again with it before a redo
	float dt = 0.f; u32 iters = 0;     // what a redo of its solve + integration needs
	bool cluster = false;              // solved by the cluster sweep (its pre-solve velocities are in cluster.velBackup)
	bool unsettled = false;            // ... which is not yet known to have completed (CTR_FLOW_STATUS not looked at)
	u32 jointPath = MI_JOINT_PATH_NONE;// where it solved its joints (mi_debug_read_joint_update)
	bool counted = true;               // its counts are in the running sums (nothing to count before the first step)
	u32 bodies = 0;                    // the bodies it ran with: its rows name the static dummy by this index (0: no step yet; mi_contact_sensors)
};

struct World
{
	int device = 0;
	hipStream_t stream = nullptr;
	// The narrowphase's second chain (closed forms + box-box beside GJK + EPA): forked from `stream` in launch_narrowphase and joined
	// into it again by launch_narrow_side, before anything else is launched, so nothing else ever sees it.  narrowSidePairs: the
	// launch size of a side chain that launch_narrowphase left to a later launch_narrow_side (0: none owed).
	// MI_NARROW_SIDE_STREAM=0: not used, every kernel on `stream`.
	hipStream_t narrowStream = nullptr; hipEvent_t narrowFork = nullptr, narrowJoin = nullptr; bool narrowSideStream = true; u32 narrowSidePairs = 0;
	int lastError = 0; std::string lastErrorText;

	// ---- host mirrors (add API) ----
	struct HBody { float pos[3], rot[4]; float localCOG[3], invMass, invInertia[9]; float gravityFactor, linDamp, angDamp; float v[3], w[3], force[3], torque[3]; std::vector<u32> colliders; bool removed = false; };
	struct HCollider { float shape[10]; float restitution, friction, density; u32 type, body; float spos[3], srot[4]; u32 zoneType, zoneIndex; }; // zoneType: 0 none, 2 force field, 3 trigger (physics_object_type, physics.h:49-57)
	struct HField { float force[3]; float pos[3], rot[4]; u32 hasTransform, numColliders; };   // force_field_component (physics.h:182-185) + the entity's transform
	struct HTrigger { float pos[3], rot[4]; u32 numColliders; };                                 // trigger_component (physics.h:200-203); the callback becomes mi_drain_events
	hipEvent_t countersEvent = nullptr;   // behind the step's asynchronous read of the counters
	// cloth_component (cloth.h:5-60): parameters + host mirror of the particle state (authoritative until the first step; refreshed by downloadCloths)
	struct HClothConstraint { u32 a, b; float restDistance, inverseMassSum; u32 color; };
	struct HCloth
	{
		float width, height, totalMass, stiffness, damping, gravityFactor, oldTotalMass, oldStiffness; u32 gridX, gridY;
		std::vector<float> pos, prev, vel, invMass;          // 3 n, 3 n, 3 n, n
		std::vector<HClothConstraint> constraints;            // sorted by colour (stable)
		bool collide = false; mi_cloth_collision collision = {}; // mi_cloth_set_collision: a parameter of the projection pass (k_cloth_collide.hip), not of the particle state
	};
	std::vector<HBody> bodies;
	std::vector<HCollider> colliders;
	struct HHull { std::vector<float> vertices; std::vector<u32> triangles; float aabbMin[3], aabbMax[3]; }; // bounding_hull_geometry (bounding_volumes.h:208-218)
	std::vector<HHull> hulls;
	JointSet joints[MI_JOINT_TYPES];
	u32 numJointKernels() const { u32 n = 0; for (const JointSet& js : joints) n += js.numColors(); return n; }      // launches of one joint iteration
	u32 numSortedJoints() const { u32 n = 0; for (const JointSet& js : joints) n += (u32)js.order.size(); return n; } // live joints (as of the last uploadJoints)
	bool topologyDirty = true;   // bodies/colliders added since last upload
	bool jointsDirty = true;
	bool stateOnDevice = false;  // device holds the authoritative pose/velocity

	// ---- device buffers of the step's own pipeline: what every file shares ----
	u32 nb = 0, nc = 0;
	DevBuf<float4> pose, pose0, poseLerp, vel, bprops, force, cog, invIw;
	DevBuf<ColliderRec> colLocal, colWorld;
	DevBuf<float4> colStaticPose, aabbMin, aabbMax;
	DevBuf<float4> hullVerts, hullInfo;   // all hull vertices (xyz); per geometry {aabbMin.xyz, firstVertex}, {aabbMax.xyz, vertexCount}
	DevBuf<uint8_t> aliveMask;            // per body: 0 = deleted (mi_delete_body); ANDed into every simulate mask handed in
	DevBuf<uint8_t> simMask;              // per body: 1 = simulated here (owned or ghost), 0 = lives on another GPU's slab
	// broadphase
	DevBuf<u32> cellCount, cellBase;      // colliders per cell bucket (+ 'large', 'simulated elsewhere'), first / end position of every bucket in the sorted order
	DevBuf<u32> hashKey, sortIdx, cellStart /* {first, end} per bucket */, pairCount, pairOffset;
	DevBuf<float4> sBox; // sorted colliders: {min.xyz, collider index} {max.xyz, cell tag} per position
	// active lists (k_bodies.hip): the simulated bodies, their colliders + the static ones, ascending; rebuilt when the simulate mask may have changed
	DevBuf<u32> actBodies, actCols, actBlockCount, actBlockBase, colBody; bool activeDirty = true; u32 estActiveBodies = 0, estActiveCols = 0, pairBound = 0, sapBlocks = 0;
	DevBuf<double> sapPartial;            // per workgroup of k_build_colliders: sum of the AABB centres (3), of their squares (3), colliders counted (1)
	DevBuf<uint2> pairs, pairSlab;
	u32 hashTableSize = 0;
	// narrowphase
	DevBuf<u32> pairKey, pairKeySorted; DevBuf<uint2> pairsSorted;
	DevBuf<ManifoldRec> manifolds;
	// colouring / solver
	DevBuf<u64> bodyMask, claim; DevBuf<u32> mColor, mKey, mKeySorted, mIdx, mOrder;
	DevBuf<uint4> actIds;                 // active manifolds: (bodyA, bodyB, count, slot)
	DevBuf<u32> epaList; DevBuf<float4> gjkSimplex; // GJK hits -> EPA work list (9 float4 per hit)
	DevBuf<float4> rowPlanes, rowShared; DevBuf<float2> rowLambda; DevBuf<uint4> rowIds;
	bool validate = false;                // MI_PHYSICS_VALIDATE=1 / mi_enable_validation: NaN / Inf guard after every stage (the reference's VALIDATE macros, physics.cpp:807-926)
	DevBuf<uint8_t> tempStorage;
	DevBuf<u32> sortHist;                 // counting sort: per-tile bucket histograms + their scan
	DevBuf<u32> dCounters; u32* hCounters = nullptr; // CTR_WORDS words each
	size_t pairCap = 0, rowCap = 0;

	// settings snapshot for the running step
	u32 iterations = 30;
	u32 coloringRounds = 24;     // adaptive: last useful round of the previous step + margin (launch-per-round colouring only)
	DevBuf<u64> colorHash[2]; u32 colorHashCur = 0, colorHashSize = 0, stepsSinceFullColoring = 0; // warm-started colouring
	bool forceFullColoring = true;
	u32 lastNumManifolds = 0;    // sizes the colouring-round launches of the next step
	mi_stats stats = {};
	StepRecord last;
	u32 jointVersion = 0;                 // bumped by every upload of the joints
	// Device-written joint PODs (mi_joint_device_pods): once a caller has the device array, JointSet::dPods is authoritative and
	// every host entry point that reads or changes JointSet::pods pulls it back first (pullJointPods).  jointGeneration changes
	// with every joint add / delete / set: the caller's pointer and slots are stale from then on.
	bool jointPodsOnDevice = false;
	u32 jointGeneration = 0;
	void pullJointPods();
	void jointsChanged();                 // jointsDirty + a new jointGeneration

	// ---- state by owner: one struct per subsystem, each naming the files that touch it ----

	// Heightmap terrain: api_scene.hip (mi_set_heightmap, mi_heightmap_*), k_heightmap.hip, terrain_shared.h, k_raycast_terrain.hip, step.hip, snapshot.hip
	struct Terrain
	{
		// heightmap_collider_component (heightmap_collider.h:127-152): chunksPerDim x chunksPerDim chunks of 129 x 129 uint16 heights
		u32 chunksPerDim = 0, slotsPerCollider = 8, minSlots = 8192; float chunkSize = 0.f, amplitude = 1.f, minCorner[3] = { 0.f, 0.f, 0.f }, material[3] = { 0.f, 0.f, 0.f };
		std::vector<uint16_t> hHeights; std::vector<u32> hValid;
		DevBuf<uint16_t> heights; DevBuf<u32> valid, counts, offsets;
		u32 slotCap(u32 numColliders) const { return chunksPerDim ? std::max(minSlots, slotsPerCollider * numColliders) : 0u; }
	} terrain;

	// Cloth: k_cloth.hip (kernels, uploadCloths, downloadCloths), k_cloth_collide.hip (the projection pass), api_scene.hip (mi_add_cloth, mi_cloth_*), step.hip, snapshot.hip
	struct Cloth
	{
		std::vector<HCloth> cloths;
		bool dirty = true, stateOnDevice = false; // dirty: the host mirror changed, upload before the next launch; onDevice: the device copy is newer than the mirror
		u32 iterations[3] = { 0, 1, 0 };  // physics_settings::numCloth{Velocity,Position,Drift}Iterations of the last mi_step (mi_set_cloth_iterations for mi_step_internal)
		DevBuf<float> planes; u32 stride = 0; // 10 planes of stride floats: position xyz, velocity xyz, previous position xyz, inverse mass
		DevBuf<uint2> ab; DevBuf<float2> restIms; DevBuf<float4> temp; DevBuf<uint8_t> descs; DevBuf<u32> list;
		u32 numSmall = 0, maxSmallParticles = 0; // cloths that fit the LDS variant come first in list
		// Collision (mi_cloth_set_collision; k_cloth_collide.hip): cloths with collision on (0: the step launches nothing for it), the pass's
		// tables {one record per colliding cloth, one {record, first particle} per 64-lane workgroup} and whether they have to be written
		// again (a setting or the particle layout changed); one word per particle of `planes`: the collider it was pushed off in the last
		// internal step (0xFFFFFFFF: none), laid out for contactsStride particles
		u32 numColliding = 0, collideBlocks = 0, collideFlags = 0, contactsStride = 0; bool collideDirty = true, collideBrute = false;
		DevBuf<uint8_t> collideDescs; DevBuf<uint2> collideBlockList; DevBuf<u32> contacts;
	} cloth;
	void uploadCloths(); void downloadCloths();

	// Spatial slab (mi_slab_*): api.hip, k_bodies.hip.  Ownership code per body, stamp of the last refresh of a ghost, this rank's interval
	struct Slab
	{
		DevBuf<uint8_t> code; DevBuf<u32> fresh; u32 rank = 0, size = 0, axis = 0, stamp = 0; float lo = 0.f, hi = 0.f, margin = 0.f;
	} slab;

	// Cluster sweep (cluster.h): k_cluster_partition.hip, k_cluster_color.hip, k_cluster_solve.hip; step.hip decides and recovers, world.hip
	// (uploadJoints) feeds the joint tables, snapshot.hip and api.hip reset and inspect
	struct Cluster
	{
		bool enabled = true;                  // MI_PHYSICS_NO_CLUSTER=1: launch-per-colour sweep only
		bool jointsEnabled = true;            // MI_CLUSTER_NO_JOINTS=1: joints keep their per-colour launches (one cluster launch per iteration then)
		u32 blocksLimit = 0, failStreak = 0, taskWeight = 64u * 1000u, taskWeightLater = 64u * 500u; // MI_CLUSTER_BLOCKS / _TASK / _TASK_LATER
		u32 taskWeightComp = 64u * 200u;      // MI_CLUSTER_TASK_COMP: the component phase's tasks, sized to fit LDS BEHIND a first task, where most of them run (profiles/sweep_comp_fit.txt)
		u32 ldsBytes = 0, blocks = 0, cooldown = 0;
		u32 regContactsCap = ~0u;             // MI_CLUSTER_REG_CONTACTS: most contacts of a workgroup's first task kept in registers (tests: where rows are stored, never what is computed)
		u32 ldsRowsCap = ~0u;                 // MI_CLUSTER_LDS_ROWS: most contact rows a workgroup keeps in LDS, the rest in the global scratch (tests: storage only, as above)
		u32 colorNarrowMax = ~0u, colorBlocksLimit = 0; // MI_CLUSTER_COLOR_NARROW_MAX: most items (manifolds + joints) of a task the narrow colouring instance takes (0: the wide kernel colours everything); MI_CLUSTER_COLOR_BLOCKS: most workgroups of the narrow launch (tests).  Dispatch only: no result depends on either
		u32 colorResident = 0, colorNarrowBlocks = 0, colorNarrowLimit = 0; // cluster_color_setup: narrow workgroups resident per compute unit, the narrow launch's grid (0: not launched), first item count that goes to the wide kernel
		bool compIdle = false;                    // the last step's curve phases left nothing over (and its rest task was empty): this step skips the component phase's launches (what is left over goes to the rest task)

		// -- the partition's private scratch: k_cluster_partition.hip alone (the joint inputs are written by World::uploadJoints) --
		bool sortDue = true; u32 sortAge = 0, sortBodies = 0; // body order along the curves: refreshed every few steps
		DevBuf<u32> keys, keysSorted, vals, sorted, rank, wsum, cum, taskKey, taskPos, taskCount;
		DevBuf<u32> jointBodyMask; bool jointListsValid = false; // per body: 1 if a joint of the sweep touches it (phase-0 bit of its phase mask); the joints' task lists of the last refresh are still good
		DevBuf<u32> compLabel, leftList;      // the component phase
		DevBuf<u32> chunk; u32 chunkJointVersion = ~0u; bool chunkWithJoints = false; // chunk of every body per curve phase, kept between re-sorts (~0u: none cut yet)
		DevBuf<u32> rep, jointTask, jointPos, jointCount; u32 numJoints = 0; // rep: island representative per body (jointed bodies must share a task)

		// -- what the partition leaves for k_cluster_color.hip and k_cluster_solve.hip --
		DevBuf<u32> phaseMask, pre, local, entry, taskStart, bodyList, sharedSlot; // entry: the contact schedule of every task (at 4 x its first manifold position): manifold position | contact << 12
		DevBuf<uint8_t> tasks;
		DevBuf<float4> rowScratch;
		// joints inside the cluster sweep: the joints of all types in (type, colour) order {type | class << 8, index in the type's
		// colour-sorted arrays, body a, body b}, and the per-step lists
		DevBuf<u32> jointStart, jointList; DevBuf<uint4> jointTable; DevBuf<uint2> taskJoints; DevBuf<u32> jointClassStart;
		u32 numJointClasses = 0; bool jointsInCluster = false; // false: more (type, colour) classes than the kernel's table: joints keep their launches
		DevBuf<u64> flow;                     // 32-byte hand-over record per (phase, shared body): two tagged 16-byte halves
		DevBuf<u64> flowTrace;                // developer timeline (mi_debug_flow_trace): CL_TRACE_WORDS x u64 per slot (a row; CL_TRACE_ROWS of them per task / workgroup), allocated on request only
		u32 flowEpoch = 0;
		// Safety net of the persistent kernels: if one gives up waiting (only possible when the GPU is shared with another persistent
		// kernel), the step's velocity integration is skipped on the device and the host redoes solve + integration with the launch
		// sweep from the saved pre-solve velocities, at the next point where it synchronises anyway.
		DevBuf<float4> velBackup; u32 flowTestAbortStep = ~0u;
	} cluster;
	void recoverFlow(); int resolvePendingFlow();

	// Force fields, triggers, events: k_events.hip (kernels, uploadFields, ensureEventBuffers), events.h, k_narrow_zone.hip, api_scene.hip, step.hip, snapshot.hip
	struct Zones
	{
		std::vector<HField> fields; std::vector<HTrigger> triggers;
		bool fieldsDirty = true;              // a force changed: re-upload the per-field world-space forces
		bool collisionBeginEvents = false, collisionEndEvents = false;
		DevBuf<float4> fieldForce;            // per field: world-space force (localized fields only; global ones are summed on the host into globalForce)
		DevBuf<u32> fieldMask; u32 fieldWords = 0; // per body: bit f set = inside localized field f this step (set by k_zone_overlap, consumed + cleared by k_apply_fields)
		float globalForce[3] = { 0.f, 0.f, 0.f }; bool anyGlobalForce = false;
		DevBuf<u64> triggerSet[2], collisionSet[2]; u32 triggerSetSize = 0, collisionSetSize = 0, triggerCur = 0, collisionCur = 0;
		DevBuf<uint8_t> eventRing; u32 eventCap = 1u << 16;
		std::vector<u64> restoredTriggerKeys, restoredCollisionKeys; // mi_world_restore: the snapshot's previous-step sets, entered when the first step sizes the tables
		std::vector<mi_event> pendingEvents;  // drained from the device, not yet handed to the caller
	} zones;
	void uploadFields(); void ensureEventBuffers(u32 numPairs);

	// World queries, rebuilt at every call: api.hip (entries, staging, buildInteractTables), k_interact.hip, k_raycast.hip, raycast_shared.h,
	// k_raycast_terrain.hip, k_raycast_sensors.hip, k_proximity.hip, k_spherecast.hip, k_overlap.hip, k_contact_query.hip, k_contact_sensors.hip
	struct Queries
	{
		// mi_test_physics_interaction_batch: colliders of every body (CSR), hull triangles as global vertex indices; rebuilt after upload()
		DevBuf<u32> bodyColStart, bodyColList; DevBuf<uint4> hullTris; DevBuf<uint2> hullTriRange; bool interactTablesValid = false;
		// mi_raycast_batch (k_raycast.hip): rebuilt at every call, read and written by nothing else.  Per collider: candidate flag + padded
		// world AABB; header words + arrival counter per internal node; Morton keys and collider indices, before and after the sort; the
		// internal nodes (64 bytes each: both children's boxes and ids); the parent of every internal node and of every sorted leaf
		DevBuf<float4> leafBox, nodes; DevBuf<u32> count, keys, keysSorted, vals, valsSorted, parentInt, parentLeaf;
		// MI_RAY_TERRAIN (k_raycast_terrain.hip): (max << 16) | min of the uint16 heights per 8 x 8-cell tile (256 per chunk) and per chunk.  Depends on the
		// heights alone (not on mi_heightmap_update's corner and amplitude): invalid after mi_set_heightmap, mi_heightmap_set_chunk and a restore
		DevBuf<u32> terrainTiles, terrainChunkRange; bool terrainTableValid = false;
		// mi_raycast_sensors (k_raycast_sensors.hip): per ray the world ray (2 x float4, used when the caller wants none back), the 32-byte
		// record k_raycast and k_rc_terrain work on (2 x float4) and the exclusion range {first, count}
		DevBuf<float4> sensorRays, sensorHits; DevBuf<uint2> sensorExclude;
		// (mi_proximity, k_proximity.hip, mi_sphere_cast_batch, k_spherecast.hip, and mi_overlap_batch, k_overlap.hip, walk the tree above and keep nothing of their own)
		// mi_contact_sensors (k_contact_sensors.hip): rebuilt at every call.  Per body of the last step {wanted by a sensor, its manifolds, its
		// first entry, fill cursor}; the entries (manifold slot << 32 | schedule position), a segment per wanted body, two per position at most;
		// the bodies whose segment one lane does not sort; {entries handed out, length of that list}
		DevBuf<uint4> csBody; DevBuf<u64> csEntries; DevBuf<u32> csLarge, csMeta;
		// mi_contact_query_batch (k_contact_query.hip): rebuilt at every call, the narrowphase of the query's own, apart from the step's.  Its
		// counter block (CTR_WORDS words in the step's layout); per query {first pair, pairs, not switched off, 0}; per pair {query, collider,
		// body, key | operand order}, the two world records in operand order, the manifold, {collider, pair} of the gather pass; the EPA work
		// list and the simplices of the GJK hits.  The per-pair buffers grow to the pair count the call reads back
		DevBuf<u32> cqCounters, cqEpaList; DevBuf<uint4> cqSeg, cqPairs; DevBuf<ColliderRec> cqCols; DevBuf<ManifoldRec> cqManifolds; DevBuf<float4> cqSimplex; DevBuf<uint2> cqSorted;
		// Staging of the queries' _host entries (api.hip, queryStaged), in bytes: the records in, the records out, the optional second output
		// (world rays, world points).  One set for all of them: every _host entry drains the world's stream before it returns
		DevBuf<uint8_t> hostIn, hostOut, hostAux;
	} queries;
	void buildInteractTables();

	// Stage timing and running sums: step.hip (harvestTiming, countPreviousStep), api.hip (mi_get_stats, mi_enable_stage_timing), world.hip
	static const u32 STAGE_RING = 32;
	struct Timing
	{
		// HIP events of the last STAGE_RING timed steps, read back without stalling every step (mi_get_stats harvests them)
		std::vector<hipEvent_t> stageEvents;  // STAGE_RING x 6
		u32 ringHead = 0, ringPending = 0, accTimed = 0; double accMs[5] = { 0, 0, 0, 0, 0 };
		bool timeStages = false;
		// Counts of the steps since the last mi_get_stats (the host learns a step's counts at its next synchronisation)
		double sumContacts = 0, sumManifolds = 0, sumColors = 0, sumPairs = 0, sumProbes = 0; u32 sumSteps = 0;
	} timing;
	void harvestTiming();
	void countPreviousStep(); void refreshCounters();

	// Replay of the reference's batch order (mi_debug_set_replay / MI_PHYSICS_REPLAY=1; a test facility: the whole contact sweep is ONE
	// workgroup): step.hip (scheduleReferenceBatches), k_solver.hip, api.hip
	struct Replay
	{
		bool referenceOrder = false; DevBuf<u32> entries; std::vector<u32> host; u32 batches = 0;
	} replay;
	u32 scheduleReferenceBatches(const std::vector<uint4>& ids, u32 numPositions);

	World(int dev);
	~World();
	void fail(int code, const std::string& what);
	void upload();
	void uploadJoints();
	void downloadState();
	int stepInternal(float dt, u32 iterations);
	int step(float* timer, const mi_physics_settings* s, float dt);
};

extern thread_local World* g_currentWorld;                 // the world MI_CHECK reports a HIP error to: set by every entry point (world.hip)
static inline u32 nextPow2(u32 v) { u32 p = 1; while (p < v) p <<= 1; return p; }
void recalculateProperties(World& w, World::HBody& rb);    // mass, centre of gravity and inertia of a body from its colliders (world.hip)
void ensurePairBuffers(World& w, size_t numPairs);         // every buffer sized by the pair count (step.hip)

// ---- launchers (one per stage; each defined next to its kernels) --------------------------------------------------
void launch_active_lists(World& w);                        // (re)builds the lists of simulated bodies / colliders if the simulate mask may have changed
void launch_restore_velocities(World& w);                  // velocities of the simulated bodies <- cluster.velBackup
u32 active_grid(u32 estimate, u32 total);
void launch_build_colliders(World& w);
void launch_broadphase_count(World& w);                    // grid build + pair count + scan; leaves numPairs in dCounters
void launch_broadphase_write(World& w, u32 numPairs, bool slabOverflow);       // slabOverflow: some collider has more partners than its slab holds (CTR_PAIR_OVERFLOW)
void launch_narrowphase(World& w, u32 numPairs, u32 stepParity, bool deferSide = false); // numPairs may exceed the device's pair count (a launch sized before the host knows it); stepParity: the internal step's k & 1 (its sorting-axis word); deferSide: the side-stream chain and the join are left to launch_narrow_side
void launch_narrow_side(World& w);                           // side chain + join that the last launch_narrowphase deferred (nothing if it deferred none): before anything else is launched on the results
void launch_zone_overlap(World& w, u32 numPairs);           // force-field / trigger overlap tests on the classified pairs (once per step)
void launch_integrate_forces(World& w, float dt, bool backupVelocities); // backupVelocities: keep the pre-solve velocities in cluster.velBackup (a cluster step)
void launch_heightmap(World& w, u32 numPairs, u32 slotCap);  // terrain contacts appended after the pair manifolds (physics.cpp:1236-1249)
void launch_cloth(World& w, float dt);                      // cloth_component::applyWindForce + simulate for every cloth (physics.cpp:1354-1358)
u32 cloth_lds_particle_limit();
void launch_cloth_collide(World& w);                        // k_cloth_collide.hip: the projection pass of the cloths with collision on, after launch_cloth (and after a recovery's integration); nothing without such a cloth
void launch_apply_fields(World& w);                        // localized + global force fields -> force accumulators (before the force integration)
void launch_trigger_events(World& w);                      // leave events + table hand-over of the trigger overlap set (after the narrowphase)
void launch_collision_events(World& w, u32 numPairs);      // begin / end events of this step's manifolds (after the force integration)
void launch_coloring(World& w, u32 numPairs);
void launch_contact_init(World& w, u32 numPairs, float dt);
void launch_solve_replay(World& w, u32 numBatches);
void launch_solve_contacts_iteration(World& w, const u32* gridBlocks, u32 numColors, u32 firstTail, bool serialBucket);
bool cluster_available(World& w);                          // sets up the cluster kernels' LDS budget once; false = this device cannot run them
void launch_active_list(World& w, u32 numPairs);           // manifolds with contacts -> actIds (no colours)
void launch_cluster_build(World& w, u32 numPairs);         // body order, tasks, local colouring, final slot order (k_cluster_partition.hip, k_cluster_color.hip)
void launch_cluster_solve(World& w, u32 itBegin, u32 itEnd); // iterations [itBegin, itEnd) of the sweep in one launch (k_cluster_solve.hip)
bool cluster_solves_joints(const World& w);                // the cluster sweep of this step runs the joints too (one launch for all iterations)
void launch_integrate_velocities(World& w, float dt);
void launch_joint_init(World& w, float dt);
void launch_joint_solve_iteration(World& w);
void launch_and_mask(World& w);
void launch_slab_classify(World& w);
void launch_slab_pack(World& w, void* left, void* right, u32 capacity);
void launch_slab_unpack(World& w, const void* left, const void* right, u32 capacity);
void launch_validate(World& w, u32 stage, u32 numPairs); // stage 0: world colliders + AABBs, 1: contacts, 2: body update records, 3: poses + velocities after the step
void launch_copy_pose0(World& w);
void launch_interaction_batch(World& w, u32 numRays, u32 firstBody, u32 bodiesPerRay, const float* dRays, int32_t* dOutBody); // k_interact.hip
void launch_raycast(World& w, u32 numRays, const float* dRays, u32 flags, mi_ray_hit* dOutHits, const uint2* dExclude = nullptr); // k_raycast.hip; dExclude: a body range per ray (mi_raycast_sensors)
enum RcBuild { RC_BUILD_NO_CANDIDATES, RC_BUILD_FAILED, RC_BUILD_DONE }; // nothing enqueued: no collider can be a candidate / w.lastError is set / the tree is on the stream
RcBuild launch_raycast_build(World& w, bool withStatic, bool brute); // k_raycast.hip: the tree in World::queries that launch_raycast, launch_proximity, launch_sphere_cast and launch_overlap walk
void launch_proximity(World& w, u32 n, const mi_proximity_query* dQueries, u32 flags, mi_proximity_reading* dOut, float* dOutWorldPoints); // k_proximity.hip
void launch_sphere_cast(World& w, u32 n, const mi_sphere_cast* dQueries, u32 flags, mi_sphere_hit* dOut, float* dOutWorldCasts); // k_spherecast.hip
void launch_overlap(World& w, u32 n, const mi_overlap_query* dQueries, u32 maxHits, u32 flags, void* dOut, float* dOutWorldShapes); // k_overlap.hip
void launch_contact_query(World& w, u32 n, const mi_overlap_query* dQueries, u32 maxHits, u32 flags, void* dOut, float* dOutWorldShapes); // k_contact_query.hip
void launch_raycast_sensors(World& w, u32 numRays, const mi_sensor_ray* dRays, u32 flags, bool terrain, mi_sensor_hit* dOutHits, float* dOutWorldRays); // k_raycast_sensors.hip
void launch_proximity_terrain(World& w, u32 n, const mi_proximity_query* dQueries, u32 flags, mi_proximity_reading* dOut); // k_proximity_terrain.hip: after launch_proximity, on its records
void launch_sphere_cast_terrain(World& w, u32 n, const mi_sphere_cast* dQueries, u32 flags, mi_sphere_hit* dOut); // k_spherecast_terrain.hip: after launch_sphere_cast, on its records
void launch_raycast_terrain(World& w, u32 numRays, const float* dRays, u32 flags, mi_ray_hit* dOutHits); // k_raycast_terrain.hip: after launch_raycast, on its records
void launch_contact_sensors(World& w, u32 numSensors, const mi_contact_sensor* dSensors, mi_contact_reading* dOut, bool withRows); // k_contact_sensors.hip
void launch_lerp_pose(World& w, float t);
void csort_pairs_u32(World& w, const u32* keys, u32* keysOut, const u32* vals, u32* valsOut, u32 n, u32 numBuckets); // stable, keys < numBuckets <= 272
void csort_pairs_u64(World& w, const u32* keys, u32* keysOut, const u64* vals, u64* valsOut, u32 n, u32 numBuckets);
