// Contact sweep around LDS-resident clusters ("K11-cluster"): the production contact solver.  This header holds what its three
// stages share — k_cluster_partition.hip (bodies -> tasks), k_cluster_color.hip (a task's body table and local colouring) and
// k_cluster_solve.hip (the sweep) — and nothing else; what one stage alone uses is defined there, next to its first use.
//
// Why.  A Gauss-Seidel sweep over a proper colouring has (colours x iterations) ~ 25 x 30 dependent phases per step.  Across the
// chip a phase boundary costs a launch (~5 us) or a tagged hand-over through L2 / the fabric (~2.5 us); inside ONE workgroup it
// costs a barrier over LDS (~0.25 us with the step's work).  So the world is cut into spatial clusters that one 512-lane workgroup
// each solves entirely out of LDS and registers for all iterations, and only what a cut crosses goes through memory:
//
//   phase 0..P-1 ("curve phases", default P = 2): the bodies are ordered along a Morton curve (each phase its own, shifted, curve)
//       and the curve is chunked by weight into tasks of ~1000 (later phases ~500) contacts; a manifold whose two bodies fall into
//       the same chunk is INTERIOR to that task.  Phase p only looks at what phases < p left over.
//   phase P ("component phase"): what the curves leave over is not cut again; its connected components are dealt whole to the tasks
//       of one more phase (~200 contacts each: they mostly run behind a first task and must fit the LDS it leaves).  A rest task (phase CL_MAX_PARTS) only takes what that cannot place (nothing, in practice).
//
// Tasks of one phase share no body, so they run concurrently, one workgroup each; a workgroup runs its (at most two per phase)
// tasks in phase order, iteration after iteration.  Inside a task the CONTACTS are coloured locally (k_cl_color: a manifold with K
// contacts takes K consecutive colours) and swept colour by colour with a workgroup barrier in between, four lanes (a quad) per
// contact row: lane q owns one of vA, wA, vB, wB in LDS and the row's vectors for it, the row velocity is summed inside the quad with
// two DPP adds.  Body velocities live in LDS for the whole launch, the rows of the workgroup's first task in registers
// (CLQ_SETS x CLQ_QUADS contacts), all other rows in LDS in the same lane-private format, global scratch only beyond that.  A body
// touched in more than one phase is handed from task to task through tagged 2 x 16-byte records (sc1 store / sc1 poll,
// MI355X_MICROARCH.md "tagged granules"): with d = number of phases that touch the body, the task of phase p is its r-th user,
// r = popcount(phaseMask & ((1 << p) - 1)), waits for turn epoch + it * d + r and publishes + 1.  Every wait points to a strictly
// earlier (iteration, phase): no cycles.
//
// The result is a Gauss-Seidel sweep in the sequential order (phase, task, local colour, position) — the order
// mi_debug_read_schedule reports and the CPU oracle follows — with bit-identical arithmetic to the launch-per-colour sweep.
#pragma once
#include "world.h"

// The counter and phase limits (CL_MAX_PARTS, CL_MAX_PHASES, CL_MAX_TASKS, CL_BODY_STRIDE, ...) are world.h's: the step and the API read them.
#define CL_TASKS_PER_PHASE 2u              // tasks of one phase a workgroup may run (LDS holds the bodies and meta of all its tasks)
#define CL_SUBCOUNTERS 8u                  // a task's append cursor is split in 8 (by workgroup) so that ~650 returning atomics do not queue on one address; taskStart[key * CL_SUBCOUNTERS] = the task's first slot
#define CL_LOCAL_STATIC 0xFFFFu            // local body index of the static dummy body
#define CL_SERIAL_COLOR 64u                // colours of a task's local colouring; what finds none below it forms the task's serial tail

MI_DEV u32 clHash(u32 x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
// Where phase p's task 0 goes: task t of phase p belongs to workgroup (clPhaseOffset + t) % G.  The first phase starts at workgroup 0;
// behind it the phases are placed LAST PHASE FIRST (rest task, then the last partition phase, ...): the workgroups the first phase
// leaves free run their task from registers, and the few tasks of the last phases — every iteration's critical path runs through
// them — get those places before the second phase's many tasks do.
MI_DEV u32 clPhaseOffset(const u32* counters, u32 p)
{
	u32 off = p ? counters[CTR_CL_NUM_TASKS] : 0u;
	for (u32 q = CL_MAX_PHASES - 1u; q > p && p; --q) off += counters[CTR_CL_NUM_TASKS + q];
	return off;
}
// A task's header, written by k_cl_color and read by k_cl_solve.
struct ClTask
{
	u32 first, count, numBodies, numShared, numColors, serialStart, numRows, sharedBase; // numRows: contacts; serialStart: first CONTACT position of the serial tail; sharedBase: first hand-over record of the task's shared bodies
	u32 colorStart[72]; // CONTACT position (relative to 4 * first in the contact tables) of the first contact of colour c; [numColors] = serialStart
};
static_assert(sizeof(ClTask) == 320, "task header");

// ---- host side: each stage sets up and launches its own kernels ----------------------------------------------------
bool cluster_color_setup(World& w, u32 computeUnits); // k_cl_color's dynamic-LDS attributes and the narrow launch's size; false = the device refuses the wide tables
void cluster_color_launch(World& w, u32 nj); // nj: joints the sweep runs (0: their tables are not read)
u32 cluster_solve_setup(const World& w);    // k_cl_solve's dynamic-LDS budget in bytes on w's device, set on both instantiations; 0 = the device refuses it
