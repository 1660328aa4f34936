/* mi_physics.h — C-ABI of the MI355X-native rigid-body stepper (libmi_physics.so).
 *
 * Drop-in boundary for the `src/physics` hot path of study-game-engines/directx-renderer-kurth: every entry point
 * below names the reference interface it replaces (file:line under /root/reference/src).  Plain pointers and sizes
 * only; all host pointers are caller-owned and only touched during the call; a world owns its device memory and one
 * HIP stream; a world is not re-entrant (the reference's physics step is single-threaded per scene).
 * Every function returning `int` returns MI_OK (0) or an MI_ERR_* code instead of the reference's ASSERT/__debugbreak
 * (pch.h:33-34); mi_last_error() gives the text.  There is NO CPU fallback: without a usable HIP device
 * mi_world_create() fails with MI_ERR_NO_DEVICE.
 *
 * The existing C-ABI precedent in the reference is the Physics-Lib DLL (learning/learned_locomotion.cpp:395-489,
 * premake5.lua:388-462): global singletons + caller-owned float buffers; we keep caller-owned buffers and replace
 * the singletons by an opaque handle.
 */
#ifndef MI_PHYSICS_H
#define MI_PHYSICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_world mi_world;

enum { MI_OK = 0, MI_ERR_NO_DEVICE = 1, MI_ERR_INVALID_ARGUMENT = 2, MI_ERR_HIP = 3, MI_ERR_CAPACITY = 4, MI_ERR_UNSUPPORTED = 5, MI_ERR_INVALID_STATE = 6 };

/* collider_type, physics.h:58-70 — the enum order is load-bearing (pair kernels are bucketed by it). */
enum { MI_COLLIDER_SPHERE = 0, MI_COLLIDER_CAPSULE = 1, MI_COLLIDER_CYLINDER = 2, MI_COLLIDER_AABB = 3, MI_COLLIDER_OBB = 4, MI_COLLIDER_HULL = 5 };
/* constraint_type, constraints.h:14-28 */
enum { MI_CONSTRAINT_DISTANCE = 0, MI_CONSTRAINT_BALL = 1, MI_CONSTRAINT_FIXED = 2, MI_CONSTRAINT_HINGE = 3, MI_CONSTRAINT_CONE_TWIST = 4, MI_CONSTRAINT_SLIDER = 5 };
/* constraint_motor_type, constraints.h:39-43 */
enum { MI_MOTOR_VELOCITY = 0, MI_MOTOR_POSITION = 1 };

#define MI_STATIC_BODY 0xFFFFFFFFu

/* physics_material (physics.h:40-47) without the sound-selection tag. */
typedef struct mi_material { float restitution, friction, density; } mi_material;

/* physics_settings (physics.h:382-397), field for field, minus the two std::function callbacks. */
typedef struct mi_physics_settings
{
	uint32_t fixedFrameRate;               /* bool */
	uint32_t frameRate;                    /* 120 */
	uint32_t maxPhysicsIterationsPerFrame; /* 4 */
	uint32_t numRigidSolverIterations;     /* 30 */
	uint32_t numClothVelocityIterations, numClothPositionIterations, numClothDriftIterations; /* iteration counts of the cloth solver (cloth.cpp:331-347) */
	uint32_t simdBroadPhase, simdNarrowPhase, simdConstraintSolver;                           /* accepted, unused: there is one (HIP) path */
} mi_physics_settings;

typedef struct mi_world_desc
{
	int32_t device;            /* HIP device ordinal; -1 = current device */
	uint32_t reserveBodies;    /* capacity hints, 0 = grow on demand */
	uint32_t reserveColliders;
	uint32_t reservePairs;
} mi_world_desc;

/* Counters of the last internal step — the reference's CPU_PROFILE_STATs (physics.cpp:1258-1262) plus per-stage times. */
typedef struct mi_stats
{
	uint32_t numRigidBodies, numColliders, numBroadphaseOverlaps, numCollisions, numContacts;
	uint32_t numColors, numJoints, numInternalSteps;
	uint32_t numGraphBuilds, coloringRounds; /* unused (kept for layout compatibility); colouring round budget of the last step */
	uint32_t flowProbes;                     /* unused (kept for layout compatibility) */
	uint32_t numFlowRecoveries;              /* steps whose cluster contact sweep gave up and was redone with the launch sweep (should stay 0) */
	float msCollidersBroad, msNarrow, msSolverSetup, msSolve, msIntegrate, msTotal; /* HIP-event times, mean over the timed steps since the previous mi_get_stats (timing enabled only) */
	float avgContacts, avgCollisions, avgColors, avgBroadphaseOverlaps, avgFlowProbes; /* means over the internal steps since the previous mi_get_stats */
	uint32_t avgSteps;                                                                 /* ... and how many steps that was */
	/* cluster contact sweep of the last step (all 0 after a launch-sweep step): tasks and manifolds per phase ([4] = the rest task),
	 * bodies handed between tasks (summed over the tasks that touch them), partition phases prepared */
	uint32_t clusterTasks[5], clusterManifolds[5], clusterSharedBodies, clusterParts;
	uint32_t numNarrowphaseRedone;           /* steps whose pair list + narrowphase, launched before the host knew the pair count, had to be launched again (the count jumped by more than 12 %) */
} mi_stats;

/* ---- lifetime ------------------------------------------------------------------------------------------------ */
mi_world* mi_world_create(const mi_world_desc* desc);                 /* replaces game_scene + memory_arena ownership (physics.cpp:1205,1361) */
void mi_world_destroy(mi_world* w);
/* Checkpoint / resume (the engine's scene files — serialization_yaml.cpp:72-230, serialization_binary.cpp:225-260 —
 * are asset formats and out of scope): a self-contained binary image of the world (bodies with current state and mass properties,
 * colliders, hull geometries, joints).  A world restored from it continues bit-identically. */
uint64_t mi_snapshot_size(mi_world* w);
int mi_snapshot_save(mi_world* w, void* buffer, uint64_t capacity);
mi_world* mi_world_restore(const mi_world_desc* desc, const void* buffer, uint64_t size); /* NULL on error: mi_last_error(NULL) */
const char* mi_last_error(mi_world* w);                               /* w may be NULL for create-time errors */

/* ---- add API --------------------------------------------------------------------------------------------------- */
/* entity.addComponent<rigid_body_component>(kinematic, gravityFactor, linearDamping=.4, angularDamping=.4) on an entity with
 * transform {pos, rot}: rigid_body.h:21, rigid_body.cpp:6-27, scene.h:69-84.  Returns the body index (= add order). */
uint32_t mi_add_body(mi_world* w, int kinematic, float gravityFactor, float linearDamping, float angularDamping, const float pos[3], const float rot[4]);
/* Convex hull geometry shared by hull colliders: replaces allocateBoundingHullGeometry(meshFilepath) (physics.h:207, physics.cpp:58-84)
 * from the mesh on — loading a model file belongs to the asset pipeline — i.e. bounding_hull_geometry::fromMesh(vertices, triangles)
 * (bounding_volumes.cpp:1394-1452).  Triangles face outwards.  Returns the geometry index (INVALID = 0xFFFFFFFF). */
uint32_t mi_add_hull_geometry(mi_world* w, const float* vertices3, uint32_t numVertices, const uint32_t* triangles3, uint32_t numTriangles);
/* entity.addComponent<collider_component>(collider_component::as{Sphere,Capsule,Cylinder,AABB,OBB,Hull}(shape, material)): physics.h:110-157,
 * scene.h:38-63 (recomputes the body's mass properties, rigid_body.cpp:29-81).  shape = up to 10 floats in the parent's local space:
 * sphere c3,r | capsule/cylinder A3,B3,r | aabb min3,max3 | obb quat4,center3,radius3 | hull quat4,position3,geometry index (as a float
 * value).  Returns the collider index. */
uint32_t mi_add_collider(mi_world* w, uint32_t body, uint32_t type, const float* shape, const mi_material* material);
/* Collider on an entity without a rigid body (static_collider, physics.cpp:667-671); {pos, rot} is that entity's transform. */
uint32_t mi_add_static_collider(mi_world* w, uint32_t type, const float* shape, const mi_material* material, const float pos[3], const float rot[4]);

/* add{Distance,Ball,Fixed,Hinge,ConeTwist,Slider}ConstraintFrom{Local,Global}Points: physics.h:209-235, physics.cpp:128-333.
 * Global variants derive the local anchors/axes from the bodies' CURRENT transforms.  Return the per-type constraint id. */
uint32_t mi_add_distance_constraint_local(mi_world* w, uint32_t a, uint32_t b, const float localAnchorA[3], const float localAnchorB[3], float distance);
uint32_t mi_add_distance_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchorA[3], const float globalAnchorB[3]);
uint32_t mi_add_ball_constraint_local(mi_world* w, uint32_t a, uint32_t b, const float localAnchorA[3], const float localAnchorB[3]);
uint32_t mi_add_ball_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchor[3]);
uint32_t mi_add_fixed_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchor[3]);
uint32_t mi_add_hinge_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchor[3], const float globalHingeAxis[3], float minLimit, float maxLimit);
uint32_t mi_add_cone_twist_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchor[3], const float globalAxis[3], float swingLimit, float twistLimit);
uint32_t mi_add_slider_constraint_global(mi_world* w, uint32_t a, uint32_t b, const float globalAnchor[3], const float globalAxis[3], float minLimit, float maxLimit);
/* addConstraint(scene_entity& a, scene_entity& b, const T& c) for the six constraint types (physics.h:239-244): the constraint is given
 * as the reference's POD (the layouts mi_constraint_get returns: 28/24/40/104/120/72 bytes), as the deserialisers hold it
 * (serialization_binary.cpp:237-260).  type = MI_CONSTRAINT_*.  Returns the constraint id within its type, 0xFFFFFFFF on error. */
uint32_t mi_add_constraint(mi_world* w, uint32_t type, uint32_t a, uint32_t b, const void* pod);

/* T& getConstraint(scene, handle) (physics.h:248-253) as get/set of the POD whose layout is byte-identical to the reference's
 * distance/ball/fixed/hinge/cone_twist/slider_constraint structs (constraints.h:73-80,129-135,175-183,229-257,346-380,497-520;
 * 28/24/40/104/120/72 bytes).  Motors are driven by writing fields, as learned_locomotion.cpp:73-91 does. */
int mi_constraint_get(mi_world* w, uint32_t type, uint32_t id, void* pod);
int mi_constraint_set(mi_world* w, uint32_t type, uint32_t id, const void* pod);
int mi_delete_constraint(mi_world* w, uint32_t type, uint32_t id);    /* deleteConstraint, physics.h:257-262 */
int mi_delete_all_constraints(mi_world* w);                           /* deleteAllConstraints, physics.h:255 */
int mi_delete_all_constraints_from_body(mi_world* w, uint32_t body);  /* deleteAllConstraintsFromEntity, physics.h:264 */
/* Deleting the entity of a rigid body (scene.deleteEntity: body, colliders and constraints go away; the colliders leave the sweep,
 * collision_broad.cpp:42-75).  Indices are add-order positions and stay valid; the body is switched off for good. */
int mi_delete_body(mi_world* w, uint32_t body);

/* ---- force fields, triggers, collision events (row N2 of SURVEY §8f) --------------------------------------------------------------
 * force_field_component (physics.h:182-185): `force` is rotated by the entity's transform when it has one (pass pos/rot, or NULL for
 * none; physics.cpp:767-771).  A field without colliders acts on every body (global, :782, :1273); a field with colliders acts on
 * the rigid bodies whose colliders overlap them (:963-967).  A body inside several localized fields receives their forces in
 * ascending field id.  Returns the field id. */
uint32_t mi_add_force_field(mi_world* w, const float force[3], const float pos[3], const float rot[4]);
int mi_set_force_field(mi_world* w, uint32_t field, const float force[3]);
/* trigger_component (physics.h:200-203): the std::function callback becomes mi_drain_events.  Returns the trigger id. */
uint32_t mi_add_trigger(mi_world* w, const float pos[3], const float rot[4]);
/* Colliders of a force-field / trigger entity (collider_component on that entity, physics.cpp:657-666): shape payload as in
 * mi_add_collider, in the entity's local space; no material.  Return the collider id. */
uint32_t mi_add_force_field_collider(mi_world* w, uint32_t field, uint32_t type, const float* shape);
uint32_t mi_add_trigger_collider(mi_world* w, uint32_t trigger, uint32_t type, const float* shape);
/* Moving a force-field / trigger entity (writing its transform_component): its colliders follow, a field's force is rotated by the new
 * rotation.  Takes effect at the next step. */
int mi_set_force_field_transform(mi_world* w, uint32_t field, const float pos[3], const float rot[4]);
int mi_set_trigger_transform(mi_world* w, uint32_t trigger, const float pos[3], const float rot[4]);
/* physics_settings::collisionBeginCallback / collisionEndCallback (physics.h:394-395) set or not.  Enable before the first step:
 * the previous step's collision set is only kept while one of the two is on. */
int mi_enable_collision_events(mi_world* w, int begin, int end);
/* trigger_event (physics.h:193-198), collision_begin_event / collision_end_event (physics.h:356-376) as one record.
 * kind: MI_EVENT_*; step: internal step that raised it; trigger events: a = trigger id, b = bodyB = body id;
 * collision events: a, b = collider ids in contact-normal order, bodyA / bodyB = their bodies (MI_STATIC_BODY for a static
 * collider); begin events carry the mean contact point, mean normal and the relative velocity (B - A) at that point. */
enum { MI_EVENT_TRIGGER_ENTER = 0, MI_EVENT_TRIGGER_LEAVE = 1, MI_EVENT_COLLISION_BEGIN = 2, MI_EVENT_COLLISION_END = 3 };
typedef struct mi_event { uint32_t kind, step, a, b, bodyA, bodyB; float position[3], normal[3], relativeVelocity[3]; } mi_event;
/* Copies out up to `capacity` pending events in the order the reference calls back in (per step: trigger events, then collision
 * events, each sorted by pair) and returns how many; call again until it returns 0.  Synchronises with the device.
 * If the device-side event ring overflowed since the last drain, mi_last_error() says so and the call after this one fails with
 * MI_ERR_CAPACITY (events were lost). */
uint32_t mi_drain_events(mi_world* w, mi_event* out, uint32_t capacity);

/* ---- heightmap terrain (row N4 of SURVEY §8f): heightmap_collider_component(chunksPerDim, chunkSize, material) + update(minCorner,
 * amplitudeScale), heightmap_collider.h:127-152.  chunksPerDim x chunksPerDim chunks, each 129 x 129 uint16 heights (row-major, z rows)
 * spanning chunkSize metres; height = minCorner.y + h / 65535 * amplitudeScale.  Every internal step, after the narrowphase, each
 * sphere / capsule / AABB / OBB collider of a rigid body is collided with the triangles under it, plus one contact if its lowest point
 * is below the surface (heightmap_collision.cpp:522-618; cylinders and hulls have no terrain case in the reference either).
 * Terrain contacts raise no collision events (physics.cpp:1049). */
int mi_set_heightmap(mi_world* w, uint32_t chunksPerDim, float chunkSize, const mi_material* material, const float minCorner[3], float amplitudeScale);
int mi_heightmap_set_chunk(mi_world* w, uint32_t x, uint32_t z, const uint16_t* heights129x129); /* heightmap_collider_chunk::setHeights; chunks never set collide with nothing */
int mi_heightmap_update(mi_world* w, const float minCorner[3], float amplitudeScale);
float mi_heightmap_height_at(mi_world* w, float x, float z);   /* getHeightAt: -FLT_MAX outside the terrain */

/* ---- cloth (row N4 of SURVEY §8f): cloth_component(width, height, gridSizeX, gridSizeY, totalMass, stiffness = .5, damping = .3,
 * gravityFactor = 1), cloth.h:8-9.  A grid of particles in the cloth's local frame (x across, -z down, upper row locked) with stretch /
 * shear / bend distance constraints; every internal step, after the rigid bodies, it receives the global force field as wind and runs
 * numCloth{Velocity,Position,Drift}Iterations of mi_physics_settings (physics.cpp:1354-1358).  The constraints are solved in a fixed
 * colour order (12 colours), not the reference's storage order.  Returns the cloth id. */
uint32_t mi_add_cloth(mi_world* w, float width, float height, uint32_t gridSizeX, uint32_t gridSizeY, float totalMass, float stiffness, float damping, float gravityFactor);
/* cloth_component::setWorldPositionOfFixedVertices(transform, moveRigid), cloth.h:17: puts the locked upper row at `transform`;
 * moveRigid also carries the rest of the cloth along rigidly. */
int mi_cloth_set_fixed_vertices(mi_world* w, uint32_t cloth, const float pos[3], const float rot[4], int moveRigid);
/* The public fields totalMass / stiffness / damping / gravityFactor (cloth.h:21-24); mass and stiffness changes re-derive the
 * particle and constraint masses at the next step (cloth.cpp:198-204, 331-347). */
int mi_cloth_set_properties(mi_world* w, uint32_t cloth, float totalMass, float stiffness, float damping, float gravityFactor);
/* Cloth iteration counts for mi_step_internal (mi_step takes them from its settings).  Default 0, 1, 0 (physics.h:387-389). */
int mi_set_cloth_iterations(mi_world* w, uint32_t velocityIterations, uint32_t positionIterations, uint32_t driftIterations);
uint32_t mi_num_cloths(mi_world* w);
uint32_t mi_cloth_num_particles(mi_world* w, uint32_t cloth);
/* Particle positions / velocities, row-major over the grid, n x 3 floats each (either pointer may be NULL). */
int mi_cloth_read(mi_world* w, uint32_t cloth, float* positions3, float* velocities3);

/* Cloth collision: the particles of a cloth are pushed out of the world's colliders and of the heightmap terrain.  (The reference's cloth
 * has no collision: the rule is this project's, as the proximity rule below is, and it is written on top of that rule.)
 * Per cloth, collision is off until mi_cloth_set_collision turns it on; a world without such a cloth launches nothing for it.  A cloth
 * that is on gets one projection pass per internal step, after the cloth kernel has written that step's positions and damped
 * velocities; it reads the body poses and velocities the step's velocity integration left.  Every particle i with invMass > 0 is handled
 * on its own: it reads no other particle, so the result does not depend on the order of the lanes.
 * Reading: exactly what mi_proximity (below) reports for a world-space query (mount = MI_STATIC_BODY) at the particle's position p with
 * radius = thickness, excludeFirst / excludeCount of the settings, and the flags MI_PROX_STATIC iff MI_CLOTH_COLLIDE_STATIC,
 * MI_PROX_TERRAIN iff MI_CLOTH_COLLIDE_TERRAIN, without MI_PROX_COUNT: the same candidates, float32 operation order, tie rules, and the
 * terrain replaces the collider reading only if its distance is strictly smaller.  Nothing found leaves the particle untouched, byte
 * for byte; so does a reading whose normal is zero (a particle at a sphere's centre, on a capsule's or a cylinder's axis).
 * Projection: with d, c, n, body of the reading, in float32 without contraction, dot, cross and length as csrc/mi_common.h writes them
 * (left to right), a vector times a scalar per component:
 *   push = thickness - d;  p' = p + n * push
 *   vs = 0 for a static collider and for the terrain, otherwise vs = v_b + cross(w_b, c - cog_b) with (v_b, w_b) the body's linear and
 *        angular velocity (mi_read_velocities) and cog_b = pos_b + rot_b * localCOG_b from its pose after the integration
 *        (mi_read_transforms, mi_read_mass_properties).  The device's centre-of-gravity array (mi_debug_read_body_state) is NOT used: the
 *        velocity integration reads it and moves the pose, and the array is formed again only by the next step's force integration.
 *   u = v - vs;  un = dot(u, n)
 *   if un < 0:  u = u - n * un;  jn = -un;  lt = |u|;  if friction > 0: u = u * s with s = 1 - (friction * jn) / lt if lt > friction * jn,
 *               else s = 0;  v' = vs + u
 *   otherwise (a NaN included) v' = v, byte for byte; the position is pushed all the same.
 * Contact plane: one uint32 per particle, the collider it was pushed off in the last internal step, MI_TERRAIN_COLLIDER for the terrain,
 * 0xFFFFFFFF for none; it reads none before the first step, for fixed particles (invMass == 0) and for a cloth whose collision is off.
 * A step whose cluster sweep gave up skips the pass with the velocity integration; the recovery runs it behind its own integration,
 * before the next step's cloth kernel, so the order above holds there too.
 * Limits: one-way (the bodies feel nothing); particles only (a collider smaller than the grid spacing slips between them); the nearest
 * candidate only, one correction per step; no self-collision; a particle that crosses more than half a thin collider in one step comes
 * out on the far side.
 * mi_cloth_set_collision(NULL) turns collision off.  MI_ERR_INVALID_ARGUMENT: a thickness or friction that is not finite or is negative,
 * unknown flag bits, non-zero reserved words, a cloth index out of range.  Setting and clearing settle a step whose cluster sweep is not
 * yet known to have completed and neither upload nor download particle state.  The settings travel with mi_snapshot_save /
 * mi_world_restore; the contact plane does not.
 * mi_debug_set_cloth_collision_brute_force: every candidate collider (and every terrain triangle) instead of the tree: same bytes. */
enum { MI_CLOTH_COLLIDE_STATIC = 1, MI_CLOTH_COLLIDE_TERRAIN = 2 };
typedef struct mi_cloth_collision { float thickness, friction; uint32_t flags, excludeFirst, excludeCount, reserved[3]; } mi_cloth_collision; /* 32 bytes */
int mi_cloth_set_collision(mi_world* w, uint32_t cloth, const mi_cloth_collision* settings);
int mi_cloth_get_collision(mi_world* w, uint32_t cloth, mi_cloth_collision* out, int* outEnabled);
int mi_cloth_read_contacts(mi_world* w, uint32_t cloth, uint32_t* outColliderPerParticle);
int mi_debug_set_cloth_collision_brute_force(mi_world* w, int on);

/* void testPhysicsInteraction(game_scene&, ray, float strength = 1000.f): physics.h:404, physics.cpp:556-628 — the closest rigid-body
 * collider hit by the ray gets force = direction * strength at the hit point.  Returns 1 + the index of the body that was
 * pushed, 0 when the ray hits nothing (this one function does not return a status code). */
int mi_test_physics_interaction(mi_world* w, const float origin[3], const float direction[3], float strength);
/* rigid_body_component::{forceAccumulator,torqueAccumulator} += (testPhysicsInteraction applies them the same way, physics.cpp:624-628). */
int mi_apply_force_torque(mi_world* w, uint32_t body, const float force[3], const float torque[3]);
int mi_set_velocity(mi_world* w, uint32_t body, const float linear[3], const float angular[3]);
int mi_set_transform(mi_world* w, uint32_t body, const float pos[3], const float rot[4]);
/* Bulk forms of the two setters above for the first n bodies: n x {pos3, quat4} / n x {linear3, angular3} (scene deserialisation,
 * serialization_binary.cpp:237-260, and state hand-over between worlds). */
int mi_write_transforms(mi_world* w, const float* in7, uint32_t n);
int mi_write_velocities(mi_world* w, const float* in6, uint32_t n);

/* ---- per-frame -------------------------------------------------------------------------------------------------- */
/* void physicsStep(game_scene&, memory_arena&, float& timer, const physics_settings&, float dt): physics.h:405, physics.cpp:1364-1413.
 * The arena argument has no counterpart (per-step arrays live in device memory owned by the world). */
int mi_step(mi_world* w, float* timer, const mi_physics_settings* settings, float dt);
/* One physicsStepInternal (physics.cpp:1180-1362) at exactly dt — what bench.py and the parity tests time and compare. */
int mi_step_internal(mi_world* w, float dt, uint32_t numRigidSolverIterations);
int mi_synchronize(mi_world* w);                                       /* waits for the world's stream */

/* ---- results (transform_component / physics_transform1 / rigid_body_component.{v,w} write-back, physics.cpp:1342-1347,1399-1411) */
/* which: 0 = interpolated transform_component, 1 = physics_transform1, 2 = physics_transform0.  out = n x {pos3, quat4}. */
int mi_read_transforms(mi_world* w, uint32_t which, float* out7, uint32_t n);
int mi_read_velocities(mi_world* w, float* out6, uint32_t n);          /* n x {linear3, angular3} */
int mi_read_mass_properties(mi_world* w, float* out13, uint32_t n);    /* n x {localCOG3, invMass, invInertia9 (column-major)} */
int mi_get_stats(mi_world* w, mi_stats* out);
/* Debug guard: the reference's VALIDATE macros (physics.cpp:807-926, compiled out there): with the guard on, every stage's output is
 * scanned for NaN / Inf on the device and the step after the one that produced one fails with MI_ERR_INVALID_STATE (the message names
 * the stage and the first offending element).  Also switched on by MI_PHYSICS_VALIDATE=1.  Costs a few small launches per step. */
int mi_enable_validation(mi_world* w, int enable);
int mi_enable_stage_timing(mi_world* w, int enable);
uint32_t mi_num_bodies(mi_world* w);
uint32_t mi_num_colliders(mi_world* w);

/* ---- device-resident access for multi-GPU halo exchange and zero-copy callers ------------------------------------- */
/* Raw device pointers (valid until the next add call): pose = 2 x float4 per body {pos.xyz,0},{quat}; vel = 2 x float4 per body
 * {v.xyz, invMass},{w.xyz,0}.  The caller may read/write them on `stream` between steps (ghost-body refresh). */
int mi_device_pointers(mi_world* w, void** pose, void** vel, void** stream);

/* Device state for callers that drive many bodies from kernels of their own (batched environments, libmi_locomotion.so).  Resolves a
 * pending step first, as mi_device_pointers does.  Pointers stay valid until the next add call.  Layouts: pose, pose0 (the pose at the
 * start of the last mi_step), poseLerp (the interpolated pose mi_read_transforms reads with which = 0): 2 x float4 per body
 * {pos.xyz,0},{quat}; vel: {v.xyz, invMass},{w.xyz,0}; force: {force.xyz,0},{torque.xyz,0}.  Between steps, on `stream`, a caller may
 *   - add to force: the next step integrates the accumulators and clears them;
 *   - write vel.xyz: vel[2i].w holds invMass and must be kept;
 *   - teleport a body: write the same pose into pose, pose0 and poseLerp, as mi_set_transform does. */
struct mi_device_state { void* pose; void* pose0; void* poseLerp; void* vel; void* force; void* stream; uint32_t numBodies, reserved; }; /* the tag names it: the function has its name */
int mi_device_state(mi_world* w, struct mi_device_state* out);

/* The device POD array of one joint type (the POD layout of mi_constraint_get, in solve order) and the slot of every joint id
 * 0 .. numIds-1 in it (0xFFFFFFFF: deleted).  Motor fields written into it on the world's stream between steps take effect at the
 * next step.  From the first call on, the device copy is authoritative: mi_constraint_get / _set, the add and delete calls and
 * mi_snapshot_save pull it back first.  The pointer and the slots hold until *outGeneration changes: any joint add, delete or set
 * and a restore give a new generation.  outSlotOfId may be NULL. */
int mi_joint_device_pods(mi_world* w, uint32_t type, void** dPods, uint32_t* outSlotOfId, uint32_t numIds, uint32_t* outGeneration);

/* mi_test_physics_interaction for many rays as one kernel on the world's stream, with no host synchronisation.  dRays (device):
 * 8 floats per ray {origin.xyz, strength, direction.xyz, enabled}; ray i only tests the colliders of the bodies
 * [firstBody + i * bodiesPerRay, firstBody + (i + 1) * bodiesPerRay), so rays never share a body.  The closest hit gets the force
 * and torque of mi_test_physics_interaction, added to the accumulators.  dOutBody[i] (device) = 1 + the pushed body, or 0. */
int mi_test_physics_interaction_batch(mi_world* w, uint32_t numRays, uint32_t firstBody, uint32_t bodiesPerRay, const float* dRays, int32_t* dOutBody);

/* Ray casts against the whole world: numRays rays, each against every candidate collider, as one call on the world's stream with no
 * host synchronisation.  Nothing is pushed and no accumulator is written.  dRays (device): 8 floats per ray {origin.xyz, maxT,
 * direction.xyz, enabled}; maxT is the largest accepted distance (+INFINITY allowed), enabled == 0 switches the ray off.  The
 * direction need not be a unit vector: t is in units of its length, as in the reference (whose sphere test, and with it a capsule's
 * ends, is geometric for unit directions only).
 * Candidates: the colliders of rigid bodies that are alive and, in a slab run, simulated here; with MI_RAY_STATIC also the colliders
 * of entities without a rigid body; with MI_RAY_TERRAIN also the heightmap terrain (below).  Force-field and trigger colliders and
 * cloth are never candidates.
 * Hit rule: a candidate's test is testPhysicsInteraction's test of that collider, in the collider's own frame.  It is a hit if
 * 0 <= t <= maxT; the smallest t wins, and of equal t the lowest collider index.  This is where the cast deviates from
 * testPhysicsInteraction: that function also accepts the negative distances its cylinder and capsule tests report for a cap disk
 * behind the origin; a ray cast reports no hit behind the ray.
 * dOutHits[i] (device): hit = 1, t, the collider, its body (MI_STATIC_BODY for a static collider) and the world hit point
 * rot * (local origin + t * local direction) + pos, bit for bit the point mi_test_physics_interaction pushes at; all zero for a miss
 * or a switched-off ray.  Hit normals are reported by mi_raycast_sensors (below), not here.
 * The acceleration structure (a BVH over the candidates) is rebuilt from the current poses at every call, in buffers of its own: poses
 * written through mi_device_state are seen, and the step's buffers are not touched.  MI_RAY_BRUTE_FORCE tests every ray against every
 * candidate instead (same answers; a yardstick, and cheaper for a handful of colliders).
 * MI_RAY_TERRAIN: the triangles the bodies collide with are candidates too (the reference has no terrain cast: the rule is this
 * project's).  Without the flag every byte of every record is what it is without a heightmap; with the flag and no heightmap the flag
 * does nothing.  Cell (cellX, cellZ) of chunk (chunkX, chunkZ) has the vertices A = (cellX, cellZ), B = (cellX, cellZ + 1),
 * C = (cellX + 1, cellZ), D = (cellX + 1, cellZ + 1), each at chunkMin + (cx * chunkScale, h * heightScale, cz * chunkScale), and the
 * triangles 0 = (A, B, C) and 1 = (C, B, D).  Per triangle (a, b, c): n = noz(cross(b - a, c - a)); a miss if |dot(direction, n)| <= 1e-6;
 * t = -(dot(origin, n) - dot(n, a)) / dot(direction, n); accepted if 0 <= t <= maxT; both faces count (a ray from below hits).
 * Containment: q = origin + t * direction, u = (q.x - A.x) / (D.x - A.x), v = (q.z - A.z) / (D.z - A.z); inside the cell if 0 <= u <= 1
 * and 0 <= v <= 1, closed on all sides; triangle 0 owns u + v <= 1, triangle 1 owns u + v >= 1.  For a vertical ray q.x and q.z are the
 * origin's, so within the x/z extent of a chunk that has heights such a ray always hits.  The smallest t wins, of equal t the lowest
 * triangle id; the terrain replaces a collider's hit only if its t is strictly smaller.  Chunks without heights are holes (a ray
 * passes and may hit a chunk behind); chunks whose border heights disagree leave a crack without a wall.  A zero direction misses.
 * A terrain hit: hit = 1, t, collider = MI_TERRAIN_COLLIDER, body = MI_STATIC_BODY, point = origin + t * direction, and in `reserved`
 * the bits of the uint32 triangle id ((chunkZ * chunksPerDim + chunkX) * 16384 + cellZ * 128 + cellX) * 2 + triangle, from which a
 * caller can form the normal; for a collider hit or a miss reserved stays 0.  A heightmap of more than 131071 chunks makes a terrain
 * cast return MI_ERR_INVALID_ARGUMENT.  The walk over the cells under the ray uses a min/max table of the heights per 8 x 8-cell tile,
 * rebuilt on the world's stream after mi_set_heightmap / mi_heightmap_set_chunk / a restore; mi_heightmap_update needs no rebuild.
 * MI_RAY_BRUTE_FORCE | MI_RAY_TERRAIN tests every triangle of every chunk instead (same answers). */
enum { MI_RAY_STATIC = 1, MI_RAY_BRUTE_FORCE = 2, MI_RAY_TERRAIN = 4 };
#define MI_TERRAIN_COLLIDER 0xFFFFFFFEu
typedef struct mi_ray_hit { float t; uint32_t collider, body, hit; float point[3]; float reserved; } mi_ray_hit; /* 32 bytes */
int mi_raycast_batch(mi_world* w, uint32_t numRays, const float* dRays, uint32_t flags, mi_ray_hit* dOutHits);
/* The same cast for callers without device memory of their own (a single pick: the C++ facade's castRay): rays and hits in HOST memory,
 * copied through staging buffers of the world around one mi_raycast_batch; returns after the hits have arrived. */
int mi_raycast_host(mi_world* w, uint32_t numRays, const float* rays, uint32_t flags, mi_ray_hit* outHits);

/* Ray sensors mounted on bodies: mi_raycast_batch for rays given in a body's frame, each with a range of bodies it does not see, and
 * with the hit normal.  One call on the world's stream with no host synchronisation; nothing is pushed and no accumulator is written;
 * the flags are the MI_RAY_* flags with unchanged meaning.  (The reference has no counterpart: the rule is this project's.)
 * Mount: `mount` is a body index; origin and direction are in that body's frame at its current pose (the pose array the cast itself
 * reads, so poses written through mi_device_state are seen).  The world ray is origin = rot * origin + pos, direction = rot * direction;
 * maxT and enabled carry over.  mount == MI_STATIC_BODY: the ray is in world space already and is taken bit for bit.  Any other mount
 * >= the number of bodies, a deleted body and, in a slab run, a body not simulated here switch the ray off: its record and its world
 * ray are all zero.  dOutWorldRays (device, may be NULL) receives 8 floats per ray, the world ray in mi_raycast_batch's input layout.
 * Exclusion: the colliders of the bodies b with b - excludeFirst < excludeCount, in uint32 arithmetic (b - excludeFirst wraps), are no
 * candidates of this ray: a range that runs past the last body is simply cut, excludeCount == 0 excludes nothing.  Static colliders and
 * the terrain are never excluded.
 * Hit: `hit` is what mi_raycast_batch reports for the world ray against the remaining candidates (the tests, 0 <= t <= maxT, smallest
 * t, then lowest collider index, terrain only if strictly closer, the triangle id in reserved, the point); with excludeCount == 0 its 32
 * bytes are those of mi_raycast_batch on dOutWorldRays.
 * Normal: the outward normal of the surface at the hit, not flipped towards the ray; zero for a miss.  It is evaluated in the
 * collider's frame at p = local origin + t * local direction (the local hit the point is made from) and rotated to world space by the
 * pose's rotation; for an OBB and a hull it is evaluated in the shape's own frame and rotated by the shape's quaternion first.
 *   sphere (c, r)       noz(p - c)
 *   capsule (a, b, r)   s = clamp(dot(p - a, b - a) / dot(b - a, b - a), 0, 1) (0 if a == b); noz(p - (a + s (b - a)))
 *   cylinder (a, b, r)  u = noz(b - a), h = |b - a|, y = dot(p - a, u), rho = (p - a) - y u; cap depth dc = min(y, h - y), side depth
 *                       ds = r - |rho|; if dc < ds the cap's normal (+u if y > h / 2, else -u), otherwise noz(rho): a tie goes to the side
 *   AABB (lo, hi)       q = p - (lo + hi) / 2, e = (hi - lo) / 2; the axis k with the largest |q_k| - e_k, the lowest k on a tie; sign(q_k) on it
 *   OBB                 the AABB rule for (-radius, radius) in the box's frame
 *   hull                noz(cross(b - a, c - a)) of the triangle that supplied t (the lowest triangle index on a tie)
 *   terrain             noz(cross(b - a, c - a)) of the hit triangle (a, b, c) as the hit rule above forms it: its y component is positive
 *                       for both triangles of a cell, also for a ray from below; no pose rotation
 * The normal follows the reported point also where the reference's tests report a point that is not on the surface: an origin inside a
 * sphere (t = 0: the normal points from the centre to the origin; zero at the centre itself) and the cylinder's radially-inside case
 * (t = 0 without a cap disk).  The rule is defined for every p.
 * mi_raycast_sensors_host: rays, hits and world rays in HOST memory, staged through buffers of the world as mi_raycast_host does;
 * returns after the hits have arrived. */
typedef struct mi_sensor_ray { float origin[3], maxT, direction[3], enabled; uint32_t mount, excludeFirst, excludeCount, reserved; } mi_sensor_ray; /* 48 bytes */
typedef struct mi_sensor_hit { mi_ray_hit hit; float normal[3], reserved; } mi_sensor_hit;                                                     /* 48 bytes */
int mi_raycast_sensors(mi_world* w, uint32_t numRays, const mi_sensor_ray* dRays, uint32_t flags, mi_sensor_hit* dOutHits, float* dOutWorldRays);
int mi_raycast_sensors_host(mi_world* w, uint32_t numRays, const mi_sensor_ray* rays, uint32_t flags, mi_sensor_hit* outHits, float* outWorldRays);

/* Proximity sensors: for a point, possibly fixed to a body, the nearest collider surface within a radius and the number of colliders
 * within it.  One call on the world's stream; like the ray entries it first settles a step whose cluster sweep is not yet known to have
 * completed and otherwise does not synchronise with the host; no step buffer and no accumulator is written; numQueries == 0 launches
 * nothing.  (The reference has no counterpart: the rule is this project's.)
 * Mount and exclusion are mi_sensor_ray's: `point` is in the frame of body `mount` at its current pose (the pose array the call itself
 * reads, so poses written through mi_device_state are seen), world point = rot * point + pos; mount == MI_STATIC_BODY: the point is in
 * world space already and is taken bit for bit.  Any other mount >= the number of bodies, a deleted body, in a slab run a body not
 * simulated here, and enabled == 0 switch the query off: its reading and its world point are all zero.  dOutWorldPoints (device, may be
 * NULL) receives 4 floats per query: the world point and the radius.  The colliders of the bodies b with b - excludeFirst < excludeCount,
 * in uint32 arithmetic (the subtraction wraps), are no candidates of this query; static colliders are never excluded.
 * Candidates are mi_raycast_batch's: the colliders of alive bodies simulated here and, with MI_PROX_STATIC, those of entities without a
 * rigid body; never force-field or trigger colliders, never cloth; with MI_PROX_TERRAIN also the heightmap terrain (below).
 * Distance: the signed Euclidean distance d from the world point to each candidate, negative inside, with the closest surface point c
 * and the outward unit normal n there.  It is evaluated in the collider's own frame, p = conjugate(rot) * (world point - pos), for an
 * OBB and a hull further through the conjugate of the shape's quaternion; c and n are rotated (and c translated) back the same way.
 * Arithmetic is float32 without contraction in the order csrc/point_tests.h writes out.  unit(v) = v / |v|, and zero where |v| is 0.
 *   sphere (ce, r)      v = p - ce; d = |v| - r; n = unit(v); c = ce + r n
 *   capsule (a, b, r)   s = clamp(dot(p - a, b - a) / dot(b - a, b - a), 0, 1) (0 if a == b): the sensor normal rule's s; the sphere
 *                       (a + s (b - a), r)
 *   cylinder (a, b, r)  u = unit(b - a), h = |b - a|, y = dot(p - a, u), rho = (p - a) - y u, l = |rho|; dax = |y - h / 2| - h / 2,
 *                       drad = l - r.  Inside or on the surface (dax <= 0 and drad <= 0): d = max(dax, drad); if dax > drad the nearer
 *                       cap (the upper one iff y > h / 2): n = +u or -u, c = p + (h - y) u or p - y u; otherwise the side: n = unit(rho),
 *                       c = a + y u + r n: a tie goes to the side, as in the sensor normal rule (on the axis itself n is zero).
 *                       Outside: c = a + clamp(y, 0, h) u + (l > r ? r unit(rho) : rho); d = |p - c|; n = unit(p - c)
 *   AABB (lo, hi)       q = p - (lo + hi) / 2, e = (hi - lo) / 2, w_k = |q_k| - e_k.  All w_k <= 0: the axis k with the largest w_k, the
 *                       lowest k on a tie; d = w_k; n = sign(q_k) on axis k (the sign of +0 and -0 is positive); c = p with its k-th
 *                       coordinate set to centre_k + sign(q_k) e_k.  Otherwise c = centre + clamp(q, -e, e); d = |p - c|; n = unit(p - c)
 *   OBB                 the AABB rule for (-radius, radius) in the box's frame
 *   hull                over its triangles f = (a, b, c) with n_f = unit(cross(b - a, c - a)): plane = max_f dot(p - a_f, n_f), the
 *                       lowest f on a tie.  plane <= 0: d = plane; n = n_f; c = p - plane n_f.  Otherwise the closest point c_f of every
 *                       triangle, with ab = b - a, ac = c - a, d1 = dot(ab, p - a), d2 = dot(ac, p - a), d3 = dot(ab, p - b),
 *                       d4 = dot(ac, p - b), d5 = dot(ab, p - c), d6 = dot(ac, p - c), the first that applies of
 *                         d1 <= 0 and d2 <= 0: a;   d3 >= 0 and d4 <= d3: b;
 *                         d1 d4 - d3 d2 <= 0 and d1 >= 0 and d3 <= 0: a + (d1 / (d1 - d3)) ab;   d6 >= 0 and d5 <= d6: c;
 *                         d5 d2 - d1 d6 <= 0 and d2 >= 0 and d6 <= 0: a + (d2 / (d2 - d6)) ac;
 *                         d3 d6 - d5 d4 <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0: b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) (c - b);
 *                         else the face: p - dot(p - a, n_f) n_f;
 *                       d = min_f |p - c_f|, the lowest f on a tie; c = that c_f; n = unit(p - c)
 * Reading: a candidate is within iff d <= radius; radius may be +INFINITY; a negative or NaN radius finds nothing.  found = 1 and
 * distance, collider, body, point (= c), normal (= n) describe the within-candidate with the smallest d, of equal d the one with the
 * lowest collider index; body is MI_STATIC_BODY for a static collider.  With MI_PROX_COUNT numWithin is the number of within-candidates,
 * without the flag 0.  With nothing within the whole record is zero.
 * The candidates and the tree over them are mi_raycast_batch's, rebuilt from the current poses at every call in the same buffers;
 * MI_PROX_BRUTE_FORCE asks every candidate instead (same bytes; a yardstick).  Calls of the two kinds may follow each other freely.
 * MI_PROX_TERRAIN: the heightmap terrain is one more candidate, the solid under its surface.  Without the flag every byte of every
 * record is what it is without a heightmap; with the flag and no heightmap the flag does nothing.  The triangles are mi_raycast_batch's
 * (MI_RAY_TERRAIN above): cell (cellX, cellZ) of a chunk that has heights has the vertices A, B, C, D in world coordinates, triangle
 * 0 = (A, B, C), triangle 1 = (C, B, D), id = ((chunkZ * chunksPerDim + chunkX) * 16384 + cellZ * 128 + cellX) * 2 + triangle.  Per
 * triangle f = (a, b, c): n_f = unit(cross(b - a, c - a)), c_f = the hull rule's closest point of the triangle to the world point p,
 * d_f = |p - c_f|.  Arithmetic is float32 without contraction in the order csrc/terrain_point.h writes out.
 *   nearest   the triangle with the smallest d_f, of equal d_f the lowest id
 *   sign      among the triangles that own p's (x, z) by the ray rule's closed containment with q = p (u = (p.x - A.x) / (D.x - A.x),
 *             v = (p.z - A.z) / (D.z - A.z), both in [0, 1]; triangle 0 owns u + v <= 1, triangle 1 owns u + v >= 1) the one with the
 *             lowest id decides: p is below iff dot(p - a_f, n_f) < 0.  A point over no chunk that has heights (outside the footprint,
 *             over a hole) is never below: the terrain has no side walls and no floor.  This is a stated limit: beside the rim, or under
 *             a hole's border, a point lower than the surface next to it reads a positive distance to that surface.
 *   reading   d = d_f above, -d_f below; point = c_f; normal = unit(p - c_f) above, unit(c_f - p) below, n_f where p == c_f
 * The terrain is within iff d <= radius, so a point below the surface is within for every radius >= 0, however deep (the search for
 * its nearest triangle is bounded by the distance to the triangles of its own column, never by the radius).  The terrain's reading
 * replaces the colliders' only if its d is strictly smaller (MI_TERRAIN_COLLIDER is the largest index: "the lowest collider index on a
 * tie").  A terrain reading has collider = MI_TERRAIN_COLLIDER, body = MI_STATIC_BODY and in `reserved` the bits of the uint32 triangle
 * id of the nearest triangle, as mi_ray_hit has; for a collider reading reserved stays 0.  With MI_PROX_COUNT the terrain adds exactly 1
 * to numWithin when it is within, also when a collider is nearer.  Exclusion ranges never exclude the terrain; mounts, switched-off
 * queries and dOutWorldPoints are unchanged.  A world point that is not finite does not meet the terrain.  A heightmap of more than
 * 131071 chunks makes a call with the flag return MI_ERR_INVALID_ARGUMENT.  The search uses the ray cast's min/max table of the heights
 * (rebuilt after mi_set_heightmap / mi_heightmap_set_chunk / a restore; mi_heightmap_update needs no rebuild);
 * MI_PROX_BRUTE_FORCE | MI_PROX_TERRAIN asks every triangle of every chunk instead (same bytes).
 * mi_proximity_host: queries, readings and world points in HOST memory, staged through buffers of the world; returns after the
 * readings have arrived. */
enum { MI_PROX_STATIC = 1, MI_PROX_BRUTE_FORCE = 2, MI_PROX_COUNT = 4, MI_PROX_TERRAIN = 8 };
typedef struct mi_proximity_query { float point[3], radius; uint32_t mount, excludeFirst, excludeCount, enabled; } mi_proximity_query; /* 32 bytes */
typedef struct mi_proximity_reading { float distance; uint32_t collider, body, found; float point[3]; uint32_t numWithin;
                                      float normal[3], reserved; } mi_proximity_reading; /* 48 bytes */
int mi_proximity(mi_world* w, uint32_t numQueries, const mi_proximity_query* dQueries, uint32_t flags, mi_proximity_reading* dOut, float* dOutWorldPoints);
int mi_proximity_host(mi_world* w, uint32_t numQueries, const mi_proximity_query* queries, uint32_t flags, mi_proximity_reading* out, float* outWorldPoints);

/* Sphere casts ("thick rays"): how far a sphere of a given radius can travel from a point in a direction before it touches a collider,
 * and where and on what it touches.  One call on the world's stream; like the ray entries it first settles a step whose cluster sweep
 * is not yet known to have completed and otherwise does not synchronise with the host; no step buffer and no accumulator is written;
 * numQueries == 0 launches nothing.  (The reference has no counterpart: the rule is this project's.)
 * Mount, exclusion and candidates are mi_sensor_ray's and mi_proximity_query's: origin and direction are in the frame of body `mount`
 * at its current pose, world origin = rot * origin + pos, world direction = rot * direction; mount == MI_STATIC_BODY: both are in world
 * space already and are taken bit for bit.  Any other mount >= the number of bodies, a deleted body, in a slab run a body not simulated
 * here, and enabled == 0 switch the query off: its hit and its world cast are all zero.  dOutWorldCasts (device, may be NULL) receives
 * 8 floats per query: {world origin, maxT, world direction, radius}.  The colliders of the bodies b with b - excludeFirst <
 * excludeCount, in uint32 arithmetic (the subtraction wraps), are no candidates of this query; static colliders are never excluded.
 * Candidates: the colliders of alive bodies simulated here and, with MI_SPHERE_STATIC, those of entities without a rigid body; never
 * force-field or trigger colliders, never cloth; with MI_SPHERE_TERRAIN also the heightmap terrain (below).
 * Query: the direction need not be a unit vector and t is in units of its length, as for the ray cast; L = |world direction| is formed
 * once per query.  maxT may be +INFINITY.  A negative or NaN radius and a negative or NaN maxT find nothing, also from inside a shape.
 * radius == 0 is allowed: a ray cast by the distance rule below (not by the reference's ray tests).
 * Per candidate, in the collider's frame: o = conjugate(rot) * (world origin - pos), v = conjugate(rot) * world direction, and the gap
 * g(t) = d(o + t v) - radius with d the signed distance of mi_proximity (above; csrc/point_tests.h).  d is convex along a line and
 * 1-Lipschitz.  With tol(t) = SC_GAP + SC_GUARD_ULPS * 2^-23 * ((|o| + t L) + radius), SC_GAP = 1e-4 m, SC_GUARD_ULPS = 16:
 *   t = 0; repeat at most SC_MAX_ITER = 32 times:
 *     evaluate g = g(t); if g <= tol(t): the candidate hits at t (an origin in touch or inside: t = 0 and a negative gap)
 *     if not L > 0: miss (a zero direction is an overlap test at the origin)
 *     with a previous sample: slope = (g - gPrev) / (t - tPrev); if slope >= 0: miss (receding: by convexity g does not come down again)
 *     t = t + max(g / L, -g / slope)   (without a previous sample t + g / L); if not t <= maxT: miss
 *   after SC_MAX_ITER samples: a hit at the last sample's t with hit = 2 (unresolved): the sphere is free up to there.
 * g / L is conservative advancement (d is 1-Lipschitz), -g / slope the root of the chord through the last two samples (a convex function
 * lies above the extension of its chord): in exact arithmetic neither passes the first contact.  Arithmetic is float32 without
 * contraction in the order csrc/sphere_cast.h writes out.
 * Result: the candidate with the smallest t wins, of equal t the lowest collider index.  hit = 1 (or 2), t, collider, body
 * (MI_STATIC_BODY for a static collider); point = the closest surface point c at the stop and normal = the outward unit normal n there,
 * both of the distance rule, rotated (and c translated) back by the pose; gap = g at the stop (negative when overlapping); iterations =
 * the samples the winner took.  The sphere's centre at the stop is world origin + t * world direction.  A miss is all zero.
 * The candidates and the tree over them are mi_raycast_batch's, rebuilt from the current poses at every call in the same buffers;
 * MI_SPHERE_BRUTE_FORCE asks every candidate instead (same bytes; a yardstick).  Calls of all query kinds may follow each other freely.
 * MI_SPHERE_TERRAIN: the heightmap terrain is a two-sided sheet of convex candidates, as it is for rays.  Without the flag every byte of
 * every record is what it is without a heightmap; with the flag and no heightmap the flag does nothing.  Each triangle f = (a, b, c) of
 * mi_proximity's terrain rule (above) is one candidate, in world space (o = world origin, v = world direction), with the unsigned gap
 * g_f(t) = |(o + t v) - c_f(o + t v)| - radius: the distance to a triangle is convex along a line and 1-Lipschitz, so the march above
 * applies to it unchanged (the same tolerance, step rule, SC_MAX_ITER and unresolved flag; csrc/terrain_point.h on csrc/sphere_cast.h).
 * The smallest t wins; of equal t a collider wins before the terrain, and among triangles the lowest id.  A terrain hit: hit = 1 (or 2),
 * t, collider = MI_TERRAIN_COLLIDER, body = MI_STATIC_BODY, point = c_f at the stop, normal = unit(centre - c_f) with centre = o + t v,
 * and n_f where they coincide; gap and iterations of the winning triangle.  mi_sphere_hit has no spare field: a terrain hit carries no
 * triangle id (mi_proximity with MI_PROX_TERRAIN at the centre names the triangle).  Limits, the sheet against mi_proximity's solid: an
 * origin nearer to the sheet than radius + tolerance, on either side, hits at t = 0 with its gap; an origin under the sheet by more than
 * that travels freely until it touches the sheet from below (the normal then points down).  radius == 0 is a ray cast by this rule, not
 * by MI_RAY_TERRAIN's plane test.  Chunks without heights are holes.  A zero direction is an overlap test at the origin, as above; a
 * cast whose world origin, direction or radius is not finite does not meet the terrain.  Exclusion ranges never exclude the terrain.
 * A heightmap of more than 131071 chunks makes a call with the flag return MI_ERR_INVALID_ARGUMENT.  The walk visits the cells under
 * the swept sphere front to back with the ray cast's min/max table; MI_SPHERE_BRUTE_FORCE | MI_SPHERE_TERRAIN marches every triangle of
 * every chunk instead (same bytes).
 * mi_sphere_cast_host: queries, hits and world casts in HOST memory, staged through buffers of the world; returns after the hits have
 * arrived. */
enum { MI_SPHERE_STATIC = 1, MI_SPHERE_BRUTE_FORCE = 2, MI_SPHERE_TERRAIN = 4 };
typedef struct mi_sphere_cast { float origin[3], maxT, direction[3], radius; uint32_t mount, excludeFirst, excludeCount, enabled; } mi_sphere_cast; /* 48 bytes */
typedef struct mi_sphere_hit { float t; uint32_t collider, body, hit; float point[3], gap; float normal[3]; uint32_t iterations; } mi_sphere_hit; /* 48 bytes */
int mi_sphere_cast_batch(mi_world* w, uint32_t numQueries, const mi_sphere_cast* dQueries, uint32_t flags, mi_sphere_hit* dOut, float* dOutWorldCasts);
int mi_sphere_cast_host(mi_world* w, uint32_t numQueries, const mi_sphere_cast* queries, uint32_t flags, mi_sphere_hit* out, float* outWorldCasts);

/* Overlap queries: which colliders a volume touches right now: "a trigger you ask once".  One call on the world's stream; like the ray
 * entries it first settles a step whose cluster sweep is not yet known to have completed, uploads, and otherwise does not synchronise
 * with the host; no step buffer and no accumulator is written; numQueries == 0 launches nothing.  (The reference has no counterpart as a
 * query: the rule is this project's, built from the reference's trigger test.)
 * Query: shape and type are exactly what mi_add_collider takes: sphere c3,r | capsule/cylinder A3,B3,r | aabb min3,max3 | obb
 * quat4,center3,radius3 | hull quat4,position3,geometry index (word 7, as a float value).  As there, only the words the type uses are
 * read (4, 7, 7, 6, 10, 8); the rest of the record counts as zero.
 * Volume frame: (pos, rot) is the volume's own pose in the frame of body `mount` at its current pose (the pose array the call itself
 * reads, so poses written through mi_device_state are seen): world rotation = mountRot * rot (quaternion product), world position =
 * mountRot * pos + mountPos, float32 without contraction.  mount == MI_STATIC_BODY: (pos, rot) is the world pose, taken bit for bit:
 * the pose a trigger entity or a static collider has.
 * World record: the volume's world record and world box are what the step builds for a collider with these shape words whose entity has
 * that world pose, bit for bit (csrc/collider_world.h, the function the step itself calls; reference physics.cpp:631-756): a sphere's
 * centre, a capsule's and a cylinder's end points, an OBB's and a hull's composed rotation and position; a cylinder's box is the tight
 * one, e = r * sqrt(max(0, 1 - a_k^2 / dot(a, a))) per axis around both end points; an AABB stays an AABB (its 8 transformed corners'
 * box) only under the rotation (0, 0, 0, 1) exactly and otherwise becomes the OBB {rot, rot * centre + pos, half extents}, type MI_OBB;
 * every other box is that of the 8 transformed corners of the local box (for a hull: of its geometry's box).  With MI_STATIC_BODY and the
 * same (pos, rot, shape) the record and the box equal those of a trigger collider placed there (mi_add_trigger, mi_add_trigger_collider).
 * Switched off: enabled == 0; a mount >= the number of bodies other than MI_STATIC_BODY, a deleted body, in a slab run a body not
 * simulated here; type >= 6; a hull geometry index that is negative, NaN or >= the number of geometries; a world box that is not finite:
 * a coordinate that is infinite or NaN, or min > max on an axis (the box of 8 corners drops a corner's NaN coordinate, so a NaN in the
 * pose can leave an empty box instead).  Such a query has valid = 0, an all-zero block and an all-zero world shape.
 * Candidates are mi_raycast_batch's: the colliders of alive bodies simulated here and, with MI_OVERLAP_STATIC, those of entities without
 * a rigid body; never force-field or trigger colliders, never cloth, never the heightmap terrain.  The colliders of the bodies b with
 * b - excludeFirst < excludeCount, in uint32 arithmetic (the subtraction wraps), are no candidates of this query; static colliders are
 * never excluded.
 * Verdict per candidate: the step's own two-stage decision for a trigger collider.  (1) The candidate's world box, as the step builds it
 * from the current pose, meets the volume's world box inclusively on all three axes: the broadphase's comparison, not (amax < bmin or
 * amin > bmax) per axis.  (2) The trigger's boolean test (overlapColliders, csrc/zone_overlap.h; reference overlapCheck,
 * collision_narrow.cpp:1593-1689) answers true on the two world records, with operand A = the record of the lower collider type after
 * promotion, and for equal types A = the query volume.  It is that test with every property tests/zone64.py documents in float64: the
 * sphere-cylinder cap rule (beside a cap the squared distance is held against the radius, not its square), the epsilon the box-box SAT
 * adds to every |R_ij|, and the GJK walk of the tube-box, cylinder-cylinder and hull pairings, which reports pairs less than about 0.2 m
 * apart (it stops at |dir|^2 < 1e-4 and answers false only on a separating support point).  Stage (1) is part of the rule, not merely
 * pruning: some of those tests answer true beyond the boxes; the step never sees such pairs and the query does not see them either.
 * Output: per query one block of 16 + 8 * maxHits bytes in dOut (device, 8-byte aligned): mi_overlap_summary, then maxHits records of
 * mi_overlap_hit.  numOverlaps counts every overlapping candidate, whatever maxHits is; numWritten = min(numOverlaps, maxHits); the hits
 * are the numWritten lowest collider indices that overlap, ascending; body is MI_STATIC_BODY for a static collider; the slots behind
 * numWritten are zero; valid = 1 for a query that is not switched off, also when nothing overlaps.  maxHits == 0 is a pure count;
 * maxHits > MI_OVERLAP_MAX_HITS returns MI_ERR_INVALID_ARGUMENT.
 * dOutWorldShapes (device, may be NULL) receives 20 floats per query: the 10 shape words of the world record, the bits of its type after
 * promotion, 0, box min xyz, 0, box max xyz, 0.
 * The candidates and the tree over them are mi_raycast_batch's, rebuilt from the current poses at every call in the same buffers;
 * MI_OVERLAP_BRUTE_FORCE asks every candidate instead (same bytes; a yardstick).  Calls of all query kinds may follow each other freely.
 * mi_overlap_host: queries, blocks and world shapes in HOST memory, staged through buffers of the world; returns after the blocks have
 * arrived. */
enum { MI_OVERLAP_STATIC = 1, MI_OVERLAP_BRUTE_FORCE = 2 };
#define MI_OVERLAP_MAX_HITS 1024u
typedef struct mi_overlap_query { float shape[10]; uint32_t type, enabled; float pos[3]; uint32_t mount; float rot[4];
                                  uint32_t excludeFirst, excludeCount, reserved[2]; } mi_overlap_query;      /* 96 bytes */
typedef struct mi_overlap_summary { uint32_t numOverlaps, numWritten, valid, reserved; } mi_overlap_summary; /* 16 bytes */
typedef struct mi_overlap_hit { uint32_t collider, body; } mi_overlap_hit;                                   /* 8 bytes */
int mi_overlap_batch(mi_world* w, uint32_t numQueries, const mi_overlap_query* dQueries, uint32_t maxHits, uint32_t flags, void* dOut, float* dOutWorldShapes);
int mi_overlap_host(mi_world* w, uint32_t numQueries, const mi_overlap_query* queries, uint32_t maxHits, uint32_t flags, void* out, float* outWorldShapes);

/* Contact queries: "a collider you ask once".  For a volume of any of the six collider types at a pose, per candidate collider of the
 * world the manifold the step's narrowphase would build for a collider of that shape at that pose: how deep, in which direction, at
 * which points.  Nothing is added to the world and nothing of the step is touched: the step's pair list, manifolds, EPA lists, counters
 * and mi_debug_narrow_limits read the same before and after a call.  (The reference has no such query: the rule is this project's, built
 * from the reference's narrowphase.)
 * Query: mi_contact_query is mi_overlap_query itself, 96 bytes.  The shape words, the volume frame and mount composition, the world
 * record and world box (csrc/collider_world.h), the switched-off conditions and dOutWorldShapes are mi_overlap_batch's, word for word
 * (above); a query that is switched off has valid = 0 and an all-zero block.
 * Candidates are mi_overlap_batch's: the colliders of alive bodies simulated here and, with MI_CONTACT_QUERY_STATIC, those of entities
 * without a rigid body; never force-field or trigger colliders, never cloth, never the heightmap terrain.  The colliders of the bodies b
 * with b - excludeFirst < excludeCount, in uint32 arithmetic, are no candidates of this query; static colliders are never excluded.
 * Decision per candidate, in two stages.  (1) The candidate's world box meets the volume's world box inclusively on all three axes, as
 * in mi_overlap_batch: part of the rule, not merely pruning.  (2) The step's narrowphase on the two world records: operand A is the
 * record of the lower collider type after promotion, and of equal types A is the VOLUME (the reference gives different manifolds for
 * the two orders of capsule-capsule, cylinder-cylinder and hull-hull).  The code is the step's own device functions (csrc/narrow_pairs.h,
 * narrow_gjk.h, narrow_epa.h): closed forms, box-box SAT with clipping, GJK with EPA, the OBB back-transform; 21 type pairs.
 * Contact: a candidate whose manifold has count > 0.  It is reported as if the volume were operand A: where the collider was A the three
 * sign bits of the normal are flipped and nothing else; points and depths are verbatim.  So the normal points from the volume into the
 * collider, and moving the volume by -|depth| * normal separates the two.  The reference's quirks arrive as they are: AABB-AABB depths
 * carry the sign of the centre offset on the least-overlap axis; a sphere centre inside a box gives depth = radius along +y; a GJK pair
 * of centrally symmetric shapes with coincident centres gives no manifold.  No friction or restitution is reported: a volume has no
 * material.
 * Output: per query one block of 32 + 96 * maxHits bytes in dOut (device, 16-byte aligned): mi_contact_query_summary, then maxHits
 * records of mi_contact_query_record.  numContacts counts every contact, whatever maxHits is; numWritten = min(numContacts, maxHits); the
 * records are the numWritten lowest collider indices with a contact, ascending; the slots behind them are zero; body is MI_STATIC_BODY
 * for a static collider; count is the manifold's 1 .. 4 points, the points behind it are zero; maxDepth is the largest |depth| of the
 * record.  deepestCollider, deepestBody, deepestDepth: the largest maxDepth over ALL contacts (it may lie outside the written records),
 * ties to the lower collider index; without a contact 0xFFFFFFFF, 0xFFFFFFFF and 0.  valid = 1 for a query that is not switched off.
 * maxHits == 0 is a pure count plus the deepest contact; maxHits > MI_CONTACT_QUERY_MAX_HITS returns MI_ERR_INVALID_ARGUMENT.
 * Sizing: the pair list (candidates that pass stage 1) is counted on the device first; the call reads that one 4-byte count back, which
 * synchronises the world's stream once, grows the world's scratch to it and then fills and runs the list: no contact is ever lost to a
 * capacity.  The scratch and the counter block are the query's own and are freed with the world.
 * The candidates and the tree over them are mi_raycast_batch's, rebuilt from the current poses at every call in the same buffers;
 * MI_CONTACT_QUERY_BRUTE_FORCE asks every candidate instead (same bytes; a yardstick).  No result depends on the order of an atomic
 * operation: two calls give the same bytes.  Calls of all query kinds may follow each other freely.
 * mi_contact_query_host: queries, blocks and world shapes in HOST memory, staged through buffers of the world. */
enum { MI_CONTACT_QUERY_STATIC = 1, MI_CONTACT_QUERY_BRUTE_FORCE = 2 };
#define MI_CONTACT_QUERY_MAX_HITS 1024u
typedef mi_overlap_query mi_contact_query;                                                                   /* 96 bytes */
typedef struct mi_contact_query_summary { uint32_t numContacts, numWritten, valid, reserved0, deepestCollider, deepestBody; float deepestDepth;
                                          uint32_t reserved1; } mi_contact_query_summary;                    /* 32 bytes */
typedef struct mi_contact_query_record { uint32_t collider, body, count, reserved; float normal[3], maxDepth;
                                         float points[4][4]; /* xyz, depth */ } mi_contact_query_record;     /* 96 bytes */
int mi_contact_query_batch(mi_world* w, uint32_t numQueries, const mi_contact_query* dQueries, uint32_t maxHits, uint32_t flags, void* dOut, float* dOutWorldShapes);
int mi_contact_query_host(mi_world* w, uint32_t numQueries, const mi_contact_query* queries, uint32_t maxHits, uint32_t flags, void* out, float* outWorldShapes);

/* Contact sensors: what the contacts of the LAST INTERNAL STEP did to a body, summed on the device from the rows its solve left behind.
 * One call on the world's stream; like the ray entries it first settles a step whose cluster sweep is not yet known to have completed
 * (after a give-up the readings describe the redone solve) and otherwise does not synchronise with the host.  The step's buffers are only
 * read.  (The reference has no counterpart: the rule is this project's.)
 * Which step: the last internal step as it was solved.  Poses or velocities written afterwards and a partner body deleted afterwards do
 * not change a reading.  A world that has not stepped since it was created or restored, a sensor `body` >= the number of bodies (or a
 * body added after that step), a deleted body and, in a slab run, a body not simulated here give an all-zero record (valid = 0).  A step
 * without any manifold gives valid = 1 and zeros.
 * Which manifolds: those of the step's schedule whose body A or body B is `body` and whose partner (the other one) passes the filter.  A
 * partner that is the static dummy (static colliders, the heightmap terrain) counts iff partners & MI_CONTACT_STATIC.  Any other partner
 * (dynamic or kinematic) counts iff partners & MI_CONTACT_DYNAMIC and not partner - excludeFirst < excludeCount in uint32 arithmetic
 * (the subtraction wraps, as for mi_sensor_ray; excludeCount == 0 excludes nothing).
 * The sums, over the contacts k < count of those manifolds, with the manifold's normal n, the contact's tangent t, its accumulated
 * impulses ln (normal) and lt (tangent), s = +1 if `body` is B and -1 if it is A, and r = contact point - centre of gravity of `body`:
 *   impulse        += s (ln n + lt t)              linear impulse applied to the body, N s, world frame
 *   angularImpulse += s (ln (r x n) + lt (r x t))  angular impulse about its centre of gravity (the r x vectors are the rows' own)
 *   normalImpulse  += ln
 * numContacts and numManifolds count what was summed.  strongestPartner is the partner of the manifold with the largest sum of ln (summed
 * ((ln0 + ln1) + ln2) + ln3), the lowest manifold slot on a tie, MI_STATIC_BODY for the dummy, 0 without a manifold.
 * Arithmetic: float32 throughout, no fused multiply-add.  A term is formed per component as fl(fl(ln n_x) + fl(lt t_x)), negated for A,
 * and the terms are added to the accumulator (which starts at 0) in ascending manifold slot (mi_debug_read_schedule's values), then
 * ascending contact index; so a reading is a function of the step's rows alone: two calls, and two runs of the same world, return the
 * same bytes.  Several sensors may name one body, with different filters.  numSensors == 0 launches nothing.
 * mi_contact_sensors_host: sensors and readings in HOST memory, staged through buffers of the world; returns after the readings have
 * arrived. */
enum { MI_CONTACT_DYNAMIC = 1, MI_CONTACT_STATIC = 2 };
typedef struct mi_contact_sensor { uint32_t body, partners, excludeFirst, excludeCount; } mi_contact_sensor; /* 16 bytes */
typedef struct mi_contact_reading { float impulse[3], normalImpulse; float angularImpulse[3]; uint32_t numContacts;
                                    uint32_t numManifolds, strongestPartner, valid, reserved; } mi_contact_reading; /* 48 bytes */
int mi_contact_sensors(mi_world* w, uint32_t numSensors, const mi_contact_sensor* dSensors, mi_contact_reading* dOut);
int mi_contact_sensors_host(mi_world* w, uint32_t numSensors, const mi_contact_sensor* sensors, mi_contact_reading* out);

/* Spatial-slab runs (one world per GPU holding ALL bodies, each simulating its slab + ghosts): copy the whole pose / velocity arrays
 * (layout as mi_device_pointers) to / from caller-owned DEVICE buffers, and set the per-body simulate mask (1 byte per body, device
 * memory; 0 = body lives on another GPU: no AABB, no integration).  The halo exchange itself (RCCL send/recv of boundary bodies) is
 * host-side logic above this ABI; the reference has no counterpart (single process). */
int mi_state_to_device_buffers(mi_world* w, void* dPose, void* dVel);
int mi_state_from_device_buffers(mi_world* w, const void* dPose, const void* dVel, const uint8_t* dMask);

/* Ghost-body halo of a spatial slab, on the device (the reference has no counterpart).  mi_slab_configure makes this
 * world rank `rank` of `size` slabs along `axis` owning [lo, hi) (use -/+INFINITY at the ends) with ghosts within `margin` of a cut,
 * and classifies every body from its current pose (owned / ghost of the left or right neighbour / inactive).  Once per step, before
 * mi_step_internal:
 *   mi_slab_pack    one kernel: every owned body within `margin` of a cut goes into that neighbour's message; one that has crossed
 *                   the cut goes with MI_SLAB_MIGRATE and becomes a ghost here.  A message is a caller-owned DEVICE buffer of
 *                   mi_slab_message_bytes(capacity) bytes: a 16-byte header {count, dropped, 0, 0} + `capacity` records of 72 bytes
 *                   {body index, flag, pose 2 x float4, velocity 2 x float4}.  Fixed capacity: no size round trip; `dropped` != 0
 *                   means the band held more bodies than records (raise the capacity).  Pass NULL for a missing neighbour.
 *   (the caller exchanges the messages: one send + one receive per neighbour, e.g. RCCL over xGMI, on the stream of mi_device_pointers)
 *   mi_slab_unpack  two kernels: the received bodies are written (owner if MI_SLAB_MIGRATE, else ghost), ghosts the neighbour no longer
 *                   sends go inactive, the simulate mask follows.
 * Nothing here synchronises with the host.  mi_slab_read_codes copies the per-body codes out (tests / assembling results). */
enum { MI_SLAB_INACTIVE = 0, MI_SLAB_OWNED = 1, MI_SLAB_GHOST_LEFT = 2, MI_SLAB_GHOST_RIGHT = 3, MI_SLAB_GHOST = 0, MI_SLAB_MIGRATE = 1 };
int mi_slab_configure(mi_world* w, uint32_t rank, uint32_t size, uint32_t axis, float lo, float hi, float margin);
uint64_t mi_slab_message_bytes(uint32_t capacity);
int mi_slab_pack(mi_world* w, void* dMessageLeft, void* dMessageRight, uint32_t capacity);
int mi_slab_unpack(mi_world* w, const void* dMessageLeft, const void* dMessageRight, uint32_t capacity);
int mi_slab_read_codes(mi_world* w, uint8_t* outCodes, uint32_t n);

/* ---- inspection of the last internal step (parity tests; mirrors the arrays of physics.cpp:1207-1228) ---------------- */
uint32_t mi_debug_num_pairs(mi_world* w);
int mi_debug_read_pairs(mi_world* w, uint32_t* outPairs2);                              /* broadphase overlaps, (A,B) collider indices */
/* sap_context::sortingAxis (collision_broad.cpp:20-24, 443-444): out[0] = the axis the last step's sweep order refers to (it orients
 * equal-type pairs: A = the collider whose box starts first on it, collision_broad.cpp:127 + collision_narrow.cpp:2374), out[1] = the
 * axis of largest AABB-centre variance of the last step = the next step's axis. */
int mi_debug_sorting_axis(mi_world* w, uint32_t out[2]);
/* High-water marks of the narrowphase's fixed-size GJK / EPA state since the world was created: [0] GJK iterations, [1] EPA triangles,
   [2] EPA edges, [3] EPA border edges of one expansion, [4] EPA runs that stopped at an out-of-memory exit; [5..7] zero. */
int mi_debug_narrow_limits(mi_world* w, uint32_t out[8]);
/* Task colouring of the last step that ran the cluster sweep: [0] tasks the narrow instance coloured, [1] tasks the wide one coloured,
   [2] tasks too large for the narrow instance as the partition counted them, [3] workgroups of the narrow launch (0: not launched),
   [4] most items (manifolds + joints) of a task it takes, [5] its workgroups resident per compute unit; [6..7] zero. */
int mi_debug_color_tasks(mi_world* w, uint32_t out[8]);
/* Sizes of the tasks the last cluster build laid out: outTasks[p] = tasks of phase p (p < 5; [5..7] zero), outItems[p * 512 + t] = manifolds +
   joints of task t of phase p (2560 words; zero beyond a phase's tasks). */
int mi_debug_task_items(mi_world* w, uint32_t* outItems, uint32_t outTasks[8]);
int mi_debug_read_world_colliders(mi_world* w, void* outColliders64, float* outAabbs6); /* worldSpaceColliders / worldSpaceAABBs */
uint32_t mi_debug_num_manifold_slots(mi_world* w);
/* Per candidate pair after prune/classify/bucket (collision_narrow.cpp:2346-2453): ordered collider pair, contact count, and up to 4
 * contacts in the reference's 32-byte collision_contact layout (physics.h:347-354). */
int mi_debug_read_manifolds(mi_world* w, uint32_t* outPairs2, uint32_t* outCounts, void* outContacts4x32, uint32_t* outBodyPairs2);
/* Gauss-Seidel schedule of the contact solve: manifold slots in execution order + colour boundaries. */
uint32_t mi_debug_num_colors(mi_world* w);
int mi_debug_read_schedule(mi_world* w, uint32_t* outManifoldSlots, uint32_t* outColorStart /* numColors+1 */);
/* Accumulated impulses of the last step's contacts: per schedule position (the order of mi_debug_read_schedule) 4 contacts x {normal, tangent}
 * impulse, 8 floats; contacts a manifold does not have read 0.  A copy of what the sweep left behind: it costs the step nothing. */
int mi_debug_read_contact_impulses(mi_world* w, float* outImpulses4x2PerPosition);
/* The direction vectors of the same rows: per schedule position 4 contacts x {t, rA x t, rB x t, rA x n, rB x n}, 15 floats each; contacts a
 * manifold does not have read 0.  Also a plain copy. */
int mi_debug_read_contact_rows(mi_world* w, float* outRows4x15PerPosition);
int mi_debug_read_joint_order(mi_world* w, uint32_t type, uint32_t* outJointIds);
/* The joint update records of the last step (what k_*_init wrote and the solve accumulated its impulses into): numJoints(type) records in
 * joint ORDER (mi_debug_read_joint_order), each MI_JOINT_UPDATE_FLOATS = {20, 20, 36, 56, 80, 72}[type] floats long (layouts: the comments of
 * csrc/k_joints.hip); at most capacityFloats are copied, after the stream has drained.  *outPath (may be null) tells where that step solved
 * its joints: in the launch sweep, inside the cluster sweep, in launches of their own between one cluster launch per iteration, or
 * nowhere (no step yet, or a world without joints). */
enum { MI_JOINT_PATH_LAUNCH_SWEEP = 0, MI_JOINT_PATH_CLUSTER = 1, MI_JOINT_PATH_INTERLEAVED = 2, MI_JOINT_PATH_NONE = 3 };
int mi_debug_read_joint_update(mi_world* w, uint32_t type, float* out, uint32_t capacityFloats, uint32_t* outPath);
int mi_debug_read_body_state(mi_world* w, float* outCog4, float* outInvInertia12, uint32_t nPlusOne); /* rbGlobal: {cog.xyz, invMass}, 3 x float4 columns */
int mi_debug_read_accumulators(mi_world* w, float* outForceTorque6, uint32_t n); /* force.xyz, torque.xyz of the first n bodies: the pushes waiting for the next step */
/* Replay of the reference's own Gauss-Seidel order (SURVEY section 7 / 8c "replay mode"): on != 0 makes the following steps run the reference's
 * greedy 8-wide batch scheduler (scheduleConstraintsSIMD, constraints.cpp:51-184) over the step's contacts in emission order and sweep
 * the batches one after the other (constraints.cpp:3618-3709) instead of the device's own schedule.  A parity facility (one workgroup
 * sweeps all contacts); mi_debug_read_replay_batches returns the last step's batches, 8 entries each: schedule position | contact << 28,
 * 0xFFFFFFFF = empty lane. */
int mi_debug_set_replay(mi_world* w, int on);
uint32_t mi_debug_num_replay_batches(mi_world* w);
int mi_debug_read_replay_batches(mi_world* w, uint32_t* outEntries8PerBatch);
/* Developer timeline of the cluster contact sweep: enable != 0 allocates it (16 rows of 32 u64 per workgroup of the solve launch), out (may be
 * NULL) receives numSlots rows: per task and iteration the wall-clock stamps (10 ns ticks) "shared bodies acquired" / "colours done", the cost of
 * every colour step of iteration 10, and the stages of the task's colouring (csrc/k_cluster_solve.hip documents the rows; tests/cluster_timeline.py prints them). */
int mi_debug_flow_trace(mi_world* w, int enable, unsigned long long* out, uint32_t numSlots);

#ifdef __cplusplus
}
#endif
#endif
