"""MI355X-native rigid-body physics stepper — Python host mirror of the C-ABI in include/mi_physics.h.

`World` exposes the reference engine's physics call shapes (study-game-engines/directx-renderer-kurth, src/physics/physics.h:
collider_component::as*, rigid_body_component(kinematic, gravityFactor, linearDamping, angularDamping),
add*ConstraintFromGlobalPoints, getConstraint, physicsStep(scene, arena, timer, settings, dt)) over libmi_physics.so,
the same way the reference's own Python side binds its Physics-Lib DLL with ctypes (learning/loco_env.py:7-45).
There is no CPU fallback: without the compiled HIP library or without a GPU, constructing a World raises.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libmi_physics.so")

STATIC = 0xFFFFFFFF
SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
DISTANCE, BALL, FIXED, HINGE, CONE_TWIST, SLIDER = range(6)
CONSTRAINT_POD_BYTES = (28, 24, 40, 104, 120, 72)
JOINT_UPDATE_FLOATS = (20, 20, 36, 56, 80, 72)   # MI_JOINT_UPDATE_FLOATS (csrc/world.h)
JOINT_PATH_LAUNCH_SWEEP, JOINT_PATH_CLUSTER, JOINT_PATH_INTERLEAVED, JOINT_PATH_NONE = range(4)

COLLIDER_DTYPE = np.dtype([("shape", "<f4", 10), ("restitution", "<f4"), ("friction", "<f4"), ("density", "<f4"),
                           ("type", "<u4"), ("objectType", "<u4"), ("objectIndex", "<u4")])
CONTACT_DTYPE = np.dtype([("point", "<f4", 3), ("depth", "<f4"), ("normal", "<f4", 3), ("friction_restitution", "<u4")])


class Material(C.Structure):
    _fields_ = [("restitution", C.c_float), ("friction", C.c_float), ("density", C.c_float)]


class Settings(C.Structure):
    """physics_settings (reference physics.h:382-397) minus the std::function callbacks."""
    _fields_ = [("fixedFrameRate", C.c_uint32), ("frameRate", C.c_uint32), ("maxPhysicsIterationsPerFrame", C.c_uint32),
                ("numRigidSolverIterations", C.c_uint32), ("numClothVelocityIterations", C.c_uint32),
                ("numClothPositionIterations", C.c_uint32), ("numClothDriftIterations", C.c_uint32),
                ("simdBroadPhase", C.c_uint32), ("simdNarrowPhase", C.c_uint32), ("simdConstraintSolver", C.c_uint32)]

    def __init__(self, **kw):
        super().__init__(1, 120, 4, 30, 0, 1, 0, 1, 1, 1)
        for k, v in kw.items():
            setattr(self, k, v)


class DeviceState(C.Structure):
    """struct mi_device_state (include/mi_physics.h): the world's device buffers and its stream"""
    _fields_ = [("pose", C.c_void_p), ("pose0", C.c_void_p), ("poseLerp", C.c_void_p), ("vel", C.c_void_p), ("force", C.c_void_p), ("stream", C.c_void_p),
                ("numBodies", C.c_uint32), ("reserved", C.c_uint32)]


class RayHit(C.Structure):
    """struct mi_ray_hit (include/mi_physics.h): one record of mi_raycast_batch, 32 bytes"""
    _fields_ = [("t", C.c_float), ("collider", C.c_uint32), ("body", C.c_uint32), ("hit", C.c_uint32), ("point", C.c_float * 3), ("reserved", C.c_float)]


RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("collider", "<u4"), ("body", "<u4"), ("hit", "<u4"), ("point", "<f4", 3), ("reserved", "<f4")])
RAY_STATIC, RAY_BRUTE_FORCE, RAY_TERRAIN = 1, 2, 4


class SensorRay(C.Structure):
    """struct mi_sensor_ray (include/mi_physics.h): one ray of mi_raycast_sensors in the frame of body `mount`, 48 bytes"""
    _fields_ = [("origin", C.c_float * 3), ("maxT", C.c_float), ("direction", C.c_float * 3), ("enabled", C.c_float),
                ("mount", C.c_uint32), ("excludeFirst", C.c_uint32), ("excludeCount", C.c_uint32), ("reserved", C.c_uint32)]


class SensorHit(C.Structure):
    """struct mi_sensor_hit (include/mi_physics.h): mi_ray_hit and the world-space normal, 48 bytes"""
    _fields_ = [("hit", RayHit), ("normal", C.c_float * 3), ("reserved", C.c_float)]


SENSOR_RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("maxT", "<f4"), ("direction", "<f4", 3), ("enabled", "<f4"),
                             ("mount", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("reserved", "<u4")])
SENSOR_HIT_DTYPE = np.dtype([("t", "<f4"), ("collider", "<u4"), ("body", "<u4"), ("hit", "<u4"), ("point", "<f4", 3), ("reserved", "<f4"),
                             ("normal", "<f4", 3), ("reserved2", "<f4")])
STATIC_BODY = 0xFFFFFFFF   # mi_ray_hit.body of a collider without a rigid body (MI_STATIC_BODY)


class ContactSensor(C.Structure):
    """struct mi_contact_sensor (include/mi_physics.h): a body and the partners whose contacts count, 16 bytes"""
    _fields_ = [("body", C.c_uint32), ("partners", C.c_uint32), ("excludeFirst", C.c_uint32), ("excludeCount", C.c_uint32)]


class ContactReading(C.Structure):
    """struct mi_contact_reading (include/mi_physics.h): what the last step's contacts did to the sensor's body, 48 bytes"""
    _fields_ = [("impulse", C.c_float * 3), ("normalImpulse", C.c_float), ("angularImpulse", C.c_float * 3), ("numContacts", C.c_uint32),
                ("numManifolds", C.c_uint32), ("strongestPartner", C.c_uint32), ("valid", C.c_uint32), ("reserved", C.c_uint32)]


CONTACT_SENSOR_DTYPE = np.dtype([("body", "<u4"), ("partners", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4")])
CONTACT_READING_DTYPE = np.dtype([("impulse", "<f4", 3), ("normalImpulse", "<f4"), ("angularImpulse", "<f4", 3), ("numContacts", "<u4"),
                                  ("numManifolds", "<u4"), ("strongestPartner", "<u4"), ("valid", "<u4"), ("reserved", "<u4")])
CONTACT_DYNAMIC, CONTACT_STATIC = 1, 2   # mi_contact_sensor.partners (MI_CONTACT_*)
class ProximityQuery(C.Structure):
    """struct mi_proximity_query (include/mi_physics.h): one point of mi_proximity in the frame of body `mount`, 32 bytes"""
    _fields_ = [("point", C.c_float * 3), ("radius", C.c_float), ("mount", C.c_uint32), ("excludeFirst", C.c_uint32), ("excludeCount", C.c_uint32),
                ("enabled", C.c_uint32)]


class ProximityReading(C.Structure):
    """struct mi_proximity_reading (include/mi_physics.h): the nearest surface within the radius and the number of colliders within it, 48 bytes"""
    _fields_ = [("distance", C.c_float), ("collider", C.c_uint32), ("body", C.c_uint32), ("found", C.c_uint32), ("point", C.c_float * 3),
                ("numWithin", C.c_uint32), ("normal", C.c_float * 3), ("reserved", C.c_float)]


PROXIMITY_QUERY_DTYPE = np.dtype([("point", "<f4", 3), ("radius", "<f4"), ("mount", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("enabled", "<u4")])
PROXIMITY_READING_DTYPE = np.dtype([("distance", "<f4"), ("collider", "<u4"), ("body", "<u4"), ("found", "<u4"), ("point", "<f4", 3), ("numWithin", "<u4"),
                                    ("normal", "<f4", 3), ("reserved", "<f4")])
PROX_STATIC, PROX_BRUTE_FORCE, PROX_COUNT, PROX_TERRAIN = 1, 2, 4, 8   # mi_proximity's flags (MI_PROX_*)


class ClothCollision(C.Structure):
    """struct mi_cloth_collision (include/mi_physics.h): the settings of a cloth's projection pass, 32 bytes"""
    _fields_ = [("thickness", C.c_float), ("friction", C.c_float), ("flags", C.c_uint32), ("excludeFirst", C.c_uint32), ("excludeCount", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


CLOTH_COLLISION_DTYPE = np.dtype([("thickness", "<f4"), ("friction", "<f4"), ("flags", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("reserved", "<u4", 3)])
CLOTH_COLLIDE_STATIC, CLOTH_COLLIDE_TERRAIN = 1, 2   # mi_cloth_collision.flags (MI_CLOTH_COLLIDE_*)
CLOTH_NO_CONTACT = 0xFFFFFFFF                        # mi_cloth_read_contacts: the particle was pushed off nothing


class SphereCast(C.Structure):
    """struct mi_sphere_cast (include/mi_physics.h): one swept sphere of mi_sphere_cast_batch in the frame of body `mount`, 48 bytes"""
    _fields_ = [("origin", C.c_float * 3), ("maxT", C.c_float), ("direction", C.c_float * 3), ("radius", C.c_float),
                ("mount", C.c_uint32), ("excludeFirst", C.c_uint32), ("excludeCount", C.c_uint32), ("enabled", C.c_uint32)]


class SphereHit(C.Structure):
    """struct mi_sphere_hit (include/mi_physics.h): where the sphere stops (t), on what, the surface point, gap and normal there, 48 bytes"""
    _fields_ = [("t", C.c_float), ("collider", C.c_uint32), ("body", C.c_uint32), ("hit", C.c_uint32), ("point", C.c_float * 3), ("gap", C.c_float),
                ("normal", C.c_float * 3), ("iterations", C.c_uint32)]


SPHERE_CAST_DTYPE = np.dtype([("origin", "<f4", 3), ("maxT", "<f4"), ("direction", "<f4", 3), ("radius", "<f4"),
                              ("mount", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("enabled", "<u4")])
SPHERE_HIT_DTYPE = np.dtype([("t", "<f4"), ("collider", "<u4"), ("body", "<u4"), ("hit", "<u4"), ("point", "<f4", 3), ("gap", "<f4"),
                             ("normal", "<f4", 3), ("iterations", "<u4")])
SPHERE_STATIC, SPHERE_BRUTE_FORCE, SPHERE_TERRAIN = 1, 2, 4   # mi_sphere_cast_batch's flags (MI_SPHERE_*)
# mi_overlap_query / mi_overlap_summary / mi_overlap_hit (include/mi_physics.h): one volume of mi_overlap_batch in the frame of body `mount`, 96 bytes;
# the head of a query's output block, 16 bytes; one of the max_hits records behind it, 8 bytes
OVERLAP_QUERY_DTYPE = np.dtype([("shape", "<f4", 10), ("type", "<u4"), ("enabled", "<u4"), ("pos", "<f4", 3), ("mount", "<u4"), ("rot", "<f4", 4),
                                ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("reserved", "<u4", 2)])
OVERLAP_SUMMARY_DTYPE = np.dtype([("numOverlaps", "<u4"), ("numWritten", "<u4"), ("valid", "<u4"), ("reserved", "<u4")])
OVERLAP_HIT_DTYPE = np.dtype([("collider", "<u4"), ("body", "<u4")])
OVERLAP_STATIC, OVERLAP_BRUTE_FORCE = 1, 2   # mi_overlap_batch's flags (MI_OVERLAP_*)
OVERLAP_MAX_HITS = 1024                      # MI_OVERLAP_MAX_HITS
# mi_contact_query (= mi_overlap_query) / mi_contact_query_summary / mi_contact_query_record (include/mi_physics.h): the head of a query's output
# block, 32 bytes; one of the max_hits records behind it, 96 bytes: points[k] = xyz, depth
CONTACT_QUERY_DTYPE = OVERLAP_QUERY_DTYPE
CONTACT_QUERY_SUMMARY_DTYPE = np.dtype([("numContacts", "<u4"), ("numWritten", "<u4"), ("valid", "<u4"), ("reserved0", "<u4"),
                                        ("deepestCollider", "<u4"), ("deepestBody", "<u4"), ("deepestDepth", "<f4"), ("reserved1", "<u4")])
CONTACT_QUERY_RECORD_DTYPE = np.dtype([("collider", "<u4"), ("body", "<u4"), ("count", "<u4"), ("reserved", "<u4"), ("normal", "<f4", 3), ("maxDepth", "<f4"),
                                       ("points", "<f4", (4, 4))])
CONTACT_QUERY_STATIC, CONTACT_QUERY_BRUTE_FORCE = 1, 2   # mi_contact_query_batch's flags (MI_CONTACT_QUERY_*)
CONTACT_QUERY_MAX_HITS = 1024                            # MI_CONTACT_QUERY_MAX_HITS
TERRAIN_COLLIDER = 0xFFFFFFFE   # mi_ray_hit.collider of a hit on the heightmap terrain (MI_TERRAIN_COLLIDER)


def heightmap_triangle_id(chunks_per_dim, chunk_x, chunk_z, cell_x, cell_z, which):
    """The uint32 triangle id a terrain hit carries in mi_ray_hit.reserved (include/mi_physics.h)"""
    return (((chunk_z * chunks_per_dim + chunk_x) * 16384 + cell_z * 128 + cell_x) * 2 + which) & 0xFFFFFFFF


def heightmap_triangle(triangle, chunks_per_dim):
    """(chunkX, chunkZ, cellX, cellZ, which) of a triangle id: which = 0 is the cell's triangle (A, B, C), 1 is (C, B, D)"""
    triangle = int(triangle)
    which, cell, chunk = triangle & 1, (triangle >> 1) & 16383, triangle >> 15
    return chunk % chunks_per_dim, chunk // chunks_per_dim, cell & 127, cell >> 7, which


class WorldDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("reserveBodies", C.c_uint32), ("reserveColliders", C.c_uint32), ("reservePairs", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("numRigidBodies", C.c_uint32), ("numColliders", C.c_uint32), ("numBroadphaseOverlaps", C.c_uint32), ("numCollisions", C.c_uint32),
                ("numContacts", C.c_uint32), ("numColors", C.c_uint32), ("numJoints", C.c_uint32), ("numInternalSteps", C.c_uint32),
                ("numGraphBuilds", C.c_uint32), ("coloringRounds", C.c_uint32), ("flowProbes", C.c_uint32), ("numFlowRecoveries", C.c_uint32),
                ("msCollidersBroad", C.c_float), ("msNarrow", C.c_float), ("msSolverSetup", C.c_float), ("msSolve", C.c_float),
                ("msIntegrate", C.c_float), ("msTotal", C.c_float),
                ("avgContacts", C.c_float), ("avgCollisions", C.c_float), ("avgColors", C.c_float), ("avgBroadphaseOverlaps", C.c_float), ("avgFlowProbes", C.c_float),
                ("avgSteps", C.c_uint32),
                ("clusterTasks", C.c_uint32 * 5), ("clusterManifolds", C.c_uint32 * 5), ("clusterSharedBodies", C.c_uint32), ("clusterParts", C.c_uint32), ("numNarrowphaseRedone", C.c_uint32)]

    def asdict(self):
        return {n: (list(getattr(self, n)) if n in ("clusterTasks", "clusterManifolds") else getattr(self, n)) for n, _ in self._fields_}


# mi_event (include/mi_physics.h): trigger_event / collision_begin_event / collision_end_event as one record
EVENT_DTYPE = np.dtype([("kind", "<u4"), ("step", "<u4"), ("a", "<u4"), ("b", "<u4"), ("bodyA", "<u4"), ("bodyB", "<u4"),
                        ("position", "<f4", 3), ("normal", "<f4", 3), ("relativeVelocity", "<f4", 3)])
TRIGGER_ENTER, TRIGGER_LEAVE, COLLISION_BEGIN, COLLISION_END = range(4)

EXPORTED_SYMBOLS = [
    "mi_world_create", "mi_world_destroy", "mi_last_error", "mi_snapshot_size", "mi_snapshot_save", "mi_world_restore", "mi_add_body", "mi_add_hull_geometry", "mi_add_collider", "mi_add_static_collider",
    "mi_add_distance_constraint_local", "mi_add_distance_constraint_global", "mi_add_ball_constraint_local", "mi_add_ball_constraint_global",
    "mi_add_fixed_constraint_global", "mi_add_hinge_constraint_global", "mi_add_cone_twist_constraint_global", "mi_add_slider_constraint_global", "mi_add_constraint",
    "mi_constraint_get", "mi_constraint_set", "mi_delete_constraint", "mi_delete_all_constraints", "mi_delete_all_constraints_from_body", "mi_delete_body",
    "mi_add_force_field", "mi_set_force_field", "mi_add_trigger", "mi_add_force_field_collider", "mi_add_trigger_collider", "mi_set_force_field_transform", "mi_set_trigger_transform", "mi_enable_collision_events", "mi_drain_events",
    "mi_set_heightmap", "mi_heightmap_set_chunk", "mi_heightmap_update", "mi_heightmap_height_at",
    "mi_add_cloth", "mi_cloth_set_fixed_vertices", "mi_cloth_set_properties", "mi_set_cloth_iterations", "mi_num_cloths", "mi_cloth_num_particles", "mi_cloth_read",
    "mi_cloth_set_collision", "mi_cloth_get_collision", "mi_cloth_read_contacts", "mi_debug_set_cloth_collision_brute_force",
    "mi_test_physics_interaction", "mi_apply_force_torque", "mi_set_velocity",
    "mi_set_transform", "mi_write_transforms", "mi_write_velocities", "mi_step", "mi_step_internal", "mi_synchronize", "mi_read_transforms", "mi_read_velocities", "mi_read_mass_properties",
    "mi_get_stats", "mi_enable_validation", "mi_enable_stage_timing", "mi_num_bodies", "mi_num_colliders", "mi_device_pointers", "mi_state_to_device_buffers", "mi_state_from_device_buffers", "mi_slab_configure", "mi_slab_message_bytes", "mi_slab_pack", "mi_slab_unpack", "mi_slab_read_codes", "mi_debug_num_pairs", "mi_debug_read_pairs", "mi_debug_sorting_axis", "mi_debug_narrow_limits", "mi_debug_color_tasks", "mi_debug_task_items",
    "mi_debug_read_world_colliders", "mi_debug_num_manifold_slots", "mi_debug_read_manifolds", "mi_debug_num_colors", "mi_debug_read_schedule", "mi_debug_read_contact_impulses",
    "mi_debug_read_joint_order", "mi_debug_read_joint_update", "mi_debug_read_body_state", "mi_debug_read_accumulators", "mi_debug_flow_trace",
    "mi_debug_set_replay", "mi_debug_num_replay_batches", "mi_debug_read_replay_batches",
    "mi_device_state", "mi_joint_device_pods", "mi_test_physics_interaction_batch", "mi_raycast_batch", "mi_raycast_host",
    "mi_raycast_sensors", "mi_raycast_sensors_host",
    "mi_contact_sensors", "mi_contact_sensors_host", "mi_debug_read_contact_rows",
    "mi_proximity", "mi_proximity_host",
    "mi_sphere_cast_batch", "mi_sphere_cast_host",
    "mi_overlap_batch", "mi_overlap_host",
    "mi_contact_query_batch", "mi_contact_query_host",
]


def build(force=False):
    """Compile libmi_physics.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j6"], stdout=subprocess.DEVNULL)
    build_locomotion()
    return _LIB_PATH


LOCOMOTION_LIB_PATH = os.path.join(_HERE, "libmi_locomotion.so")
LOCOMOTION_SYMBOLS = ["getPhysicsStateSize", "getPhysicsActionSize", "getPhysicsRanges", "resetPhysics", "updatePhysics", "setPhysicsSeed",
                      "resetPhysicsBatch", "updatePhysicsBatch", "updatePhysicsBatchDevice", "resetPhysicsBatchEnvs", "observePhysicsBatch",
                      "getPhysicsBatchWorld", "getPhysicsBatchStream", "getPhysicsBatchPushes",
                      "setPhysicsPolicy", "inferPhysicsPolicy", "updatePhysicsPolicy", "inferPhysicsBatchDevice", "updatePhysicsBatchPolicy",
                      "updatePhysicsBatchPolicyDevice", "rolloutPhysicsBatchDevice",
                      "setPhysicsValueNetwork", "inferPhysicsValue", "inferPhysicsBatchValueDevice", "setPhysicsActionStd", "samplePhysicsBatchNoiseDevice",
                      "samplePhysicsNoise", "samplePhysicsNoiseUniforms", "getPhysicsBatchNoiseCounter", "collectPhysicsBatchDevice", "gaePhysicsBatchDevice",
                      "beginPhysicsBatchTraining", "endPhysicsBatchTraining", "updatePhysicsBatchPPODevice", "gradientsPhysicsBatchPPODevice",
                      "readPhysicsBatchPolicy", "readPhysicsBatchValueNetwork", "readPhysicsBatchLogStd"]
_HIPCC = "/opt/rocm/bin/hipcc"


def build_locomotion():
    """libmi_locomotion.so: the reference's ragdoll RL environment (learned_locomotion.cpp:395-489) as host C++ over the C-ABI (g++),
    plus the batched environments of host/locomotion_batch.hip and the PPO gradient step of host/locomotion_update.hip (hipcc, gfx950,
    strict fp32 like libmi_physics.so)."""
    host = os.path.join(_HERE, "host")
    include = "-I" + os.path.join(os.path.dirname(_HERE), "include")
    cpp, hips = os.path.join(host, "locomotion_env.cpp"), [os.path.join(host, "locomotion_batch.hip"), os.path.join(host, "locomotion_update.hip")]
    headers = [os.path.join(host, h) for h in ("locomotion_shared.h", "locomotion_policy.h", "locomotion_layers.h", "locomotion_update.h")]
    deps = [cpp] + hips + headers + [os.path.join(os.path.dirname(_HERE), "include", "mi_physics.h"), _LIB_PATH]
    if os.path.exists(LOCOMOTION_LIB_PATH) and os.path.getmtime(LOCOMOTION_LIB_PATH) >= max(os.path.getmtime(p) for p in deps):
        return LOCOMOTION_LIB_PATH
    cpp_o, hip_os = os.path.join(host, "locomotion_env.o"), [h[:-len(".hip")] + ".o" for h in hips]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", include, "-c", cpp, "-o", cpp_o])
    for hip, hip_o in zip(hips, hip_os):
        subprocess.check_call([_HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", include, "-c", hip, "-o", hip_o])
    subprocess.check_call([_HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", cpp_o] + hip_os + ["-L" + _HERE, "-lmi_physics", "-Wl,-rpath,$ORIGIN",
                           "-o", LOCOMOTION_LIB_PATH])
    return LOCOMOTION_LIB_PATH


_lib = None


def load_library():
    """dlopen the C-ABI library.  Raises if it has not been built — there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError("libmi_physics.so is missing: run __graft_entry__.build() (hipcc) first; there is no CPU fallback")
        lib = C.CDLL(_LIB_PATH)
        lib.mi_world_create.restype = C.c_void_p
        lib.mi_world_restore.restype = C.c_void_p
        lib.mi_snapshot_size.restype = C.c_uint64
        lib.mi_slab_message_bytes.restype = C.c_uint64
        lib.mi_last_error.restype = C.c_char_p
        lib.mi_heightmap_height_at.restype = C.c_float
        for name in EXPORTED_SYMBOLS:
            fn = getattr(lib, name)
            if name.startswith("mi_add_") or name in ("mi_num_bodies", "mi_num_colliders", "mi_debug_num_pairs", "mi_debug_num_manifold_slots", "mi_debug_num_colors", "mi_drain_events", "mi_num_cloths", "mi_cloth_num_particles"):
                fn.restype = C.c_uint32
        _lib = lib
    return _lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_tensor(a):
    """a torch tensor?  (without importing torch for callers who pass numpy)"""
    return not isinstance(a, np.ndarray) and type(a).__module__.startswith("torch")


def _ray_flags(static, brute_force, terrain):
    return (RAY_STATIC if static else 0) | (RAY_BRUTE_FORCE if brute_force else 0) | (RAY_TERRAIN if terrain else 0)


def _fill_mount(rec, mount, exclude_first, exclude_count):
    """mount (None: world space) and the exclusion range (None: nothing) of SENSOR_RAY_DTYPE / PROXIMITY_QUERY_DTYPE / SPHERE_CAST_DTYPE records"""
    rec["mount"] = STATIC_BODY if mount is None else np.asarray(mount, np.uint32)
    rec["excludeFirst"] = 0 if exclude_first is None else np.asarray(exclude_first, np.uint32)
    rec["excludeCount"] = 0 if exclude_count is None else np.asarray(exclude_count, np.uint32)


def _hit_tuple(hits, terrain):
    """(t, collider, body, hit, point[, triangle]) of RAY_HIT_DTYPE / SENSOR_HIT_DTYPE records"""
    out = (hits["t"].copy(), hits["collider"].copy(), hits["body"].copy(), hits["hit"].copy(), hits["point"].copy())
    return out + (hits["reserved"].view(np.uint32).copy(),) if terrain else out


class PhysicsError(RuntimeError):
    pass


class World:
    """One physics world on one MI355X.  Method names follow the reference's free functions / component factories."""

    def __init__(self, device=-1, reserve_bodies=0, reserve_colliders=0, reserve_pairs=0):
        self.lib = load_library()
        desc = WorldDesc(device, reserve_bodies, reserve_colliders, reserve_pairs)
        h = self.lib.mi_world_create(C.byref(desc))
        if not h:
            raise PhysicsError("mi_world_create failed: %s" % (self.lib.mi_last_error(None) or b"").decode())
        self.w = C.c_void_p(h)
        self.timer = C.c_float(0.0)

    def snapshot(self):
        """Self-contained binary image of the world (checkpoint); World.restore(blob) continues it bit-identically."""
        n = int(self.lib.mi_snapshot_size(self.w))
        buf = np.zeros(n, np.uint8)
        self._check(self.lib.mi_snapshot_save(self.w, _p(buf), C.c_uint64(n)))
        return buf.tobytes()

    @classmethod
    def restore(cls, blob, device=-1):
        self = cls.__new__(cls)
        self.lib = load_library()
        desc = WorldDesc(device, 0, 0, 0)
        buf = np.frombuffer(blob, np.uint8)
        h = self.lib.mi_world_restore(C.byref(desc), _p(buf), C.c_uint64(len(buf)))
        if not h:
            raise PhysicsError("mi_world_restore failed: %s" % (self.lib.mi_last_error(None) or b"").decode())
        self.w = C.c_void_p(h)
        self.timer = C.c_float(0.0)
        return self

    def close(self):
        if getattr(self, "w", None):
            self.lib.mi_world_destroy(self.w)
            self.w = None

    def __del__(self):
        self.close()

    def _check(self, code):
        if code:
            raise PhysicsError("mi_physics error %d: %s" % (code, (self.lib.mi_last_error(self.w) or b"").decode()))

    def _id(self, v):
        if v == 0xFFFFFFFF:
            raise PhysicsError((self.lib.mi_last_error(self.w) or b"invalid id").decode())
        return v

    # ---- add API ------------------------------------------------------------------------------------------
    def add_body(self, pos, rot=(0, 0, 0, 1), kinematic=False, gravity_factor=1.0, linear_damping=0.4, angular_damping=0.4):
        return self._id(self.lib.mi_add_body(self.w, int(kinematic), C.c_float(gravity_factor), C.c_float(linear_damping), C.c_float(angular_damping), _f(pos), _f(rot)))

    def add_hull_geometry(self, vertices, triangles):
        """bounding_hull_geometry::fromMesh (reference bounding_volumes.cpp:1394-1452): convex vertex set + outward-facing triangles."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3); t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        return self._id(self.lib.mi_add_hull_geometry(self.w, _f(v), C.c_uint32(len(v)), t.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(len(t))))

    def add_collider(self, body, ctype, shape, material):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        m = Material(*material)
        return self._id(self.lib.mi_add_collider(self.w, C.c_uint32(body), C.c_uint32(ctype), _f(s), C.byref(m)))

    def add_static_collider(self, ctype, shape, material, pos=(0, 0, 0), rot=(0, 0, 0, 1)):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        m = Material(*material)
        return self._id(self.lib.mi_add_static_collider(self.w, C.c_uint32(ctype), _f(s), C.byref(m), _f(pos), _f(rot)))

    # ---- force fields, triggers, events (physics.h:182-203, 356-380; physics.cpp:759-787, 952-1178) ----
    def add_force_field(self, force, pos=None, rot=None):
        """force_field_component: without colliders it acts on every body, with colliders on the bodies overlapping them."""
        return self._id(self.lib.mi_add_force_field(self.w, _f(force), _f(pos) if pos is not None else None, _f(rot) if rot is not None else None))

    def set_force_field(self, field, force):
        self._check(self.lib.mi_set_force_field(self.w, C.c_uint32(field), _f(force)))

    def add_trigger(self, pos=None, rot=None):
        """trigger_component: enter / leave events for rigid bodies overlapping its colliders come out of drain_events()."""
        return self._id(self.lib.mi_add_trigger(self.w, _f(pos) if pos is not None else None, _f(rot) if rot is not None else None))

    def add_force_field_collider(self, field, ctype, shape):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self._id(self.lib.mi_add_force_field_collider(self.w, C.c_uint32(field), C.c_uint32(ctype), _f(s)))

    def add_trigger_collider(self, trigger, ctype, shape):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self._id(self.lib.mi_add_trigger_collider(self.w, C.c_uint32(trigger), C.c_uint32(ctype), _f(s)))

    def set_force_field_transform(self, field, pos, rot=(0, 0, 0, 1)):
        self._check(self.lib.mi_set_force_field_transform(self.w, C.c_uint32(field), _f(pos), _f(rot)))

    def set_trigger_transform(self, trigger, pos, rot=(0, 0, 0, 1)):
        self._check(self.lib.mi_set_trigger_transform(self.w, C.c_uint32(trigger), _f(pos), _f(rot)))

    def enable_collision_events(self, begin=True, end=True):
        """physics_settings::collisionBeginCallback / collisionEndCallback set; enable before the first step."""
        self._check(self.lib.mi_enable_collision_events(self.w, int(begin), int(end)))

    def drain_events(self, capacity=1 << 16):
        """Pending trigger / collision events in the reference's callback order, as a structured array (EVENT_DTYPE)."""
        chunks = []
        while True:
            out = np.zeros(capacity, EVENT_DTYPE)
            n = self.lib.mi_drain_events(self.w, _p(out), C.c_uint32(capacity))
            chunks.append(out[:n])
            if n < capacity:
                break
        return np.concatenate(chunks) if len(chunks) > 1 else chunks[0]

    # ---- heightmap terrain (heightmap_collider.h:127-152) ----
    def set_heightmap(self, chunks_per_dim, chunk_size, material, min_corner, amplitude_scale):
        m = Material(*material)
        self._terrain_chunks_per_dim = int(chunks_per_dim)
        self._check(self.lib.mi_set_heightmap(self.w, C.c_uint32(chunks_per_dim), C.c_float(chunk_size), C.byref(m), _f(min_corner), C.c_float(amplitude_scale)))

    def heightmap_set_chunk(self, x, z, heights):
        h = np.ascontiguousarray(heights, np.uint16).reshape(129, 129)
        self._check(self.lib.mi_heightmap_set_chunk(self.w, C.c_uint32(x), C.c_uint32(z), _p(h)))

    def heightmap_update(self, min_corner, amplitude_scale):
        self._check(self.lib.mi_heightmap_update(self.w, _f(min_corner), C.c_float(amplitude_scale)))

    def heightmap_height_at(self, x, z):
        return float(self.lib.mi_heightmap_height_at(self.w, C.c_float(x), C.c_float(z)))

    def heightmap_triangle(self, triangle, chunks_per_dim=None):
        """(chunkX, chunkZ, cellX, cellZ, which) of the triangle id of a terrain hit (raycast(..., terrain=True)).  A restored world
        does not know chunks_per_dim: pass it."""
        cpd = chunks_per_dim if chunks_per_dim is not None else getattr(self, "_terrain_chunks_per_dim", None)
        if not cpd:
            raise ValueError("heightmap_triangle: no heightmap was set on this World object (pass chunks_per_dim)")
        return heightmap_triangle(triangle, cpd)

    # ---- cloth (cloth.h:5-60; stepped after the rigid bodies, physics.cpp:1354-1358) ----
    def add_cloth(self, width, height, grid_x, grid_y, total_mass, stiffness=0.5, damping=0.3, gravity_factor=1.0):
        return self._id(self.lib.mi_add_cloth(self.w, C.c_float(width), C.c_float(height), C.c_uint32(grid_x), C.c_uint32(grid_y), C.c_float(total_mass),
                                              C.c_float(stiffness), C.c_float(damping), C.c_float(gravity_factor)))

    def cloth_set_fixed_vertices(self, cloth, pos, rot=(0, 0, 0, 1), move_rigid=False):
        self._check(self.lib.mi_cloth_set_fixed_vertices(self.w, C.c_uint32(cloth), _f(pos), _f(rot), int(move_rigid)))

    def cloth_set_properties(self, cloth, total_mass, stiffness, damping, gravity_factor):
        self._check(self.lib.mi_cloth_set_properties(self.w, C.c_uint32(cloth), C.c_float(total_mass), C.c_float(stiffness), C.c_float(damping), C.c_float(gravity_factor)))

    def set_cloth_iterations(self, velocity=0, position=1, drift=0):
        self._check(self.lib.mi_set_cloth_iterations(self.w, C.c_uint32(velocity), C.c_uint32(position), C.c_uint32(drift)))

    def set_cloth_colour_order(self, on=True):
        """The device always solves cloth constraints in colour order; present so that a scene instantiates into either world."""

    def cloth_state(self, cloth):
        n = self.lib.mi_cloth_num_particles(self.w, C.c_uint32(cloth))
        p = np.zeros((n, 3), np.float32); v = np.zeros((n, 3), np.float32)
        self._check(self.lib.mi_cloth_read(self.w, C.c_uint32(cloth), _p(p), _p(v)))
        return p, v

    def cloth_set_collision(self, cloth, thickness, friction=0.0, static=True, terrain=False, exclude=(0, 0)):
        """mi_cloth_set_collision: from the next internal step on the cloth's free particles are pushed to `thickness` from the nearest
        collider surface (static: also the colliders without a rigid body; terrain: also the heightmap) and lose their approaching
        velocity relative to it, with Coulomb `friction` on the rest (the rule is in include/mi_physics.h).  exclude = (first, count): the
        colliders of these bodies are not met (the body the cloth hangs from)."""
        s = ClothCollision(thickness, friction, (CLOTH_COLLIDE_STATIC if static else 0) | (CLOTH_COLLIDE_TERRAIN if terrain else 0), exclude[0], exclude[1])
        self._check(self.lib.mi_cloth_set_collision(self.w, C.c_uint32(cloth), C.byref(s)))

    def cloth_clear_collision(self, cloth):
        self._check(self.lib.mi_cloth_set_collision(self.w, C.c_uint32(cloth), None))

    def cloth_collision(self, cloth):
        """None while collision is off, else dict(thickness, friction, static, terrain, exclude)"""
        s, on = ClothCollision(), C.c_int(0)
        self._check(self.lib.mi_cloth_get_collision(self.w, C.c_uint32(cloth), C.byref(s), C.byref(on)))
        if not on.value:
            return None
        return dict(thickness=s.thickness, friction=s.friction, static=bool(s.flags & CLOTH_COLLIDE_STATIC), terrain=bool(s.flags & CLOTH_COLLIDE_TERRAIN),
                    exclude=(s.excludeFirst, s.excludeCount))

    def cloth_contacts(self, cloth):
        """uint32 [n]: the collider every particle was pushed off in the last internal step (TERRAIN_COLLIDER: the heightmap;
        CLOTH_NO_CONTACT: none)"""
        out = np.zeros(self.lib.mi_cloth_num_particles(self.w, C.c_uint32(cloth)), np.uint32)
        self._check(self.lib.mi_cloth_read_contacts(self.w, C.c_uint32(cloth), _p(out)))
        return out

    def set_cloth_collision_brute_force(self, on=True):
        """debug: the projection pass asks every candidate instead of walking the tree (same bytes)"""
        self._check(self.lib.mi_debug_set_cloth_collision_brute_force(self.w, int(on)))

    def add_constraint(self, ctype, a, b, pod):
        """addConstraint(a, b, const T&) (reference physics.h:239-244): the constraint as its POD bytes (layout of constraint_get)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(pod), np.uint8))
        assert len(buf) == (28, 24, 40, 104, 120, 72)[ctype]
        cid = self.lib.mi_add_constraint(self.w, C.c_uint32(ctype), C.c_uint32(a), C.c_uint32(b), _p(buf))
        if cid == 0xFFFFFFFF:
            self._check(1)
        return cid

    def add_distance_constraint_local(self, a, b, la, lb, distance):
        return self._id(self.lib.mi_add_distance_constraint_local(self.w, a, b, _f(la), _f(lb), C.c_float(distance)))

    def add_distance_constraint_global(self, a, b, ga, gb):
        return self._id(self.lib.mi_add_distance_constraint_global(self.w, a, b, _f(ga), _f(gb)))

    def add_ball_constraint_local(self, a, b, la, lb):
        return self._id(self.lib.mi_add_ball_constraint_local(self.w, a, b, _f(la), _f(lb)))

    def add_ball_constraint_global(self, a, b, g):
        return self._id(self.lib.mi_add_ball_constraint_global(self.w, a, b, _f(g)))

    def add_fixed_constraint_global(self, a, b, g):
        return self._id(self.lib.mi_add_fixed_constraint_global(self.w, a, b, _f(g)))

    def add_hinge_constraint_global(self, a, b, anchor, axis, min_limit=1.0, max_limit=-1.0):
        return self._id(self.lib.mi_add_hinge_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(min_limit), C.c_float(max_limit)))

    def add_cone_twist_constraint_global(self, a, b, anchor, axis, swing_limit, twist_limit):
        return self._id(self.lib.mi_add_cone_twist_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(swing_limit), C.c_float(twist_limit)))

    def add_slider_constraint_global(self, a, b, anchor, axis, min_limit=1.0, max_limit=-1.0):
        return self._id(self.lib.mi_add_slider_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(min_limit), C.c_float(max_limit)))

    def constraint_get(self, ctype, cid, nbytes=None):
        buf = np.zeros(nbytes or CONSTRAINT_POD_BYTES[ctype], np.uint8)
        self._check(self.lib.mi_constraint_get(self.w, ctype, cid, _p(buf)))
        return buf

    def constraint_set(self, ctype, cid, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        self._check(self.lib.mi_constraint_set(self.w, ctype, cid, _p(buf)))

    def delete_constraint(self, ctype, cid):
        self._check(self.lib.mi_delete_constraint(self.w, ctype, cid))

    def delete_all_constraints_from_body(self, body):
        self._check(self.lib.mi_delete_all_constraints_from_body(self.w, C.c_uint32(body)))

    def delete_body(self, body):
        self._check(self.lib.mi_delete_body(self.w, C.c_uint32(body)))

    def test_physics_interaction(self, origin, direction, strength=1000.0):
        """testPhysicsInteraction(scene, ray, strength) — reference physics.h:404.  Returns the pushed body's index or None."""
        r = self.lib.mi_test_physics_interaction(self.w, _f(origin), _f(direction), C.c_float(strength))
        return r - 1 if r > 0 else None

    def device_state(self):
        """mi_device_state: the device addresses of pose, pose0, poseLerp, vel, force and the world's stream, after an upload."""
        ds = DeviceState()
        self._check(self.lib.mi_device_state(self.w, C.byref(ds)))
        return ds

    def _interaction_batch(self, rays, first_body, bodies_per_ray, fill, extra):
        """(status code, int32 results [n + extra], every entry `fill` before the launch) of mi_test_physics_interaction_batch"""
        import torch
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        dev = torch.device("cuda", torch.cuda.current_device())
        ext = torch.cuda.ExternalStream(self.device_state().stream or 0, device=dev)
        with torch.cuda.stream(ext):
            d_rays = torch.from_numpy(rays).to(dev) if n else torch.zeros((1, 8), dtype=torch.float32, device=dev)
            d_out = torch.full((n + extra,), fill, dtype=torch.int32, device=dev)
            code = self.lib.mi_test_physics_interaction_batch(self.w, C.c_uint32(n), C.c_uint32(first_body), C.c_uint32(bodies_per_ray),
                                                              C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_out.data_ptr()))
            ext.synchronize()
            out = d_out.cpu().numpy()
        return code, out

    def test_physics_interaction_batch(self, rays, first_body, bodies_per_ray, fill=0, extra=0):
        """mi_test_physics_interaction_batch: test_physics_interaction for rays [n, 8] = origin, strength, direction, enabled, ray i against
        the bodies first_body + i * bodies_per_ray ... only, as one kernel on the world's stream (import torch before the first World).
        Returns int32 [n + extra]: 1 + the pushed body or 0 per ray; the buffer holds `fill` before the launch."""
        code, out = self._interaction_batch(rays, first_body, bodies_per_ray, fill, extra)
        self._check(code)
        return out

    # The query methods below hand one of these helpers a call(n, in, out, aux): the C entry on addresses (None: a null pointer).
    def _query_in_place(self, name, call, q, cols_in, cols_out, cols_aux=0):
        """A device entry on the caller's device tensor q (float32, contiguous, [n, cols_in]): outputs [n, cols_out] and, if wanted,
        [n, cols_aux], enqueued on the world's stream behind the caller's current stream, which then waits for it; no host synchronisation."""
        import torch
        if not q.is_cuda or q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != cols_in or not q.is_contiguous():
            raise ValueError("%s: a device tensor must be float32, contiguous and [n, %d]" % (name, cols_in))
        ext = torch.cuda.ExternalStream(self.device_state().stream or 0, device=q.device)
        ext.wait_stream(torch.cuda.current_stream(q.device))   # q was written on the caller's stream
        with torch.cuda.stream(ext):
            out = torch.empty((q.shape[0], cols_out), dtype=torch.float32, device=q.device)
            aux = torch.empty((q.shape[0], cols_aux), dtype=torch.float32, device=q.device) if cols_aux else None
            self._check(call(q.shape[0], q.data_ptr(), out.data_ptr(), aux.data_ptr() if cols_aux else None))
        q.record_stream(ext)
        torch.cuda.current_stream(q.device).wait_stream(ext)   # stream order, not a host synchronisation
        return (out, aux) if cols_aux else out

    def _query_numpy(self, call, rec, out, aux=None, device=False):
        """numpy records `rec` [n] in, `out` [n] and `aux` [n, k] (or None) filled: `call` is a _host entry on the arrays themselves or,
        with device=True, a device entry on device tensors made here."""
        n = len(rec)
        if not n:
            self._check(call(0, None, None, None))
        elif not device:
            self._check(call(n, rec.ctypes.data, out.ctypes.data, aux.ctypes.data if aux is not None else None))
        else:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            d_in = torch.from_numpy(rec.view(np.int32).reshape(n, -1).copy()).to(dev)
            d_out = torch.empty((n, out.itemsize // 4), dtype=torch.float32, device=dev)
            d_aux = torch.empty(aux.shape, dtype=torch.float32, device=dev) if aux is not None else None
            torch.cuda.current_stream(dev).synchronize()   # the records are on the device before the world's stream reads them
            self._check(call(n, d_in.data_ptr(), d_out.data_ptr(), d_aux.data_ptr() if aux is not None else None))
            self.synchronize()
            out[:] = d_out.cpu().numpy().view(out.dtype).reshape(n)
            if aux is not None:
                aux[:] = d_aux.cpu().numpy()

    def raycast(self, rays, static=True, brute_force=False, terrain=False):
        """mi_raycast_batch: rays [n, 8] = origin, maxT, direction, enabled, each against every candidate collider of the world (with
        `static` also the colliders of entities without a rigid body); nothing is pushed.  brute_force: every ray against every
        candidate, no tree (same answers).  terrain: the heightmap's triangles are candidates too (RAY_TERRAIN; nothing changes without a
        heightmap): such a hit has collider TERRAIN_COLLIDER, body STATIC_BODY and a triangle id (heightmap_triangle).
        numpy rays are copied to the device and the hits back: returns (t [n], collider [n], body [n], hit [n], point [n, 3]); body is
        STATIC_BODY for a static collider, everything 0 for a miss.  With terrain=True a sixth array follows: triangle [n] uint32, 0 where
        the hit is not on the terrain.
        A torch tensor on the device (float32, contiguous) is used in place: returns one float32 tensor [n, 8] of mi_ray_hit records
        (columns 1..3 hold the bits of collider, body, hit, column 7 those of the triangle id: view them with .view(torch.int32)),
        enqueued on the world's stream with no synchronisation."""
        flags = _ray_flags(static, brute_force, terrain)

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(flags), C.c_void_p(d_out))
        if _is_tensor(rays):
            return self._query_in_place("raycast", entry(self.lib.mi_raycast_batch), rays, 8, 8)
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros(len(rays), RAY_HIT_DTYPE)
        self._query_numpy(entry(self.lib.mi_raycast_host), rays, hits)
        return _hit_tuple(hits, terrain)

    def raycast_sensors(self, rays, mount=None, exclude_first=None, exclude_count=None, static=True, brute_force=False, terrain=False, world_rays=False):
        """mi_raycast_sensors: rays [n, 8] = origin, maxT, direction, enabled in the frame of body mount[i] at its current pose
        (mount: an index or an array [n]; STATIC_BODY: the ray is in world space), each blind to the colliders of the bodies
        exclude_first[i] ... exclude_first[i] + exclude_count[i] - 1 (None: nothing is excluded); flags as raycast.
        numpy rays go through the world's staging buffers (mi_raycast_sensors_host): returns raycast's tuple (t, collider, body, hit,
        point[, triangle with terrain=True]) plus normal [n, 3], and plus the world rays [n, 8] with world_rays=True.
        A torch tensor on the device (float32, contiguous, [n, 12]: the 8 floats and the bits of mount, excludeFirst, excludeCount, 0;
        mount and the exclusion arguments are then not used) is cast in place: returns one float32 tensor [n, 12] of mi_sensor_hit
        records (columns 8..10 the normal), with world_rays=True a tuple with the [n, 8] world rays; enqueued on the world's stream
        with no synchronisation.  (The rays tensor is recorded on that stream, as in raycast: release it before close().)"""
        flags = _ray_flags(static, brute_force, terrain)

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(flags), C.c_void_p(d_out), C.c_void_p(d_aux))
        if _is_tensor(rays):
            return self._query_in_place("raycast_sensors", entry(self.lib.mi_raycast_sensors), rays, 12, 12, 8 if world_rays else 0)
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        rec = np.zeros(n, SENSOR_RAY_DTYPE)
        rec["origin"], rec["maxT"], rec["direction"], rec["enabled"] = rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7]
        _fill_mount(rec, mount, exclude_first, exclude_count)
        hits, wr = np.zeros(n, SENSOR_HIT_DTYPE), np.zeros((n, 8), np.float32)
        self._query_numpy(entry(self.lib.mi_raycast_sensors_host), rec, hits, wr if world_rays else None)
        out = _hit_tuple(hits, terrain) + (hits["normal"].copy(),)
        return out + (wr,) if world_rays else out

    def proximity(self, points, radius=np.inf, mount=None, exclude_first=None, exclude_count=None, static=True, brute_force=False, count=True,
                  world_points=False, device=False, terrain=False):
        """mi_proximity: per point the nearest collider surface within `radius` (signed distance, negative inside; closest point; outward
        normal) and, with `count`, the number of colliders within it (the rule is in include/mi_physics.h).  terrain: the heightmap is one more
        candidate, the solid under its surface (PROX_TERRAIN; nothing changes without a heightmap): such a reading has collider
        TERRAIN_COLLIDER, body STATIC_BODY, a negative distance below the surface, and in `reserved` the bits of the nearest triangle's id
        (reading["reserved"].view(np.uint32), for heightmap_triangle); it counts 1 in numWithin; exclusion never hides it.
        points [n, 3] in the frame of body mount[i] at its current pose (mount: an index or an array [n]; None / STATIC_BODY: world space);
        radius: a number or an array [n], may be inf; blind to the colliders of the bodies exclude_first[i] ... + exclude_count[i] - 1.
        `points` may also be a PROXIMITY_QUERY_DTYPE array (radius, mount and the exclusion arguments are then not used).
        numpy queries return a PROXIMITY_READING_DTYPE array [n], with world_points=True a tuple with the world points [n, 4] = xyz, radius:
        through the world's staging buffers (mi_proximity_host), or with device=True through device tensors of the caller's (mi_proximity).
        A torch tensor on the device (float32, contiguous, [n, 8]: the bits of mi_proximity_query) is queried in place: returns one float32
        tensor [n, 12] of mi_proximity_reading records (with world_points=True a tuple with the [n, 4] world points), enqueued on the
        world's stream with no synchronisation.  (The tensor is recorded on that stream, as in raycast: release it before close().)"""
        flags = (PROX_STATIC if static else 0) | (PROX_BRUTE_FORCE if brute_force else 0) | (PROX_COUNT if count else 0) | (PROX_TERRAIN if terrain else 0)

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(flags), C.c_void_p(d_out), C.c_void_p(d_aux))
        if _is_tensor(points):
            return self._query_in_place("proximity", entry(self.lib.mi_proximity), points, 8, 12, 4 if world_points else 0)
        if isinstance(points, np.ndarray) and points.dtype == PROXIMITY_QUERY_DTYPE:
            rec = np.ascontiguousarray(points).reshape(-1)
        else:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            rec = np.zeros(len(pts), PROXIMITY_QUERY_DTYPE)
            rec["point"], rec["radius"], rec["enabled"] = pts, np.asarray(radius, np.float32), 1
            _fill_mount(rec, mount, exclude_first, exclude_count)
        out, wp = np.zeros(len(rec), PROXIMITY_READING_DTYPE), np.zeros((len(rec), 4), np.float32)
        self._query_numpy(entry(self.lib.mi_proximity if device else self.lib.mi_proximity_host), rec, out, wp if world_points else None, device)
        return (out, wp) if world_points else out

    def sphere_cast(self, origins, directions=None, radius=0.0, max_t=np.inf, mount=None, exclude_first=None, exclude_count=None, static=True, brute_force=False,
                    world_casts=False, device=False, terrain=False):
        """mi_sphere_cast_batch: per query how far a sphere of `radius` travels from origins[i] along directions[i] (t in units of the
        direction's length, at most max_t) before it touches a collider, and where and on what (the rule is in include/mi_physics.h).
        terrain: the heightmap's triangles are candidates too, as a two-sided sheet (SPHERE_TERRAIN; nothing changes without a heightmap):
        such a hit has collider TERRAIN_COLLIDER, body STATIC_BODY, the touched point and the normal from it to the sphere's centre, and
        no triangle id (proximity(terrain=True) at origin + t * direction names the triangle).  origins, directions [n, 3] in the frame of body mount[i] at its current pose (mount: an index or an
        array [n]; None / STATIC_BODY: world space); radius, max_t: numbers or arrays [n]; blind to the colliders of the bodies
        exclude_first[i] ... + exclude_count[i] - 1.  `origins` may also be a SPHERE_CAST_DTYPE array (the other query arguments are then
        not used).
        numpy queries return a SPHERE_HIT_DTYPE array [n] (hit = 1, or 2 for a cast that used up its iterations; all zero for a miss), with
        world_casts=True a tuple with the world casts [n, 8] = origin, maxT, direction, radius: through the world's staging buffers
        (mi_sphere_cast_host), or with device=True through device tensors of the caller's (mi_sphere_cast_batch).
        A torch tensor on the device (float32, contiguous, [n, 12]: the bits of mi_sphere_cast) is cast in place: returns one float32
        tensor [n, 12] of mi_sphere_hit records (with world_casts=True a tuple with the [n, 8] world casts), enqueued on the world's
        stream with no synchronisation.  (The tensor is recorded on that stream, as in raycast: release it before close().)"""
        flags = (SPHERE_STATIC if static else 0) | (SPHERE_BRUTE_FORCE if brute_force else 0) | (SPHERE_TERRAIN if terrain else 0)

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(flags), C.c_void_p(d_out), C.c_void_p(d_aux))
        if _is_tensor(origins):
            return self._query_in_place("sphere_cast", entry(self.lib.mi_sphere_cast_batch), origins, 12, 12, 8 if world_casts else 0)
        if isinstance(origins, np.ndarray) and origins.dtype == SPHERE_CAST_DTYPE:
            rec = np.ascontiguousarray(origins).reshape(-1)
        else:
            o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
            rec = np.zeros(len(o), SPHERE_CAST_DTYPE)
            rec["origin"], rec["direction"], rec["enabled"] = o, np.ascontiguousarray(directions, np.float32).reshape(-1, 3), 1
            rec["radius"], rec["maxT"] = np.asarray(radius, np.float32), np.asarray(max_t, np.float32)
            _fill_mount(rec, mount, exclude_first, exclude_count)
        out, wc = np.zeros(len(rec), SPHERE_HIT_DTYPE), np.zeros((len(rec), 8), np.float32)
        self._query_numpy(entry(self.lib.mi_sphere_cast_batch if device else self.lib.mi_sphere_cast_host), rec, out, wc if world_casts else None, device)
        return (out, wc) if world_casts else out

    def overlap(self, ctype, shape=None, pos=(0, 0, 0), rot=(0, 0, 0, 1), mount=None, exclude_first=None, exclude_count=None, max_hits=16, static=True,
                brute_force=False, world_shapes=False, device=False):
        """mi_overlap_batch: per volume the colliders it touches right now, "a trigger you ask once": the step's own decision for a trigger
        collider of that shape at that pose: the world boxes meet and the trigger's boolean test answers true (the rule is in
        include/mi_physics.h).  ctype, shape: what add_collider takes (SPHERE ... HULL and up to 10 floats; missing words are zero), one
        volume or arrays [n], [n, k]; pos [n, 3], rot [n, 4]: the volume's pose in the frame of body mount[i] at its current pose (mount:
        an index or an array [n]; None / STATIC_BODY: the world pose, the one a trigger entity has); blind to the colliders of the bodies
        exclude_first[i] ... + exclude_count[i] - 1; static: the colliders of entities without a rigid body are candidates too.
        `ctype` may also be an OVERLAP_QUERY_DTYPE array (the other query arguments are then not used).
        numpy queries return (summary [n] of OVERLAP_SUMMARY_DTYPE, colliders [n, max_hits], bodies [n, max_hits]): numOverlaps counts every
        overlapping candidate, the lists hold the numWritten = min(numOverlaps, max_hits) lowest collider indices, ascending, and zeros
        behind them; with world_shapes=True a fourth array [n, 20] follows: the world record's 10 shape words, the bits of its type, 0, the
        world box min xyz, 0, max xyz, 0.  Through the world's staging buffers (mi_overlap_host), or with device=True through device
        tensors of the caller's (mi_overlap_batch).
        A torch tensor on the device (float32, contiguous, [n, 24]: the bits of mi_overlap_query) is queried in place: returns one float32
        tensor [n, 4 + 2 * max_hits] of raw blocks (view them with .view(torch.int32)), with world_shapes=True a tuple with the [n, 20]
        world shapes; enqueued on the world's stream with no synchronisation.  (The tensor is recorded on that stream, as in raycast:
        release it before close().)"""
        flags = (OVERLAP_STATIC if static else 0) | (OVERLAP_BRUTE_FORCE if brute_force else 0)
        max_hits = int(max_hits)
        if max_hits < 0:
            raise ValueError("overlap: max_hits must not be negative")

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(max_hits), C.c_uint32(flags), C.c_void_p(d_out), C.c_void_p(d_aux))
        if _is_tensor(ctype):
            return self._query_in_place("overlap", entry(self.lib.mi_overlap_batch), ctype, 24, 4 + 2 * max_hits, 20 if world_shapes else 0)
        if isinstance(ctype, np.ndarray) and ctype.dtype == OVERLAP_QUERY_DTYPE:
            rec = np.ascontiguousarray(ctype).reshape(-1)
        else:
            sh = np.atleast_2d(np.asarray(shape, np.float32))
            n = max(len(sh), np.atleast_1d(ctype).size, np.atleast_2d(np.asarray(pos)).shape[0], np.atleast_2d(np.asarray(rot)).shape[0], np.atleast_1d(0 if mount is None else mount).size)
            rec = np.zeros(n, OVERLAP_QUERY_DTYPE)
            rec["shape"][:, :sh.shape[1]] = sh
            rec["type"], rec["enabled"], rec["pos"], rec["rot"] = np.asarray(ctype, np.uint32), 1, np.asarray(pos, np.float32), np.asarray(rot, np.float32)
            _fill_mount(rec, mount, exclude_first, exclude_count)
        n = len(rec)
        out, ws = np.zeros(n, np.dtype([("words", "<u4", (4 + 2 * max_hits,))])), np.zeros((n, 20), np.float32)
        self._query_numpy(entry(self.lib.mi_overlap_batch if device else self.lib.mi_overlap_host), rec, out, ws if world_shapes else None, device)
        words = out["words"].reshape(n, 4 + 2 * max_hits)
        result = (words[:, :4].copy().view(OVERLAP_SUMMARY_DTYPE).reshape(n), words[:, 4::2].copy(), words[:, 5::2].copy())
        return result + (ws,) if world_shapes else result

    def contact_query(self, ctype, shape=None, pos=(0, 0, 0), rot=(0, 0, 0, 1), mount=None, exclude_first=None, exclude_count=None, max_hits=16, static=True,
                      brute_force=False, world_shapes=False, device=False):
        """mi_contact_query_batch: per volume and per collider it touches the manifold the step's narrowphase would build for a collider of
        that shape at that pose, "a collider you ask once" (the rule is in include/mi_physics.h).  The query arguments are overlap()'s.
        numpy queries return (summary [n] of CONTACT_QUERY_SUMMARY_DTYPE, records [n, max_hits] of CONTACT_QUERY_RECORD_DTYPE): numContacts
        counts every contact, the records are the numWritten = min(numContacts, max_hits) lowest collider indices, ascending, zeros behind
        them; the normal points from the volume into the collider; deepestCollider / deepestBody / deepestDepth name the largest |depth| over
        all contacts (STATIC_BODY, STATIC_BODY, 0 without one).  With world_shapes=True a third array [n, 20] follows, as in overlap().
        Through the world's staging buffers (mi_contact_query_host), or with device=True through device tensors of the caller's
        (mi_contact_query_batch).
        A torch tensor on the device (float32, contiguous, [n, 24]: the bits of mi_contact_query) is queried in place: returns one float32
        tensor [n, 8 + 24 * max_hits] of raw blocks, with world_shapes=True a tuple with the [n, 20] world shapes.  The call reads one
        4-byte count back from the device, so it synchronises the world's stream once."""
        flags = (CONTACT_QUERY_STATIC if static else 0) | (CONTACT_QUERY_BRUTE_FORCE if brute_force else 0)
        max_hits = int(max_hits)
        if max_hits < 0:
            raise ValueError("contact_query: max_hits must not be negative")

        def entry(fn):
            return lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_uint32(max_hits), C.c_uint32(flags), C.c_void_p(d_out), C.c_void_p(d_aux))
        if _is_tensor(ctype):
            return self._query_in_place("contact_query", entry(self.lib.mi_contact_query_batch), ctype, 24, 8 + 24 * max_hits, 20 if world_shapes else 0)
        if isinstance(ctype, np.ndarray) and ctype.dtype == CONTACT_QUERY_DTYPE:
            rec = np.ascontiguousarray(ctype).reshape(-1)
        else:
            sh = np.atleast_2d(np.asarray(shape, np.float32))
            n = max(len(sh), np.atleast_1d(ctype).size, np.atleast_2d(np.asarray(pos)).shape[0], np.atleast_2d(np.asarray(rot)).shape[0], np.atleast_1d(0 if mount is None else mount).size)
            rec = np.zeros(n, CONTACT_QUERY_DTYPE)
            rec["shape"][:, :sh.shape[1]] = sh
            rec["type"], rec["enabled"], rec["pos"], rec["rot"] = np.asarray(ctype, np.uint32), 1, np.asarray(pos, np.float32), np.asarray(rot, np.float32)
            _fill_mount(rec, mount, exclude_first, exclude_count)
        n = len(rec)
        out, ws = np.zeros(n, np.dtype([("words", "<u4", (8 + 24 * max_hits,))])), np.zeros((n, 20), np.float32)
        self._query_numpy(entry(self.lib.mi_contact_query_batch if device else self.lib.mi_contact_query_host), rec, out, ws if world_shapes else None, device)
        words = out["words"].reshape(n, 8 + 24 * max_hits)
        result = (words[:, :8].copy().view(CONTACT_QUERY_SUMMARY_DTYPE).reshape(n), words[:, 8:].copy().view(CONTACT_QUERY_RECORD_DTYPE).reshape(n, max_hits))
        return result + (ws,) if world_shapes else result

    def contact_sensors(self, sensors, device=False):
        """mi_contact_sensors: per sensor the impulses the contacts of the last internal step applied to its body, summed on the device
        (the rule is in include/mi_physics.h).  sensors: a CONTACT_SENSOR_DTYPE array or a uint32 array [n, 4] = body, partners
        (CONTACT_DYNAMIC | CONTACT_STATIC), excludeFirst, excludeCount.  Returns a CONTACT_READING_DTYPE array [n]: through the world's
        staging buffers (mi_contact_sensors_host), or with device=True through device tensors of the caller's (mi_contact_sensors)."""
        if isinstance(sensors, np.ndarray) and sensors.dtype == CONTACT_SENSOR_DTYPE:
            rec = np.ascontiguousarray(sensors).reshape(-1)
        else:
            rec = np.ascontiguousarray(sensors, np.uint32).reshape(-1, 4).view(CONTACT_SENSOR_DTYPE).reshape(-1)
        fn = self.lib.mi_contact_sensors if device else self.lib.mi_contact_sensors_host
        out = np.zeros(len(rec), CONTACT_READING_DTYPE)
        self._query_numpy(lambda n, d_in, d_out, d_aux: fn(self.w, C.c_uint32(n), C.c_void_p(d_in), C.c_void_p(d_out)), rec, out, None, device)
        return out

    def accumulators(self):
        """Force and torque accumulators of every body [n, 6]: the pushes the next step will apply and clear."""
        out = np.zeros((self.num_bodies, 6), np.float32)
        self._check(self.lib.mi_debug_read_accumulators(self.w, _p(out), C.c_uint32(len(out))))
        return out

    def apply_force_torque(self, body, force, torque=(0, 0, 0)):
        self._check(self.lib.mi_apply_force_torque(self.w, body, _f(force), _f(torque)))

    def set_transform(self, body, pos, rot=(0, 0, 0, 1)):
        """mi_set_transform: one body's pose (physics_transform0 / 1 and the interpolated one alike)."""
        self._check(self.lib.mi_set_transform(self.w, C.c_uint32(body), _f(pos), _f(rot)))

    def set_velocity(self, body, lin, ang=(0, 0, 0)):
        self._check(self.lib.mi_set_velocity(self.w, body, _f(lin), _f(ang)))

    def write_state(self, transforms, velocities):
        """Bulk overwrite of physics_transform1 ([n,7]) and velocities ([n,6])."""
        t = np.ascontiguousarray(transforms, np.float32); v = np.ascontiguousarray(velocities, np.float32)
        self._check(self.lib.mi_write_transforms(self.w, _p(t), C.c_uint32(len(t))))
        self._check(self.lib.mi_write_velocities(self.w, _p(v), C.c_uint32(len(v))))

    # ---- stepping -------------------------------------------------------------------------------------------
    def step(self, dt, settings=None):
        """physicsStep(scene, arena, timer, settings, dt) — reference physics.h:405."""
        settings = settings or Settings()
        self._check(self.lib.mi_step(self.w, C.byref(self.timer), C.byref(settings), C.c_float(dt)))

    def step_internal(self, dt, iterations=30):
        """One physicsStepInternal (reference physics.cpp:1180-1362) at exactly dt."""
        self._check(self.lib.mi_step_internal(self.w, C.c_float(dt), C.c_uint32(iterations)))

    def synchronize(self):
        self._check(self.lib.mi_synchronize(self.w))

    def enable_stage_timing(self, on=True):
        self._check(self.lib.mi_enable_stage_timing(self.w, int(on)))

    # ---- results --------------------------------------------------------------------------------------------
    @property
    def num_bodies(self):
        return self.lib.mi_num_bodies(self.w)

    @property
    def num_colliders(self):
        return self.lib.mi_num_colliders(self.w)

    def transforms(self, which=1):
        out = np.zeros((self.num_bodies, 7), np.float32)
        self._check(self.lib.mi_read_transforms(self.w, C.c_uint32(which), _p(out), C.c_uint32(len(out))))
        return out

    def velocities(self):
        out = np.zeros((self.num_bodies, 6), np.float32)
        self._check(self.lib.mi_read_velocities(self.w, _p(out), C.c_uint32(len(out))))
        return out

    def mass_properties(self):
        out = np.zeros((self.num_bodies, 13), np.float32)
        self._check(self.lib.mi_read_mass_properties(self.w, _p(out), C.c_uint32(len(out))))
        return out

    def enable_validation(self, on=True):
        """Debug guard: NaN / Inf scan after every stage (the reference's VALIDATE macros, physics.cpp:807-926); a step after one that
        produced a non-finite value fails."""
        self._check(self.lib.mi_enable_validation(self.w, int(on)))

    # ---- spatial slab halo (device side) -------------------------------------------------------------------
    def slab_configure(self, rank, size, axis, lo, hi, margin):
        self._check(self.lib.mi_slab_configure(self.w, C.c_uint32(rank), C.c_uint32(size), C.c_uint32(axis), C.c_float(lo), C.c_float(hi), C.c_float(margin)))

    def slab_message_bytes(self, capacity):
        return int(self.lib.mi_slab_message_bytes(C.c_uint32(capacity)))

    def slab_pack(self, left_ptr, right_ptr, capacity):
        """left_ptr / right_ptr: device addresses (int) of message buffers, or 0 for a missing neighbour."""
        self._check(self.lib.mi_slab_pack(self.w, C.c_void_p(left_ptr or None), C.c_void_p(right_ptr or None), C.c_uint32(capacity)))

    def slab_unpack(self, left_ptr, right_ptr, capacity):
        self._check(self.lib.mi_slab_unpack(self.w, C.c_void_p(left_ptr or None), C.c_void_p(right_ptr or None), C.c_uint32(capacity)))

    def slab_codes(self):
        out = np.zeros(self.num_bodies, np.uint8)
        self._check(self.lib.mi_slab_read_codes(self.w, _p(out), C.c_uint32(len(out))))
        return out

    def stats(self):
        s = Stats()
        self._check(self.lib.mi_get_stats(self.w, C.byref(s)))
        return s.asdict()

    def device_pointers(self):
        pose, vel, stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mi_device_pointers(self.w, C.byref(pose), C.byref(vel), C.byref(stream)))
        return pose.value, vel.value, stream.value

    def state_to_device_buffers(self, pose_ptr, vel_ptr):
        self._check(self.lib.mi_state_to_device_buffers(self.w, C.c_void_p(pose_ptr), C.c_void_p(vel_ptr)))

    def state_from_device_buffers(self, pose_ptr, vel_ptr, mask_ptr):
        self._check(self.lib.mi_state_from_device_buffers(self.w, C.c_void_p(pose_ptr), C.c_void_p(vel_ptr), C.c_void_p(mask_ptr)))

    # ---- inspection of the last internal step (parity tests) -------------------------------------------------------
    def pairs(self):
        out = np.zeros((self.lib.mi_debug_num_pairs(self.w), 2), np.uint32)
        if len(out):
            self._check(self.lib.mi_debug_read_pairs(self.w, _p(out)))
        return out

    def sorting_axis(self):
        """(axis the last step oriented its equal-type pairs by, axis of the next step): the reference's sap_context::sortingAxis."""
        out = np.zeros(2, np.uint32)
        self._check(self.lib.mi_debug_sorting_axis(self.w, _p(out)))
        return int(out[0]), int(out[1])

    def narrow_limits(self):
        """High-water marks of the GJK / EPA caps (narrow_gjk.h: GJK_MAX_ITERATIONS, k_narrow_gjk.hip: EPA_MAX_*) since the world was created, with the
        number of EPA runs that stopped at an out-of-memory exit; same keys as the oracle's stats()."""
        out = np.zeros(8, np.uint32)
        self._check(self.lib.mi_debug_narrow_limits(self.w, _p(out)))
        return dict(gjk_max_iters=int(out[0]), epa_max_triangles=int(out[1]), epa_max_edges=int(out[2]), epa_max_border=int(out[3]), epa_out_of_memory=int(out[4]))

    def color_tasks(self):
        """Task colouring of the last step that ran the cluster sweep: tasks the narrow and the wide instance of k_cl_color coloured, tasks
        too large for the narrow one, and the narrow launch's shape (workgroups, most items of a task it takes, workgroups resident per
        compute unit).  Dispatch only: no result depends on which instance coloured a task."""
        out = np.zeros(8, np.uint32)
        self._check(self.lib.mi_debug_color_tasks(self.w, _p(out)))
        return dict(narrow=int(out[0]), wide=int(out[1]), oversize=int(out[2]), narrow_blocks=int(out[3]), narrow_max=int(out[4]), resident=int(out[5]))

    def task_items(self):
        """Items (manifolds + joints) of every task the last cluster build laid out: one array per phase."""
        items, tasks = np.zeros(5 * 512, np.uint32), np.zeros(8, np.uint32)
        self._check(self.lib.mi_debug_task_items(self.w, _p(items), _p(tasks)))
        return [items[p * 512:p * 512 + int(tasks[p])].copy() for p in range(5)]

    def world_colliders(self):
        n = self.num_colliders
        cols = np.zeros(n, COLLIDER_DTYPE); aabbs = np.zeros((n, 6), np.float32)
        self._check(self.lib.mi_debug_read_world_colliders(self.w, _p(cols), _p(aabbs)))
        return cols, aabbs

    def manifolds(self):
        """(ordered collider pairs [n,2], counts [n], contacts [n,4] CONTACT_DTYPE, body pairs [n,2]) per candidate pair slot."""
        n = self.lib.mi_debug_num_manifold_slots(self.w)
        pairs = np.zeros((n, 2), np.uint32); counts = np.zeros(n, np.uint32); contacts = np.zeros((n, 4), CONTACT_DTYPE); bp = np.zeros((n, 2), np.uint32)
        if n:
            self._check(self.lib.mi_debug_read_manifolds(self.w, _p(pairs), _p(counts), _p(contacts), _p(bp)))
        return pairs, counts, contacts, bp

    def schedule(self):
        """(manifold slots in Gauss-Seidel execution order, colour start offsets [66])."""
        cs = np.zeros(66, np.uint32)
        n = self.lib.mi_debug_num_manifold_slots(self.w)
        slots = np.zeros(max(n, 1), np.uint32)
        self._check(self.lib.mi_debug_read_schedule(self.w, _p(slots), _p(cs)))
        return slots[:int(cs[65])], cs

    def contact_impulses(self):
        """Accumulated (normal, tangent) impulses of the last step's contacts [positions, 4, 2], by position in schedule()'s order."""
        n = len(self.schedule()[0])
        out = np.zeros((max(n, 1), 4, 2), np.float32)
        self._check(self.lib.mi_debug_read_contact_impulses(self.w, _p(out)))
        return out[:n]

    def contact_rows(self):
        """The direction vectors of the last step's contact rows [positions, 4, 15], by position in schedule()'s order and contact:
        t, rA x t, rB x t, rA x n, rB x n (mi_debug_read_contact_rows)."""
        n = len(self.schedule()[0])
        out = np.zeros((max(n, 1), 4, 15), np.float32)
        self._check(self.lib.mi_debug_read_contact_rows(self.w, _p(out)))
        return out[:n]

    def joint_order(self, ctype, n):
        out = np.zeros(max(n, 1), np.uint32)
        self._check(self.lib.mi_debug_read_joint_order(self.w, ctype, _p(out)))
        return out[:n]

    def joint_update(self, ctype, n):
        """(update records [n, JOINT_UPDATE_FLOATS[ctype]] of the last step in joint order, raw float32 with the flag words as bits;
        JOINT_PATH_* of that step).  The record layouts are the comments of csrc/k_joints.hip."""
        out = np.zeros((max(n, 1), JOINT_UPDATE_FLOATS[ctype]), np.float32); path = C.c_uint32(0)
        self._check(self.lib.mi_debug_read_joint_update(self.w, ctype, _p(out), C.c_uint32(n * JOINT_UPDATE_FLOATS[ctype]), C.byref(path)))
        return out[:n], int(path.value)

    def flow_trace(self, enable=True, num_slots=0):
        out = np.zeros((max(1, num_slots), 32), np.uint64)
        self._check(self.lib.mi_debug_flow_trace(self.w, int(enable), _p(out) if num_slots else None, C.c_uint32(num_slots)))
        return out

    def set_replay(self, on=True):
        """Solve contacts in the REFERENCE's own order from now on (its greedy 8-wide batch schedule, batch after batch): parity facility."""
        self._check(self.lib.mi_debug_set_replay(self.w, int(on)))

    def replay_batches(self):
        """The last step's batches [numBatches, 8]: schedule position | contact << 28, 0xFFFFFFFF = empty lane."""
        self.lib.mi_debug_num_replay_batches.restype = C.c_uint32
        n = int(self.lib.mi_debug_num_replay_batches(self.w))
        out = np.zeros((max(n, 1), 8), np.uint32)
        self._check(self.lib.mi_debug_read_replay_batches(self.w, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:n]

    def body_state(self):
        n = self.num_bodies + 1
        cog = np.zeros((n, 4), np.float32); inv = np.zeros((n, 12), np.float32)
        self._check(self.lib.mi_debug_read_body_state(self.w, _p(cog), _p(inv), C.c_uint32(n)))
        return cog, inv


class _BorrowedWorld(World):
    """A World over a handle someone else owns (the batched environments' world): closing it does not destroy the world."""

    def __init__(self, handle):
        self.lib = load_library()
        self.w = C.c_void_p(handle)
        self.timer = C.c_float(0.0)

    def close(self):
        self.w = None


POLICY_NAMES = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
                "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias")
VALUE_NAMES = ("mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
               "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias")
_locomotion_lib = None
_policy_hidden = 0  # H of the policy the library holds (it holds one, for the single environment and the batch)
_value_hidden = 0   # Hv of the critic it holds


def _load_locomotion():
    global _locomotion_lib
    if _locomotion_lib is None:
        build_locomotion()
        lib = C.CDLL(LOCOMOTION_LIB_PATH)
        lib.setPhysicsSeed.argtypes = [C.c_ulonglong]
        lib.getPhysicsBatchWorld.restype = C.c_void_p
        lib.getPhysicsBatchStream.restype = C.c_void_p
        lib.getPhysicsBatchNoiseCounter.restype = C.c_ulonglong
        lib.samplePhysicsNoise.argtypes = [C.c_ulonglong, C.c_uint32, C.c_ulonglong, C.c_void_p]
        lib.samplePhysicsBatchNoiseDevice.argtypes = [C.c_ulonglong, C.c_uint32, C.c_void_p]
        lib.gaePhysicsBatchDevice.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 6
        lib.beginPhysicsBatchTraining.argtypes = [C.c_float] * 4
        lib.updatePhysicsBatchPPODevice.argtypes = [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_float] * 4 + [C.c_int, C.c_void_p]
        lib.gradientsPhysicsBatchPPODevice.argtypes = [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p] + [C.c_float] * 3 + [C.c_int] + [C.c_void_p] * 3
        _locomotion_lib = lib
    return _locomotion_lib


def _policy_arrays(args, names=POLICY_NAMES, outputs=27):
    """The six arrays W1 [H, 66], b1 [H], W2 [H, H], b2 [H], W3 [27, H], b3 [27] as contiguous float32, shapes checked; `args` is the
    six of them, or one mapping with the stable-baselines names (POLICY_NAMES) whose values are arrays or tensors.  With VALUE_NAMES
    and outputs=1: the critic's."""
    if len(args) == 1 and hasattr(args[0], "keys"):
        args = [args[0][k] for k in names]
    if len(args) != 6:
        raise ValueError("a network is six arrays: w1, b1, w2, b2, w3, b3")
    arrays = [np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32) for a in args]
    h = arrays[1].size
    shapes = [(h, 66), (h,), (h, h), (h,), (outputs, h), (outputs,)]
    for a, shape in zip(arrays, shapes):
        if a.shape != shape:
            raise ValueError("network array of shape %s where %s is expected" % (a.shape, shape))
    return h, arrays


def set_policy(*args):
    """setPhysicsPolicy: the 66 -> H -> H -> 27 tanh network of the learned controller, for the single environment and the batch."""
    global _policy_hidden
    h, arrays = _policy_arrays(args)
    code = _load_locomotion().setPhysicsPolicy(C.c_uint32(h), *[_p(a) for a in arrays])
    if code:
        raise PhysicsError("setPhysicsPolicy failed (%d)" % code)
    _policy_hidden = h


def infer_policy(state, hidden=False):
    """inferPhysicsPolicy: the network on one state [66], on the host.  Returns the action [27], with hidden also (tanh(z1), tanh(z2))."""
    state = np.ascontiguousarray(state, np.float32).reshape(66)
    action = np.zeros(27, np.float32)
    ab = np.zeros(2 * max(_policy_hidden, 1), np.float32)
    code = _load_locomotion().inferPhysicsPolicy(_p(state), _p(action), _p(ab) if hidden else None)
    if code:
        raise PhysicsError("inferPhysicsPolicy failed (%d)" % code)
    return (action, ab[:_policy_hidden], ab[_policy_hidden:]) if hidden else action


def set_value_network(*args):
    """setPhysicsValueNetwork: the critic 66 -> Hv -> Hv -> 1 (tanh) of training: six arrays w1 [Hv, 66], b1, w2 [Hv, Hv], b2, w3 [1, Hv],
    b3 [1], or one mapping with the stable-baselines names (VALUE_NAMES)."""
    global _value_hidden
    h, arrays = _policy_arrays(args, VALUE_NAMES, 1)
    code = _load_locomotion().setPhysicsValueNetwork(C.c_uint32(h), *[_p(a) for a in arrays])
    if code:
        raise PhysicsError("setPhysicsValueNetwork failed (%d)" % code)
    _value_hidden = h


def infer_value(state, hidden=False):
    """inferPhysicsValue: the critic on one state [66], on the host.  Returns the value, with hidden also (tanh(z1), tanh(z2))."""
    state = np.ascontiguousarray(state, np.float32).reshape(66)
    value = np.zeros(1, np.float32)
    ab = np.zeros(2 * max(_value_hidden, 1), np.float32)
    code = _load_locomotion().inferPhysicsValue(_p(state), _p(value), _p(ab) if hidden else None)
    if code:
        raise PhysicsError("inferPhysicsValue failed (%d)" % code)
    return (value[0], ab[:_value_hidden], ab[_value_hidden:]) if hidden else value[0]


def set_log_std(log_std):
    """setPhysicsActionStd: the Gaussian's per-action log-scale [27] (a scalar is broadcast); the library receives it together with
    std = float32(exp(float64(log_std))) and evaluates neither."""
    if hasattr(log_std, "detach"):
        log_std = log_std.detach().cpu().numpy()
    log_std = np.ascontiguousarray(np.broadcast_to(np.asarray(log_std, np.float32), (27,)))
    std = np.exp(log_std.astype(np.float64)).astype(np.float32)
    code = _load_locomotion().setPhysicsActionStd(_p(std), _p(log_std))
    if code:
        raise PhysicsError("setPhysicsActionStd failed (%d)" % code)


def sample_noise(seed, env, update):
    """samplePhysicsNoise: the exploration noise [27] of environment `env` at update counter `update` under `seed`, on the host."""
    out = np.zeros(27, np.float32)
    code = _load_locomotion().samplePhysicsNoise(C.c_ulonglong(seed), C.c_uint32(env), C.c_ulonglong(update), _p(out))
    if code:
        raise PhysicsError("samplePhysicsNoise failed (%d)" % code)
    return out


def update_policy():
    """updatePhysicsPolicy: one closed-loop update of the single environment.  Returns (state [66], reward, fallen)."""
    state = np.zeros(66, np.float32); reward = C.c_float(0.0)
    code = _load_locomotion().updatePhysicsPolicy(_p(state), C.byref(reward))
    if code < 0:
        raise PhysicsError("updatePhysicsPolicy failed (%d)" % code)
    return state, reward.value, bool(code)


def _network_floats(hidden, outputs):
    return hidden * 66 + hidden + hidden * hidden + hidden + outputs * hidden + outputs


def _split_flat(flat, hidden, value_hidden):
    """A tensor in the flat parameter order of host/locomotion_update.h (the device's [in][out] layouts: actor, critic, log_std) as a
    dict under the stable-baselines names, weights transposed back to [out, in]."""
    out, at = {}, 0
    for names, h, outputs in ((POLICY_NAMES, hidden, 27), (VALUE_NAMES, value_hidden, 1)):
        for name, (inputs, units) in zip(names[0::2], ((66, h), (h, h), (h, outputs))):
            out[name] = flat[at:at + inputs * units].reshape(inputs, units).t().contiguous(); at += inputs * units
            out[name.replace("weight", "bias")] = flat[at:at + units].clone(); at += units
    out["log_std"] = flat[at:at + 27].clone()
    assert at + 27 == flat.numel()
    return out


class LocomotionBatch:
    """N ragdoll environments of libmi_locomotion.so stepped together in one world (host/locomotion_batch.hip).  One instance per
    process: the library holds one batch, as it holds one single environment.  step() takes a [n, 27] numpy array, or a ROCm torch
    tensor, which goes to updatePhysicsBatchDevice on the world's stream and returns device tensors.  For the tensor path, import
    torch before the first World or LocomotionBatch: the process then runs one HIP runtime, the one torch loads."""

    def __init__(self, n, seed=None):
        lib = _load_locomotion()
        self.lib, self.n = lib, int(n)
        self.state_size, self.action_size = lib.getPhysicsStateSize(), lib.getPhysicsActionSize()
        if seed is not None:
            lib.setPhysicsSeed(C.c_ulonglong(seed))
        self.reset()

    def _check(self, code, what, count=False):
        """Status codes are 0 or an MI_ERR_*; a count (updatePhysicsBatch) is >= 0 or a negated MI_ERR_*."""
        if code < 0 or (code and not count):
            raise PhysicsError("%s failed (%d)" % (what, code))
        return code

    def reset(self):
        """Builds the world and resets every environment; returns the states [n, 66]."""
        states = np.zeros((self.n, self.state_size), np.float32)
        self._check(self.lib.resetPhysicsBatch(C.c_uint32(self.n), _p(states)), "resetPhysicsBatch")
        return states

    def step(self, actions):
        """(states [n, 66], rewards [n], fallen [n] int32) after one update with `actions` [n, 27]."""
        if hasattr(actions, "is_cuda") and actions.is_cuda:
            return self._step_device(actions)
        a = np.ascontiguousarray(actions, np.float32).reshape(self.n, self.action_size)
        states = np.zeros((self.n, self.state_size), np.float32); rewards = np.zeros(self.n, np.float32); fallen = np.zeros(self.n, np.int32)
        self._check(self.lib.updatePhysicsBatch(_p(a), _p(states), _p(rewards), _p(fallen)), "updatePhysicsBatch", count=True)
        return states, rewards, fallen

    def _step_device(self, actions):
        import torch
        a = actions.detach().to(torch.float32).contiguous().reshape(self.n, self.action_size)
        dev = a.device
        states = torch.empty((self.n, self.state_size), dtype=torch.float32, device=dev)
        rewards = torch.empty(self.n, dtype=torch.float32, device=dev); fallen = torch.empty(self.n, dtype=torch.int32, device=dev)
        code = self._on_stream(dev, (a, states, rewards, fallen), lambda: self.lib.updatePhysicsBatchDevice(
            C.c_void_p(a.data_ptr()), C.c_void_p(states.data_ptr()), C.c_void_p(rewards.data_ptr()), C.c_void_p(fallen.data_ptr())))
        self._check(code, "updatePhysicsBatchDevice")
        return states, rewards, fallen

    def _on_stream(self, dev, tensors, call):
        """Runs `call` (which enqueues on the world's stream) between the two stream hand-overs of the tensor path."""
        import torch
        ext = torch.cuda.ExternalStream(self.lib.getPhysicsBatchStream(), device=dev)
        ext.wait_stream(torch.cuda.current_stream(dev))      # the inputs are ready
        with torch.cuda.stream(ext):
            code = call()
            for t in tensors:
                t.record_stream(ext)
        torch.cuda.current_stream(dev).wait_stream(ext)      # the outputs are ready for the caller's stream
        return code

    # ---- the learned controller (host/locomotion_policy.h, k_loco_policy) ----
    def set_policy(self, *args):
        """The controller's network: six arrays w1 [H, 66], b1, w2 [H, H], b2, w3 [27, H], b3, or one mapping with the stable-baselines
        names (POLICY_NAMES).  Replaces the previous one; the library keeps it across reset()."""
        set_policy(*args)

    @property
    def hidden(self):
        return _policy_hidden

    def act(self, states, hidden=False):
        """The network on `states` [count, 66], any count, on the device, touching no environment: numpy in, numpy out; ROCm tensor in,
        tensors out.  Returns the raw actions [count, 27]; with hidden=True (actions, a [count, H], b [count, H]), the two tanh vectors."""
        import torch
        if not self.hidden:
            raise PhysicsError("act: no policy set")
        on_device = hasattr(states, "is_cuda") and states.is_cuda
        s = states.detach() if on_device else torch.from_numpy(np.ascontiguousarray(states, np.float32)).cuda()
        s = s.to(torch.float32).contiguous().reshape(-1, self.state_size)
        count, dev = s.shape[0], s.device
        actions = torch.empty((count, self.action_size), dtype=torch.float32, device=dev)
        ab = torch.empty((count, 2 * self.hidden), dtype=torch.float32, device=dev) if hidden else None
        code = self._on_stream(dev, [t for t in (s, actions, ab) if t is not None], lambda: self.lib.inferPhysicsBatchDevice(
            C.c_uint32(count), C.c_void_p(s.data_ptr()), C.c_void_p(actions.data_ptr()), C.c_void_p(ab.data_ptr()) if hidden else None))
        self._check(code, "inferPhysicsBatchDevice")
        out = (actions, ab[:, :self.hidden], ab[:, self.hidden:]) if hidden else (actions,)
        if not on_device:
            torch.cuda.synchronize(dev)
            out = tuple(t.cpu().numpy() for t in out)
        return out if hidden else out[0]

    # ---- training data (k_loco_sample, k_loco_policy<1, false>, k_loco_gae) ----
    def set_value_network(self, *args):
        """The critic: six arrays w1 [Hv, 66], b1, w2 [Hv, Hv], b2, w3 [1, Hv], b3 [1], or one mapping with the stable-baselines names
        (VALUE_NAMES).  Hv is independent of the policy's H; the library keeps it across reset()."""
        set_value_network(*args)

    def set_log_std(self, log_std):
        """The log of the per-action scale of the Gaussian that collect() samples from ([27], or a scalar)."""
        set_log_std(log_std)

    @property
    def value_hidden(self):
        return _value_hidden

    @property
    def noise_counter(self):
        """Collecting updates since reset(): the update counter the next collect() starts at."""
        return int(self.lib.getPhysicsBatchNoiseCounter())

    def _device(self):
        import torch
        return torch.device("cuda", torch.cuda.current_device())

    def values(self, states, hidden=False):
        """The critic on `states` [count, 66], like act(): numpy in, numpy out; ROCm tensor in, tensors out.  Returns the values [count];
        with hidden=True (values, a [count, Hv], b [count, Hv])."""
        import torch
        if not self.value_hidden:
            raise PhysicsError("values: no value network set")
        on_device = hasattr(states, "is_cuda") and states.is_cuda
        s = states.detach() if on_device else torch.from_numpy(np.ascontiguousarray(states, np.float32)).cuda()
        s = s.to(torch.float32).contiguous().reshape(-1, self.state_size)
        count, dev, hv = s.shape[0], s.device, self.value_hidden
        values = torch.empty(count, dtype=torch.float32, device=dev)
        ab = torch.empty((count, 2 * hv), dtype=torch.float32, device=dev) if hidden else None
        code = self._on_stream(dev, [t for t in (s, values, ab) if t is not None], lambda: self.lib.inferPhysicsBatchValueDevice(
            C.c_uint32(count), C.c_void_p(s.data_ptr()), C.c_void_p(values.data_ptr()), C.c_void_p(ab.data_ptr()) if hidden else None))
        self._check(code, "inferPhysicsBatchValueDevice")
        out = (values, ab[:, :hv], ab[:, hv:]) if hidden else (values,)
        if not on_device:
            torch.cuda.synchronize(dev)
            out = tuple(t.cpu().numpy() for t in out)
        return out if hidden else out[0]

    def noise(self, first_update, num_updates):
        """The exploration noise of update counters first_update .. first_update + num_updates - 1 as a ROCm tensor [num_updates, n, 27]:
        what collect() draws there.  A function of (seed, environment, counter, action index) alone; moves no state."""
        import torch
        dev = self._device()
        eps = torch.empty((num_updates, self.n, self.action_size), dtype=torch.float32, device=dev)
        code = self._on_stream(dev, (eps,), lambda: self.lib.samplePhysicsBatchNoiseDevice(C.c_ulonglong(first_update), C.c_uint32(num_updates), C.c_void_p(eps.data_ptr())))
        self._check(code, "samplePhysicsBatchNoiseDevice")
        return eps

    def collect(self, steps, clip=True):
        """`steps` closed-loop updates with actions sampled around the policy's output, enqueued back to back with the device-side reset
        of the fallen.  Returns a dict of ROCm tensors; row t: obs [steps, n, 66] the states the networks saw (after a fall the reset
        state), actions [steps, n, 27] = mu + std * eps (unclipped), eps, log_probs [steps, n], values [steps, n] = V(obs), rewards and
        dones (int32) after the update; last_values [n] = V of the states after the last update.  With clip the environment receives the
        action clamped to the action ranges, as stable-baselines clips to the environment's Box."""
        import torch
        dev = self._device()
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        out = dict(obs=new(steps, self.n, self.state_size), actions=new(steps, self.n, self.action_size), eps=new(steps, self.n, self.action_size),
                   log_probs=new(steps, self.n), values=new(steps, self.n), rewards=new(steps, self.n), dones=new(steps, self.n, dtype=torch.int32),
                   last_values=new(self.n))
        code = self._on_stream(dev, tuple(out.values()), lambda: self.lib.collectPhysicsBatchDevice(
            C.c_uint32(steps), C.c_int(1 if clip else 0), *[C.c_void_p(t.data_ptr()) for t in out.values()]))
        self._check(code, "collectPhysicsBatchDevice")
        return out

    def gae(self, rewards, values, dones, last_values, gamma=0.99, lam=0.95):
        """Generalised advantage estimation on [steps, n] ROCm tensors (dones int32), on the device.  Returns (advantages, returns).
        Episodes end by falling only: a done row bootstraps nothing."""
        import torch
        r = rewards.detach().to(torch.float32).contiguous(); v = values.detach().to(torch.float32).contiguous()
        d = dones.detach().to(torch.int32).contiguous(); last = last_values.detach().to(torch.float32).contiguous()
        steps, n = r.shape
        assert v.shape == d.shape == (steps, n) and last.shape == (n,)
        advantages = torch.empty_like(r); returns = torch.empty_like(r)
        code = self._on_stream(r.device, (r, v, d, last, advantages, returns), lambda: self.lib.gaePhysicsBatchDevice(
            C.c_uint32(steps), C.c_uint32(n), C.c_float(gamma), C.c_float(lam), *[C.c_void_p(t.data_ptr()) for t in (r, v, d, last, advantages, returns)]))
        self._check(code, "gaePhysicsBatchDevice")
        return advantages, returns

    # ---- the gradient step (host/locomotion_update.hip) ----
    def begin_training(self, lr=2.5e-5, betas=(0.9, 0.999), eps=1e-5):
        """Opens a training session: torch.optim.Adam(lr, betas, eps) with zeroed moments over the networks and log_std as they are on the
        device.  From here on the device holds the master copy of the parameters (parameters() reads it); set_policy, set_value_network,
        set_log_std and reset() end the session."""
        self._check(self.lib.beginPhysicsBatchTraining(lr, betas[0], betas[1], eps), "beginPhysicsBatchTraining")

    def end_training(self):
        """Drops the optimiser state; the parameters stay as they are on the device."""
        self._check(self.lib.endPhysicsBatchTraining(), "endPhysicsBatchTraining")

    def _rows(self, obs, actions, old_log_probs, advantages, returns):
        import torch
        t = [x.detach().to(torch.float32).contiguous() for x in (obs, actions, old_log_probs, advantages, returns)]
        rows = t[2].numel()
        t = [t[0].reshape(rows, self.state_size), t[1].reshape(rows, self.action_size)] + [x.reshape(rows) for x in t[2:]]
        if not all(x.is_cuda for x in t):
            raise ValueError("the rows of the gradient step are ROCm tensors")
        return rows, t

    def _indices(self, order, rows):
        """Row indices as an int32 ROCm tensor; a host tensor or array is checked against `rows` before it is uploaded."""
        import torch
        order = order if hasattr(order, "is_cuda") else torch.as_tensor(np.asarray(order))
        if not order.is_cuda and order.numel() and (int(order.min()) < 0 or int(order.max()) >= rows):
            raise ValueError("row index outside [0, %d)" % rows)
        return order.to(device=self._device(), dtype=torch.int32).contiguous()

    def ppo_update(self, obs, actions, old_log_probs, advantages, returns, order, batch_size=128, clip_range=0.1, vf_coef=0.5, ent_coef=0.0,
                   max_grad_norm=0.5, normalize_advantage=True):
        """PPO's epochs on the device, enqueued without a host synchronisation: `order` [epochs, rows] holds one permutation of the rows per
        epoch, each cut into minibatches of batch_size (the last one short); every minibatch is one optimiser step (training.ppo_loss,
        clip_grad_norm_, Adam) on the device's parameters.  Returns a ROCm tensor [epochs * minibatches, 5]: per step loss, policy loss,
        value loss, clip fraction and the gradient's norm before clipping."""
        import torch
        rows, t = self._rows(obs, actions, old_log_probs, advantages, returns)
        order = self._indices(order, rows).reshape(-1, rows)
        epochs = order.shape[0]
        stats = torch.empty((epochs * ((rows + batch_size - 1) // batch_size), 5), dtype=torch.float32, device=order.device)
        code = self._on_stream(order.device, t + [order, stats], lambda: self.lib.updatePhysicsBatchPPODevice(
            rows, *[x.data_ptr() for x in t], epochs, order.data_ptr(), batch_size, clip_range, vf_coef, ent_coef, max_grad_norm, 1 if normalize_advantage else 0, stats.data_ptr()))
        self._check(code, "updatePhysicsBatchPPODevice")
        return stats

    def ppo_gradients(self, obs, actions, old_log_probs, advantages, returns, indices=None, clip_range=0.1, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True):
        """The unclipped gradient of training.ppo_loss on one minibatch (the rows `indices`, all rows if None) with the parameters as they
        are, moving nothing.  Returns (gradients, ratios [count], stats [4]): gradients under the names of parameters(), in their shapes;
        stats = loss, policy loss, value loss, clip fraction."""
        import torch
        rows, t = self._rows(obs, actions, old_log_probs, advantages, returns)
        idx = None if indices is None else self._indices(indices, rows).reshape(-1)
        count, dev = rows if idx is None else idx.numel(), t[0].device
        h, hv = self.hidden, self.value_hidden
        flat = torch.empty(_network_floats(h, 27) + _network_floats(hv, 1) + 27, dtype=torch.float32, device=dev)
        ratios = torch.empty(count, dtype=torch.float32, device=dev); stats = torch.empty(4, dtype=torch.float32, device=dev)
        code = self._on_stream(dev, t + [flat, ratios, stats] + ([] if idx is None else [idx]), lambda: self.lib.gradientsPhysicsBatchPPODevice(
            rows, *[x.data_ptr() for x in t], count, None if idx is None else idx.data_ptr(), clip_range, vf_coef, ent_coef, 1 if normalize_advantage else 0,
            flat.data_ptr(), ratios.data_ptr(), stats.data_ptr()))
        self._check(code, "gradientsPhysicsBatchPPODevice")
        return _split_flat(flat, h, hv), ratios, stats

    def parameters(self):
        """The parameters as they are on the device now, as float32 numpy arrays under the stable-baselines names of
        training.ActorCritic.state_dict(): POLICY_NAMES, VALUE_NAMES and "log_std", in the [out, in] shapes set_policy takes."""
        h, hv = self.hidden, self.value_hidden
        out = {}
        for names, hidden, outputs, call in ((POLICY_NAMES, h, 27, self.lib.readPhysicsBatchPolicy), (VALUE_NAMES, hv, 1, self.lib.readPhysicsBatchValueNetwork)):
            arrays = [np.zeros(shape, np.float32) for shape in ((hidden, 66), (hidden,), (hidden, hidden), (hidden,), (outputs, hidden), (outputs,))]
            self._check(call(*[_p(a) for a in arrays]), "readPhysicsBatch network")
            out.update(zip(names, arrays))
        out["log_std"] = np.zeros(27, np.float32)
        self._check(self.lib.readPhysicsBatchLogStd(None, _p(out["log_std"])), "readPhysicsBatchLogStd")
        return out

    def step_policy(self, device=False):
        """One closed-loop update: the policy on the current states, smoothing, motors, push, step.  Returns (states, rewards, fallen) as
        numpy arrays; with device=True ROCm tensors (states, rewards, fallen, actions), actions being the raw network outputs, enqueued
        without a host synchronisation."""
        if not device:
            states = np.zeros((self.n, self.state_size), np.float32); rewards = np.zeros(self.n, np.float32); fallen = np.zeros(self.n, np.int32)
            self._check(self.lib.updatePhysicsBatchPolicy(_p(states), _p(rewards), _p(fallen)), "updatePhysicsBatchPolicy", count=True)
            return states, rewards, fallen
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        states = torch.empty((self.n, self.state_size), dtype=torch.float32, device=dev); actions = torch.empty((self.n, self.action_size), dtype=torch.float32, device=dev)
        rewards = torch.empty(self.n, dtype=torch.float32, device=dev); fallen = torch.empty(self.n, dtype=torch.int32, device=dev)
        code = self._on_stream(dev, (states, rewards, fallen, actions), lambda: self.lib.updatePhysicsBatchPolicyDevice(
            C.c_void_p(states.data_ptr()), C.c_void_p(rewards.data_ptr()), C.c_void_p(fallen.data_ptr()), C.c_void_p(actions.data_ptr())))
        self._check(code, "updatePhysicsBatchPolicyDevice")
        return states, rewards, fallen, actions

    def rollout(self, steps, auto_reset=True):
        """`steps` closed-loop updates enqueued back to back on the device.  Returns ROCm tensors (states [steps, n, 66], actions
        [steps, n, 27], rewards [steps, n], fallen [steps, n] int32): row t holds the raw action taken at update t and the state, reward
        and fallen after it.  With auto_reset every environment that has fallen after an update is reset on the device before the next
        (its row keeps the terminal state; its random stream goes on)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        states = torch.empty((steps, self.n, self.state_size), dtype=torch.float32, device=dev); actions = torch.empty((steps, self.n, self.action_size), dtype=torch.float32, device=dev)
        rewards = torch.empty((steps, self.n), dtype=torch.float32, device=dev); fallen = torch.empty((steps, self.n), dtype=torch.int32, device=dev)
        code = self._on_stream(dev, (states, actions, rewards, fallen), lambda: self.lib.rolloutPhysicsBatchDevice(
            C.c_uint32(steps), C.c_int(1 if auto_reset else 0), C.c_void_p(states.data_ptr()), C.c_void_p(actions.data_ptr()), C.c_void_p(rewards.data_ptr()), C.c_void_p(fallen.data_ptr())))
        self._check(code, "rolloutPhysicsBatchDevice")
        return states, actions, rewards, fallen

    def reset_envs(self, ids, states=None):
        """Resets the listed environments; writes their rows of `states` ([n, 66], a new zero array if None) and returns it."""
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        states = np.zeros((self.n, self.state_size), np.float32) if states is None else states
        assert states.dtype == np.float32 and states.shape == (self.n, self.state_size) and states.flags.c_contiguous
        self._check(self.lib.resetPhysicsBatchEnvs(_p(ids), C.c_uint32(len(ids)), _p(states)), "resetPhysicsBatchEnvs")
        return states

    def observe(self):
        """(states, rewards, fallen) of the environments as they are, without stepping."""
        states = np.zeros((self.n, self.state_size), np.float32); rewards = np.zeros(self.n, np.float32); fallen = np.zeros(self.n, np.int32)
        self._check(self.lib.observePhysicsBatch(_p(states), _p(rewards), _p(fallen)), "observePhysicsBatch")
        return states, rewards, fallen

    def pushes(self):
        """The pushes of the last update: 1 + the pushed body per environment, or 0."""
        out = np.zeros(self.n, np.int32)
        if self.lib.getPhysicsBatchPushes(_p(out)) < 0:
            raise PhysicsError("getPhysicsBatchPushes failed")
        return out

    @property
    def world(self):
        """The batch's world as a World (not owned: closing it leaves the world alive)."""
        return _BorrowedWorld(self.lib.getPhysicsBatchWorld())
