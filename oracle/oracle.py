"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes front-end to oracle/liboracle.so (strict fp32 restatement of the reference's src/physics path) and
oracle/liboracle_avx2.so (same sources, -O3 -mavx2 -mfma: the single-thread cpu_baseline).  Only tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the product never does.
The class mirrors the product's `World` (directx-renderer-kurth_amd/__init__.py) so a scene description can be
instantiated into either.  PARITY UNPINNED: the reference ships no tests or golden vectors.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
STATIC = 0xFFFFFFFF

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
DISTANCE, BALL, FIXED, HINGE, CONE_TWIST, SLIDER = range(6)
SOLVER_SCALAR, SOLVER_WIDE8, SOLVER_CUSTOM, SOLVER_REPLAY = 0, 1, 2, 3  # REPLAY: the reference's batch order (scheduleConstraintsSIMD) with the device's row-form arithmetic

COLLIDER_DTYPE = np.dtype([("shape", "<f4", 10), ("restitution", "<f4"), ("friction", "<f4"), ("density", "<f4"),
                           ("type", "<u4"), ("objectType", "<u4"), ("objectIndex", "<u4")])
CONTACT_DTYPE = np.dtype([("point", "<f4", 3), ("depth", "<f4"), ("normal", "<f4", 3), ("friction_restitution", "<u4")])
RB_GLOBAL_DTYPE = np.dtype([("rotation", "<f4", 4), ("localCOG", "<f4", 3), ("position", "<f4", 3), ("invInertia", "<f4", 9),
                            ("invMass", "<f4"), ("v", "<f4", 3), ("w", "<f4", 3)])
# trigger_event / collision_begin_event / collision_end_event as one record (same layout as mi_event, include/mi_physics.h)
EVENT_DTYPE = np.dtype([("kind", "<u4"), ("step", "<u4"), ("a", "<u4"), ("b", "<u4"), ("bodyA", "<u4"), ("bodyB", "<u4"),
                        ("position", "<f4", 3), ("normal", "<f4", 3), ("relativeVelocity", "<f4", 3)])
TRIGGER_ENTER, TRIGGER_LEAVE, COLLISION_BEGIN, COLLISION_END = range(4)
assert EVENT_DTYPE.itemsize == 60
assert COLLIDER_DTYPE.itemsize == 64 and CONTACT_DTYPE.itemsize == 32 and RB_GLOBAL_DTYPE.itemsize == 104


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


def build(force=False):
    """Compile the oracle with its committed Makefile (gcc only).  make is a no-op when the libraries are newer than their sources; on a
    box without the sources' build tools the prebuilt libraries are used as they are."""
    if force:
        subprocess.check_call(["make", "-C", _HERE, "clean"], stdout=subprocess.DEVNULL)
    have = os.path.exists(os.path.join(_HERE, "liboracle.so")) and os.path.exists(os.path.join(_HERE, "liboracle_avx2.so"))
    try:
        subprocess.check_call(["make", "-C", _HERE, "-j2"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL if have else None)
    except (OSError, subprocess.CalledProcessError):
        if not have:
            raise


_libs = {}


def _lib(avx2=False):
    key = "avx2" if avx2 else "strict"
    if key not in _libs:
        build()
        lib = C.CDLL(os.path.join(_HERE, "liboracle_avx2.so" if avx2 else "liboracle.so"))
        lib.orc_world_create.restype = C.c_void_p
        for name in ("orc_add_body", "orc_add_collider", "orc_add_static_collider", "orc_add_distance_constraint_local",
                     "orc_add_distance_constraint_global", "orc_add_ball_constraint_local", "orc_add_ball_constraint_global",
                     "orc_add_fixed_constraint_global", "orc_add_hinge_constraint_global", "orc_add_cone_twist_constraint_global",
                     "orc_add_slider_constraint_global", "orc_num_bodies", "orc_num_colliders", "orc_num_pairs", "orc_num_contacts",
                     "orc_num_collisions", "orc_sorting_axis_used", "orc_sorting_axis_next", "orc_num_contact_slots",
                     "orc_narrowphase_ordered", "orc_schedule", "orc_read_slot_counts", "orc_add_hull_geometry", "orc_test_physics_interaction",
                     "orc_terrain_slot_mismatch", "orc_read_contact_impulses", "orc_terrain_contacts", "orc_add_cloth", "orc_cloth_num_particles", "orc_cloth_num_constraints", "orc_add_force_field", "orc_add_trigger", "orc_add_force_field_collider", "orc_add_trigger_collider", "orc_drain_events"):
            getattr(lib, name).restype = C.c_uint32
        lib.orc_heightmap_height_at.restype = C.c_float
        lib.orc_poly_trig.restype = C.c_float
        lib.orc_last_interaction_distance.restype = C.c_float
        _libs[key] = lib
    return _libs[key]


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleWorld:
    def __init__(self, avx2=False, solver=SOLVER_SCALAR):
        self.lib = _lib(avx2)
        self.w = C.c_void_p(self.lib.orc_world_create())
        self.solver = solver
        self.timer = C.c_float(0.0)

    def __del__(self):
        if getattr(self, "w", None):
            self.lib.orc_world_destroy(self.w)
            self.w = None

    # ---- add API (reference physics.h:110-157, 209-235; rigid_body.h:21) -------------------------------
    def add_body(self, pos, rot=(0, 0, 0, 1), kinematic=False, gravity_factor=1.0, linear_damping=0.4, angular_damping=0.4):
        return self.lib.orc_add_body(self.w, int(kinematic), C.c_float(gravity_factor), C.c_float(linear_damping), C.c_float(angular_damping), _f(pos), _f(rot))

    def add_hull_geometry(self, vertices, triangles):
        """bounding_hull_geometry::fromMesh: convex vertex set + triangle list; returns the geometry index used by HULL colliders."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3); t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        return self.lib.orc_add_hull_geometry(self.w, _f(v), C.c_uint32(len(v)), t.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(len(t)))

    def use_hull_geometries(self):
        """Stage-level functions (narrowphase_ordered) read hull vertices from this world's geometry table from now on."""
        self.lib.orc_use_hull_geometries(self.w)

    def add_collider(self, body, ctype, shape, material):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self.lib.orc_add_collider(self.w, C.c_uint32(body), C.c_uint32(ctype), _f(s), _f(material))

    def add_static_collider(self, ctype, shape, material, pos=(0, 0, 0), rot=(0, 0, 0, 1)):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self.lib.orc_add_static_collider(self.w, C.c_uint32(ctype), _f(s), _f(material), _f(pos), _f(rot))

    # ---- force fields, triggers, events (physics.h:182-203, 356-380; physics.cpp:759-787, 952-1178) ----
    def add_force_field(self, force, pos=None, rot=None):
        """A field without colliders acts on every body; with colliders, on the bodies overlapping them."""
        return self.lib.orc_add_force_field(self.w, _f(force), _f(pos) if pos is not None else None, _f(rot) if rot is not None else None)

    def set_force_field(self, field, force):
        return self.lib.orc_set_force_field(self.w, C.c_uint32(field), _f(force))

    def add_trigger(self, pos=None, rot=None):
        return self.lib.orc_add_trigger(self.w, _f(pos) if pos is not None else None, _f(rot) if rot is not None else None)

    def add_force_field_collider(self, field, ctype, shape):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self.lib.orc_add_force_field_collider(self.w, C.c_uint32(field), C.c_uint32(ctype), _f(s))

    def add_trigger_collider(self, trigger, ctype, shape):
        s = np.zeros(10, np.float32); s[:len(shape)] = shape
        return self.lib.orc_add_trigger_collider(self.w, C.c_uint32(trigger), C.c_uint32(ctype), _f(s))

    def set_force_field_transform(self, field, pos, rot=(0, 0, 0, 1)):
        assert self.lib.orc_set_force_field_transform(self.w, C.c_uint32(field), _f(pos), _f(rot)) == 0

    def set_trigger_transform(self, trigger, pos, rot=(0, 0, 0, 1)):
        assert self.lib.orc_set_trigger_transform(self.w, C.c_uint32(trigger), _f(pos), _f(rot)) == 0

    def enable_collision_events(self, begin=True, end=True):
        self.lib.orc_enable_collision_events(self.w, int(begin), int(end))

    def zone_pair_stats(self):
        """(tested[6,6], hit[6,6]): overlap checks by (typeA, typeB) since the world was created."""
        t = np.zeros(36, np.uint32); h = np.zeros(36, np.uint32)
        self.lib.orc_zone_pair_stats(self.w, _p(t), _p(h))
        return t.reshape(6, 6), h.reshape(6, 6)

    def drain_events(self, capacity=1 << 16):
        out = np.zeros(capacity, EVENT_DTYPE)
        n = self.lib.orc_drain_events(self.w, _p(out), C.c_uint32(capacity))
        return out[:n]

    # ---- heightmap terrain (heightmap_collider.h:127-152) ----
    def set_heightmap(self, chunks_per_dim, chunk_size, material, min_corner, amplitude_scale):
        self.lib.orc_set_heightmap(self.w, C.c_uint32(chunks_per_dim), C.c_float(chunk_size), _f(material), _f(min_corner), C.c_float(amplitude_scale))

    def heightmap_set_chunk(self, x, z, heights):
        h = np.ascontiguousarray(heights, np.uint16).reshape(129, 129)
        assert self.lib.orc_heightmap_set_chunk(self.w, C.c_uint32(x), C.c_uint32(z), _p(h)) == 0

    def heightmap_update(self, min_corner, amplitude_scale):
        self.lib.orc_heightmap_update(self.w, _f(min_corner), C.c_float(amplitude_scale))

    def heightmap_height_at(self, x, z):
        return float(self.lib.orc_heightmap_height_at(self.w, C.c_float(x), C.c_float(z)))

    def terrain_contacts(self, collider, capacity=256):
        """Terrain contacts of one collider at the poses of the last step, device emission order: rows {point3, depth, normal3, isLowestPoint}."""
        out = np.zeros((capacity, 8), np.float32)
        n = self.lib.orc_terrain_contacts(self.w, C.c_uint32(collider), _p(out), C.c_uint32(capacity))
        return out[:min(n, capacity)]

    def terrain_slot_mismatch(self):
        """Follow mode: number of colliders whose terrain contact count differs from the slots the device reported (0 = same contact set)."""
        return self.lib.orc_terrain_slot_mismatch(self.w)

    # ---- cloth (cloth.h:5-60; stepped after the rigid bodies, physics.cpp:1354-1358) ----
    def add_cloth(self, width, height, grid_x, grid_y, total_mass, stiffness=0.5, damping=0.3, gravity_factor=1.0):
        return self.lib.orc_add_cloth(self.w, C.c_float(width), C.c_float(height), C.c_uint32(grid_x), C.c_uint32(grid_y), C.c_float(total_mass),
                                      C.c_float(stiffness), C.c_float(damping), C.c_float(gravity_factor))

    def cloth_set_fixed_vertices(self, cloth, pos, rot=(0, 0, 0, 1), move_rigid=False):
        assert self.lib.orc_cloth_set_fixed_vertices(self.w, C.c_uint32(cloth), _f(pos), _f(rot), int(move_rigid)) == 0

    def cloth_set_properties(self, cloth, total_mass, stiffness, damping, gravity_factor):
        assert self.lib.orc_cloth_set_properties(self.w, C.c_uint32(cloth), C.c_float(total_mass), C.c_float(stiffness), C.c_float(damping), C.c_float(gravity_factor)) == 0

    def set_cloth_iterations(self, velocity=0, position=1, drift=0):
        self.lib.orc_set_cloth_iterations(self.w, C.c_uint32(velocity), C.c_uint32(position), C.c_uint32(drift))

    def set_cloth_colour_order(self, on=True):
        """Gauss-Seidel order of the cloth constraints: the reference's storage order (False) or the device's colour order (True)."""
        self.lib.orc_set_cloth_colour_order(self.w, int(on))

    def cloth_state(self, cloth):
        n = self.lib.orc_cloth_num_particles(self.w, C.c_uint32(cloth))
        p = np.zeros((n, 3), np.float32); v = np.zeros((n, 3), np.float32)
        assert self.lib.orc_cloth_read(self.w, C.c_uint32(cloth), _p(p), _p(v)) == 0
        return p, v

    def cloth_constraints(self, cloth):
        n = self.lib.orc_cloth_num_constraints(self.w, C.c_uint32(cloth))
        c = np.zeros(n, np.dtype([("a", "<u4"), ("b", "<u4"), ("restDistance", "<f4"), ("inverseMassSum", "<f4")])); col = np.zeros(n, np.uint32)
        self.lib.orc_cloth_read_constraints(self.w, C.c_uint32(cloth), _p(c), _p(col))
        return c, col

    def add_distance_constraint_local(self, a, b, la, lb, distance):
        return self.lib.orc_add_distance_constraint_local(self.w, a, b, _f(la), _f(lb), C.c_float(distance))

    def add_distance_constraint_global(self, a, b, ga, gb):
        return self.lib.orc_add_distance_constraint_global(self.w, a, b, _f(ga), _f(gb))

    def add_ball_constraint_local(self, a, b, la, lb):
        return self.lib.orc_add_ball_constraint_local(self.w, a, b, _f(la), _f(lb))

    def add_ball_constraint_global(self, a, b, g):
        return self.lib.orc_add_ball_constraint_global(self.w, a, b, _f(g))

    def add_fixed_constraint_global(self, a, b, g):
        return self.lib.orc_add_fixed_constraint_global(self.w, a, b, _f(g))

    def add_hinge_constraint_global(self, a, b, anchor, axis, min_limit=1.0, max_limit=-1.0):
        return self.lib.orc_add_hinge_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(min_limit), C.c_float(max_limit))

    def add_cone_twist_constraint_global(self, a, b, anchor, axis, swing_limit, twist_limit):
        return self.lib.orc_add_cone_twist_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(swing_limit), C.c_float(twist_limit))

    def add_slider_constraint_global(self, a, b, anchor, axis, min_limit=1.0, max_limit=-1.0):
        return self.lib.orc_add_slider_constraint_global(self.w, a, b, _f(anchor), _f(axis), C.c_float(min_limit), C.c_float(max_limit))

    def constraint_get(self, ctype, cid, nbytes):
        buf = np.zeros(nbytes, np.uint8)
        assert self.lib.orc_constraint_get(self.w, ctype, cid, _p(buf)) == 0
        return buf

    def constraint_set(self, ctype, cid, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        assert self.lib.orc_constraint_set(self.w, ctype, cid, _p(buf)) == 0

    def delete_body(self, body):
        assert self.lib.orc_delete_body(self.w, C.c_uint32(body)) == 0

    def test_physics_interaction(self, origin, direction, strength=1000.0):
        r = self.lib.orc_test_physics_interaction(self.w, _f(origin), _f(direction), C.c_float(strength))
        return r - 1 if r > 0 else None

    def last_interaction_distance(self):
        """The distance t of the closest hit of this world's last test_physics_interaction (the push does not depend on it)."""
        return float(self.lib.orc_last_interaction_distance(self.w))

    def accumulators(self):
        """forceAccumulator, torqueAccumulator of every body [n, 6]: what the next step will apply and clear."""
        out = np.zeros((self.num_bodies, 6), np.float32)
        self.lib.orc_read_accumulators(self.w, _p(out))
        return out

    def apply_force_torque(self, body, force, torque=(0, 0, 0)):
        assert self.lib.orc_apply_force_torque(self.w, body, _f(force), _f(torque)) == 0

    def set_velocity(self, body, lin, ang=(0, 0, 0)):
        assert self.lib.orc_set_velocity(self.w, body, _f(lin), _f(ang)) == 0

    def write_state(self, transforms, velocities, presort=True):
        t = np.ascontiguousarray(transforms, np.float32); v = np.ascontiguousarray(velocities, np.float32)
        self.lib.orc_write_state(self.w, _p(t), _p(v), C.c_uint32(len(t)))
        if presort:
            self.lib.orc_presort_endpoints(self.w)

    # ---- stepping ---------------------------------------------------------------------------------------
    def step(self, dt, settings=None):
        """physicsStep(scene, arena, timer, settings, dt) — reference physics.h:405."""
        settings = settings or Settings()
        self.lib.orc_step(self.w, C.byref(self.timer), C.byref(settings), C.c_uint32(self.solver), C.c_float(dt))

    def step_internal(self, dt, iterations=30):
        """One physicsStepInternal (reference physics.cpp:1180)."""
        self.lib.orc_step_internal(self.w, C.c_uint32(iterations), C.c_uint32(self.solver), C.c_float(dt))

    def set_follow(self, ordered_pairs, slot_order):
        """Follow a device run: narrowphase on its ordered candidate pairs, contacts solved manifold by manifold in slot_order."""
        pairs = np.ascontiguousarray(ordered_pairs, np.uint32).reshape(-1, 2)
        order = np.ascontiguousarray(slot_order, np.uint32)
        self._follow_keep = (pairs, order)
        self.lib.orc_set_follow(self.w, _p(pairs), C.c_uint32(len(pairs)), _p(order), C.c_uint32(len(order)))

    def set_row_form(self, on=True):
        """Custom-order and replay-order contact solves in the device's row form (default) or with the reference formula."""
        self.lib.orc_set_row_form(self.w, int(on))

    def set_scalar_row_form(self, on=True):
        """SOLVER_SCALAR (the reference's emission order) with the row-form arithmetic instead of the reference formula: lets a test
        measure the distance between the two on one order.  Off by default, and not touched by set_row_form."""
        self.lib.orc_set_scalar_row_form(self.w, int(on))

    def set_wide_rsqrt(self, on=True):
        """The 8-lane solver's noz with the host's rsqrtss estimate (the reference's AVX2 semantics) instead of exact 1/sqrt.  Process-wide."""
        self.lib.orc_set_wide_rsqrt(int(on))

    def set_wide_joint_math(self, on=True):
        """Joint initialisation (hinge / cone-twist limit and motor angles) with the reference's wide math — polynomial cos / sin /
        atan2 / acos (core/simd.h:28-49, 122-164), rsqrt-based normalisation, wide rotateFromTo / getAxisRotation — instead of the
        scalar path's libm calls: the "AVX2 semantics" of constraints.cpp:1309-1777, 2072-2634.  Process-wide."""
        self.lib.orc_set_wide_joint_math(int(on))

    def poly_trig(self, which, a, b=0.0):
        """The reference's polynomial cos (0) / sin (1) / atan2(a, b) (2) / acos (3) for one float."""
        self.lib.orc_poly_trig.restype = C.c_float
        return float(self.lib.orc_poly_trig(int(which), C.c_float(a), C.c_float(b)))

    def stage_seconds(self, reset=True):
        """Cumulative wall time per stage since the last reset: colliders + broadphase, narrowphase, forces + constraint setup, solve, integration."""
        out = np.zeros(5, np.float64)
        self.lib.orc_stage_seconds(self.w, _p(out), int(reset))
        return out

    def clear_follow(self):
        self.lib.orc_clear_follow(self.w)

    JOINT_DECISION_FLOATS = 24

    def joint_decisions(self, ctype, n):
        """What the joints of one type decided and accumulated in the last step, [n, 24] in storage order (= constraint ids): flags,
        limit signs, motor target velocities, impulses and bounds, the angles and the swing rotation (layout: oworld.cpp, at the fill)."""
        out = np.zeros((max(n, 1), self.JOINT_DECISION_FLOATS), np.float32)
        self.lib.orc_read_joint_decisions.restype = C.c_uint32
        got = self.lib.orc_read_joint_decisions(self.w, C.c_uint32(ctype), _p(out), C.c_uint32(n * self.JOINT_DECISION_FLOATS))
        assert got == n, (got, n)
        return out[:n]

    def set_joint_order(self, ctype, order):
        order = np.ascontiguousarray(order, np.uint32)
        self.lib.orc_set_joint_order(self.w, C.c_uint32(ctype), _p(order), C.c_uint32(len(order)))

    def slot_counts(self):
        out = np.zeros(max(1, len(getattr(self, "_follow_keep", (np.zeros((0, 2)),))[0])), np.uint8)
        n = self.lib.orc_read_slot_counts(self.w, _p(out))
        return out[:n]

    def set_custom_order(self, order):
        order = np.ascontiguousarray(order, np.uint32)
        self.lib.orc_set_custom_order(self.w, _p(order), C.c_uint32(len(order)))

    # ---- read-back --------------------------------------------------------------------------------------
    @property
    def num_bodies(self):
        return self.lib.orc_num_bodies(self.w)

    @property
    def num_colliders(self):
        return self.lib.orc_num_colliders(self.w)

    def transforms(self, which=1):
        out = np.zeros((self.num_bodies, 7), np.float32)
        self.lib.orc_read_transforms(self.w, C.c_uint32(which), _p(out))
        return out

    def velocities(self):
        out = np.zeros((self.num_bodies, 6), np.float32)
        self.lib.orc_read_velocities(self.w, _p(out))
        return out

    def mass_properties(self):
        out = np.zeros((self.num_bodies, 13), np.float32)
        self.lib.orc_read_mass_properties(self.w, _p(out))
        return out

    def world_colliders(self):
        n = self.num_colliders
        cols = np.zeros(n, COLLIDER_DTYPE); aabbs = np.zeros((n, 6), np.float32)
        self.lib.orc_read_world_colliders(self.w, _p(cols), _p(aabbs))
        return cols, aabbs

    def pairs(self):
        out = np.zeros((self.lib.orc_num_pairs(self.w), 2), np.uint32)
        self.lib.orc_read_pairs(self.w, _p(out))
        return out

    def contacts(self):
        n = self.lib.orc_num_contacts(self.w)
        c = np.zeros(n, CONTACT_DTYPE); bp = np.zeros((n, 2), np.uint32); ci = np.zeros(n, np.uint32)
        self.lib.orc_read_contacts(self.w, _p(c), _p(bp), _p(ci))
        return c, bp, ci

    def contact_impulses(self):
        """(normal, tangent) impulses the last step accumulated [numContacts, 2], parallel to contacts() (scalar, follow and replay solvers)."""
        out = np.zeros((max(1, self.lib.orc_num_contacts(self.w)), 2), np.float32)
        n = self.lib.orc_read_contact_impulses(self.w, _p(out))
        return out[:n]

    def collisions(self):
        n = self.lib.orc_num_collisions(self.w)
        pairs = np.zeros((n, 2), np.uint32); counts = np.zeros(n, np.uint8)
        self.lib.orc_read_collisions(self.w, _p(pairs), _p(counts))
        return pairs, counts

    def rb_global(self, pre_solve=False):
        out = np.zeros(self.num_bodies + 1, RB_GLOBAL_DTYPE)
        self.lib.orc_read_rb_global(self.w, C.c_uint32(1 if pre_solve else 0), _p(out))
        return out

    def contact_slots(self):
        out = np.zeros((self.lib.orc_num_contact_slots(self.w), 8), np.uint32)
        self.lib.orc_read_contact_slots(self.w, _p(out))
        return out

    def sorting_axis(self):
        return self.lib.orc_sorting_axis_used(self.w), self.lib.orc_sorting_axis_next(self.w)

    def set_wide_broadphase(self, on=True):
        """physics_settings::simdBroadPhase: the 8-wide sweep (collision_broad.cpp:168-295) instead of the scalar one; same pair list."""
        self.lib.orc_set_wide_broadphase(self.w, int(on))

    def set_sim_mask(self, simulate):
        """Per body: non-zero = simulated in this world; the others' colliders take no part and their state is frozen (a spatial slab)."""
        m = np.ascontiguousarray(simulate, np.uint8)
        self.lib.orc_set_sim_mask(self.w, m.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(len(m)))

    def set_sorting_axis(self, axis):
        """sap_context::sortingAxis of the next broadphase (a world taking over another world's state mid-run)."""
        self.lib.orc_set_sorting_axis(self.w, C.c_uint32(int(axis)))

    def sorting_variance(self):
        """Variance of the last broadphase's AABB centres per axis (float, summed collider after collider as the reference does)."""
        out = np.zeros(3, np.float32)
        self.lib.orc_sorting_variance(self.w, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out


# ---- stage-level functions ---------------------------------------------------------------------------------
def narrowphase_ordered(colliders, pairs):
    """Contacts for ORDERED collider pairs (A,B as given).  Returns (contacts, counts_per_pair)."""
    lib = _lib()
    colliders = np.ascontiguousarray(colliders, COLLIDER_DTYPE)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    out = np.zeros(4 * len(pairs), CONTACT_DTYPE); counts = np.zeros(len(pairs), np.uint8)
    n = lib.orc_narrowphase_ordered(_p(colliders), _p(pairs), C.c_uint32(len(pairs)), _p(out), _p(counts))
    return out[:n], counts


def overlap_ordered(colliders, pairs):
    """Boolean overlapCheck (collision_narrow.cpp:1593-1689) for ORDERED collider pairs (typeA <= typeB).  Returns one flag per pair."""
    lib = _lib()
    colliders = np.ascontiguousarray(colliders, COLLIDER_DTYPE)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    out = np.zeros(len(pairs), np.uint8)
    lib.orc_overlap_ordered(_p(colliders), _p(pairs), C.c_uint32(len(pairs)), _p(out))
    return out.astype(bool)


def schedule(body_pairs, dummy):
    lib = _lib()
    bp = np.ascontiguousarray(body_pairs, np.uint32).reshape(-1, 2)
    out = np.zeros((len(bp) + 8, 8), np.uint32)
    n = lib.orc_schedule(_p(bp), C.c_uint32(len(bp)), C.c_uint32(dummy), _p(out))
    return out[:n]


def solve_contacts(rb_global, contacts, body_pairs, order, iterations, dt):
    """Contact init + GS sweeps in `order` on 104-byte body records.  Returns (rb_global_out, impulses[n,2])."""
    lib = _lib()
    rb = np.array(rb_global, RB_GLOBAL_DTYPE, copy=True)
    contacts = np.ascontiguousarray(contacts, CONTACT_DTYPE)
    bp = np.ascontiguousarray(body_pairs, np.uint32).reshape(-1, 2)
    order = np.ascontiguousarray(order, np.uint32)
    imp = np.zeros((len(contacts), 2), np.float32)
    lib.orc_solve_contacts(_p(rb), C.c_uint32(len(rb)), _p(contacts), _p(bp), C.c_uint32(len(contacts)), _p(order), C.c_uint32(len(order)),
                           C.c_uint32(iterations), C.c_float(dt), _p(imp))
    return rb, imp


def stats():
    """High-water marks of the GJK / EPA caps over every narrowphase since the library was loaded or stats_reset(), and the number
    of EPA runs that stopped at an out-of-memory exit (the device's World.narrow_limits() has the same keys)."""
    out = np.zeros(8, np.uint32)
    _lib().orc_stats(_p(out))
    return dict(gjk_max_iters=int(out[0]), epa_max_triangles=int(out[1]), epa_max_edges=int(out[2]), epa_max_border=int(out[3]), epa_out_of_memory=int(out[4]))


def stats_reset():
    _lib().orc_stats_reset()
