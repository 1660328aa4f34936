"""The cloth step (csrc/k_cloth.hip, the host half in csrc/api_scene.hip) read in float64 from the reference's src/physics/cloth.cpp
(constructor, setWorldPositionOfFixedVertices, applyWindForce, simulate, solveVelocities, solvePositions, recalculateProperties), the
battery the device and the oracle's restatement (oracle/ocloth.h) are held to, and the measured distance of a float32 step from this one.
Plain numpy, no GPU, and nothing taken from ocloth.h: this is the independent side of the comparison.

Construction.  Inputs are rounded to float32 and the initial positions are the float32 values mi_add_cloth produces; rest lengths and
inverse mass sums are float64 functions of those.  Constraints are built in the reference's storage order (per particle, row by row:
stretch right, stretch down, the two shear diagonals of the cell, bend right, bend down).

Colours.  The device solves a colour in parallel, so a colour must not name a particle twice.  The rule, stated here on its own:
    family 0  stretch right   (x, y)-(x+1, y)      colour  0 + (x & 1)
    family 1  stretch down    (x, y)-(x, y+1)      colour  2 + (y & 1)
    family 2  shear down      (x, y)-(x+1, y+1)    colour  4 + (x & 1)
    family 3  shear up        (x, y+1)-(x+1, y)    colour  6 + (x & 1)
    family 4  bend right      (x, y)-(x+2, y)      colour  8 + ((x >> 1) & 1)
    family 5  bend down       (x, y)-(x, y+2)      colour 10 + ((y >> 1) & 1)
A constraint of span s along an axis shares a particle only with the one s further along; x & 1 tells neighbours of span 1 apart and
(x >> 1) & 1 those of span 2 (x and x + 2 differ in bit 1).  Cloth64 asserts the uniqueness per colour on every grid it builds.

The step.  step64 is one cloth_component::simulate (after applyWindForce) from a float32 state, in float64, in colour order (one numpy
scatter per colour) or in the reference's storage order (a sequential loop).  The branches invMass > 0, inverseMassSum > 0,
sqRest + len > 1e-5 and dt > 1e-5 are decided on the float32 values the device would see; dt is the float32 value.

The battery.  battery() crosses the eleven grids with the seven iteration mixes; a world of the GPU tests holds the eleven cloths of one
mix (world_order(): LDS-sized and larger ones, small and large n interleaved).  The iteration mix, the wind and the running dt belong to
the world, so they go with the mix; gravity factor, damping, stiffness and the pose cycle over (grid, mix), so that every grid, hence
both kernel variants, meets every value.  The two dt values at the invDt branch are not given worlds of their own, in which nothing
would ever move: every case takes its first step at the float32 above 1e-5 and its sixth at 1e-5, and the others at its running dt
(step_dt).  The sixth step meets a cloth in motion, and invDt = 1 leaves it nearly at rest.  The step above the branch has to be the
first: there invDt is 1e5, so a position or drift pass turns a stretch of a tenth of a millimetre into 10 m/s, in the reference as
here, and only a cloth still in its construction pose stays below the battery's speed limit.  That first step barely moves anything, so
the tests that compare single steps also take the second, the first at the running dt.

The deviation table.  E_F32 is what one float32 step in colour order (the oracle's) lies from step64 started at the same float32
state, per iteration class, in units (units()):
    positions   eps32 * max(1, max|p|)
    velocities  eps32 * max(1, max|v|), and, once a position or drift pass ran and left v = (p - prev) * invDt,
                eps32 * max(1, max|p|) * invDt if that is larger (invDt is 1 for dt <= 1e-5, so such steps are scaled by |p| alone)
with p, v the float64 result of the step.  The velocity unit carries invDt, so the steps at the two boundary dt values belong to the
class of their mix like any other.  (Scaling the dt <= 1e-5 steps by |p| as well as |v| is this module's choice: there a position or
drift pass leaves v = (p - prev) x 1, whose float32 error is an ulp of p whatever v is; by |v| alone the far-off cloths would set the
figure for all.)
test_cloth64_cpu.py holds the table to its own measurement within 1.5 x either way; the device's tolerance is 4 x the figure."""
import math

import numpy as np

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
GRAVITY = -9.81   # physics.h:11
GRAVITY_F32 = float(np.float32(GRAVITY))

# The last cloth the LDS variant of k_cloth_simulate takes: 64 KiB of LDS over 7 float planes (x, y, z of position and velocity, inverse
# mass) = 65536 // 28.  csrc/k_cloth.hip keeps the figure in cloth_lds_particle_limit(), which is not exported: if that changes, this
# constant and the four grids around it below (2340 = 52 x 45 = 2 x 1170; 2342 = 1171 x 2; 2343 = 33 x 71) move with it.
LDS_PARTICLE_LIMIT = 65536 // 28
CLOTH_BLOCK = 512   # threads of the kernel's one workgroup per cloth: 32 x 16 fills the strided loops' first trip, 27 x 19 starts a second

DT_EDGE = f32(1e-5)                                   # invDt = 1
DT_ABOVE = np.nextafter(DT_EDGE, f32(1), dtype=f32)   # invDt = 1 / dt
assert float(DT_EDGE) <= 1e-5 < float(DT_ABOVE)

# (gridX, gridY, width, height): cells within an aspect ratio of 4
GRIDS = [
    (2, 2, 0.5, 0.4),           # no bend constraints, one colour per family
    (2, 3, 0.4, 0.9),           # one bend colour along y only
    (3, 2, 0.9, 0.4),
    (3, 3, 1.0, 1.2),           # one bend colour per axis
    (4, 5, 1.2, 1.5),
    (32, 16, 3.1, 2.0),         # 512: the block exactly
    (27, 19, 2.6, 2.7),         # 513: one particle in the second trip
    (52, 45, 4.0, 3.0),         # 2340: the LDS limit
    (2, 1170, 0.02, 11.69),     # 2340 as a strip along y (cells 0.02 x 0.01)
    (33, 71, 3.2, 7.0),         # 2343: global planes
    (1171, 2, 11.7, 0.02),      # 2342 as a strip along x
]
assert [gx * gy for gx, gy, _, _ in GRIDS[7:]] == [LDS_PARTICLE_LIMIT, LDS_PARTICLE_LIMIT, LDS_PARTICLE_LIMIT + 3, LDS_PARTICLE_LIMIT + 2]
assert GRIDS[5][0] * GRIDS[5][1] == CLOTH_BLOCK and GRIDS[6][0] * GRIDS[6][1] == CLOTH_BLOCK + 1
STORAGE_ORDER_GRIDS = GRIDS[:7]   # the sequential float64 loop is slow: up to 27 x 19
ORDER_GRIDS = GRIDS[:8]           # colour order against storage order: up to 52 x 45

MIXES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 0, 2), (2, 3, 1), (8, 8, 8)]
WIND_NONE, WIND_IN_PLANE, WIND, WIND_STRONG = None, (2.0, 0.0, 1.0), (3.0, 0.5, 1.5), (30.0, 5.0, 15.0)
# per mix: the world's wind and running dt.  In the worlds with the in-plane wind every cloth keeps its sheet horizontal (a yaw only),
# so that the horizontal wind lies in its initial plane.
WORLD_OF_MIX = [(WIND, 1.0 / 120.0), (WIND_NONE, 1.0 / 30.0), (WIND_STRONG, 1.0 / 120.0), (WIND_IN_PLANE, 1.0 / 30.0),
                (WIND, 1.0 / 30.0), (WIND_STRONG, 1.0 / 120.0), (WIND_NONE, 1.0 / 120.0)]
GRAVITY_FACTORS = [1.0, 0.0, -1.0]
DAMPINGS = [0.3, 0.0, 50.0]
STIFFNESSES = [0.5, 1.0, 0.001, 5.0]   # the last two through cloth_set_properties, which clamps them to 0.01 and 1 (mi_add_cloth does not clamp)
POSITIONS = [(0.0, 3.0, 0.0), (2.5, 1.0, -1.5), (-3.0, 4.0, 2.0), (97.0, 12.0, -64.0), (1.0, -2.0, 3.5), (-1.5, 5.0, -2.5), (4.0, 2.0, 1.0)]   # one far off
_S = math.sqrt(0.5)
ROTATIONS = [(0.0, 0.0, 0.0, 1.0), (-_S, 0.0, 0.0, _S), (0.18257419, 0.36514837, 0.54772256, 0.73029674), (0.0, 0.38268343, 0.0, 0.92387953),
             (-0.5, 0.5, 0.5, 0.5), (0.36514837, -0.18257419, 0.54772256, 0.73029674), (0.25881905, 0.0, 0.0, 0.96592583)]
YAWS = [(0.0, 0.0, 0.0, 1.0), (0.0, 0.38268343, 0.0, 0.92387953), (0.0, -_S, 0.0, _S), (0.0, 0.25881905, 0.0, 0.96592583),
        (0.0, 0.96592583, 0.0, 0.25881905), (0.0, -0.38268343, 0.0, 0.92387953), (0.0, 0.5, 0.0, 0.8660254)]
TOLERANCE = 4.0    # the device may lie this many table figures from step64 / set_fixed64
MAX_SPEED = 50.0   # the battery's condition: the oracle's own trajectory of every case stays finite and below this (test_cloth64_cpu.py)

# max over the battery of |oracle32 - step64| after one step from the same float32 state, in units(): {class: (positions, velocities)}
# (test_cloth64_cpu.py::test_deviation_table measures it and holds this table to the measurement within 1.5 x either way)
E_F32 = {
    "integrate": (0.478, 1.47),
    "velocity": (0.503, 2.5),
    "position": (2.05, 2.04),
    "drift": (1.47, 1.47),
    "mixed": (14.1, 14),
}
# |oracle32 - set_fixed64| right after setWorldPositionOfFixedVertices, in eps32 * max(1, max|p|) (test_cloth64_cpu.py::test_fixed_vertices)
E_F32_FIXED = 0.806
# largest particle distance in metres between the oracle's colour order and its storage order after 120 free steps of mix (2, 3, 1) on
# ORDER_GRIDS (test_cloth64_cpu.py::test_colour_order_against_storage_order)
ORDER_DISTANCE = 0.1606


# ---------------------------------------------------------------------------------------------------------------------------
# The cloth
# ---------------------------------------------------------------------------------------------------------------------------
def particle_position32(width, height, rel_x, rel_y):
    """getParticlePosition in float32"""
    width, height, rel_x, rel_y = f32(width), f32(height), f32(rel_x), f32(rel_y)
    x = f32(f32(rel_x * width) - f32(width * f32(0.5)))
    return np.array([x, f32(0), f32(-rel_y * height)], f32)


class Cloth64:
    def __init__(self, width, height, grid_x, grid_y, total_mass, stiffness=0.5, damping=0.3, gravity_factor=1.0):
        self.width, self.height, self.gx, self.gy = f32(width), f32(height), int(grid_x), int(grid_y)
        self.total_mass, self.stiffness, self.damping, self.gravity_factor = f32(total_mass), f32(stiffness), f32(damping), f32(gravity_factor)
        gx, gy, n = self.gx, self.gy, self.gx * self.gy
        self.n = n
        self.p0 = np.zeros((n, 3), f32)
        self.inv_mass = np.zeros(n, f32)
        per_particle = f32(f32(n) / self.total_mass)
        for y in range(gy):
            for x in range(gx):
                self.p0[y * gx + x] = particle_position32(width, height, f32(x) / f32(gx - 1), f32(y) / f32(gy - 1))
                self.inv_mass[y * gx + x] = f32(0) if y == 0 else per_particle   # the upper row is locked
        a, b, colour = [], [], []
        for y in range(gy):
            for x in range(gx):
                i = y * gx + x
                if x < gx - 1:
                    a.append(i); b.append(i + 1); colour.append(0 + (x & 1))
                if y < gy - 1:
                    a.append(i); b.append(i + gx); colour.append(2 + (y & 1))
                if x < gx - 1 and y < gy - 1:
                    a.append(i); b.append(i + gx + 1); colour.append(4 + (x & 1))
                    a.append(i + gx); b.append(i + 1); colour.append(6 + (x & 1))
                if x < gx - 2:
                    a.append(i); b.append(i + 2); colour.append(8 + ((x >> 1) & 1))
                if y < gy - 2:
                    a.append(i); b.append(i + 2 * gx); colour.append(10 + ((y >> 1) & 1))
        self.a, self.b, self.colour = np.array(a, np.int64), np.array(b, np.int64), np.array(colour, np.int64)
        p0 = self.p0.astype(np.float64)
        self.rest = np.linalg.norm(p0[self.a] - p0[self.b], axis=1)
        self.rest32 = self.rest.astype(f32)
        self.old_total_mass, self.old_stiffness = self.total_mass, self.stiffness
        self._mass_sums()
        self.colours = []   # per colour: constraint indices in storage order
        for c in range(12):
            k = np.nonzero(self.colour == c)[0]
            touched = np.concatenate([self.a[k], self.b[k]])
            assert len(np.unique(touched)) == len(touched), "colour %d of a %d x %d cloth names a particle twice" % (c, gx, gy)
            self.colours.append(k)

    def _mass_sums(self):
        """inverseMassSum = (invMassA + invMassB) / stiffness in float64 from the float32 values; its float32 value decides the branch"""
        s = self.inv_mass[self.a].astype(np.float64) + self.inv_mass[self.b].astype(np.float64)
        self.ims = s / float(self.stiffness)
        self.ims32 = self.ims.astype(f32)

    def set_properties(self, total_mass, stiffness, damping, gravity_factor):
        self.total_mass, self.stiffness, self.damping, self.gravity_factor = f32(total_mass), f32(stiffness), f32(damping), f32(gravity_factor)

    def recalculate_if_changed(self):
        """the head of simulate, and recalculateProperties"""
        if self.total_mass != self.old_total_mass or self.stiffness != self.old_stiffness:
            per_particle = f32(f32(self.n) / self.total_mass)
            self.inv_mass = np.where(self.inv_mass != 0, per_particle, f32(0)).astype(f32)
            self.stiffness = f32(min(max(self.stiffness, f32(0.01)), f32(1.0)))
            self._mass_sums()
            self.old_total_mass, self.old_stiffness = self.total_mass, self.stiffness


# ---------------------------------------------------------------------------------------------------------------------------
# setWorldPositionOfFixedVertices
# ---------------------------------------------------------------------------------------------------------------------------
def _qrot(q, v):
    """quat * vec3 of core/math.h: q * (v, 0) * conjugate(q), rows of v at once"""
    v = np.atleast_2d(v)
    qv, w = q[:3], q[3]
    t = w * v + np.cross(qv, v)              # vector part of q * (v, 0)
    s = -(v @ qv)                            # scalar part
    # (t, s) * (-qv, w)
    return -s[:, None] * qv + w * t - np.cross(t, qv)


def _unit(v):
    return v / np.linalg.norm(v)


def rotate_from_to64(a, b):
    """rotateFromTo of core/math.cpp; M_PI is the float32 constant there"""
    a, b = _unit(a), _unit(b)
    d = float(np.dot(a, b))
    if d >= 1.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    if d < 1e-6 - 1.0:   # a half turn about some axis
        axis = np.cross([1.0, 0.0, 0.0], a)
        if np.dot(axis, axis) == 0.0:
            axis = np.cross([0.0, 1.0, 0.0], a)
        axis = _unit(axis)
        h = float(f32(3.14159265359)) * 0.5
        q = np.array([axis[0] * math.sin(h), axis[1] * math.sin(h), axis[2] * math.sin(h), math.cos(h)])
        return _unit(q)
    s = math.sqrt((1.0 + d) * 2.0)
    c = np.cross(a, b)
    return _unit(np.array([c[0] / s, c[1] / s, c[2] / s, s * 0.5]))


def set_fixed64(cloth, p32, pos, rot, move_rigid):
    """positions after setWorldPositionOfFixedVertices({rot, pos}, move_rigid) from the float32 positions p32, in float64"""
    p = np.asarray(p32, f32).astype(np.float64).copy()
    q, t = np.asarray(rot, f32).astype(np.float64), np.asarray(pos, f32).astype(np.float64)
    gx = cloth.gx
    local = lambda rel_x: particle_position32(cloth.width, cloth.height, rel_x, 0.0).astype(np.float64)
    xform = lambda v: _qrot(q, v)[0] + t
    if move_rigid:
        pivot = p[gx // 2] if gx % 2 == 1 else (p[gx // 2] + p[gx // 2 - 1]) * 0.5
        current_axis = _unit(p[gx - 1] - p[0])
        new_axis = _unit(xform(local(1.0)) - xform(local(0.0)))
        new_pivot = xform(local(0.5))
        delta = rotate_from_to64(current_axis, new_axis)
        p[gx:] = _qrot(delta, p[gx:] - pivot) + new_pivot
    for x in range(gx):
        p[x] = xform(local(f32(x) / f32(gx - 1)))
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# The step
# ---------------------------------------------------------------------------------------------------------------------------
def wind_forces64(cloth, p, wind):
    """applyWindForce: the force accumulators of all particles from positions p [n, 3]"""
    gx, gy = cloth.gx, cloth.gy
    force = np.zeros((cloth.n, 3))
    if wind is None:
        return force
    wind = np.asarray(wind, f32).astype(np.float64)
    g = p.reshape(gy, gx, 3)
    tl, tr, bl, br = g[:-1, :-1], g[:-1, 1:], g[1:, :-1], g[1:, 1:]
    idx = np.arange(cloth.n).reshape(gy, gx)
    itl, itr, ibl, ibr = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()

    def triangle(a, b, c):
        normal = np.cross(b - a, c - a).reshape(-1, 3)
        unit = normal / np.linalg.norm(normal, axis=1)[:, None]
        return normal * (unit @ wind)[:, None] / 3.0
    f1 = triangle(tl, bl, tr)
    f2 = triangle(br, tr, bl)
    for i, f in ((itl, f1), (itr, f1), (ibl, f1), (ibr, f2), (itr, f2), (ibl, f2)):
        np.add.at(force, i, f)
    return force


def _solve_positions_colour(cloth, p, im):
    for k in cloth.colours:
        if not len(k):
            continue
        a, b = cloth.a[k], cloth.b[k]
        delta = p[b] - p[a]
        length = np.einsum("ij,ij->i", delta, delta)
        sq_rest = cloth.rest[k] ** 2
        on = (cloth.ims32[k] > 0) & ((f32(cloth.rest32[k] * cloth.rest32[k]) + length.astype(f32)).astype(f32) > f32(1e-5))
        kk = np.zeros(len(k))
        kk[on] = (sq_rest[on] - length[on]) / (cloth.ims[k][on] * (sq_rest[on] + length[on]))
        p[a] -= delta * (kk * im[a])[:, None]   # a colour names no particle twice (asserted at construction): the scatter is the sweep
        p[b] += delta * (kk * im[b])[:, None]


def _solve_positions_storage(cloth, p, im):
    """p: list of [x, y, z] lists (plain Python floats are float64)"""
    A, B, rest, rest32, ims, ims32 = cloth.a.tolist(), cloth.b.tolist(), cloth.rest.tolist(), cloth.rest32, cloth.ims.tolist(), cloth.ims32
    sq32 = (rest32 * rest32).astype(f32)
    lim = f32(1e-5)
    for i in range(len(A)):
        if ims32[i] > 0:
            pa, pb = p[A[i]], p[B[i]]
            dx, dy, dz = pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]
            length = dx * dx + dy * dy + dz * dz
            sq_rest = rest[i] * rest[i]
            if f32(sq32[i] + f32(length)) > lim:
                k = (sq_rest - length) / (ims[i] * (sq_rest + length))
                ka, kb = k * im[A[i]], k * im[B[i]]
                pa[0] -= dx * ka; pa[1] -= dy * ka; pa[2] -= dz * ka
                pb[0] += dx * kb; pb[1] += dy * kb; pb[2] += dz * kb


def step64(cloth, p32, v32, wind, iterations, dt, order="colour"):
    """One applyWindForce + simulate from the float32 state (p32, v32): (positions, velocities) in float64.  Mass or stiffness set
    since the last step are taken up first, as simulate does."""
    assert order in ("colour", "storage")
    cloth.recalculate_if_changed()
    dt32 = f32(dt)
    dt = float(dt32)
    vit, pit, dit = iterations
    im32 = cloth.inv_mass
    im = im32.astype(np.float64)
    prev = np.asarray(p32, f32).astype(np.float64)
    v = np.asarray(v32, f32).astype(np.float64).copy()
    force = wind_forces64(cloth, prev, wind)
    gravity_velocity = GRAVITY_F32 * dt * float(cloth.gravity_factor)
    v[im32 > 0, 1] += gravity_velocity
    v += force * (im * dt)[:, None]
    p = prev + v * dt
    inv_dt = (1.0 / dt) if dt32 > f32(1e-5) else 1.0

    if order == "storage":
        A, B = cloth.a.tolist(), cloth.b.tolist()
        iml = im.tolist()
    if vit > 0:
        grad = prev[cloth.b] - prev[cloth.a]
        sq = np.einsum("ij,ij->i", grad, grad)
        scale = np.zeros(len(sq))
        on = cloth.ims32 != 0
        scale[on] = 1.0 / (sq[on] * cloth.ims[on])
        if order == "colour":
            for _ in range(vit):
                for k in cloth.colours:
                    if not len(k):
                        continue
                    a, b = cloth.a[k], cloth.b[k]
                    j = -np.einsum("ij,ij->i", grad[k], v[a] - v[b]) * scale[k]
                    v[a] += grad[k] * (j * im[a])[:, None]
                    v[b] -= grad[k] * (j * im[b])[:, None]
        else:
            vl, gl, sl = v.tolist(), grad.tolist(), scale.tolist()
            for _ in range(vit):
                for i in range(len(A)):
                    va, vb, g = vl[A[i]], vl[B[i]], gl[i]
                    j = -(g[0] * (va[0] - vb[0]) + g[1] * (va[1] - vb[1]) + g[2] * (va[2] - vb[2])) * sl[i]
                    ja, jb = j * iml[A[i]], j * iml[B[i]]
                    va[0] += g[0] * ja; va[1] += g[1] * ja; va[2] += g[2] * ja
                    vb[0] -= g[0] * jb; vb[1] -= g[1] * jb; vb[2] -= g[2] * jb
            v = np.array(vl)
        p = prev + v * dt

    def solve(p, count):
        if order == "colour":
            for _ in range(count):
                _solve_positions_colour(cloth, p, im)
            return p
        pl = p.tolist()
        for _ in range(count):
            _solve_positions_storage(cloth, pl, iml)
        return np.array(pl)

    if pit > 0:
        p = solve(p, pit)
        v = (p - prev) * inv_dt
    if dit > 0:
        prev = p.copy()
        p = solve(p, dit)
        v = v + (p - prev) * inv_dt
    v = v * (1.0 / (1.0 + dt * float(cloth.damping)))
    return p, v


def mix_class(iterations):
    vit, pit, dit = (int(i > 0) for i in iterations)
    return {0: "integrate", 1: "velocity", 2: "position", 4: "drift"}.get(vit + 2 * pit + 4 * dit, "mixed")


def units(p, v, iterations, dt):
    """(position unit, velocity unit) of the deviation table for a step that ended at the float64 state (p, v)"""
    dt32 = f32(dt)
    inv_dt = 1.0 / float(dt32) if dt32 > f32(1e-5) else 1.0
    scale_p = max(1.0, float(np.abs(p).max()))
    scale_v = max(1.0, float(np.abs(v).max()))
    if iterations[1] > 0 or iterations[2] > 0:
        scale_v = max(scale_v, scale_p * inv_dt)
    return EPS32 * scale_p, EPS32 * scale_v


def deviation(p32, v32, p64, v64, iterations, dt):
    """(positions, velocities) of a float32 result from step64's, in units()"""
    up, uv = units(p64, v64, iterations, dt)
    return float(np.abs(p32.astype(np.float64) - p64).max()) / up, float(np.abs(v32.astype(np.float64) - v64).max()) / uv


# ---------------------------------------------------------------------------------------------------------------------------
# The battery
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, grid, mix):
        gx, gy, width, height = GRIDS[grid]
        self.grid, self.mix = grid, mix
        self.gx, self.gy, self.width, self.height = gx, gy, width, height
        self.n = gx * gy
        self.iterations = MIXES[mix]
        self.wind, self.dt = WORLD_OF_MIX[mix]
        self.gravity_factor = GRAVITY_FACTORS[(grid + mix) % 3]
        self.damping = DAMPINGS[(grid + 2 * mix) % 3]
        self.stiffness = STIFFNESSES[(3 * grid + mix) % 4]
        self.mass = (2.0 + (grid + mix) % 2) * max(width * height, 2.0)   # 2 or 3 kg per square metre, the small and the strips heavier: the wind's acceleration stays that of a cloth
        self.pos = POSITIONS[(grid + mix) % 7]
        self.rot = (YAWS if self.wind is WIND_IN_PLANE else ROTATIONS)[(2 * grid + mix) % 7]
        self.name = "%dx%d-%d%d%d" % ((gx, gy) + self.iterations)

    def instantiate(self, world):
        """the cloth in a device or oracle world; stiffness values outside the clamp go in through cloth_set_properties"""
        late = not 0.01 <= self.stiffness <= 1.0
        c = world.add_cloth(self.width, self.height, self.gx, self.gy, self.mass, 0.5 if late else self.stiffness, self.damping, self.gravity_factor)
        world.cloth_set_fixed_vertices(c, self.pos, self.rot, True)
        if late:
            world.cloth_set_properties(c, self.mass, self.stiffness, self.damping, self.gravity_factor)
        return c

    def cloth64(self):
        late = not 0.01 <= self.stiffness <= 1.0
        c = Cloth64(self.width, self.height, self.gx, self.gy, self.mass, 0.5 if late else self.stiffness, self.damping, self.gravity_factor)
        if late:
            c.set_properties(self.mass, self.stiffness, self.damping, self.gravity_factor)
        return c


def battery():
    """every grid with every iteration mix"""
    return [Case(g, m) for m in range(len(MIXES)) for g in range(len(GRIDS))]


def world_order():
    """grid indices in the order a world holds them: 33 x 71, 2 x 2, 52 x 45, 3 x 3, 27 x 19, 1171 x 2, 32 x 16, 4 x 5, 2 x 1170, 2 x 3,
    3 x 2.  Larger-than-LDS cloths sit first, in the middle and between LDS-sized ones, so the kernel's `list` is a true reordering, and
    most cloths' n is below maxSmallParticles."""
    return [9, 0, 7, 3, 6, 10, 5, 4, 8, 1, 2]


def step_dt(case_or_dt, k):
    """dt of the step with index k: the first step is taken at the float32 above 1e-5 and the sixth at 1e-5 (see the module's docstring)"""
    dt = case_or_dt.dt if isinstance(case_or_dt, Case) else case_or_dt
    return {0: DT_ABOVE, 5: DT_EDGE}.get(k, f32(dt))


def far_body(w):
    """a world without a rigid body does not step (physics.cpp returns before the cloths): one small sphere, far from every cloth"""
    b = w.add_body((500.0, 500.0, 500.0), (0, 0, 0, 1), gravity_factor=0.0)
    w.add_collider(b, 0, (0.0, 0.0, 0.0, 0.5), (0.1, 0.5, 1.0))
    return b


def build_world(world_module, mix, grids=None, colour_order=True):
    """A world (device or oracle: world_module.World / OracleWorld is passed in as the constructor) with the cloths of one mix in
    world_order(), its wind as a global force field, and one far-away rigid body, because a world without one does not step.
    Returns (world, cases, cloth ids)."""
    w = world_module()
    far_body(w)
    cases = [Case(g, mix) for g in (world_order() if grids is None else grids)]
    ids = [c.instantiate(w) for c in cases]
    w.set_cloth_iterations(*MIXES[mix])
    w.set_cloth_colour_order(colour_order)
    wind = WORLD_OF_MIX[mix][0]
    if wind is not None:
        w.add_force_field(wind)
    return w, cases, ids
