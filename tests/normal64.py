"""Float64 reading of the hit normal of mi_raycast_sensors (the rule: include/mi_physics.h; the device: csrc/ray_normals.h), on top of
ray64's Shape / reference_hit and raycast_util's whole-world expectation, and of the terrain normal on top of terrain_ray64.

The normal is the surface's outward normal at p = local origin + t * local direction, t being what the reference's ray test reports
(ray64.reference_hit), rotated to world space.  Per kind, in the collider's frame:
  sphere    (p - c) / |p - c|
  capsule   away from the closest point of the segment a b
  cylinder  the cap's normal where p is less deep under a cap than under the side (dc < ds), else the radial direction
  boxes     the face whose plane p is farthest out of (or least deep under); of equal ones the lowest axis
  hull      the normal of the lowest-indexed triangle among those the ray meets at the smallest distance
  terrain   the normal of the hit triangle, y > 0
With the normal comes the decision margin, relative to the shape's size: how far p is from every place where the rule switches branch
(cylinder: dc = ds, the rim; boxes: two axes equally far out, edges and corners; hull: the edges of the winning triangle; sphere,
capsule and the cylinder's side: the centre or axis, where the direction is not defined; terrain: terrain_ray64's triangle_decided,
i.e. the cell diagonal and the cell border).  A case is `decided` when the hit itself is (raycast_util.expect_cast) and the margin
clears ray64.DECIDED_MARGIN plus the rounding of the coordinates.  An undecided case carries `alternatives`: the normals of the
branches next to p, one of which the device must still report.

rule32() restates csrc/ray_normals.h in float32 numpy, operation by operation, from the float32 world ray, pose and record and a
float32 t.  tests/test_normal64_cpu.py measures, per family, the largest |n32 - n64| (the chord, which is the angle for small angles) over the decided
cases, with t32 the distance the oracle reports for the case (the device reports its bits: tests/test_gpu_raycast.py): the figure
then holds the rounding of t, of the local ray and of the rule.  MEASURED_ANGLE holds what tests/test_normal64_cpu.py printed on
x86-64; the device's tolerance is 4 x these (tests/test_gpu_raycast_sensors.py)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402
import raycast_util as rcu  # noqa: E402

F32_EPS = r64.F32_EPS

# family -> largest |n32 - n64| over the family's decided hits (tests/test_normal64_cpu.py prints it).  bound() returns 4 x these.
MEASURED_ANGLE = {
    "axis+y": 6.89e-07,
    "axis-antiparallel": 6.89e-07,
    "axis-skew": 2.63e-06,
    "box-axis-aligned": 0,
    "capsule-degenerate": 7.9e-07,
    "cylinder-cap": 0,
    "cylinder-perpendicular": 9.65e-08,
    "far-1e3": 1.25e-05,              # the local ray is formed at coordinates of 1e3: one rounding there is 6e-5 against radii of 0.3 .. 0.5
    "hull": 0,
    "hull-back-face": 0,
    "hull-two-geometries": 5.42e-08,
    "inside-capsule": 5.8e-07,
    "inside-cylinder": 6.24e-07,
    "inside-hull": 6.69e-08,
    "inside-sphere": 6.79e-08,
    "normal-box-faces": 6.97e-08,
    "normal-cap-inside-radius": 0,
    "normal-capsule-parts": 6.13e-07,
    "normal-far-cylinder": 6.37e-06,  # as far-1e3
    "nothing": 9.65e-08,
    "order": 9.65e-08,
    "posed-aabb": 6.27e-08,
    "posed-capsule": 9.35e-07,
    "posed-cylinder": 9.35e-07,
    "posed-hull": 1.16e-07,
    "posed-obb": 6.97e-08,
    "posed-sphere": 1.39e-06,
    "scale-100m": 1.04e-06,
    "scale-1cm": 9.05e-07,
    "sphere": 1.23e-06,
    "tangent-sphere": 7.03e-05,       # just-inside: the ray runs along the surface, so the error of t (5.9e-6 of 1 + t, ray64.MEASURED) moves the point across the normals
    "tie": 4.41e-07,
    "unwritten-t": 9.77e-07,
}
# the terrain battery: family -> largest |n32 - n64| over the decided hits
MEASURED_TERRAIN_ANGLE = {
    "far-origin": 1.64e-06,
    "from-below": 8.01e-07,
    "from-outside": 1.15e-06,
    "max-t": 1.04e-06,
    "slanted": 1.49e-06,
    "through-hole": 5.58e-07,
    "vertical-interior": 1.14e-06,
}
# families of terrain_ray64's battery whose rays are aimed at grid lines, vertices, diagonals, seams or the rim on purpose: their
# triangle, and with it the normal, is undecided by construction.  They are kept apart from the battery the 90 % condition is put on
# (terrain_battery) and checked as knife edges (terrain_knife_edges): one of the adjacent triangles' normals.
TERRAIN_KNIFE_EDGE = ("vertical-corner", "vertical-axis-edge", "vertical-diagonal", "vertical-seam", "vertical-rim", "grid-line")


def bound(family):
    return 4.0 * MEASURED_ANGLE[family]


def terrain_bound(family):
    return 4.0 * MEASURED_TERRAIN_ANGLE[family]


# ---------------------------------------------------------------------------------------------------------------------------
# The rule in float64, in the collider's frame
# ---------------------------------------------------------------------------------------------------------------------------
class Normal:
    """n: the unit normal (zero where the rule gives zero); margin: distance of p to the nearest branch switch, relative to the
    shape's size; alternatives: the normals of every branch within reach of p (n among them)."""

    def __init__(self, n, margin, alternatives=None):
        self.n, self.margin = np.asarray(n, np.float64), float(margin)
        self.alternatives = [self.n] if alternatives is None else [np.asarray(a, np.float64) for a in alternatives]


def _unit(v):
    l = float(np.linalg.norm(v))
    return v / l if l * l >= 1e-8 else np.zeros(3)          # noz


def _point_triangle_distance(p, tri):
    """distance of p to the (closed) triangle tri [3, 3]"""
    a, b, c = tri
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n)
    off = float((p - a) @ n)
    q = p - off * n
    inside = all(float(np.cross(tri[(i + 1) % 3] - tri[i], q - tri[i]) @ n) >= 0.0 for i in range(3))
    if inside:
        return abs(off)
    return min(float(r64._segment_distance(p, tri[i], tri[(i + 1) % 3])) for i in range(3))


def local_normal(shape, origin, direction, t, reach=r64.DECIDED_MARGIN):
    """Normal of `shape` (a ray64.Shape) for the ray (origin, direction) in its frame and the distance t; `reach`: how far, relative
    to the shape's size, a neighbouring branch counts as an alternative."""
    o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
    p = o + t * d
    size = float(shape.size)
    if shape.kind == r64.SPHERE:
        return Normal(_unit(p - shape.c), float(np.linalg.norm(p - shape.c)) / size)
    if shape.kind == r64.CAPSULE:
        ab = shape.b - shape.a
        den = float(ab @ ab)
        s = min(1.0, max(0.0, float((p - shape.a) @ ab) / den)) if den > 0 else 0.0
        away = p - (shape.a + s * ab)
        return Normal(_unit(away), float(np.linalg.norm(away)) / size)
    if shape.kind == r64.CYLINDER:
        u, h = r64._axis(shape)
        y = float((p - shape.a) @ u)
        rho = (p - shape.a) - y * u
        dc, ds = min(y, h - y), shape.r - float(np.linalg.norm(rho))
        cap, side = (u if y > 0.5 * h else -u), _unit(rho)
        switch = abs(dc - ds) / size
        if dc < ds:
            margin, n = min(switch, abs(y - 0.5 * h) / size), cap
        else:
            margin, n = min(switch, float(np.linalg.norm(rho)) / size), side
        return Normal(n, margin, [cap, side] if switch <= reach else [n])
    if shape.kind in (r64.AABB, r64.OBB):
        sd = shape.n @ p - shape.h                      # per face: > 0 outside its plane; faces k and k + 3 are the two of axis k
        out = np.maximum(sd[0:3], sd[3:6])              # |q_k| - e_k
        k = int(np.argmax(out))                         # (argmax takes the lowest index of equal ones)
        face = k if sd[k] >= sd[k + 3] else k + 3       # sign(q_k), + at q_k = 0
        rest = np.delete(out, k)
        margin = min(float(out[k] - rest.max()), float(abs(sd[k] - sd[k + 3])) * 0.5) / size
        alts = [shape.n[j if sd[j] >= sd[j + 3] else j + 3] for j in range(3) if out[k] - out[j] <= reach * size]
        return Normal(shape.n[face], margin, alts)
    if shape.kind == r64.HULL:
        dl = float(np.linalg.norm(d))
        best, win = math.inf, None
        for f, tri in enumerate(shape.tris):
            nd = float(shape.n[f] @ d)
            if abs(nd) <= 1e-6:
                continue
            tt = float(shape.h[f] - shape.n[f] @ o) / nd
            if tt < 0.0 or _point_triangle_distance(o + tt * d, tri) > 1e-9 * (1.0 + size):
                continue
            if tt < best - 1e-9 * (1.0 + abs(best) if math.isfinite(best) else 1.0):
                best, win = tt, f
        if win is None:
            return Normal(np.zeros(3), 0.0, [np.zeros(3)] + [shape.n[f] for f in range(len(shape.tris)) if _point_triangle_distance(p, shape.tris[f]) <= reach * size])
        tri = shape.tris[win]
        edges = min(float(r64._segment_distance(p, tri[i], tri[(i + 1) % 3])) for i in range(3))
        grazing = abs(float(shape.n[win] @ d)) / dl
        alts = [shape.n[f] for f in range(len(shape.tris)) if _point_triangle_distance(p, shape.tris[f]) <= reach * size]
        return Normal(shape.n[win], min(edges / size, grazing), alts if alts else [shape.n[win]])
    raise ValueError(shape.kind)


# ---------------------------------------------------------------------------------------------------------------------------
# The whole-world expectation
# ---------------------------------------------------------------------------------------------------------------------------
class Expected:
    """raycast_util.CastExpected plus the world normal: hit, collider, body, t; normal [3] float64 (zero for a miss); decided: neither
    the hit nor the branch of the normal rule can be flipped by float32; alternatives: world normals of the branches next to the hit."""

    def __init__(self, cast):
        self.cast = cast
        self.hit, self.collider, self.body, self.t = cast.hit, cast.collider, cast.body, cast.t
        self.normal, self.alternatives, self.decided, self.margin = np.zeros(3), [np.zeros(3)], cast.decided, math.inf


def expect(cw, ray, static=True, poses=None, exclude=None):
    """What mi_raycast_sensors must report for the WORLD ray `ray` [8] in the CastWorld cw; exclude = (first, count): the bodies whose
    colliders are no candidates."""
    cands = cw.candidates(static, poses)
    if exclude is not None:
        first, count = exclude
        cands = [c for c in cands if c[1] == rcu.STATIC_BODY or ((c[1] - first) & 0xFFFFFFFF) >= count]
    e = Expected(rcu.expect_cast(ray, cands))
    if not e.hit:
        return e
    pos, rot = e.cast.frame
    R = r64.quat_to_matrix(rot)
    shape = cw._prepared(e.collider)[0]
    r = r64._f64(ray)
    o, d = R.T @ (r[0:3] - pos), R.T @ r[4:7]
    rounding = 64 * F32_EPS * (float(np.abs(r[0:3]).max()) + float(np.abs(pos).max()) + shape.size) / shape.size
    ln = local_normal(shape, o, d, e.t, reach=2.0 * (r64.DECIDED_MARGIN + rounding))
    e.normal, e.alternatives, e.margin = R @ ln.n, [R @ a for a in ln.alternatives], ln.margin
    if ln.margin <= r64.DECIDED_MARGIN + rounding:
        e.decided = False
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# The rays the rule needs and ray64.ray_battery() lacks
# ---------------------------------------------------------------------------------------------------------------------------
def extra_cases():
    """[ray64.Case]: the cap from inside the radius (the cap disk is taken by rule R4 and the hit is on the cap), each of the six faces
    of a box, and a capsule's cylinder part against its end spheres."""
    cases = []
    cyl = r64.Scene([((0, 0, 0), r64.IDENT)], [(0, r64.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5))])
    cases.append(r64.Case("normal-cap-inside-radius", "top-from-above", cyl, r64.ray((0.2, 3, 0.1), (0.02, -1, 0.03))))
    cases.append(r64.Case("normal-cap-inside-radius", "bottom-from-below", cyl, r64.ray((-0.1, -3, 0.25), (0.03, 1, -0.02))))
    cases.append(r64.Case("normal-cap-inside-radius", "top-near-the-rim", cyl, r64.ray((0.42, 2, 0.0), (0, -1, 0), unit=False)))
    body = (np.array([1.0, 0.5, -2.0], np.float32), r64.Q_BODY)
    for kind, name in ((r64.AABB, "aabb"), (r64.OBB, "obb")):
        sc = r64.Scene([body], [(0, kind, r64._local_shape(kind))])
        Rb = r64.quat_to_matrix(r64.Q_BODY)
        Rs = r64.quat_to_matrix(r64.Q_COL) if kind == r64.OBB else np.eye(3)
        he = np.array([0.5, 0.3, 0.4])
        for axis in range(3):
            for sign in (1.0, -1.0):
                nl = np.zeros(3)
                nl[axis] = sign
                on_face = np.array([0.11, -0.07, 0.09]) * (1.0 - np.abs(nl)) + nl * he       # a point of the face, off its middle
                to_world = lambda v: r64._f64(body[0]) + Rb @ (np.array([0.3, -0.2, 0.1]) + Rs @ v)   # noqa: E731
                target, start = to_world(on_face), to_world(on_face + 3.0 * nl + np.array([0.2, 0.15, -0.1]) * (1.0 - np.abs(nl)))
                cases.append(r64.Case("normal-box-faces", "%s-%s%s" % (name, "+" if sign > 0 else "-", "xyz"[axis]), sc, r64.ray(start, target - start)))
    cap = r64.Scene([((0, 0, 0), r64.IDENT)], [(0, r64.CAPSULE, (0, -1, 0, 0, 1, 0, 0.5))])
    cases.append(r64.Case("normal-capsule-parts", "cylinder-part", cap, r64.ray((-3, 0.4, 0.1), (1, 0, 0), unit=False)))
    cases.append(r64.Case("normal-capsule-parts", "cylinder-part-oblique", cap, r64.ray((-3, 0.9, 0.2), (1, -0.2, -0.05))))
    cases.append(r64.Case("normal-capsule-parts", "upper-sphere", cap, r64.ray((-3, 1.3, 0.1), (1, 0, 0), unit=False)))
    cases.append(r64.Case("normal-capsule-parts", "lower-sphere-from-below", cap, r64.ray((0.1, -4, 0.15), (0, 1, 0), unit=False)))
    far = (np.array([1000.0, -1000.0, 1000.0], np.float32), r64.Q_BODY)
    sc = r64.Scene([far], [(0, r64.CYLINDER, r64._local_shape(r64.CYLINDER))])
    axis = r64._world_dir(far, r64.quat_to_matrix(r64.Q_COL) @ np.array([0.0, 1.0, 0.0]))
    side = np.cross(axis, (0.3, 1.0, 0.2))
    side /= np.linalg.norm(side)
    centre = r64._world_point(far, (0.3, -0.2, 0.1))
    cases.append(r64.Case("normal-far-cylinder", "side", sc, r64.ray(centre + 5.0 * side + 0.05 * axis + 0.1 * np.cross(axis, side), -side)))
    cases.append(r64.Case("normal-capsule-parts", "just-above-the-seam", cap, r64.ray((-3, 1.05, 0.0), (1, 0, 0), unit=False)))
    return cases


# Cases of ray64.ray_battery() whose HIT is decided but whose hit point lies on a branch switch of the normal rule by construction (the
# ray enters through a box corner, through a cylinder's rim): for the normal they are knife edges and get a family name that says so.
NORMAL_KNIFE_EDGE = {"box-through-corner/aabb-diagonal": "vertex-box-through-corner", "box-through-corner/obb-diagonal": "vertex-box-through-corner",
                     "cylinder-cap/in-through-the-rim": "edge-cylinder-cap-rim"}
# Left out: the hit is 1.6 % of the cylinder's size from its rim, and at coordinates of 1e3 the rounding allowance (64 ulps of 2e3
# against a size of 0.9) is 1.7 %: not a knife edge, not decided.  extra_cases() has a cylinder at 1e3 hit in the middle of its side.
LEFT_OUT = ("far-1e3/cylinder",)
_BATTERY = None


def battery():
    """ray64.ray_battery() (NORMAL_KNIFE_EDGE renamed, LEFT_OUT left out) and extra_cases()"""
    global _BATTERY
    if _BATTERY is None:
        base = [c if c.id not in NORMAL_KNIFE_EDGE else r64.Case(NORMAL_KNIFE_EDGE[c.id], c.name, c.scene, c.ray) for c in r64.ray_battery() if c.id not in LEFT_OUT]
        _BATTERY = base + extra_cases()
    return _BATTERY


def case_expect(case, max_t=np.inf):
    """Expected of a case in a world of its own (raycast_util.single_world), unmoved, bodies only"""
    return expect(rcu.single_world(case), rcu.with_max_t(case.ray, max_t), static=False)


# ---------------------------------------------------------------------------------------------------------------------------
# The terrain
# ---------------------------------------------------------------------------------------------------------------------------
def terrain_normal_of(T, triangle):
    """float64 normal of triangle id `triangle` of a terrain_ray64.Terrain"""
    tri = T.triangles()
    k = int(np.searchsorted(tri["id"], triangle))
    assert tri["id"][k] == triangle
    return tri["n"][k]


class TerrainExpected:
    def __init__(self, e, T):
        self.e, self.hit, self.t, self.triangle = e, e.hit, e.t, e.triangle
        self.decided = bool(e.hit and e.triangle_decided)
        self.hit_decided = e.hit_decided
        self.normal = terrain_normal_of(T, e.triangle) if e.hit else np.zeros(3)


def terrain_expect(T, ray):
    return TerrainExpected(T.expect(ray), T)


def terrain_battery():
    """(layouts, cases of terrain_ray64's battery outside TERRAIN_KNIFE_EDGE)"""
    import terrain_ray64 as t64
    layouts, cases = t64.battery()
    return layouts, [c for c in cases if c.family not in TERRAIN_KNIFE_EDGE]


def terrain_knife_edges():
    import terrain_ray64 as t64
    layouts, cases = t64.battery()
    return layouts, [c for c in cases if c.family in TERRAIN_KNIFE_EDGE]


def terrain_triangle_normal32(T, tri_id):
    """noz(cross(b - a, c - a)) of a triangle by the device's formulas in float32 numpy (vertex formulas as terrain_ray64.triangle_t32)"""
    import terrain_ray64 as t64
    f = np.float32
    tri_id = int(tri_id)
    which, cell, chunk = tri_id & 1, (tri_id >> 1) & 16383, tri_id >> 15
    cx, cz, X, Z = cell & 127, cell >> 7, chunk % T.cpd, chunk // T.cpd
    H = T.chunks[(X, Z)]
    cs, hs = f(T.chunk_size / f(t64.CELLS)), f(T.amplitude / f(65535))
    mn = np.array([f(f(X) * T.chunk_size) + T.corner[0], f(0) + T.corner[1], f(f(Z) * T.chunk_size) + T.corner[2]], f)

    def vert(dx, dz):
        return np.array([f(f(cx + dx) * cs) + mn[0], f(f(H[cz + dz, cx + dx]) * hs) + mn[1], f(f(cz + dz) * cs) + mn[2]], f)
    A, B, C, D = vert(0, 0), vert(0, 1), vert(1, 0), vert(1, 1)
    a, b, c = (A, B, C) if which == 0 else (C, B, D)
    return _noz32(_cross32((b - a).astype(f), (c - a).astype(f)))


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/ray_normals.h in float32 numpy
# ---------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _v32(*a):
    return np.array(a, f32)


def _dot32(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _cross32(a, b):
    return _v32(f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0])))


def _noz32(a):
    sl = _dot32(a, a)
    return np.zeros(3, f32) if sl < f32(1e-8) else (a * f32(f32(1) / np.sqrt(sl))).astype(f32)


def _qmul32(a, b):
    av, bv = a[0:3], b[0:3]
    w = f32(f32(a[3] * b[3]) - _dot32(av, bv))
    v = ((av * b[3]).astype(f32) + (bv * a[3]).astype(f32)).astype(f32) + _cross32(av, bv)
    return _v32(v[0], v[1], v[2], w)


def _conj32(q):
    return _v32(-q[0], -q[1], -q[2], q[3])


def _rot32(q, v):
    return _qmul32(_qmul32(q, _v32(v[0], v[1], v[2], 0)), _conj32(q))[0:3]


def _box32(p, lo, hi):
    q, e = (p - ((lo + hi).astype(f32) * f32(0.5)).astype(f32)).astype(f32), ((hi - lo).astype(f32) * f32(0.5)).astype(f32)
    dist = (np.abs(q) - e).astype(f32)
    k, best = 0, dist[0]
    for j in (1, 2):
        if dist[j] > best:
            k, best = j, dist[j]
    n = np.zeros(3, f32)
    n[k] = f32(-1) if q[k] < 0 else f32(1)
    return n


def rule32(ctype, shape10, hulls, ray, pos, rot, t, triangle=None):
    """The world normal by csrc/ray_normals.h and k_rc_sensor_normals in float32: the world ray [8], the pose and the 10 shape floats as
    float32, t the float32 distance; triangle: for a hull, the index of the winning triangle (its choice is not restated)."""
    s = np.asarray(shape10, f32)
    ray, pos, rot, t = np.asarray(ray, f32), np.asarray(pos, f32), np.asarray(rot, f32), f32(t)
    lo, ld = _rot32(_conj32(rot), (ray[0:3] - pos).astype(f32)), _rot32(_conj32(rot), ray[4:7])
    p = (lo + (ld * t).astype(f32)).astype(f32)
    if ctype == r64.SPHERE:
        n = _noz32((p - s[0:3]).astype(f32))
    elif ctype == r64.CAPSULE:
        a, b = s[0:3], s[3:6]
        ab = (b - a).astype(f32)
        den = _dot32(ab, ab)
        k = f32(0)
        if den > 0:
            k = f32(_dot32((p - a).astype(f32), ab) / den)
            k = f32(0) if k < 0 else (f32(1) if k > 1 else k)
        n = _noz32((p - (a + (ab * k).astype(f32)).astype(f32)).astype(f32))
    elif ctype == r64.CYLINDER:
        a, b, r = s[0:3], s[3:6], s[6]
        ab = (b - a).astype(f32)
        u, h = _noz32(ab), np.sqrt(_dot32(ab, ab))
        pa = (p - a).astype(f32)
        y = _dot32(pa, u)
        rho = (pa - (u * y).astype(f32)).astype(f32)
        dc = y if y < f32(h - y) else f32(h - y)
        ds = f32(r - np.sqrt(_dot32(rho, rho)))
        n = (u if y > f32(h * f32(0.5)) else -u) if dc < ds else _noz32(rho)
    elif ctype == r64.AABB:
        n = _box32(p, s[0:3], s[3:6])
    elif ctype == r64.OBB:
        q, ce, ra = s[0:4], s[4:7], s[7:10]
        bo, bd = _rot32(_conj32(q), (lo - ce).astype(f32)), _rot32(_conj32(q), ld)
        n = _rot32(q, _box32((bo + (bd * t).astype(f32)).astype(f32), (np.zeros(3, f32) - ra).astype(f32), ra))
    elif ctype == r64.HULL:
        v, tri = hulls[int(s[7])]
        a, b, c = (np.asarray(v, f32).reshape(-1, 3)[i] for i in np.asarray(tri).reshape(-1, 3)[triangle])
        n = _rot32(s[0:4], _noz32(_cross32((b - a).astype(f32), (c - a).astype(f32))))
    else:
        raise ValueError(ctype)
    return _rot32(rot, n)


def winning_triangle(shape, n_local):
    """index of the hull triangle whose normal is n_local (the lowest of equal ones)"""
    return int(np.argmin(np.linalg.norm(shape.n - n_local[None, :], axis=1)))


def case_normal32(case, e, t32):
    """rule32 for a battery case in a world of its own whose expectation is e (an Expected with a hit) and whose float32 distance is t32"""
    cw = rcu.single_world(case)
    c = cw.colliders[e.collider]
    pos, rot = cw.bodies[c["body"]]
    tri = None
    if c["type"] == r64.HULL:
        R = r64.quat_to_matrix(r64._f64(rot))
        tri = winning_triangle(cw._prepared(e.collider)[0], R.T @ e.normal)
    return rule32(c["type"], c["shape"], cw.hulls, case.ray, pos, rot, t32, tri)
