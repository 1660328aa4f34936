"""Float64 reading of testPhysicsInteraction's ray tests (csrc/ray_tests.h, the oracle's intersect*) and the ray edge-case battery.

An independent reference in the style of geom64.py and joint64.py: pure numpy in float64 on the float32 records.  It shares no
formula with ray_tests.h or the oracle, only the 10-float shape layouts (sphere c,r | capsule, cylinder a,b,r | aabb min,max |
obb q,centre,half extents | hull q,position,geometry index).  Two layers, kept apart:

GEOMETRY.  first_hit(shape, origin, direction): the distance t at which a ray that starts OUTSIDE a shape first touches it, or None.
Every shape but the capsule is convex and written as an intersection of convex sets whose crossing interval has a closed form: the
sphere and the infinite cylinder a quadratic, boxes three slabs, the cylinder's caps one slab, a hull the half-spaces of its
triangles.  The ray hits where the intervals overlap, at the largest entry.  A capsule is the union of a cylinder and two spheres:
the smallest first hit of the three.  With t comes the decision margin: how far the ray is from flipping between hit and miss,
relative to the shape's size: the length of the overlap (the chord: 0 for a tangent ray, a ray through a rim or along an edge), the
distance to the faces the ray runs parallel to, how far behind the origin the shape ends.  push() turns t into force and torque.

THE REFERENCE'S SEMANTICS WHERE THEY ARE NOT GEOMETRY.  reference_hit() applies these rules, each stated where it is implemented:
  R1  an origin inside a sphere gives t = 0 (the distance is clamped); an origin on the surface looking inwards gives t = 0 too.
  R2  an origin inside a box is a miss (the entry distance must be > 0).
  R2a an origin exactly on a slab plane of an axis the ray does not move along is a miss: (plane - origin) * (1 / 0) is 0 * inf, a
      NaN, and the reference's min / max (`(a < b) ? a : b`, `(a < b) ? b : a`: a NaN first operand is replaced by the second in
      min and kept in max) turn it into an entry distance of +inf (lower plane) or an exit distance of -inf (upper plane), first,
      second or third axis alike.  The component is always +0 by then: a -0 does not survive the rotation into the body's frame
      (w * -0 + y * 0 - z * 0 = +0), so the cases a -0 would open (the axis ignored, earlier exits forgotten) cannot be reached.
  R2b an origin exactly on a face and strictly within the other two slabs is a miss whichever way it looks: looking in, the entry
      distance is exactly 0, which is not > 0; looking out it is negative.  (Exact means exact: bodies and boxes with identity
      rotation and float32 coordinates.  Anything else near a face is a knife edge and undecided.)
  R3  a hull is a surface, not a solid: every triangle is tested with t >= 0 and the smallest wins, so an origin inside hits the
      face it leaves through.  A point on an edge or vertex shared by two triangles may belong to neither (sign-bit test).
  R4  a cylinder whose origin is radially inside the infinite cylinder never tests its side.  It takes the cap disk that faces
      the ray (the upper one for a ray going down the axis, the lower one for a ray going up) where the ray's LINE crosses its
      plane within the radius, at the signed distance: negative, a hit behind the ray, when the origin is beyond that end looking
      away, or inside.  Where no disk is taken the distance stays what it was initialised to, 0, and it is a hit if the origin
      is between the end planes.  (The reference leaves that start value unwritten for capsules; 0 is what the cylinder
      collider gets, and what the oracle and the device now use for both.)
  R5  direction components below 1e-6 against a plane are a miss of that plane (cap disks, hull triangles); the cylinder's side
      needs a discriminant >= 1e-6 and a distance > 1e-6 (absolute numbers: a 1 cm cylinder loses its outermost 2 % of radius).
  R6  a capsule is its cylinder by R4 / R5 and its two spheres by R1, smallest distance (negative ones included); a capsule of
      zero length has no cylinder part (its axis cannot be normalised: every comparison is false).
  R7  a disabled ray (r1.w == 0), a dead body and a body without colliders give 0.
  R8  of equal distances the lowest collider index wins; the push goes to that collider's body.

expect() combines both for one ray against a body range and says whether the answer is `decided`: every margin clear of what
float32 rounding can move (DECIDED_MARGIN plus the rounding of the coordinates involved).  Undecided cases exist on purpose
(tangent, edge, vertex, parallel families): the device, the host and the oracle must still agree with each other on them.

BOUNDS.  The oracle's error against this module was measured over the battery per family (tests/test_oracle_rays.py prints it):
worst |t32 - t64| / (1 + |t64|) and worst |torque32 - torque64| / (strength * (1 + |arm|)), arm = hit point - centre of gravity.
(t comes from the oracle's own getter: the force is along the ray, so the torque does not depend on where along the ray it is applied,
and t cannot be recovered from the push.  It decides which collider is hit, and its rounding shows in the torque's last bits.)  The bound used is
4 x the measured worst (headroom for another libm on another host, nothing more).  MEASURED below holds the values; families
above 64 * 2**-23 = 7.6e-6 carry their reason.
"""
import math

import numpy as np

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
TYPE_NAMES = ("sphere", "capsule", "cylinder", "aabb", "obb", "hull")
MATERIAL = (0.1, 0.5, 1.0)
DECIDED_MARGIN = 1e-3          # relative to the shape's size
F32_EPS = 2.0 ** -23
KNIFE_EDGE = ("tangent", "edge", "vertex", "parallel")   # only families whose name starts with one of these may hold undecided cases
ANTIPARALLEL = "axis-antiparallel"                       # the family whose cylinder frame goes through libm sinf / cosf
WELL_CONDITIONED = 64 * F32_EPS

# family -> (worst t error, worst torque error) of the oracle over the battery's decided cases, measured by test_oracle_rays.py
# (x86-64, glibc).  Units: see BOUNDS above.  bound() returns 4 x these.
MEASURED = {
    "axis+y": (2.25e-07, 3.65e-08),
    "axis-antiparallel": (2.25e-07, 3.65e-08),
    "axis-skew": (6.11e-07, 5.63e-08),
    "box-axis-aligned": (0, 7.37e-09),
    "box-through-corner": (2.42e-08, 3.3e-08),
    "capsule-degenerate": (1.88e-07, 1.6e-07),
    "cylinder-behind": (2.03e-08, 5.76e-09),
    "cylinder-cap": (1.5e-07, 9.3e-09),
    "cylinder-perpendicular": (6.28e-08, 1.94e-09),
    "far-1e3": (9.81e-07, 2.49e-05),
    "hull": (0, 1.21e-08),
    "hull-back-face": (2.7e-08, 1.5e-08),
    "hull-two-geometries": (1.75e-07, 1.02e-07),
    "inside-capsule": (0, 2.39e-08),
    "inside-cylinder": (0, 1.89e-08),
    "inside-hull": (7.64e-08, 1.46e-08),
    "inside-sphere": (0, 1.89e-08),
    "nothing": (3.67e-08, 9.93e-10),
    "order": (7.32e-08, 9.93e-10),
    "posed-aabb": (6.32e-08, 2.84e-07),
    "posed-capsule": (9.25e-07, 2.88e-07),
    "posed-cylinder": (9.25e-07, 2.96e-07),
    "posed-hull": (6.55e-08, 1.92e-07),
    "posed-obb": (1.25e-08, 3.05e-07),
    "posed-sphere": (1.21e-06, 4.11e-07),
    "scale-100m": (9.51e-07, 1.14e-06),
    "scale-1cm": (2.03e-08, 1.33e-07),
    "sphere": (2.48e-07, 2.54e-09),
    "tangent-sphere": (5.87e-06, 8.9e-09),
    "tie": (6.28e-08, 5.38e-08),
    "unwritten-t": (1.31e-06, 5.92e-08),
}
# why the families above WELL_CONDITIONED are there
CONDITIONING = {
    "far-1e3": "torque: the hit point is formed in world space at coordinates of 1e3 (one rounding there is 6e-5) and the centre of "
               "gravity subtracted afterwards, against a lever of about 1: the error is eps * 1e3 / (1 + arm), not eps",
}


def bound(family):
    t, q = MEASURED[family]
    return 4.0 * t, 4.0 * q


# ---------------------------------------------------------------------------------------------------------------------------
# Records -> float64
# ---------------------------------------------------------------------------------------------------------------------------
def quat_to_matrix(q):
    x, y, z, w = (float(v) for v in q)
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


class Shape:
    """One collider in its body's frame.  kind; size (bounding radius); and per kind: c, r | a, b, r | planes (n [k,3], h [k]: n.x <= h)
    with, for hulls, the triangles [m,3,3]."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


def shape_from_record(ctype, shape10, hulls=()):
    """ctype, the 10 local shape floats, hulls = [(vertices [n,3], triangles [m,3])] by geometry index."""
    s = _f64(shape10)
    if ctype == SPHERE:
        return Shape(SPHERE, c=s[0:3], r=s[3], size=s[3])
    if ctype in (CAPSULE, CYLINDER):
        a, b, r = s[0:3], s[3:6], s[6]
        return Shape(ctype, a=a, b=b, r=r, size=0.5 * np.linalg.norm(b - a) + r)
    if ctype == AABB:
        lo, hi = s[0:3], s[3:6]
        n = np.concatenate([np.eye(3), -np.eye(3)])
        return Shape(AABB, n=n, h=np.concatenate([hi, -lo]), size=0.5 * np.linalg.norm(hi - lo))
    if ctype == OBB:
        R = quat_to_matrix(s[0:4])
        n = np.concatenate([R.T, -R.T])
        off = n @ s[4:7]
        return Shape(OBB, n=n, h=off + np.concatenate([s[7:10], s[7:10]]), size=np.linalg.norm(s[7:10]))
    if ctype == HULL:
        R = quat_to_matrix(s[0:4])
        v, tri = hulls[int(s[7])]
        v = s[4:7] + _f64(v).reshape(-1, 3) @ R.T
        t = v[np.asarray(tri, np.int64).reshape(-1, 3)]
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        return Shape(HULL, n=n, h=(n * t[:, 0]).sum(axis=1), tris=t, size=float(np.linalg.norm(v - v.mean(axis=0), axis=1).max()))
    raise ValueError(ctype)


# ---------------------------------------------------------------------------------------------------------------------------
# Layer 1: geometry.  Crossing intervals of convex sets; first hit of a ray that starts outside.
# ---------------------------------------------------------------------------------------------------------------------------
class _Interval:
    """[tin, tout] of the ray's line inside a convex set; `lateral`: distance to the boundaries the line runs parallel to (inside);
    `outside`: distance by which a parallel line, or one that misses, stays out (0: it crosses)."""

    def __init__(self, tin=-math.inf, tout=math.inf, lateral=math.inf, outside=0.0):
        self.tin, self.tout, self.lateral, self.outside = tin, tout, lateral, outside

    def meet(self, o):
        return _Interval(max(self.tin, o.tin), min(self.tout, o.tout), min(self.lateral, o.lateral), max(self.outside, o.outside))


def _halfspaces(n, h, o, d):
    den, dist = n @ d, h - n @ o            # dist >= 0: inside
    it = _Interval()
    par = np.abs(den) <= 1e-14 * np.linalg.norm(d)
    if np.any(par):
        it.outside = max(0.0, float((-dist[par]).max()))
        it.lateral = float(np.where(dist[par] >= 0, dist[par], np.inf).min())
    t = dist[~par] / den[~par]
    ent = den[~par] < 0
    if np.any(ent):
        it.tin = float(t[ent].max())
    if np.any(~ent):
        it.tout = float(t[~ent].min())
    return it


def _quadric(o, d, r):
    """|o + t d| <= r with o, d already projected (sphere: the full vectors, infinite cylinder: their parts across the axis)."""
    a, b, c = d @ d, o @ d, o @ o - r * r
    if a <= 1e-28:
        rho = math.sqrt(o @ o)
        return _Interval(lateral=r - rho) if rho <= r else _Interval(outside=rho - r)
    disc = b * b - a * c
    if disc < 0:
        return _Interval(math.inf, -math.inf, outside=math.sqrt(max(o @ o - b * b / a, 0.0)) - r)
    s = math.sqrt(disc)
    return _Interval((-b - s) / a, (-b + s) / a)


def _axis(shape):
    ab = shape.b - shape.a
    h = float(np.linalg.norm(ab))
    return ab / h, h


def _convex_interval(shape, o, d):
    if shape.kind == SPHERE:
        return _quadric(o - shape.c, d, shape.r)
    if shape.kind == CYLINDER:
        u, h = _axis(shape)
        rel = o - shape.a
        side = _quadric(rel - (rel @ u) * u, d - (d @ u) * u, shape.r)
        return side.meet(_halfspaces(np.array([u, -u]), np.array([h, 0.0]), rel, d))
    return _halfspaces(shape.n, shape.h, o, d)


def _convex_first_hit(shape, o, d):
    it, dl = _convex_interval(shape, o, d), float(np.linalg.norm(d))
    hit = it.outside == 0.0 and it.tin <= it.tout and it.tout >= 0.0
    if hit:
        return it.tin, min((it.tout - it.tin) * dl, it.lateral, it.tout * dl) / shape.size
    miss = [it.outside]
    if it.tin > it.tout and math.isfinite(it.tin - it.tout):
        miss.append((it.tin - it.tout) * dl)
    if it.tout < 0 and math.isfinite(it.tout):
        miss.append(-it.tout * dl)
    return None, max(miss) / shape.size


def _parts(shape):
    """a capsule as its convex parts; a capsule of zero length is one sphere"""
    ends = [Shape(SPHERE, c=shape.a, r=shape.r, size=shape.r), Shape(SPHERE, c=shape.b, r=shape.r, size=shape.r)]
    if np.all(shape.a == shape.b):
        return ends
    return [Shape(CYLINDER, a=shape.a, b=shape.b, r=shape.r, size=shape.size)] + ends


def first_hit(shape, origin, direction):
    """(t or None, margin) of the ray origin + t * direction, t >= 0, in the shape's frame; valid for origins outside the shape."""
    o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
    if shape.kind != CAPSULE:
        return _convex_first_hit(shape, o, d)
    got = [_convex_first_hit(p, o, d) for p in _parts(shape)]
    ts = [t for t, _ in got if t is not None]
    return (min(ts) if ts else None), min(m for _, m in got)


def inside_depth(shape, o):
    """> 0: the point is inside by that much; < 0: outside (not a distance, but 0 on the surface and of the right scale)"""
    if shape.kind == SPHERE:
        return shape.r - float(np.linalg.norm(o - shape.c))
    if shape.kind == CAPSULE:
        ab = shape.b - shape.a
        den = ab @ ab
        s = min(1.0, max(0.0, ((o - shape.a) @ ab) / den)) if den > 0 else 0.0
        return shape.r - float(np.linalg.norm(o - shape.a - s * ab))
    if shape.kind == CYLINDER:
        u, h = _axis(shape)
        y = (o - shape.a) @ u
        return min(shape.r - float(np.linalg.norm(o - shape.a - y * u)), y, h - y)
    return float((shape.h - shape.n @ o).min())


def push(origin, direction, strength, t, position, rotation, local_cog):
    """(force, torque about the centre of gravity) of the push at origin + t * direction; everything in world space."""
    o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
    cog = np.asarray(position, np.float64) + quat_to_matrix(rotation) @ np.asarray(local_cog, np.float64)
    force = d * strength
    return force, np.cross(o + t * d - cog, force)


# ---------------------------------------------------------------------------------------------------------------------------
# Layer 2: the reference's semantics
# ---------------------------------------------------------------------------------------------------------------------------
def _segment_distance(p, a, b):
    ab = b - a
    s = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    return np.linalg.norm(p - a - s[..., None] * ab, axis=-1)


def _sphere_rule(shape, o, d):
    depth = inside_depth(shape, o) / shape.size
    m = o - shape.c
    inward = -(m @ d) / (shape.r * np.linalg.norm(d))      # > 0: looking at the centre
    if abs(depth) < DECIDED_MARGIN and inward > 10 * DECIDED_MARGIN:
        return 0.0, inward                                   # R1, on the surface looking in: t is 0 from either side of it
    if depth > 0:
        return 0.0, depth                                    # R1
    t, margin = _convex_first_hit(shape, o, d)
    return t, min(margin, -depth)


def _box_rule(shape, o, d):
    depth = inside_depth(shape, o) / shape.size
    if depth > 0:
        return None, depth                                   # R2
    dist, den = shape.h - shape.n @ o, shape.n @ d           # per face: how far inside its plane, how fast the ray leaves through it
    on = dist == 0.0                                         # exactly: identity frames and float32 coordinates, or never
    if np.any(on & (den == 0.0)):
        return None, 1.0                                     # R2a: 0 * inf poisons the interval, whatever the other slabs say
    if np.count_nonzero(on) == 1 and np.all(dist[~on] > 0):
        return None, float(dist[~on].min()) / shape.size     # R2b: entry distance exactly 0 looking in, negative looking out
    t, margin = _convex_first_hit(shape, o, d)
    return t, min(margin, -depth)


def _hull_rule(shape, o, d):
    depth = inside_depth(shape, o) / shape.size
    it, dl = _convex_interval(shape, o, d), float(np.linalg.norm(d))
    if depth > 0:
        t, margin = it.tout, depth                           # R3: the face the ray leaves through
    else:
        t, margin = _convex_first_hit(shape, o, d)
        margin = min(margin, -depth)
        if t is None:
            return None, margin
    p = o + t * d
    tr = shape.tris
    edges = min(float(_segment_distance(p, tr[:, i], tr[:, (i + 1) % 3]).min()) for i in range(3))
    on = np.abs(shape.n @ p - shape.h) <= 1e-9 * (1 + shape.size)     # the faces through the hit point
    grazing = float(np.abs(shape.n[on] @ d).min()) / dl if on.any() else 0.0   # R5: |n.d| <= 1e-6 is a miss of that triangle
    return t, min(margin, edges / shape.size, grazing)                # R3: an edge or a vertex may belong to no triangle


def _cylinder_rule(shape, o, d):
    u, h = _axis(shape)
    rel = o - shape.a
    y0, dy = float(rel @ u), float(d @ u)
    op, dp = rel - y0 * u, d - dy * u
    rho, r, size = float(np.linalg.norm(op)), shape.r, shape.size
    radial = abs(rho - r) / size
    if rho > r:
        t, margin = _convex_first_hit(shape, o, d)
        a, b, c = dp @ dp, op @ dp, op @ op - r * r
        delta = b * b - a * c
        if abs(delta - 1e-6) <= 1e-4 * (b * b + abs(a * c)):     # ~800 float32 roundings of the terms
            margin = 0.0
        if delta < 1e-6:
            t = None                                         # R5
        if t is not None:
            if abs(t - 1e-6) < 1e-3 * 1e-6:
                margin = 0.0
            if t <= 1e-6:
                t = None                                     # R5
        return t, min(margin, radial)
    # R4: radially inside
    margin, taken, t = radial, False, 0.0
    if dy != 0.0:
        plane = h if dy < 0 else 0.0
        if abs(dy) >= 1e-6:                                  # R5
            tp = (plane - y0) / dy
            rho_p = float(np.linalg.norm(op + tp * dp))
            margin = min(margin, abs(rho_p - r) / size)
            if rho_p <= r:
                taken, t = True, tp
        if 1e-7 * np.linalg.norm(d) < abs(dy) < 1e-5 * np.linalg.norm(d):
            margin = 0.0
    if taken:
        return t, margin
    margin = min(margin, min(abs(y0), abs(h - y0)) / size)
    return (0.0 if -1e-6 < y0 < h + 1e-6 else None), margin


def reference_hit(shape, origin, direction):
    """(t or None, margin): what testPhysicsInteraction's test of this collider reports for a ray in the body's frame."""
    o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
    if shape.kind == SPHERE:
        return _sphere_rule(shape, o, d)
    if shape.kind in (AABB, OBB):
        return _box_rule(shape, o, d)
    if shape.kind == HULL:
        return _hull_rule(shape, o, d)
    if shape.kind == CYLINDER:
        return _cylinder_rule(shape, o, d)
    got = [(_cylinder_rule if p.kind == CYLINDER else _sphere_rule)(p, o, d) for p in _parts(shape)]   # R6
    ts = [t for t, _ in got if t is not None]
    return (min(ts) if ts else None), min(m for _, m in got)


class Expected:
    """body: the pushed body (index in the world) or None; collider, t, force, torque, arm (hit point - centre of gravity) of the hit;
    decided: float32 cannot flip the answer."""

    def __init__(self):
        self.body = self.collider = self.t = None
        self.force = self.torque = np.zeros(3)
        self.arm = 0.0
        self.decided = True


def expect(ray, bodies, colliders, hulls, local_cogs, alive=None):
    """One ray [8] = origin, strength, direction, enabled against `bodies` = [(index, position [3], rotation [4])], the candidates in
    index order; colliders = [(collider index, body index, type, shape10)] of the whole world; local_cogs[body index]."""
    e = Expected()
    ray = _f64(ray)
    o, strength, d, enabled = ray[0:3], ray[3], ray[4:7], ray[7]
    if enabled == 0.0:
        return e                                             # R7
    hits = []
    for b, pos, rot in bodies:
        if alive is not None and not alive[b]:
            continue                                         # R7
        pos, R = _f64(pos), quat_to_matrix(_f64(rot))
        lo, ld = R.T @ (o - pos), R.T @ d
        for c, cb, ctype, shape10 in colliders:
            if cb != b:
                continue
            shape = shape_from_record(ctype, shape10, hulls)
            t, margin = reference_hit(shape, lo, ld)
            # what float32 moves: the coordinates' rounding against the shape's size
            rounding = 64 * F32_EPS * (float(np.abs(o).max()) + float(np.abs(pos).max()) + shape.size) / shape.size
            if margin <= DECIDED_MARGIN + rounding:
                e.decided = False
            if t is not None:
                hits.append((t, c, b, pos, _f64(rot)))
    if not hits:
        return e
    hits.sort(key=lambda h_: (h_[0], h_[1]))                 # R8
    t, c, b, pos, rot = hits[0]
    for t2, c2, b2, _, _ in hits[1:]:
        if t2 != t and abs(t2 - t) <= 1e-4 * (1 + abs(t)) and b2 != b:
            e.decided = False                                # two bodies nearly as close: float32 may order them the other way
    e.body, e.collider, e.t = b, c, t
    e.force, e.torque = push(o, d, strength, t, pos, rot, _f64(local_cogs[b]))
    e.arm = float(np.linalg.norm(o + t * d - (pos + quat_to_matrix(rot) @ _f64(local_cogs[b]))))
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# The battery
# ---------------------------------------------------------------------------------------------------------------------------
def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _qaxis(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([a * math.sin(0.5 * angle), [math.cos(0.5 * angle)]]).astype(np.float32)


IDENT = np.array([0, 0, 0, 1], np.float32)
Q_BODY = _qaxis((1, 2, 3), 0.9)
Q_COL = _qaxis((-2, 1, 0.5), 1.3)

TETRA = (np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32), np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.uint32))
_BOX_SIGNS = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float32)
_BOX_TRIS = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (0, 4, 7), (0, 7, 3)], np.uint32)
BRICK = (_BOX_SIGNS * np.array([1.0, 0.5, 0.75], np.float32), _BOX_TRIS)


class Scene:
    """bodies [(position, rotation)], colliders [(body, type, shape10)] in collider index order (hull shapes carry the index into
    `hulls`), hulls [(vertices, triangles)], dead: bodies deleted after building."""

    def __init__(self, bodies, colliders, hulls=(), dead=()):
        self.bodies = [(np.asarray(p, np.float32), np.asarray(q, np.float32)) for p, q in bodies]
        self.colliders = []
        for b, t, s in colliders:
            s10 = np.zeros(10, np.float32); s10[:len(s)] = s
            self.colliders.append((b, t, s10))
        self.hulls, self.dead = list(hulls), tuple(dead)

    def instantiate(self, world, geometry_ids=None):
        """Adds the scene to a World or an OracleWorld; returns the body indices.  geometry_ids: scene hull -> geometry of the world,
        for a world that already holds them."""
        if geometry_ids is None:
            geometry_ids = [world.add_hull_geometry(v, t) for v, t in self.hulls]
        ids = [world.add_body(p, q, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0) for p, q in self.bodies]
        for b, t, s in self.colliders:
            s = s.copy()
            if t == HULL:
                s[7] = geometry_ids[int(s[7])]
            world.add_collider(ids[b], t, s, MATERIAL)
        for b in self.dead:
            world.delete_body(ids[b])
        return ids

    def expect(self, ray, local_cogs):
        alive = [i not in self.dead for i in range(len(self.bodies))]
        return expect(ray, [(i, p, q) for i, (p, q) in enumerate(self.bodies)], [(c, b, t, s) for c, (b, t, s) in enumerate(self.colliders)],
                      self.hulls, local_cogs, alive)


class Case:
    def __init__(self, family, name, scene, ray):
        self.family, self.name, self.scene = family, name, scene
        self.ray = np.asarray(ray, np.float32)
        assert self.ray.shape == (8,)

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)

    @property
    def knife_edge(self):
        return self.family.startswith(KNIFE_EDGE)


def ray(origin, direction, strength=1000.0, enabled=1.0, unit=True):
    d = _unit32(direction) if unit else np.asarray(direction, np.float32)
    return np.concatenate([np.asarray(origin, np.float32), [np.float32(strength)], d, [np.float32(enabled)]]).astype(np.float32)


def _world_point(body, local):
    p, q = body
    return _f64(p) + quat_to_matrix(_f64(q)) @ np.asarray(local, np.float64)


def _world_dir(body, local):
    return quat_to_matrix(_f64(body[1])) @ np.asarray(local, np.float64)


def _local_shape(kind, scale=1.0, q=Q_COL, offset=(0.3, -0.2, 0.1), hull=0):
    off = np.asarray(offset, np.float64) * scale
    if kind == SPHERE:
        return (*off, 0.5 * scale)
    if kind in (CAPSULE, CYLINDER):
        ax = quat_to_matrix(q) @ np.array([0.0, 0.6 * scale, 0.0])
        return (*(off - ax), *(off + ax), 0.3 * scale)
    if kind == AABB:
        he = np.array([0.5, 0.3, 0.4]) * scale
        return (*(off - he), *(off + he))
    if kind == OBB:
        return (*q, *off, 0.5 * scale, 0.3 * scale, 0.4 * scale)
    return (*q, *off, hull)


def ray_battery():
    """[Case]: small scenes and rays, every case tagged with its family."""
    cases = []

    def add(family, name, scene, r):
        cases.append(Case(family, name, scene, r))

    # ---- every type under a rotated, translated body, the collider with its own offset and rotation -------------------------------
    body = (np.array([2.0, -1.0, 3.0], np.float32), Q_BODY)
    for kind in range(6):
        sc = Scene([body], [(0, kind, _local_shape(kind))], [TETRA])
        centre = _world_point(body, (0.3, -0.2, 0.1))
        for k, dirn in enumerate(((1, 0.3, -0.2), (-0.4, -1, 0.5), (0.2, 0.1, 1))):
            dn = np.asarray(dirn, np.float64) / np.linalg.norm(dirn)
            add("posed-" + TYPE_NAMES[kind], "through-%d" % k, sc, ray(centre + np.array([0.05, 0.03, -0.04]) - 6 * dn, dn, 700.0 + 100 * k))
            side = np.cross(dn, (0.3, 1, 0.2)); side /= np.linalg.norm(side)
            add("posed-" + TYPE_NAMES[kind], "miss-%d" % k, sc, ray(centre + 2.5 * side - 6 * dn, dn))
        add("inside-" + TYPE_NAMES[kind], "centre", sc, ray(centre + np.array([0.02, 0.01, -0.03]), (0.3, 0.5, -0.8)))

    # ---- boxes: axis-parallel rays (1/0 = inf), origins on slab planes (0 * inf), edges and corners --------------------------------
    box = Scene([((0, 0, 0), IDENT)], [(0, AABB, (-1, -0.5, -0.75, 1, 0.5, 0.75))])
    obx = Scene([((0, 0, 0), IDENT)], [(0, OBB, (0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.75))])
    for nm, sc in (("aabb", box), ("obb", obx)):
        add("box-axis-aligned", nm + "+x", sc, ray((-5, 0.2, 0.1), (1, 0, 0), unit=False))
        add("box-axis-aligned", nm + "-y", sc, ray((0.3, 4, -0.2), (0, -1, 0), unit=False))
        add("box-axis-aligned", nm + "-z-negzero", sc, ray((0.3, 0.1, 6), (-0.0, -0.0, -1), unit=False))
        add("box-axis-aligned", nm + "+x-miss", sc, ray((-5, 0.9, 0.1), (1, 0, 0), unit=False))
        add("box-axis-aligned", nm + "away", sc, ray((-5, 0.2, 0.1), (-1, 0, 0), unit=False))
        add("parallel-box-slab-plane", nm + "-x-lo", sc, ray((-1, 3, 0.1), (0, -1, 0), unit=False))
        add("parallel-box-slab-plane", nm + "-x-hi", sc, ray((1, 3, 0.1), (0, -1, 0), unit=False))
        add("parallel-box-slab-plane", nm + "-y-lo", sc, ray((-5, -0.5, 0.1), (1, 0, 0), unit=False))
        add("parallel-box-slab-plane", nm + "-y-lo-negzero", sc, ray((-5, -0.5, 0.1), (1, -0.0, 0), unit=False))
        add("parallel-box-slab-plane", nm + "-z-hi-negzero", sc, ray((-5, 0.1, 0.75), (1, 0, -0.0), unit=False))
        add("box-on-face", nm + "-looking-in", sc, ray((-1, 0.2, 0.1), (1, 0.3, -0.2)))
        add("box-on-face", nm + "-looking-in-along-the-axis", sc, ray((0.3, 0.5, -0.2), (0, -1, 0), unit=False))
        add("box-on-face", nm + "-looking-out", sc, ray((-1, 0.2, 0.1), (-1, 0.3, -0.2)))
        add("edge-box", nm + "-along-edge", sc, ray((-5, 0.5, 0.75), (1, 0, 0), unit=False))
        add("vertex-box", nm + "-touching-corner", sc, ray((1 - 3, 0.5 + 3, 0.75), (1, -1, 0)))
        add("box-through-corner", nm + "-diagonal", sc, ray((3, 1.5, 2.25), (-1, -0.5, -0.75)))

    # ---- spheres ------------------------------------------------------------------------------------------------------------------
    sph = Scene([((1, 2, 3), IDENT)], [(0, SPHERE, (0, 0, 0, 0.5))])
    add("tangent-sphere", "grazing", sph, ray((-4, 2.5, 3), (1, 0, 0), unit=False))
    add("tangent-sphere", "just-inside", sph, ray((-4, 2.4999, 3), (1, 0, 0), unit=False))
    add("sphere", "pointing-away", sph, ray((-4, 2.1, 3), (-1, 0, 0), unit=False))
    add("sphere", "surface-looking-in", sph, ray((0.5, 2, 3), (1, 0.2, 0.1)))
    add("tangent-sphere", "surface-looking-along", sph, ray((0.5, 2, 3), (0, 1, 0), unit=False))
    add("sphere", "head-on", sph, ray((-4, 2.1, 3.2), (1, 0, 0), unit=False))

    # ---- cylinders and capsules by axis: +y (identity frame), -y (the antiparallel branch), skew ---------------------------------------
    for kind in (CYLINDER, CAPSULE):
        nm = TYPE_NAMES[kind]
        for fam, a, b in (("axis+y", (0, -0.5, 0), (0, 0.75, 0)), (ANTIPARALLEL, (0, 0.75, 0), (0, -0.5, 0)), ("axis-skew", (-0.3, -0.5, 0.2), (0.4, 0.6, -0.1))):
            sc = Scene([((0.5, 0.25, -0.5), IDENT)], [(0, kind, (*a, *b, 0.25))])
            mid = 0.5 * (np.array(a) + np.array(b)) + np.array([0.5, 0.25, -0.5])
            add(fam, nm + "-side", sc, ray(mid + np.array([-3, 0.1, 0.05]), (1, 0, 0), unit=False))
            add(fam, nm + "-oblique", sc, ray(mid + np.array([-3, 1.0, 0.6]), (3, -0.9, -0.55)))
            add(fam, nm + "-down-the-end", sc, ray(mid + np.array([0.05, 3, 0.02]), (0.01, -1, 0.0)))
            add(fam, nm + "-miss", sc, ray(mid + np.array([-3, 0.1, 0.9]), (1, 0, 0), unit=False))
    cyl = Scene([((0, 0, 0), IDENT)], [(0, CYLINDER, (0, -1, 0, 0, 1, 0, 0.5))])
    cap = Scene([((0, 0, 0), IDENT)], [(0, CAPSULE, (0, -1, 0, 0, 1, 0, 0.5))])
    add("cylinder-cap", "through-cap", cyl, ray((0.1, 3, 0.1), (0.05, -1, 0.02)))
    add("cylinder-cap", "cap-from-outside-radius", cyl, ray((1.2, 2.2, 0), (-1, -1, 0)))
    add("cylinder-cap", "along-axis", cyl, ray((0.2, 3, -0.1), (0, -1, 0), unit=False))
    add("cylinder-cap", "along-axis-from-below", cyl, ray((0.2, -3, -0.1), (0, 1, 0), unit=False))
    add("cylinder-cap", "along-axis-outside", cyl, ray((0.7, 3, 0), (0, -1, 0), unit=False))
    add("cylinder-cap", "in-through-the-rim", cyl, ray((0.5 + 2, 1 + 2, 0), (-1, -1, 0)))
    add("edge-cylinder-rim", "touching-the-rim", cyl, ray((0.5 - 2, 1 + 2, 0), (1, -1, 0)))
    add("tangent-cylinder", "side", cyl, ray((-3, 0.2, 0.5), (1, 0, 0), unit=False))
    add("cylinder-perpendicular", "dy-zero", cyl, ray((-3, 0.2, 0.1), (1, 0, 0), unit=False))
    add("cylinder-perpendicular", "dy-zero-above", cyl, ray((-3, 1.2, 0.1), (1, 0, 0), unit=False))
    add("cylinder-behind", "beyond-end-looking-away", cyl, ray((0.1, 2, 0.1), (0.05, 1, 0.02)))
    add("cylinder-behind", "capsule-beyond-end-looking-away", cap, ray((0.1, 2, 0.1), (0.05, 1, 0.02)))
    add("cylinder-behind", "inside-looking-down", cyl, ray((0.1, 0.3, 0.1), (0.05, -1, 0.02)))
    # the pose whose hit distance the reference leaves unwritten for capsules (R4): radially inside, no cap disk taken
    for nm, sc in (("cylinder", cyl), ("capsule", cap)):
        add("unwritten-t", nm + "-inside-perpendicular", sc, ray((0.125, 0.25, 0), (1, 0, 0), unit=False))
        add("unwritten-t", nm + "-beyond-end-sideways", sc, ray((0.125, 2.5, 0), (1, -0.1, 0)))
        add("unwritten-t", nm + "-beyond-end-perpendicular", sc, ray((0.125, 2.5, 0), (1, 0, 0), unit=False))
    two = Scene([((20, 0.75, 0), IDENT), ((0, 0, 0), IDENT)], [(0, SPHERE, (0, 0, 0, 0.5)), (1, CAPSULE, (0, -1, 0, 0, 1, 0, 0.5))])
    add("unwritten-t", "capsule-after-a-far-hit", two, ray((0.125, 2.5, 0), (1, -0.0875, 0)))
    add("unwritten-t", "capsule-inside-before-a-far-hit", two, ray((0.125, 0.75, 0), (1, 0, 0), unit=False))
    deg = Scene([((0, 0, 0), Q_BODY)], [(0, CAPSULE, (0.2, 0.1, -0.3, 0.2, 0.1, -0.3, 0.4))])
    c0 = _world_point(deg.bodies[0], (0.2, 0.1, -0.3))
    add("capsule-degenerate", "hit", deg, ray(c0 + np.array([-3, 0.1, 0.05]), (1, 0, 0), unit=False))
    add("capsule-degenerate", "miss", deg, ray(c0 + np.array([-3, 0.6, 0.05]), (1, 0, 0), unit=False))
    add("capsule-degenerate", "inside", deg, ray(c0 + np.array([0.1, 0.1, 0.05]), (1, 0, 0), unit=False))

    # ---- hulls ------------------------------------------------------------------------------------------------------------------------
    brick = Scene([((0, 0, 0), IDENT)], [(0, HULL, (0, 0, 0, 1, 0, 0, 0, 0))], [BRICK])
    add("edge-hull", "shared-diagonal-of-a-face", brick, ray((0.2, 0.1, 5), (0, 0, -1), unit=False))      # (x, y) on the +z face's diagonal
    add("edge-hull", "shared-edge-of-two-faces", brick, ray((1 + 2, 0.1, 0.75 + 2), (-1, 0, -1)))
    add("vertex-hull", "shared-vertex", brick, ray((1 + 2, 0.5 + 2, 0.75 + 2), (-1, -1, -1)))
    add("parallel-hull-face", "along-a-face-into-another", brick, ray((-4, 0.2, 0.3), (1, 0, 0), unit=False))
    add("parallel-hull-face", "in-a-face-plane", brick, ray((-4, 0.5, 0.3), (1, 0, 0), unit=False))
    add("hull-back-face", "from-inside", brick, ray((0.2, 0.1, -0.3), (0.3, 0.2, 1)))
    add("hull", "face-interior", brick, ray((0.6, 0.1, 5), (0, 0, -1), unit=False))
    add("hull", "pointing-away", brick, ray((0.6, 0.1, 5), (0, 0, 1), unit=False))
    both = Scene([((0, 0, 0), Q_BODY), ((3, 0.5, 0), IDENT)], [(0, HULL, (*Q_COL, 0.1, 0, 0, 0)), (1, HULL, (*IDENT, 0, 0.1, 0, 1))], [TETRA, BRICK])
    add("hull-two-geometries", "first", both, ray((-0.1, 0.1, 5), (0.02, 0, -1)))
    add("hull-two-geometries", "second", both, ray((3.2, 0.7, 5), (0, 0.01, -1)))
    add("hull-two-geometries", "through-both", both, ray((-5, 0.2, 0.1), (1, 0.05, 0)))
    add("hull-two-geometries", "second-from-behind", both, ray((9, 0.7, 0.2), (-1, 0, 0), unit=False))

    # ---- far from the origin, tiny and huge -----------------------------------------------------------------------------------------
    far = (np.array([1000.0, -1000.0, 1000.0], np.float32), Q_BODY)
    for kind in range(6):
        sc = Scene([far], [(0, kind, _local_shape(kind))], [TETRA])
        centre = _world_point(far, (0.3, -0.2, 0.1))
        add("far-1e3", TYPE_NAMES[kind], sc, ray(centre + np.array([-5, 0.1, 0.1]), (1, -0.02, -0.01)))
        for fam, scale in (("scale-1cm", 0.01), ("scale-100m", 100.0)):
            sc = Scene([body], [(0, kind, _local_shape(kind, scale))], [(TETRA[0] * np.float32(scale), TETRA[1])])
            centre = _world_point(body, np.array([0.3, -0.2, 0.1]) * scale)
            dn = np.array([1, 0.3, -0.2]) / np.linalg.norm([1, 0.3, -0.2])
            add(fam, TYPE_NAMES[kind], sc, ray(centre + scale * np.array([0.05, 0.03, -0.04]) - 6 * scale * dn, dn))

    # ---- equal distances: R8 ---------------------------------------------------------------------------------------------------------
    s1 = (0, 0, 0, 0.5)
    add("tie", "two-colliders-one-body", Scene([((0, 0, 0), IDENT)], [(0, SPHERE, s1), (0, SPHERE, s1)]), ray((-3, 0.1, 0), (1, 0, 0), unit=False))
    add("tie", "two-bodies-collider-order-reversed", Scene([((0, 0, 0), IDENT), ((0, 0, 0), IDENT)], [(1, OBB, (0, 0, 0, 1, 0, 0, 0, 0.5, 0.5, 0.5)), (0, OBB, (0, 0, 0, 1, 0, 0, 0, 0.5, 0.5, 0.5))]),
        ray((-3, 0.1, 0.2), (1, 0, 0), unit=False))
    add("tie", "three-bodies-middle-first", Scene([((0, 0, 0), Q_BODY)] * 3, [(1, CAPSULE, _local_shape(CAPSULE)), (2, CAPSULE, _local_shape(CAPSULE)), (0, CAPSULE, _local_shape(CAPSULE))]),
        ray(_world_point((np.zeros(3), Q_BODY), (0.3, -0.2, 0.1)) + np.array([-3, 0.02, 0.01]), (1, 0, 0), unit=False))
    add("order", "nearer-body-has-the-higher-collider", Scene([((0, 0, 0), IDENT), ((-1.5, 0, 0), IDENT)], [(0, SPHERE, s1), (1, SPHERE, s1)]), ray((-4, 0.1, 0), (1, 0, 0), unit=False))

    # ---- R7 ----------------------------------------------------------------------------------------------------------------------------
    line = [((0, 0, 0), IDENT), ((1.5, 0, 0), IDENT), ((3, 0, 0), IDENT)]
    add("nothing", "dead-body-in-front", Scene(line, [(0, SPHERE, s1), (1, SPHERE, s1), (2, SPHERE, s1)], dead=(0,)), ray((-4, 0.1, 0), (1, 0, 0), unit=False))
    add("nothing", "all-dead", Scene(line[:1], [(0, SPHERE, s1)], dead=(0,)), ray((-4, 0.1, 0), (1, 0, 0), unit=False))
    add("nothing", "no-colliders", Scene(line[:2], []), ray((-4, 0.1, 0), (1, 0, 0), unit=False))
    add("nothing", "disabled-ray", Scene(line[:1], [(0, SPHERE, s1)]), ray((-4, 0.1, 0), (1, 0, 0), enabled=0.0, unit=False))
    add("nothing", "body-without-colliders-in-front", Scene(line[:2], [(1, SPHERE, s1)]), ray((-4, 0.1, 0), (1, 0, 0), unit=False))
    return cases


MAX_BODIES_PER_CASE = 3


def scenes_of(cases):
    """[(scene, [case index])] in first-use order: one world serves every ray of a scene"""
    order, by_id = [], {}
    for i, c in enumerate(cases):
        if id(c.scene) not in by_id:
            by_id[id(c.scene)] = (c.scene, [])
            order.append(by_id[id(c.scene)])
        by_id[id(c.scene)][1].append(i)
    return order


def run_whole_world(cases, make_world, read_accumulators, after_cast=None):
    """Every case through a whole-world entry point (the oracle's, or the device's host entry point): one world per scene, one cast
    per case.  After each cast the accumulators it wrote are read and taken back by applying their negation (x + f - f is exactly 0),
    so every cast starts from zero.  Returns per case (pushed body or None, accumulators [6] of it, local centres of gravity [n, 3],
    what after_cast(world) returned)."""
    out = [None] * len(cases)
    for scene, idx in scenes_of(cases):
        w = make_world()
        ids = scene.instantiate(w)
        assert ids == list(range(len(ids)))
        cogs = np.array(w.mass_properties()[:, 0:3], np.float32) if ids else np.zeros((0, 3), np.float32)
        for i in idx:
            r = cases[i].ray
            pushed = w.test_physics_interaction(r[0:3], r[4:7], float(r[3])) if r[7] != 0.0 else None   # R7: a disabled ray is not cast
            extra = after_cast(w) if after_cast else None
            acc = np.zeros(6, np.float32)
            if pushed is not None:
                acc = np.array(read_accumulators(w)[pushed], np.float32)
                w.apply_force_torque(pushed, -acc[0:3], -acc[3:6])
                assert not np.any(read_accumulators(w)), "the accumulators did not return to zero"
            out[i] = (pushed, acc, cogs, extra)
        if hasattr(w, "close"):
            w.close()
    return out


def errors(case, expected, acc, t=None):
    """(t error or None, force error, torque error) in the units of BOUNDS"""
    strength = abs(float(case.ray[3]))
    et = None if t is None else abs(float(t) - expected.t) / (1 + abs(expected.t))
    ef = float(np.abs(acc[0:3].astype(np.float64) - expected.force).max()) / strength
    eq = float(np.abs(acc[3:6].astype(np.float64) - expected.torque).max()) / (strength * (1 + expected.arm))
    return et, ef, eq
