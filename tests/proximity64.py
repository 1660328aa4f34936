"""What mi_proximity (World.proximity) must report: a float64 reading of the rule of include/mi_physics.h on the float32 records, a
numpy float32 restatement of it in the operation order of csrc/point_tests.h, and the battery both are held to.

Float64: the signed distance is geom64.point_signed_distance on the collider's LOCAL record with the point brought into its frame in
float64 (a distance does not change under the pose); the closest point and the normal are written here from the geometry (closest point of
the core for spheres and capsules, the nearest face plane inside a polytope, projection or nearest edge outside), not from point_tests.h.
Every candidate also reports a branch margin: how far the point is from the place where the rule switches expression (inside / outside,
cap against side, the box axis, the hull's plane tie, the hull's closest-triangle tie, the centre where unit(0) = 0).

A case is CLEAR if every margin (d against the radius, best against second best, the winner's branch margin) is at least CLEAR_MARGIN
of its scale (1 + |d|, resp. the shape's size).  The rest are ties by construction (Case.tie names the reason and what still has to
hold) or undecided; classify() raises when an undecided case is outside the edge / vertex / tie families or when they exceed 15 %."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g64  # noqa: E402
import ray64 as r64  # noqa: E402
from raycast_util import CastWorld, STATIC_BODY, ZONE_NONE  # noqa: E402

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
TYPE_NAMES = g64.TYPE_NAMES
CLEAR_MARGIN = 1e-4
UNDECIDED_CAP = 0.15
UNDECIDED_FAMILIES = ("edge", "vertex", "tie")
F32_EPS = 2.0 ** -23
# float32 restatement against float64 on the clear cases of the battery, per family (collider type, "@1e3" for coordinates of 1e3 m):
# (distance error / (1 + |d|), closest point error / (1 + |p|), normal angle in radians).  Measured by test_proximity64_cpu.py, which
# holds this table to its measurement within 1.5 x either way; the device's tolerance is max(4 x figure, 4 float32 ulps).
E_F32 = {
    "aabb": (6.6e-08, 4.1e-08, 2.2e-07),
    "aabb@1e3": (7e-08, 3.7e-08, 6.7e-08),
    "capsule": (3.7e-08, 4.9e-08, 4.8e-07),
    "capsule@1e3": (7.9e-08, 4.8e-08, 2.5e-07),
    "cylinder": (6e-08, 4.3e-08, 1.1e-07),
    "cylinder@1e3": (4e-08, 3.4e-08, 7.3e-07),
    "hull": (1.3e-07, 2.9e-08, 2.1e-07),
    "hull@1e3": (1e-07, 3.6e-08, 7.5e-08),
    "obb": (1.2e-07, 3.5e-08, 3.8e-07),
    "obb@1e3": (1.4e-07, 3e-08, 3.3e-07),
    "sphere": (1.1e-07, 8.5e-08, 1.4e-07),
    "sphere@1e3": (2.2e-07, 4.7e-08, 8.8e-08),
}


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# Float64
# ---------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    n = float(np.linalg.norm(v))
    return v / n if n > 0 else np.zeros(3)


def _closest_on_triangle64(p, a, b, c):
    n = np.cross(b - a, c - a); n = n / np.linalg.norm(n)
    q = p - np.dot(p - a, n) * n
    if all(np.dot(np.cross(v - u, q - u), n) >= 0 for u, v in ((a, b), (b, c), (c, a))):
        return q
    cands = [g64._closest_on_segments(p, u, v) for u, v in ((a, b), (b, c), (c, a))]
    return min(cands, key=lambda x: float(np.linalg.norm(p - x)))


_shapes = {}


def local64(ctype, shape10, hulls, p):
    """(d, c, n, branch margin, size) of the point p (float64, collider frame) against the LOCAL record."""
    s = _f64(shape10)
    key = (ctype, np.asarray(shape10, np.float32).tobytes(), id(hulls))
    if key not in _shapes:
        _shapes[key] = g64.shape_from_record({"type": ctype, "shape": np.asarray(shape10, np.float32)}, hulls)
    shape = _shapes[key]
    d = float(g64.point_signed_distance(shape, p[None])[0])
    size = shape.size
    if ctype in (SPHERE, CAPSULE):
        q = s[0:3] if ctype == SPHERE else g64._closest_on_segments(p, s[0:3], s[3:6])
        r = s[3] if ctype == SPHERE else s[6]
        v = p - q
        n = _unit(v)
        return d, q + r * n, n, float(np.linalg.norm(v)), size
    if ctype == CYLINDER:
        a, b, r = s[0:3], s[3:6], s[6]
        h = float(np.linalg.norm(b - a)); u = (b - a) / h
        y = float(np.dot(p - a, u)); rho = (p - a) - y * u; l = float(np.linalg.norm(rho))
        dax, drad = abs(y - 0.5 * h) - 0.5 * h, l - r
        if dax <= 0 and drad <= 0:
            margin = min(abs(dax - drad), -min(max(dax, drad), 0.0) if max(dax, drad) < 0 else 0.0)
            if dax > drad:
                top = y > 0.5 * h
                return d, (p + (h - y) * u if top else p - y * u), (u if top else -u), min(margin, abs(y - 0.5 * h)), size
            n = _unit(rho)
            return d, a + y * u + r * n, n, min(margin, l), size
        c = a + min(max(y, 0.0), h) * u + (r * _unit(rho) if l > r else rho)
        return d, c, _unit(p - c), abs(d), size
    tri = shape.triangles()
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    planes = ((p[None] - tri[:, 0]) * nrm).sum(axis=1)
    f = int(np.argmax(planes))
    if planes[f] <= 0:
        other = planes[np.abs(nrm @ nrm[f] - 1.0) > 1e-9]       # planes of another face (a box face is two triangles)
        margin = min(-planes[f], float(planes[f] - other.max()) if len(other) else math.inf)
        return d, p - planes[f] * nrm[f], nrm[f], margin, size
    pts = np.array([_closest_on_triangle64(p, *t) for t in tri])
    dist = np.linalg.norm(p[None] - pts, axis=1)
    k = int(np.argmin(dist))
    elsewhere = dist[np.linalg.norm(pts - pts[k], axis=1) > 1e-9 * (1.0 + size)]   # (the same point through a shared edge is no tie)
    margin = min(abs(d), float(elsewhere.min() - dist[k]) if len(elsewhere) else math.inf)
    return d, pts[k], _unit(p - pts[k]), margin, size


def candidates(cw, static=True, poses=None, dead=()):
    """[(collider, body | STATIC_BODY, type, shape10, pos, rot)] of a CastWorld, the bodies at poses [n, 7] if given."""
    out = []
    for i, c in enumerate(cw.colliders):
        if c["zone"] != ZONE_NONE:
            continue
        if c["body"] is None:
            if static:
                out.append((i, STATIC_BODY, c["type"], c["shape"], c["pos"], c["rot"]))
        elif c["body"] not in cw.dead and c["body"] not in dead:
            p, q = cw.bodies[c["body"]] if poses is None else (poses[c["body"], 0:3], poses[c["body"], 3:7])
            out.append((i, c["body"], c["type"], c["shape"], p, q))
    return out


class Reading:
    def __init__(self):
        self.found, self.collider, self.body, self.d, self.point, self.normal, self.within = False, None, None, 0.0, np.zeros(3), np.zeros(3), 0
        self.type = None
        self.margin_radius = self.margin_gap = self.margin_branch = math.inf   # relative to their scales

    @property
    def margin(self):
        return min(self.margin_radius, self.margin_gap, self.margin_branch)

    @property
    def clear(self):
        return self.margin >= CLEAR_MARGIN


def expect(cw, point, radius, cands, hulls=None, exclude=(0, 0)):
    """The float64 reading of one world-space query against the candidates."""
    e = Reading()
    p, radius = _f64(point), float(radius)
    if not radius >= 0.0:
        return e
    hits = []
    for col, body, ctype, shape10, pos, rot in cands:
        if body != STATIC_BODY and ((body - exclude[0]) & 0xFFFFFFFF) < exclude[1]:
            continue
        R = g64.quat_to_matrix(_f64(rot))
        d, c, n, branch, size = local64(ctype, shape10, cw.hulls if hulls is None else hulls, R.T @ (p - _f64(pos)))
        if math.isfinite(radius):
            e.margin_radius = min(e.margin_radius, abs(d - radius) / (1.0 + abs(d)))
        if d <= radius:
            hits.append((d, col, body, R @ c + _f64(pos), R @ n, branch / size, ctype))
    if not hits:
        return e
    hits.sort(key=lambda h: (h[0], h[1]))
    e.found, e.within = True, len(hits)
    e.d, e.collider, e.body, e.point, e.normal, e.margin_branch, e.type = hits[0]
    if len(hits) > 1:
        e.margin_gap = (hits[1][0] - hits[0][0]) / (1.0 + abs(hits[0][0]))
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# Float32 in the order of csrc/point_tests.h (numpy float32 scalars: every operation rounds once)
# ---------------------------------------------------------------------------------------------------------------------------
f = np.float32


def _v(x):
    return np.asarray(x, f)


def _dot(a, b):
    return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))


def _cross(a, b):
    return _v([f(f(a[1] * b[2]) - f(a[2] * b[1])), f(f(a[2] * b[0]) - f(a[0] * b[2])), f(f(a[0] * b[1]) - f(a[1] * b[0]))])


def _len(a):
    return f(np.sqrt(_dot(a, a)))


def _unit32(a):
    l = _len(a)
    return _v(a / l) if l > 0 else np.zeros(3, f)


def _qmul(a, b):
    w = f(f(a[3] * b[3]) - _dot(a[0:3], b[0:3]))
    v = _v(_v(_v(a[0:3] * b[3]) + _v(b[0:3] * a[3])) + _cross(a[0:3], b[0:3]))
    return _v([v[0], v[1], v[2], w])


def _conj(q):
    return _v([-q[0], -q[1], -q[2], q[3]])


def _rot(q, v):
    return _qmul(_qmul(q, _v([v[0], v[1], v[2], 0])), _conj(q))[0:3]


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _sphere32(p, ce, r):
    v = _v(p - ce)
    n = _unit32(v)
    return f(_len(v) - r), _v(ce + _v(r * n)), n


def _capsule32(p, a, b, r):
    ab = _v(b - a)
    den = _dot(ab, ab)
    s = _clamp(f(_dot(_v(p - a), ab) / den), f(0), f(1)) if den > 0 else f(0)
    return _sphere32(p, _v(a + _v(s * ab)), r)


def _cylinder32(p, a, b, r):
    u = _unit32(_v(b - a))
    h, pa = _len(_v(b - a)), _v(p - a)
    y = _dot(pa, u)
    rho = _v(pa - _v(y * u))
    l = _len(rho)
    hh = f(h * f(0.5))
    dax, drad = f(f(abs(f(y - hh))) - hh), f(l - r)
    if dax <= 0 and drad <= 0:
        if dax > drad:
            top = y > hh
            return dax, (_v(p + _v(f(h - y) * u)) if top else _v(p - _v(y * u))), (u if top else _v(-u))
        n = _unit32(rho)
        return drad, _v(_v(a + _v(y * u)) + _v(r * n)), n
    c = _v(_v(a + _v(_clamp(y, f(0), h) * u)) + (_v(r * _unit32(rho)) if l > r else rho))
    v = _v(p - c)
    return _len(v), c, _unit32(v)


def _box32(p, lo, hi):
    ce, e = _v(_v(lo + hi) * f(0.5)), _v(_v(hi - lo) * f(0.5))
    q = _v(p - ce)
    w = _v(np.abs(q) - e)
    if np.all(w <= 0):
        k = 0
        if w[1] > w[k]: k = 1
        if w[2] > w[k]: k = 2
        s = f(-1) if q[k] < 0 else f(1)
        n = np.zeros(3, f); n[k] = s
        c = p.copy(); c[k] = f(ce[k] + f(s * e[k]))
        return w[k], c, n
    c = _v(ce + _v([_clamp(q[i], f(-e[i]), e[i]) for i in range(3)]))
    v = _v(p - c)
    return _len(v), c, _unit32(v)


def _closest_on_triangle32(p, a, b, c, n):
    ab, ac, ap = _v(b - a), _v(c - a), _v(p - a)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    if d1 <= 0 and d2 <= 0: return a
    bp = _v(p - b)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    if d3 >= 0 and d4 <= d3: return b
    vc = f(f(d1 * d4) - f(d3 * d2))
    if vc <= 0 and d1 >= 0 and d3 <= 0: return _v(a + _v(f(d1 / f(d1 - d3)) * ab))
    cp = _v(p - c)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    if d6 >= 0 and d5 <= d6: return c
    vb = f(f(d5 * d2) - f(d1 * d6))
    if vb <= 0 and d2 >= 0 and d6 <= 0: return _v(a + _v(f(d2 / f(d2 - d6)) * ac))
    va = f(f(d3 * d6) - f(d5 * d4))
    if va <= 0 and f(d4 - d3) >= 0 and f(d5 - d6) >= 0: return _v(b + _v(f(f(d4 - d3) / f(f(d4 - d3) + f(d5 - d6))) * _v(c - b)))
    return _v(p - _v(_dot(ap, n) * n))


def _hull32(p, verts, tris):
    plane, dist, plane_n, close = f(-np.inf), f(np.inf), np.zeros(3, f), p
    for t in tris:
        a, b, c = _v(verts[t[0]]), _v(verts[t[1]]), _v(verts[t[2]])
        n = _unit32(_cross(_v(b - a), _v(c - a)))
        pl = _dot(_v(p - a), n)
        if pl > plane: plane, plane_n = pl, n
        cf = _closest_on_triangle32(p, a, b, c, n)
        df = _len(_v(p - cf))
        if df < dist: dist, close = df, cf
    if plane <= 0:
        return plane, _v(p - _v(plane * plane_n)), plane_n
    return dist, close, _unit32(_v(p - close))


def local32(ctype, s, hulls, p):
    s, p = _v(s), _v(p)
    if ctype == SPHERE: return _sphere32(p, s[0:3], s[3])
    if ctype == CAPSULE: return _capsule32(p, s[0:3], s[3:6], s[6])
    if ctype == CYLINDER: return _cylinder32(p, s[0:3], s[3:6], s[6])
    if ctype == AABB: return _box32(p, s[0:3], s[3:6])
    q, ce = s[0:4], s[4:7]
    lp = _rot(_conj(q), _v(p - ce))
    if ctype == OBB:
        d, c, n = _box32(lp, _v(np.zeros(3, f) - s[7:10]), s[7:10])
    else:
        v, t = hulls[int(s[7])]
        d, c, n = _hull32(lp, np.asarray(v, f), t)
    return d, _v(_rot(q, c) + ce), _rot(q, n)


def world32(ctype, shape10, hulls, pos, rot, point):
    """(d, c, n) in world space as pxTestCollider forms them."""
    pos, rot, point = _v(pos), _v(rot), _v(point)
    d, c, n = local32(ctype, shape10, hulls, _rot(_conj(rot), _v(point - pos)))
    return d, _v(_rot(rot, c) + pos), _rot(rot, n)


def mount32(pos, rot, local):
    """the world point of a mounted query as k_proximity's head forms it"""
    return _v(_rot(_v(rot), _v(local)) + _v(pos))


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(math.atan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


# ---------------------------------------------------------------------------------------------------------------------------
# The battery
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """family/name; the world-space point and radius; tie: None, or (reason, winner collider | None = nothing found, fields that still
    have to match float64: a subset of "distance", "point", "normal", "within")."""

    def __init__(self, family, name, point, radius, tie=None):
        self.family, self.name, self.point, self.radius, self.tie = family, name, np.asarray(point, np.float32), np.float32(radius), tie

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)


def _surface(cw, col, centre, u, hi):
    """the point where the ray centre + t u leaves collider col (float64 bisection on the signed distance)"""
    c = cw.colliders[col]
    pos, rot = (c["pos"], c["rot"]) if c["body"] is None else cw.bodies[c["body"]]
    R = g64.quat_to_matrix(_f64(rot))
    sd = lambda t: local64(c["type"], c["shape"], cw.hulls, R.T @ (centre + t * u - _f64(pos)))[0]
    lo = 0.0
    assert sd(lo) < 0 < sd(hi), (col, sd(lo), sd(hi))
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if sd(mid) < 0 else (lo, mid)
    return centre + hi * u


def _centre_local(ctype, s):
    s = _f64(s)
    return {SPHERE: s[0:3], CAPSULE: 0.5 * (s[0:3] + s[3:6]), CYLINDER: 0.5 * (s[0:3] + s[3:6]), AABB: 0.5 * (s[0:3] + s[3:6]), OBB: s[4:7], HULL: s[4:7]}[ctype]


_battery = None


def battery():
    """(CastWorld, [Case]): every case has a collider of its own, 50 m from the next (30 m shapes 300 m), on bodies posed by ray64.Q_BODY."""
    global _battery
    if _battery is not None:
        return _battery
    cw = CastWorld()
    geoms = {1.0: (cw.add_hull(*r64.TETRA), cw.add_hull(*r64.BRICK))}
    for scale in (0.01, 30.0):
        geoms[scale] = (cw.add_hull(r64.TETRA[0] * np.float32(scale), r64.TETRA[1]), cw.add_hull(r64.BRICK[0] * np.float32(scale), r64.BRICK[1]))
    cases = []
    slot = [0]
    dirs = [np.array(d, np.float64) / np.linalg.norm(d) for d in ((1, 0.3, -0.2), (-0.4, 1, 0.5), (0.2, -0.6, -1))]

    def place(kind, scale=1.0, base=0.0, hull=0, shape=None, offset=(0.3, -0.2, 0.1)):
        k = slot[0]; slot[0] += 1
        pitch = 300.0 if scale > 10 else 50.0
        pos = np.array([base + pitch * (k % 12), base + (600.0 if scale > 10 else 0.0), base + pitch * (k // 12)])
        b = cw.add_body(pos, r64.Q_BODY)
        s = shape if shape is not None else r64._local_shape(kind, scale=scale, offset=offset, hull=geoms[scale if scale in geoms else 1.0][hull])
        col = cw.add_collider(b, kind, s)
        centre = r64._world_point(cw.bodies[b], _centre_local(kind, cw.colliders[col]["shape"]))
        return col, centre

    def radius_for(scale):
        return 4.0 * scale + 1.0

    for kind in range(6):
        name = TYPE_NAMES[kind]
        for scale, base, tag in ((1.0, 0.0, ""), (0.01, 0.0, "-1cm"), (30.0, 0.0, "-30m"), (1.0, 1e3, "@1e3"), (1.0, -1e3, "@-1e3")):
            col, centre = place(kind, scale, base, hull=(kind + int(scale)) % 2)
            reach = 3.0 * scale
            for j, u in enumerate(dirs if tag == "" else dirs[:1]):
                surf = _surface(cw, col, centre, u, reach)
                t = float(np.linalg.norm(surf - centre))
                cases.append(Case("outside" + tag, "%s-%d" % (name, j), centre + (t + 0.7 * scale) * u, radius_for(scale)))
                cases.append(Case("inside" + tag, "%s-%d" % (name, j), centre + 0.55 * t * u, radius_for(scale)))
                if j == 0:
                    cases.append(Case("tie-surface" + tag, name, surf, radius_for(scale), tie=("the point is within an ulp of the surface: the distance is decided, the normal of unit(p - c) is not", col, ("distance", "point", "within"))))
            if tag == "":
                cases.append(Case("tie-centre", name, centre, radius_for(scale), tie=("at the centre several faces or directions are equally near", col, ("distance", "within"))))
                cases.append(Case("radius-inf", name, centre + 2.0 * dirs[1], np.inf))
                cases.append(Case("radius-short", name, centre + 2.5 * dirs[2], 0.5))
                cases.append(Case("radius-negative", name, centre, -0.01, tie=("a negative radius finds nothing, also inside a shape", None, ())))
    # beyond a cylinder's rim, a box corner, a hull vertex and edge
    for kind in (CYLINDER, AABB, OBB, HULL):
        col, centre = place(kind, 1.0, 0.0, hull=1)
        c = cw.colliders[col]
        body = cw.bodies[c["body"]]
        s = _f64(c["shape"])
        if kind == CYLINDER:
            a, b, r = s[0:3], s[3:6], s[6]
            u = (b - a) / np.linalg.norm(b - a)
            side = np.cross(u, [0.3, 0.1, 0.9]); side /= np.linalg.norm(side)
            cases.append(Case("edge-rim", "cylinder-above", r64._world_point(body, b + 0.3 * u + (r + 0.4) * side), 3.0))
            cases.append(Case("edge-rim", "cylinder-below", r64._world_point(body, a - 0.2 * u + (r + 0.1) * side), 3.0))
            cases.append(Case("edge-rim", "cylinder-on", r64._world_point(body, b + r * side), 3.0))
            cases.append(Case("tie-cap-side", "cylinder", r64._world_point(body, b - 0.1 * u + (r - 0.1) * side), 3.0,
                              tie=("cap and side are equally near: the distance is decided, which of the two is reported is not", col, ("distance", "within"))))
        elif kind == AABB:
            lo, hi = s[0:3], s[3:6]
            cases.append(Case("vertex-corner", "aabb", r64._world_point(body, hi + [0.3, 0.2, 0.4]), 3.0))
            cases.append(Case("edge-box", "aabb", r64._world_point(body, np.array([hi[0] + 0.3, 0.5 * (lo[1] + hi[1]), lo[2] - 0.2])), 3.0))
            cases.append(Case("vertex-corner", "aabb-on", r64._world_point(body, hi), 3.0))
            cases.append(Case("tie-axis", "aabb", r64._world_point(body, hi - 0.1), 3.0, tie=("three faces are equally near", col, ("distance", "within"))))
        elif kind == OBB:
            Rq = g64.quat_to_matrix(s[0:4])
            cases.append(Case("vertex-corner", "obb", r64._world_point(body, s[4:7] + Rq @ (s[7:10] + [0.3, 0.2, 0.4])), 3.0))
            cases.append(Case("edge-box", "obb", r64._world_point(body, s[4:7] + Rq @ (np.array([s[7] + 0.3, 0.0, -s[9] - 0.2]))), 3.0))
            cases.append(Case("vertex-corner", "obb-on", r64._world_point(body, s[4:7] + Rq @ s[7:10]), 3.0))
        else:
            Rq = g64.quat_to_matrix(s[0:4])
            v = _f64(cw.hulls[int(s[7])][0])
            cases.append(Case("vertex-hull", "brick", r64._world_point(body, s[4:7] + Rq @ (1.4 * v[6])), 3.0))
            cases.append(Case("vertex-hull", "brick-on", r64._world_point(body, s[4:7] + Rq @ v[6]), 3.0))
            mid = 0.5 * (v[5] + v[6])
            cases.append(Case("edge-hull", "brick", r64._world_point(body, s[4:7] + Rq @ (mid + 0.5 * mid / np.linalg.norm(mid))), 3.0))
            cases.append(Case("edge-hull", "brick-on", r64._world_point(body, s[4:7] + Rq @ mid), 3.0))
            cases.append(Case("tie-plane", "brick", r64._world_point(body, s[4:7] + Rq @ (v[6] - 0.1)), 3.0, tie=("three face planes are equally near", col, ("distance", "within"))))
    # capsules with a == b
    for k, off in enumerate(((0.3, -0.2, 0.1), (0.0, 0.0, 0.0))):
        col, centre = place(CAPSULE, shape=(*off, *off, 0.4))
        cases.append(Case("degenerate-capsule", "outside-%d" % k, centre + 0.9 * dirs[k], 3.0))
        cases.append(Case("degenerate-capsule", "inside-%d" % k, centre + 0.1 * dirs[k], 3.0))
    # exact ties between two colliders: one record twice on one body; two static boxes mirrored about the point
    k = slot[0]; slot[0] += 2
    pos = np.array([50.0 * (k % 12), 0.0, 50.0 * (k // 12)])
    b = cw.add_body(pos, r64.Q_BODY)
    first = cw.add_collider(b, SPHERE, (0.1, 0.2, -0.1, 0.5)); cw.add_collider(b, SPHERE, (0.1, 0.2, -0.1, 0.5))
    reason = ("two colliders at exactly the same distance: the lowest index wins", first, ("distance", "point", "normal", "within"))
    cases.append(Case("tie-colliders", "same-record", pos + [1.0, 0.5, 0.25], 3.0, tie=reason))
    pos2 = pos + [50.0, 0.0, 0.0]
    left = cw.add_static(AABB, (1, -1, -1, 2, 1, 1), pos=pos2); cw.add_static(AABB, (-2, -1, -1, -1, 1, 1), pos=pos2)
    cases.append(Case("tie-colliders", "mirrored", pos2, 3.0, tie=("two colliders at exactly the same distance: the lowest index wins", left, ("distance", "point", "normal", "within"))))
    # radius 0 on a surface (exact in float32: face at x = 1 of a box centred at 1.5), just short of it, and inside with radius 0
    cases.append(Case("tie-radius-zero", "on-face", pos2 + [1.0, 0.0, 0.0], 0.0, tie=("d is exactly 0 = radius: within", left, ("distance", "point", "within"))))
    cases.append(Case("radius-zero", "inside", pos2 + [1.75, 0.25, 0.0], 0.0))
    cases.append(Case("radius-zero", "off-face", pos2 + [0.5, 0.0, 0.0], 0.0))
    _battery = (cw, cases)
    return _battery


_expected = None


def battery_expected():
    """[Reading] of the battery's cases in float64 against every candidate of its world, computed once."""
    global _expected
    if _expected is None:
        cw, cases = battery()
        cands = candidates(cw)
        _expected = [expect(cw, c.point, c.radius, cands) for c in cases]
    return _expected


def classify():
    """(clear, ties, undecided): indices into the battery.  Raises on an undecided case outside the edge / vertex / tie families, on a tie
    whose stated winner float64 contradicts, and when the undecided exceed the cap."""
    cw, cases = battery()
    clear, ties, undecided = [], [], []
    for i, (c, e) in enumerate(zip(cases, battery_expected())):
        if c.tie is not None:
            assert (c.tie[1] is None and not e.found) or (e.found and abs(e.d - _tie_distance(cw, c, e)) <= 1e-5 * (1 + abs(e.d))), (c.id, e.found, e.collider)
            ties.append(i)
        elif e.clear:
            clear.append(i)
        else:
            if not c.family.startswith(UNDECIDED_FAMILIES):
                raise AssertionError("undecided outside the knife-edge families: %s (margins %g %g %g)" % (c.id, e.margin_radius, e.margin_gap, e.margin_branch))
            undecided.append(i)
    if len(undecided) > UNDECIDED_CAP * len(cases):
        raise AssertionError("%d of %d cases undecided" % (len(undecided), len(cases)))
    return clear, ties, undecided


def _tie_distance(cw, case, e):
    """float64 distance of the tie's stated winner (it must be as near as float64's own winner)"""
    col = [c for c in candidates(cw) if c[0] == case.tie[1]][0]
    R = g64.quat_to_matrix(_f64(col[5]))
    return local64(col[2], col[3], cw.hulls, R.T @ (_f64(case.point) - _f64(col[4])))[0]


def family_of(case, reading):
    """the E_F32 key: the winner's type, "@1e3" for coordinates of 1e3 m"""
    return TYPE_NAMES[reading.type] + ("@1e3" if float(np.abs(case.point).max()) > 500.0 else "")


def errors(reading, d, point, normal):
    """(distance error / (1 + |d|), point error / (1 + |p|), normal angle) of a float32 answer against the float64 reading"""
    return (abs(float(d) - reading.d) / (1.0 + abs(reading.d)),
            float(np.linalg.norm(np.asarray(point, np.float64) - reading.point)) / (1.0 + float(np.linalg.norm(reading.point))),
            angle(normal, reading.normal))


def measure_f32():
    """{family: (distance, point, normal)} the worst float32 restatement error over the clear cases"""
    cw, cases = battery()
    clear, _, _ = classify()
    cands = {c[0]: c for c in candidates(cw)}
    out = {}
    for i in clear:
        c, e = cases[i], battery_expected()[i]
        if not e.found:
            continue
        _, _, ctype, shape10, pos, rot = cands[e.collider]
        got = errors(e, *world32(ctype, shape10, cw.hulls, pos, rot, c.point))
        fam = family_of(c, e)
        out[fam] = tuple(max(a, b) for a, b in zip(out.get(fam, (0.0, 0.0, 0.0)), got))
    return out


def tolerance(family):
    return tuple(max(4.0 * v, 4.0 * F32_EPS) for v in E_F32[family])
