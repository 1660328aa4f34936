"""What mi_sphere_cast_batch (World.sphere_cast) must report: a float64 reading of what the rule of include/mi_physics.h MEANS (not of
its iteration), a numpy float32 restatement of the iteration in the operation order of csrc/sphere_cast.h, and the battery both are
held to.

Float64: for one candidate the gap g(t) = dist64(o + t v) - radius, with geom64.point_signed_distance on the collider's LOCAL record
and the cast brought into its frame in float64, is convex in t.  The reading is the first t* in [0, maxT] with g(t*) = 0, found by
bracketing the minimum of g and then its first root on grids that shrink 16-fold per round, to 1e-12; the contact normal there
(proximity64.local64) and cos(theta*) = -n.v / L; and the least clearance min g over the path for a cast that never touches.  For a
world: the smallest t*, of equal t* the lowest collider index.

Decision margins (the device stops where g <= tol, so its t is t* - tol / (L cos(theta*)) .. t* in exact arithmetic):
  hit       cos(theta*) >= COS_MIN, maxT at least CLEAR_MARGIN (in metres of path) beyond t*, and every other candidate clear of the path
            up to there by more than tol + CLEAR_MARGIN
  miss      the least clearance of every candidate over the path exceeds tol by CLEAR_MARGIN (proximity64's margin)
  inside    g(0) <= -CLEAR_MARGIN for the winner (the lowest collider index that overlaps), every lower index clear by tol + CLEAR_MARGIN
  undecided everything else; at most UNDECIDED_CAP of the battery
COS_MIN = 0.05: at shallower incidence tol / (L cos) exceeds 2 mm of path and the device's slope test meets a g that is flat to within
its rounding; the battery's graze family sits below it on purpose and is what the undecided share consists of."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g64  # noqa: E402
import proximity64 as p64  # noqa: E402
import ray64 as r64  # noqa: E402
from raycast_util import CastWorld, STATIC_BODY  # noqa: E402

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
TYPE_NAMES = g64.TYPE_NAMES
SC_GAP = 1e-4
SC_GUARD_ULPS = 16.0
SC_MAX_ITER = 32
F32_EPS = p64.F32_EPS
COS_MIN = 0.05
CLEAR_MARGIN = p64.CLEAR_MARGIN
UNDECIDED_CAP = p64.UNDECIDED_CAP
UNDECIDED_FAMILIES = ("graze", "near-miss", "touch")
# float32 restatement against float64 on the decided hits of the battery, per family (collider type, "@1e3" for coordinates of 1e3 m,
# "/r0" for radius 0, where the normal is the unit vector of a difference of SC_GAP's length):
#   t       how far t leaves [t* - tol / (L cos), t*], in metres of path, / (1 + |origin| + t* L)
#   point   closest point against float64 AT THE RESTATEMENT'S OWN t, / (1 + |c|)
#   normal  angle against float64 at that t, radians
#   gap     against float64 at that t, / (1 + |origin| + t* L)
# Measured by test_spherecast64_cpu.py, which holds this table to its measurement within 1.5 x either way; the device's tolerance is
# max(4 x figure, 4 float32 ulps).
E_F32 = {
    "aabb": (3.4e-09, 4.9e-08, 2.1e-06, 3.8e-09),
    "aabb/r0": (2.1e-09, 4.8e-08, 3e-08, 1.6e-09),
    "aabb@1e3": (5.7e-09, 2.9e-08, 3e-08, 8.8e-10),
    "capsule": (3.5e-09, 3.6e-08, 1e-06, 8.4e-09),
    "capsule/r0": (2.1e-09, 3.5e-08, 1e-06, 5.3e-09),
    "capsule@1e3": (0, 3.3e-08, 1.2e-06, 7.1e-09),
    "cylinder": (1.6e-09, 3.7e-08, 1.8e-06, 4e-09),
    "cylinder/r0": (8.1e-10, 3.2e-08, 0.0012, 1.2e-09),
    "cylinder@1e3": (0, 3.3e-08, 4.2e-06, 2e-09),
    "hull": (8.3e-10, 2.6e-08, 1.7e-06, 1.3e-09),
    "hull/r0": (3.1e-10, 2.8e-08, 6.5e-08, 5.1e-10),
    "hull@1e3": (2.1e-09, 2.5e-08, 2e-07, 3.6e-09),
    "obb": (9.5e-10, 2.4e-08, 9.6e-07, 1.7e-09),
    "obb/r0": (1.5e-10, 3e-08, 6.5e-08, 1.5e-09),
    "obb@1e3": (1.5e-10, 3.5e-08, 5.9e-07, 8.9e-09),
    "sphere": (7.3e-08, 1.3e-07, 9.1e-07, 8.2e-08),
    "sphere/r0": (2.3e-08, 1.5e-07, 6.6e-07, 1.7e-08),
    "sphere@1e3": (5.5e-09, 3e-08, 1.1e-06, 1.4e-09),
}
# The most samples one candidate took in the restatement: over the battery, and over 10 000 seeded random casts (measure_iterations).
MAX_ITER_BATTERY, MAX_ITER_RANDOM = 12, 11

_f64 = p64._f64


# ---------------------------------------------------------------------------------------------------------------------------
# Float64
# ---------------------------------------------------------------------------------------------------------------------------
class Cand:
    """one candidate collider: index, reported body, type, LOCAL record, pose (float64), its geom64 shape and a ball that holds it"""

    def __init__(self, idx, body, ctype, shape10, pos, rot, hulls):
        self.idx, self.body, self.type, self.shape10, self.hulls = idx, body, ctype, np.asarray(shape10, np.float32), hulls
        self.pos, self.rot, self.R = _f64(pos), _f64(rot), g64.quat_to_matrix(_f64(rot))
        self.shape = g64.shape_from_record({"type": ctype, "shape": self.shape10}, hulls)
        self.ball = math.sqrt(3.0) * self.shape.size
        self.centre_w = self.pos + self.R @ self.shape.center

    def local(self, O, D):
        return self.R.T @ (O - self.pos), self.R.T @ D

    def gap(self, o, v, radius, ts):
        ts = np.atleast_1d(np.asarray(ts, np.float64))
        return g64.point_signed_distance(self.shape, o[None] + ts[:, None] * v[None]) - radius

    def contact(self, o, v, t):
        """(d, c, n) in WORLD space of the centre o + t v (local)"""
        d, c, n, _, _ = p64.local64(self.type, self.shape10, self.hulls, o + t * v)
        return d, self.R @ c + self.pos, self.R @ n


_cands = {}


def candidates(cw, static=True, poses=None, dead=()):
    """[Cand] of a CastWorld (proximity64.candidates with the shapes prepared), cached for the described poses"""
    key = (id(cw), static, len(cw.colliders), tuple(sorted(cw.dead)), tuple(sorted(dead))) if poses is None else None
    if key is not None and key in _cands:
        return _cands[key]
    out = [Cand(i, b, t, s, p, q, cw.hulls) for i, b, t, s, p, q in p64.candidates(cw, static, poses, dead)]
    if key is not None:
        _cands[key] = out
    return out


def tol64(len_o, t, L, radius):
    return SC_GAP + SC_GUARD_ULPS * F32_EPS * (len_o + t * L + radius)


class One:
    """one candidate's reading: t (None: never touches within maxT), g0 = g(0), clearance = min g over the path, cos, tol at the stop"""
    t = None; g0 = 0.0; clearance = math.inf; cos = 0.0; tol = SC_GAP; n = None


def _refine(f, lo, hi, pick, rounds=12, k=33):
    for _ in range(rounds):
        ts = np.linspace(lo, hi, k)
        j = pick(f(ts))
        lo, hi = ts[max(j - 1, 0)], ts[min(j + 1, k - 1)]
    return lo, hi


def candidate64(c, O, D, radius, max_t, rounds=12, root=True):
    """The reading of one candidate: the first root of the convex g on [0, max_t].  root=False: only whether it touches (t is then some
    t with g <= 0) and the clearance, the minimum bracketed in `rounds` rounds."""
    o, v = c.local(O, D)
    L, len_o = float(np.linalg.norm(D)), float(np.linalg.norm(o))
    r = One()
    r.g0 = r.clearance = float(c.gap(o, v, radius, 0.0)[0])
    r.tol = tol64(len_o, 0.0, L, radius)
    if r.g0 <= 0.0:
        r.t = 0.0
        return r
    if L == 0.0:
        return r
    tc = float(np.dot(c.shape.center - o, v)) / (L * L)           # g has its minimum within ball / L of the closest approach to the centre
    hi = min(float(max_t), max(tc, 0.0) + c.ball / L)
    if not hi > 0.0:
        return r
    f = lambda ts: c.gap(o, v, radius, ts)
    lo_m, hi_m = _refine(f, 0.0, hi, lambda g: int(np.argmin(g)), rounds)
    tm = 0.5 * (lo_m + hi_m)
    gm = float(f(tm)[0])
    r.tol = tol64(len_o, tm, L, radius)
    if gm > 0.0:
        gs = f(np.array([lo_m, tm, hi_m]))
        r.clearance = float(gs.min())
        return r
    if not root:
        r.t, r.clearance = tm, 0.0
        return r
    first = lambda g: int(np.argmax(g <= 0.0))                     # g > 0 at 0 and <= 0 at tm: the first grid point at or below 0
    lo_r, hi_r = _refine(f, 0.0, tm, first)
    r.t = hi_r
    r.clearance = 0.0
    r.tol = tol64(len_o, r.t, L, radius)
    _, _, n = c.contact(o, v, r.t)
    r.n = n
    r.cos = float(-np.dot(n, D)) / L
    return r


class Reading:
    def __init__(self):
        self.kind, self.t, self.collider, self.body, self.type, self.cos, self.tol, self.L, self.why = "miss", None, None, None, None, 0.0, SC_GAP, 0.0, ""
        self.cand = None

    @property
    def decided(self):
        return self.kind != "undecided"


def _near(c, O, D, reach, radius):
    """may the path (a segment of length `reach` from O along D, or the point O) come within radius + 1 m of the candidate's ball?"""
    L = float(np.linalg.norm(D))
    rel = c.centre_w - O
    s = 0.0 if L == 0.0 else min(max(float(rel @ D) / (L * L), 0.0), reach / L if math.isfinite(reach) else math.inf)
    return float(np.linalg.norm(rel - s * D)) <= c.ball + radius + 1.0


def expect(cands, origin, direction, radius, max_t, exclude=(0, 0)):
    """The float64 reading of one world-space cast against the candidates, with its decision."""
    e = Reading()
    O, D, radius, max_t = _f64(origin), _f64(direction), float(np.float32(radius)), float(np.float32(max_t))
    e.L = L = float(np.linalg.norm(D))
    if not radius >= 0.0 or not max_t >= 0.0:
        return e
    if math.isinf(radius):
        e.kind, e.why = "undecided", "an infinite radius overlaps everything"
        return e
    ones = []
    for c in cands:
        if c.body != STATIC_BODY and ((c.body - exclude[0]) & 0xFFFFFFFF) < exclude[1]:
            continue
        if _near(c, O, D, max_t * L if L > 0 else 0.0, radius):
            ones.append((c, candidate64(c, O, D, radius, max_t)))
    touching = [(c, r) for c, r in ones if r.t == 0.0]
    if touching or L == 0.0:
        # t = 0: the lowest index that overlaps; anything of a lower index must be clear of the origin
        open_ = [(c, r) for c, r in ones if r.g0 <= r.tol + CLEAR_MARGIN]
        if not open_:
            return e
        if not touching or open_[0][0].idx != touching[0][0].idx or touching[0][1].g0 > -CLEAR_MARGIN:
            e.kind, e.why = "undecided", "a candidate within the margins of touching at the origin"
            if touching:
                e.t, e.collider, e.body, e.type, e.cand = 0.0, touching[0][0].idx, touching[0][0].body, touching[0][0].type, touching[0][0]
            return e
        c, r = touching[0]
        e.kind, e.t, e.collider, e.body, e.type, e.tol, e.cand = "inside", 0.0, c.idx, c.body, c.type, r.tol, c
        return e
    hits = sorted(((r.t, c.idx, c, r) for c, r in ones if r.t is not None), key=lambda h: (h[0], h[1]))
    if not hits:
        if any(r.clearance <= r.tol + CLEAR_MARGIN for _, r in ones):
            e.kind, e.why = "undecided", "a candidate passes within the margin"
        return e
    t, _, c, r = hits[0]
    e.kind, e.t, e.collider, e.body, e.type, e.cos, e.tol, e.cand = "hit", t, c.idx, c.body, c.type, r.cos, r.tol, c
    if r.cos < COS_MIN:
        e.kind, e.why = "undecided", "incidence shallower than COS_MIN"
    elif (max_t - t) * L < CLEAR_MARGIN:
        e.kind, e.why = "undecided", "maxT within the margin of t*"
    else:
        upto = t + CLEAR_MARGIN / L
        for c2, r2 in ones:
            if c2 is c:
                continue
            r3 = candidate64(c2, O, D, radius, upto)
            if r3.t is not None or r3.clearance <= r3.tol + CLEAR_MARGIN:
                e.kind, e.why = "undecided", "another candidate nearly as early"
                break
    return e


def at(c, origin, direction, radius, t):
    """float64 (gap, closest point, normal) in world space of candidate c with the sphere's centre at origin + t direction"""
    o, v = c.local(_f64(origin), _f64(direction))
    d, cw_, n = c.contact(o, v, float(t))
    return d - float(np.float32(radius)), cw_, n


# ---------------------------------------------------------------------------------------------------------------------------
# Float32 in the order of csrc/sphere_cast.h and of k_spherecast.hip's leaf (numpy float32 scalars: every operation rounds once)
# ---------------------------------------------------------------------------------------------------------------------------
f = np.float32
MISS, HIT, UNRESOLVED, BEATEN = range(4)
_v, _len, _rot, _conj = p64._v, p64._len, p64._rot, p64._conj
_GUARD = f(f(SC_GUARD_ULPS) * f(1.1920929e-7))


def _tol32(len_o, t, L, radius):
    return f(f(SC_GAP) + f(_GUARD * f(f(len_o + f(t * L)) + radius)))


def march32(ctype, shape10, hulls, o, v, L, radius, max_t, beyond=f(np.inf)):
    """sphereCastCollider: (hit, t, gap, c, n, iterations) in the collider's frame"""
    o, v, L, radius, max_t = _v(o), _v(v), f(L), f(radius), f(max_t)
    len_o = _len(o)
    t = t_prev = g_prev = f(0)
    hit, out = MISS, None
    with np.errstate(all="ignore"):
        for it in range(SC_MAX_ITER):
            d, c, n = p64.local32(ctype, shape10, hulls, _v(o + _v(t * v)))
            g = f(d - radius)
            out = (t, g, c, n, it + 1)
            if g <= _tol32(len_o, t, L, radius):
                hit = HIT
                break
            if not L > 0:
                break
            step = f(g / L)
            if it > 0:
                slope = f(f(g - g_prev) / f(t - t_prev))
                if slope >= 0:
                    break
                chord = f(f(-g) / slope)
                step = chord if (chord > step or step != step) else step      # fmaxf
            t_prev, g_prev = t, g
            t = f(t + step)
            if not t <= max_t:
                break
            if t > beyond:
                hit = BEATEN
                break
        else:
            hit = UNRESOLVED
    return (hit,) + out


def cast32(cw, cand_list, origin, direction, radius, max_t, exclude=(0, 0)):
    """The leaf of k_spherecast.hip over the candidates [Cand] in index order (brute force): None, or
    (hit, t, collider, body, point, gap, normal, iterations); the second value is the most samples any candidate took."""
    O, D, radius, max_t = _v(origin), _v(direction), f(radius), f(max_t)
    L = _len(D)
    best, most = None, 0
    if not (radius >= 0 and max_t >= 0):
        return None, 0
    for c in cand_list:
        if c.body != STATIC_BODY and ((c.body - exclude[0]) & 0xFFFFFFFF) < exclude[1]:
            continue
        pos, rot = _v(c.pos), _v(c.rot)
        o, v = _rot(_conj(rot), _v(O - pos)), _rot(_conj(rot), D)
        hit, t, g, cl, n, its = march32(c.type, c.shape10, cw.hulls, o, v, L, radius, max_t, f(np.inf) if best is None else best[1])
        most = max(most, its)
        if hit in (HIT, UNRESOLVED) and (best is None or t < best[1] or (t == best[1] and c.idx < best[2])):
            best = (hit, t, c.idx, c.body, _v(_rot(rot, cl) + pos), g, _rot(rot, n), its)
    return best, most


def mount32(pos, rot, origin, direction):
    """the world cast of a mounted query as k_sphere_cast's head forms it"""
    return _v(_rot(_v(rot), _v(origin)) + _v(pos)), _rot(_v(rot), _v(direction))


angle = p64.angle


# ---------------------------------------------------------------------------------------------------------------------------
# The battery
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, name, origin, direction, radius, max_t=np.inf):
        self.family, self.name = family, name
        self.origin, self.direction, self.radius, self.max_t = np.asarray(origin, np.float32), np.asarray(direction, np.float32), np.float32(radius), np.float32(max_t)

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _perp(u, hint=(0.3, 0.1, 0.9)):
    return _unit(np.cross(u, hint))


def _graze_offset(c, centre, u, w, radius, reach):
    """the offset h along w at which the line centre + h w + s u just touches the candidate's surface inflated by radius (bisection on the
    least clearance, which grows with h beyond the shape)"""
    def clearance(h):
        r = candidate64(c, centre + h * w + reach * u, -u, radius, 2.0 * reach, rounds=6, root=False)
        return -1.0 if r.t is not None else r.clearance
    lo, hi = 0.0, 4.0 * c.ball + radius
    assert clearance(lo) <= 0 < clearance(hi)
    for _ in range(30):                      # to 1e-8 m: the families' offsets from it are 2e-4 m and more
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if clearance(mid) <= 0 else (lo, mid)
    return hi


_battery = None


def battery():
    """(CastWorld, [Case]): every target collider on a body of its own posed by ray64.Q_BODY, 50 m from the next (30 m shapes 300 m)."""
    global _battery
    if _battery is not None:
        return _battery
    cw = CastWorld()
    geoms = {1.0: (cw.add_hull(*r64.TETRA), cw.add_hull(*r64.BRICK))}
    for scale in (0.01, 30.0):
        geoms[scale] = (cw.add_hull(r64.TETRA[0] * np.float32(scale), r64.TETRA[1]), cw.add_hull(r64.BRICK[0] * np.float32(scale), r64.BRICK[1]))
    cases, slot = [], [0]
    dirs = [_unit(d) for d in ((1, 0.3, -0.2), (-0.4, 1, 0.5), (0.2, -0.6, -1))]

    def place(kind, scale=1.0, base=0.0, hull=0):
        k = slot[0]; slot[0] += 1
        pitch = 300.0 if scale > 10 else 50.0
        pos = np.array([base + pitch * (k % 12), base + (600.0 if scale > 10 else 0.0), base + pitch * (k // 12)])
        b = cw.add_body(pos, r64.Q_BODY)
        col = cw.add_collider(b, kind, r64._local_shape(kind, scale=scale, hull=geoms[scale][hull]))
        rec = cw.colliders[col]
        return Cand(col, b, kind, rec["shape"], cw.bodies[b][0], cw.bodies[b][1], cw.hulls)

    def add(family, name, origin, direction, radius, max_t=np.inf):
        cases.append(Case(family, name, origin, direction, radius, max_t))
        return cases[-1]

    def t_star(c, case):
        r = candidate64(c, _f64(case.origin), _f64(case.direction), float(case.radius), float(case.max_t))
        assert r.t is not None and r.t > 0, case.id
        return r.t

    for kind in range(6):
        name = TYPE_NAMES[kind]
        c = place(kind, hull=kind % 2)
        centre, far = c.centre_w, 4.0
        for j, u in enumerate(dirs[:2]):
            add("head-on", "%s-%d" % (name, j), centre + far * u, -u, 0.3)
        u, w = dirs[0], _perp(dirs[0])
        radius = 0.2
        h0 = _graze_offset(c, centre, u, w, radius, far)
        for family, h in (("oblique", h0 - 0.3 * (radius + 0.3)), ("graze", h0 - 2e-4), ("past", h0 + 0.02)):
            add(family, name, centre + h * w + far * u, -u, radius)
        for depth in (0.02, 0.04, 0.08, 0.16):       # shallow: the first of these depths at which the incidence is decided with room to spare
            cos = candidate64(c, centre + (h0 - depth) * w + far * u, -u, radius, math.inf).cos
            if cos >= 3.0 * COS_MIN:
                break
        add("shallow", name, centre + (h0 - depth) * w + far * u, -u, radius)
        if kind % 2 == 0:
            add("near-miss", name, centre + (h0 + 1.5e-4) * w + far * u, -u, radius)
        add("inside", name, centre, dirs[1], 0.2, 10.0)
        # in touch at the origin: the surface point along dirs[2], the sphere's centre radius - 3e-4 (inside the margin: decided) or
        # radius + 5e-5 (between the margins: the rule hits at 0 or after 5e-5 m; undecided) off it
        surf = p64._surface(cw, c.idx, centre, dirs[2], 3.0)
        _, _, n = at(c, surf + 1e-3 * dirs[2], dirs[2], 0.0, 0.0)
        add("touch" if kind % 2 else "inside-touch", name, surf + (0.25 + (5e-5 if kind % 2 else -3e-4)) * n, -n, 0.25, 10.0)
        add("radius-zero", name + "-head-on", centre + far * dirs[2], -dirs[2], 0.0)
        add("radius-zero", name + "-oblique", centre + 0.5 * h0 * w + far * u, -u, 0.0)
        head = add("max-t", name + "-inf", centre + far * dirs[2], -dirs[2], 0.15)
        ts = t_star(c, head)
        add("max-t", name + "-short", head.origin, head.direction, 0.15, ts - 2e-3)
        add("max-t", name + "-beyond", head.origin, head.direction, 0.15, ts + 1e-3)
        add("zero-direction", name + ("-inside" if kind % 2 else "-outside"), centre if kind % 2 else centre + far * u, (0, 0, 0), 0.2)
        add("non-unit", name + "-long", centre + far * dirs[1], -2.5 * dirs[1], 0.1)
        add("non-unit", name + "-short", centre + far * dirs[1], -0.01 * dirs[1], 0.1, 1e4)
        add("receding", name, centre + 1.5 * dirs[0], dirs[0], 0.2)
    # past an edge and past a vertex of the three polytopes: along the box's own x axis, offset along y (the entry face's edge) or along
    # the y-z diagonal (its corner)
    for kind in (AABB, OBB, HULL):
        c = place(kind, hull=1)
        name = TYPE_NAMES[kind]
        Rs = c.R if kind == AABB else c.R @ g64.quat_to_matrix(_f64(c.shape10[0:4]))
        u = -Rs[:, 0]
        for feature, w in (("edge", Rs[:, 1]), ("vertex", _unit(Rs[:, 1] + Rs[:, 2]))):
            h0 = _graze_offset(c, c.centre_w, u, w, 0.2, 4.0)
            add("past-" + feature, name + "-hit", c.centre_w + (h0 - 0.08) * w + 4.0 * u, -u, 0.2)
            add("past-" + feature, name + "-miss", c.centre_w + (h0 + 0.02) * w + 4.0 * u, -u, 0.2)
    # 1 cm and 30 m shapes, coordinates of +- 1e3
    for kind in range(6):
        name = TYPE_NAMES[kind]
        for scale, base, tag in ((0.01, 0.0, "-1cm"), (30.0, 0.0, "-30m"), (1.0, 1e3, "@1e3"), (1.0, -1e3, "@-1e3")):
            c = place(kind, scale, base, hull=(kind + int(scale)) % 2)
            far, radius = 4.0 * scale + 1.0, 0.3 * min(scale, 1.0) + (0.05 if scale < 1 else 0.0)
            add("head-on" + tag, name, c.centre_w + far * dirs[1], -dirs[1], radius)
            u, w = dirs[0], _perp(dirs[0])
            h0 = _graze_offset(c, c.centre_w, u, w, radius, far)
            add("oblique" + tag, name, c.centre_w + (h0 - 0.3 * (radius + 0.3 * scale)) * w + far * u, -u, radius)
    # a huge sphere: 40 m of radius towards a 30 m shape from 200 m (the battery's other colliders are farther than that from its path),
    # and one that swallows its target at the origin
    for kind in (SPHERE, OBB, HULL):
        c = place(kind, 30.0, 0.0, hull=1)
        add("huge-radius", TYPE_NAMES[kind], c.centre_w + 200.0 * dirs[1], -dirs[1], 40.0)
        add("huge-radius", TYPE_NAMES[kind] + "-swallowed", c.centre_w + 20.0 * dirs[1], -dirs[1], 100.0, 5.0)
    _battery = (cw, cases)
    return _battery


_expected = None


def battery_expected():
    """[Reading] of the battery's cases in float64 against every candidate of its world, computed once."""
    global _expected
    if _expected is None:
        cw, cases = battery()
        cands = candidates(cw)
        _expected = [expect(cands, c.origin, c.direction, c.radius, c.max_t) for c in cases]
    return _expected


def classify():
    """{kind: [indices into the battery]}.  Raises on an undecided case outside the knife-edge families and when they exceed the cap."""
    cw, cases = battery()
    out = {"hit": [], "miss": [], "inside": [], "undecided": []}
    for i, (c, e) in enumerate(zip(cases, battery_expected())):
        out[e.kind].append(i)
        if e.kind == "undecided" and not c.family.startswith(UNDECIDED_FAMILIES):
            raise AssertionError("undecided outside the knife-edge families: %s (%s)" % (c.id, e.why))
    if len(out["undecided"]) > UNDECIDED_CAP * len(cases):
        raise AssertionError("%d of %d cases undecided" % (len(out["undecided"]), len(cases)))
    return out


def family_of(case, reading):
    """the E_F32 key: the winner's type, "@1e3" for coordinates of 1e3 m, "/r0" for a radius of 0"""
    return TYPE_NAMES[reading.type] + ("@1e3" if float(np.abs(case.origin).max()) > 500.0 else "") + ("/r0" if case.radius == 0 else "")


def scale_of(case, reading):
    return 1.0 + float(np.abs(case.origin).max()) + reading.t * reading.L


def t_window(reading):
    """[lo, hi]: where the rule stops in exact arithmetic, t* - tol / (L cos(theta*)) .. t*"""
    return reading.t - reading.tol / (reading.L * reading.cos), reading.t


def errors(case, reading, t, point, normal, gap):
    """(t, point, normal, gap) errors of a float32 answer on the reading's collider, in E_F32's units"""
    lo, hi = t_window(reading)
    s = scale_of(case, reading)
    g, c, n = at(reading.cand, case.origin, case.direction, case.radius, float(t))
    return (max(float(t) - hi, lo - float(t), 0.0) * reading.L / s,
            float(np.linalg.norm(np.asarray(point, np.float64) - c)) / (1.0 + float(np.linalg.norm(c))),
            angle(normal, n), abs(float(gap) - g) / s)


_restated = None


def battery_restated():
    """[(cast32 answer | None, most samples)] of the battery in float32, each case against the candidates its path comes near"""
    global _restated
    if _restated is None:
        cw, cases = battery()
        cands = candidates(cw)
        _restated = []
        for c in cases:
            O, D = _f64(c.origin), _f64(c.direction)
            L = float(np.linalg.norm(D))
            near = [k for k in cands if _near(k, O, D, float(c.max_t) * L if L > 0 else 0.0, float(c.radius))]
            _restated.append(cast32(cw, near, c.origin, c.direction, c.radius, c.max_t))
    return _restated


def measure_f32():
    """{family: (t, point, normal, gap)} the worst float32 restatement error over the decided hits"""
    cw, cases = battery()
    out = {}
    for i in classify()["hit"]:
        c, e, (got, _) = cases[i], battery_expected()[i], battery_restated()[i]
        assert got is not None and got[2] == e.collider, (c.id, got)
        err = errors(c, e, got[1], got[4], got[6], got[5])
        fam = family_of(c, e)
        out[fam] = tuple(max(a, b) for a, b in zip(out.get(fam, (0.0,) * 4), err))
    return out


def tolerance(family):
    return tuple(max(4.0 * v, 4.0 * F32_EPS) for v in E_F32[family])


def random_casts(n, seed=20261020):
    """(CastWorld, [Cand], origins, directions, radii, max_t): n seeded casts, each aimed near one collider of raycast_util.random_world"""
    from raycast_util import random_world
    cw, _ = random_world()
    cands = candidates(cw)
    rng = np.random.default_rng(seed)
    O, D, R, T = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    target = rng.integers(0, len(cands), n)
    for i in range(n):
        c = cands[target[i]]
        u = _unit(rng.normal(size=3))
        R[i] = rng.choice([0.0, 0.05, 0.3, 1.0])
        aim = c.centre_w + _unit(rng.normal(size=3)) * rng.uniform(0.0, 1.2) * (c.shape.size + R[i])     # from dead centre to just past the rim
        O[i] = aim + u * rng.uniform(0.5, 30.0)
        D[i] = -u * rng.choice([1.0, 1.0, 0.1, 7.0])
        T[i] = np.inf if i % 4 else rng.uniform(1.0, 40.0)
    return cw, cands, target, O, D, R, T


def measure_iterations(n=10000):
    """the most samples sphereCastCollider takes, float32 restatement: (over the battery, over n random casts against their target)"""
    worst_b = max(m for _, m in battery_restated())
    cw, cands, target, O, D, R, T = random_casts(n)
    worst_r = 0
    for i in range(n):
        _, m = cast32(cw, [cands[target[i]]], O[i], D[i], R[i], T[i])
        worst_r = max(worst_r, m)
    return worst_b, worst_r
