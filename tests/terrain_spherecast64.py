"""What mi_sphere_cast_batch with MI_SPHERE_TERRAIN (World.sphere_cast(terrain=True)) must report for the heightmap terrain alone: a
float64 reading of what the rule of include/mi_physics.h MEANS (not of its iteration), a numpy float32 restatement of the triangle march
in the operation order of csrc/terrain_point.h on csrc/sphere_cast.h, and the battery both are held to.

Float64: the terrain is the sheet of terrain_ray64.Terrain.triangles(); G(t) = min_f |(o + t v) - c_f| - radius.  The reading is the
first t* in [0, maxT] with G(t*) = 0.  Each g_f is convex in t and 1-Lipschitz in path length, so: advance t by G / 2L (no root is
passed, and between two samples G stays above half the smaller of them) until G <= TRACE_NEAR; every triangle with a root in the next
WINDOW metres of path then has g_f <= TRACE_NEAR + WINDOW now, and for each of those the first root of its convex g_f is bracketed
(minimum, then first sign change, on grids that shrink 16-fold per round, spherecast64._refine); the smallest root wins.  If none has a
root in the window the advance goes on behind it.  The contact normal is unit(centre - c) at t*, cos(theta*) = -n.v / L.

Decision margins are spherecast64's (the device stops where g <= tol, so its t is t* - tol / (L cos) .. t* in exact arithmetic):
  hit       cos(theta*) >= COS_MIN and maxT at least CLEAR_MARGIN (metres of path) beyond t*
  miss      half the smallest G sampled along the path exceeds tol + CLEAR_MARGIN
  touch     G(0) <= -CLEAR_MARGIN: in touch at the origin, t = 0
  undecided everything else (incidence shallower than COS_MIN, maxT or the origin's gap within the margins)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spherecast64 as s64  # noqa: E402
import terrain_prox64 as tp  # noqa: E402
import terrain_ray64 as t64  # noqa: E402
from terrain_ray64 import CELLS, F32_EPS  # noqa: E402

SC_GAP, SC_MAX_ITER, COS_MIN, CLEAR_MARGIN = s64.SC_GAP, s64.SC_MAX_ITER, s64.COS_MIN, s64.CLEAR_MARGIN
TRACE_NEAR, WINDOW = 1e-3, 0.05
MISS, HIT, UNRESOLVED, BEATEN = s64.MISS, s64.HIT, s64.UNRESOLVED, s64.BEATEN
# float32 restatement against float64 on the decided hits of the battery, per family, in spherecast64.E_F32's units:
#   t       how far t leaves [t* - tol / (L cos), t*], metres of path, / (1 + |origin| + t* L)
#   point   closest point of the winning triangle against float64 AT THE RESTATEMENT'S OWN t, / (1 + |c|)
#   normal  angle against float64 at that t, radians, x |centre - c| / (1 + |origin| + t* L): the unit vector of a difference of that length
#   gap     against float64 at that t, / (1 + |origin| + t* L)
# Measured by test_terrain_spherecast64_cpu.py, which holds this table to its measurement within 1.5 x either way; the device's
# tolerance is max(4 x figure, 4 float32 ulps).
E_F32 = {
    "along-ground": (5.1e-08, 4.5e-08, 4.2e-08, 2.5e-08),
    "drop-face": (7.8e-09, 1.8e-07, 1.3e-07, 1.6e-08),
    "drop-ridge-peak": (1.4e-08, 4.8e-08, 5.1e-08, 1.5e-08),
    "far": (2.3e-08, 4e-08, 4.3e-08, 2.9e-08),
    "far/r0": (1.5e-08, 3.2e-08, 1.4e-08, 3.4e-08),
    "from-below": (0.0, 7.5e-08, 6.3e-08, 1.7e-08),
    "from-below/r0": (0.0, 3.3e-08, 6.4e-09, 1.6e-08),
    "from-outside": (3.3e-08, 1e-07, 1.4e-08, 6.9e-09),
    "max-t": (8.9e-09, 7.2e-08, 3.3e-08, 2e-08),
    "non-unit": (3e-08, 5.7e-08, 4.1e-08, 2.3e-08),
    "radius-zero": (2.2e-08, 4.6e-08, 2.8e-08, 1.3e-08),
    "slanted": (4.2e-08, 9e-08, 7.8e-08, 3e-08),
    "through-hole": (5.1e-09, 1.3e-07, 3.1e-08, 6.5e-09),
}
# The most samples one triangle took in the restatement: over the battery, and over 10 000 seeded random casts on the scene's layout
# (measure_iterations(10000): 2 749 of them hit, none unresolved).  SC_MAX_ITER = 32 holds with the same room it has for colliders (12 / 11).
MAX_ITER_BATTERY, MAX_ITER_RANDOM = 9, 11


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
def _path_triangles(T, O, D, radius, t_end, pad):
    """indices of the triangles whose cell, in x / z, lies within radius + pad of the path's segment [0, t_end] (or of the point O)"""
    tri = T.triangles()
    P0, P1 = O[[0, 2]], (O + t_end * D)[[0, 2]]
    cx, cz = 0.5 * (tri["x0"] + tri["x1"]), 0.5 * (tri["z0"] + tri["z1"])
    C = np.stack([cx, cz], 1)
    seg = P1 - P0
    ll = float(seg @ seg)
    s = np.clip(((C - P0[None]) @ seg) / ll, 0.0, 1.0) if ll > 0 else np.zeros(len(C))
    dist = np.linalg.norm(C - (P0[None] + s[:, None] * seg[None]), axis=1)
    return np.flatnonzero(dist <= radius + pad + T.cell)


class Sheet:
    """the triangles a cast can meet, and G over them"""

    def __init__(self, T, idx):
        tri = T.triangles()
        self.a, self.b, self.c, self.n, self.id = tri["a"][idx], tri["b"][idx], tri["c"][idx], tri["n"][idx], tri["id"][idx]

    def gaps(self, centre, radius):
        cf = tp.closest_on_triangles64(centre, self.a, self.b, self.c)
        return np.linalg.norm(centre[None] - cf, axis=1) - radius, cf

    def contact(self, centre, radius):
        """(gap, closest point, normal) of the sheet at a centre"""
        g, cf = self.gaps(centre, radius)
        k = int(np.argmin(g))
        w = centre - cf[k]
        ln = float(np.linalg.norm(w))
        return float(g[k]), cf[k], (w / ln if ln > 0 else self.n[k])


class Reading:
    def __init__(self):
        self.kind, self.t, self.cos, self.tol, self.L, self.why, self.sheet, self.g0, self.clearance = "miss", None, 0.0, SC_GAP, 0.0, "", None, math.inf, math.inf

    @property
    def decided(self):
        return self.kind != "undecided"


def _reach(T, O, D, radius, max_t):
    """the part [0, t_end] of the path on which the sphere can touch the terrain's box at all (None: never)"""
    lo, hi = T.box()
    lo, hi = lo - (radius + 1.0), hi + (radius + 1.0)
    t0, t1 = 0.0, float(max_t)
    for k in range(3):
        if D[k] == 0.0:
            if O[k] < lo[k] or O[k] > hi[k]:
                return None
        else:
            a, b = (lo[k] - O[k]) / D[k], (hi[k] - O[k]) / D[k]
            t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return (t0, t1) if t0 <= t1 else None


ZERO = 1e-9   # a gap this small counts as a root: with radius 0 a g_f only touches 0 (a tangency), it never goes below


def _first_root(f, lo, hi):
    """first t in [lo, hi] with the convex f <= ZERO, given f(lo) > ZERO; None if it stays above"""
    lo_m, hi_m = s64._refine(f, lo, hi, lambda g: int(np.argmin(g)))
    tm = 0.5 * (lo_m + hi_m)
    if float(f(np.array([tm]))[0]) > ZERO:
        return None
    _, hi_r = s64._refine(f, lo, tm, lambda g: int(np.argmax(g <= ZERO)))
    return hi_r


def expect(T, origin, direction, radius, max_t):
    """The float64 reading of one world-space cast against the terrain alone, with its decision"""
    e = Reading()
    O, D = np.asarray(origin, np.float32).astype(np.float64), np.asarray(direction, np.float32).astype(np.float64)
    radius, max_t = float(np.float32(radius)), float(np.float32(max_t))
    e.L = L = float(np.linalg.norm(D))
    if not radius >= 0.0 or not max_t >= 0.0 or not (np.isfinite(O).all() and np.isfinite(D).all() and math.isfinite(radius)):
        return e
    len_o = float(np.linalg.norm(O))
    span = _reach(T, O, D, radius, max_t) if L > 0 else (0.0, 0.0)
    if span is None:
        return e
    t_begin, t_end = span
    idx = _path_triangles(T, O, D, radius, t_end, 1.0)
    if not len(idx):
        return e
    sheet = e.sheet = Sheet(T, idx)
    g0 = float(sheet.gaps(O, radius)[0].min())
    e.g0, e.tol = g0, s64.tol64(len_o, 0.0, L, radius)
    if g0 <= e.tol + CLEAR_MARGIN or L == 0.0:
        if g0 <= -CLEAR_MARGIN:
            e.kind, e.t = "touch", 0.0
        elif g0 <= e.tol + CLEAR_MARGIN:
            e.kind, e.why = "undecided", "the origin's gap is within the margins of touching"
            e.t = 0.0 if g0 <= 0 else None
        return e
    t, least = 0.0, g0
    while t <= t_end:
        g, _ = sheet.gaps(O + t * D, radius)
        G = float(g.min())
        least = min(least, G)
        if G > TRACE_NEAR:
            t += G / (2.0 * L)
            continue
        stop = min(t + WINDOW / L, t_end)
        roots = []
        for k in np.flatnonzero(g <= TRACE_NEAR + WINDOW + 1e-9):
            a, b, c = sheet.a[k:k + 1], sheet.b[k:k + 1], sheet.c[k:k + 1]

            def f(ts, a=a, b=b, c=c):
                return np.array([np.linalg.norm(O + s * D - tp.closest_on_triangles64(O + s * D, a, b, c)[0]) - radius for s in np.atleast_1d(ts)])
            r = _first_root(f, t, stop) if g[k] > ZERO else t
            if r is not None:
                roots.append(r)
        if roots:
            e.t = min(roots)
            break
        t = stop + 1e-9 / L
        if stop >= t_end:
            break
    e.clearance = least
    if e.t is None:
        e.tol = s64.tol64(len_o, t_end if math.isfinite(t_end) else 0.0, L, radius)
        if 0.5 * least <= e.tol + CLEAR_MARGIN:
            e.kind, e.why = "undecided", "the sheet passes within the margin"
        return e
    e.kind = "hit"
    e.tol = s64.tol64(len_o, e.t, L, radius)
    _, _, n = sheet.contact(O + e.t * D, radius)
    e.cos = float(-np.dot(n, D)) / L
    if e.cos < COS_MIN:
        e.kind, e.why = "undecided", "incidence shallower than COS_MIN"
    elif (max_t - e.t) * L < CLEAR_MARGIN:
        e.kind, e.why = "undecided", "maxT within the margin of t*"
    return e


def t_window(e):
    return e.t - e.tol / (e.L * e.cos), e.t


# ---- float32 in the order of csrc/terrain_point.h on csrc/sphere_cast.h ----------------------------------------------------------------
f = np.float32
_v, _len, _unit32 = tp._v, tp._len, tp._unit32


def march32(a, b, c, o, v, L, radius, max_t, beyond=f(np.inf)):
    """sphereCastMarch with TpTriangleDistance: (hit, t, gap, c, n, iterations)"""
    o, v, L, radius, max_t = _v(o), _v(v), f(L), f(radius), f(max_t)
    len_o = _len(o)
    t = t_prev = g_prev = f(0)
    hit, out = MISS, None
    with np.errstate(all="ignore"):
        for it in range(SC_MAX_ITER):
            p = _v(o + _v(t * v))
            nf, cf, d = tp.triangle32(p, a, b, c)
            w = _v(p - cf)
            n = _unit32(w) if _len(w) > 0 else nf
            g = f(d - radius)
            out = (t, g, cf, n, it + 1)
            if g <= s64._tol32(len_o, t, L, radius):
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


def cast_ids(T, origin, direction, radius, max_t):
    """ids of the triangles a float32 cast can stop on or be bounded by: those of the float64 sheet (cell within radius + 1 m of the path)
    that come within radius + 0.05 m of the path before the float64 first contact + 0.05 m.  The restatement over these is the restatement
    over all: every other triangle's march misses or is beaten."""
    e = expect(T, origin, direction, radius, max_t)
    if e.sheet is None:
        return e, np.zeros(0, np.int64)
    O, D = np.asarray(origin, np.float32).astype(np.float64), np.asarray(direction, np.float32).astype(np.float64)
    L = e.L
    upto = (e.t if e.t is not None else 0.0) + (0.05 / L if L > 0 else 0.0)
    keep = np.zeros(len(e.sheet.id), bool)
    n = max(int(upto * L / (0.25 * T.cell)) + 2, 2) if L > 0 else 1
    for s in np.linspace(0.0, upto, n):
        g, _ = e.sheet.gaps(O + s * D, float(np.float32(radius)))
        keep |= g <= 0.05 + 0.25 * T.cell
    return e, e.sheet.id[keep]


def cast32(T, origin, direction, radius, max_t, ids, beyond=f(np.inf)):
    """k_sc_terrain's answer over the triangles `ids` in id order: (None | (hit, t, point, gap, normal, iterations, id), most samples)"""
    O, D, radius, max_t = _v(origin), _v(direction), f(radius), f(max_t)
    if not (radius >= 0 and max_t >= 0) or not (np.isfinite(O).all() and np.isfinite(D).all() and np.isfinite(radius)):
        return None, 0
    L = _len(D)
    best, best_t, most = None, f(beyond), 0
    for tid in sorted(int(i) for i in ids):
        a, b, c = tp.vertices32(T, tid)[0:3]
        hit, t, g, cf, n, its = march32(a, b, c, O, D, L, radius, max_t, best_t)
        most = max(most, its)
        if hit in (HIT, UNRESOLVED) and t < best_t:              # ids ascend: of equal t the lowest id stays; a collider's t (beyond) stays too
            best, best_t = (hit, t, cf, g, n, its, tid), t
    return best, most


# ---- the battery -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, layout, family, origin, direction, radius, max_t=np.inf):
        self.layout, self.family = layout, family
        self.origin, self.direction, self.radius, self.max_t = np.asarray(origin, np.float32), np.asarray(direction, np.float32), np.float32(radius), np.float32(max_t)


FAMILIES = ("drop-face", "drop-ridge-peak", "slanted", "along-ground", "from-below", "through-hole", "touch", "max-t", "radius-zero", "zero-direction", "non-unit", "from-outside", "far")
KNIFE_EDGE = ("along-ground", "touch")


def _battery_of(name, T, rng, families=FAMILIES):
    out = []
    cell, n = T.cell, T.cpd * CELLS
    x0, z0, y0 = float(T.corner[0]), float(T.corner[2]), float(T.corner[1])
    top = y0 + float(T.amplitude)

    def add(family, origin, direction, radius, max_t=np.inf):
        if family in families:
            out.append(Case(name, family, origin, direction, radius, max_t))

    def pick(family, make):
        """the first of 12 fresh draws whose float64 reading is decided (terrain_prox64._battery_of.pick)"""
        if family not in families:
            return
        for attempt in range(12):
            args = make()
            if expect(T, *(args + (np.inf,))[:4]).decided or attempt == 11:
                return add(family, *args)

    def interior(margin=3.0):
        while True:
            gx, gz = int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1))
            if all(T.height(gx + dx, gz + dz) is not None and not T.near_rim(*T.vertex_xz(gx + dx, gz + dz), margin, margin) for dx in (0, 1) for dz in (0, 1)):
                return gx, gz

    def unit(v):
        v = np.asarray(v, np.float64)
        return v / np.linalg.norm(v)

    peaks = tp._local_extrema(T, +1, 32, rng)
    for k in range(8):
        pick("drop-face", lambda: ((x0 + (interior()[0] + 0.3) * cell, top + 1.0, z0 + (interior()[1] + 0.25) * cell), (0.0, -1.0, 0.0), (0.1, 0.35, 0.8, 1.5)[k % 4]))
    for k in range(8):
        def make():
            gx, gz = peaks[int(rng.integers(len(peaks)))]
            off = ((0.0, 0.0), (0.3, 0.0), (0.0, -0.4), (0.2, 0.2))[k % 4]
            return (x0 + (gx + off[0]) * cell, top + 0.5, z0 + (gz + off[1]) * cell), (0.0, -2.0, 0.0), (0.05, 0.3)[k % 2]
        pick("drop-ridge-peak", make)
    for k in range(10):
        def make():
            gx, gz = interior()
            az = rng.uniform(0, 2 * math.pi)
            return (x0 + (gx + 0.4) * cell, top + rng.uniform(0.3, 2.0), z0 + (gz + 0.6) * cell), unit((math.cos(az), -(1.0, 0.5, 0.25)[k % 3], math.sin(az))), (0.1, 0.4, 1.0)[k % 3]
        pick("slanted", make)
    for k in range(6):                                                    # nearly along the ground: shallow incidence, some undecided by construction
        gx, gz = interior()
        az = rng.uniform(0, 2 * math.pi)
        add("along-ground", (x0 + (gx + 0.4) * cell, T.height(gx, gz) + 0.6, z0 + (gz + 0.6) * cell), unit((math.cos(az), -0.03, math.sin(az))), 0.25, 40.0)
    for k in range(6):
        def make():
            gx, gz = interior()
            return (x0 + (gx + 0.3) * cell, y0 - 3.0, z0 + (gz + 0.7) * cell), unit((rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3))), (0.0, 0.3, 0.7)[k % 3]
        pick("from-below", make)
    if T.cpd > 1:
        hx, hz = x0 + 1.5 * float(T.chunk_size), z0 + 1.5 * float(T.chunk_size)
        add("through-hole", (hx, top + 1.0, hz), (0.0, -1.0, 0.0), 0.5)                                   # falls through: a miss
        add("through-hole", (hx, top + 1.0, hz), unit((-1.0, -0.35, 0.1)), 0.3)                           # over the hole onto chunk (0, 1)
        add("through-hole", (hx, top + 1.0, hz), unit((0.1, -0.35, -1.0)), 0.3)                           # onto chunk (1, 0)
        add("through-hole", (hx, y0 - 1.0, hz), unit((-1.0, 0.12, 0.05)), 0.2)                            # from under the hole against the underside
        add("through-hole", (hx + 3.0, top + 4.0, hz + 2.0), unit((-0.05, -1.0, 0.02)), 1.0)              # through the hole and away below
        add("through-hole", (hx - 11.0, top + 1.0, hz - 11.5), (0.0, -1.0, 0.0), 1.2)                     # beside the hole's corner: the rim's edge
    for k in range(6):                                                    # in touch at the origin: well inside the margin, and between the margins
        gx, gz = interior()
        h = T.height(gx, gz)
        r = 0.3
        gap = (-0.05, 5e-5, -0.2)[k % 3]
        p = np.array([x0 + gx * cell, h, z0 + gz * cell])
        d = tp.expect(T, p + np.array([0.0, 1.0, 0.0]), np.inf)
        add("touch", d.point + (r + gap) * d.normal, (0.3, -1.0, 0.1), r, 5.0)
    for k in range(8):
        def make():
            gx, gz = interior()
            org = (x0 + (gx + 0.3) * cell, top + 1.0, z0 + (gz + 0.6) * cell)
            dirn = (0.0, -1.0, 0.0) if k % 2 == 0 else tuple(unit((0.5, -1.0, 0.25)))
            full = expect(T, org, dirn, 0.2, np.inf)
            return org, dirn, 0.2, np.float32(full.t + ((-2e-3, 1e-3, -0.5, 2.0)[k % 4]))
        if "max-t" in families:
            add("max-t", *make())
    for k in range(8):
        def make():
            gx, gz = interior()
            az = rng.uniform(0, 2 * math.pi)
            return (x0 + (gx + 0.37) * cell, top + 0.5, z0 + (gz + 0.21) * cell), unit((0.3 * math.cos(az), -1.0, 0.3 * math.sin(az))), 0.0
        pick("radius-zero", make)
    for k in range(4):
        gx, gz = interior()
        h = T.height(gx, gz)
        add("zero-direction", (x0 + gx * cell, h + (0.1, 1.0, -0.1, -1.0)[k], z0 + gz * cell), (0.0, 0.0, 0.0), 0.3)   # an overlap test: in touch from either side, or clear
    for k in range(6):
        def make():
            gx, gz = interior()
            return (x0 + (gx + 0.4) * cell, top + 1.0, z0 + (gz + 0.6) * cell), np.array((0.2, -1.0, -0.1)) * (2.5, 0.01, 7.0)[k % 3], 0.25
        pick("non-unit", make)
    for k in range(6):
        def make():
            az = rng.uniform(0, 2 * math.pi)
            cx_, cz_ = x0 + 0.5 * T.span, z0 + 0.5 * T.span
            org = np.array([cx_ + 0.9 * T.span * math.cos(az), top + rng.uniform(1.0, 6.0), cz_ + 0.9 * T.span * math.sin(az)])
            gx, gz = interior()
            aim = np.array([x0 + (gx + 0.4) * cell, T.height(gx, gz), z0 + (gz + 0.3) * cell])
            return org, unit(aim - org), (0.1, 0.6)[k % 2]
        pick("from-outside", make)
    return out


_BATTERY = None


def battery():
    """({layout name: Terrain}, [Case]): about 150 casts over one chunk, the scene's layout with its hole, and one chunk far from the origin"""
    global _BATTERY
    if _BATTERY is None:
        layouts = tp.layouts()
        rng = np.random.default_rng(20261021)
        cases = []
        for name in ("one-chunk", "scene"):
            cases += _battery_of(name, layouts[name], rng)
        far = [Case("far", "far", c.origin, c.direction, c.radius, c.max_t) for c in _battery_of("far", layouts["far"], rng, ("drop-face", "slanted", "from-below", "radius-zero"))][::2]
        _BATTERY = (layouts, cases + far)
    return _BATTERY


_DONE = None


def battery_done():
    """[(float64 Reading, ids, (float32 answer | None, most samples))] of the battery, computed once"""
    global _DONE
    if _DONE is None:
        layouts, cases = battery()
        _DONE = []
        for c in cases:
            T = layouts[c.layout]
            e, ids = cast_ids(T, c.origin, c.direction, c.radius, c.max_t)
            _DONE.append((e, ids, cast32(T, c.origin, c.direction, c.radius, c.max_t, ids)))
    return _DONE


def family_of(case):
    return case.family + ("/r0" if case.radius == 0 and case.family != "radius-zero" else "")


def scale_of(case, e):
    return 1.0 + float(np.abs(case.origin).max()) + e.t * e.L


def errors(case, e, T, tri_id, t, point, normal, gap):
    """(t, point, normal, gap) errors of a float32 answer that names its triangle, in E_F32's units.  Point, normal and gap are held to
    THAT triangle at the answer's own t: the rule's winner is the triangle whose march stops first, and where two triangles are within
    the tolerance of each other the sheet's nearest point may be the other one's, up to sqrt(2 radius tol) away."""
    lo, hi = t_window(e)
    s = scale_of(case, e)
    O, D = case.origin.astype(np.float64), case.direction.astype(np.float64)
    tri = T.triangles()
    k = int(np.searchsorted(tri["id"], tri_id))
    centre = O + float(t) * D
    c = tp.closest_on_triangles64(centre, tri["a"][k:k + 1], tri["b"][k:k + 1], tri["c"][k:k + 1])[0]
    w = centre - c
    dist = float(np.linalg.norm(w))
    n = w / dist if dist > 0 else tri["n"][k]
    return (max(float(t) - hi, lo - float(t), 0.0) * e.L / s, float(np.linalg.norm(np.asarray(point, np.float64) - c)) / (1.0 + float(np.linalg.norm(c))),
            tp.angle(normal, n) * dist / s, abs(float(gap) - (dist - float(case.radius))) / s)


def measure_f32():
    """{family: (t, point, normal, gap)}: the worst error of the restatement over the decided hits"""
    layouts, cases = battery()
    out = {}
    for c, (e, ids, (got, _)) in zip(cases, battery_done()):
        if e.kind != "hit":
            continue
        assert got is not None, (c.family, c.origin)
        fam = family_of(c)
        out[fam] = tuple(max(a, b) for a, b in zip(out.get(fam, (0.0,) * 4), errors(c, e, layouts[c.layout], got[6], got[1], got[2], got[4], got[3])))
    return out


def tolerance(family):
    return tuple(max(4.0 * v, 4.0 * F32_EPS) for v in E_F32[family])


# ---- the stop against the proximity reading there ---------------------------------------------------------------------------------------
# A cast from above that hits, then terrain_prox64.reading32 at the float32 centre origin + t * direction: distance - radius against the
# hit's gap, in float32 ulps of the gap's scale.  Both evaluate tpTriangle at the same float32 centre, so where the cast's winner is the
# nearest triangle there the difference is 0 bits; cross_check_applies() says where it is (two triangles within the tolerance of each
# other may be won by the one whose march stops first while the other is nearer by less than the tolerance).  Measured by
# test_terrain_spherecast64_cpu.py: CROSS_CHECK_ULPS over the cases that apply.
CROSS_CHECK_FAMILIES = ("drop-face", "slanted", "non-unit", "max-t")
CROSS_CHECK_ULPS = 0
_CROSS = None


def cross_check32():
    """{battery index: (|(d - radius) - gap| in float32 ulps of max(|gap|, radius, 1e-4), winner is the nearest triangle, point and normal equal)}"""
    global _CROSS
    if _CROSS is None:
        layouts, cases = battery()
        _CROSS = {}
        for i, (c, (e, ids, (got, _))) in enumerate(zip(cases, battery_done())):
            if c.family not in CROSS_CHECK_FAMILIES or got is None or got[0] != HIT:
                continue
            T = layouts[c.layout]
            centre = _v(c.origin + _v(got[1] * c.direction))
            near = tp.reading32(T, centre, np.inf)
            diff = abs(float(f(near[0] - c.radius)) - float(got[3])) / (F32_EPS * max(abs(float(got[3])), float(c.radius), 1e-4))
            _CROSS[i] = (diff, near[3] == got[6], near[1].tobytes() == got[2].tobytes() and near[2].tobytes() == got[4].tobytes())
    return _CROSS


def cross_check_applies(i):
    x = cross_check32().get(i)
    return x is not None and x[1]


def random_casts(T, n, seed=20261022):
    """n seeded casts all over the layout: origins in and around the terrain's box, every kind of direction, radii 0 .. 1.5"""
    rng = np.random.default_rng(seed)
    lo, hi = T.box()
    O = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (n, 3))).astype(np.float32)
    O[:, 1] = (lo[1] + (hi[1] - lo[1]) * rng.uniform(-0.5, 2.0, n)).astype(np.float32)
    D = rng.normal(size=(n, 3))
    D[::3] = (0.0, -1.0, 0.0)
    D[1::7, 1] *= 0.05
    D = (D * rng.choice([1.0, 1.0, 0.1, 7.0], n)[:, None]).astype(np.float32)
    R = rng.choice([0.0, 0.05, 0.3, 1.0, 1.5], n).astype(np.float32)
    Tm = np.where(np.arange(n) % 4 == 0, rng.uniform(1.0, 40.0, n), np.inf).astype(np.float32)
    return O, D, R, Tm


def measure_iterations(n=10000):
    """the most samples a triangle's march takes in the restatement: (over the battery, over n random casts on the scene's layout, each
    against the triangles around its float64 first contact, and the number of unresolved casts among both)"""
    worst_b = max(m for _, _, (_, m) in battery_done())
    unresolved = sum(1 for _, _, (got, _) in battery_done() if got is not None and got[0] == UNRESOLVED)
    T = t64.scene_layout()
    O, D, R, Tm = random_casts(T, n)
    worst_r = 0
    for i in range(n):
        _, ids = cast_ids(T, O[i], D[i], R[i], Tm[i])
        got, m = cast32(T, O[i], D[i], R[i], Tm[i], ids)
        worst_r = max(worst_r, m)
        unresolved += got is not None and got[0] == UNRESOLVED
    return worst_b, worst_r, unresolved


# ---- the battery's answers as a fixture --------------------------------------------------------------------------------------------------
# The float64 readings and the float32 restatement of the battery take minutes of numpy; the GPU tests read them from
# tests/golden/terrain_spherecast64.npz, which golden_arrays() computes and test_terrain_spherecast64_cpu.py holds to a fresh computation.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_spherecast64.npz")
KINDS = ("miss", "hit", "touch", "undecided")


def golden_arrays():
    layouts, cases = battery()
    done, cross = battery_done(), cross_check32()
    n = len(cases)
    g = dict(layout=np.array([c.layout for c in cases]), family=np.array([c.family for c in cases]), origin=np.array([c.origin for c in cases], f),
             direction=np.array([c.direction for c in cases], f), radius=np.array([c.radius for c in cases], f), max_t=np.array([c.max_t for c in cases], f),
             kind=np.array([KINDS.index(e.kind) for e, _, _ in done], np.int32), t=np.array([np.nan if e.t is None else e.t for e, _, _ in done]),
             cos=np.array([e.cos for e, _, _ in done]), tol=np.array([e.tol for e, _, _ in done]), L=np.array([e.L for e, _, _ in done]),
             hit=np.zeros(n, np.uint32), iterations=np.zeros(n, np.uint32), triangle=np.zeros(n, np.uint32), answer=np.zeros((n, 8), f),
             cross=np.array([bool(cross.get(i, (0, False))[1]) for i in range(n)]))
    for i, (_, _, (got, _)) in enumerate(done):
        if got is not None:
            g["hit"][i], g["iterations"][i], g["triangle"][i] = got[0], got[5], got[6]
            g["answer"][i] = np.concatenate([[got[1]], got[2], [got[3]], got[4]])      # t, point, gap, normal
    return g


def load_golden():
    return dict(np.load(GOLDEN))
