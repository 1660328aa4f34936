"""What mi_proximity with MI_PROX_TERRAIN (World.proximity(terrain=True)) must report for the heightmap terrain alone: a float64
reading of the rule stated in include/mi_physics.h, brute force over terrain_ray64.Terrain.triangles(), a numpy float32 restatement in the
operation order of csrc/terrain_point.h, and the battery both are held to.

The rule: per triangle f = (a, b, c), n_f = unit(cross(b - a, c - a)), c_f = the closest point of the triangle to p, d_f = |p - c_f|.  The
nearest triangle is the smallest d_f, of equal d_f the lowest id.  Sign: among the triangles whose cell contains p's (x, z) (u, v in
[0, 1] closed; triangle 0 owns u + v <= 1, triangle 1 owns u + v >= 1) the lowest id decides, below iff dot(p - a_f, n_f) < 0; over no
chunk that has heights a point is never below.  d = d_f above, -d_f below; point = c_f; normal = unit(p - c_f) above, unit(c_f - p)
below, n_f where p == c_f.  Within iff d <= radius.

Decision margins of a reading (Reading.margins, metres unless said otherwise):
  near     d_f of the nearest triangle whose closest point is another point, minus the best d_f: below it float32 may switch triangle
           AND point (two triangles that share the closest point, on an edge or a vertex, tie in d_f and in the point: there only the id
           is undecided, Reading.tri_decided)
  sign     |dot(p - a_f, n_f)| of the deciding triangle: the height over the surface along its normal
  radius   |d - radius|
  rim      distance in x / z from p to the border of the region that has heights (inf when that region is the whole plane)
A reading is decided if every margin is at least DECIDE_ULPS = 16 float32 ulps of M = largest |coordinate| of p + of the terrain's box,
the scale terrain_ray64 uses: a vertex carries 3 roundings at M, p - c_f one more per coordinate and the distance 3 relative ones, so
d_f and the plane distance are good to about 6 ulps of M, and 16 leaves that more than twice over (measured: under 1 ulp, E_F32)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_ray64 as t64  # noqa: E402
from terrain_ray64 import CELLS, F32_EPS, TERRAIN_COLLIDER, STATIC_BODY  # noqa: E402,F401

DECIDE_ULPS = 16.0
# float32 restatement against float64 over the decided cases of the battery, per family: (distance error / M, point error / M, normal
# angle in radians x distance / M: the normal is the unit vector of a difference of that length).  Measured by
# test_terrain_prox64_cpu.py, which holds this table to its measurement within 1.5 x either way; the device's tolerance is
# max(4 x figure, 4 float32 ulps).
E_F32 = {
    "below-deep": (1.5e-08, 9.9e-08, 1e-07),
    "below-shallow": (9.3e-09, 2e-08, 1.9e-08),
    "face": (1.7e-08, 6.7e-08, 6.4e-08),
    "far-corner": (9.5e-09, 2.5e-08, 2.5e-08),
    "hole": (1.9e-08, 1.5e-08, 1.5e-08),
    "radius": (4e-09, 1.9e-08, 1.9e-08),
    "radius-inf": (3.9e-08, 1.4e-08, 1.7e-08),
    "ridge-peak": (1.2e-08, 1.1e-08, 7.2e-11),
    "rim-outside": (1.1e-08, 5.4e-08, 5.2e-08),
    "seam": (4.3e-09, 2.8e-08, 2.7e-08),
    "surface": (0.0, 0.0, 0.0),     # (no decided case: the family is the sign's knife edge)
    "valley": (2.5e-08, 6.8e-08, 6.4e-08),
}


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
def closest_on_triangles64(p, a, b, c):
    """The closest point of each triangle (a, b, c) [T, 3] to p, by the regions of its vertices, edges and face, vectorised"""
    ab, ac, ap = b - a, c - a, p[None] - a
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    bp = p[None] - b
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    cp = p[None] - c
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        sab, sac, sbc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    face = a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    vals = [a, b, a + sab[:, None] * ab, c, a + sac[:, None] * ac, b + sbc[:, None] * (c - b)]
    out = face
    for cond, val in reversed(list(zip(conds, vals))):
        out = np.where(cond[:, None], val, out)
    return out


class Reading:
    found = False; d = 0.0; d_f = 0.0; point = None; normal = None; tri = None; below = False; tri_decided = True; on_surface = False

    def __init__(self):
        self.margins = {"near": math.inf, "sign": math.inf, "radius": math.inf, "rim": math.inf}
        self.m = 1.0

    @property
    def decided(self):
        return min(self.margins.values()) >= DECIDE_ULPS * F32_EPS * self.m


def _rim_distance(T, x, z):
    """distance in x / z from (x, z) to the border of the union of the chunks that have heights"""
    best = math.inf
    inside = False
    size = float(T.chunk_size)
    for (X, Z) in T.chunks:
        x0, z0 = float(T.corner[0]) + X * size, float(T.corner[2]) + Z * size
        dx, dz = max(x0 - x, x - (x0 + size), 0.0), max(z0 - z, z - (z0 + size), 0.0)
        if dx == 0.0 and dz == 0.0:
            inside = True
            # the sides of this chunk that no other chunk with heights adjoins
            for (nx, nz, dist) in ((X - 1, Z, x - x0), (X + 1, Z, x0 + size - x), (X, Z - 1, z - z0), (X, Z + 1, z0 + size - z)):
                if (nx, nz) not in T.chunks:
                    best = min(best, dist)
        else:
            best = min(best, math.hypot(dx, dz))
    return best if (inside or T.chunks) else math.inf


def expect(T, point, radius):
    """The float64 reading of the terrain alone for the float32 world point and radius"""
    r = Reading()
    p = np.asarray(point, np.float32).astype(np.float64)
    radius = float(np.float32(radius))
    if not radius >= 0.0 or not np.isfinite(p).all():
        return r
    tri = T.triangles()
    if not len(tri["id"]):
        return r
    r.m = T.magnitude(p)
    cf = closest_on_triangles64(p, tri["a"], tri["b"], tri["c"])
    df = np.linalg.norm(p[None] - cf, axis=1)
    k = int(np.lexsort((tri["id"], df))[0])
    r.d_f, r.point, r.tri = float(df[k]), cf[k], int(tri["id"][k])
    elsewhere = np.linalg.norm(cf - cf[k][None], axis=1) > 1e-9 * (1.0 + r.m)
    if elsewhere.any():
        r.margins["near"] = float(df[elsewhere].min() - df[k])
    r.tri_decided = int((df <= df[k] + DECIDE_ULPS * F32_EPS * r.m).sum()) == 1
    u, v = (p[0] - tri["x0"]) / (tri["x1"] - tri["x0"]), (p[2] - tri["z0"]) / (tri["z1"] - tri["z0"])
    owns = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & np.where(tri["which"] == 0, u + v <= 1, u + v >= 1)
    r.margins["rim"] = _rim_distance(T, p[0], p[2])
    if owns.any():
        j = int(np.flatnonzero(owns)[0])                      # the triangles are sorted by id
        h = float(np.dot(p - tri["a"][j], tri["n"][j]))
        r.below = h < 0.0
        r.margins["sign"] = abs(h)
    r.d = -r.d_f if r.below else r.d_f
    r.margins["radius"] = abs(r.d - radius) if math.isfinite(radius) else math.inf
    w = (r.point - p) if r.below else (p - r.point)
    ln = float(np.linalg.norm(w))
    r.on_surface = ln == 0.0
    r.normal = w / ln if ln > 0 else tri["n"][k]
    r.found = r.d <= radius
    return r


# ---- the float32 restatement of csrc/terrain_point.h ---------------------------------------------------------------------------------
import proximity64 as p64  # noqa: E402

f = np.float32
_v, _dot, _cross, _len, _unit32 = p64._v, p64._dot, p64._cross, p64._len, p64._unit32


def vertices32(T, tri_id):
    """(a, b, c, A.x, D.x, A.z, D.z, which) of a triangle by terrainCellVertices / terrainChunkMin in float32"""
    tri_id = int(tri_id)
    which, cell, chunk = tri_id & 1, (tri_id >> 1) & 16383, tri_id >> 15
    cx, cz, X, Z = cell & 127, cell >> 7, chunk % T.cpd, chunk // T.cpd
    H = T.chunks[(X, Z)]
    cs, hs = f(T.chunk_size / f(CELLS)), f(T.amplitude / f(65535))
    mn = _v([f(f(X) * T.chunk_size) + T.corner[0], f(0) + T.corner[1], f(f(Z) * T.chunk_size) + T.corner[2]])

    def vert(dx, dz):
        return _v([f(f(cx + dx) * cs) + mn[0], f(f(H[cz + dz, cx + dx]) * hs) + mn[1], f(f(cz + dz) * cs) + mn[2]])
    A, B, C, D = vert(0, 0), vert(0, 1), vert(1, 0), vert(1, 1)
    a, b, c = (A, B, C) if which == 0 else (C, B, D)
    return a, b, c, A[0], D[0], A[2], D[2], which


def triangle32(p, a, b, c):
    """tpTriangle: (n, c_f, d_f)"""
    n = _unit32(_cross(_v(b - a), _v(c - a)))
    cf = p64._closest_on_triangle32(p, a, b, c, n)
    return n, cf, _len(_v(p - cf))


def owns32(p, x0, x1, z0, z1, which):
    with np.errstate(all="ignore"):
        u, v = f(f(p[0] - x0) / f(x1 - x0)), f(f(p[2] - z0) / f(z1 - z0))
    if not (u >= 0 and u <= 1 and v >= 0 and v <= 1):
        return False
    return f(u + v) <= 1 if which == 0 else f(u + v) >= 1


def near_ids(T, point, extra=0.0):
    """ids of the triangles that can decide a float32 reading of p: those within 1e-3 (1 + d) + extra of the smallest float64 distance
    and those whose cell, widened by a hundredth of a cell, holds p's (x, z).  The restatement over these is the restatement over all."""
    p = np.asarray(point, np.float32).astype(np.float64)
    tri = T.triangles()
    cf = closest_on_triangles64(p, tri["a"], tri["b"], tri["c"])
    df = np.linalg.norm(p[None] - cf, axis=1)
    w = 0.01 * T.cell
    col = (p[0] >= tri["x0"] - w) & (p[0] <= tri["x1"] + w) & (p[2] >= tri["z0"] - w) & (p[2] <= tri["z1"] + w)
    return tri["id"][(df <= df.min() + 1e-3 * (1.0 + df.min()) + extra) | col]


def reading32(T, point, radius, ids=None):
    """k_px_terrain's answer for the terrain alone: None, or (d, point, normal, triangle id) in float32"""
    p, radius = _v(point), f(radius)
    if not radius >= 0 or not np.isfinite(p).all():
        return None
    ids = near_ids(T, point) if ids is None else ids
    best_d, best_id, best_c, best_n, sign_id, below = f(np.inf), None, None, None, None, False
    for tid in sorted(int(i) for i in ids):
        a, b, c, x0, x1, z0, z1, which = vertices32(T, tid)
        n, cf, df = triangle32(p, a, b, c)
        if df < best_d:                                       # ids ascend: a tie keeps the lower id
            best_d, best_id, best_c, best_n = df, tid, cf, n
        if sign_id is None and owns32(p, x0, x1, z0, z1, which):
            sign_id, below = tid, bool(_dot(_v(p - a), n) < 0)
    if best_id is None:
        return None
    d = f(-best_d) if below else best_d
    if not d <= radius:
        return None
    w = _v(best_c - p) if below else _v(p - best_c)
    n = _unit32(w) if _len(w) > 0 else best_n
    return d, best_c, n, best_id


# ---- the battery -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, layout, family, point, radius=np.inf):
        self.layout, self.family, self.point, self.radius = layout, family, np.asarray(point, np.float32), np.float32(radius)


FAMILIES = ("face", "ridge-peak", "valley", "surface", "below-shallow", "below-deep", "seam", "hole", "rim-outside", "radius", "radius-inf", "far-corner")


def _local_extrema(T, kind, count, rng):
    """global vertex indices (gx, gz) of strict local maxima (kind = +1) or minima (-1) of the heights, away from the rim"""
    out = []
    n = T.cpd * CELLS
    tries = 0
    while len(out) < count and tries < 200000:
        tries += 1
        gx, gz = int(rng.integers(2, n - 1)), int(rng.integers(2, n - 1))
        hs = [[T.height(gx + dx, gz + dz) for dx in (-1, 0, 1)] for dz in (-1, 0, 1)]
        if any(h is None for row in hs for h in row):
            continue
        c = hs[1][1]
        others = [h for j, row in enumerate(hs) for i, h in enumerate(row) if (i, j) != (1, 1)]
        if all(kind * (c - h) > 1e-3 for h in others):
            out.append((gx, gz))
    return out


def _battery_of(name, T, rng):
    out = []
    cell, n = T.cell, T.cpd * CELLS
    x0, z0, y0 = float(T.corner[0]), float(T.corner[2]), float(T.corner[1])

    def add(family, point, radius=np.inf):
        out.append(Case(name, family, point, radius))

    def interior():
        while True:
            gx, gz = int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1))
            if all(T.height(gx + dx, gz + dz) is not None and not T.near_rim(*T.vertex_xz(gx + dx, gz + dz), 1.5 * cell, 1.5 * cell) for dx in (0, 1) for dz in (0, 1)):
                return gx, gz

    def surface_y(gx, gz, fx, fz):
        """height of the surface over the point (gx + fx, gz + fz) of a cell, fx + fz != 1"""
        ha, hb, hc, hd = T.height(gx, gz), T.height(gx, gz + 1), T.height(gx + 1, gz), T.height(gx + 1, gz + 1)
        return ha + fx * (hc - ha) + fz * (hb - ha) if fx + fz < 1 else hd + (1 - fx) * (hb - hd) + (1 - fz) * (hc - hd)

    def pick(family, make):
        """make() draws a point (and radius) of the family afresh; the first draw of 24 whose float64 reading is decided is taken, so a
        family's share of undecided cases is what its geometry forces, not what the draw happened to meet"""
        for attempt in range(24):
            point, radius = make()
            if expect(T, point, radius).decided or attempt == 23:
                return add(family, point, radius)

    def over_cell(fx, fz, dy, radius=np.inf):
        def make():
            gx, gz = interior()
            return (x0 + (gx + fx) * cell, surface_y(gx, gz, fx, fz) + dy, z0 + (gz + fz) * cell), radius
        return make

    for k in range(8):
        fx, fz = (0.3, 0.25) if k % 2 else (0.7, 0.65)
        pick("face", over_cell(fx, fz, (0.02, 0.05, 0.4, 2.5)[k % 4], (np.inf, 5.0)[k % 2]))
    peaks, pits = _local_extrema(T, +1, 64, rng), _local_extrema(T, -1, 64, rng)
    for k in range(8):
        off = ((0.0, 0.0), (0.01, 0.0), (0.0, -0.01), (0.006, 0.007))[k % 4]        # over the vertex itself and just beside it: vertex and edge regions

        def make():
            gx, gz = peaks[int(rng.integers(len(peaks)))]
            return (x0 + (gx + off[0]) * cell, T.height(gx, gz) + (0.3, 1.0)[k % 2], z0 + (gz + off[1]) * cell), np.inf
        pick("ridge-peak", make)
    for k in range(8):
        def make():
            gx, gz = pits[int(rng.integers(len(pits)))]
            return (x0 + (gx + 0.3) * cell, T.height(gx, gz) + (0.5, 1.5, 3.0, 6.0)[k % 4], z0 + (gz + 0.2) * cell), np.inf   # high over a pit: the nearest triangle is up a slope
        pick("valley", make)
    for k in range(3):                                          # on the surface: the sign is a coin's toss by construction (undecided)
        gx, gz = interior()
        if k == 0:
            add("surface", (x0 + gx * cell, T.height(gx, gz), z0 + gz * cell), 1.0)
        else:
            add("surface", (x0 + (gx + 0.3) * cell, surface_y(gx, gz, 0.3, 0.2), z0 + (gz + 0.2) * cell), 1.0)
    for k in range(8):
        pick("below-shallow", over_cell(0.35, 0.4, -(0.01, 0.05, 0.1, 0.3)[k % 4], (0.0, 0.5, np.inf, 0.02)[k % 4]))
    for k in range(8):
        pick("below-deep", over_cell(0.6, 0.7, -(1.0, 2.5, 5.0, 9.0)[k % 4], (0.0, 0.25)[k % 2]))   # deeper than the radius: within all the same
    if T.cpd > 1:
        for k in range(8):
            on_x = k % 2 == 0                                   # the seam between chunks (0, 0) and (1, 0), resp. (0, 0) and (0, 1)
            dy = (0.2, -0.2, 1.0, -1.0)[k // 2]

            def make():
                g = int(rng.integers(5, CELLS - 5))
                gx, gz = (CELLS, g) if on_x else (g, CELLS)
                return ((x0 + gx * cell, T.height(gx, gz) + dy, z0 + (gz + 0.5) * cell) if on_x else (x0 + (gx + 0.5) * cell, T.height(gx, gz) + dy, z0 + gz * cell)), np.inf
            pick("seam", make)
        hx, hz = x0 + 1.5 * float(T.chunk_size), z0 + 1.5 * float(T.chunk_size)
        for k in range(8):
            # over the hole, high and low, and 0.4 cell into it beside its border with chunk (0, 1) / (1, 0)
            def make():
                if k < 4:
                    j = rng.uniform(-1.0, 1.0)
                    return (hx + (k - 1.5) * 2.0 + j, y0 + (8.0, 1.0, -1.0, 3.0)[k], hz - (k - 1.5) * 1.5 + j), (np.inf, 30.0)[k % 2]
                g = int(rng.integers(5, CELLS - 5))
                side = (CELLS + 0.4, g + 0.3) if k % 2 else (g + 0.3, CELLS + 0.4)
                hgt = T.height(CELLS, g) if k % 2 else T.height(g, CELLS)
                return (x0 + side[0] * cell, hgt + (0.5, -0.5)[(k // 2) % 2], z0 + side[1] * cell), np.inf
            pick("hole", make)
    for k in range(8):
        out_by = (0.3, 2.0, 0.05, 6.0)[k % 4]
        dy = (0.5, -0.7, 2.0, -3.0)[(k // 2) % 4]               # also lower than the surface beside it: never below (no side walls)

        def make():
            g = int(rng.integers(5, CELLS - 5))
            edge_h = T.height(0, g) if k % 2 == 0 else T.height(g, 0)
            return ((x0 - out_by, edge_h + dy, z0 + (g + 0.5) * cell) if k % 2 == 0 else (x0 + (g + 0.5) * cell, edge_h + dy, z0 - out_by)), np.inf
        pick("rim-outside", make)
    for k in range(8):
        def make():
            gx, gz = interior()
            pt = (x0 + (gx + 0.3) * cell, T.height(gx, gz) + (0.5, 1.2)[k % 2], z0 + (gz + 0.3) * cell)
            d = expect(T, pt, np.inf).d
            return pt, (d * (1.0 - 2e-3) if k % 2 else d * (1.0 + 2e-3))       # just under (nothing within) and just over the distance
        pick("radius", make)
    for k in range(4):
        def make():
            gx, gz = interior()
            return (x0 + (gx + 0.5) * cell + (40.0 if k == 3 else 0.0), y0 + float(T.amplitude) + (1.0, 10.0, 40.0, 15.0)[k], z0 + (gz + 0.25) * cell), np.inf
        pick("radius-inf", make)
    return out


_BATTERY = None


def layouts():
    """{layout name: Terrain}: one chunk, the scene's 2 x 2 layout with its hole, and the one chunk far from the origin"""
    out = {"one-chunk": t64.one_chunk(), "scene": t64.scene_layout()}
    out["far"] = out["one-chunk"].moved((1000.0, 200.0, -1500.0))    # (exact in float32, like every grid line from there)
    return out


def battery():
    """({layout name: Terrain}, [Case]): about 150 points over one chunk, the scene's 2 x 2 layout with its hole, and that layout moved far
    from the origin (seeded)"""
    global _BATTERY
    if _BATTERY is None:
        lay = layouts()
        rng = np.random.default_rng(20261020)
        cases = []
        for name in ("one-chunk", "scene"):
            cases += _battery_of(name, lay[name], rng)
        far = [Case("far", "far-corner", c.point, c.radius) for c in _battery_of("far", lay["far"], rng) if c.family in ("face", "ridge-peak", "below-shallow", "below-deep")][::2]
        _BATTERY = (lay, cases + far)
    return _BATTERY


_EXPECTED = None


def battery_expected():
    global _EXPECTED
    if _EXPECTED is None:
        layouts, cases = battery()
        _EXPECTED = [expect(layouts[c.layout], c.point, c.radius) for c in cases]
    return _EXPECTED


_RESTATED = None


def battery_restated():
    global _RESTATED
    if _RESTATED is None:
        layouts, cases = battery()
        _RESTATED = [reading32(layouts[c.layout], c.point, c.radius) for c in cases]
    return _RESTATED


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(math.atan2(np.linalg.norm(np.cross(a, b)), float(np.dot(a, b))))


def errors(e, d, point, normal):
    """(distance, point, normal) errors of a float32 answer against the reading e, in E_F32's units"""
    return (abs(float(d) - e.d) / e.m, float(np.linalg.norm(np.asarray(point, np.float64) - e.point)) / e.m, angle(normal, e.normal) * e.d_f / e.m)


def measure_f32():
    """{family: (distance, point, normal)}: the worst error of the restatement over the decided, found cases"""
    layouts, cases = battery()
    out = {fam: (0.0, 0.0, 0.0) for fam in FAMILIES}
    for c, e, got in zip(cases, battery_expected(), battery_restated()):
        if not (e.decided and e.found):
            continue
        assert got is not None, (c.family, c.point)
        out[c.family] = tuple(max(a, b) for a, b in zip(out[c.family], errors(e, got[0], got[1], got[2])))
    return out


def tolerance(family):
    return tuple(max(4.0 * v, 4.0 * F32_EPS) for v in E_F32[family])


# ---- the battery's answers as a fixture --------------------------------------------------------------------------------------------------
# The GPU tests read the float64 readings and the float32 restatement of the battery from tests/golden/terrain_prox64.npz, which
# golden_arrays() computes and test_terrain_prox64_cpu.py holds to a fresh computation.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_prox64.npz")


def golden_arrays():
    layouts, cases = battery()
    ex, re = battery_expected(), battery_restated()
    n = len(cases)
    g = dict(layout=np.array([c.layout for c in cases]), family=np.array([c.family for c in cases]), point=np.array([c.point for c in cases], f),
             radius=np.array([c.radius for c in cases], f), decided=np.array([e.decided for e in ex]), found=np.array([e.found for e in ex]),
             below=np.array([e.below for e in ex]), tri_decided=np.array([e.tri_decided for e in ex]), tri=np.array([-1 if e.tri is None else e.tri for e in ex], np.int64),
             d=np.array([e.d for e in ex]), d_f=np.array([e.d_f for e in ex]), m=np.array([e.m for e in ex]), c=np.array([e.point for e in ex]), n=np.array([e.normal for e in ex]),
             found32=np.array([r is not None for r in re]), triangle32=np.zeros(n, np.uint32), answer32=np.zeros((n, 7), f))
    for i, r in enumerate(re):
        if r is not None:
            g["triangle32"][i] = r[3]
            g["answer32"][i] = np.concatenate([[r[0]], r[1], r[2]])                    # d, point, normal
    return g


def load_golden():
    return dict(np.load(GOLDEN))
