"""Float64 geometry of the world-space collider records (COLLIDER_DTYPE) and the collision edge-case batteries.

This is an independent reference for the narrowphase: it shares no formula with the oracle or the device, only the record
layout (narrow.h asSphere / asCapsule / asBox / asObb / asHull).  Every value is computed in float64 on the float32 records.

Signed depth of a pair: d = min over unit n of h_A(n) + h_B(-n), h = support function.  d > 0: the shapes overlap and d is the
penetration depth (minimum translation distance); d < 0: they are apart by -d.  n points from A to B (the contact normal's sense).
Spheres and capsules are a core (point / segment) swept by a ball, so h = h_core + r and the depth is the core pair's plus the radii.
How each pair is solved, and how exact the answer is:
  * EXACT (rounding only, <= 1e-12 relative): every pair of sphere, capsule, AABB, OBB and hull.  Cores that intersect: minimum of
    h_A + h_B over the exact candidate set (face normals of both polytopes, edge x edge and segment x edge crosses; a superset of
    the Minkowski difference's face normals, so the minimum is attained in it).  Cores apart: minus their distance, from closed
    forms over features (point-point, point-segment, segment-segment, point-triangle, segment-triangle edges): the closest points
    of two disjoint convex polytopes lie on a vertex/edge/face pair.
  * APPROXIMATE: every pair with a cylinder (its rims are curved).  The candidates above (with the cylinder's axis as an edge and
    face normal), 2562 Fibonacci directions, then a Nelder-Mead refinement of the best three on the sphere of directions (pairs
    sampled clearly apart, below -(size A + size B) / 4, are not refined and carry that as their error).  The value
    is an upper bound of the true minimum (a minimum over fewer directions); CYLINDER_DEPTH_ERR is the stated bound on how far
    above, checked against closed forms in tests/test_oracle_geometry.py.
Point-to-shape signed distances are exact for every shape (hull: max of face planes inside, nearest triangle outside).
"""
import math

import numpy as np

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
TYPE_NAMES = ("sphere", "capsule", "cylinder", "aabb", "obb", "hull")
CYLINDER_DEPTH_ERR_REL = 1e-9   # x (1 + size of the pair): stated error of the approximate (cylinder) depths


# ---------------------------------------------------------------------------------------------------------------------------
# Records -> float64 shapes
# ---------------------------------------------------------------------------------------------------------------------------
def quat_to_matrix(q):
    x, y, z, w = (float(v) for v in q)
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


_BOX_TRIS = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (0, 4, 7), (0, 7, 3)])
_BOX_SIGNS = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float64)


class Shape:
    """kind; core vertices `pts` (point, segment or polytope) and `radius` swept around them; polytopes: outward triangles `tris`,
    face normals, edge directions; cylinder: endpoints a, b and radius."""

    def __init__(self, kind, pts, radius=0.0, tris=None, normals=(), edges=(), cyl=None):
        self.kind = kind
        self.pts = np.asarray(pts, np.float64).reshape(-1, 3)
        self.radius = float(radius)
        self.tris = tris
        self.normals = np.asarray(normals, np.float64).reshape(-1, 3)
        self.edges = np.asarray(edges, np.float64).reshape(-1, 3)
        self.cyl = cyl
        self.center = self.pts.mean(axis=0)
        self.size = float(np.abs(self.pts - self.center).max()) + self.radius + (cyl[2] if cyl is not None else 0.0)

    def support(self, n):
        """h(n) for directions n [k, 3] (not necessarily unit: h is positively homogeneous)."""
        n = np.atleast_2d(n)
        if self.kind == CYLINDER:
            a, b, r = self.cyl
            u = (b - a) / np.linalg.norm(b - a)
            along = n @ u
            perp = np.sqrt(np.maximum((n * n).sum(axis=1) - along * along, 0.0))
            return np.maximum(n @ a, n @ b) + r * perp
        return (n @ self.pts.T).max(axis=1) + self.radius * np.linalg.norm(n, axis=1)

    def triangles(self):
        return self.pts[self.tris]


def _polytope(kind, verts, tris):
    verts = np.asarray(verts, np.float64)
    tris = np.asarray(tris, np.int64)
    t = verts[tris]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    e = np.concatenate([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]])
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    e = np.where(((e[:, 0] < 0) | ((e[:, 0] == 0) & (e[:, 1] < 0)) | ((e[:, 0] == 0) & (e[:, 1] == 0) & (e[:, 2] < 0)))[:, None], -e, e)
    e = np.unique(np.round(e, 12), axis=0)
    return Shape(kind, verts, 0.0, tris, nrm, e)


def shape_from_record(rec, hulls=()):
    """rec: one COLLIDER_DTYPE record (world space); hulls: [(vertices [n, 3], triangles [m, 3])] by geometry index."""
    t = int(rec["type"])
    s = np.asarray(rec["shape"], np.float32).astype(np.float64)
    if t == SPHERE:
        return Shape(SPHERE, s[0:3], s[3])
    if t == CAPSULE:
        return Shape(CAPSULE, [s[0:3], s[3:6]], s[6], edges=[s[3:6] - s[0:3]] if np.any(s[3:6] != s[0:3]) else ())
    if t == CYLINDER:
        a, b = s[0:3], s[3:6]
        assert np.any(a != b), "zero-length cylinder: float32 cannot hold its endpoints apart"
        u = (b - a) / np.linalg.norm(b - a)
        return Shape(CYLINDER, [a, b], 0.0, normals=[u], edges=[u], cyl=(a, b, float(s[6])))
    if t == AABB:
        lo, hi = s[0:3], s[3:6]
        verts = np.where(_BOX_SIGNS > 0, hi, lo)
        return Shape(AABB, verts, 0.0, _BOX_TRIS, np.eye(3), np.eye(3))
    if t == OBB:
        R = quat_to_matrix(s[0:4])
        verts = s[4:7] + (_BOX_SIGNS * s[7:10]) @ R.T
        return Shape(OBB, verts, 0.0, _BOX_TRIS, R.T, R.T)
    if t == HULL:
        R = quat_to_matrix(s[0:4])
        v, tri = hulls[int(s[7])]
        return _polytope(HULL, s[4:7] + np.asarray(v, np.float32).astype(np.float64) @ R.T, tri)
    raise ValueError(t)


# ---------------------------------------------------------------------------------------------------------------------------
# Closest-feature distances (vectorised, float64)
# ---------------------------------------------------------------------------------------------------------------------------
def _closest_on_segments(p, a, b):
    """closest point of segments [a, b] to points p (broadcast)."""
    ab = b - a
    den = (ab * ab).sum(axis=-1)
    t = np.where(den > 0, ((p - a) * ab).sum(axis=-1) / np.where(den > 0, den, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[..., None] * ab


def point_segment_distance(p, a, b):
    return np.linalg.norm(p - _closest_on_segments(p, a, b), axis=-1)


def segment_segment_distance(p1, q1, p2, q2):
    """distance between segments [p1, q1] and [p2, q2] (broadcast): the unconstrained-then-clamped closed form (Ericson 5.1.9) and,
    to be robust where it degenerates (parallel or zero-length segments), the four endpoint-to-segment distances."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a = (d1 * d1).sum(-1); e = (d2 * d2).sum(-1); f = (d2 * r).sum(-1); c = (d1 * r).sum(-1); b = (d1 * d2).sum(-1)
    den = a * e - b * b
    safe = np.where(den > 1e-300, den, 1.0)
    s = np.clip(np.where(den > 1e-300, (b * f - c * e) / safe, 0.0), 0.0, 1.0)
    t = np.where(e > 0, (b * s + f) / np.where(e > 0, e, 1.0), 0.0)
    s = np.where(t < 0, np.clip(np.where(a > 0, -c / np.where(a > 0, a, 1.0), 0.0), 0, 1), np.where(t > 1, np.clip(np.where(a > 0, (b - c) / np.where(a > 0, a, 1.0), 0.0), 0, 1), s))
    t = np.clip(t, 0.0, 1.0)
    best = np.linalg.norm(p1 + s[..., None] * d1 - (p2 + t[..., None] * d2), axis=-1)
    for d in (point_segment_distance(p1, p2, q2), point_segment_distance(q1, p2, q2), point_segment_distance(p2, p1, q1), point_segment_distance(q2, p1, q1)):
        best = np.minimum(best, d)
    return best


def point_triangle_distance(p, tri):
    """distance from points p [..., 3] to triangles tri [..., 3, 3] (broadcast): inside the prism, the plane distance; else the
    nearest edge."""
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=-1)
    n = n / np.where(nn > 0, nn, 1.0)[..., None]
    inside = np.ones(np.broadcast_shapes(p.shape[:-1], a.shape[:-1]), bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, p - u) * n).sum(-1) >= 0
    plane = np.abs(((p - a) * n).sum(-1))
    edge = np.minimum(np.minimum(point_segment_distance(p, a, b), point_segment_distance(p, b, c)), point_segment_distance(p, c, a))
    return np.where(inside & (nn > 0), plane, edge)


def _core_kind(s):
    return "point" if len(s.pts) == 1 else ("segment" if len(s.pts) == 2 and s.tris is None else "polytope")


def _core_distance(A, B):
    """distance between the cores of A and B (exact when they are disjoint; meaningless when they intersect)."""
    ka, kb = _core_kind(A), _core_kind(B)
    if ka == "polytope" and kb != "polytope":
        A, B, ka, kb = B, A, kb, ka
    if ka == "point" and kb == "point":
        return float(np.linalg.norm(A.pts[0] - B.pts[0]))
    if ka == "point" and kb == "segment":
        return float(point_segment_distance(A.pts[0], B.pts[0], B.pts[1]))
    if ka == "segment" and kb == "point":
        return float(point_segment_distance(B.pts[0], A.pts[0], A.pts[1]))
    if ka == "segment" and kb == "segment":
        return float(segment_segment_distance(A.pts[0], A.pts[1], B.pts[0], B.pts[1]))
    tb = B.triangles()
    if ka == "point":
        return float(point_triangle_distance(A.pts[0][None], tb).min())
    if ka == "segment":
        d = min(float(point_triangle_distance(A.pts[0][None], tb).min()), float(point_triangle_distance(A.pts[1][None], tb).min()))
        e0, e1 = tb.reshape(-1, 3)[None], np.roll(tb, -1, axis=1).reshape(-1, 3)[None]
        return min(d, float(segment_segment_distance(A.pts[0][None, None], A.pts[1][None, None], e0, e1).min()))
    ta = A.triangles()
    d = min(float(point_triangle_distance(A.pts[:, None, :], tb[None]).min()), float(point_triangle_distance(B.pts[:, None, :], ta[None]).min()))
    ea0, ea1 = ta.reshape(-1, 3), np.roll(ta, -1, axis=1).reshape(-1, 3)
    eb0, eb1 = tb.reshape(-1, 3), np.roll(tb, -1, axis=1).reshape(-1, 3)
    for k in range(0, len(ea0), 64):
        d = min(d, float(segment_segment_distance(ea0[k:k + 64, None], ea1[k:k + 64, None], eb0[None], eb1[None]).min()))
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# Signed depth
# ---------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    n = np.linalg.norm(v, axis=1)
    v = v[n > 1e-12 * max(1.0, float(n.max()) if len(n) else 1.0)]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = math.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def candidate_axes(A, B):
    ax = [A.normals, B.normals]
    if len(A.edges) and len(B.edges):
        ea, eb = A.edges, B.edges
        for k in range(0, len(ea), 256):
            ax.append(np.cross(ea[k:k + 256, None, :], eb[None, :, :]).reshape(-1, 3))
    ax.append((B.center - A.center)[None])
    ax.append(np.eye(3))   # (any direction is a valid candidate: keeps the set non-empty for parallel segments on one line)
    u = _unit(np.concatenate(ax))
    return np.concatenate([u, -u])


def _f(A, B, n):
    return A.support(n) + B.support(-n)


def signed_depth(A, B):
    """(depth, unit normal A->B, stated error).  See the module docstring for which pairs are exact."""
    cand = candidate_axes(A, B)
    vals = np.concatenate([_f(A, B, cand[k:k + 8192]) for k in range(0, len(cand), 8192)])
    i = int(np.argmin(vals))
    best, n = float(vals[i]), cand[i]
    if A.kind != CYLINDER and B.kind != CYLINDER:
        rsum = A.radius + B.radius
        if _core_kind(A) != "polytope" and _core_kind(B) != "polytope":   # point / segment cores: a flat Minkowski difference
            d = _core_distance(A, B)
            return rsum - d, (_unit(B.center - A.center)[0] if np.any(B.center != A.center) else n), 1e-12 * (1.0 + max(A.size, B.size) + float(np.abs(np.concatenate([A.pts, B.pts])).max()))
        if best - rsum < 0.0:        # the cores are apart (the candidates are a superset of the exact SAT axes): minus their distance
            best = rsum - _core_distance(A, B)
            n = _unit(B.center - A.center)[0] if np.any(B.center != A.center) else n
        return best, n, 1e-12 * (1.0 + max(A.size, B.size) + float(np.abs(np.concatenate([A.pts, B.pts])).max()))
    from scipy.optimize import minimize
    dirs = fibonacci_sphere(2562)
    allv = np.concatenate([cand, dirs])
    fv = np.concatenate([vals, _f(A, B, dirs)])
    order = np.argsort(fv)[:3]
    if fv[order[0]] < -0.25 * (A.size + B.size):   # clearly apart: the sampled value (an upper bound) is all any check needs
        return float(fv[order[0]]), allv[order[0]], 0.25 * (A.size + B.size)

    def g(x):
        v = x / max(np.linalg.norm(x), 1e-300)
        return float(_f(A, B, v[None])[0])
    for j in order:
        r = minimize(g, allv[j], method="Nelder-Mead", options={"xatol": 1e-13, "fatol": 1e-15, "maxiter": 4000})
        if r.fun < best:
            best, n = float(r.fun), r.x / np.linalg.norm(r.x)
    return best, n, CYLINDER_DEPTH_ERR_REL * (1.0 + max(A.size, B.size))


def point_signed_distance(s, p):
    """exact signed distance from points p [k, 3] to shape s (negative inside)."""
    p = np.atleast_2d(np.asarray(p, np.float64))
    if s.kind == SPHERE:
        return np.linalg.norm(p - s.pts[0], axis=1) - s.radius
    if s.kind == CAPSULE:
        return point_segment_distance(p, s.pts[0], s.pts[1]) - s.radius
    if s.kind == CYLINDER:
        a, b, r = s.cyl
        L = float(np.linalg.norm(b - a)); u = (b - a) / L
        t = (p - a) @ u
        rho = np.linalg.norm((p - a) - t[:, None] * u, axis=1)
        dax, drad = np.abs(t - 0.5 * L) - 0.5 * L, rho - r
        return np.minimum(np.maximum(dax, drad), 0.0) + np.hypot(np.maximum(dax, 0.0), np.maximum(drad, 0.0))
    tri = s.triangles()
    nrm = s.normals if s.kind == HULL else None
    if nrm is None:
        t = tri
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    plane = ((p[:, None, :] - tri[None, :, 0, :]) * nrm[None]).sum(-1).max(axis=1)
    out = point_triangle_distance(p[:, None, :], tri[None]).min(axis=1)
    return np.where(plane <= 0, plane, out)


def box_local_frame(s):
    """(rotation R with local axes as columns, centre, half extents) of an AABB / OBB shape."""
    if s.kind == AABB:
        lo, hi = s.pts.min(axis=0), s.pts.max(axis=0)
        return np.eye(3), 0.5 * (lo + hi), 0.5 * (hi - lo)
    R = s.normals.T
    c = s.pts.mean(axis=0)
    h = np.abs((s.pts - c) @ R).max(axis=0)
    return R, c, h


# ---------------------------------------------------------------------------------------------------------------------------
# Broadphase brute force
# ---------------------------------------------------------------------------------------------------------------------------
def brute_force_pairs(aabbs):
    """keys (hi << 32 | lo) of every collider pair whose [min, max] boxes overlap inclusively (aabbVsAABB): O(n^2) in blocks."""
    a = np.asarray(aabbs, np.float32)
    lo, hi = a[:, 0:3], a[:, 3:6]
    valid = np.all(lo <= hi, axis=1)
    keys = []
    n = len(a)
    for s in range(0, n, 512):
        i = np.arange(s, min(n, s + 512))
        ov = np.all((hi[i, None, :] >= lo[None, :, :]) & (lo[i, None, :] <= hi[None, :, :]), axis=2)
        ov &= (np.arange(n)[None, :] > i[:, None]) & valid[i, None] & valid[None, :]
        ii, jj = np.nonzero(ov)
        keys.append((jj.astype(np.uint64) << np.uint64(32)) | i[ii].astype(np.uint64))
    return np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# Edge-case batteries: deterministic scenes.Scene worlds (instantiate on mi.World and oracle.OracleWorld alike)
# ---------------------------------------------------------------------------------------------------------------------------
MATERIAL = (0.1, 0.5, 1.0)
BASES = (0.0, 1e3, -1e3, 1e4, -1e4, 1e5, -1e5)
KINDS = ("sphere", "capsule", "cylinder", "aabb", "obb", "hull")
TYPE_PAIRS = [(a, b) for i, a in enumerate(KINDS) for b in KINDS[i:]]
GAPS = (("touch", 0.0), ("gap+1e-6", 1e-6), ("gap-1e-6", -1e-6), ("gap+1e-4", 1e-4), ("gap-1e-4", -1e-4))
NEAR_PARALLEL = (("cos0.99+1e-4", math.acos(0.99 + 1e-4)), ("cos0.99-1e-4", math.acos(0.99 - 1e-4)), ("angle1e-5", 1e-5))


def fibonacci_hull(n):
    """n points on the unit sphere (Fibonacci) and their convex hull's outward triangles."""
    from scipy.spatial import ConvexHull
    v = fibonacci_sphere(n)
    tris = ConvexHull(v).simplices.copy()
    t = v[tris]
    flip = (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) * t.mean(axis=1)).sum(axis=1) < 0
    tris[flip] = tris[flip][:, ::-1]
    return v, tris


def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


def _qaxis(axis, angle):
    s = math.sin(0.5 * angle)
    return (axis[0] * s, axis[1] * s, axis[2] * s, math.cos(0.5 * angle))


def _local(kind, variant, scale, geoms):
    """(type, body-local shape tuple) of one battery collider."""
    if kind == "sphere":
        return SPHERE, (0, 0, 0, 0.5 * scale)
    if kind in ("capsule", "cylinder"):
        h, r = (5.0, 0.01) if variant == "long" else (0.5 * scale, (0.3 if kind == "capsule" else 0.4) * scale)   # long: 10 m / 2 cm = 1:500
        return (CAPSULE if kind == "capsule" else CYLINDER), (0, -h, 0, 0, h, 0, r)
    if kind in ("aabb", "obb"):
        he = (0.5 * scale, 1e-3, 0.45 * scale) if variant == "thin" else (0.5 * scale, 0.4 * scale, 0.45 * scale)
        return (AABB, (-he[0], -he[1], -he[2], he[0], he[1], he[2])) if kind == "aabb" else (OBB, (0, 0, 0, 1, 0, 0, 0) + he)
    return HULL, (0, 0, 0, 1, 0, 0, 0, float(geoms[variant if variant in geoms else ("s30" if scale > 1 else ("s1e-2" if scale < 1 else "std"))]))


def _posed(ctype, shape, q, hulls):
    """float64 Shape of a battery collider on a body at the origin with rotation q (for placing pairs; AABBs ignore q)."""
    R = quat_to_matrix(q)
    s = np.asarray(shape, np.float64)
    rec = {"type": ctype, "shape": np.zeros(10, np.float32)}
    if ctype == SPHERE:
        rec["shape"][:4] = [*(R @ s[0:3]), s[3]]
    elif ctype in (CAPSULE, CYLINDER):
        rec["shape"][:7] = [*(R @ s[0:3]), *(R @ s[3:6]), s[6]]
    elif ctype == AABB:
        rec["shape"][:6] = s[:6]
    else:
        rec["shape"][:len(s)] = s
        rec["shape"][0:4] = _qmul(q, tuple(s[0:4]))
    return shape_from_record(rec, hulls)


def narrow_battery():
    """[(name, Scene, cases)] one world per collider type pair; a case = dict(a, b (collider indices), label, variant, base, scale).
    Variants: std (scale 1) at every base coordinate; s1e-2 and s30 (shape scale 1 cm / 30 m; 1 cm shapes stay at |base| <= 1e4,
    where float32 still holds a 1 cm cylinder's endpoints apart), thin (1 mm half-extent boxes) and
    long (1:500 capsules / cylinders) at three bases; hull42 / hull162 (Fibonacci hulls) for the pairs with a hull.  Configurations:
    exact touching along +y, gaps of +-1e-6 and +-1e-4 m, B's centre inside A, coincident centres, a random pose, axes at
    cos = 0.99 +- 1e-4 and 1e-5 rad side by side, and (box-like pairs) edge on edge at 1 degree."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from directx_renderer_kurth_amd import scenes
    out = []
    for ka, kb in TYPE_PAIRS:
        rng = scenes.XorShift64(0x9E3779B97F4A7C15 ^ (KINDS.index(ka) * 8 + KINDS.index(kb)))
        s = scenes.Scene("edges_%s_%s" % (ka, kb))
        geoms = {}
        if "hull" in (ka, kb):
            v42, t42 = fibonacci_hull(42); v162, t162 = fibonacci_hull(162)
            for name, (v, t) in (("std", scenes.hull_icosahedron(0.55)), ("s1e-2", (v42 * 0.005, t42)), ("s30", (v42 * 15.0, t42)),
                                 ("hull42", (v42 * 0.5, t42)), ("hull162", (v162 * 0.5, t162)), ("box", scenes.hull_box(0.5, 0.5, 0.5)),
                                 ("oct", scenes.hull_octahedron(0.6)), ("thin", scenes.hull_box(0.5, 1e-3, 0.45))):
                geoms[name] = s.add_hull_geometry(v, t)
        hulls = s.hulls
        variants = [("std", 1.0, BASES), ("s1e-2", 1e-2, (0.0, 1e3, -1e4)), ("s30", 30.0, (0.0, 1e4, -1e5))]
        if {"aabb", "obb", "hull"} & {ka, kb}:
            variants.append(("thin", 1.0, (0.0, -1e3, 1e4)))
        if {"capsule", "cylinder"} & {ka, kb}:
            variants.append(("long", 1.0, (0.0, 1e3, -1e4)))
        if "hull" in (ka, kb):
            variants += [("hull42", 1.0, (0.0, 1e5)), ("hull162", 1.0, (0.0, -1e4)), ("box", 1.0, (0.0,)), ("oct", 1.0, (0.0,))]
        cases = []
        cursor = 0.0
        for variant, scale, bases in variants:
            ta, sa = _local(ka, variant, scale, geoms)
            tb, sb = _local(kb, variant, scale, geoms)
            for base in bases:
                configs = []
                I = (0.0, 0.0, 0.0, 1.0)
                for label, gap in GAPS:
                    configs.append((label, I, I, ("y", gap)))
                rq = lambda kind: I if kind == "aabb" else tuple(float(x) for x in rng.unit_quat())
                configs.append(("deep", rq(ka), rq(kb), ("inside", 0.3)))
                configs.append(("coincident", rq(ka), rq(kb), ("inside", 0.0)))
                configs.append(("random", rq(ka), rq(kb), ("random", 0.8)))
                for label, ang in NEAR_PARALLEL:
                    q = I if "aabb" in (ka, kb) else rq(ka)
                    configs.append((label, q, _qmul(q, _qaxis((1.0, 0.0, 0.0) if kb != "aabb" else (0.0, 0.0, 1.0), ang)) if kb != "aabb" else q,
                                    ("side", -1e-3 * scale, q)))
                if variant in ("std", "thin", "box") and ka in ("aabb", "obb", "hull") and kb in ("obb", "hull"):
                    qa = I if ka == "aabb" else _qaxis((0.0, 0.0, 1.0), math.pi / 4)
                    qb = _qmul(_qaxis((0.0, 1.0, 0.0), math.radians(1.0)), _qaxis((0.0, 0.0, 1.0), math.pi / 4))
                    configs.append(("edge1deg", qa, qb, ("y", -1e-3 * scale)))
                for label, qa, qb, (mode, amount, *rest) in configs:
                    A, B = _posed(ta, sa, qa, hulls), _posed(tb, sb, qb, hulls)
                    if mode == "y":
                        off = np.array([0.0, A.support(np.array([0.0, 1.0, 0.0]))[0] + B.support(np.array([0.0, -1.0, 0.0]))[0] + amount, 0.0])
                    elif mode == "inside":
                        d = np.array([rng.between(-1, 1), rng.between(-1, 1), rng.between(-1, 1)]); d /= max(np.linalg.norm(d), 1e-9)
                        off = d * amount * float(min(-A.support(-d[None])[0], A.support(d[None])[0], A.size))
                    elif mode == "random":
                        d = np.array([rng.between(-1, 1), rng.between(-1, 1), rng.between(-1, 1)]); d /= max(np.linalg.norm(d), 1e-9)
                        off = d * amount * (A.size + B.size)
                    else:   # side by side along the first body's local x
                        x = quat_to_matrix(rest[0])[:, 0]
                        off = x * (A.support(x[None])[0] + B.support(-x[None])[0] + amount)
                    span = 2.0 * (A.size + B.size) + 4.0
                    cursor += span
                    pa = (base + cursor, base + 5.0, base - 0.5 * cursor) if base else (cursor, 5.0, -0.5 * cursor)
                    a = s.add_body(pa, qa)
                    b = s.add_body(tuple(np.float32(np.float64(np.float32(p)) + o) for p, o in zip(pa, off)), qb)
                    ia = s.add_collider(a, ta, sa, MATERIAL)
                    ib = s.add_collider(b, tb, sb, MATERIAL)
                    cases.append(dict(a=ia, b=ib, label=label, variant=variant, base=base, scale=scale))
                    cursor += span
        out.append((s.name, s, cases))
    return out


def broad_battery():
    """[(name, Scene, expect)] broadphase grid edges; `expect` names what each world must exercise (checked by the tests), and
    `ties` the number of inclusive pairs the reference's sweep drops because their endpoints tie on its sorting axis (counted by
    the oracle on these worlds: every touching lattice face that lies across the sorting axis)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from directx_renderer_kurth_amd import scenes
    I = (0.0, 0.0, 0.0, 1.0)
    out = []
    # 1. lattice of unit cubes (extent = maxExtent = 1): one lattice with faces on multiples of the cell size (k * 1.001, gaps of 1e-3)
    #    and one of touching neighbours (faces shared exactly), both signs of every coordinate; statics of extent 1 - 1e-6, 1, 1 + 1e-6
    #    (the boundary of the "large" list) touching and crossing the lattice.
    s = scenes.Scene("bp_lattice")
    cell = float(np.float32(1.0) * np.float32(1.001))
    for origin, pitch in (((-3.0, -3.0, -3.0), 1.0), ((20.0, -20.0, 20.0), cell), ((-1000.0, 1000.0, -1000.0), 1.0)):
        for i in range(6):
            for j in range(6):
                for k in range(6):
                    lo = np.float32(np.array(origin) + pitch * np.array([i, j, k]))
                    b = s.add_body(tuple(float(x) for x in lo + np.float32(0.5)), I)
                    s.add_collider(b, AABB, (-0.5, -0.5, -0.5, 0.5, 0.5, 0.5), MATERIAL)
    for n, e in enumerate((np.float32(1.0) - np.float32(1e-6), np.float32(1.0), np.float32(1.0) + np.float32(1e-6))):
        for x0 in (-3.0, 0.0, 2.5):
            lo = (x0, -3.0 + 2.0 * n, 0.0)
            s.add_collider(STATIC_BODY, AABB, (lo[0], lo[1], lo[2], float(np.float32(lo[0]) + e), lo[1] + 0.5, lo[2] + 0.5), MATERIAL)
    out.append((s.name, s, {"touching": True, "large_boundary": True, "ties": 2570}))
    # 2. one sphere with more than 32 partners (the MODE_WRITE pass), and groups exactly 1024 cells apart on every axis
    s = scenes.Scene("bp_partners_alias")
    c = s.add_body((0.0, 0.0, 0.0), I)
    s.add_collider(c, SPHERE, (0, 0, 0, 0.5), MATERIAL)
    dirs = fibonacci_sphere(40)
    for d in dirs:
        b = s.add_body(tuple(float(x) for x in d * 0.6), I)
        s.add_collider(b, SPHERE, (0, 0, 0, 0.2), MATERIAL)
    cell = float(np.float32(1.0) * np.float32(1.001))
    for sign in (1.0, -1.0):
        for k in range(4):
            p = np.array([3.0 + k * 0.9, -2.0, 5.0]) * sign
            for shift in (0.0, 1024.0, 2048.0):
                b = s.add_body(tuple(float(x) for x in np.float32(p + sign * shift * cell)), I)
                s.add_collider(b, SPHERE, (0, 0, 0, 0.5), MATERIAL)
            b = s.add_body(tuple(float(x) for x in np.float32(p + sign * np.array([1025.0, 1024.0, 1023.0]) * cell)), I)
            s.add_collider(b, SPHERE, (0, 0, 0, 0.5), MATERIAL)
    out.append((s.name, s, {"max_partners": 33, "ties": 0}))
    # 3. 1 cm colliders at +-2e4 m: |x| / cell > 2^20 there, beyond the CELL_BIAS clamp (every collider clamps into one cell per axis)
    s = scenes.Scene("bp_clamp")
    for corner in ((2e4, 2e4, -2e4), (-2e4, -2e4, 2e4), (2e4, -3e4, 1.0), (-25000.0, 0.5, -0.25)):
        for i in range(5):
            for j in range(4):
                for k in range(3):
                    p = np.float32(np.array(corner) + np.array([i * 0.008, j * 0.0095, k * 0.01]))
                    b = s.add_body(tuple(float(x) for x in p), I)
                    s.add_collider(b, SPHERE, (0, 0, 0, 0.005), MATERIAL)
    out.append((s.name, s, {"clamped": True, "ties": 0}))
    return out


STATIC_BODY = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------
# Float64 invariants of reported manifolds (shared by the oracle test and the device test)
# ---------------------------------------------------------------------------------------------------------------------------
def pair_tolerance(A, B, err64):
    """1e-5 (1 + |coord| / 1 m) plus the float64 reference's own stated error."""
    coord = float(np.abs(np.concatenate([A.pts, B.pts])).max())
    return 1e-5 * (1.0 + coord) + err64


# The reference formulas behind the cases where a reported contact lies beyond the plain float64 bounds, restated in float64 so that
# check_manifolds can assert their exact shape instead of widening a bound.
def _tube_axis(s):
    return (s.pts[0], s.pts[1]) if s.kind == CAPSULE else (s.cyl[0], s.cyl[1])


def _tube_radius(s):
    return s.radius if s.kind == CAPSULE else s.cyl[2]


def cap_disc_point(cyl, c):
    """sphereCylinder's end-cap branch (collision_narrow.cpp:408-449) for a sphere centred at c beyond a cap: the point of that cap's
    disc nearest to c (its `closestToSphere`), or None when c projects onto the side (0 <= t <= 1: the sphere-sphere branch)."""
    a, b, r = cyl.cyl
    ab = b - a
    t = float(np.dot(c - a, ab) / np.dot(ab, ab))
    if 0.0 <= t <= 1.0:
        return None
    p, u = (a, ab) if t <= 0.0 else (b, ab)
    u = u / np.linalg.norm(u)
    radial = (c - p) - np.dot(c - p, u) * u
    n = np.linalg.norm(radial)
    return p + (radial * min(1.0, r / n) if n > 0 else radial)


def sphere_cylinder_cap_points(centres, cyl, depth):
    """collision_narrow.cpp:445: point = closestToSphere + 0.5 depth (closestToSphere - centre), the normal BEFORE normalisation."""
    out = []
    for c in centres:
        q = cap_disc_point(cyl, c)
        if q is not None:
            out.append(q + 0.5 * depth * (q - c))
    return out


def parallel_tube_points(A, B):
    """capsule vs capsule / cylinder with |cos| > 0.99 and overlapping axis intervals (collision_narrow.cpp:545-600): the two points
    midway between contactA on A's AXIS and its nearest point on B's AXIS, at the ends of the overlap; None if that branch is not taken."""
    a0, a1 = _tube_axis(A); b0_, b1_ = _tube_axis(B)
    L = float(np.linalg.norm(a1 - a0)); ad = (a1 - a0) / L
    bd = (b1_ - b0_) / np.linalg.norm(b1_ - b0_)
    cos = float(np.dot(ad, bd))
    if abs(cos) <= 0.99:
        return None
    pBa, pBb = (b1_, b0_) if cos < 0 else (b0_, b1_)
    left, right = max(0.0, float(np.dot(ad, pBa - a0))), min(L, float(np.dot(ad, pBb - a0)))
    if right < left:
        return None
    cA0, cA1 = a0 + left * ad, a0 + right * ad
    cB0 = _closest_on_segments(cA0, pBa, pBb)
    cB1 = cB0 + (right - left) * ad
    return [0.5 * (cA0 + cB0), 0.5 * (cA1 + cB1)]


def tube_box_clip_shape(A, B, c, tol):
    """capsule / cylinder vs AABB / OBB after GJK + EPA, when EPA's normal n lies within 0.99 of a box axis and across the tube
    (|n . axis| < 0.01; collision_narrow.cpp:731-768, cylinders :979-1010): the tube's surface segment [a + r n, b + r n] is clipped to the box's side
    planes and projected onto the REFERENCE plane through the box corner on the -n side with normal -n (getAABBReferencePlane
    :291-299, bounding_volumes.h:166) — EPA's normal, not the face's.  Each point lies on that plane and point - depth (-n) on the
    surface segment; the depth is therefore measured to a plane tilted from the face by EPA's residual angle.  Returns None when the
    branch is not taken, else whether every point has that shape."""
    n = c["normal"][0].astype(np.float64)
    R, cB, h = box_local_frame(B)
    nl = R.T @ n
    a0, a1 = _tube_axis(A)
    u = (a1 - a0) / np.linalg.norm(a1 - a0)
    if not (np.abs(nl).max() > 0.99 and abs(float(np.dot(n, u))) < 0.01):
        return None
    corner = cB + R @ np.where(-nl < 0, -h, h)
    r = _tube_radius(A)
    ok = True
    for p, d in zip(c["point"].astype(np.float64), c["depth"].astype(np.float64)):
        on_plane = abs(float(np.dot(-n, p - corner))) <= tol
        s = p + n * d                                       # point = s + (-n) depth
        on_surface = float(point_segment_distance(s, a0 + r * n, a1 + r * n)) <= tol
        ok = ok and on_plane and on_surface
    return ok


def box_face_sat_depth(A, B):
    """(parallel, face-only depth) of the reference's OBB SAT (collision_narrow.cpp:1216-1226): when
    some |R_ij| + 1e-6 >= 0.99 the nine edge axes are skipped and the depth is the least overlap over the six face axes."""
    RA, cA, hA = box_local_frame(A)
    RB, cB, hB = box_local_frame(B)
    r = RA.T @ RB
    t = RA.T @ (cB - cA)
    ar = np.abs(r)
    pen = [hA[i] + float(ar[i] @ hB) - abs(t[i]) for i in range(3)] + [float(ar[:, i] @ hA) + hB[i] - abs(float(r[:, i] @ t)) for i in range(3)]
    return bool(ar.max() + 1e-6 >= 0.99), min(pen)


def check_manifolds(cols, hulls, manifolds, must_collide=()):
    """manifolds: [(a, b, contacts CONTACT_DTYPE[count])] with a, b as the narrowphase ordered them (count > 0); must_collide:
    ordered (a, b) pairs that the float64 depth is computed for even without a manifold.  Returns (report, failures, misses): report
    maps 'typeA-typeB' to the worst (depth excess over float64, point distance excess, |normal| error) and the quirk counts; misses
    are the must_collide pairs without a manifold that float64 finds overlapping by more than tol: (family, a, b, depth, tol)."""
    report, failures = {}, []
    got = {(int(a), int(b)): c for a, b, c in manifolds}
    cache = {}

    def shapes(a, b):
        if (a, b) not in cache:
            A, B = shape_from_record(cols[a], hulls), shape_from_record(cols[b], hulls)
            d, n, err = signed_depth(A, B)
            assert np.isfinite(d) and np.isfinite(err), ("float64 depth not finite", a, b, d)
            cache[(a, b)] = (A, B, d, n, err, pair_tolerance(A, B, err))
        return cache[(a, b)]

    for (a, b), c in got.items():
        A, B, d64, n64, err, tol = shapes(a, b)
        fam = "%s-%s" % (TYPE_NAMES[A.kind], TYPE_NAMES[B.kind])
        r = report.setdefault(fam, {"manifolds": 0, "depth_excess": -np.inf, "point_excess": -np.inf, "normal_err": 0.0, "aabb_signed": 0, "sphere_inside_box": 0, "max_tol": 0.0})
        r["manifolds"] += 1; r["max_tol"] = max(r["max_tol"], tol)
        pts = c["point"].astype(np.float64); dep = c["depth"].astype(np.float64); nrm = c["normal"].astype(np.float64)
        if not (np.isfinite(pts).all() and np.isfinite(dep).all() and np.isfinite(nrm).all()):
            failures.append((fam, a, b, "non-finite contact")); continue
        nerr = float(np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max())
        r["normal_err"] = max(r["normal_err"], nerr)
        if nerr > 1e-5:
            failures.append((fam, a, b, "normal length off by %.3g" % nerr))
        if A.kind == AABB and B.kind == AABB:
            # quirk: the depth carries the sign of the centres' offset on the least-overlap axis (collision_narrow.cpp:1092-1093)
            axis = int(np.argmax(np.abs(nrm[0])))
            sgn = 1.0 if (B.center - A.center)[axis] >= 0 else -1.0
            ok = np.all(np.abs(np.abs(dep) - d64) <= tol) and np.all(np.sign(dep[dep != 0]) == sgn) and np.allclose(nrm, sgn * np.eye(3)[axis], atol=0)
            if not ok:
                failures.append((fam, a, b, "AABB-AABB signed depth %s vs float64 %.9g, axis %d sign %g" % (dep, d64, axis, sgn)))
            r["aabb_signed"] += int(np.any(dep < 0))
            # quirk, same lines: the points lie on the plane centreA + radiusA - depth / 2 along that axis, whatever the sign, so a
            # negative depth puts them half a depth outside A's upper face instead of inside the overlap; that shape is asserted
            # and the points are measured against the overlap rectangle on the other two axes only
            lo, hi = A.pts.min(axis=0).astype(np.float32), A.pts.max(axis=0).astype(np.float32)
            plane = (np.float32(0.5) * (lo[axis] + hi[axis]) + np.float32(0.5) * (hi[axis] - lo[axis])) - c["depth"] * np.float32(0.5)
            if not np.all(np.abs(c["point"][:, axis].astype(np.float64) - plane) <= tol):
                failures.append((fam, a, b, "AABB-AABB contact points off the plane centreA + radiusA - depth / 2"))
            pts = pts.copy(); pts[:, axis] = np.clip(pts[:, axis], max(A.pts[:, axis].min(), B.pts[:, axis].min()), min(A.pts[:, axis].max(), B.pts[:, axis].max()))
            dep = np.abs(dep)
        if A.kind == SPHERE and B.kind in (AABB, OBB):
            R, cB, h = box_local_frame(B)
            local = (A.pts[0] - cB) @ R
            if np.all(np.abs(local) < h):
                # quirk: a sphere centre inside the box gives depth = radius and normal = the box's local +y (collision_narrow.cpp:451-491)
                ok = len(dep) == 1 and float(c["depth"][0]) == np.float32(A.radius) and np.allclose(nrm[0], R[:, 1], atol=1e-6)
                if not ok:
                    failures.append((fam, a, b, "sphere centre inside the box: depth %s normal %s" % (dep, nrm)))
                r["sphere_inside_box"] += 1
        fam_box = A.kind in (CAPSULE, CYLINDER) and B.kind in (AABB, OBB)
        clip = tube_box_clip_shape(A, B, c, tol) if fam_box else None
        bound = d64
        if clip is not None:
            # tube vs box through the clipping branch: its exact shape replaces the depth bound (see tube_box_clip_shape)
            r["tube_box_clip"] = r.get("tube_box_clip", 0) + 1
            if not clip:
                failures.append((fam, a, b, "tube-box clipping contact off the reference plane / surface segment"))
            bound = np.inf
        elif A.kind in (AABB, OBB) and B.kind == OBB:
            parallel, d_face = box_face_sat_depth(A, B)
            if parallel and d_face > d64:
                # the SAT skips the edge axes when two box axes are within 0.99 (collision_narrow.cpp:1216-1226): the face-only depth,
                # with the reference's 1e-6 added to |R| on every face axis
                r["sat_parallel"] = r.get("sat_parallel", 0) + 1
                bound = d_face + 1e-6 * float(np.abs(np.concatenate([A.pts, B.pts]) - np.concatenate([A.pts, B.pts]).mean(axis=0)).max()) * 6
        if np.isfinite(bound):
            excess = float(dep.max() - bound)
            r["depth_excess"] = max(r["depth_excess"], excess)
            if excess > tol:
                failures.append((fam, a, b, "depth %.9g exceeds float64 %.9g by %.3g > tol %.3g" % (dep.max(), bound, excess, tol)))
        sa, sb = point_signed_distance(A, pts), point_signed_distance(B, pts)
        pex = np.maximum(sa, sb) - np.abs(dep)
        # points whose position is the reference's own formula (asserted exactly instead of bounded): sphere / capsule end sphere
        # vs cylinder cap (collision_narrow.cpp:445), nearly parallel capsule vs capsule / cylinder (:545-600), tube-box clipping
        formula = []
        if B.kind == CYLINDER and A.kind in (SPHERE, CAPSULE):
            centres = [A.pts[0]]
            if A.kind == CAPSULE:   # its end spheres (parallel branch) and closestSegmentSegment's point on its axis (general branch)
                from scipy.optimize import minimize_scalar
                p1, p2 = A.pts[0], A.pts[1]
                t = minimize_scalar(lambda t: float(point_segment_distance(p1 + t * (p2 - p1), B.cyl[0], B.cyl[1])), bounds=(0.0, 1.0), method="bounded", options={"xatol": 1e-13}).x
                centres = [p1, p2, p1 + t * (p2 - p1)]
            formula += sphere_cylinder_cap_points(centres, B, float(np.abs(dep).max()))
        if A.kind == CAPSULE and B.kind in (CAPSULE, CYLINDER):
            formula += parallel_tube_points(A, B) or []
        bad = pex > tol
        excused = np.zeros(len(bad), bool)
        if clip:
            excused[:] = bad; bad[:] = False
        for i in np.nonzero(bad)[0]:
            if any(float(np.linalg.norm(pts[i] - f)) <= tol for f in formula):
                bad[i] = False; excused[i] = True
                r["formula_points"] = r.get("formula_points", 0) + 1
        if (~bad & ~excused).any():
            r["point_excess"] = max(r["point_excess"], float(pex[~bad & ~excused].max()))
        if bad.any():
            failures.append((fam, a, b, "contact point %.3g outside a shape beyond its depth (tol %.3g) and not at the reference's formula" % (float(pex[bad].max()), tol)))
    misses = []
    for a, b in must_collide:
        a, b = int(a), int(b)
        if (a, b) in got or (b, a) in got:
            continue
        A, B, d64, n64, err, tol = shapes(a, b)
        fam = "%s-%s" % (TYPE_NAMES[A.kind], TYPE_NAMES[B.kind])
        r = report.setdefault(fam, {"manifolds": 0, "depth_excess": -np.inf, "point_excess": -np.inf, "normal_err": 0.0, "aabb_signed": 0, "sphere_inside_box": 0, "max_tol": 0.0})
        r["missed_depth"] = max(r.get("missed_depth", -np.inf), d64)
        if d64 > tol:
            misses.append((fam, a, b, d64, tol))
    return report, failures, misses


GJK_FAMILIES = ("capsule-aabb", "capsule-obb", "cylinder-cylinder", "cylinder-aabb", "cylinder-obb") + tuple("%s-hull" % k for k in KINDS)


def centrally_symmetric(s, tol):
    """the shape equals its reflection through its centre (spheres, capsules, cylinders and boxes always; hulls checked)."""
    if s.kind != HULL:
        return True
    refl = 2.0 * s.center - s.pts
    d = np.linalg.norm(refl[:, None, :] - s.pts[None, :, :], axis=2).min(axis=1)
    return bool(d.max() <= tol)


def assert_misses_are_gjk_coincident(misses, cols, hulls):
    """Quirk: for two centrally symmetric shapes with coincident centres the GJK test reports no intersection — its second support
    point is the first one mirrored, the search direction cross(cross(c - b, -b), c - b) is zero and the loop exits on
    |dir|^2 < 1e-4 (collision_gjk.h:183-238).  Every pair float64 finds overlapping without a manifold must be such a case: a GJK
    family, both shapes centrally symmetric, centres equal to within tol."""
    bad = []
    for fam, a, b, d64, tol in misses:
        A, B = shape_from_record(cols[a], hulls), shape_from_record(cols[b], hulls)
        ok = fam in GJK_FAMILIES and centrally_symmetric(A, tol) and centrally_symmetric(B, tol) and float(np.linalg.norm(A.center - B.center)) <= tol
        if not ok:
            bad.append((fam, a, b, d64, tol))
    assert not bad, bad[:10]
    return len(misses)
