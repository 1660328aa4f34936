"""spherecast64 itself: the float64 reading against closed forms (a ray against the shape inflated by the radius, plane offsets,
inflated segments and points), the battery's classification, the float32 restatement of csrc/sphere_cast.h against the reading with
the measured table the device test takes its tolerances from, the iteration budget, and the new symbols in the header.  No GPU."""
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402
import spherecast64 as s64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = (0.0, 0.0, 0.0, 1.0)


def _cand(ctype, *v, hulls=()):
    s = np.zeros(10, np.float32); s[:len(v)] = v
    return s64.Cand(0, 0, ctype, s, (0, 0, 0), IDENT, hulls)


def _ray_sphere(o, d, ce, r):
    """first t of the ray o + t d on the sphere (ce, r), None without one (float64, closed form)"""
    o, d, ce = (np.asarray(x, np.float64) for x in (o, d, ce))
    a, b, c = d @ d, 2.0 * (d @ (o - ce)), (o - ce) @ (o - ce) - r * r
    disc = b * b - 4 * a * c
    if disc < 0:
        return None
    t = (-b - math.sqrt(disc)) / (2 * a)
    return t if t >= 0 else None


def _ray_capsule(o, d, a, b, r):
    """first t on the capsule: the infinite cylinder's root if it lies between the ends, else the nearer end sphere"""
    o, d, a, b = (np.asarray(x, np.float64) for x in (o, d, a, b))
    u = (b - a) / np.linalg.norm(b - a)
    op, dp = (o - a) - ((o - a) @ u) * u, d - (d @ u) * u
    best = None
    A, B, C = dp @ dp, 2 * (dp @ op), op @ op - r * r
    if A > 0 and B * B - 4 * A * C >= 0:
        t = (-B - math.sqrt(B * B - 4 * A * C)) / (2 * A)
        if t >= 0 and 0 <= ((o + t * d) - a) @ u <= np.linalg.norm(b - a):
            best = t
    for e in (a, b):
        t = _ray_sphere(o, d, e, r)
        if t is not None and (best is None or t < best):
            best = t
    return best


def test_reading_against_closed_forms():
    hulls = [r64.BRICK]
    checks = []
    # sphere and capsule targets: a ray against the shape inflated by the radius
    for o, d, rad in (((5, 0.3, -0.2), (-1, 0, 0), 0.25), ((4, 3, 0), (-2, -1.4, 0.1), 0.375), ((0, 6, 0.7), (0, -0.5, 0), 0.0)):
        checks.append((_cand(s64.SPHERE, 0.125, 0.25, -0.125, 0.5), o, d, rad, _ray_sphere(o, d, (0.125, 0.25, -0.125), 0.5 + rad)))
        checks.append((_cand(s64.CAPSULE, 0, -1, 0, 0, 1, 0, 0.25), o, d, rad, _ray_capsule(o, d, (0, -1, 0), (0, 1, 0), 0.25 + rad)))
    # box faces: a plane offset.  AABB (-1, -2, -3) .. (1, 2, 3): from x = 5 straight and obliquely onto the face x = 1
    box = _cand(s64.AABB, -1, -2, -3, 1, 2, 3)
    checks.append((box, (5, 0.5, 0.5), (-1, 0, 0), 0.25, 5 - 1.25))
    checks.append((box, (5, 0.5, 0.5), (-2, 0.2, -0.1), 0.25, (5 - 1.25) / 2))
    checks.append((_cand(s64.OBB, *IDENT, 1, 1, 1, 1, 2, 3), (1, 1, 9), (0, 0, -1), 0.5, 9 - 4.5))
    checks.append((_cand(s64.HULL, *IDENT, 0, 0, 0, 0, hulls=hulls), (0.2, 4, 0.1), (0, -1, 0), 0.25, 4 - 0.75))
    # box edges and corners: inflated segments and points.  Past the edge x = 1, y = 2 (parallel to z) and towards the corner (1, 2, 3)
    checks.append((box, (5, 2.1, 0), (-1, 0, 0), 0.25, _ray_capsule((5, 2.1, 0), (-1, 0, 0), (1, 2, -3), (1, 2, 3), 0.25)))
    checks.append((box, (5, 2.1, 3.1), (-1, 0, 0), 0.25, _ray_sphere((5, 2.1, 3.1), (-1, 0, 0), (1, 2, 3), 0.25)))
    checks.append((box, (5, 2.3, 0), (-1, 0, 0), 0.25, None))
    # a cylinder's cap is a plane offset, its side an inflated infinite cylinder
    cyl = _cand(s64.CYLINDER, 0, 0, 0, 0, 2, 0, 1)
    checks.append((cyl, (0.3, 7, 0.2), (0, -1, 0), 0.25, 7 - 2.25))
    checks.append((cyl, (6, 1, 0.5), (-1, 0, 0), 0.25, 6 - math.sqrt(1.25 ** 2 - 0.25)))
    for c, o, d, rad, want in checks:
        got = s64.candidate64(c, np.array(o, np.float64), np.array(d, np.float64), rad, math.inf)
        assert (got.t is None) == (want is None), (c.type, o, d, got.t, want)
        if want is not None:
            assert abs(got.t - want) <= 1e-10 * (1 + want), (c.type, o, d, got.t, want)
            dist, _, n = c.contact(*c.local(np.array(o, np.float64), np.array(d, np.float64)), got.t)
            assert abs(dist - rad) <= 1e-10 and abs(got.cos + float(n @ np.asarray(d, np.float64)) / np.linalg.norm(d)) <= 1e-12
        else:
            assert got.clearance > 0
    # maxT cuts the path, a start inside is t = 0, a zero direction is an overlap test
    c, o, d = checks[0][0], np.array(checks[0][1], np.float64), np.array(checks[0][2], np.float64)
    assert s64.candidate64(c, o, d, 0.25, checks[0][4] - 1e-6).t is None and s64.candidate64(c, o, d, 0.25, checks[0][4] + 1e-6).t is not None
    assert s64.candidate64(c, np.array([0.1, 0.2, 0.3]), d, 0.25, math.inf).t == 0.0
    assert s64.candidate64(c, o, np.zeros(3), 0.25, math.inf).t is None and s64.candidate64(c, np.array([0.1, 0.9, -0.1]), np.zeros(3), 0.25, math.inf).t == 0.0


def test_battery_is_classified_and_under_the_cap():
    cw, cases = s64.battery()
    kinds = s64.classify()
    expected = s64.battery_expected()
    counts = {k: len(v) for k, v in kinds.items()}
    print(len(cases), counts)
    assert len(cases) >= 140 and sum(counts.values()) == len(cases)
    assert counts["undecided"] <= s64.UNDECIDED_CAP * len(cases)
    assert counts["hit"] >= 80 and counts["miss"] >= 15 and counts["inside"] >= 10
    families = {c.family for c in cases}
    for need in ("head-on", "oblique", "shallow", "graze", "past", "past-edge", "past-vertex", "inside", "inside-touch", "touch", "radius-zero", "huge-radius", "max-t",
                 "zero-direction", "non-unit", "receding", "head-on-1cm", "head-on-30m", "head-on@1e3", "head-on@-1e3"):
        assert need in families, need
    assert {expected[i].type for i in kinds["hit"]} == set(range(6))
    by_name = {c.id: (c, e) for c, e in zip(cases, expected)}
    for kind in range(6):
        name = s64.TYPE_NAMES[kind]
        assert by_name["max-t/%s-short" % name][1].kind == "miss" and by_name["max-t/%s-beyond" % name][1].kind == "hit" and by_name["max-t/%s-inf" % name][1].kind == "hit"
        assert by_name["past/" + name][1].kind == "miss" and by_name["receding/" + name][1].kind == "miss"
        assert by_name["head-on/%s-0" % name][1].cos > by_name["shallow/" + name][1].cos > s64.COS_MIN
        long, short = by_name["non-unit/%s-long" % name][1], by_name["non-unit/%s-short" % name][1]
        assert abs(long.t * 2.5 - short.t * 0.01) <= 1e-9 * short.t and long.kind == short.kind == "hit"
    assert all(by_name["zero-direction/%s-%s" % (s64.TYPE_NAMES[k], "inside" if k % 2 else "outside")][1].kind == ("inside" if k % 2 else "miss") for k in range(6))


def test_float32_restatement_decides_like_float64():
    """hits stop inside [t* - tol / (L cos), t*] up to the measured rounding and on the same collider; misses miss; inside starts report
    t = 0 with a negative gap; nothing uses up SC_MAX_ITER"""
    cw, cases = s64.battery()
    kinds, expected, got = s64.classify(), s64.battery_expected(), s64.battery_restated()
    for i in kinds["hit"]:
        c, e, (a, _) = cases[i], expected[i], got[i]
        assert a is not None and a[0] == s64.HIT and a[2] == e.collider and a[3] == e.body, (c.id, a)
        lo, hi = s64.t_window(e)
        R = s64.tolerance(s64.family_of(c, e))[0] * s64.scale_of(c, e) / e.L
        assert lo - R <= float(a[1]) <= hi + R, (c.id, a[1], lo, hi, R)
        assert float(a[5]) <= e.tol * (1 + 1e-6), (c.id, a[5], e.tol)
    for i in kinds["miss"]:
        assert got[i][0] is None, (cases[i].id, got[i])
    for i in kinds["inside"]:
        a = got[i][0]
        assert a is not None and a[0] == s64.HIT and a[1] == 0 and a[5] < 0 and a[2] == expected[i].collider and a[7] == 1, (cases[i].id, a)
    for i in kinds["undecided"]:           # one of the rule's two answers: nothing, or a stop on the path with a gap within the tolerance
        a = got[i][0]
        assert a is None or (a[0] == s64.HIT and float(a[5]) <= 2 * s64.SC_GAP), (cases[i].id, a)
    most = max(m for _, m in got)
    print("most samples over the battery:", most)
    assert most == s64.MAX_ITER_BATTERY and all(a is None or a[0] != s64.UNRESOLVED for a, _ in got)
    assert s64.SC_MAX_ITER == 1 << math.ceil(math.log2(2 * max(s64.MAX_ITER_BATTERY, s64.MAX_ITER_RANDOM)))


def test_measured_float32_table():
    """spherecast64.E_F32 is the measurement, within 1.5 x either way (figures below an eighth of an ulp are not held from below)."""
    measured = s64.measure_f32()
    for k, m in sorted(measured.items()):
        print('    "%s": (%s),' % (k, ", ".join("%.2g" % v for v in m)))
    assert set(measured) == set(s64.E_F32)
    for fam, m in measured.items():
        for got, stated in zip(m, s64.E_F32[fam]):
            assert got <= 1.5 * stated and (got >= stated / 1.5 or stated <= 0.125 * s64.F32_EPS), (fam, m, s64.E_F32[fam])
        assert all(t >= 4 * s64.F32_EPS for t in s64.tolerance(fam))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "directx-renderer-kurth_amd", "csrc", "sphere_cast.h")).read()
    assert float(re.search(r"#define SC_GAP ([0-9.e-]+)f", text).group(1)) == s64.SC_GAP
    assert float(re.search(r"#define SC_GUARD_ULPS ([0-9.]+)f", text).group(1)) == s64.SC_GUARD_ULPS
    assert int(re.search(r"#define SC_MAX_ITER ([0-9]+)u", text).group(1)) == s64.SC_MAX_ITER


def test_new_symbols_are_declared_and_exported(mi):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_physics.h")).read(), flags=re.S)
    for name in ("mi_sphere_cast_batch", "mi_sphere_cast_host"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in mi.EXPORTED_SYMBOLS and hasattr(mi.load_library(), name)
    assert re.search(r"MI_SPHERE_STATIC = 1, MI_SPHERE_BRUTE_FORCE = 2", text)
    import ctypes
    assert ctypes.sizeof(mi.SphereCast) == 48 == mi.SPHERE_CAST_DTYPE.itemsize and ctypes.sizeof(mi.SphereHit) == 48 == mi.SPHERE_HIT_DTYPE.itemsize
    assert (mi.SPHERE_STATIC, mi.SPHERE_BRUTE_FORCE) == (1, 2) and callable(mi.World.sphere_cast)
