"""Collision detection on the device at the poses and scales no scene reaches (tests/geom64.py batteries), against the oracle,
a brute-force pair set and the float64 geometry.  Each world is stepped once with step_internal(1e-9, 1), as
test_gpu_golden.test_narrow_pairs_golden does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g  # noqa: E402
from parity_util import pair_set  # noqa: E402

pytestmark = pytest.mark.gpu
CAPS = {"gjk_max_iters": 64, "epa_max_triangles": 128, "epa_max_edges": 160, "epa_max_border": 32}


def _step_both(mi, oracle, scene):
    w = scene.instantiate(mi.World())
    o = scene.instantiate(oracle.OracleWorld()); o.use_hull_geometries()
    w.step_internal(1e-9, 1); o.step_internal(1e-9, 1)
    cols, aabbs = w.world_colliders()
    ocols, oaabbs = o.world_colliders()
    for f in ("shape", "restitution", "friction", "type", "objectIndex"):
        assert np.array_equal(cols[f].view(np.uint32), ocols[f].view(np.uint32)), f
    assert np.array_equal(aabbs.view(np.uint32), oaabbs.view(np.uint32))
    return w, o, cols, aabbs


def _pairs_against_brute_force(w, o, aabbs):
    """device pair set == brute force on the device's own AABBs; == the oracle's sweep except the endpoint ties it drops."""
    dev, brute, orc = pair_set(w.pairs()), g.brute_force_pairs(aabbs), pair_set(o.pairs())
    assert len(w.pairs()) == len(dev)                       # no pair twice
    assert np.array_equal(dev, brute), (len(np.setdiff1d(dev, brute)), len(np.setdiff1d(brute, dev)))
    assert len(np.setdiff1d(orc, dev)) == 0
    extra = np.setdiff1d(dev, orc)
    i = (extra & np.uint64(0xFFFFFFFF)).astype(np.int64); j = (extra >> np.uint64(32)).astype(np.int64)
    axis = o.sorting_axis()[0]
    tie = (aabbs[i, 3 + axis] == aabbs[j, axis]) | (aabbs[j, 3 + axis] == aabbs[i, axis])
    assert tie.all()
    return len(dev), int(len(extra))


@pytest.mark.parametrize("index", range(3))
def test_broadphase_grid_edges(mi, oracle, index):
    """Touching lattices with faces on cell multiples, statics at maxExtent x (1 - 1e-6, 1, 1 + 1e-6), a collider with 40 partners
    (the MODE_WRITE pass), colliders 1024 cells apart (cellTag aliasing) and 1 cm colliders beyond the CELL_BIAS clamp: the device's
    pair set equals the brute-force inclusive set, and the world exercises what it was built for."""
    name, scene, expect = g.broad_battery()[index]
    w, o, cols, aabbs = _step_both(mi, oracle, scene)
    n, ties = _pairs_against_brute_force(w, o, aabbs)
    ext = (aabbs[:, 3:6] - aabbs[:, 0:3]).max(axis=1)
    dynamic = cols["objectType"] == 0
    max_extent = float(ext[dynamic].max())
    lo, hi = aabbs[:, 0:3], aabbs[:, 3:6]
    touching = int(sum(np.sum(hi[:, None, k] == lo[None, :, k]) for k in range(3)))
    print("%s: %d pairs = brute force; %d excused endpoint ties in the oracle's sweep (expected %d); maxExtent %.9g; faces touching exactly: %d" % (name, n, ties, expect["ties"], max_extent, touching))
    assert ties == expect["ties"]
    if expect.get("touching"):
        assert touching > 100
    if expect.get("large_boundary"):
        st = ext[~dynamic]
        assert (st < max_extent).any() and (st == max_extent).any() and (st > max_extent).any()
    if expect.get("max_partners"):
        p = w.pairs().astype(np.int64)
        assert np.bincount(p.reshape(-1)).max() >= expect["max_partners"]
    if expect.get("clamped"):
        cell = float(np.float32(max_extent) * np.float32(1.001))
        assert np.abs(lo).max() / cell > 2 ** 20


@pytest.mark.parametrize("pair", ["%s-%s" % p for p in g.TYPE_PAIRS])
def test_narrowphase_edges(mi, oracle, pair):
    """Per type pair, the narrowphase battery: world colliders and AABBs bit-equal to the oracle's, pair set = brute force, device
    manifolds = oracle.narrowphase_ordered on the device's ordered pairs (counts and friction/restitution exact, point / depth /
    normal within 1e-5 (1 + |coord|)), the float64 invariants of test_oracle_geometry, and the GJK / EPA high-water marks equal to
    the oracle's over the same pairs, below their caps, with no out-of-memory exit."""
    from test_oracle_geometry import print_report
    idx = [i for i, p in enumerate(g.TYPE_PAIRS) if "%s-%s" % p == pair][0]
    name, scene, cases = g.narrow_battery()[idx]
    w, o, cols, aabbs = _step_both(mi, oracle, scene)
    _pairs_against_brute_force(w, o, aabbs)
    slots, counts, contacts, _ = w.manifolds()
    oracle.stats_reset()
    exp, ecounts = oracle.narrowphase_ordered(cols, slots)
    assert np.array_equal(counts.astype(np.int64), ecounts.astype(np.int64))
    dev = w.narrow_limits(); orc = oracle.stats()
    print(name, "device GJK/EPA marks:", dev, "oracle's:", orc, "caps:", CAPS)
    assert dev == orc, (dev, orc)
    for k, cap in CAPS.items():
        assert dev[k] < cap, (k, dev[k], cap)
    assert dev["epa_out_of_memory"] == 0
    start = np.concatenate([[0], np.cumsum(ecounts.astype(np.int64))])
    worst_abs, worst_rel = {}, 0.0
    manifolds = []
    for i, (a, b) in enumerate(slots):
        c = int(counts[i])
        if not c:
            continue
        got, ref = contacts[i][:c], exp[start[i]:start[i + 1]]
        assert np.array_equal(got["friction_restitution"], ref["friction_restitution"])
        scale = 1.0 + float(np.abs(ref["point"]).max())
        fam = "%s-%s" % (g.TYPE_NAMES[cols["type"][a]], g.TYPE_NAMES[cols["type"][b]])
        for f in ("point", "depth", "normal"):
            d = float(np.abs(got[f].astype(np.float64) - ref[f]).max())
            worst_abs[(fam, f)] = max(worst_abs.get((fam, f), 0.0), d)
            worst_rel = max(worst_rel, d / scale)
        manifolds.append((int(a), int(b), got))
    print(name, "device vs oracle, worst |difference| per field:", {"%s %s" % k: "%.3g" % v for k, v in sorted(worst_abs.items())},
          "| worst relative to 1 + |coord|: %.3g (bound 1e-5)" % worst_rel)
    assert worst_rel <= 1e-5
    report, failures, misses = g.check_manifolds(cols, scene.hulls, manifolds, [(c["a"], c["b"]) for c in cases])
    print_report(name + " (device vs float64)", report, misses)
    assert not failures, failures[:10]
    g.assert_misses_are_gjk_coincident(misses, cols, scene.hulls)
