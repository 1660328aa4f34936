"""The float64 side of the trigger / force-field overlap battery (tests/zone64.py), checked without a GPU: the oracle's overlapCheck on
the battery's world colliders against the restated rules, the battery's own cap on undecided cases, every disagreement between a rule
and the true depth attributed to a named rule, and the oracle's boxes containing their shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g  # noqa: E402
import zone64 as z  # noqa: E402


def _oracle_world(oracle, pairing):
    scene, zone_ids, body_ids = z.build_scene(pairing, "trigger")
    o = scene.instantiate(oracle.OracleWorld()); o.use_hull_geometries()
    o.step_internal(1e-9, 1)
    cols, aabbs = o.world_colliders()
    return o, cols, aabbs, zone_ids, body_ids


@pytest.mark.parametrize("pairing", z.PAIRINGS, ids=z.pairing_name)
def test_oracle_overlap_follows_the_rules(oracle, pairing):
    """Per ordered pairing (zone type, body type): overlap_ordered on the type-ordered pairs (both orders where the types are equal)
    equals the restated rule on every decided case; the battery keeps its cap (at most 15 % undecided, at least 6 decided cases of
    each sign); a rule that contradicts the sign of the true depth on a decided case belongs to a named rule."""
    o, cols, aabbs, zone_ids, body_ids = _oracle_world(oracle, pairing)
    cases = z.battery()[pairing]
    exp = z.evaluate(pairing, cols)
    assert len(cases) <= z.MAX_CASES
    ordered = np.array([(a, b) if cols["type"][a] <= cols["type"][b] else (b, a) for a, b in zip(zone_ids, body_ids)], np.uint32)
    flags = oracle.overlap_ordered(cols, ordered)
    flags_swapped = oracle.overlap_ordered(cols, ordered[:, ::-1]) if pairing[0] == pairing[1] else flags
    name = z.rule_of(*pairing)
    wrong, quirks, undecided, signs = [], [], 0, [0, 0]
    for k, (c, (rule, depth, tol, ok, overlap)) in enumerate(zip(cases, exp)):
        if not ok:
            undecided += 1
            continue
        signs[int(overlap)] += 1
        if bool(flags[k]) != overlap or bool(flags_swapped[k]) != overlap:
            wrong.append((k, c.tag, "oracle %s/%s, rule %s, depth %.6g, tol %.3g" % (flags[k], flags_swapped[k], overlap, depth, tol)))
        if overlap != (depth >= 0.0) and not c.exact:
            quirks.append((c.tag, "adds" if overlap else "loses", "depth %.4g" % depth))
    print("%s: %d cases, %d decided (%d apart, %d overlapping), %d undecided; rule %s; rule != sign(depth) on %d: %s"
          % (z.pairing_name(pairing), len(cases), len(cases) - undecided, signs[0], signs[1], undecided, name or "depth >= 0", len(quirks), quirks))
    assert not wrong, wrong
    assert undecided <= z.MAX_UNDECIDED_FRACTION * len(cases), (undecided, len(cases))
    assert min(signs) >= z.MIN_DECIDED_PER_SIGN, signs
    assert not quirks or name is not None, quirks


@pytest.mark.parametrize("pairing", z.PAIRINGS, ids=z.pairing_name)
def test_oracle_boxes_contain_their_shapes(oracle, pairing):
    """Every collider's box holds the float64 support extent of its shape along +-x, +-y, +-z, within 4 float32 ulps of the largest
    coordinate involved: a box a hair too tight drops a zone pair before the overlap test sees it."""
    o, cols, aabbs, zone_ids, body_ids = _oracle_world(oracle, pairing)
    hulls = z.hull_geometries()
    eye = np.eye(3)
    for i in range(len(cols)):
        s = g.shape_from_record(cols[i], hulls)
        hi, lo = s.support(eye), -s.support(-eye)
        slack = 4.0 * float(np.spacing(np.float32(max(np.abs(hi).max(), np.abs(lo).max(), np.abs(aabbs[i]).max()))))
        assert (aabbs[i, 0:3].astype(np.float64) <= lo + slack).all() and (aabbs[i, 3:6].astype(np.float64) >= hi - slack).all(), (i, z.battery()[pairing][i % len(zone_ids)].tag, aabbs[i], lo, hi)
