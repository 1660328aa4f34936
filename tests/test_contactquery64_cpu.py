"""tests/contactquery64.py, the expectation of the contact queries, checked on the CPU in float64: per type pair of geom64.narrow_battery()
the expectation is built in both roles (a as the volume with b in the world, b as the volume with a in the world), every manifold is
held to geom64.check_manifolds and every miss to assert_misses_are_gjk_coincident.  No case is left out and no failure is allowed.
Then the reporting rules on a hand-made world: the sign rule, ascending order, truncation, the deepest contact, switched-off queries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contactquery64 as c64  # noqa: E402
import geom64 as g  # noqa: E402
import overlap64 as o64  # noqa: E402


def _twin(oracle, cw):
    return cw.instantiate(oracle.OracleWorld())


@pytest.mark.parametrize("pair", ["%s-%s" % p for p in g.TYPE_PAIRS])
def test_battery_both_roles_in_float64(oracle, pair):
    idx = [i for i, p in enumerate(g.TYPE_PAIRS) if "%s-%s" % p == pair][0]
    name, scene, cases, cw, qs = c64.battery_world(idx)
    assert len(qs) == 2 * len(cases)
    e = c64.expectation(oracle, _twin(oracle, cw), cw, qs, 4)
    assert (e.summary["valid"] == 1).all()
    nc = len(cw.colliders)
    every = []   # the ordered pair of every case in both roles, whether its boxes meet or not: none is left out of the float64 check
    for k, c in enumerate(cases):   # every case is asked in both roles: against its partner if their boxes meet (stage 1 of the rule), and nothing else
        for role, (me, other) in enumerate(((c["a"], c["b"]), (c["b"], c["a"]))):
            pairs = e.ordered[2 * k + role]
            v = nc + 2 * k + role
            meet = not ((e.aabbs[other, 3:6] < e.aabbs[v, 0:3]) | (e.aabbs[other, 0:3] > e.aabbs[v, 3:6])).any()
            assert [(min(A, B), max(A, B)) for A, B, _, _ in pairs] == ([(other, v)] if meet else []), (k, role, [(A, B) for A, B, _, _ in pairs])
            assert np.array_equal(e.cols["shape"][v].view(np.uint32), e.cols["shape"][me].view(np.uint32))
            every.append((v, other) if e.cols["type"][v] <= e.cols["type"][other] else (other, v))
    manifolds, asked = c64.manifolds_of(e)
    assert len(cases) < len(asked) <= 2 * len(cases)   # (gaps of +1e-4 m part the boxes at small coordinates; most cases meet)
    assert set(asked) <= set(every) and len(every) == 2 * len(cases)
    report, failures, misses = g.check_manifolds(e.cols, scene.hulls, manifolds, every)
    print("%s: %d ordered pairs in both roles, %d with meeting boxes, %d manifolds, %d failures, %d misses" % (name, len(every), len(asked), len(manifolds), len(failures), len(misses)))
    for fam, r in sorted(report.items()):
        print("   %-20s %s" % (fam, {k: ("%.3g" % v if isinstance(v, float) else v) for k, v in r.items()}))
    assert not failures, failures[:10]
    g.assert_misses_are_gjk_coincident(misses, e.cols, scene.hulls)
    # the two roles of equal-type pairs are the two operand orders; of unequal types the same order with the sign rule applied once
    flipped = sum(1 for q in e.ordered for _, _, c, va in q if len(c) and not va)
    assert (flipped == 0) == (g.TYPE_PAIRS[idx][0] == g.TYPE_PAIRS[idx][1])


# ---- the reporting rules on a hand-made world ----------------------------------------------------------------------------------
BIG = (o64.AABB, (-1.5, -3, -3, 40, 3, 3))   # holds bodies 0 .. 7, the static box and the far sphere of overlap64.hand_world


def _hand(oracle, qs, max_hits, static=True):
    cw = o64.hand_world()
    return c64.expectation(oracle, _twin(oracle, cw), cw, qs, max_hits, static)


def test_hand_order_truncation_and_deepest(oracle):
    full = _hand(oracle, o64.query(*BIG), 16)
    s = full.summary[0]
    assert [int(r["collider"]) for r in full.all[0]] == [0, 1, 2, 3, 4, 6, 7, 8, 9]     # body 5 is deleted; 10 and 11 are zones
    assert (s["numContacts"], s["numWritten"], s["valid"]) == (9, 9, 1) and not full.records[0, 9:].view(np.uint32).any()
    depths = [float(r["maxDepth"]) for r in full.all[0]]
    best = int(np.argmax(depths))   # (argmax takes the first of equal values: the lower collider index)
    assert (s["deepestCollider"], s["deepestDepth"]) == (full.all[0][best]["collider"], np.float32(depths[best]))
    cut = _hand(oracle, o64.query(*BIG), 1)
    assert (cut.summary[0]["numContacts"], cut.summary[0]["numWritten"]) == (9, 1) and cut.records[0, 0]["collider"] == 0
    assert cut.summary[0]["deepestCollider"] == s["deepestCollider"]
    count = _hand(oracle, o64.query(*BIG), 0)
    assert count.blocks().shape == (1, 8) and count.blocks()[0].tolist() == [9, 0, 1, 0] + full.blocks()[0, 4:8].tolist()


def test_hand_sign_rule(oracle):
    """A sphere volume under body 1's sphere is operand A (equal types: the volume) and the normal points up, from the volume into the
    collider; a box volume there is operand B (sphere < aabb), the narrowphase's normal points from the sphere down into the box, and the
    reported one is flipped: up again.  Points and depths are the narrowphase's."""
    qs = o64.queries([o64.query(o64.SPHERE, (0, 0, 0, 1.0), (3.0, -1.5, 0.0)), o64.query(o64.AABB, (-1, -1, -1, 1, 1, 1), (3.0, -1.5, 0.0), exclude_first=0, exclude_count=0)])
    e = _hand(oracle, qs, 4, static=False)
    for k, va in ((0, True), (1, False)):
        (A, B, c, volume_is_a), = e.ordered[k]
        assert volume_is_a == va and e.records[k, 0]["collider"] == 1 and e.records[k, 0]["count"] == len(c) >= 1
        assert e.records[k, 0]["normal"][1] > 0.99
        assert np.array_equal(e.records[k, 0]["points"][:len(c), 3], c["depth"]) and np.array_equal(e.records[k, 0]["points"][:len(c), 0:3], c["point"])
        sign = 1.0 if va else -1.0
        assert np.array_equal(e.records[k, 0]["normal"], sign * c["normal"][0])


def test_hand_switched_off_and_empty(oracle):
    qs = o64.queries([o64.query(*BIG, enabled=0), o64.query(*BIG, mount=5), o64.query(o64.SPHERE, (0, 0, 0, 0.25), (0.0, 50.0, 0.0))])
    e = _hand(oracle, qs, 2)
    assert not e.blocks()[0:2].any()
    assert e.blocks()[2].tolist() == [0, 0, 1, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0] + [0] * 48
