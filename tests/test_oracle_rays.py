"""The CPU oracle's testPhysicsInteraction against the float64 reading of tests/ray64.py over the whole ray battery (no GPU).

Known-answer tests pin ray64's geometry to numbers worked out by hand; the battery is checked for what it promises (families,
size, share of undecided cases); then the oracle must push the body ray64 names on every decided case, with the force, the torque
and the hit distance inside the measured bounds of ray64.MEASURED.  The measured figures are printed next to their bounds."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402

CASES = r64.ray_battery()


def shape(t, *s):
    return r64.shape_from_record(t, np.array(list(s) + [0.0] * (10 - len(s)), np.float32), [r64.BRICK])


def test_kat_first_hit():
    """first_hit against distances worked out by hand"""
    t, m = r64.first_hit(shape(r64.SPHERE, 0, 0, 0, 0.5), (-3, 0.3, 0), (1, 0, 0))
    assert abs(t - (3 - 0.4)) <= 1e-12 and abs(m - 0.8 / 0.5) <= 1e-12                          # chord 2 * sqrt(0.25 - 0.09) = 0.8
    assert r64.first_hit(shape(r64.SPHERE, 0, 0, 0, 0.5), (-3, 0.5, 0), (1, 0, 0))[1] <= 1e-7    # tangent: margin 0
    assert r64.first_hit(shape(r64.SPHERE, 0, 0, 0, 0.5), (-3, 0.75, 0), (1, 0, 0)) == (None, 0.5)
    t, m = r64.first_hit(shape(r64.AABB, -1, -0.5, -0.75, 1, 0.5, 0.75), (-5, 0.25, 0.5), (2, 0, 0))
    assert abs(t - 2.0) <= 1e-12                                                                # a direction of length 2: t in its units
    t, m = r64.first_hit(shape(r64.OBB, 0, 0, math.sin(math.pi / 8), math.cos(math.pi / 8), 0, 0, 0, 1, 1, 1), (-5, 0, 0), (1, 0, 0))
    assert abs(t - (5 - math.sqrt(2))) <= 1e-6                                                  # a cube turned by 45 degrees: hit on its edge
    t, m = r64.first_hit(shape(r64.CYLINDER, 0, -1, 0, 0, 1, 0, 0.5), (0.25, 4, 0), (0, -1, 0))
    assert abs(t - 3.0) <= 1e-12 and abs(m - 0.25 / 1.5) <= 1e-12                                # the cap; 0.25 from the side it runs along
    t, m = r64.first_hit(shape(r64.CYLINDER, 0, -1, 0, 0, 1, 0, 0.5), (-3, 0.5, 0), (1, 0, 0))
    assert abs(t - 2.5) <= 1e-12
    t, m = r64.first_hit(shape(r64.CAPSULE, 0, -1, 0, 0, 1, 0, 0.5), (0, 4, 0), (0, -1, 0))
    assert abs(t - 2.5) <= 1e-12                                                                # the end sphere, before the cylinder's cap
    t, m = r64.first_hit(shape(r64.HULL, 0, 0, 0, 1, 0, 0, 0, 0), (0.6, 0.1, 5), (0, 0, -1))
    assert abs(t - 4.25) <= 1e-12
    assert r64.first_hit(shape(r64.HULL, 0, 0, 0, 1, 0, 0, 0, 0), (0.6, 0.6, 5), (0, 0, -1))[0] is None


def test_kat_reference_rules():
    sph, box, cyl = shape(r64.SPHERE, 0, 0, 0, 0.5), shape(r64.AABB, -1, -1, -1, 1, 1, 1), shape(r64.CYLINDER, 0, -1, 0, 0, 1, 0, 0.5)
    assert r64.reference_hit(sph, np.array([0.1, 0, 0]), np.array([1.0, 0, 0]))[0] == 0.0                       # R1
    assert r64.reference_hit(box, np.array([0.1, 0, 0]), np.array([1.0, 0, 0]))[0] is None                      # R2
    assert r64.reference_hit(box, np.array([-1.0, 3, 0]), np.array([0, -1.0, 0])) == (None, 1.0)                # R2a
    assert r64.reference_hit(box, np.array([-1.0, 0.5, 0]), np.array([1.0, 0, 0]))[0] is None                   # R2b, looking in
    assert r64.reference_hit(box, np.array([-1.0 - 2.0 ** -30, 0.5, 0]), np.array([1.0, 0, 0]))[0] == 2.0 ** -30           # ... and only exactly there
    assert abs(r64.reference_hit(shape(r64.HULL, 0, 0, 0, 1, 0, 0, 0, 0), np.array([0.2, 0.1, 0]), np.array([0, 0, 1.0]))[0] - 0.75) <= 1e-12   # R3
    assert abs(r64.reference_hit(cyl, np.array([0.1, 3, 0]), np.array([0, 1.0, 0]))[0] + 4.0) <= 1e-12         # R4: the lower disk, behind
    assert r64.reference_hit(cyl, np.array([0.1, 3, 0]), np.array([1.0, 0, 0]))[0] is None                      # R4: no disk, outside the ends
    assert r64.reference_hit(cyl, np.array([0.1, 0.5, 0]), np.array([1.0, 0, 0]))[0] == 0.0                     # R4: no disk, between the ends
    assert r64.reference_hit(shape(r64.CAPSULE, 1, 1, 1, 1, 1, 1, 0.5), np.array([-2.0, 1, 1]), np.array([1.0, 0, 0]))[0] == 2.5   # R6


def test_battery_is_what_it_promises(oracle):
    fams = {c.family for c in CASES}
    for need in ["posed-" + n for n in r64.TYPE_NAMES] + ["inside-" + n for n in r64.TYPE_NAMES] + [
            "box-axis-aligned", "box-on-face", "parallel-box-slab-plane", "edge-box", "vertex-box", "box-through-corner", "tangent-sphere", "sphere", "axis+y",
            r64.ANTIPARALLEL, "axis-skew", "cylinder-cap", "edge-cylinder-rim", "cylinder-perpendicular", "cylinder-behind", "unwritten-t",
            "capsule-degenerate", "edge-hull", "vertex-hull", "parallel-hull-face", "hull-back-face", "hull-two-geometries", "far-1e3",
            "scale-1cm", "scale-100m", "tie", "nothing"]:
        assert need in fams, need
    scenes = r64.scenes_of(CASES)
    assert sum(len(s.bodies) for s, _ in scenes) <= 200 and max(len(s.bodies) for s, _ in scenes) <= r64.MAX_BODIES_PER_CASE
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def run(oracle):
    got = r64.run_whole_world(CASES, oracle.OracleWorld, lambda w: w.accumulators(), lambda w: w.last_interaction_distance())
    return [(c, c.scene.expect(c.ray, g[2]), g) for c, g in zip(CASES, got)]


def test_undecided_cases_are_few_and_knife_edge(run):
    undecided = [c.id for c, e, g in run if not e.decided]
    print("%d cases, %d undecided: %s" % (len(run), len(undecided), undecided))
    assert len(undecided) <= 0.15 * len(run)
    assert all(c.knife_edge for c, e, g in run if not e.decided), [c.id for c, e, g in run if not e.decided and not c.knife_edge]


def test_oracle_pushes_the_decided_body(run):
    wrong = [(c.id, e.body, g[0]) for c, e, g in run if e.decided and e.body != g[0]]
    assert not wrong, wrong


def test_oracle_push_within_the_measured_bounds(run):
    worst = {}
    for c, e, g in run:
        if not e.decided or e.body is None:
            continue
        et, ef, eq = r64.errors(c, e, g[1], g[3])
        w = worst.setdefault(c.family, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], et), max(w[1], ef), max(w[2], eq)
    print("family: measured now (t, force, torque) | table (t, torque) | bound = 4 x table")
    for f in sorted(worst):
        print("    %-28s %.3g %.3g %.3g | %s | %s" % (f, *worst[f], r64.MEASURED.get(f), r64.bound(f) if f in r64.MEASURED else None))
    assert set(worst) == set(r64.MEASURED), set(worst) ^ set(r64.MEASURED)
    for f, (et, ef, eq) in worst.items():
        bt, bq = r64.bound(f)
        assert ef <= 2.0 ** -24, (f, ef)            # the force is one rounded product per component
        assert et <= bt and eq <= bq, (f, et, bt, eq, bq)
        if max(r64.MEASURED[f]) > r64.WELL_CONDITIONED:
            assert f in r64.CONDITIONING, f
