"""tests/contact_sensor64.py on hand-made arrays: the rule of mi_contact_sensors where every sum can be checked by hand, and the float32
evaluation against the float64 one on a long segment (the rounding yardstick recorded in the module)."""
import numpy as np
import pytest

import contact_sensor64 as cs

BOTH = cs.DYNAMIC | cs.STATIC
NB = 6            # bodies 0..5; 6 is the static dummy


def _world():
    """Position: (A, B, count, slot).  Body 1 is B of slot 7 and A of slot 2; body 0 touches the dummy twice."""
    ids = np.array([[0, 1, 1, 7], [1, 2, 2, 2], [0, NB, 3, 5], [NB, 0, 4, 1], [3, 4, 1, 9]], np.uint32)
    normal = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [0.75, -0.5, 0]], np.float32)   # (not a unit vector: every value stays exact)
    rows = np.zeros((5, 4, 15), np.float32)
    lam = np.zeros((5, 4, 2), np.float32)
    for p in range(5):
        for k in range(int(ids[p, 2])):
            rows[p, k, 0:3] = (1, 0, 0) if p != 1 else (0, 0, 1)                                  # t
            rows[p, k, 3:6], rows[p, k, 6:9] = (0.5, 0, 0), (0, 0.25, 0)                          # rA x t, rB x t
            rows[p, k, 9:12], rows[p, k, 12:15] = (0, 0, 2), (0, 0, -4)                           # rA x n, rB x n
            lam[p, k] = (1.0 + p + 0.5 * k, 0.125 * (p + 1))
    return ids, normal, rows, lam


def _both(sensors, world=None, dead=()):
    ids, normal, rows, lam = world or _world()
    r32 = cs.evaluate32(ids, normal, rows, lam, sensors, NB, dead)
    r64 = cs.evaluate64(ids, normal, rows, lam, sensors, NB, dead)
    for f in ("impulse", "normalImpulse", "angularImpulse"):   # all values here are exact in float32
        assert np.array_equal(r32[f].astype(np.float64), r64[f]), f
    for f in ("numContacts", "numManifolds", "strongestPartner", "valid"):
        assert np.array_equal(r32[f], r64[f]), f
    return r32


def test_record_sizes():
    assert cs.SENSOR_DTYPE.itemsize == 16 and cs.READING_DTYPE.itemsize == 48


def test_sign_for_a_and_b():
    r = _both([[3, BOTH, 0, 0], [4, BOTH, 0, 0]])
    # position 4: ln = 5, lt = 0.625, n = (0.75, -0.5, 0), t = (1, 0, 0): B gets +, A gets -
    want = np.float32(5.0) * np.array([0.75, -0.5, 0], np.float32) + np.float32(0.625) * np.array([1, 0, 0], np.float32)
    assert np.array_equal(r["impulse"][1], want) and np.array_equal(r["impulse"][0], -want)
    assert np.array_equal(r["angularImpulse"][0], -np.array([0.5 * 0.625, 0, 2 * 5.0], np.float32))   # A: -(ln rA x n + lt rA x t)
    assert np.array_equal(r["angularImpulse"][1], np.array([0, 0.25 * 0.625, -4 * 5.0], np.float32))  # B: +(ln rB x n + lt rB x t)
    assert r["normalImpulse"].tolist() == [5.0, 5.0] and r["strongestPartner"].tolist() == [4, 3]
    assert r["numContacts"].tolist() == [1, 1] and r["numManifolds"].tolist() == [1, 1] and r["valid"].tolist() == [1, 1]


def test_body_that_is_a_and_b():
    r = _both([[1, BOTH, 0, 0]])[0]
    # B of position 0 (ln 1, lt .125, n y, t x): +(0.125, 1, 0); A of position 1, two contacts (ln 2, 2.5; lt .25; n x, t z): -(4.5, 0, 0.5)
    assert r["impulse"].tolist() == [0.125 - 4.5, 1.0, -0.5]
    assert r["normalImpulse"] == 1.0 + 2.0 + 2.5 and r["numContacts"] == 3 and r["numManifolds"] == 2
    assert r["strongestPartner"] == 2      # 4.5 against 1


def test_partner_classes():
    r = _both([[0, cs.STATIC, 0, 0], [0, cs.DYNAMIC, 0, 0], [0, BOTH, 0, 0], [0, 0, 0, 0]])
    assert r["numManifolds"].tolist() == [2, 1, 3, 0] and r["numContacts"].tolist() == [7, 1, 8, 0]
    assert r["valid"].tolist() == [1, 1, 1, 1]
    assert r["strongestPartner"].tolist() == [cs.STATIC_BODY, 1, cs.STATIC_BODY, 0]
    assert not r["impulse"][3].any() and r["normalImpulse"][3] == 0.0
    # the static part and the dynamic part add up to the whole where every value is exact
    assert np.array_equal(r["impulse"][0] + r["impulse"][1], r["impulse"][2])
    assert r["normalImpulse"][0] + r["normalImpulse"][1] == r["normalImpulse"][2]


def test_counts_one_to_four():
    ids, normal, rows, lam = _world()
    for p, body, partner_class in ((0, 0, cs.DYNAMIC), (1, 2, cs.DYNAMIC), (2, 0, cs.STATIC), (3, 0, cs.STATIC)):
        keep = [p]
        r = _both([[body, partner_class, 0, 0]], (ids[keep], normal[keep], rows[keep], lam[keep]))[0]
        count = int(ids[p, 2])
        assert r["numContacts"] == count == p + 1 and r["numManifolds"] == 1
        assert r["normalImpulse"] == sum(1.0 + p + 0.5 * k for k in range(count))


def test_exclusion_wraps():
    s = lambda first, count: [1, cs.DYNAMIC, first, count]   # body 1 has partners 0 and 2
    r = _both([s(0, 0), s(0, 1), s(2, 1), s(0, 3), s(0xFFFFFFFF, 2), s(2, 0xFFFFFFFF), s(3, 0xFFFFFFFF)])
    # (0xFFFFFFFF, 2) wraps to {0xFFFFFFFF, 0}: partner 0 goes; (2, 0xFFFFFFFF) is every index but 1 (0 - 2 wraps inside the range): both
    # partners go; (3, 0xFFFFFFFF) is every index but 2: partner 2 stays
    assert r["numManifolds"].tolist() == [2, 1, 1, 0, 1, 0, 1]
    assert r["strongestPartner"].tolist() == [2, 2, 0, 0, 2, 0, 2]
    # the static dummy is never excluded
    r = _both([[0, BOTH, 0, 0xFFFFFFFF], [0, BOTH, NB, 1]])
    assert r["numManifolds"].tolist() == [2, 3]


def test_several_sensors_per_body_and_invalid_ones():
    r = _both([[0, BOTH, 0, 0], [0, BOTH, 0, 0], [NB, BOTH, 0, 0], [77, BOTH, 0, 0], [5, BOTH, 0, 0], [2, BOTH, 0, 0]], dead=[2])
    assert r[0].tobytes() == r[1].tobytes()
    assert r["valid"].tolist() == [1, 1, 0, 0, 1, 0]
    assert r[2].tobytes() == bytes(48) and r[3].tobytes() == bytes(48) and r[5].tobytes() == bytes(48)
    assert r[4]["numManifolds"] == 0 and r[4].tobytes() == np.array([(0, 0, 0, 0, 0, 0, 1, 0)], cs.READING_DTYPE).tobytes()


def test_strongest_partner_tie_goes_to_the_lowest_slot():
    ids = np.array([[0, 1, 1, 9], [0, 2, 2, 3], [3, 0, 1, 6], [0, 4, 1, 8]], np.uint32)
    normal = np.tile(np.array([0, 1, 0], np.float32), (4, 1))
    rows = np.zeros((4, 4, 15), np.float32)
    lam = np.zeros((4, 4, 2), np.float32)
    lam[0, 0, 0], lam[1, 0, 0], lam[1, 1, 0], lam[2, 0, 0], lam[3, 0, 0] = 2.0, 0.75, 1.25, 2.0, 1.0
    r = _both([[0, BOTH, 0, 0], [0, BOTH, 2, 1], [0, BOTH, 2, 2]], (ids, normal, rows, lam))
    assert r["strongestPartner"].tolist() == [2, 3, 1]    # three manifolds sum to 2.0: slot 3 wins, without it slot 6, then slot 9


def test_order_is_slot_then_contact():
    """Three terms whose float32 sum depends on the order: 1e8, 1 and -1e8 in slot order give 0, in position order 1."""
    ids = np.array([[1, 0, 1, 5], [2, 0, 1, 9], [3, 0, 1, 2]], np.uint32)   # slots 2, 5, 9 are positions 2, 0, 1
    normal = np.tile(np.array([0, 1, 0], np.float32), (3, 1))
    rows = np.zeros((3, 4, 15), np.float32)
    lam = np.zeros((3, 4, 2), np.float32)
    lam[2, 0, 0], lam[0, 0, 0], lam[1, 0, 0] = 1e8, 1.0, 1e8
    normal[1] = (0, -1, 0)
    r = cs.evaluate32(ids, normal, rows, lam, [[0, BOTH, 0, 0]], 4)[0]
    assert r["impulse"][1] == 0.0                            # (1e8 + 1) - 1e8 in float32
    assert cs.evaluate64(ids, normal, rows, lam, [[0, BOTH, 0, 0]], 4)[0]["impulse"][1] == 1.0


def test_rounding_yardstick_of_2100_manifolds():
    ids, normal, rows, lam, nb = cs.synthetic_segment()
    sensor = [[0, BOTH, 0, 0]]
    r32, r64 = cs.evaluate32(ids, normal, rows, lam, sensor, nb)[0], cs.evaluate64(ids, normal, rows, lam, sensor, nb)[0]
    assert r32["numManifolds"] == r64["numManifolds"] == 2100 and r32["numContacts"] == r64["numContacts"] == int(ids[:, 2].sum())
    assert r32["strongestPartner"] == r64["strongestPartner"]
    figures = {}
    for f in ("impulse", "angularImpulse", "normalImpulse"):
        a, b = np.atleast_1d(r32[f]).astype(np.float64), np.atleast_1d(r64[f])
        figures[f] = float(np.abs(a - b).max() / np.abs(b).max())
    print("float32 against float64 on 2 100 manifolds, relative to the sum:", figures)
    worst = max(figures.values())
    assert cs.ROUNDING_2100 / 2.0 <= worst <= cs.ROUNDING_2100, (figures, cs.ROUNDING_2100)
    # a float32 sum of N terms of one sign loses at most about N ulps / 2 of its final value and typically sqrt(N): the figure sits between
    n = int(r32["numContacts"])
    assert 2.0 ** -24 <= worst <= n * 2.0 ** -24
