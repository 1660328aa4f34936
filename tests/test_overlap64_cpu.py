"""tests/overlap64.py, the expectation of the overlap queries, checked on the CPU: against zone64's float64 rules on its battery, on a
hand-made world (truncation, exclusion wrap-around, static flag, switched-off queries), and that the random world the GPU tests use is
not vacuous.  Then the float32 pose composition of mounted volumes against float64.

Largest error of compose32 against compose64 per family of mounts (metres for the position; the rotation as the largest component
error of the quaternion), as test_pose_composition_error prints it; the GPU tolerance for mounted volumes is 4 x the figure:
    family                              position      rotation
    rotations, offset ~1                3.2e-07       8.2e-08
    offset 1e3 (mount and volume)       1.6e-04       8.2e-08
    scale 1e-2                          3.9e-09       8.2e-08
    scale 1e2                           3.2e-05       8.2e-08
In units of 2^-24 x (|pos| + |mountPos|) the position errors are 1.16, 1.24, 1.21 and 1.29.  The bound they must stay under comes from
the arithmetic, not from these figures: the sandwich q * (p, 0) * conj(q) is two quaternion products of at most 6 roundings per
component each, every intermediate of magnitude <= |pos|, then one sum with mountPos: POSE_ULPS = 12 of those units; a quaternion
product of two unit quaternions has 4 products and 3 sums per component, all <= 1: within 4 x 2^-24."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap64 as o64  # noqa: E402
import raycast_util as ru  # noqa: E402
import zone64 as z  # noqa: E402

POSE_ULPS = 12.0   # x 2^-24 x (|pos| + |mountPos|): the stated bound of compose32's position; the GPU tolerance is 4 x the measured error


def _twin(oracle, cw):
    return cw.instantiate(oracle.OracleWorld())


@pytest.mark.parametrize("pairing", z.PAIRINGS, ids=z.pairing_name)
def test_battery_agrees_with_zone64(oracle, pairing):
    """Volume k = zone k of the battery, asked against all bodies: its verdict on body k agrees with zone64.evaluate wherever that is
    decided and the two boxes meet.  (The caps on undecided cases are test_zone64_cpu.py's.)"""
    cw, qs = o64.battery_world(pairing)
    n = len(qs)
    e = o64.expectation(oracle, _twin(oracle, cw), cw, qs, 8)
    assert (e.summary[:, 2] == 1).all()
    exp = z.evaluate(pairing, e.cols)
    wrong, checked = [], 0
    for k, (rule, depth, tol, ok, overlap) in enumerate(exp):
        if ok and k in e.boxpass[k]:
            checked += 1
            if (k in [c for c, _ in e.all[k]]) != bool(overlap):
                wrong.append((k, z.battery()[pairing][k].tag, depth, tol))
    print("%s: %d cases, %d decided with meeting boxes, %d overlapping" % (z.pairing_name(pairing), n, checked, sum(1 for k in range(n) if k in [c for c, _ in e.all[k]])))
    assert not wrong, wrong
    assert checked >= z.MIN_DECIDED_PER_SIGN


# ---- a hand-made world ---------------------------------------------------------------------------------------------------------
def _hand(oracle, qs, max_hits, static=True):
    cw = o64.hand_world()
    return o64.expectation(oracle, _twin(oracle, cw), cw, qs, max_hits, static)


BIG = (o64.AABB, (-1.5, -3, -3, 40, 3, 3))   # holds bodies 0 .. 7, the static box and the far sphere


def test_hand_truncation(oracle):
    full = _hand(oracle, o64.query(*BIG), 16)
    assert [c for c, _ in full.all[0]] == [0, 1, 2, 3, 4, 6, 7, 8, 9]   # body 5 is deleted; 10 and 11 are zones
    assert [b for _, b in full.all[0]] == [0, 1, 2, 3, 4, 6, 7, o64.STATIC_BODY, o64.STATIC_BODY]
    assert full.summary[0].tolist() == [9, 9, 1, 0] and not full.colliders[0, 9:].any()
    cut = _hand(oracle, o64.query(*BIG), 4)
    assert cut.summary[0].tolist() == [9, 4, 1, 0] and cut.colliders[0].tolist() == [0, 1, 2, 3]
    count = _hand(oracle, o64.query(*BIG), 0)
    assert count.summary[0].tolist() == [9, 0, 1, 0] and count.blocks().shape == (1, 4)


def test_hand_exclusion_wraps(oracle):
    qs = o64.queries([o64.query(*BIG, exclude_first=2, exclude_count=3), o64.query(*BIG, exclude_first=0xFFFFFFFE, exclude_count=4),
                      o64.query(*BIG, exclude_first=0, exclude_count=0xFFFFFFFF)])
    e = _hand(oracle, qs, 16)
    assert [c for c, _ in e.all[0]] == [0, 1, 6, 7, 8, 9]
    assert [c for c, _ in e.all[1]] == [2, 3, 4, 6, 7, 8, 9]       # 2^32 - 2, 2^32 - 1, 0, 1
    assert [c for c, _ in e.all[2]] == [8, 9]                      # static colliders are never excluded


def test_hand_static_flag_and_touch(oracle):
    e = _hand(oracle, o64.query(*BIG), 16, static=False)
    assert [c for c, _ in e.all[0]] == [0, 1, 2, 3, 4, 6, 7]
    # a sphere whose box touches body 1's box exactly (x = 4 .. 6 against 2 .. 4): the boxes meet, the spheres touch
    t = _hand(oracle, o64.query(o64.SPHERE, (0, 0, 0, 1.0), (5.0, 0.0, 0.0)), 4)
    assert [c for c, _ in t.all[0]] == [1, 2]


def test_hand_switched_off(oracle):
    nan = float("nan")
    qs = o64.queries([o64.query(*BIG), o64.query(6, BIG[1]), o64.query(o64.HULL, (0, 0, 0, 1, 0, 0, 0, 0.0)), o64.query(*BIG, pos=(nan, 0, 0)),
                      o64.query(*BIG, enabled=0), o64.query(*BIG, mount=5), o64.query(*BIG, mount=8), o64.query(*BIG, mount=0)])
    e = _hand(oracle, qs, 4)
    assert e.summary[:, 2].tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    assert not e.blocks()[1:7].any() and not e.shapes[1:7].any()
    assert e.blocks()[0].tolist() == e.blocks()[7].tolist()        # body 0 sits at the origin with the identity rotation


# ---- the random world ------------------------------------------------------------------------------------------------------------
def test_random_world_is_not_vacuous(oracle):
    cw, _ = ru.random_world()
    qs = o64.random_volumes()
    assert len(cw.colliders) == 300 + 4 + 2 and len(qs) == 64 and set(qs["type"].tolist()) == set(range(6))
    e = o64.expectation(oracle, _twin(oracle, cw), cw, qs, 64)
    counts = e.summary[:, 0]
    candidates = len(cw.candidates(static=True))
    print("overlaps per volume:", counts.tolist(), "candidates:", candidates)
    assert (e.summary[:, 2] == 1).all()
    assert int((counts >= 5).sum()) >= 8 and int((counts == 0).sum()) >= 4
    assert int((counts == candidates).sum()) >= 1
    seen = set()
    for k in range(len(qs)):
        vt = int(e.shapes[k, 10:11].view(np.uint32)[0])
        seen.update((vt, int(e.cols["type"][c])) for c in e.boxpass[k])
    assert seen == {(a, b) for a in range(6) for b in range(6)}, sorted({(a, b) for a in range(6) for b in range(6)} - seen)
    assert any(len(a) > 0 and qs["excludeCount"][k] > 0 for k, a in enumerate(e.all))


# ---- the pose of a mounted volume ------------------------------------------------------------------------------------------------
def _families():
    rng = np.random.default_rng(7)
    fam = {"rotations, offset ~1": [], "offset 1e3 (mount and volume)": [], "scale 1e-2": [], "scale 1e2": []}
    for _ in range(200):
        q1, q2 = ru._random_quat(rng), ru._random_quat(rng)
        fam["rotations, offset ~1"].append((rng.uniform(-2, 2, 3), q1, rng.uniform(-2, 2, 3), q2))
        fam["offset 1e3 (mount and volume)"].append((rng.uniform(-1e3, 1e3, 3), q1, rng.uniform(-1e3, 1e3, 3), q2))
        fam["scale 1e-2"].append((rng.uniform(-2e-2, 2e-2, 3), q1, rng.uniform(-2e-2, 2e-2, 3), q2))
        fam["scale 1e2"].append((rng.uniform(-2e2, 2e2, 3), q1, rng.uniform(-2e2, 2e2, 3), q2))
    for axis in np.eye(3):   # quarter and half turns: exact products
        for ang in (0.5 * np.pi, np.pi):
            q = np.float32([*(axis * np.sin(0.5 * ang)), np.cos(0.5 * ang)])
            fam["rotations, offset ~1"].append((np.array([1.0, 2.0, 3.0]), q, np.array([0.5, -0.25, 0.125]), q))
    return fam


def test_pose_composition_error():
    """compose32 against compose64 on a battery of mounts: the largest error per family is printed (the module's docstring holds the
    table) and stays under the stated bound; 4 x the measured figure is the tolerance of the GPU test for mounted volumes."""
    for name, cases in _families().items():
        worst_p = worst_q = worst_rel = 0.0
        for mp, mq, p, q in cases:
            mp, p = np.float32(mp), np.float32(p)
            p32, q32 = o64.compose32(mp, mq, p, q)
            p64, q64 = o64.compose64(mp, mq, p, q)
            ep = float(np.abs(p32.astype(np.float64) - p64).max())
            worst_p, worst_q = max(worst_p, ep), max(worst_q, float(np.abs(q32.astype(np.float64) - q64).max()))
            worst_rel = max(worst_rel, ep / (2.0 ** -24 * (float(np.linalg.norm(p)) + float(np.linalg.norm(mp)))))
        print("%-36s position %.2g  rotation %.2g  (%.2f of the bound's units)" % (name, worst_p, worst_q, worst_rel))
        assert worst_rel <= POSE_ULPS and worst_q <= 4 * 2.0 ** -24
