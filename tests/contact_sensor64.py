"""The rule of mi_contact_sensors (include/mi_physics.h) read over plain arrays, independent of the device kernels.

Inputs, all by schedule position p of the last step:
    ids     [P, 4] uint32   body A, body B, contact count, manifold slot (rowIds: schedule() and manifolds())
    normal  [P, 3] float32  the manifold's normal (rowShared.xyz = the normal of manifolds())
    rows    [P, 4, 15] float32  per contact t, rA x t, rB x t, rA x n, rB x n (contact_rows())
    lam     [P, 4, 2] float32   per contact the accumulated normal and tangent impulse (contact_impulses())
    sensors CONTACT_SENSOR records or [n, 4] uint32: body, partners, excludeFirst, excludeCount
    num_bodies: the bodies of the step; the static dummy is the index num_bodies.  dead: bodies whose sensors read valid = 0.

Two evaluations of the same sums.  `evaluate32` is the device's arithmetic: float32, every product and every sum a numpy float32
scalar operation (one correctly rounded IEEE operation each, no fused multiply-add), a term formed per component as
fl(fl(ln n_x) + fl(lt t_x)), negated for side A, added to an accumulator that starts at +0 in ascending manifold slot, then ascending
contact index: its result is what the device must return bit for bit.  `evaluate64` forms the same sums in float64 (the float32 inputs
taken exactly), in the same order; at float64 the order is of no consequence for the comparisons it serves.

ROUNDING_2100: the float32 evaluation against the float64 one on a synthetic segment of 2 100 manifolds (synthetic_segment(): one
body, every manifold one to four contacts with impulses of one sign of order 1, the case that accumulates the largest sum),
relative to the largest accumulated magnitude; measured by tests/test_contact_sensor64_cpu.py, which re-checks the figure.  It is the
yardstick for what a float32 sum of that length may lose: comparisons of a reading with a float64 quantity cannot ask for less.
"""
import numpy as np

DYNAMIC, STATIC = 1, 2
STATIC_BODY = 0xFFFFFFFF
SENSOR_DTYPE = np.dtype([("body", "<u4"), ("partners", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4")])
READING_DTYPE = np.dtype([("impulse", "<f4", 3), ("normalImpulse", "<f4"), ("angularImpulse", "<f4", 3), ("numContacts", "<u4"),
                          ("numManifolds", "<u4"), ("strongestPartner", "<u4"), ("valid", "<u4"), ("reserved", "<u4")])
READING64_DTYPE = np.dtype([("impulse", "<f8", 3), ("normalImpulse", "<f8"), ("angularImpulse", "<f8", 3), ("numContacts", "<u4"),
                            ("numManifolds", "<u4"), ("strongestPartner", "<u4"), ("valid", "<u4"), ("largestTerm", "<f8")])

ROUNDING_2100 = 2.7e-6   # measured: 2.63e-6 (linear), 1.33e-6 (angular), 5.3e-8 (normal) of the largest component of the sum; the test admits [figure / 2, figure]


def as_sensors(sensors):
    if isinstance(sensors, np.ndarray) and sensors.dtype == SENSOR_DTYPE:
        return sensors.reshape(-1)
    return np.ascontiguousarray(sensors, np.uint32).reshape(-1, 4).view(SENSOR_DTYPE).reshape(-1)


def passes(partner, sensor, num_bodies):
    """The partner filter of one sensor."""
    if partner == num_bodies:
        return bool(int(sensor["partners"]) & STATIC)
    excluded = ((int(partner) - int(sensor["excludeFirst"])) & 0xFFFFFFFF) < int(sensor["excludeCount"])
    return bool(int(sensor["partners"]) & DYNAMIC) and not excluded


def segments(ids):
    """body -> [(slot, position, is B)] in ascending slot."""
    out = {}
    for p, (a, b, _, slot) in enumerate(np.asarray(ids, np.uint32).reshape(-1, 4).tolist()):
        out.setdefault(a, []).append((slot, p, False))
        out.setdefault(b, []).append((slot, p, True))
    for seg in out.values():
        seg.sort()
    return out


def _evaluate(ids, normal, rows, lam, sensors, num_bodies, dead, real, out_dtype):
    ids = np.asarray(ids, np.uint32).reshape(-1, 4)
    normal, rows, lam = np.asarray(normal, np.float32), np.asarray(rows, np.float32), np.asarray(lam, np.float32)
    sensors = as_sensors(sensors)
    segs = segments(ids)
    dead = set(int(b) for b in dead)
    out = np.zeros(len(sensors), out_dtype)
    zero = real(0.0)
    for i, sn in enumerate(sensors):
        body = int(sn["body"])
        if body >= num_bodies or body in dead:
            continue
        lin, ang, nrm = [zero, zero, zero], [zero, zero, zero], zero
        contacts = manifolds = strongest = 0
        best, largest = zero, 0.0
        for slot, p, is_b in segs.get(body, ()):
            partner = int(ids[p, 0] if is_b else ids[p, 1])
            if not passes(partner, sn, num_bodies):
                continue
            n = [real(x) for x in normal[p]]
            total = zero
            for k in range(int(ids[p, 2])):
                r = rows[p, k]
                t = [real(x) for x in r[0:3]]
                ct = [real(x) for x in (r[6:9] if is_b else r[3:6])]
                cn = [real(x) for x in (r[12:15] if is_b else r[9:12])]
                ln, lt = real(lam[p, k, 0]), real(lam[p, k, 1])
                for c in range(3):
                    term = ln * n[c] + lt * t[c]            # fl(fl(ln n) + fl(lt t)): three rounded operations
                    lin[c] = lin[c] + (term if is_b else -term)
                    aterm = ln * cn[c] + lt * ct[c]
                    ang[c] = ang[c] + (aterm if is_b else -aterm)
                    largest = max(largest, abs(float(term)))
                nrm = nrm + ln
                total = total + ln
            if manifolds == 0 or total > best:                   # ascending slots: a tie keeps the lower slot
                best, strongest = total, (STATIC_BODY if partner == num_bodies else partner)
            manifolds += 1
            contacts += int(ids[p, 2])
        o = out[i]
        o["impulse"], o["angularImpulse"], o["normalImpulse"] = lin, ang, nrm
        o["numContacts"], o["numManifolds"], o["strongestPartner"], o["valid"] = contacts, manifolds, strongest, 1
        if "largestTerm" in out_dtype.names:
            o["largestTerm"] = largest
    return out


def evaluate32(ids, normal, rows, lam, sensors, num_bodies, dead=()):
    """READING_DTYPE records: the bytes mi_contact_sensors must return."""
    with np.errstate(all="ignore"):
        return _evaluate(ids, normal, rows, lam, sensors, num_bodies, dead, np.float32, READING_DTYPE)


def evaluate64(ids, normal, rows, lam, sensors, num_bodies, dead=()):
    """READING64_DTYPE records: the sums in float64, and the largest linear term component of each sensor."""
    return _evaluate(ids, normal, rows, lam, sensors, num_bodies, dead, np.float64, READING64_DTYPE)


def from_world(world):
    """(ids, normal, rows, lam, num_bodies) of a device world's last step, from its debug readbacks."""
    order, _ = world.schedule()
    _, counts, contacts4, body_pairs = world.manifolds()
    order = order.astype(np.int64)
    ids = np.zeros((len(order), 4), np.uint32)
    if len(order):
        ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3] = body_pairs[order, 0], body_pairs[order, 1], counts[order], order
    normal = contacts4["normal"][order, 0] if len(order) else np.zeros((0, 3), np.float32)
    return ids, normal, world.contact_rows(), world.contact_impulses(), world.num_bodies


def synthetic_segment(manifolds=2100, seed=11):
    """One body (index 0) with `manifolds` manifolds against bodies 1.., alternately as A and as B with the normal turned so that every
    normal impulse pushes body 0 the same way: the sum grows to its full length.  Returns (ids, normal, rows, lam, num_bodies)."""
    rng = np.random.RandomState(seed)
    ids = np.zeros((manifolds, 4), np.uint32)
    as_b = (np.arange(manifolds) % 2).astype(bool)
    ids[:, 0] = np.where(as_b, 1 + np.arange(manifolds), 0)
    ids[:, 1] = np.where(as_b, 0, 1 + np.arange(manifolds))
    ids[:, 2] = 1 + rng.randint(0, 4, manifolds)
    ids[:, 3] = rng.permutation(manifolds * 3)[:manifolds]
    n = rng.normal(size=(manifolds, 3)) * 0.2 + np.array([0.0, 1.0, 0.0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[~as_b] *= -1.0
    rows = rng.uniform(-1.0, 1.0, (manifolds, 4, 15))
    rows[:, :, 9:15] = np.abs(rows[:, :, 9:15]) * np.where(as_b, 1.0, -1.0)[:, None, None]   # r x n of one sign too
    lam = np.zeros((manifolds, 4, 2))
    lam[:, :, 0] = rng.uniform(0.5, 1.5, (manifolds, 4))
    lam[:, :, 1] = rng.uniform(-0.5, 0.5, (manifolds, 4))
    return ids, n.astype(np.float32), rows.astype(np.float32), lam.astype(np.float32), manifolds + 1
