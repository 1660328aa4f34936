"""The device's joints on the joint battery (tests/joint64.py): one step from identical inputs on each of the three solve paths,
against the scalar oracle (bit for bit where no libm trigonometry is involved) and against the float64 reference, with the flags, signs,
motor targets and accumulated impulses read back from the joint update records."""
import os

import numpy as np
import pytest

import joint64 as j64

pytestmark = pytest.mark.gpu

PATHS = ("launch_sweep", "cluster", "interleaved")


def _refs(wd):
    return [j64.reference(c, pl, j64.mass_of(wd["mass"], 2 * k), j64.mass_of(wd["mass"], 2 * k + 1)) for k, (c, pl) in enumerate(zip(wd["cases"], wd["placed"]))]


@pytest.fixture(scope="module")
def oracle_side(oracle):
    out = []
    for key, cs in j64.groups(j64.battery()).items():
        placed = j64.place(cs)
        w = oracle.OracleWorld(solver=oracle.SOLVER_SCALAR)
        ids = j64.build_world(w, cs, placed)
        wd = dict(key=key, cases=cs, placed=placed, ids=ids, mass=w.mass_properties(), pods=[j64.pod_of(w, c, i).copy() for c, i in zip(cs, ids)])
        wd["refs"] = _refs(wd)
        w.step_internal(key[0], key[1])
        wd["vel"], wd["tr"] = w.velocities(), w.transforms(1)
        rows = {t: w.joint_decisions(t, sum(1 for c in cs if c["type"] == t)) for t in range(6)}
        wd["decisions"] = [j64.decode_oracle(c["type"], rows[c["type"]][i]) for c, i in zip(cs, ids)]
        out.append(wd)
    return out


_device_runs = {}


def _device(mi, oracle_side, path):
    """The battery stepped once on the device on one solve path: per world the PODs, mass properties, velocities, poses, update
    records (by case) and the path the step reports."""
    if path in _device_runs:
        if isinstance(_device_runs[path], BaseException):    # it went wrong once: nothing of it is started on the GPU again
            raise RuntimeError("the %s run failed earlier in this session: %r" % (path, _device_runs[path]))
        return _device_runs[path]
    env = {"MI_CLUSTER_NO_JOINTS": "1"} if path == "interleaved" else {}
    old = {k: os.environ.get(k) for k in env}
    runs = []
    try:
        os.environ.update(env)
        for wd in oracle_side:
            g = mi.World()                                   # the switches are read when the world is created
            ids = j64.build_world(g, wd["cases"], wd["placed"], contact_far_away=path != "launch_sweep")
            assert ids == wd["ids"]
            run = dict(mass=g.mass_properties(), pods=[j64.pod_of(g, c, i).copy() for c, i in zip(wd["cases"], ids)])
            g.step_internal(wd["key"][0], wd["key"][1])
            n = 2 * len(wd["cases"])
            run["vel"], run["tr"] = g.velocities()[:n], g.transforms(1)[:n]
            run["records"], run["paths"] = [None] * len(wd["cases"]), set()
            for t in range(6):
                mine = [k for k, c in enumerate(wd["cases"]) if c["type"] == t]
                order = g.joint_order(t, len(mine))
                rec, p = g.joint_update(t, len(mine))
                run["paths"].add(p)
                by_id = {wd["ids"][k]: k for k in mine}
                for row, cid in enumerate(order):
                    run["records"][by_id[int(cid)]] = rec[row].copy()
            run["stats"] = g.stats()
            g.close()
            runs.append(run)
    except BaseException as e:
        _device_runs[path] = e
        raise
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    _device_runs[path] = runs
    return runs


def _no_libm(c):
    """Cases whose initialisation calls no libm trigonometry: the device must equal the oracle bit for bit."""
    if c["type"] in (j64.DISTANCE, j64.BALL, j64.FIXED, j64.SLIDER):
        return True
    a, e = c["args"], c["edits"]
    return c["type"] == j64.HINGE and a.get("min", 1.0) > 0.0 and a.get("max", -1.0) < 0.0 and e.get("maxMotorTorque", -1.0) <= 0.0


@pytest.mark.parametrize("path", PATHS)
def test_path_taken(mi, oracle_side, path):
    want = {"launch_sweep": mi.JOINT_PATH_LAUNCH_SWEEP, "cluster": mi.JOINT_PATH_CLUSTER, "interleaved": mi.JOINT_PATH_INTERLEAVED}[path]
    for run in _device(mi, oracle_side, path):
        assert run["paths"] == {want}, (path, run["paths"])
        assert run["stats"]["numFlowRecoveries"] == 0
        assert (run["stats"]["numContacts"] > 0) == (path != "launch_sweep")


@pytest.mark.parametrize("path", PATHS)
def test_frames_and_mass_properties(mi, oracle_side, path):
    for wd, run in zip(oracle_side, _device(mi, oracle_side, path)):
        assert np.array_equal(run["mass"][:len(wd["mass"])].view(np.uint32), wd["mass"].view(np.uint32))
        for c, gp, op, r in zip(wd["cases"], run["pods"], wd["pods"], wd["refs"]):
            assert gp.tobytes() == op.tobytes(), c["name"]
            for name in gp.dtype.names:
                want = np.asarray(r["pod"][name], np.float64)
                scale = 2000.0 if "Anchor" in name and c["far"] else max(1.0, float(np.abs(want).max()))
                assert np.abs(np.asarray(gp[name], np.float64) - want).max() <= 8 * 2.0 ** -23 * scale, (c["name"], name)


@pytest.mark.parametrize("path", PATHS)
def test_decisions_signs_and_impulses(mi, oracle_side, path):
    bounds = {"motor": "maxMotorImpulse", "swingMotor": "maxSwingMotorImpulse", "twistMotor": "maxTwistMotorImpulse"}
    checked = 0
    for wd, run in zip(oracle_side, _device(mi, oracle_side, path)):
        for c, rec, r, o in zip(wd["cases"], run["records"], wd["refs"], wd["decisions"]):
            d = j64.decode_update(c["type"], rec)
            tol = j64.tolerance(c) * r["scale"]
            exact = _no_libm(c)
            for k, v in d.items():
                if k.startswith("solve"):
                    assert v == r["values"][k] and v == o[k], (c["name"], k)
                    checked += 1
            rows_on = {"limitSign": d.get("solveLimit"), "twistSign": d.get("solveTwistLimit")}
            for k, on in rows_on.items():
                if on:
                    assert d[k] == r["values"][k] and d[k] == o[k], (c["name"], k)
            motors = {"motorVelocity": d.get("solveMotor"), "swingMotorVelocity": d.get("solveSwingMotor"), "twistMotorVelocity": d.get("solveTwistMotor")}
            for k, on in motors.items():
                if on:
                    # Against the oracle: the same float32 arithmetic, so equal, or (libm against OCML) 4 ulps of an angle of at most pi, over dt.
                    assert d[k] == o[k] if exact else abs(d[k] - o[k]) <= 4 * 2.0 ** -23 * np.pi / c["dt"], (c["name"], k, d[k], o[k])
                    # Against joint64: a position motor's target is (target - angle) / dt, a limit bias (limit - angle) * 0.1 / dt.  The class
                    # tolerance is what the float32 error of such an angle or distance does to a velocity THROUGH a bias, so the same
                    # error without the 0.1 is tol / 0.1 (a velocity motor's target is a stored constant: 8 ulps).
                    assert abs(d[k] - r["values"][k]) <= tol / 0.1 + 8 * 2.0 ** -23 * abs(r["values"][k]), (c["name"], k, d[k], r["values"][k])
            for k, v in d["impulses"].items():
                on = {"limit": d.get("solveLimit"), "twist": d.get("solveTwistLimit"), "swing": d.get("solveSwingLimit"),
                      "motor": d.get("solveMotor"), "swingMotor": d.get("solveSwingMotor"), "twistMotor": d.get("solveTwistMotor")}[k]
                if not on:
                    assert v == 0.0, (c["name"], k)
                    continue
                # an accumulated impulse is the sum over the iterations of effective mass x (velocity error + bias): each iteration may add
                # the row's effective mass (joint64's) x a velocity error within the velocity tolerance
                eff = r["values"]["eff"][k] * c["iterations"]
                ref = r["impulses"][k]
                assert v == o["impulses"][k] if exact else abs(v - o["impulses"][k]) <= tol * eff if np.isfinite(eff) else True, (c["name"], k, v, o["impulses"][k])
                if k in ("limit", "twist", "swing"):
                    assert v >= 0.0, (c["name"], k)
                    assert (v > 0.0) == (ref > 0.0) and abs(v - ref) <= tol * eff, (c["name"], k, v, ref, tol * eff)
                else:
                    bound = np.float32(d[bounds[k]])
                    assert bound == np.float32(np.float32(c["edits"][{"motor": "maxMotorTorque" if c["type"] == j64.HINGE else "maxMotorForce", "swingMotor": "maxSwingMotorTorque", "twistMotor": "maxTwistMotorTorque"}[k]]) * np.float32(c["dt"])), (c["name"], k)
                    assert abs(np.float32(v)) <= bound, (c["name"], k)
                    if "saturated" in c["tags"]:
                        assert abs(np.float32(v)) == bound and np.sign(v) == np.sign(ref), (c["name"], k, v, bound)
                    if "unsaturated" in c["tags"]:
                        assert abs(np.float32(v)) < bound and abs(v - ref) <= tol * eff, (c["name"], k, v, ref, tol * eff)
    assert checked > 100


@pytest.mark.parametrize("path", PATHS)
def test_velocities_and_poses(mi, oracle_side, path):
    worst, worst_orc = {}, {}
    for wd, run in zip(oracle_side, _device(mi, oracle_side, path)):
        for k, (c, r) in enumerate(zip(wd["cases"], wd["refs"])):
            gv, gt, ov, ot = run["vel"][2 * k:2 * k + 2], run["tr"][2 * k:2 * k + 2], wd["vel"][2 * k:2 * k + 2], wd["tr"][2 * k:2 * k + 2]
            assert np.isfinite(gv).all() and np.isfinite(gt).all(), c["name"]
            tol = j64.tolerance(c)
            key = (c["type"], c["group"])
            e64 = float(np.abs(gv.astype(np.float64) - r["vel"]).max()) / r["scale"]
            eo = float(np.abs(gv.astype(np.float64) - ov).max()) / r["scale"]
            worst[key] = max(worst.get(key, (0.0, "")), (e64, c["name"])); worst_orc[key] = max(worst_orc.get(key, (0.0, "")), (eo, c["name"]))
            if _no_libm(c):
                assert np.array_equal(gv.view(np.uint32), ov.view(np.uint32)) and np.array_equal(gt.view(np.uint32), ot.view(np.uint32)), (c["name"], "not bit-equal to the oracle", eo)
            else:
                assert eo <= tol, (c["name"], "oracle", eo, tol)
                assert np.abs(gt[:, :3].astype(np.float64) - ot[:, :3]).max() <= tol * r["scale"] * c["dt"] + 2 * 2.0 ** -23 * max(1.0, float(np.abs(ot[:, :3]).max())), c["name"]
                assert np.abs(gt[:, 3:].astype(np.float64) - ot[:, 3:]).max() <= tol * r["scale"] * c["dt"] + 2 * 2.0 ** -23, c["name"]
            assert e64 <= tol, (c["name"], "joint64", e64, tol)
            for j in range(2):
                pos, rot = r["pose"][j]
                assert np.abs(gt[j, :3] - pos).max() <= tol * r["scale"] * c["dt"] + 4 * 2.0 ** -23 * max(1.0, float(np.abs(pos).max())), (c["name"], j)
                assert min(np.abs(gt[j, 3:] - rot).max(), np.abs(gt[j, 3:] + rot).max()) <= tol * r["scale"] * c["dt"] + 4 * 2.0 ** -23, (c["name"], j)
    for key in sorted(worst):
        print("%-12s %-10s %-5s vs joint64 %.2e (%s), vs oracle %.2e (%s), tolerance %.1e" % (path, j64.TYPE_NAMES[key[0]], key[1], worst[key][0], worst[key][1],
                                                                                          worst_orc[key][0], worst_orc[key][1], max(j64.K * j64.E_ORACLE[key], j64.FLOOR_ULPS * 2.0 ** -23)))


def test_three_paths_agree_bit_for_bit(mi, oracle_side):
    runs = [_device(mi, oracle_side, p) for p in PATHS]
    for w in range(len(oracle_side)):
        for other, p in zip(runs[1:], PATHS[1:]):
            assert np.array_equal(runs[0][w]["vel"].view(np.uint32), other[w]["vel"].view(np.uint32)), p
            assert np.array_equal(runs[0][w]["tr"].view(np.uint32), other[w]["tr"].view(np.uint32)), p
            for c, a, b in zip(oracle_side[w]["cases"], runs[0][w]["records"], other[w]["records"]):
                used = {0: 17, 1: 18, 2: 30, 3: 47, 4: 60, 5: 59}[c["type"]]   # floats the kernels write (layouts: k_joints.hip)
                assert np.array_equal(a[:used].view(np.uint32), b[:used].view(np.uint32)), (p, c["name"])
