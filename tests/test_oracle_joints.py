"""The scalar oracle's joints against tests/joint64.py (an independent float64 reading of the reference) on the whole joint battery:
local frames, post-step velocities and poses; the battery's own classification (every case clear or a listed tie, none left out); and
a sensitivity test on joint64 alone: every constant and sign that matters moves a case tagged for it by more than 10 x its tolerance."""
import numpy as np
import pytest

import joint64 as j64
from oracle import oracle as orc


@pytest.fixture(scope="module")
def battery():
    cases = j64.battery()
    worlds = []
    for key, cs in j64.groups(cases).items():
        placed = j64.place(cs)
        w = orc.OracleWorld(solver=orc.SOLVER_SCALAR)
        ids = j64.build_world(w, cs, placed)
        mp = w.mass_properties()
        worlds.append(dict(key=key, cases=cs, placed=placed, world=w, ids=ids, mass=mp))
    return cases, worlds


def _refs(wd, **kw):
    return [j64.reference(c, pl, j64.mass_of(wd["mass"], 2 * k), j64.mass_of(wd["mass"], 2 * k + 1), **kw) for k, (c, pl) in enumerate(zip(wd["cases"], wd["placed"]))]


def test_battery_is_complete_and_classified(battery):
    cases, worlds = battery
    assert len(cases) >= 140 and sum(len(w["cases"]) for w in worlds) == len(cases)
    kinds = {}
    for wd in worlds:
        for k, (c, pl) in enumerate(zip(wd["cases"], wd["placed"])):
            kinds[c["name"]] = j64.classify(c, pl, j64.mass_of(wd["mass"], 2 * k), j64.mass_of(wd["mass"], 2 * k + 1))
    assert len(kinds) == len(cases)                                   # no case left out
    assert {n for n, k in kinds.items() if k == "tie"} == set(j64.TIES)
    print({k: sum(1 for v in kinds.values() if v == k) for k in ("clear", "tie")})
    for t in range(6):
        names = {c["name"].split("/", 1)[1] for c in cases if c["type"] == t}
        assert {"plain", "dyn_kin", "kin_dyn", "kin_kin", "cog_offset", "lever_1cm", "lever_10m", "far", "mass_1e4", "needle", "dt60", "dt_below_threshold"} <= names
    for wd in worlds:                                                 # jointed bodies never touch: their boxes are apart on some axis
        for c, pl in zip(wd["cases"], wd["placed"]):
            ext = [0.29 if c[s]["collider"][0] == j64.CAPSULE else 0.105 for s in "AB"]
            assert (np.abs(pl["A"]["pos"] - pl["B"]["pos"]) > ext[0] + ext[1]).any(), c["name"]
    for c in cases:
        assert (c["type"], c["group"]) in j64.E_ORACLE and j64.tolerance(c) <= j64.CAP, c["name"]


def test_mass_properties_are_what_the_cases_mean(battery):
    _, worlds = battery
    for wd in worlds:
        for k, c in enumerate(wd["cases"]):
            for j, s in enumerate("AB"):
                inv_mass, cog, inv_i = j64.mass_of(wd["mass"], 2 * k + j)
                if c[s]["kinematic"]:
                    assert inv_mass == 0.0 and not inv_i.any(), c["name"]
                else:
                    assert inv_mass > 0.0 and np.allclose(inv_i, inv_i.T, rtol=1e-6, atol=0.0), c["name"]
                    assert np.allclose(cog, c[s]["collider"][1][:3] if c[s]["collider"][0] == j64.SPHERE else 0.0, atol=1e-6), c["name"]
            if c["name"].endswith("/mass_1e4"):
                assert abs(j64.mass_of(wd["mass"], 2 * k)[0] / j64.mass_of(wd["mass"], 2 * k + 1)[0] - 1e4) < 1.0
            if c["name"].endswith("/needle"):
                d = np.sort(np.linalg.eigvalsh(j64.mass_of(wd["mass"], 2 * k)[2]))
                assert d[2] / d[0] > 400.0, d


def test_oracle_frames_match_joint64(battery):
    _, worlds = battery
    for wd in worlds:
        for c, cid, r in zip(wd["cases"], wd["ids"], _refs(wd)):
            pod = j64.pod_of(wd["world"], c, cid)
            for name in pod.dtype.names:
                want = np.asarray(r["pod"][name], np.float64)
                got = np.asarray(pod[name], np.float64)
                scale = 2000.0 if "Anchor" in name and c["far"] else max(1.0, float(np.abs(want).max()))
                # anchors of a far case are differences of 2000 m float32 coordinates rotated in float32: a few ulps of 2000 x 2^-23
                assert np.abs(got - want).max() <= 8 * 2.0 ** -23 * scale, (c["name"], name, got, want)


def test_oracle_velocities_and_poses_match_joint64(battery):
    _, worlds = battery
    worst = {}
    for wd in worlds:
        w = wd["world"]
        refs = _refs(wd)
        w.step_internal(wd["key"][0], wd["key"][1])
        vel, tr = w.velocities().astype(np.float64), w.transforms(1).astype(np.float64)
        for k, (c, r) in enumerate(zip(wd["cases"], refs)):
            assert np.isfinite(r["vel"]).all() and np.isfinite(vel[2 * k:2 * k + 2]).all(), c["name"]
            e = float(np.abs(vel[2 * k:2 * k + 2] - r["vel"]).max()) / r["scale"]
            key = (c["type"], c["group"])
            if e > worst.get(key, (0.0, ""))[0]:
                worst[key] = (e, c["name"])
            assert e <= j64.ORACLE_HEADROOM * j64.E_ORACLE[key], (c["name"], e, j64.E_ORACLE[key])
            for j in range(2):
                pos, rot = r["pose"][j]
                pscale = max(1.0, float(np.abs(pos).max()))
                assert np.abs(tr[2 * k + j, :3] - pos).max() <= j64.ORACLE_HEADROOM * j64.E_ORACLE[key] * r["scale"] * c["dt"] + 4 * 2.0 ** -23 * pscale, (c["name"], j)
                assert min(np.abs(tr[2 * k + j, 3:] - rot).max(), np.abs(tr[2 * k + j, 3:] + rot).max()) <= j64.ORACLE_HEADROOM * j64.E_ORACLE[key] * r["scale"] * c["dt"] + 4 * 2.0 ** -23, (c["name"], j)
    for key in sorted(worst):
        print("e_oracle %-10s %-5s %.2e (%s)  bound %.1e" % (j64.TYPE_NAMES[key[0]], key[1], worst[key][0], worst[key][1], j64.E_ORACLE[key]))
    # the table must stay the measurement: no figure more than the headroom above what the oracle shows here
    for key, measured in j64.E_ORACLE.items():
        assert key in worst and measured <= j64.ORACLE_HEADROOM * worst[key][0], (key, measured, worst.get(key))


def test_oracle_decisions_match_joint64(battery):
    """Every branch decision of the oracle's initialisation against joint64's, clear cases and ties alike: limit rows on and their
    signs, motors on and their targets, the time step threshold (any bias non-zero), the distance joint's l > 0.001, rotateFromTo's
    branch, sq > 0 and the swing position motor's noz; the angles behind them; and the accumulated impulses.  Run on a fresh step of
    fresh worlds, so that it does not depend on the order of the tests."""
    _, worlds = battery
    checked = 0
    for wd in worlds:
        w = orc.OracleWorld(solver=orc.SOLVER_SCALAR)
        ids = j64.build_world(w, wd["cases"], wd["placed"])
        assert ids == wd["ids"]
        refs = _refs(wd)
        w.step_internal(wd["key"][0], wd["key"][1])
        rows = {t: w.joint_decisions(t, sum(1 for c in wd["cases"] if c["type"] == t)) for t in range(6)}
        for c, cid, r in zip(wd["cases"], ids, refs):
            d = j64.decode_oracle(c["type"], rows[c["type"]][cid])
            v, tol = r["values"], j64.ORACLE_HEADROOM * j64.E_ORACLE[(c["type"], c["group"])] * r["scale"]
            indifferent = "indifferent" in c["tags"]
            # the time step threshold: below it no bias at all; above it a bias wherever joint64 has one beyond float32's rounding of the poses
            assert r["decisions"]["dt"] or (not d["biasNonzero"] and v["biasMax"] == 0.0), c["name"]
            assert d["biasNonzero"] or v["biasMax"] < 0.01, (c["name"], v["biasMax"])
            for k in ("solveLimit", "solveMotor", "solveSwingLimit", "solveTwistLimit", "solveSwingMotor", "solveTwistMotor", "lengthNonzero"):
                if k in d:
                    assert d[k] == v[k], (c["name"], k)
                    checked += 1
            for k, on in (("limitSign", d.get("solveLimit")), ("twistSign", d.get("solveTwistLimit"))):
                if on:
                    assert d[k] == v[k], (c["name"], k)
            # angles: float32 atan2f / acosf of float32 dots; an angle error is what a limit bias multiplies by 0.1 / dt
            for k in ("angle", "twistAngle"):
                if k in d and k in v and (c["type"] == j64.CONE_TWIST or d["solveLimit"] or d["solveMotor"] or c["args"].get("min", 1.0) <= 0 or c["args"].get("max", -1.0) >= 0):
                    assert abs(d[k] - v[k]) <= tol * c["dt"] / 0.1 + 8 * 2.0 ** -23 * np.pi, (c["name"], k, d[k], v[k])
            if c["type"] == j64.CONE_TWIST:
                if not indifferent:   # (the indifferent ties are those where float32 may take either branch, with the same result)
                    assert d["rotateFromTo"] == v["rotateFromTo"] and d["swingSq"] == r["decisions"]["swing_sq"], (c["name"], d["rotateFromTo"], v["rotateFromTo"])
                    # acosf near w = 1 turns an ulp of w (6e-8) into sqrt(2 * 6e-8) = 3.5e-4 rad: the swing angle is compared where the cosine is away from 1
                    if v["swingAngle"] > 0.05:
                        assert abs(d["swingAngle"] - v["swingAngle"]) <= tol * c["dt"] / 0.1 + 8 * 2.0 ** -23 * np.pi, (c["name"], d["swingAngle"], v["swingAngle"])
                    else:
                        assert d["swingAngle"] == 0.0 or abs(d["swingAngle"] - v["swingAngle"]) <= 4e-4, (c["name"], d["swingAngle"], v["swingAngle"])
                if "swing_pm_noz" in r["decisions"]:
                    assert d["swingMotorAxisZero"] == r["decisions"]["swing_pm_noz"], c["name"]
            for k, on in (("motorVelocity", d.get("solveMotor")), ("swingMotorVelocity", d.get("solveSwingMotor")), ("twistMotorVelocity", d.get("solveTwistMotor"))):
                if on:
                    # a position motor's target is (target - angle) / dt: the same angle or distance error as a bias, without the 0.1
                    assert abs(d[k] - v[k]) <= tol / 0.1 + 8 * 2.0 ** -23 * abs(v[k]), (c["name"], k, d[k], v[k])
            for k, x in d["impulses"].items():
                if np.isfinite(r["impulses"][k]):
                    assert (x != 0.0) == (r["impulses"][k] != 0.0) or abs(x - r["impulses"][k]) <= tol, (c["name"], k, x, r["impulses"][k])
    assert checked > 100


def test_saturated_motors_sit_on_the_bound_in_joint64(battery):
    _, worlds = battery
    for wd in worlds:
        for c, r in zip(wd["cases"], _refs(wd)):
            bounds = {"motor": "maxMotorImpulse", "swingMotor": "maxSwingMotorImpulse", "twistMotor": "maxTwistMotorImpulse"}
            active = [(k, r["values"][b]) for k, b in bounds.items() if b in r["values"] and r["values"][b] > 0.0]
            if "saturated" in c["tags"]:
                assert active and all(abs(r["impulses"][k]) == m for k, m in active), c["name"]
            if "unsaturated" in c["tags"]:
                assert active and all(abs(r["impulses"][k]) < m for k, m in active), c["name"]
            assert all(r["impulses"].get(k, 0.0) >= 0.0 for k in ("limit", "twist", "swing")), c["name"]


PERTURBATIONS = [("beta_distance", 1.1, "beta", (j64.DISTANCE,)), ("beta_ball", 1.1, "beta", (j64.BALL, j64.FIXED, j64.HINGE, j64.CONE_TWIST)),
                 ("beta_slider", 1.1, "beta", (j64.FIXED, j64.SLIDER)), ("beta_hinge_rot", 1.1, "beta_hinge_rot", (j64.HINGE,)),
                 ("beta_hinge_limit", 1.1, "beta_hinge_limit", (j64.HINGE, j64.CONE_TWIST)), ("beta_twist_limit", 1.1, "beta_twist_limit", (j64.CONE_TWIST,)),
                 ("beta_slider_limit", 1.1, "beta_slider_limit", (j64.SLIDER,)), ("dt_threshold", 1.0e-7 / 1.0e-5, "dt_threshold", tuple(range(6))),
                 ("limit_sign", -1.0, "limit_sign", (j64.HINGE, j64.CONE_TWIST, j64.SLIDER)), ("swap_tangents", None, "tangents", (j64.HINGE, j64.SLIDER)),
                 ("pm_clamp", 1.1, "pm_clamp", (j64.HINGE, j64.CONE_TWIST, j64.SLIDER)), ("swing_pm_factor", 1.1, "swing_pm_factor", (j64.CONE_TWIST,)),
                 ("rot_bias_factor", 1.1, "rot2", (j64.FIXED, j64.SLIDER))]


@pytest.mark.parametrize("constant,factor,tag,types", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_battery_sees_every_constant(battery, constant, factor, tag, types):
    """joint64 with one constant off by 10 % (a sign flipped, the tangents swapped, DT_THRESHOLD moved below the small time step) moves
    at least one case tagged for it, in every joint type that uses it, by more than 10 x that case's tolerance."""
    _, worlds = battery
    value = 1.0 if factor is None else j64.CONSTANTS[constant] * factor
    seen = {}
    for wd in worlds:
        base, pert = _refs(wd), _refs(wd, constants={constant: value})
        for c, r, p in zip(wd["cases"], base, pert):
            if tag in c["tags"]:
                moved = float(np.abs(p["vel"] - r["vel"]).max()) / r["scale"]
                seen[c["type"]] = max(seen.get(c["type"], 0.0), moved / j64.tolerance(c))
    for t in types:
        assert seen.get(t, 0.0) > 10.0, (constant, j64.TYPE_NAMES[t], seen.get(t))


def test_tiny_swing_is_lost_not_nan():
    """getAxisRotation takes acosf(q.w) unclamped (math.cpp:582): a w above 1 would give NaN and switch the swing limit off without a
    word.  300 swings from 1e-5 to 5e-3 rad about random axes, at two orientations, swingLimit 0: float32 never gets w above 1 here
    (rotateFromTo normalises, and the general branch's w is s / 2 / |q| <= 1), no angle is NaN, and the limit row is on in every case.
    What does happen is a loss: below about 1e-3 rad w rounds to 1 and the swing angle reads an exact 0 (the limit's bias then is 0, not
    swing x 0.1 / dt), and where it does not, it is quantised by acosf near 1 (0, 6.9e-4, 9.8e-4, ...): within 1e-3 rad of the truth."""
    rng = np.random.RandomState(1)
    anchor, pose_b, zero = (0.3, 0.05, -0.02), ((0.6, 0.0, 0.0), j64._IDENT), np.zeros(3)
    cases, truth = [], []
    for ang in np.logspace(-5, -2.3, 150):
        axis = j64.normalize(np.array([rng.uniform(-1, 1), 0.0, rng.uniform(-1, 1)]))
        for q in (j64._IDENT, j64._GENERIC_Q):
            pos, _ = j64._rot_about(pose_b, anchor, axis, ang)
            body = lambda p: dict(pos=p, rot=q, kinematic=False, collider=j64._SMALL, v=zero, w=zero)
            cases.append(dict(name="tiny%d" % len(cases), type=j64.CONE_TWIST, group="trig", tags=set(), A=body((0.0, 0.0, 0.0)), B=body((0.6, 0.0, 0.0)),
                              args=dict(anchor=anchor, axis=(0.0, 1.0, 0.0), swing=0.0, twist=-1.0), edits={}, moveA=None,
                              moveB=(pos, j64.qnorm(j64.qmul(j64.qaxis(axis, ang), np.array(q, np.float64)))), dt=float(np.float32(1.0 / 120.0)), iterations=1, far=False))
            truth.append(ang)
    w = orc.OracleWorld(solver=orc.SOLVER_SCALAR)
    j64.build_world(w, cases, j64.place(cases))
    w.step_internal(cases[0]["dt"], 1)
    d = w.joint_decisions(j64.CONE_TWIST, len(cases))
    qw, angle, truth = d[:, 20], d[:, 16], np.array(truth)
    assert (qw <= 1.0).all() and np.isfinite(angle).all() and np.isfinite(w.velocities()).all()
    assert ((d[:, 0].astype(int) & 1) == 1).all()                      # the swing limit row is on everywhere
    assert np.abs(angle - truth).max() <= 1e-3
    lost = angle == 0.0
    assert lost[truth < 3e-4].all() and not lost[truth > 1.5e-3].any(), (truth[lost].max(), truth[~lost].min())
