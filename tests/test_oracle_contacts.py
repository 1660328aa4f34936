"""The scalar oracle's contacts against tests/contact64.py (an independent float64 reading of the reference) on the contact battery and
the coupled groups: the battery's classification, the measured E_ORACLE table, the oracle's row form against the reference formula,
known answers of contact64 itself, and a sensitivity test: every constant and the row order move a case tagged for them."""
import numpy as np
import pytest

import contact64 as c64
from oracle import oracle as orc


def run_scalar(build, dt, iterations, row_form=False):
    """One step of a fresh SOLVER_SCALAR world (reference formula, or the device's row form in the same emission order)."""
    w = orc.OracleWorld(solver=orc.SOLVER_SCALAR)
    w.set_scalar_row_form(row_form)
    ids = build(w)
    out = dict(ids=ids, n=w.num_bodies, mass=w.mass_properties(), tr0=w.transforms(1), ve0=w.velocities())
    w.step_internal(dt, iterations)
    out["contacts"], out["pairs"], _ = w.contacts()
    out["impulses"], out["vel"], out["tr"] = w.contact_impulses(), w.velocities(), w.transforms(1)
    return out


def case_reference(run, ids, dt, iterations, **kw):
    idx = c64.contacts_of(ids, run["n"], run["contacts"], run["pairs"])
    return idx, c64.reference(run["mass"], run["tr0"], run["ve0"], run["contacts"][idx], run["pairs"][idx], range(len(idx)), dt, iterations, **kw)


def deviation(run, idx, ref):
    """(velocity, impulse) deviation of a run from a reference() result, relative to the case's velocity scale / largest impulse."""
    ev = max(float(np.abs(run["vel"][b].astype(np.float64) - v).max()) for b, v in ref["vel"].items()) / ref["scale"]
    ei = float(np.abs(run["impulses"][idx].astype(np.float64) - ref["impulses"]).max()) / ref["impulse_scale"] if ref["impulse_scale"] > 0.0 else 0.0
    return ev, ei


@pytest.fixture(scope="module")
def battery():
    cases = c64.battery()
    worlds = []
    for key, cs in c64.groups(cases).items():
        placed = c64.place(cs)
        runs = {rf: run_scalar(lambda w: c64.build_world(w, cs, placed), key[0], key[1], row_form=rf) for rf in (False, True)}
        refs = [case_reference(runs[False], ids, key[0], key[1]) for ids in runs[False]["ids"]]
        worlds.append(dict(key=key, cases=cs, placed=placed, runs=runs, refs=refs))
    return cases, worlds


@pytest.fixture(scope="module")
def coupled_runs():
    out = {}
    for name, g in c64.coupled().items():
        runs = {rf: run_scalar(g["build"], g["dt"], g["iterations"], row_form=rf) for rf in (False, True)}
        r = runs[False]
        n = len(r["contacts"])
        out[name] = dict(runs=runs, ref=c64.reference(r["mass"], r["tr0"], r["ve0"], r["contacts"], r["pairs"], range(n), g["dt"], g["iterations"]), idx=list(range(n)))
    return out


@pytest.fixture(scope="module")
def world_runs():
    """The connected groups of contact64.worlds() that the device test holds to float64, as (class, name, runs, contacts, reference)."""
    rows = []
    for name, g in c64.worlds().items():
        runs = {rf: run_scalar(g["build"], g["dt"], g["iterations"], row_form=rf) for rf in (False, True)}
        r = runs[False]
        for bodies, idx in c64.components(r["n"], r["pairs"]):
            if set(bodies) & g["sample"]:
                ref = c64.reference(r["mass"], r["tr0"], r["ve0"], r["contacts"][idx], r["pairs"][idx], range(len(idx)), g["dt"], g["iterations"])
                rows.append(("coupled" if len(bodies) > 1 else "plain", "%s bodies %s" % (name, bodies), runs, idx, ref, g["dt"]))
    return rows


def test_battery_is_complete_and_classified(battery):
    cases, worlds = battery
    assert 60 <= len(cases) <= 120 and sum(len(w["cases"]) for w in worlds) == len(cases)
    kinds, counts = {}, {}
    for wd in worlds:
        for c, (idx, ref) in zip(wd["cases"], wd["refs"]):
            kinds[c["name"]] = c64.classify(c, ref)
            counts[c["name"]] = len(idx)
            assert c["group"] in c64.E_ORACLE and c64.tolerance(c["group"]) <= c64.CAP and c64.tolerance(c["group"], "impulse") <= c64.CAP
    assert {n for n, k in kinds.items() if k == "tie"} == set(c64.TIES)
    print({k: sum(1 for v in kinds.values() if v == k) for k in ("clear", "tie")}, "contacts per case:", {k: sum(1 for v in counts.values() if v == k) for k in sorted(set(counts.values()))})
    # what the narrowphase makes of the collider pairs: every count from 1 to 4, at every depth
    for shape, want in (("sphere", 1), ("capsule", 2), ("box3", 3), ("box", 4)):
        for depth in ("in_slop", "touching", "deep"):
            assert counts["count/%s_%s" % (shape, depth)] == want, (shape, depth, counts["count/%s_%s" % (shape, depth)])
    assert min(counts.values()) >= 1
    names = {c["name"] for c in cases}
    assert {"bodies/sphere_kin_static", "bodies/sphere_kin_kin", "bodies/box_kin_static", "bodies/box_kin_kin", "bodies/bar_45", "bodies/offset_collider",
            "bodies/box_on_static_sphere", "dt/sphere_on_threshold", "dt/sphere_below", "iterations/box_30", "far/box_deep"} <= names


def test_cases_are_what_they_mean(battery):
    """The decisions the names promise, and the mass properties behind the body kinds."""
    _, worlds = battery
    for wd in worlds:
        run = wd["runs"][False]
        for c, ids, (idx, ref) in zip(wd["cases"], run["ids"], wd["refs"]):
            dec = [{n: d for n, d, _, _ in p} for p in ref["preds"]]
            name = c["name"]
            if name.endswith("_in_slop") or name.endswith("_touching"):
                assert not any(d["slop"] for d in dec), name
            if name.endswith("_deep") or name.startswith("restitution/"):
                assert all(d["slop"] and d["vrel"] for d in dec) and all(k["bias"] > 0.0 for k in ref["constraints"]), name
            if "separating" in c["tags"]:
                assert all(d["slop"] and not d["vrel"] for d in dec) and all(k["bias"] == 0.0 for k in ref["constraints"]) and not ref["impulses"].any(), name
            if name.startswith("dt/") and ("below" in name or "threshold" in name):
                assert not any(d["dt"] for d in dec) and all(k["bias"] == 0.0 for k in ref["constraints"]), name
            if "noz" in c["tags"] or name.endswith("mu0.3_zero"):
                assert all(d["noz"] for d in dec) and not ref["impulses"][:, 1].any(), name
            if "cone" in c["tags"]:   # on the cone at the end: |impT| == friction x impN of before the last normal row, which moved it by rounding at most
                k = ref["constraints"]
                assert len(k) > 1 or (abs(abs(k[0]["impT"]) - k[0]["friction"] * k[0]["impN"]) <= 1e-9 * k[0]["impN"] and k[0]["impT"] != 0.0), name
            if name.endswith("_stick") and c["material"][1] > 0.0 and c["iterations"] > 1:
                assert all(abs(x["impT"]) < x["friction"] * x["impN"] for x in ref["constraints"]), name
            for s, b in zip(("upper", "lower"), ids):
                if b is None:
                    continue
                inv_mass, cog, inv_i = c64.mass_of(run["mass"], b)
                assert (inv_mass == 0.0 and not inv_i.any()) == (c[s]["kind"] == c64.KIN), name
            if "cog" in c["tags"]:
                assert np.abs(c64.mass_of(run["mass"], ids[0])[1]).min() > 0.03, name
            if "bar" in c["tags"]:
                d = np.sort(np.linalg.eigvalsh(c64.mass_of(run["mass"], ids[0])[2]))
                assert d[2] / d[0] > 1000.0, d
            if name.endswith("light_on_heavy") or name.endswith("heavy_on_light"):
                ratio = c64.mass_of(run["mass"], ids[0])[0] / c64.mass_of(run["mass"], ids[1])[0]
                assert 990.0 < max(ratio, 1.0 / ratio) < 1010.0 and (ratio > 1.0) == name.endswith("light_on_heavy"), (name, ratio)


def test_e_oracle_table(battery, coupled_runs, world_runs):
    """The reference-formula oracle against contact64, per class; the row-form oracle (what the device is bit-equal to) as well."""
    _, worlds = battery
    worst = {False: {}, True: {}}
    rows = [(c["group"], c["name"], wd["runs"], idx, ref, c["dt"]) for wd in worlds for c, (idx, ref) in zip(wd["cases"], wd["refs"])]
    rows += [("coupled", name, g["runs"], g["idx"], g["ref"], c64.coupled()[name]["dt"]) for name, g in coupled_runs.items()] + world_runs
    for group, name, runs, idx, ref, dt in rows:
        for rf in (False, True):
            assert np.isfinite(runs[rf]["vel"]).all() and np.isfinite(runs[rf]["impulses"]).all(), name
            ev, ei = deviation(runs[rf], idx, ref)
            w = worst[rf].setdefault(group, [(0.0, ""), (0.0, "")])
            w[0], w[1] = max(w[0], (ev, name)), max(w[1], (ei, name))
            # poses: integrateVelocity of the solved velocities, a float32 rounding of the position and of the quaternion on top
            for b, (pos, rot) in ref["pose"].items():
                t = runs[rf]["tr"][b].astype(np.float64)
                bound = c64.ORACLE_HEADROOM * c64.K * c64.E_ORACLE[group][0] * ref["scale"] * dt
                assert np.abs(t[:3] - pos).max() <= bound + 4 * 2.0 ** -23 * max(1.0, float(np.abs(pos).max())), (name, b)
                assert min(np.abs(t[3:] - rot).max(), np.abs(t[3:] + rot).max()) <= bound + 4 * 2.0 ** -23, (name, b)
    for group in sorted(worst[False]):
        (ev, nv), (ei, ni) = worst[False][group]
        (rv, _), (ri, _) = worst[True][group]
        print("e_oracle %-8s velocity %.2e (%s)  impulse %.2e (%s)  table (%.1e, %.1e)  | row form: velocity %.2e impulse %.2e" % (group, ev, nv, ei, ni, *c64.E_ORACLE[group], rv, ri))
    assert set(worst[False]) == set(c64.E_ORACLE)
    for group, table in c64.E_ORACLE.items():
        for k in (0, 1):
            measured = worst[False][group][k][0]
            assert measured <= c64.ORACLE_HEADROOM * table[k] and table[k] <= c64.ORACLE_HEADROOM * measured, (group, ("velocity", "impulse")[k], measured, table[k])
            # the reason for K: the row form, the arithmetic the device runs, stays inside K x the reference formula's own distance
            assert worst[True][group][k][0] <= c64.tolerance(group, ("velocity", "impulse")[k]), (group, worst[True][group][k])


def test_row_form_against_the_reference_formula_on_the_battery(battery, coupled_runs, world_runs):
    """The two float32 formulations of the oracle side by side, same order, same inputs (test_oracle.py measured 1.5e-8 per step on the
    scenes): per class their distance stays inside the device's tolerance K x E_ORACLE, which is the reason for K."""
    _, worlds = battery
    worst = {}
    rows = [(c["group"], c["name"], wd["runs"], ref) for wd in worlds for c, (_, ref) in zip(wd["cases"], wd["refs"])] + [("coupled", n, g["runs"], g["ref"]) for n, g in coupled_runs.items()]
    rows += [(group, name, runs, ref) for group, name, runs, _, ref, _ in world_runs]
    for group, name, runs, ref in rows:
        d = max(float(np.abs(runs[False]["vel"][b].astype(np.float64) - runs[True]["vel"][b]).max()) for b in ref["vel"]) / ref["scale"]
        worst[group] = max(worst.get(group, (0.0, "")), (d, name))
    for group in sorted(worst):
        print("row form vs reference formula %-8s worst relative velocity difference %.2e (%s)  tolerance %.1e" % (group, *worst[group], c64.tolerance(group)))
        assert worst[group][0] <= c64.tolerance(group), (group, worst[group])


@pytest.mark.parametrize("name", sorted(c64.SCENE_STEPS))
def test_row_form_against_the_reference_formula_on_the_scenes(name):
    """The yardstick of test_gpu_contact_edges.py::test_follow_against_the_reference_formula: per step from identical inputs."""
    d = c64.formulation_distances(orc, name)
    worst = max(x for _, x in d)
    print("%s: %d of %d steps with contacts (up to %d); row form vs reference formula per step: worst %.2e, median %.2e; table %.2e" % (
        name, sum(1 for n, _ in d if n), len(d), max(n for n, _ in d), worst, float(np.median([x for _, x in d])), c64.E_FORMULATIONS[name]))
    assert sum(1 for n, _ in d if n) >= len(d) // 2
    assert worst <= c64.ORACLE_HEADROOM * c64.E_FORMULATIONS[name] and c64.E_FORMULATIONS[name] <= c64.ORACLE_HEADROOM * worst
    assert c64.K * c64.E_FORMULATIONS[name] <= c64.CAP


def test_zero_inverse_mass_pairs_change_nothing(battery):
    """constraints.cpp:3394-3397 skips them; the row form does not, and relies on mN = mT = 0: either way nothing moves, bit for bit."""
    _, worlds = battery
    seen = 0
    for wd in worlds:
        for rf in (False, True):
            run = wd["runs"][rf]
            for c, ids, (idx, ref) in zip(wd["cases"], run["ids"], wd["refs"]):
                if "no_mass" in c["tags"]:
                    seen += 1
                    assert len(idx) > 0 and not run["impulses"][idx].any() and not ref["impulses"].any(), c["name"]
                    for b in ids:
                        if b is not None:
                            assert np.array_equal(run["vel"][b].view(np.uint32), run["ve0"][b].view(np.uint32)), c["name"]
                            assert np.array_equal(ref["vel"][b], run["ve0"][b].astype(np.float64)), c["name"]
    assert seen >= 10


# ---- known answers of contact64 itself -----------------------------------------------------------------------------------------------
def _sphere(pos, v, w=(0.0, 0.0, 0.0), mass=2.0, radius=0.25, kinematic=False):
    inv_i = 0.0 if kinematic else 1.0 / (0.4 * mass * radius * radius)
    return c64.Body(pos, (0.0, 0.0, 0.0, 1.0), v, w, 0.0 if kinematic else 1.0 / mass, np.zeros(3), np.eye(3).ravel() * inv_i)


def _contact(point, depth, normal, friction, restitution):
    """A contact in float64 (the fields contact64 reads), so that the known answers hold to float64 rounding."""
    return dict(point=np.asarray(point, np.float64), depth=depth, normal=np.asarray(normal, np.float64),
                friction_restitution=(int(friction * 0xFFFF) << 16) | int(restitution * 0xFFFF))


_N = c64.normalize(c64.v3(0.25, 1.0, -0.5))
_DT = 1.0 / 120.0


@pytest.mark.parametrize("e", [0.0, 0.5, 1.0])
def test_known_restitution(e):
    """One central contact against the static body, one iteration, penetration exactly the slop (the branch forced on: its bias term is
    then an exact 0): the sphere leaves with -e x its approach speed along the normal."""
    A = _sphere(c64.v3(0, 0, 0), -1.5 * _N + c64.v3(0.25, 0.0, 0.125))
    c = _contact(-0.25 * _N, -c64.CONSTANTS["slop"], -_N, 0.0, e)     # A is the sphere: the normal points from A to the static B
    vn = float(-_N @ A.v)
    ks = c64.solve({0: A, 1: c64.static_body()}, [c], [(0, 1)], [0], _DT, 1, force={"slop": True})
    e_dec = c64.decode(c["friction_restitution"])[1]
    assert abs(e_dec - e) < 1e-5 and ks[0]["bias"] == -e_dec * -vn
    assert abs(float(-_N @ A.v) - (-e_dec * vn)) <= 1e-12


def test_known_friction_answers():
    n = -_N
    r = -0.25 * _N
    tangential = lambda B: (lambda u: u - (n @ u) * n)(-(B.v + np.cross(B.w, r)))
    # friction 0: the tangential anchor velocity stays
    A = _sphere(c64.v3(0, 0, 0), -1.0 * _N + c64.v3(0.5, 0.0, 0.25), w=(0.5, 0.25, 0.0))
    before = tangential(A)
    c64.solve({0: A, 1: c64.static_body()}, [_contact(r, 0.01, n, 0.0, 0.0)], [(0, 1)], [0], _DT, 4)
    assert np.abs(tangential(A) - before).max() <= 1e-12
    # sticking: slow sideways, friction 1: the anchor stops sideways
    A = _sphere(c64.v3(0, 0, 0), -1.0 * _N + c64.v3(0.05, 0.0, 0.02), w=(0.1, 0.0, 0.0))
    ks = c64.solve({0: A, 1: c64.static_body()}, [_contact(r, 0.01, n, 1.0, 0.0)], [(0, 1)], [0], _DT, 3)
    assert np.abs(tangential(A)).max() <= 1e-12 and 0.0 < abs(ks[0]["impT"]) < ks[0]["friction"] * ks[0]["impN"]
    # clamped: fast sideways: |impulse_t| is friction x the normal impulse of before this contact's last normal row
    A = _sphere(c64.v3(0, 0, 0), -1.0 * _N + c64.v3(5.0, 0.0, 2.0))
    bodies = {0: A, 1: c64.static_body()}
    k = c64.init(bodies, _contact(r, 0.01, n, 0.3, 0.0), (0, 1), _DT)
    c64.solve_one(bodies, k)
    assert k["impT"] == 0.0 and k["impN"] > 0.0            # first sweep: the normal impulse of before is 0, so is the cone
    previous = k["impN"]
    c64.solve_one(bodies, k)
    assert abs(abs(k["impT"]) - k["friction"] * previous) <= 1e-12 * previous and np.abs(tangential(A)).max() > 1.0


def test_known_momentum_and_no_mass():
    def momentum(bodies, masses):
        p = sum(m * B.v for B, m in zip(bodies, masses))
        h = sum(np.linalg.inv(B.invI) @ B.w + m * np.cross(B.pos, B.v) for B, m in zip(bodies, masses))
        return np.concatenate([p, h])
    A = _sphere(c64.v3(10.0, 0.0, 3.0), c64.v3(0.5, 1.0, 0.25), w=(1.0, 0.5, -0.5), mass=2.0)
    B = _sphere(c64.v3(10.0, 0.0, 3.0) + 0.49 * _N, c64.v3(0.0, -0.5, 0.0), w=(0.0, 0.25, 1.0), mass=2000.0)
    cs = [_contact(A.pos + 0.245 * _N + d, 0.01, _N, 0.5, 0.5) for d in (np.cross(_N, c64.v3(0.02, 0, 0)), np.cross(_N, c64.v3(0, 0, -0.02)))]
    before = momentum((A, B), (2.0, 2000.0))
    ks = c64.solve({0: A, 1: B}, cs, [(0, 1), (0, 1)], [0, 1], _DT, 6)
    assert all(k["impN"] > 0.0 and k["impT"] != 0.0 for k in ks)
    assert np.abs(momentum((A, B), (2.0, 2000.0)) - before).max() <= 1e-12 * np.abs(before).max()
    # both inverse masses zero: nothing changes
    A, B = _sphere(c64.v3(0, 0, 0), c64.v3(0.5, -1.0, 0.25), w=(1.0, 0.5, -0.5), kinematic=True), _sphere(0.49 * _N, c64.v3(0, 1, 0), kinematic=True)
    va, vb = np.concatenate([A.v, A.w]), np.concatenate([B.v, B.w])
    ks = c64.solve({0: A, 1: B}, [_contact(0.245 * _N, 0.01, _N, 0.5, 0.5)], [(0, 1)], [0], _DT, 6)
    assert ks[0]["impN"] == 0.0 and ks[0]["impT"] == 0.0 and ks[0]["mN"] == 0.0 and ks[0]["mT"] == 0.0
    assert np.array_equal(np.concatenate([A.v, A.w]), va) and np.array_equal(np.concatenate([B.v, B.w]), vb)


PERTURBATIONS = [("beta", dict(beta=c64.CONSTANTS["beta"] * 1.1), "bias"), ("slop", dict(slop=c64.CONSTANTS["slop"] * 0.4), "slop"),
                 ("dt_threshold", dict(dt_threshold=1e-7), "dt"), ("noz_threshold", dict(noz_threshold=1e-10), "noz"), ("row_order", dict(friction_first=0.0), "order")]


@pytest.mark.parametrize("name,constants,tag", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_battery_sees_every_constant(battery, name, constants, tag):
    """contact64 with one constant off (the bias factor by 10 %, the slop at 0.4 mm, the time step threshold below the small time step,
    noz's threshold a hundred times smaller, the normal row before the friction row) moves a case tagged for it by more than 10 x its
    tolerance."""
    _, worlds = battery
    seen = 0.0
    for wd in worlds:
        for c, ids, (idx, ref) in zip(wd["cases"], wd["runs"][False]["ids"], wd["refs"]):
            if tag in c["tags"]:
                _, pert = case_reference(wd["runs"][False], ids, wd["key"][0], wd["key"][1], constants=constants)
                moved = max(float(np.abs(pert["vel"][b] - v).max()) for b, v in ref["vel"].items()) / ref["scale"]
                seen = max(seen, moved / c64.tolerance(c["group"]))
    assert seen > 10.0, (name, seen)
