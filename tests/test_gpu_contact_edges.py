"""The device's contact rows and sweeps on the contact battery (tests/contact64.py) and on worlds built to reach every sweep kernel:
one step from identical inputs on each of the three solve paths (the launch-per-colour sweep, the cluster sweep, the replay of the
reference's batch order), against the following row-form oracle bit for bit and against the float64 statement within the class
tolerance, velocities, poses and the accumulated impulses read back from the device."""
import os

import numpy as np
import pytest

import contact64 as c64
from parity_util import follow_step

pytestmark = pytest.mark.gpu

PATHS = ("launch_sweep", "cluster", "replay")
FLOOR = c64.FLOOR_ULPS * 2.0 ** -23


def _step(mi, oracle, path, build, dt, iterations):
    """One step of a device world on `path` and of the oracle following it (row form): everything both sides hold afterwards, the
    contacts flattened manifold slot by manifold slot (the oracle's contact order in follow mode)."""
    env = {"MI_PHYSICS_NO_CLUSTER": "1"} if path == "launch_sweep" else {}
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        g = mi.World()                                   # the switches are read when the world is created
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if path == "replay":
        g.set_replay(True)
    ids = build(g)
    o = oracle.OracleWorld(solver=oracle.SOLVER_REPLAY if path == "replay" else oracle.SOLVER_CUSTOM)
    assert build(o) == ids
    run = dict(ids=ids, n=g.num_bodies, mass=g.mass_properties(), tr0=g.transforms(1), ve0=g.velocities(), dt=dt, iterations=iterations)
    assert np.array_equal(run["mass"].view(np.uint32), o.mass_properties().view(np.uint32))
    g.step_internal(dt, iterations)
    slots, counts, contacts4, bp = g.manifolds()
    order, cs = g.schedule()
    by_position = g.contact_impulses()
    run.update(vel=g.velocities(), tr=g.transforms(1), stats=g.stats(), batches=g.replay_batches(), order=order, colour_start=cs, counts=counts, slot_pairs=bp)
    g.close()
    o.set_follow(slots, order)
    o.step_internal(dt, iterations)
    assert np.array_equal(o.slot_counts().astype(np.uint32), counts), "contact counts differ"
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    mask = np.arange(4)[None, :] < counts[:, None]
    run["contacts"], run["pairs"], run["slot_start"] = contacts4[mask], np.repeat(bp, counts, axis=0), start
    assert np.array_equal(np.sort(order), np.flatnonzero(counts)), "the schedule is not a permutation of the manifolds with contacts"
    imp = np.zeros((int(start[-1]), 2), np.float32)
    for p, s in enumerate(order):
        imp[start[s]:start[s + 1]] = by_position[p, :counts[s]]
        assert not by_position[p, counts[s]:].any()
    run["impulses"] = imp
    oc, obp, _ = o.contacts()
    assert oc.tobytes() == run["contacts"].tobytes() and np.array_equal(obp, run["pairs"]), "the oracle's manifolds differ from the device's"
    run.update(o_vel=o.velocities(), o_tr=o.transforms(1), o_impulses=o.contact_impulses())
    # the order the contacts were solved in, for float64
    if path == "replay":
        e = run["batches"][run["batches"] != 0xFFFFFFFF]
        run["contact_order"] = [int(start[order[int(x) & 0x0FFFFFFF]] + (int(x) >> 28)) for x in e]
    else:
        run["contact_order"] = [int(i) for s in order for i in range(start[s], start[s + 1])]
    assert sorted(run["contact_order"]) == list(range(int(start[-1])))
    return run


def _bit_equal(run, what=""):
    assert np.isfinite(run["vel"]).all() and np.isfinite(run["tr"]).all() and np.isfinite(run["impulses"]).all(), what
    for k, o in (("vel", "o_vel"), ("tr", "o_tr"), ("impulses", "o_impulses")):
        same = run[k].view(np.uint32) == run[o].view(np.uint32)
        assert same.all(), (what, k, "not bit-equal to the row-form oracle at rows", np.flatnonzero(~same.reshape(len(same), -1).all(axis=1))[:8],
                            float(np.abs(run[k].astype(np.float64) - run[o]).max()))


def _against_float64(run, bodies, idx, group, what, worst=None):
    """One connected group against contact64 solved in the device's order: velocities, poses, impulses within the class tolerance."""
    pos = {c: k for k, c in enumerate(idx)}
    order = [pos[c] for c in run["contact_order"] if c in pos]
    ref = c64.reference(run["mass"], run["tr0"], run["ve0"], run["contacts"][idx], run["pairs"][idx], order, run["dt"], run["iterations"])
    tol_v, tol_i = c64.tolerance(group), c64.tolerance(group, "impulse")
    ev = max(float(np.abs(run["vel"][b].astype(np.float64) - v).max()) for b, v in ref["vel"].items()) / ref["scale"]
    ei = float(np.abs(run["impulses"][idx].astype(np.float64) - ref["impulses"]).max()) / ref["impulse_scale"] if ref["impulse_scale"] > 0.0 else 0.0
    if worst is not None:
        w = worst.setdefault(group, [(0.0, ""), (0.0, "")])
        w[0], w[1] = max(w[0], (ev, what)), max(w[1], (ei, what))
    assert sorted(ref["vel"]) == bodies
    assert ev <= tol_v, (what, "velocity", ev, tol_v)
    assert ei <= tol_i, (what, "impulse", ei, tol_i)
    assert ((run["impulses"][idx, 0] > 0.0) == (ref["impulses"][:, 0] > 0.0))[np.abs(ref["impulses"][:, 0]) > tol_i * ref["impulse_scale"]].all(), what
    assert (run["impulses"][idx, 0] >= 0.0).all(), what
    for b, (p, q) in ref["pose"].items():
        t = run["tr"][b].astype(np.float64)
        assert np.abs(t[:3] - p).max() <= tol_v * ref["scale"] * run["dt"] + 4 * 2.0 ** -23 * max(1.0, float(np.abs(p).max())), (what, b)
        assert min(np.abs(t[3:] - q).max(), np.abs(t[3:] + q).max()) <= tol_v * ref["scale"] * run["dt"] + 4 * 2.0 ** -23, (what, b)
    return ref


def _report(path, worst):
    for group in sorted(worst):
        (ev, nv), (ei, ni) = worst[group]
        print("%-12s %-8s vs contact64: velocity %.2e (%s) tolerance %.1e, impulse %.2e (%s) tolerance %.1e" % (
            path, group, ev, nv, c64.tolerance(group), ei, ni, c64.tolerance(group, "impulse")))


_runs = {}


def _cached(key, make):
    """One device run per key; it went wrong once: nothing of it is started on the GPU again."""
    if "error" in _runs:                                  # not a failed comparison: an error of the device or of the run itself
        raise RuntimeError("the %s run raised earlier in this session: %r" % _runs["error"])
    if key in _runs:
        if isinstance(_runs[key], BaseException):
            raise RuntimeError("the %s run failed earlier in this session: %r" % (key, _runs[key]))
        return _runs[key]
    try:
        _runs[key] = make()
    except BaseException as e:
        _runs[key] = e
        if not isinstance(e, AssertionError):
            _runs["error"] = (key, e)
        raise
    return _runs[key]


def _battery(mi, oracle, path):
    def make():
        out = []
        for key, cs in c64.groups(c64.battery()).items():
            placed = c64.place(cs)
            out.append((cs, _step(mi, oracle, path, lambda w: c64.build_world(w, cs, placed), key[0], key[1])))
        return out
    return _cached(("battery", path), make)


def _coupled(mi, oracle, path, name):
    g = c64.coupled()[name]
    return _cached((name, path), lambda: _step(mi, oracle, path, g["build"], g["dt"], g["iterations"]))


def _world_run(mi, oracle, path, name):
    g = c64.worlds()[name]
    return _cached((name, path), lambda: _step(mi, oracle, path, g["build"], g["dt"], g["iterations"]))


def _check_path(path, run, what):
    st = run["stats"]
    if path == "cluster":
        assert sum(st["clusterTasks"]) > 0 and st["numFlowRecoveries"] == 0, (what, st["clusterTasks"], st["numFlowRecoveries"])
    else:
        assert sum(st["clusterTasks"]) == 0, (what, st["clusterTasks"])
        assert (len(run["batches"]) > 0) == (path == "replay"), what
    assert st["numContacts"] == len(run["contacts"]) > 0, what


@pytest.mark.parametrize("path", PATHS)
def test_path_taken(mi, oracle, path):
    for cs, run in _battery(mi, oracle, path):
        _check_path(path, run, cs[0]["name"])
    for name in c64.coupled():
        _check_path(path, _coupled(mi, oracle, path, name), name)


@pytest.mark.parametrize("path", PATHS)
def test_bit_equal_to_the_row_form_oracle(mi, oracle, path):
    for cs, run in _battery(mi, oracle, path):
        _bit_equal(run, cs[0]["name"])
    for name in ("stack3", "hub5"):
        _bit_equal(_coupled(mi, oracle, path, name), name)


@pytest.mark.parametrize("path", PATHS)
def test_against_float64(mi, oracle, path):
    """Clear cases and ties alike: a tie sits on its threshold exactly, so float64 takes the branch the float32 input selects."""
    worst, seen = {}, 0
    for cs, run in _battery(mi, oracle, path):
        for c, ids in zip(cs, run["ids"]):
            idx = c64.contacts_of(ids, run["n"], run["contacts"], run["pairs"])
            assert idx, c["name"]
            ref = _against_float64(run, sorted(b for b in ids if b is not None), idx, c["group"], c["name"], worst)
            assert (c64.classify(c, ref) == "tie") == (c["name"] in c64.TIES)
            seen += 1
    assert seen == len(c64.battery())
    for name in ("stack3", "hub5"):
        run = _coupled(mi, oracle, path, name)
        comps = c64.components(run["n"], run["pairs"])
        assert len(comps) == 1 and len(run["contacts"]) == {"stack3": 12, "hub5": 5}[name]
        _against_float64(run, comps[0][0], comps[0][1], "coupled", name, worst)
    _report(path, worst)


@pytest.mark.parametrize("path", PATHS)
def test_zero_inverse_mass_pairs(mi, oracle, path):
    """Kinematic on static and kinematic on kinematic: the narrowphase keeps the manifold, constraints.cpp:3394-3397 skips its solve, the
    row form runs it with mN = mT = 0: no impulse, and the kinematic bodies' velocities come back as they went in."""
    seen = 0
    for cs, run in _battery(mi, oracle, path):
        for c, ids in zip(cs, run["ids"]):
            if "no_mass" not in c["tags"]:
                continue
            seen += 1
            idx = c64.contacts_of(ids, run["n"], run["contacts"], run["pairs"])
            assert len(idx) == (1 if "sphere" in c["name"] else 4), c["name"]
            for b in ids:
                if b is not None:
                    assert run["mass"][b, 3] == 0.0 and not run["mass"][b, 4:13].any(), c["name"]
                    assert np.array_equal(run["vel"][b].view(np.uint32), run["ve0"][b].view(np.uint32)), c["name"]
            assert not run["impulses"][idx].view(np.uint32).any(), (c["name"], run["impulses"][idx])
    assert seen >= 5


@pytest.mark.parametrize("path", PATHS)
def test_serial_colour(mi, oracle, path):
    """A hub box with 66 spheres on it: more partners than colours."""
    run = _coupled(mi, oracle, path, "hub66")
    _check_path(path, run, "hub66")
    assert len(run["contacts"]) == 66 and (run["pairs"] == 0).any(axis=1).all()
    cs = run["colour_start"]
    if path != "cluster":
        assert cs[65] > cs[64], "no manifold in the serial colour"
    assert run["stats"]["numFlowRecoveries"] == 0
    _bit_equal(run, "hub66")
    comps = c64.components(run["n"], run["pairs"])
    assert len(comps) == 1
    worst = {}
    _against_float64(run, comps[0][0], comps[0][1], "coupled", "hub66", worst)
    _report(path, worst)


def _colour_mix(run, colour):
    cs = run["colour_start"]
    return [int(x) for x in run["counts"][run["order"][cs[colour]:cs[colour + 1]]]]


def _check_world(run, what, sample=None):
    """Bit-equality with the oracle on everything, the float64 bound on every connected group (or on those of `sample` bodies)."""
    _bit_equal(run, what)
    worst, checked = {}, 0
    for bodies, idx in c64.components(run["n"], run["pairs"]):
        if sample is not None and not (set(bodies) & sample):
            continue
        _against_float64(run, bodies, idx, "coupled" if len(bodies) > 1 else "plain", "%s bodies %s" % (what, bodies), worst)
        checked += len(bodies)
    return worst, checked


@pytest.mark.parametrize("path", PATHS)
def test_count_from_slot_position(mi, oracle, path):
    """k_solve_color and k_solve_tail take a manifold's contact count from its position inside its colour (4, 3, 2, 1 contacts, in that
    order, between the colour's count boundaries): colours that mix every count, checked manifold by manifold."""
    run = _world_run(mi, oracle, path, "counts")
    _check_path(path, run, "counts")
    have = sorted(int(x) for x in run["counts"][run["counts"] > 0])
    assert have == sorted([4] * 5 + [2] * 3 + [1] * 7 + [4] * 9 + [3] * 2 + [1] * 3 + [2] * 2 + [4] * 2), have
    if path != "cluster":       # (the cluster sweep has no global colours: its tasks colour their own contacts)
        mix0, mix1 = _colour_mix(run, 0), _colour_mix(run, 1)
        print(path, "colour 0:", {k: mix0.count(k) for k in (4, 3, 2, 1)}, "colour 1:", {k: mix1.count(k) for k in (4, 3, 2, 1)})
        assert run["colour_start"][2] == run["colour_start"][65] == len(have), "two colours, no serial bucket"
        assert len(mix0) == 15 + 9 and len(mix1) == 9
        for mix in (mix0, mix1):
            assert mix == sorted(mix, reverse=True), "a colour's manifolds are not in the order of their contact counts"
        assert min(mix0.count(4), mix0.count(2), mix0.count(1)) >= 3 and sorted(mix0) != sorted(mix1)
        assert 3 in mix0 + mix1, "no three-contact manifold"
    worst, checked = _check_world(run, "counts", c64.worlds()["counts"]["sample"])
    assert checked == run["n"]
    _report(path, worst)


@pytest.mark.parametrize("world", sorted(c64.KERNEL_WORLDS))
@pytest.mark.parametrize("path", PATHS)
def test_launch_sweep_kernel_choice(mi, oracle, path, world):
    """The launch sweep's three shapes (runSolverSweep): one colour (k_solve_color), two to five colours none above 2048 manifolds (all of
    them in k_solve_tail's one workgroup), a colour above 2048 with others (k_solve_color for each)."""
    spheres, stacks, height = c64.KERNEL_WORLDS[world]
    run = _world_run(mi, oracle, path, world)
    _check_path(path, run, world)
    assert run["n"] == spheres + stacks * height <= 2200 and len(run["contacts"]) == spheres + 4 * stacks * height
    if path != "cluster":
        cs = run["colour_start"].astype(np.int64)
        sizes = [int(x) for x in np.diff(cs[:65]) if x]
        print(path, world, "colours:", sizes)
        assert cs[65] == cs[64], "no serial bucket expected"
        if world == "one_colour":
            assert sizes == [100]
        elif world == "small_colours":
            assert 2 <= len(sizes) <= 5 and max(sizes) <= 2048 and sizes[0] >= 40
        else:
            assert len(sizes) >= 2 and max(sizes) > 2048
    worst, checked = _check_world(run, world, c64.worlds()[world]["sample"])
    assert checked == min(run["n"], 64)
    _report(path, worst)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(c64.SCENE_STEPS))
def test_follow_against_the_reference_formula(mi, oracle, path, name):
    """The device against the oracle solving the same order with the REFERENCE FORMULA (cross-product anchor velocities,
    constraints.cpp:3381-3449), every step from identical inputs: within K x the distance of the oracle's own two formulations on the
    same scene and steps (contact64.E_FORMULATIONS, re-measured by test_oracle_contacts.py), never below the float32 floor."""
    from directx_renderer_kurth_amd import scenes
    scene = scenes.by_name(name)
    env = {"MI_PHYSICS_NO_CLUSTER": "1"} if path == "launch_sweep" else {}
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        g = scene.instantiate(mi.World())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if path == "replay":
        g.set_replay(True)
    o = scene.instantiate(oracle.OracleWorld(solver=oracle.SOLVER_REPLAY if path == "replay" else oracle.SOLVER_CUSTOM))
    o.set_row_form(False)
    bound = max(c64.K * c64.E_FORMULATIONS[name], FLOOR)
    worst, with_contacts = 0.0, 0
    for i in range(c64.SCENE_STEPS[name]):
        r = follow_step(g, o, scene.dt, 30, resync=True)
        assert r["pairs_equal"] and r["counts_equal"], "step %d" % i
        rel = r["vel_err"] / max(1.0, r["vel_scale"])
        worst, with_contacts = max(worst, rel), with_contacts + bool(r.get("num_contacts", 0))
        assert rel <= bound, "step %d: %.3e relative, bound %.3e" % (i, rel, bound)
    st = g.stats()
    print("%s %s: worst relative velocity difference to the reference formula per step %.2e over %d steps with contacts; bound %.2e" % (path, name, worst, with_contacts, bound))
    assert with_contacts >= c64.SCENE_STEPS[name] // 2 and st["numFlowRecoveries"] == 0
    assert (sum(st["clusterTasks"]) > 0) == (path == "cluster") and (len(g.replay_batches()) > 0) == (path == "replay")
    g.close()
