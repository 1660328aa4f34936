"""The cloth kernel (csrc/k_cloth.hip) and its host half at the edges no scene reaches: the battery of cloth64.py (grids without a
constraint family, below / at / past the block size, at and past the LDS limit; every iteration kind alone and none; the invDt branch;
the stiffness clamp), in worlds whose cloth list interleaves LDS-sized and larger cloths.  Each case is held to the colour-ordered oracle
bit for bit and, independently of oracle/ocloth.h, to the float64 reading of the reference in cloth64.py; then the life of the particle
state between host and device: reads between steps, cloths added mid-run, property changes and bar moves without a read before them, a
world without a rigid body, snapshot and restore."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloth64 as c64  # noqa: E402

pytestmark = pytest.mark.gpu
STEPS = 12
READ_AFTER = (0, 1, 4, 5, 10, 11)   # step indices after which both worlds are read: around the first, second, sixth and twelfth step
MIX_231, MIX_302 = c64.MIXES.index((2, 3, 1)), c64.MIXES.index((3, 0, 2))
HALF_TURN_Y = (0.0, 1.0, 0.0, 0.0)
GENERIC = (0.36514837, -0.18257419, 0.54772256, 0.73029674)
ABOUT_X = (0.25881905, 0.0, 0.0, 0.96592583)


def _states(w, ids):
    return [w.cloth_state(i) for i in ids]


def _assert_same(got, want, what):
    for k, ((gp, gv), (wp, wv)) in enumerate(zip(got, want)):
        assert np.array_equal(gp, wp) and np.array_equal(gv, wv), "%s, cloth %d: max |dp| %g, max |dv| %g" % (what, k, np.abs(gp - wp).max(), np.abs(gv - wv).max())


def _step(worlds, dt, count=1, first=0):
    for k in range(first, first + count):
        for w in worlds:
            w.step_internal(float(c64.step_dt(dt, k)), 4)


def _run(worlds, dt, count):
    for _ in range(count):
        for w in worlds:
            w.step_internal(dt, 4)


_trajectories = {}


def _trajectory(mi, oracle, mix):
    """The device's and the oracle's world of one mix, stepped STEPS times with the same calls: (cases, {step index: device states},
    {step index: oracle states}); index -1 is the state before the first step."""
    if mix not in _trajectories:
        g, cases, ids = c64.build_world(mi.World, mix)
        o, _, _ = c64.build_world(oracle.OracleWorld, mix)
        dev, orc = {-1: _states(g, ids)}, {-1: _states(o, ids)}
        for k in range(STEPS):
            _step((g, o), cases[0].dt, 1, k)
            if k in READ_AFTER:
                dev[k], orc[k] = _states(g, ids), _states(o, ids)
        _trajectories[mix] = (cases, dev, orc)
    return _trajectories[mix]


def _assert_within_reading(cases, before, after, k, what):
    """the device's step with index k from its own state before it, against step64, within 4 x the table"""
    dt = c64.step_dt(cases[0], k)
    for case, (p0, v0), (p1, v1) in zip(cases, before, after):
        p64, v64 = c64.step64(case.cloth64(), p0, v0, case.wind, case.iterations, dt)
        dp, dv = c64.deviation(p1, v1, p64, v64, case.iterations, dt)
        ep, ev = c64.E_F32[c64.mix_class(case.iterations)]
        print("%s %s: positions %.3g of %.3g units, velocities %.3g of %.3g" % (what, case.name, dp, ep, dv, ev))
        assert dp <= c64.TOLERANCE * ep and dv <= c64.TOLERANCE * ev, "%s %s: positions %.3g of %.3g units, velocities %.3g of %.3g" % (what, case.name, dp, ep, dv, ev)


# ---------------------------------------------------------------------------------------------------------------------------
# The battery
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_bit_equal_to_the_oracle(mi, oracle, mix):
    """every case: positions and velocities equal the colour-ordered oracle bit for bit as built and after steps 1, 2 and 12"""
    cases, dev, orc = _trajectory(mi, oracle, mix)
    assert [k.n for k in cases][:3] == [2343, 4, 2340]   # the interleaved order: the kernel's list is a reordering
    for k in (-1, 0, 1, 11):
        _assert_same(dev[k], orc[k], "mix %s after step %d" % (c64.MIXES[mix], k + 1))
    moved = [float(np.abs(p1 - p0).max()) for (p0, _), (p1, _) in zip(dev[-1], dev[11])]
    assert all(np.isfinite(p).all() and np.isfinite(v).all() for p, v in dev[11])
    assert sum(m > 1e-4 for m in moved) >= 7, moved   # (gravity factor 0 without wind leaves a cloth where it is)


@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_against_the_float64_reading(mi, oracle, mix):
    """every case, at the first, the second and the twelfth step: the device's state after the step within 4 x cloth64.E_F32 of step64
    from the device's state before it.  Nothing here goes through oracle/ocloth.h.  (The first step is the one just above dt = 1e-5
    and moves next to nothing; the second is the first at the running dt, from the construction pose.)"""
    cases, dev, _ = _trajectory(mi, oracle, mix)
    assert c64.step_dt(cases[0], 0) == c64.DT_ABOVE and c64.step_dt(cases[0], 1) == np.float32(cases[0].dt)
    _assert_within_reading(cases, dev[-1], dev[0], 0, "step 1")
    _assert_within_reading(cases, dev[0], dev[1], 1, "step 2")
    _assert_within_reading(cases, dev[10], dev[11], 11, "step 12")


@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_dt_boundary(mi, oracle, mix):
    """dt = 1e-5 (invDt = 1): the sixth step, which meets a cloth in motion, bit for bit against the oracle and against step64, which
    decides dt > 1e-5 on the float32 values.  (The next float32 above 1e-5, invDt = 1 / dt, is the first step of every world: the two
    tests above hold it.)"""
    cases, dev, orc = _trajectory(mi, oracle, mix)
    assert c64.step_dt(cases[0], 0) == c64.DT_ABOVE and c64.step_dt(cases[0], 5) == c64.DT_EDGE
    _assert_same(dev[5], orc[5], "mix %s after step 6" % (c64.MIXES[mix],))
    _assert_within_reading(cases, dev[4], dev[5], 5, "dt 1e-5")
    if c64.MIXES[mix][1] > 0:
        # The branch is visible: a position pass at invDt = 1 leaves v = p - prev = v dt + the pass's corrections, millimetres at most, where
        # 1 / dt would have left v + corrections x 1e5.  Cloths that moved at 5 cm/s or more are all but at rest afterwards.
        fast = [k for k, (_, v) in enumerate(dev[4]) if np.abs(v).max() > 0.05]
        assert len(fast) >= 5 and all(np.abs(dev[5][k][1]).max() < 0.05 * np.abs(dev[4][k][1]).max() for k in fast)


# ---------------------------------------------------------------------------------------------------------------------------
# The life of the state
# ---------------------------------------------------------------------------------------------------------------------------
def test_reads_between_steps_and_repeated_runs(mi, oracle):
    """Reading cloth_state after every step does not change the trajectory (a twin reads only at the end), and the interleaved world
    built twice gives equal bytes after 12 steps (with the oracle equality nearly implied; it names the failure if a colour ever races)."""
    cases, _, orc = _trajectory(mi, oracle, MIX_231)
    worlds = [c64.build_world(mi.World, MIX_231) for _ in range(3)]
    reader, ids = worlds[0][0], worlds[0][2]
    for k in range(STEPS):
        _step([w for w, _, _ in worlds], cases[0].dt, 1, k)
        _states(reader, ids)
    ends = [_states(w, ids) for w, _, _ in worlds]
    _assert_same(ends[0], ends[1], "read every step against read at the end")
    _assert_same(ends[1], ends[2], "the same world built twice")
    _assert_same(ends[1], orc[11], "read at the end against the oracle")


def _small_world(make, grids, mix=MIX_231, body=True, rot=None):
    """cloths of the battery's shapes (grid indices into cloth64.GRIDS) under the mix's wind; rot: one rotation for all, not the battery's"""
    w = make()
    if body:
        c64.far_body(w)
    cases = [c64.Case(g, mix) for g in grids]
    for k in cases:
        k.rot = k.rot if rot is None else rot
    ids = [k.instantiate(w) for k in cases]
    w.set_cloth_iterations(*c64.MIXES[mix]); w.set_cloth_colour_order(True)
    if cases[0].wind is not None:
        w.add_force_field(cases[0].wind)
    return w, cases, ids


G2x2, G2x3, G3x3, G4x5, G32x16, G27x19, G52x45, G33x71 = 0, 1, 3, 4, 5, 6, 7, 9


@pytest.mark.parametrize("grids,added", [((G4x5, G27x19), G32x16), ((G32x16, G3x3), G33x71), ((G33x71, G4x5), G2x2)],
                         ids=["lds-into-lds", "first-large", "small-behind-large"])
def test_cloth_added_mid_run(mi, oracle, grids, added):
    """A cloth added after five steps, with no read before it: the particle state lives on the device, the stride changes, and the
    download has to happen before the push.  The old cloths continue bit-equal to the oracle and to a twin that got no new cloth; the new
    one starts from its construction pose.  (an LDS-sized cloth into a world of such; a large one into a world that had none, so the
    second kernel's first launch happens mid-run; a small one behind a large one, which the list moves in front of it)"""
    (g, cases, ids), (o, _, _), (twin, _, _) = (_small_world(m, grids) for m in (mi.World, oracle.OracleWorld, mi.World))
    dt = 1.0 / 120.0
    _run((g, o, twin), dt, 5)
    new = c64.Case(added, MIX_231)
    new_ids = [new.instantiate(w) for w in (g, o)]
    assert new_ids == [len(grids)] * 2
    all_ids = ids + [new_ids[0]]
    _assert_same(_states(g, all_ids), _states(o, all_ids), "right after the add")
    p, v = g.cloth_state(new_ids[0])
    assert not np.any(v) and np.abs(p - c64.set_fixed64(new.cloth64(), new.cloth64().p0, new.pos, new.rot, True)).max() <= c64.TOLERANCE * c64.E_F32_FIXED * c64.EPS32 * max(1.0, np.abs(p).max())
    _run((g, o, twin), dt, 7)
    _assert_same(_states(g, all_ids), _states(o, all_ids), "seven steps after the add")
    _assert_same(_states(g, ids), _states(twin, ids), "the old cloths against a twin without the new one")
    assert np.abs(g.cloth_state(new_ids[0])[0] - p).max() > 1e-5


def test_properties_changed_mid_run(mi, oracle):
    """cloth_set_properties after five steps without a read before it: a mass change on a large cloth, stiffness 5.0 and 0.001 (clamped
    to 1 and 0.01) on two LDS-sized ones.  Bit-equal to the oracle given the same calls, and different from a twin that skipped them."""
    (g, cases, ids), (o, _, _), (twin, _, _) = (_small_world(m, (G33x71, G32x16, G2x3)) for m in (mi.World, oracle.OracleWorld, mi.World))
    assert all(k.stiffness == 0.5 for k in cases)
    dt = 1.0 / 120.0
    _run((g, o, twin), dt, 5)
    for w in (g, o):
        w.cloth_set_properties(ids[0], 2.0 * cases[0].mass, cases[0].stiffness, cases[0].damping, cases[0].gravity_factor)
        w.cloth_set_properties(ids[1], cases[1].mass, 5.0, cases[1].damping, cases[1].gravity_factor)
        w.cloth_set_properties(ids[2], cases[2].mass, 0.001, cases[2].damping, cases[2].gravity_factor)
    _run((g, o, twin), dt, 1)
    _assert_same(_states(g, ids), _states(o, ids), "one step after the change")
    _run((g, o, twin), dt, 5)
    got = _states(g, ids)
    _assert_same(got, _states(o, ids), "six steps after the change")
    for (gp, _), (tp, _) in zip(got, _states(twin, ids)):
        assert not np.array_equal(gp, tp)


@pytest.mark.parametrize("move_rigid", [True, False])
@pytest.mark.parametrize("rot", [HALF_TURN_Y, GENERIC], ids=["half-turn", "generic"])
def test_bar_moved_mid_run(mi, oracle, move_rigid, rot):
    """cloth_set_fixed_vertices after five steps without a read before it, rigid and not, on even gridX (4 x 5, 52 x 45) and odd (27 x 19,
    33 x 71), with a half turn about y and a generic rotation: equal to the oracle right after the call and after five more steps, and
    within the float32 figure of the float64 reading of the call.  All four cloths hang tilted about x, their bars along x, so the half
    turn asks rotateFromTo for x to -x, its antiparallel branch, with the even and with the odd pivot."""
    grids = (G4x5, G33x71, G27x19, G52x45)
    (g, cases, ids), (o, _, _) = (_small_world(m, grids, rot=ABOUT_X) for m in (mi.World, oracle.OracleWorld))
    dt = 1.0 / 120.0
    _run((g, o), dt, 5)
    before = _states(o, ids)   # (the oracle's: reading the device here would hide a missing download)
    for case, (p0, _) in zip(cases, before):
        bar = (p0[case.gx - 1] - p0[0]).astype(np.float64)
        d = float(np.dot(bar / np.linalg.norm(bar), c64._qrot(np.asarray(rot, np.float64), [1.0, 0.0, 0.0])[0]))
        assert (d < 1e-6 - 1.0) == (rot is HALF_TURN_Y), (case.name, d)
    for w in (g, o):
        for i, case in zip(ids, cases):
            w.cloth_set_fixed_vertices(i, (case.pos[0] + 0.5, case.pos[1] - 0.25, case.pos[2] + 1.0), rot, move_rigid)
    after = _states(g, ids)
    _assert_same(after, _states(o, ids), "right after the call")
    for case, (p0, v0), (p1, v1) in zip(cases, before, after):
        p64 = c64.set_fixed64(case.cloth64(), p0, (case.pos[0] + 0.5, case.pos[1] - 0.25, case.pos[2] + 1.0), rot, move_rigid)
        assert np.abs(p1 - p64).max() <= c64.TOLERANCE * c64.E_F32_FIXED * c64.EPS32 * max(1.0, np.abs(p64).max()), case.name
        assert np.array_equal(v1, v0)
    _run((g, o), dt, 5)
    _assert_same(_states(g, ids), _states(o, ids), "five steps after the call")


def test_world_without_a_rigid_body(mi, oracle):
    """The reference returns from its step before the cloths when there is no rigid body: 10 steps leave two cloths (one per kernel
    variant) untouched, on the device and in the oracle.  Adding a body starts them, and they stay equal for 10 more steps."""
    (g, cases, ids), (o, _, _) = (_small_world(m, (G32x16, G33x71), body=False) for m in (mi.World, oracle.OracleWorld))
    start = _states(o, ids)
    _run((g, o), 1.0 / 120.0, 10)
    _assert_same(_states(g, ids), start, "device, ten steps without a body")
    _assert_same(_states(o, ids), start, "oracle, ten steps without a body")
    for w in (g, o):
        c64.far_body(w)
    _run((g, o), 1.0 / 120.0, 10)
    end = _states(g, ids)
    _assert_same(end, _states(o, ids), "ten steps with a body")
    assert all(np.abs(p1 - p0).max() > 1e-4 for (p0, _), (p1, _) in zip(start, end))


def test_snapshot_mid_run(mi, oracle):
    """snapshot at step 6 of the interleaved world with mix (3, 0, 2): the restored world and the original continue bit-equal for six
    steps, and end where the oracle ends"""
    cases, _, orc = _trajectory(mi, oracle, MIX_302)
    g, _, ids = c64.build_world(mi.World, MIX_302)
    _step((g,), cases[0].dt, 6, 0)
    r = mi.World.restore(g.snapshot())
    _step((g, r), cases[0].dt, 6, 6)
    end = _states(r, ids)
    _assert_same(end, _states(g, ids), "restored against original")
    _assert_same(end, orc[11], "restored against the oracle")
