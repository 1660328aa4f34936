"""Float64 statement of the contact rows and their Gauss-Seidel sweep, independent of the oracle and of the device kernels, and the
contact battery.

Written from the scalar formulation of the reference: initializeCollisionVelocityConstraints (constraints.cpp:3307-3379),
solveCollisionVelocityConstraints (constraints.cpp:3381-3449), noz (math.h:595) and integrateVelocity (rigid_body.cpp:126-142).  Plain
numpy, float64 throughout; the inputs (poses, velocities, mass properties, and the world's own manifolds: point, depth, normal, packed
friction / restitution) are float32 values taken exactly.  The vector, quaternion and body helpers are joint64's.

`init` builds one contact's constraint and reports every branch predicate with its decision and its margin; `solve` runs N iterations
over a list of contacts in a given order, the friction row before the normal row, the friction limit from the normal impulse of before
this contact's normal row.  The sweep's clamps (max(.., 0) and the friction cone) are continuous in their arguments, so no predicate is
recorded for them.  `battery()` returns isolated body pairs built from real colliders, `coupled()` the groups whose result depends on
the order (a stack, a hub with 5 and with 66 partners); `classify` sorts each case into clear / tie by construction and refuses
anything else.

Contact counts: the narrowphase gives 1 contact for sphere on box, 2 for capsule on box, 4 for box on box, and 3 for a box turned 45
degrees whose corner reaches over the edge of the box below (the clipped overlap is a triangle): the cases "count/box3_*".
"""
import math
import numpy as np

from joint64 import (Body, Preds, K, FLOOR_ULPS, CAP, ORACLE_HEADROOM, MARGIN, _f, _f32, v3, qmul, qaxis, qnorm, normalize, mass_of,  # noqa: F401
                     far_base, _CELLS)

SPHERE, CAPSULE, OBB = 0, 1, 4
CONTACT_DTYPE = np.dtype([("point", "<f4", 3), ("depth", "<f4"), ("normal", "<f4", 3), ("friction_restitution", "<u4")])

# ---- tolerances -------------------------------------------------------------------------------------------------------------
# Per class: E_ORACLE is the worst deviation of the float32 reference-formula oracle (SOLVER_SCALAR, set_scalar_row_form(False)) from
# this file on the class, as measured on the CPU: velocities relative to the case's velocity scale max(1, |v|), impulses relative to
# the case's largest impulse.  tests/test_oracle_contacts.py prints both and re-checks them on every run (measurement and table within
# ORACLE_HEADROOM of each other, either way).  The device runs the same float32 arithmetic in row form, which sits about 1e-7 from the
# reference formula (measured on this battery by the same test), so it gets K times the figure, never less than FLOOR_ULPS float32
# ulps, and a class above CAP is not admitted.
# Classes: plain (counts, depths, restitution, friction inside the cone or off, body kinds, time steps, iterations), clamp (the
# friction cone or the normal row's max(.., 0) is active at the end), hard (1 : 1000 masses, the 0.05 x 0.05 x 4 m bar, a centre of gravity off the body origin), far
# (+-2000 m), coupled (stack and hubs, in one fixed order).  The connected groups of worlds() count too: an isolated body as plain, a
# pile or a stack as coupled.
E_ORACLE = {  # class: (velocity, impulse)
    "plain": (8.37e-7, 3.95e-7), "clamp": (1.41e-7, 1.15e-7), "hard": (1.84e-6, 1.93e-5), "far": (2.55e-7, 1.55e-7), "coupled": (4.45e-7, 1.13e-7),
    # plain: the battery alone shows 2.5e-7; the figure is a capsule of worlds()["counts"] that friction spins about its own axis (the
    # smallest moment of inertia of the file).  coupled: the battery's groups alone show 1.1e-7; the figure is a two-box stack of worlds().
    # hard: the velocity figure is the offset centre of gravity (rounded to float32 at its world coordinate, against a 0.25 m lever), the
    # impulse figure the bar: four contacts 5 cm apart share one impulse almost freely among themselves, their sum is as sharp as elsewhere
}


# The oracle's two float32 formulations of the sweep (the reference formula and the device's row form), both in the reference's emission
# order, stepped side by side on a scene from identical inputs at every step: the worst relative velocity difference of one step over
# SCENE_STEPS steps.  tests/test_oracle_contacts.py re-measures it; the device following the reference formula gets K times it per step.
SCENE_STEPS = {"c1": 90, "c3_small": 40}
E_FORMULATIONS = {"c1": 4.08e-7, "c3_small": 1.32e-6}


def formulation_distances(orc, name):
    """Per step of SCENE_STEPS[name]: (contacts, relative velocity difference row form vs reference formula from the same inputs)."""
    from directx_renderer_kurth_amd import scenes
    scene = scenes.by_name(name)
    a = scene.instantiate(orc.OracleWorld(solver=orc.SOLVER_SCALAR))
    b = scene.instantiate(orc.OracleWorld(solver=orc.SOLVER_SCALAR)); b.set_scalar_row_form(True)
    out = []
    for _ in range(SCENE_STEPS[name]):
        a.step_internal(scene.dt); b.step_internal(scene.dt)
        va, vb = a.velocities(), b.velocities()
        out.append((len(a.contacts()[0]), float(np.abs(va - vb).max() / max(1.0, np.abs(va).max()))))
        b.write_state(a.transforms(1), va, presort=False)     # the next step starts from the reference formula's state in both
    return out


def tolerance(group, what="velocity"):
    """Relative tolerance of a class for the device: x the case's velocity scale, or x its largest impulse."""
    return max(K * E_ORACLE[group][0 if what == "velocity" else 1], FLOOR_ULPS * 2.0 ** -23)


# ---- constants of the reference (constraints.cpp:3357-3364, math.h:595), as the float32 values the compiler sees ---------------------
CONSTANTS = dict(dt_threshold=_f(1e-5), slop=-_f(0.001), beta=_f(0.1), noz_threshold=_f(1e-8),
                 friction_first=1.0)   # 0: the normal row before the friction row (for the sensitivity test)


def decode(word):
    """(friction, restitution) of the packed 16 + 16 bit word, as the reference decodes it: (float)x / (float)0xFFFF."""
    word = int(word)
    return (word >> 16) / 65535.0, (word & 0xFFFF) / 65535.0


def static_body():
    return Body(np.zeros(3), (0.0, 0.0, 0.0, 1.0), np.zeros(3), np.zeros(3), 0.0, np.zeros(3), np.zeros(9))


# ---- one contact -------------------------------------------------------------------------------------------------------------------
def init(bodies, contact, pair, dt, constants=None, force=None):
    """The constraint of one contact (constraints.cpp:3317-3370).  bodies: index -> Body; contact: one CONTACT_DTYPE record; pair:
    (a, b).  Returns a dict with the constraint's fields, impulses at 0, and `preds`: (name, decision, margin, scale)."""
    c = dict(CONSTANTS); c.update(constants or {})
    P = Preds(force)
    A, B = bodies[pair[0]], bodies[pair[1]]
    point, n = np.asarray(contact["point"], np.float64), np.asarray(contact["normal"], np.float64)
    depth = float(contact["depth"])
    friction, restitution = decode(contact["friction_restitution"])
    rA, rB = point - A.pos, point - B.pos
    rel = (B.v + np.cross(B.w, rB)) - (A.v + np.cross(A.w, rA))
    t = rel - (n @ rel) * n
    sl = t @ t
    speed = math.sqrt(rel @ rel)
    # noz: the squared length is a sum of squares of differences of velocity components: its rounding scale is |t| |rel|
    if P.test("noz", sl < c["noz_threshold"], sl - c["noz_threshold"], max(c["noz_threshold"], math.sqrt(sl) * speed)):
        t = np.zeros(3)
    else:
        t = t * (1.0 / math.sqrt(sl))
    crAt, crBt = np.cross(rA, t), np.cross(rB, t)
    invT = A.invMass + crAt @ (A.invI @ crAt) + B.invMass + crBt @ (B.invI @ crBt)
    mT = 1.0 / invT if P.test("invT", invT != 0.0, invT, invT if invT != 0.0 else 1.0) else 0.0
    crAn, crBn = np.cross(rA, n), np.cross(rB, n)
    invN = A.invMass + crAn @ (A.invI @ crAn) + B.invMass + crBn @ (B.invI @ crBn)
    mN = 1.0 / invN if P.test("invN", invN != 0.0, invN, invN if invN != 0.0 else 1.0) else 0.0
    bias = 0.0
    if P.test("dt", dt > c["dt_threshold"], dt - c["dt_threshold"], c["dt_threshold"]):
        vrel = n @ rel
        deep = P.test("slop", -depth < c["slop"], -depth - c["slop"], abs(c["slop"]))
        closing = P.test("vrel", vrel < 0.0, vrel, max(1.0, speed))
        if deep and closing:
            bias = -restitution * vrel - c["beta"] * (-depth - c["slop"]) * (1.0 / dt)
    return dict(a=pair[0], b=pair[1], n=n, t=t, rA=rA, rB=rB, mT=mT, mN=mN, bias=bias, friction=friction, restitution=restitution,
                tA=A.invI @ crAt, tB=B.invI @ crBt, nA=A.invI @ crAn, nB=B.invI @ crBn, impN=0.0, impT=0.0, preds=list(P),
                friction_first=bool(c["friction_first"]))


def _anchor_velocity(A, B, k):
    return (B.v + np.cross(B.w, k["rB"])) - (A.v + np.cross(A.w, k["rA"]))


def _tangent_row(A, B, k):
    lam = -k["mT"] * (_anchor_velocity(A, B, k) @ k["t"])
    limit = k["friction"] * k["impN"]
    new = min(limit, max(-limit, k["impT"] + lam))
    lam, k["impT"] = new - k["impT"], new
    p = lam * k["t"]
    A.v -= A.invMass * p; A.w -= k["tA"] * lam; B.v += B.invMass * p; B.w += k["tB"] * lam


def _normal_row(A, B, k):
    lam = -k["mN"] * (_anchor_velocity(A, B, k) @ k["n"] - k["bias"])
    new = max(k["impN"] + lam, 0.0)
    lam, k["impN"] = new - k["impN"], new
    p = lam * k["n"]
    A.v -= A.invMass * p; A.w -= k["nA"] * lam; B.v += B.invMass * p; B.w += k["nB"] * lam


def solve_one(bodies, k):
    """One contact, once (constraints.cpp:3385-3448): nothing at all between two bodies without inverse mass."""
    A, B = bodies[k["a"]], bodies[k["b"]]
    if A.invMass == 0.0 and B.invMass == 0.0:
        return
    if k["friction_first"]:
        _tangent_row(A, B, k); _normal_row(A, B, k)
    else:
        _normal_row(A, B, k); _tangent_row(A, B, k)


def solve(bodies, contacts, pairs, order, dt, iterations, constants=None, force=None):
    """Initialise every contact from the pre-solve state, then `iterations` sweeps over `order` (indices into contacts).  bodies are
    modified in place (velocities).  Returns the constraints (impN, impT, preds, ...), parallel to contacts."""
    ks = [init(bodies, c, p, dt, constants, force) for c, p in zip(contacts, pairs)]
    for _ in range(iterations):
        for i in order:
            solve_one(bodies, ks[i])
    return ks


def reference(mass, transforms, velocities, contacts, pairs, order, dt, iterations, constants=None, force=None):
    """contact64 on the contacts given (all that touch the bodies they touch, or the result means nothing), from a world's float32
    state: mass = World.mass_properties(), transforms [n, 7], velocities [n, 6]; a body index >= n is the static body.
    Returns dict(vel {body: [6]}, pose {body: (pos, rot)}, impulses [len(contacts), 2], preds [per contact], scale, impulse_scale)."""
    n = len(transforms)
    pairs = [(int(a), int(b)) for a, b in pairs]
    bodies = {}
    for b in {x for p in pairs for x in p}:
        bodies[b] = Body(transforms[b, :3], transforms[b, 3:], velocities[b, :3], velocities[b, 3:], *mass_of(mass, b)) if b < n else static_body()
    before = [np.concatenate([bodies[b].v, bodies[b].w]) for b in bodies if b < n]
    ks = solve(bodies, contacts, pairs, order, dt, iterations, constants, force)
    vel = {b: np.concatenate([B.v, B.w]) for b, B in bodies.items() if b < n}
    imp = np.array([[k["impN"], k["impT"]] for k in ks], np.float64).reshape(-1, 2)
    return dict(vel=vel, pose={b: B.integrate(dt) for b, B in bodies.items() if b < n}, impulses=imp, preds=[k["preds"] for k in ks], constraints=ks,
                scale=max(1.0, float(np.abs(before).max()), float(np.abs(list(vel.values())).max())),
                impulse_scale=float(np.abs(imp).max()) if len(imp) else 0.0)


# ---- the battery ---------------------------------------------------------------------------------------------------------------
# Ties by construction: case name -> {predicate: why the float32 quantity sits on the threshold exactly}.
_ZERO_VN = "no velocity along the axis-aligned normal (0, 1, 0) and no spin: dot(n, rel) is a sum of exact zeros"
_DT_EXACT = "dt is the float32 value of 1e-5 itself: dt > 1e-5f is false in float32 as in float64"
_NO_MASS = "both bodies have inverse mass 0 and inverse inertia 0: the sum is an exact 0"
TIES = {}

_IDENT = (0.0, 0.0, 0.0, 1.0)
_Y45 = tuple(_f32(qaxis((0.0, 1.0, 0.0), math.pi / 4)))
_GENERIC_Q = (0.18257418, 0.36514837, -0.54772256, 0.73029674)
DYN, KIN, STATIC = "dynamic", "kinematic", "static"

# upper shape -> (collider type, shape, height of the collider's lowest point below the body origin); the lower box's top is y = 0.25
_LOWER_BOX = (OBB, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5, 0.25, 0.5))
_UPPER = {
    "sphere": ((SPHERE, (0.0, 0.0, 0.0, 0.25)), 0.25, (0.1, 0.0, 0.05)),
    "capsule": ((CAPSULE, (-0.25, 0.0, 0.0, 0.25, 0.0, 0.0, 0.125)), 0.125, (0.1, 0.0, 0.05)),
    "box": ((OBB, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.125, 0.25)), 0.125, (0.1, 0.0, 0.05)),
    # a box turned 45 degrees about y (by the body's rotation) whose corner reaches 0.25 m over the lower box's +x edge: a triangle
    "box3": ((OBB, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.125, 0.25)), 0.125, (0.5 + 0.35355339 - 0.25, 0.0, 0.0)),
    "bar": ((OBB, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.025, 0.025, 2.0)), 0.025, (0.0, 0.0, 0.0)),
    "offset_sphere": ((SPHERE, (0.0625, -0.03125, 0.046875, 0.25)), 0.25 + 0.03125, (0.1, 0.0, 0.05)),
}


def battery():
    """The list of cases.  A case: dict(name, group, tags, upper / lower (dicts: kind, collider, pos, rot, v, w, relative to the case's
    base; the lower one may be static), material (restitution, friction), densities, dt, iterations, far)."""
    cases = []

    def add(name, shape="sphere", depth=0.0078125, upper=DYN, lower=STATIC, vu=(0.25, -1.0, 0.125), wu=(0.0, 0.0, 0.0), vl=(0.0, 0.0, 0.0), wl=(0.0, 0.0, 0.0),
            e=0.0, mu=0.3, dt=1.0 / 120.0, iterations=6, far=False, group="plain", tags=(), dens=(1000.0, 1000.0), rot=_IDENT, lower_shape=None, ties=None):
        col, drop, off = _UPPER[shape]
        if shape == "box3":
            rot = _Y45
        up = dict(kind=upper, collider=col, pos=(off[0], 0.25 + drop - depth, off[2]), rot=rot, v=vu, w=wu, density=dens[0])
        lo = dict(kind=lower, collider=lower_shape or _LOWER_BOX, pos=(0.0, 0.0, 0.0), rot=_IDENT, v=vl, w=wl, density=dens[1])
        assert name not in {c["name"] for c in cases}, name
        cases.append(dict(name=name, group=group, tags=set(tags), upper=up, lower=lo, material=(e, mu), dt=float(np.float32(dt)), iterations=iterations, far=far))
        if ties:
            TIES[name] = dict(ties)

    # -- a collider offset from the body origin (first: nearest the origin, see near_base)
    add("bodies/offset_collider", "offset_sphere", wu=(0.5, 0.25, -0.5), group="hard", tags={"cog"})
    add("bodies/offset_collider_rotated", "offset_sphere", rot=(0.0, 0.38268343, 0.0, 0.92387953), wu=(0.5, 0.25, -0.5), lower=DYN, group="hard", tags={"cog", "momentum"})
    # -- contact counts x depths (inside the slop, barely touching, about 1 cm deep), approaching
    for shape in ("sphere", "capsule", "box", "box3"):
        add("count/%s_in_slop" % shape, shape, depth=0.00048828125)
        add("count/%s_touching" % shape, shape, depth=2.0 ** -20)
        add("count/%s_deep" % shape, shape, tags={"bias", "slop"} | ({"corner"} if shape == "box3" else set()))
    # -- normal velocity: zero (a tie: vRel == 0 exactly), separating (no bias although 1 cm deep)
    for shape in ("sphere", "box"):
        add("vn/%s_zero" % shape, shape, vu=(0.5, 0.0, 0.25), ties={"vrel": _ZERO_VN})
        add("vn/%s_separating" % shape, shape, vu=(0.25, 1.0, 0.125), group="clamp", tags={"separating"})
    add("vn/all_zero", "sphere", vu=(0.0, 0.0, 0.0), ties={"vrel": _ZERO_VN})
    # -- restitution
    for e in (0.0, 0.5, 1.0):
        add("restitution/sphere_%g" % e, "sphere", e=e, tags={"restitution"} if e else ())
        add("restitution/box_%g" % e, "box", e=e)
    # -- friction x tangential velocity
    tang = dict(zero=dict(vu=(0.0, -1.0, 0.0)), below_noz=dict(vu=(2.0 ** -15, -1.0, 2.0 ** -15)), stick=dict(vu=(0.03125, -1.0, 0.015625)),
                slide=dict(vu=(4.0, -1.0, 2.0)), spin=dict(vu=(0.0, -1.0, 0.0), wu=(3.0, 0.0, 1.0)))
    for mu, names in ((0.0, ("stick", "slide")), (0.3, ("zero", "below_noz", "stick", "slide", "spin")), (1.0, ("stick", "slide", "spin"))):
        for nm in names:
            sliding = nm == "slide" or mu == 0.0 or (nm == "spin" and mu < 1.0)
            add("friction/mu%g_%s" % (mu, nm), "sphere", mu=mu, group="clamp" if sliding else "plain",
                tags={"noz"} if nm == "below_noz" else ({"cone"} if nm == "slide" and mu else ({"order"} if nm == "stick" and mu else ())), **tang[nm])
    add("friction/box_mu0.3_slide", "box", mu=0.3, group="clamp", tags={"cone"}, **tang["slide"])
    add("friction/box_mu1_stick", "box", mu=1.0, **tang["stick"])
    add("friction/capsule_mu0.3_spin", "capsule", mu=0.3, group="clamp", vu=(0.0, -1.0, 0.0), wu=(3.0, 0.5, 0.0))
    # -- bodies
    no_mass = {"invT": _NO_MASS, "invN": _NO_MASS}
    for shape in ("sphere", "box"):
        add("bodies/%s_dyn_kin" % shape, shape, lower=KIN, vl=(0.5, 0.25, 0.0), wl=(0.0, 0.5, 0.0))
        add("bodies/%s_kin_static" % shape, shape, upper=KIN, wu=(0.5, 0.0, 0.25), tags={"no_mass"}, ties=no_mass)
        add("bodies/%s_kin_kin" % shape, shape, upper=KIN, lower=KIN, vl=(0.5, 0.25, 0.0), wu=(0.5, 0.0, 0.25), tags={"no_mass"}, ties=no_mass)
        add("bodies/%s_dyn_dyn" % shape, shape, lower=DYN, vl=(0.0, 0.5, 0.0), wl=(0.25, 0.0, 0.0), tags={"momentum"})
        ratio = 0.5 / {"sphere": 4.0 / 3.0 * math.pi * 0.25 ** 3, "box": 0.0625}[shape]    # volume of the lower box / of the upper collider
        add("bodies/%s_light_on_heavy" % shape, shape, lower=DYN, dens=(1000.0, 1.0e6 / ratio), group="hard", vl=(0.0, 0.5, 0.0), tags={"momentum"})   # 1 : 1000
        add("bodies/%s_heavy_on_light" % shape, shape, lower=DYN, dens=(1.0e6 * ratio, 1000.0), group="hard", vl=(0.0, 0.5, 0.0), tags={"momentum"})   # 1000 : 1
    add("bodies/capsule_dyn_dyn", "capsule", lower=DYN, wu=(0.0, 1.0, 0.5), tags={"momentum"})
    # the other type order: the sphere is the static one (collider A of the pair), the box the dynamic one (collider B)
    add("bodies/box_on_static_sphere", "box", lower_shape=(SPHERE, (0.1, 0.0, 0.05, 0.25)))
    add("bodies/box_on_kinematic_sphere", "box", lower=KIN, vl=(0.0, 0.25, 0.0), lower_shape=(SPHERE, (0.1, 0.0, 0.05, 0.25)))
    add("bodies/bar_45", "bar", rot=_Y45, group="hard", wu=(0.5, 0.0, 0.25), tags={"bar"})
    add("bodies/bar_45_dyn_dyn", "bar", rot=_Y45, lower=DYN, group="hard", wu=(0.5, 0.0, 0.25), tags={"momentum"})
    # -- time steps: above, on and below the threshold 1e-5f
    for nm, dt in (("60", 1.0 / 60.0), ("1e-3", 1e-3), ("below", 0.99e-5)):
        add("dt/sphere_" + nm, "sphere", dt=dt, e=0.5, tags={"dt"} if nm == "below" else ())
        add("dt/box_" + nm, "box", dt=dt)
    add("dt/sphere_on_threshold", "sphere", dt=1e-5, e=0.5, ties={"dt": _DT_EXACT})
    add("dt/box_on_threshold", "box", dt=1e-5, ties={"dt": _DT_EXACT})
    # -- iterations
    for it in (1, 2, 30):
        add("iterations/sphere_%d" % it, "sphere", iterations=it, vu=tang["stick"]["vu"], mu=1.0, tags={"order"})
        add("iterations/box_%d" % it, "box", iterations=it, lower=DYN)
    # -- far: the same basics 2 km out
    for shape in ("sphere", "capsule", "box"):
        add("far/%s_deep" % shape, shape, far=True, group="far", e=0.5)
    add("far/sphere_in_slop", "sphere", far=True, group="far", depth=0.00048828125)
    add("far/sphere_slide", "sphere", far=True, group="far", mu=0.3, **tang["slide"])
    add("far/sphere_spin", "sphere", far=True, group="far", mu=1.0, **tang["spin"])
    add("far/box_dyn_dyn", "box", far=True, group="far", lower=DYN, vl=(0.0, 0.5, 0.0), tags={"momentum"})
    add("far/box_kin_kin", "box", far=True, group="far", upper=KIN, lower=KIN, vl=(0.5, 0.25, 0.0), tags={"no_mass"}, ties=no_mass)
    return cases


def near_base(k):
    """Pairs 8 m apart on a grid around the origin, nearest cells first (the longest collider is the 4 m bar).  The centre of gravity of
    an offset collider is rounded to float32 at its world coordinate and the lever arm point - cog inherits that: 20 m out that is
    1e-6 of a 0.25 m lever, at joint64's 50 m spacing it was 4e-5.  Coordinates are the far class's business."""
    return 8.0 * v3(*_CELLS[k])


def groups(cases):
    """Cases by world: one world per (dt, iterations); returns {key: [case, ...]} in battery order."""
    out = {}
    for c in cases:
        out.setdefault((c["dt"], c["iterations"]), []).append(c)
    return out


def place(cases_of_world):
    """Absolute float32 poses and velocities of one world's cases, 50 m apart (joint64's grid; far cases at +-2000 m)."""
    out, near, far = [], 0, 0
    for c in cases_of_world:
        if c["far"]:
            base, far = far_base(far), far + 1
        else:
            base, near = near_base(near), near + 1
        out.append({s: dict(pos=_f32(base + np.asarray(c[s]["pos"], np.float64)), rot=_f32(c[s]["rot"]), v=_f32(c[s]["v"]), w=_f32(c[s]["w"])) for s in ("upper", "lower")})
    return out


def build_world(world, cases_of_world, placed):
    """One isolated pair per case (gravity off, no damping: the force integration is the identity, so the velocities written are the
    pre-solve velocities).  Returns the body ids per case: (upper, lower), lower None where it is static."""
    ids, tr, ve = [], [], []
    for c, pl in zip(cases_of_world, placed):
        pair = []
        for s in ("upper", "lower"):
            b, p = c[s], pl[s]
            mat = (c["material"][0], c["material"][1], b["density"])
            if b["kind"] == STATIC:
                world.add_static_collider(b["collider"][0], b["collider"][1], mat, pos=tuple(p["pos"]), rot=tuple(p["rot"]))
                pair.append(None)
                continue
            i = world.add_body(tuple(p["pos"]), tuple(p["rot"]), kinematic=b["kind"] == KIN, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
            world.add_collider(i, b["collider"][0], b["collider"][1], mat)
            assert i == len(tr)
            tr.append(np.concatenate([p["pos"], p["rot"]])); ve.append(np.concatenate([p["v"], p["w"]]))
            pair.append(i)
        ids.append(tuple(pair))
    world.write_state(np.array(tr, np.float32), np.array(ve, np.float32))
    return ids


def contacts_of(ids, num_bodies, contacts, pairs):
    """Indices of the contacts between the two bodies of one case (a static partner is body num_bodies), in the order given."""
    want = {ids[0], num_bodies if ids[1] is None else ids[1]}
    return [i for i, p in enumerate(pairs) if {int(p[0]), int(p[1])} == want]


def classify(case, ref):
    """'clear' or 'tie' for a case and its reference() result; raises for a case that is neither.
    clear: every predicate of every contact has margin >= MARGIN x its scale.  tie: the unclear predicates are exactly those listed in
    TIES for the case, and each sits on its threshold exactly (margin 0): the float32 input decides it as float64 does."""
    unclear = [(n, d, m) for preds in ref["preds"] for n, d, m, s in preds if m < MARGIN * s]
    if not unclear:
        assert case["name"] not in TIES, case["name"] + ": listed as a tie but clear"
        return "clear"
    assert case["name"] in TIES, (case["name"], "unclear predicates", unclear)
    assert {n for n, _, _ in unclear} == set(TIES[case["name"]]), (case["name"], unclear)
    assert all(m == 0.0 for _, _, m in unclear), (case["name"], unclear)
    return "tie"


# ---- coupled groups: the result depends on the order, which the caller supplies ------------------------------------------------------
def coupled():
    """name -> dict(build(world) -> number of bodies, dt, iterations).  Gravity off, no damping; everything moves into contact."""
    def stack(world):
        mat = (0.0, 0.5, 1000.0)
        world.add_static_collider(OBB, (0, 0, 0, 1, 0, 0, 0, 2.0, 0.25, 2.0), mat, pos=(0.0, -0.25, 0.0))
        tr, ve = [], []
        for k in range(3):
            pos = (0.03125 * k, 0.25 + 0.5 * k - 0.0078125 * (k + 1), -0.015625 * k)
            b = world.add_body(pos, _IDENT, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
            world.add_collider(b, OBB, (0, 0, 0, 1, 0, 0, 0, 0.25, 0.25, 0.25), mat)
            tr.append(pos + _IDENT); ve.append((0.125 * k, -1.0 - 0.5 * k, 0.0625, 0.0, 0.25 * k, 0.0))
        world.write_state(np.array(tr, np.float32), np.array(ve, np.float32))
        return 3

    def hub(count, columns):
        def build(world):
            mat = (0.25, 0.5, 1000.0)
            tr, ve = [(0.0, 0.0, 0.0) + _IDENT], [(0.0, 0.5, 0.0, 0.0, 0.0, 0.125)]
            b = world.add_body((0.0, 0.0, 0.0), _IDENT, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
            world.add_collider(b, OBB, (0, 0, 0, 1, 0, 0, 0, 1.5, 0.125, 1.5), mat)
            for k in range(count):
                pos = (-1.25 + 0.3125 * (k % columns), 0.125 + 0.125 - 0.0078125, -1.25 + 0.3125 * (k // columns))
                s = world.add_body(pos, _IDENT, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
                world.add_collider(s, SPHERE, (0.0, 0.0, 0.0, 0.125), mat)
                tr.append(pos + _IDENT); ve.append((0.03125 * (k % 5), -1.0 - 0.015625 * k, 0.0625, 0.5, 0.0, 0.25))
            world.write_state(np.array(tr, np.float32), np.array(ve, np.float32))
            return count + 1
        return build

    return {"stack3": dict(build=stack, dt=float(np.float32(1.0 / 120.0)), iterations=8),
            "hub5": dict(build=hub(5, 3), dt=float(np.float32(1.0 / 120.0)), iterations=8),
            "hub66": dict(build=hub(66, 9), dt=float(np.float32(1.0 / 120.0)), iterations=4)}   # 66 partners of one body: more than the 64 colours, so the last ones land in the serial bucket


# ---- worlds that reach every sweep kernel ------------------------------------------------------------------------------------------------
def pile_world(singles, piles, rows=8, pitch=2.0):
    """A static slab with isolated items on it (one manifold each) and piles (a dynamic box on the slab with an item on top: two
    manifolds sharing the box, so two colours).  An item is one of the battery's upper colliders: sphere (1 contact), capsule (2),
    box (4), and on a pile box3 (3: a corner over the lower box's edge)."""
    mat = (0.25, 0.5, 1000.0)
    items = [(k, False) for k in singles] + [(k, True) for k in piles]
    nrows = -(-len(items) // rows)

    def build(world):
        tr, ve = [], []

        def body(pos, rot, col, v):
            b = world.add_body(pos, rot, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
            world.add_collider(b, col[0], col[1], mat)
            tr.append(tuple(pos) + tuple(rot)); ve.append(v)
        world.add_static_collider(OBB, (0, 0, 0, 1, 0, 0, 0, 0.5 * pitch * rows + 1.0, 0.25, 0.5 * pitch * nrows + 1.0), mat, pos=(0.0, -0.25, 0.0))
        for i, (kind, pile) in enumerate(items):
            x, z, y = pitch * (i % rows - 0.5 * rows + 0.5), pitch * (i // rows - 0.5 * nrows + 0.5), 0.0
            if pile:
                body((x, 0.25 - 0.0078125, z), _IDENT, _LOWER_BOX, (0.0625, -0.5, 0.0, 0.0, 0.0, 0.0))
                y = 0.5 - 0.0078125
            col, drop, off = _UPPER[kind]
            assert kind != "box3" or pile
            body((x + off[0], y + drop - 0.0078125, z + off[2]), _Y45 if kind == "box3" else _IDENT, col, (0.125, -1.0 - 0.0078125 * (i % 7), 0.0625, 0.0, 0.0, 0.25))
        world.write_state(np.array(tr, np.float32), np.array(ve, np.float32))
        return len(tr)
    return build


def sphere_world(spheres, stacks, stack_height):
    """`spheres` isolated spheres on one static slab (all of one colour) and `stacks` stacks of `stack_height` boxes (one colour per storey)."""
    mat = (0.25, 0.5, 1000.0)
    side = int(np.ceil(np.sqrt(spheres + stacks)))

    def build(world):
        tr, ve = [], []
        world.add_static_collider(OBB, (0, 0, 0, 1, 0, 0, 0, 0.25 * side + 1.0, 0.25, 0.25 * side + 1.0), mat, pos=(0.0, -0.25, 0.0))
        for i in range(spheres + stacks):
            x, z = -0.25 * side + 0.5 * (i % side) + 0.25, -0.25 * side + 0.5 * (i // side) + 0.25
            if i < spheres:
                pos, col = [(x, 0.125 - 0.0078125, z)], (SPHERE, (0.0, 0.0, 0.0, 0.125))
            else:
                pos, col = [(x + 0.015625 * k, 0.125 + 0.25 * k - 0.0078125 * (k + 1), z) for k in range(stack_height)], (OBB, (0, 0, 0, 1, 0, 0, 0, 0.125, 0.125, 0.125))
            for k, p in enumerate(pos):
                b = world.add_body(p, _IDENT, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
                world.add_collider(b, col[0], col[1], mat)
                tr.append(p + _IDENT); ve.append((0.03125 * (i % 5), -1.0 - 0.25 * k - 0.00390625 * (i % 11), 0.0625, 0.0, 0.125 * (i % 3), 0.0))
        world.write_state(np.array(tr, np.float32), np.array(ve, np.float32))
        return len(tr)
    return build


COUNT_SINGLES = ["box"] * 5 + ["capsule"] * 3 + ["sphere"] * 7
COUNT_PILES = ["box3"] * 2 + ["sphere"] * 3 + ["capsule"] * 2 + ["box"] * 2
KERNEL_WORLDS = {"one_colour": (100, 0, 0), "small_colours": (40, 3, 3), "large_colour": (2100, 3, 2)}   # spheres, stacks, boxes per stack


def worlds():
    """name -> dict(build(world) -> number of bodies, dt, iterations, sample): the bodies whose connected groups are held to float64 (an
    isolated body is of class plain, a group of several of class coupled)."""
    dt = float(np.float32(1.0 / 120.0))
    out = {"counts": dict(build=pile_world(COUNT_SINGLES, COUNT_PILES), dt=dt, iterations=4, sample=set(range(len(COUNT_SINGLES) + 2 * len(COUNT_PILES))))}
    for name, (spheres, stacks, height) in KERNEL_WORLDS.items():
        picked = np.random.RandomState(7).choice(spheres, min(spheres, 64 - stacks * height), replace=False)
        out[name] = dict(build=sphere_world(spheres, stacks, height), dt=dt, iterations=4, sample={int(b) for b in picked} | set(range(spheres, spheres + stacks * height)))
    return out


def components(num_bodies, pairs):
    """The contacts by connected group of non-static bodies: [(bodies, contact indices)], pairs per contact."""
    parent = list(range(num_bodies))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        if a < num_bodies and b < num_bodies:
            parent[find(int(a))] = find(int(b))
    found = {}
    for i, (a, b) in enumerate(pairs):
        found.setdefault(find(int(min(a, b))), []).append(i)
    return [(sorted({int(x) for i in idx for x in pairs[i] if x < num_bodies}), idx) for idx in found.values()]
