"""Float64 statement of the six joint types, independent of the oracle and of the device kernels, and the joint battery.

Written from the scalar formulations of the reference (constraints.cpp:189-264 distance, 460-528 ball, 736-823 fixed, 1079-1307
hinge, 1782-2070 cone-twist, 2638-2846 slider), its joint constructors (physics.cpp:147-333), its math helpers (math.cpp:528-592
rotateFromTo / getAxisRotation, 1342-1371 solveLinearSystem, 1416-1426 getTangents, math.h:595 noz, 932-936 quat(axis, angle)) and
integrateVelocity (rigid_body.cpp:126-142).  Plain numpy, float64 throughout; the inputs are float32 values taken exactly.

`derive` turns the global construction arguments into the local frames of the POD; `solve` runs one joint between two bodies for N
iterations in the reference's row order and reports every branch predicate of the initialisation with its decision and its margin.
`battery()` returns the cases; `classify` sorts each into clear / tie by construction and refuses anything else.
"""
import math
import numpy as np

DISTANCE, BALL, FIXED, HINGE, CONE_TWIST, SLIDER = range(6)
TYPE_NAMES = ("distance", "ball", "fixed", "hinge", "cone_twist", "slider")
VELOCITY_MOTOR, POSITION_MOTOR = 0, 1
SPHERE, CAPSULE = 0, 1

# ---- tolerances -------------------------------------------------------------------------------------------------------------
# Per class (joint type, tag group): E_ORACLE is the scalar oracle's own worst deviation from this file on the class, relative to the
# case's velocity scale max(1, |v|), as measured on the CPU (tests/test_oracle_joints.py prints it and re-checks it on every run: the
# oracle may sit up to ORACLE_HEADROOM above the figure, and the figure may not sit more than ORACLE_HEADROOM above the oracle).  The
# device differs from the oracle only in the last ulp of atan2f / acosf / sinf / cosf feeding the same float32 arithmetic, so it gets
# K times the measured figure, and never less than FLOOR_ULPS float32 ulps of the velocity scale.  A class above CAP is
# ill-conditioned and proves nothing: it is not admitted.
K = 4.0
FLOOR_ULPS = 4.0
CAP = 1e-3
ORACLE_HEADROOM = 1.5  # for the oracle's own CPU check only (another libm, another compiler): never part of the device's tolerance
MARGIN = 1e-4          # a predicate is clear when its margin is at least MARGIN x the scale of the quantities compared
E_ORACLE = {
    # (type, group): measured worst.  Groups: plain (body kinds, centre of gravity, 1 cm lever, time steps, type-specific rows without
    # libm), trig (hinge / cone-twist limits and motors), hard (1 : 1e4 masses, 500 : 1 inertia, 10 m lever), far (+-2000 m, |v| up to 10).
    # Every class is dominated by the float32 cancellation in (B.pos + rB) - (A.pos + rA), which the 0.1 / dt bias multiplies by 12.
    (DISTANCE, "plain"): 7.56e-6, (DISTANCE, "hard"): 1.95e-5, (DISTANCE, "far"): 1.02e-4,
    (BALL, "plain"): 1.02e-4, (BALL, "hard"): 8.97e-6, (BALL, "far"): 9.21e-5,
    (FIXED, "plain"): 5.41e-5, (FIXED, "hard"): 1.28e-5, (FIXED, "far"): 8.96e-5,
    (HINGE, "plain"): 4.40e-5, (HINGE, "hard"): 1.04e-5, (HINGE, "trig"): 4.20e-5, (HINGE, "far"): 4.81e-5,
    (CONE_TWIST, "plain"): 6.14e-5, (CONE_TWIST, "hard"): 3.91e-5, (CONE_TWIST, "trig"): 7.40e-5, (CONE_TWIST, "far"): 8.46e-5,
    (SLIDER, "plain"): 4.88e-5, (SLIDER, "hard"): 5.31e-5, (SLIDER, "far"): 1.33e-4,
}


def tolerance(case):
    """Relative velocity tolerance of a case for the device (x its velocity scale)."""
    return max(K * E_ORACLE[(case["type"], case["group"])], FLOOR_ULPS * 2.0 ** -23)


# ---- constants of the reference (constraints.cpp:9-17), as the float32 values the compiler sees --------------------------------
def _f(x):
    return float(np.float32(x))


CONSTANTS = dict(beta_distance=_f(0.1), beta_ball=_f(0.1), beta_slider=_f(0.1), beta_hinge_rot=_f(0.3), beta_hinge_limit=_f(0.1),
                 beta_twist_limit=_f(0.1), beta_slider_limit=_f(0.1), dt_threshold=_f(1e-5),
                 rot_bias_factor=2.0,       # rotationError.v * (beta * invDt * 2)  (fixed, slider)
                 swing_pm_factor=_f(0.2),   # swing position motor: deltaAngle * invDt * 0.2
                 limit_sign=1.0,            # -1: min / max limit signs flipped
                 swap_tangents=0.0,         # 1: the tangent and bitangent biases of the hinge rotation / slider translation rows exchanged
                 pm_clamp=1.0)              # scales the clamp bounds of the position motors' targets


# ---- math (math.h / math.cpp) -------------------------------------------------------------------------------------------------
def v3(*a):
    return np.array(a, np.float64)


def qmul(a, b):
    av, bv = a[:3], b[:3]
    return np.concatenate([av * b[3] + bv * a[3] + np.cross(av, bv), [a[3] * b[3] - av @ bv]])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qrot(q, v):
    return qmul(qmul(q, np.concatenate([v, [0.0]])), qconj(q))[:3]


def qaxis(axis, angle):
    return np.concatenate([np.asarray(axis, np.float64) * math.sin(angle * 0.5), [math.cos(angle * 0.5)]])


def qnorm(q):
    return q / math.sqrt(q @ q)


def qmat(q):
    return np.stack([qrot(q, v3(1, 0, 0)), qrot(q, v3(0, 1, 0)), qrot(q, v3(0, 0, 1))], axis=1)


def normalize(v):
    return v / math.sqrt(v @ v)


def skew(r):
    return np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], np.float64)


def get_tangent(n):
    t = v3(n[1], -n[0], 0.0) if abs(n[0]) >= _f(0.57735) else v3(0.0, n[2], -n[1])
    return normalize(t)


def get_tangents(n):
    t = get_tangent(n)
    return t, np.cross(n, t)


def solve2(m, b):
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    if det != 0.0:
        det = 1.0 / det
    return np.array([det * (m[1, 1] * b[0] - m[0, 1] * b[1]), det * (m[0, 0] * b[1] - m[1, 0] * b[0])])


def solve3(m, b):
    ex, ey, ez = m[:, 0], m[:, 1], m[:, 2]
    det = ex @ np.cross(ey, ez)
    if det != 0.0:
        det = 1.0 / det
    return np.array([det * (b @ np.cross(ey, ez)), det * (ex @ np.cross(b, ez)), det * (ex @ np.cross(ey, b))])


def clamp(x, lo, hi):
    return min(hi, max(lo, x))


class Preds(list):
    """Branch predicates of one initialisation: (name, decision, margin, scale).  `force` overrides decisions by name."""

    def __init__(self, force=None):
        super().__init__()
        self.force = force or {}

    def test(self, name, decision, margin, scale):
        self.append((name, bool(decision), abs(float(margin)), float(scale)))
        return self.force.get(name, bool(decision))


def rotate_from_to(a, b, P):
    f, t = normalize(a), normalize(b)
    d = f @ t
    if P.test("rft_identity", d >= 1.0, d - 1.0, 1.0):
        return np.array([0.0, 0.0, 0.0, 1.0]), "identity"
    if P.test("rft_antiparallel", d < _f(1e-6) - 1.0, d - (_f(1e-6) - 1.0), 1.0):
        axis = np.cross(v3(1, 0, 0), f)
        if axis @ axis == 0.0:
            axis = np.cross(v3(0, 1, 0), f)
        return qnorm(qaxis(normalize(axis), _f(math.pi))), "antiparallel"
    s = math.sqrt((1.0 + d) * 2.0)
    c = np.cross(f, t)
    return qnorm(np.concatenate([c / s, [s * 0.5]])), "general"


# ---- constructors (physics.cpp:147-333): global arguments -> POD ---------------------------------------------------------------
def derive(jtype, TA, TB, args):
    """TA / TB: (position, rotation) of the two entities at construction.  Returns the POD as a dict of float64 fields."""
    (pA, qA), (pB, qB) = [(np.asarray(p, np.float64), np.asarray(q, np.float64)) for p, q in (TA, TB)]
    inv_pos = lambda p, q, g: qrot(qconj(q), np.asarray(g, np.float64) - p)
    inv_dir = lambda q, d: qrot(qconj(q), np.asarray(d, np.float64))
    if jtype == DISTANCE:
        gA, gB = np.asarray(args["anchor_a"], np.float64), np.asarray(args["anchor_b"], np.float64)
        return dict(localAnchorA=inv_pos(pA, qA, gA), localAnchorB=inv_pos(pB, qB, gB), globalLength=math.sqrt((gA - gB) @ (gA - gB)))
    pod = dict(localAnchorA=inv_pos(pA, qA, args["anchor"]), localAnchorB=inv_pos(pB, qB, args["anchor"]))
    if jtype in (FIXED, SLIDER):
        pod["initialInvRotationDifference"] = qmul(qconj(qB), qA)
    if jtype == HINGE:
        pod["localHingeAxisA"], pod["localHingeAxisB"] = inv_dir(qA, args["axis"]), inv_dir(qB, args["axis"])
        pod["localHingeTangentA"], pod["localHingeBitangentA"] = get_tangents(pod["localHingeAxisA"])
        pod["localHingeTangentB"] = qrot(qconj(qB), qrot(qA, pod["localHingeTangentA"]))
        pod.update(minRotationLimit=float(args.get("min", 1.0)), maxRotationLimit=float(args.get("max", -1.0)),
                   maxMotorTorque=-1.0, motorType=VELOCITY_MOTOR, motorVelocity=0.0)
    if jtype == CONE_TWIST:
        pod["localLimitAxisA"], pod["localLimitAxisB"] = inv_dir(qA, args["axis"]), inv_dir(qB, args["axis"])
        pod["localLimitTangentA"], pod["localLimitBitangentA"] = get_tangents(pod["localLimitAxisA"])
        pod["localLimitTangentB"] = qrot(qconj(qB), qrot(qA, pod["localLimitTangentA"]))
        pod.update(swingLimit=float(args["swing"]), twistLimit=float(args["twist"]), swingMotorType=VELOCITY_MOTOR, swingMotorVelocity=0.0,
                   maxSwingMotorTorque=-1.0, swingMotorAxis=0.0, twistMotorType=VELOCITY_MOTOR, twistMotorVelocity=0.0, maxTwistMotorTorque=-1.0)
    if jtype == SLIDER:
        pod["localAxisA"] = inv_dir(qA, args["axis"])
        pod.update(negDistanceLimit=float(args.get("min", 1.0)), posDistanceLimit=float(args.get("max", -1.0)),
                   maxMotorForce=-1.0, motorType=VELOCITY_MOTOR, motorVelocity=0.0)
    return pod


POD_DTYPES = (
    np.dtype([("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3), ("globalLength", "<f4")]),
    np.dtype([("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3)]),
    np.dtype([("initialInvRotationDifference", "<f4", 4), ("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3)]),
    np.dtype([("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3), ("localHingeAxisA", "<f4", 3), ("localHingeAxisB", "<f4", 3),
              ("minRotationLimit", "<f4"), ("maxRotationLimit", "<f4"), ("maxMotorTorque", "<f4"), ("motorType", "<u4"), ("motorVelocity", "<f4"),
              ("localHingeTangentA", "<f4", 3), ("localHingeBitangentA", "<f4", 3), ("localHingeTangentB", "<f4", 3)]),
    np.dtype([("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3), ("localLimitAxisA", "<f4", 3), ("localLimitAxisB", "<f4", 3),
              ("localLimitTangentA", "<f4", 3), ("localLimitBitangentA", "<f4", 3), ("localLimitTangentB", "<f4", 3),
              ("swingLimit", "<f4"), ("twistLimit", "<f4"), ("swingMotorType", "<u4"), ("swingMotorVelocity", "<f4"), ("maxSwingMotorTorque", "<f4"),
              ("swingMotorAxis", "<f4"), ("twistMotorType", "<u4"), ("twistMotorVelocity", "<f4"), ("maxTwistMotorTorque", "<f4")]),
    np.dtype([("initialInvRotationDifference", "<f4", 4), ("localAnchorA", "<f4", 3), ("localAnchorB", "<f4", 3), ("localAxisA", "<f4", 3),
              ("negDistanceLimit", "<f4"), ("posDistanceLimit", "<f4"), ("maxMotorForce", "<f4"), ("motorType", "<u4"), ("motorVelocity", "<f4")]),
)
assert tuple(d.itemsize for d in POD_DTYPES) == (28, 24, 40, 104, 120, 72)


# ---- one joint, N iterations -----------------------------------------------------------------------------------------------------
class Body:
    """Global state of one body at the solve (rigid_body_global_state): built from the entity pose and the local mass properties."""

    def __init__(self, pos, rot, v, w, inv_mass, cog, inv_inertia):
        self.epos, self.rot = np.asarray(pos, np.float64), np.asarray(rot, np.float64)
        self.v, self.w = np.array(v, np.float64), np.array(w, np.float64)
        self.invMass, self.cog = float(inv_mass), np.asarray(cog, np.float64)
        R = qmat(self.rot)
        self.invI = R @ np.asarray(inv_inertia, np.float64).reshape(3, 3) @ R.T
        self.pos = self.epos + qrot(self.rot, self.cog)

    def integrate(self, dt):
        """integrateVelocity (rigid_body.cpp:126-142): the entity pose after the step."""
        d = qmul(np.concatenate([0.5 * self.w, [0.0]]), self.rot)
        rot = qnorm(self.rot + d * dt)
        return self.pos + self.v * dt - qrot(rot, self.cog), rot


def _point_block(A, B, rA, rB):
    sA, sB = skew(rA), skew(rB)
    return sA @ A.invI @ sA.T + sB @ B.invI @ sB.T + np.eye(3) * (A.invMass + B.invMass)


def _solve_point(A, B, rA, rB, bias, inv_eff):
    cdot = (B.v + np.cross(B.w, rB)) - (A.v + np.cross(A.w, rA)) + bias
    p = solve3(inv_eff, -cdot)
    A.v -= A.invMass * p; A.w -= A.invI @ np.cross(rA, p)
    B.v += B.invMass * p; B.w += B.invI @ np.cross(rB, p)


def _inv_or_zero(x):
    return 1.0 / x if x != 0.0 else 0.0


def _axial_motor(A, B, axis, eff, target, imp, max_imp):
    lam = -eff * ((axis @ B.w - axis @ A.w) - target)
    new = clamp(imp + lam, -max_imp, max_imp)
    lam = new - imp
    A.w -= (A.invI @ axis) * lam; B.w += (B.invI @ axis) * lam
    return new


def _axial_limit(A, B, axis, eff, sign, bias, imp):
    lam = -eff * (sign * (axis @ B.w - axis @ A.w) + bias)
    new = max(imp + lam, 0.0)
    lam = (new - imp) * sign
    A.w -= (A.invI @ axis) * lam; B.w += (B.invI @ axis) * lam
    return new


def solve(jtype, pod, A, B, dt, iterations, constants=None, force=None):
    """Initialise and solve one joint.  A and B are modified in place (velocities).  Returns dict(preds, decisions, impulses, values)."""
    c = dict(CONSTANTS); c.update(constants or {})
    P = Preds(force)
    inv_dt = 1.0 / dt
    bias_on = P.test("dt", dt > c["dt_threshold"], dt - c["dt_threshold"], c["dt_threshold"])
    rA = qrot(A.rot, pod["localAnchorA"] - A.cog); rB = qrot(B.rot, pod["localAnchorB"] - B.cog)
    gA, gB = A.pos + rA, B.pos + rB
    imp, val = {}, {}
    with np.errstate(all="ignore"):
        if jtype == DISTANCE:
            u = gB - gA
            l = math.sqrt(u @ u)
            u = u / l if P.test("length", l > _f(0.001), l - _f(0.001), _f(0.001)) else np.zeros(3)
            crAu, crBu = np.cross(rA, u), np.cross(rB, u)
            eff = _inv_or_zero(A.invMass + crAu @ A.invI @ crAu + B.invMass + crBu @ B.invI @ crBu)
            bias = (l - pod["globalLength"]) * (c["beta_distance"] * inv_dt) if bias_on else 0.0
            jA, jB = A.invI @ np.cross(rA, crAu), B.invI @ np.cross(rB, crBu)
            val.update(length=l, bias=bias, effectiveMass=eff, biasMax=abs(bias), lengthNonzero=bool(u.any()))
            for _ in range(iterations):
                lam = -eff * (u @ ((B.v + np.cross(B.w, rB)) - (A.v + np.cross(A.w, rA))) + bias)
                p = lam * u
                A.v -= A.invMass * p; A.w -= jA * lam; B.v += B.invMass * p; B.w += jB * lam
        else:
            point = _point_block(A, B, rA, rB)
            point_bias = (gB - gA) * (c["beta_ball"] * inv_dt) if bias_on else np.zeros(3)
            val["biasMax"] = float(np.abs(point_bias).max()) if jtype != SLIDER else 0.0   # (the slider has no point rows)
        if jtype == BALL:
            for _ in range(iterations):
                _solve_point(A, B, rA, rB, point_bias, point)
        if jtype in (FIXED, SLIDER):
            rot_mass = A.invI + B.invI
            err = qmul(qmul(B.rot, pod["initialInvRotationDifference"]), qconj(A.rot))
            rot_bias = err[:3] * (c["beta_slider"] * inv_dt * c["rot_bias_factor"]) if bias_on else np.zeros(3)
            val["rotationBias"] = rot_bias
            val["biasMax"] = max(val["biasMax"], float(np.abs(rot_bias).max()))
        if jtype == FIXED:
            for _ in range(iterations):
                lam = solve3(rot_mass, -((B.w - A.w) + rot_bias))
                A.w -= A.invI @ lam; B.w += B.invI @ lam
                _solve_point(A, B, rA, rB, point_bias, point)
        if jtype == HINGE:
            axA, axB = qrot(A.rot, pod["localHingeAxisA"]), qrot(B.rot, pod["localHingeAxisB"])
            tB, bB = get_tangents(axB)
            bxa, cxa = np.cross(tB, axA), np.cross(bB, axA)
            I2 = A.invI + B.invI
            m = np.array([[bxa @ I2 @ bxa, bxa @ I2 @ cxa], [cxa @ I2 @ bxa, cxa @ I2 @ cxa]])
            rb = np.array([axA @ tB, axA @ bB]) * (c["beta_hinge_rot"] * inv_dt) if bias_on else np.zeros(2)
            if c["swap_tangents"]:
                rb = rb[::-1]
            val["biasMax"] = max(val["biasMax"], float(np.abs(rb).max()))
            lo, hi, torque = pod["minRotationLimit"], pod["maxRotationLimit"], pod["maxMotorTorque"]
            solve_limit = solve_motor = False
            if lo <= 0.0 or hi >= 0.0 or torque > 0.0:
                cmp_ = qrot(qconj(A.rot), qrot(B.rot, pod["localHingeTangentB"]))
                angle = math.atan2(cmp_ @ pod["localHingeBitangentA"], cmp_ @ pod["localHingeTangentA"])
                val["angle"] = angle
                P.append(("angle_branch_cut", abs(angle) < math.pi, math.pi - abs(angle), math.pi))
                min_v = lo <= 0.0 and P.test("hinge_min", angle <= lo, angle - lo, math.pi)
                max_v = hi >= 0.0 and P.test("hinge_max", angle >= hi, angle - hi, math.pi)
                solve_limit, solve_motor = min_v or max_v, torque > 0.0
                if solve_limit or solve_motor:
                    eff = _inv_or_zero(axA @ A.invI @ axA + axA @ B.invI @ axA)
                    sign = (1.0 if min_v else -1.0) * c["limit_sign"]
                    max_imp = torque * dt
                    mv = pod["motorVelocity"]
                    if pod["motorType"] == POSITION_MOTOR:
                        lo2 = lo if lo <= 0.0 else -_f(math.pi) * c["pm_clamp"]
                        hi2 = hi if hi >= 0.0 else _f(math.pi) * c["pm_clamp"]
                        if lo <= 0.0: lo2 *= c["pm_clamp"]
                        if hi >= 0.0: hi2 *= c["pm_clamp"]
                        mv = (clamp(pod["motorVelocity"], lo2, hi2) - angle) * inv_dt if bias_on else 0.0
                    lb = ((angle - lo) if min_v else (hi - angle)) * c["beta_hinge_limit"] * inv_dt if bias_on else 0.0
                    val.update(limitSign=sign, motorVelocity=mv, limitBias=lb, maxMotorImpulse=max_imp, eff=dict(limit=eff, motor=eff))
            imp.update(motor=0.0, limit=0.0)
            for _ in range(iterations):
                if solve_motor:
                    imp["motor"] = _axial_motor(A, B, axA, eff, mv, imp["motor"], max_imp)
                if solve_limit:
                    imp["limit"] = _axial_limit(A, B, axA, eff, sign, lb, imp["limit"])
                dw = B.w - A.w
                lam = solve2(m, -(np.array([bxa @ dw, cxa @ dw]) + rb))
                p = bxa * lam[0] + cxa * lam[1]
                A.w -= A.invI @ p; B.w += B.invI @ p
                _solve_point(A, B, rA, rB, point_bias, point)
            val.update(solveLimit=solve_limit, solveMotor=solve_motor)
        if jtype == CONE_TWIST:
            btoa = qmul(qconj(A.rot), B.rot)
            axis_a = pod["localLimitAxisA"]
            axis_cmp = qrot(btoa, pod["localLimitAxisB"])
            swing_q, branch = rotate_from_to(axis_a, axis_cmp, P)
            tt, tb = qrot(swing_q, pod["localLimitTangentA"]), qrot(swing_q, pod["localLimitBitangentA"])
            tcmp = qrot(btoa, pod["localLimitTangentB"])
            twist = math.atan2(tcmp @ tb, tcmp @ tt)
            if pod["twistLimit"] >= 0.0 or pod["maxTwistMotorTorque"] > 0.0:   # (nothing reads the twist angle otherwise)
                P.append(("angle_branch_cut", abs(twist) < math.pi, math.pi - abs(twist), math.pi))
            sq = swing_q[:3] @ swing_q[:3]
            if P.test("swing_sq", sq > 0.0, sq, 1.0):
                assert swing_q[3] <= 1.0                      # (acos(q.w) as the reference, unclamped: sq > 0 keeps a normalised float64 w below 1)
                swing, swing_axis = 2.0 * math.acos(swing_q[3]), swing_q[:3] / math.sqrt(sq)
            else:
                swing, swing_axis = 0.0, v3(1, 0, 0)
            val.update(twistAngle=twist, swingAngle=swing, rotateFromTo=branch, swingRotation=swing_q)
            sl, tl = pod["swingLimit"], pod["twistLimit"]
            swing_limit = sl >= 0.0 and P.test("swing_limit", swing >= sl, swing - sl, math.pi)
            if swing_limit:
                g_sw = qrot(A.rot, swing_axis)
                eff_sw = _inv_or_zero(g_sw @ A.invI @ g_sw + g_sw @ B.invI @ g_sw)
                sw_bias = (sl - swing) * (c["beta_hinge_limit"] * inv_dt) if bias_on else 0.0
                val["swingLimitBias"] = sw_bias
                val.setdefault("eff", {})["swing"] = eff_sw
            swing_motor = pod["maxSwingMotorTorque"] > 0.0
            if swing_motor:
                max_sw = pod["maxSwingMotorTorque"] * dt
                local_axis = math.cos(pod["swingMotorAxis"]) * pod["localLimitTangentA"] + math.sin(pod["swingMotorAxis"]) * pod["localLimitBitangentA"]
                if pod["swingMotorType"] == VELOCITY_MOTOR:
                    g_sm, sm_vel = qrot(A.rot, local_axis), pod["swingMotorVelocity"]
                else:
                    target = pod["swingMotorVelocity"]
                    if sl >= 0.0:
                        target = clamp(target, -sl * c["pm_clamp"], sl * c["pm_clamp"])
                    tdir = qrot(qaxis(local_axis, target), axis_a)
                    cr = np.cross(axis_cmp, tdir)
                    s2 = cr @ cr
                    cr = np.zeros(3) if P.test("swing_pm_noz", s2 < _f(1e-8), s2 - _f(1e-8), _f(1e-8)) else cr / math.sqrt(s2)
                    g_sm = qrot(A.rot, cr)
                    delta = math.acos(clamp(tdir @ axis_cmp, 0.0, 1.0))
                    sm_vel = delta * inv_dt * c["swing_pm_factor"] if bias_on else 0.0
                eff_sm = _inv_or_zero(g_sm @ A.invI @ g_sm + g_sm @ B.invI @ g_sm)
                val.update(swingMotorVelocity=sm_vel, maxSwingMotorImpulse=max_sw, swingMotorAxis=g_sm)
                val.setdefault("eff", {})["swingMotor"] = eff_sm
            min_t = tl >= 0.0 and P.test("twist_min", twist <= -tl, twist + tl, math.pi)
            max_t = tl >= 0.0 and P.test("twist_max", twist >= tl, twist - tl, math.pi)
            twist_limit, twist_motor = min_t or max_t, pod["maxTwistMotorTorque"] > 0.0
            if twist_limit or twist_motor:
                g_tw = qrot(A.rot, axis_a)
                eff_tw = _inv_or_zero(g_tw @ A.invI @ g_tw + g_tw @ B.invI @ g_tw)
                t_sign = (1.0 if min_t else -1.0) * c["limit_sign"]
                max_tw = pod["maxTwistMotorTorque"] * dt
                tm_vel = pod["twistMotorVelocity"]
                if pod["twistMotorType"] == POSITION_MOTOR:
                    lim = (tl if tl >= 0.0 else _f(math.pi)) * c["pm_clamp"]
                    tm_vel = (clamp(pod["twistMotorVelocity"], -lim, lim) - twist) * inv_dt if bias_on else 0.0
                t_bias = ((tl + twist) if min_t else (tl - twist)) * c["beta_twist_limit"] * inv_dt if bias_on else 0.0
                val.update(twistSign=t_sign, twistMotorVelocity=tm_vel, twistLimitBias=t_bias, maxTwistMotorImpulse=max_tw)
                val.setdefault("eff", {}).update(twist=eff_tw, twistMotor=eff_tw)
            val.update(solveSwingLimit=swing_limit, solveTwistLimit=twist_limit, solveSwingMotor=swing_motor, solveTwistMotor=twist_motor)
            imp.update(twistMotor=0.0, swingMotor=0.0, twist=0.0, swing=0.0)
            for _ in range(iterations):
                if twist_motor:
                    imp["twistMotor"] = _axial_motor(A, B, g_tw, eff_tw, tm_vel, imp["twistMotor"], max_tw)
                if swing_motor:
                    imp["swingMotor"] = _axial_motor(A, B, g_sm, eff_sm, sm_vel, imp["swingMotor"], max_sw)
                if twist_limit:
                    imp["twist"] = _axial_limit(A, B, g_tw, eff_tw, t_sign, t_bias, imp["twist"])
                if swing_limit:
                    lam = -eff_sw * (g_sw @ A.w - g_sw @ B.w + sw_bias)
                    new = max(imp["swing"] + lam, 0.0)
                    lam, imp["swing"] = new - imp["swing"], new
                    A.w += (A.invI @ g_sw) * lam; B.w -= (B.invI @ g_sw) * lam
                _solve_point(A, B, rA, rB, point_bias, point)
        if jtype == SLIDER:
            axis = qrot(A.rot, pod["localAxisA"])
            t, b = get_tangents(axis)
            u = gB - gA
            rAu = rA + u
            rBxt, rBxb, rAuxt, rAuxb = np.cross(rB, t), np.cross(rB, b), np.cross(rAu, t), np.cross(rAu, b)
            ms = A.invMass + B.invMass
            m = np.array([[rAuxt @ A.invI @ rAuxt + rBxt @ B.invI @ rBxt + ms, rAuxt @ A.invI @ rAuxb + rBxt @ B.invI @ rBxb],
                          [rAuxb @ A.invI @ rAuxt + rBxb @ B.invI @ rBxt, rAuxb @ A.invI @ rAuxb + rBxb @ B.invI @ rBxb + ms]])
            tbias = np.array([u @ t, u @ b]) * (c["beta_slider"] * inv_dt) if bias_on else np.zeros(2)
            if c["swap_tangents"]:
                tbias = tbias[::-1]
            val["biasMax"] = max(val["biasMax"], float(np.abs(tbias).max()))
            dist = u @ axis
            val["distance"] = dist
            lo, hi = pod["negDistanceLimit"], pod["posDistanceLimit"]
            min_v = lo <= 0.0 and P.test("slider_min", dist < lo, dist - lo, max(1.0, abs(lo)))
            max_v = hi >= 0.0 and P.test("slider_max", dist > hi, dist - hi, max(1.0, abs(hi)))
            solve_limit = min_v or max_v
            if solve_limit:
                rAuxs, rBxs = np.cross(rAu, axis), np.cross(rB, axis)
                eff = _inv_or_zero(ms + rAuxs @ A.invI @ rAuxs + rBxs @ B.invI @ rBxs)
                sign = (1.0 if min_v else -1.0) * c["limit_sign"]
                lb = ((dist - lo) if min_v else (hi - dist)) * (c["beta_slider_limit"] * inv_dt) if bias_on else 0.0
                val.update(limitSign=sign, limitBias=lb)
                val.setdefault("eff", {})["limit"] = eff
            solve_motor = pod["maxMotorForce"] > 0.0
            if solve_motor:
                max_imp = pod["maxMotorForce"] * dt
                mv = pod["motorVelocity"]
                if pod["motorType"] == POSITION_MOTOR:
                    lo2 = lo * c["pm_clamp"] if lo <= 0.0 else -math.inf
                    hi2 = hi * c["pm_clamp"] if hi >= 0.0 else math.inf
                    mv = (clamp(pod["motorVelocity"], lo2, hi2) - dist) * inv_dt if bias_on else 0.0
                val.update(motorVelocity=mv, maxMotorImpulse=max_imp)
                val.setdefault("eff", {})["motor"] = float(np.float64(1.0) / np.float64(ms))
            val.update(solveLimit=solve_limit, solveMotor=solve_motor)
            imp.update(motor=0.0, limit=0.0)
            for _ in range(iterations):
                if solve_motor:
                    cdot = B.v @ axis - A.v @ axis - mv
                    mass = np.float64(1.0) / np.float64(ms)       # 1 / (0 + 0) = inf between two kinematic bodies, as the reference
                    lam = -mass * cdot
                    new = clamp(imp["motor"] + lam, -max_imp, max_imp)
                    lam, imp["motor"] = new - imp["motor"], float(new)
                    p = lam * axis
                    A.v -= A.invMass * p; B.v += B.invMass * p
                if solve_limit:
                    cdot = B.v @ axis + B.w @ rBxs - A.v @ axis - A.w @ rAuxs
                    lam = -eff * (sign * cdot + lb)
                    new = max(imp["limit"] + lam, 0.0)
                    lam, imp["limit"] = (new - imp["limit"]) * sign, new
                    p = lam * axis
                    A.v -= A.invMass * p; A.w -= (A.invI @ rAuxs) * lam
                    B.v += B.invMass * p; B.w += (B.invI @ rBxs) * lam
                lam = solve3(rot_mass, -((B.w - A.w) + rot_bias))
                A.w -= A.invI @ lam; B.w += B.invI @ lam
                cd = np.array([t @ B.v + rBxt @ B.w - t @ A.v - rAuxt @ A.w, b @ B.v + rBxb @ B.w - b @ A.v - rAuxb @ A.w])
                lam = solve2(m, -(cd + tbias))
                tb_ = t * lam[0] + b * lam[1]
                A.v -= A.invMass * tb_; A.w -= A.invI @ (rAuxt * lam[0] + rAuxb * lam[1])
                B.v += B.invMass * tb_; B.w += B.invI @ (rBxt * lam[0] + rBxb * lam[1])
    return dict(preds=list(P), decisions={n: d for n, d, _, _ in P}, impulses=imp, values=val)


# ---- the battery ---------------------------------------------------------------------------------------------------------------
# Ties by construction: predicates that sit ON their threshold, with the argument why the float32 quantity is exact (so the oracle and
# the device decide as float64 does).  case name -> {predicate: argument}.
_IDENTITY_ANGLE = "identity relative rotation: the compared tangent is the stored one, its bitangent component is an exact 0, atan2f(0, 1) == 0"
_IDENTITY_SWING = "identity relative rotation: from == to, so the normalised dot is x*x + y*y + z*z of one axis-aligned unit vector == 1, rotateFromTo returns the identity quaternion and sq == 0"
_INDIFFERENT = "a swing this small leaves d within float32 rounding of 1 and w of acosf's argument within an ulp of 1; no row reads the swing (limit 0.5 far away, no swing motor) and the twist frame is continuous there: classify() forces the predicate both ways and finds the same velocities"
TIES = {}

_GENERIC_Q = (0.18257418, 0.36514837, -0.54772256, 0.73029674)   # (1, 2, -3, 4) / sqrt(30)
_IDENT = (0.0, 0.0, 0.0, 1.0)
_SMALL = (SPHERE, (0.0, 0.0, 0.0, 0.1), 1000.0)
_OFFSET = (SPHERE, (0.05, -0.03, 0.04, 0.08), 1000.0)           # offset collider: centre of gravity off the body origin
_HEAVY = (SPHERE, (0.0, 0.0, 0.0, 0.1), 1.0e7)                  # 1 : 1e4 against _SMALL
_NEEDLE = (CAPSULE, (0.0, -0.27, 0.0, 0.0, 0.27, 0.0, 0.01), 1000.0)  # thin capsule: transverse / axial inertia about 500 : 1


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _rot_about(pose, anchor, axis, angle):
    """The pose turned by `angle` about the line through `anchor` along `axis` (float64, rounded to float32 by the caller)."""
    p, q = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    r = qaxis(normalize(np.asarray(axis, np.float64)), angle)
    a = np.asarray(anchor, np.float64)
    return a + qrot(r, p - a), qnorm(qmul(r, q))


def battery():
    """The list of cases.  A case: dict(name, type, group, tags, A, B (dicts: pos, rot, kinematic, collider, v, w, relative to the
    case's base position), args (global construction arguments, relative to the base), edits (POD fields overwritten after
    construction), move (poses at the step, if they differ from the construction's), dt, iterations, far)."""
    cases = []
    rng = np.random.RandomState(12345)

    def add(name, jtype, tags=(), group="plain", A=None, B=None, args=None, edits=None, moveA=None, moveB=None, dt=1.0 / 120.0, iterations=6, far=False,
            kinA=False, kinB=False, colA=_SMALL, colB=_SMALL, rotA=_IDENT, rotB=_IDENT, posB=(0.6, 0.0, 0.0), vel=1.0):
        vs = (rng.uniform(-1.0, 1.0, 12) * vel).astype(np.float32).astype(np.float64)
        a = dict(pos=(0.0, 0.0, 0.0), rot=rotA, kinematic=kinA, collider=colA, v=vs[0:3], w=vs[3:6])
        b = dict(pos=posB, rot=rotB, kinematic=kinB, collider=colB, v=vs[6:9], w=vs[9:12])
        assert name not in {c["name"] for c in cases}, name
        cases.append(dict(name=name, type=jtype, group=group, tags=set(tags), A=a, B=b, args=dict(args), edits=dict(edits or {}), moveA=moveA, moveB=moveB,
                          dt=float(np.float32(dt)), iterations=iterations, far=far))

    anchor = (0.3, 0.05, -0.02)
    y, x = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    gen_axis = tuple(normalize(v3(0.3, 0.8, -0.52)))
    poseB = ((0.6, 0.0, 0.0), _IDENT)

    def base_args(t, **kw):
        if t == DISTANCE:
            return dict(anchor_a=(0.1, 0.02, 0.0), anchor_b=(0.5, -0.03, 0.04))
        d = dict(anchor=anchor)
        if t == HINGE:
            d.update(axis=gen_axis, min=-0.5, max=0.7)
        if t == CONE_TWIST:
            d.update(axis=gen_axis, swing=0.6, twist=0.4)
        if t == SLIDER:
            d.update(axis=gen_axis, min=-0.2, max=0.3)
        d.update(kw)
        return d

    def perturbB(t, k=1.0):
        """B displaced a little from its construction pose so that every bias row has an error to work on."""
        p, q = _rot_about(poseB, anchor, (0.2, -0.5, 0.84), 0.07 * k)
        return p + v3(0.004, -0.003, 0.005) * k, q

    # -- every type: body kinds, mass properties, levers, coordinates, time steps
    for t in range(6):
        n = TYPE_NAMES[t]
        cons = {"beta", "rot2"} if t in (FIXED, SLIDER) else {"beta"}
        add(n + "/plain", t, cons | {"tangents"}, args=base_args(t), moveB=perturbB(t))
        add(n + "/generic_orientation", t, cons | {"tangents"}, args=base_args(t), rotA=_GENERIC_Q, rotB=(0.5, -0.5, 0.5, 0.5), moveB=perturbB(t))
        add(n + "/dyn_kin", t, args=base_args(t), kinB=True, moveB=perturbB(t))
        add(n + "/kin_dyn", t, args=base_args(t), kinA=True, moveB=perturbB(t))
        add(n + "/kin_kin", t, args=base_args(t), kinA=True, kinB=True, moveB=perturbB(t))
        add(n + "/cog_offset", t, args=base_args(t), colA=_OFFSET, colB=_OFFSET, rotA=_GENERIC_Q, moveB=perturbB(t))
        add(n + "/mass_1e4", t, group="hard", args=base_args(t), colB=_HEAVY, moveB=perturbB(t))
        add(n + "/needle", t, group="hard", args=base_args(t), colA=_NEEDLE, colB=_NEEDLE, rotA=_GENERIC_Q, rotB=(0.5, -0.5, 0.5, 0.5), posB=(0.9, 0.0, 0.0), moveB=perturbB(t))
        if t == DISTANCE:
            add(n + "/lever_1cm", t, args=dict(anchor_a=(0.01, 0.0, 0.0), anchor_b=(0.59, 0.0, 0.0)), moveB=perturbB(t))
            add(n + "/lever_10m", t, group="hard", args=dict(anchor_a=(4.0, 3.0, 0.0), anchor_b=(10.0, 1.0, 0.0)), posB=(20.0, 0.0, 0.0), vel=0.1)
        else:
            add(n + "/lever_1cm", t, args=base_args(t, anchor=(0.006, 0.008, 0.0)), moveB=perturbB(t))
            add(n + "/lever_10m", t, group="hard", args=base_args(t, anchor=(10.0, 0.0, 0.0)), posB=(20.0, 0.0, 0.0), vel=0.1,
                moveB=_rot_about(((20.0, 0.0, 0.0), _IDENT), (10.0, 0.0, 0.0), (0.2, -0.5, 0.84), 0.05))
        add(n + "/far", t, group="far", args=base_args(t), far=True, rotA=_GENERIC_Q, moveB=perturbB(t), vel=10.0)
        add(n + "/dt60", t, cons, args=base_args(t), moveB=perturbB(t), dt=1.0 / 60.0)
        add(n + "/dt_below_threshold", t, {"dt_threshold"}, args=base_args(t), moveB=perturbB(t), dt=5e-6)

    # -- distance
    da = dict(anchor_a=(0.1, 0.0, 0.0), anchor_b=(0.5, 0.0, 0.0))
    add("distance/rest", DISTANCE, args=da)
    add("distance/stretched", DISTANCE, {"beta"}, args=da, moveB=((0.7, 0.02, 0.0), _IDENT))
    add("distance/compressed", DISTANCE, {"beta"}, args=da, moveB=((0.45, 0.0, 0.03), _IDENT))
    add("distance/anchors_half_mm", DISTANCE, {"length"}, args=dict(anchor_a=(0.3, 0.0, 0.0), anchor_b=(0.3005, 0.0, 0.0)))

    # -- fixed / slider: initial rotation difference
    for t in (FIXED, SLIDER):
        add(TYPE_NAMES[t] + "/rotated_initial_frame", t, {"beta", "rot2"}, args=base_args(t), rotA=_GENERIC_Q, rotB=(0.5, -0.5, 0.5, 0.5), moveB=_rot_about(((0.6, 0.0, 0.0), (0.5, -0.5, 0.5, 0.5)), anchor, (0.6, 0.0, 0.8), 0.2))

    # -- hinge
    H = HINGE
    hinge = lambda ang, ax=y: _rot_about(poseB, anchor, ax, ang)
    ha = lambda **kw: dict(dict(anchor=anchor, axis=y), **kw)
    trig = dict(group="trig")
    add("hinge/limits_off", H, args=ha(min=1.0, max=-1.0), moveB=hinge(0.3))
    add("hinge/min_only_inside", H, args=ha(min=-0.5, max=-1.0), moveB=hinge(0.3), **trig)
    add("hinge/min_only_violated", H, {"limit_sign", "beta_hinge_limit"}, args=ha(min=-0.5, max=-1.0), moveB=hinge(-0.6), **trig)
    add("hinge/max_only_inside", H, args=ha(min=1.0, max=0.5), moveB=hinge(-0.3), **trig)
    add("hinge/max_only_violated", H, {"limit_sign", "beta_hinge_limit"}, args=ha(min=1.0, max=0.5), moveB=hinge(0.6), **trig)
    add("hinge/both_inside", H, args=ha(min=-0.5, max=0.5), moveB=hinge(0.2), **trig)
    for d in (1e-3, 0.1, 1.0):
        add("hinge/min_violated_%g" % d, H, {"limit_sign", "beta_hinge_limit"}, args=ha(min=-0.5, max=0.5), moveB=hinge(-0.5 - d), **trig)
        add("hinge/max_violated_%g" % d, H, {"limit_sign", "beta_hinge_limit"}, args=ha(min=-0.5, max=0.5), moveB=hinge(0.5 + d), **trig)
    add("hinge/min_zero_identity", H, {"tie"}, args=ha(min=0.0, max=-1.0), **trig)
    add("hinge/max_zero_identity", H, {"tie"}, args=ha(min=1.0, max=0.0), **trig)
    TIES["hinge/min_zero_identity"] = {"hinge_min": _IDENTITY_ANGLE}
    TIES["hinge/max_zero_identity"] = {"hinge_max": _IDENTITY_ANGLE}
    # (about the line through both bodies: half a turn about any other axis through the anchor would put B on top of A)
    add("hinge/angle_plus_pi", H, args=ha(axis=x, min=-3.0, max=3.0), moveB=hinge(math.pi - 1e-3, x), **trig)
    add("hinge/angle_minus_pi", H, args=ha(axis=x, min=-3.0, max=3.0), moveB=hinge(-(math.pi - 1e-3), x), **trig)
    vm = dict(motorType=VELOCITY_MOTOR, motorVelocity=2.0)
    add("hinge/velocity_motor", H, {"unsaturated"}, args=ha(), edits=dict(vm, maxMotorTorque=1.0e6), moveB=hinge(0.1), **trig)
    add("hinge/velocity_motor_saturated", H, {"saturated"}, args=ha(), edits=dict(vm, maxMotorTorque=1.0e-3), moveB=hinge(0.1), **trig)
    pm = lambda target, torque=1.0e6: dict(motorType=POSITION_MOTOR, motorVelocity=target, maxMotorTorque=torque)
    add("hinge/position_motor_inside", H, {"unsaturated"}, args=ha(min=-0.5, max=0.5), edits=pm(0.3), moveB=hinge(0.1), **trig)
    add("hinge/position_motor_outside", H, {"unsaturated", "pm_clamp"}, args=ha(min=-0.5, max=0.5), edits=pm(0.9), moveB=hinge(0.1), **trig)
    add("hinge/position_motor_outside_min", H, {"unsaturated", "pm_clamp"}, args=ha(min=-0.5, max=0.5), edits=pm(-0.9), moveB=hinge(0.1), **trig)
    add("hinge/position_motor_no_limits_beyond_pi", H, {"unsaturated", "pm_clamp"}, args=ha(), edits=pm(4.0), moveB=hinge(0.1), **trig)
    add("hinge/position_motor_no_limits_beyond_minus_pi", H, {"unsaturated", "pm_clamp"}, args=ha(), edits=pm(-4.0), moveB=hinge(0.1), **trig)
    add("hinge/position_motor_saturated", H, {"saturated"}, args=ha(min=-0.5, max=0.5), edits=pm(0.3, 1.0e-3), moveB=hinge(0.1), **trig)
    add("hinge/motor_and_violated_limit", H, {"unsaturated", "limit_sign", "beta_hinge_limit"}, args=ha(min=-0.5, max=0.5), edits=dict(vm, maxMotorTorque=1.0e6), moveB=hinge(0.6), **trig)
    add("hinge/rotation_error", H, {"beta_hinge_rot", "tangents"}, args=ha(min=1.0, max=-1.0), moveB=_rot_about(poseB, anchor, (1.0, 0.0, 0.3), 0.1))

    # -- cone-twist
    CT = CONE_TWIST
    ca = lambda swing, twist: dict(anchor=anchor, axis=y, swing=swing, twist=twist)
    swingB = lambda ang, ax=(0.6, 0.0, 0.8): _rot_about(poseB, anchor, ax, ang)
    both = lambda sw, tw: _rot_about(_rot_about(poseB, anchor, y, tw), anchor, (0.6, 0.0, 0.8), sw)
    for nm, lim in (("zero", 0.0), ("positive", 0.5), ("disabled", -1.0)):
        add("cone_twist/swing_zero_limit_" + nm, CT, {"tie"}, args=ca(lim, 0.4), **trig)
        TIES["cone_twist/swing_zero_limit_" + nm] = {"rft_identity": _IDENTITY_SWING, "swing_sq": _IDENTITY_SWING}
    TIES["cone_twist/swing_zero_limit_zero"]["swing_limit"] = _IDENTITY_SWING + "; the swing angle is an exact 0 == swingLimit"
    add("cone_twist/swing_limit_violated", CT, {"beta_hinge_limit"}, args=ca(0.5, 0.4), moveB=swingB(0.8), **trig)
    add("cone_twist/swing_inside", CT, args=ca(0.5, 0.4), moveB=swingB(0.3), **trig)
    add("cone_twist/twist_min_violated", CT, {"limit_sign", "beta_twist_limit"}, args=ca(0.5, 0.4), moveB=both(0.2, -0.6), **trig)
    add("cone_twist/twist_max_violated", CT, {"limit_sign", "beta_twist_limit"}, args=ca(0.5, 0.4), moveB=both(0.2, 0.6), **trig)
    svm = lambda ang, torque=1.0e6: dict(swingMotorType=VELOCITY_MOTOR, swingMotorVelocity=1.5, maxSwingMotorTorque=torque, swingMotorAxis=ang)
    add("cone_twist/swing_velocity_motor_axis_0", CT, {"unsaturated"}, args=ca(-1.0, -1.0), edits=svm(0.0), moveB=swingB(0.3), **trig)
    add("cone_twist/swing_velocity_motor_axis_half_pi", CT, {"unsaturated"}, args=ca(-1.0, -1.0), edits=svm(math.pi / 2), moveB=swingB(0.3), **trig)
    add("cone_twist/swing_velocity_motor_axis_generic", CT, {"unsaturated"}, args=ca(-1.0, -1.0), edits=svm(2.2), moveB=swingB(0.3), **trig)
    add("cone_twist/swing_velocity_motor_saturated", CT, {"saturated"}, args=ca(-1.0, -1.0), edits=svm(2.2, 1.0e-3), moveB=swingB(0.3), **trig)
    spm = lambda target, ang=0.7, torque=1.0e6: dict(swingMotorType=POSITION_MOTOR, swingMotorVelocity=target, maxSwingMotorTorque=torque, swingMotorAxis=ang)
    add("cone_twist/swing_position_motor_inside", CT, {"unsaturated", "swing_pm_factor"}, args=ca(0.8, -1.0), edits=spm(0.5), moveB=swingB(0.2), **trig)
    add("cone_twist/swing_position_motor_beyond_limit", CT, {"unsaturated", "swing_pm_factor", "pm_clamp"}, args=ca(0.4, -1.0), edits=spm(1.2), moveB=swingB(0.1), **trig)
    add("cone_twist/swing_position_motor_no_limit", CT, {"unsaturated", "swing_pm_factor"}, args=ca(-1.0, -1.0), edits=spm(1.2), moveB=swingB(0.1), **trig)
    add("cone_twist/swing_position_motor_reached", CT, {"tie"}, args=ca(0.8, -1.0), edits=spm(0.0), **trig)
    TIES["cone_twist/swing_position_motor_reached"] = {"rft_identity": _IDENTITY_SWING, "swing_sq": _IDENTITY_SWING}
    tpm = lambda target, torque=1.0e6: dict(twistMotorType=POSITION_MOTOR, twistMotorVelocity=target, maxTwistMotorTorque=torque)
    add("cone_twist/twist_position_motor_with_limit", CT, {"unsaturated", "pm_clamp"}, args=ca(0.8, 0.4), edits=tpm(0.9), moveB=both(0.2, 0.1), **trig)
    add("cone_twist/twist_position_motor_no_limit", CT, {"unsaturated", "pm_clamp"}, args=ca(0.8, -1.0), edits=tpm(4.0), moveB=both(0.2, 0.1), **trig)
    add("cone_twist/twist_velocity_motor_saturated", CT, {"saturated"}, args=ca(0.8, -1.0), edits=dict(twistMotorType=VELOCITY_MOTOR, twistMotorVelocity=3.0, maxTwistMotorTorque=1.0e-3), moveB=both(0.2, 0.1), **trig)
    add("cone_twist/all_rows", CT, {"unsaturated", "limit_sign", "beta_twist_limit", "beta_hinge_limit", "swing_pm_factor"}, args=ca(0.3, 0.2),
        edits=dict(spm(0.2), **tpm(0.1)), moveB=both(0.5, 0.35), rotA=_GENERIC_Q, rotB=_GENERIC_Q, **trig)
    for nm, ang in (("1e-4", 1e-4), ("1e-3", 1e-3)):
        add("cone_twist/swing_" + nm, CT, {"tie", "indifferent"}, args=ca(0.5, 0.1), moveB=both(ang, 0.3), **trig)
        TIES["cone_twist/swing_" + nm] = {k: _INDIFFERENT for k in ("rft_identity", "swing_sq")}
    add("cone_twist/swing_near_pi", CT, {"tie"}, args=ca(-1.0, 0.1), moveB=swingB(math.pi - 1e-3), **trig)
    TIES["cone_twist/swing_near_pi"] = {"rft_antiparallel": "d = -1 + 5.0e-7 against the threshold -1 + 1e-6: the float32 dot of two normalised vectors is within 3 ulps (1.8e-7) of it, so float32 decides as float64 does"}
    add("cone_twist/swing_exactly_pi", CT, {"tie", "beta_hinge_limit"}, args=ca(3.0, -1.0), moveB=((0.6, 0.1, 0.04), (1.0, 0.0, 0.0, 0.0)), **trig)
    TIES["cone_twist/swing_exactly_pi"] = {"rft_antiparallel": "half a turn about x as the exact quaternion (1, 0, 0, 0) maps the limit axis y to exactly -y: d == -1 in float32, 17 ulps below the threshold -1 + 1e-6"}

    # -- slider
    S = SLIDER
    sa = lambda **kw: dict(dict(anchor=anchor, axis=x), **kw)
    slide = lambda d: ((0.6 + d, 0.0, 0.0), _IDENT)
    add("slider/limits_off", S, args=sa(min=1.0, max=-1.0), moveB=slide(0.1))
    add("slider/neg_only_violated", S, {"limit_sign", "beta_slider_limit"}, args=sa(min=-0.05, max=-1.0), moveB=slide(-0.1))
    add("slider/neg_only_inside", S, args=sa(min=-0.05, max=-1.0), moveB=slide(0.2))
    add("slider/pos_only_violated", S, {"limit_sign", "beta_slider_limit"}, args=sa(min=1.0, max=0.05), moveB=slide(0.1))
    add("slider/pos_only_inside", S, args=sa(min=1.0, max=0.05), moveB=slide(-0.2))
    add("slider/both_min_violated", S, {"limit_sign", "beta_slider_limit"}, args=sa(min=-0.05, max=0.05), moveB=slide(-0.08))
    add("slider/both_max_violated", S, {"limit_sign", "beta_slider_limit"}, args=sa(min=-0.05, max=0.05), moveB=slide(0.08))
    svel = lambda force: dict(motorType=VELOCITY_MOTOR, motorVelocity=0.8, maxMotorForce=force)
    add("slider/velocity_motor", S, {"unsaturated"}, args=sa(), edits=svel(1.0e6), moveB=slide(0.02))
    add("slider/velocity_motor_saturated", S, {"saturated"}, args=sa(), edits=svel(1.0e-2), moveB=slide(0.02))
    spos = lambda target, force=1.0e6: dict(motorType=POSITION_MOTOR, motorVelocity=target, maxMotorForce=force)
    add("slider/position_motor_with_limits", S, {"unsaturated", "pm_clamp"}, args=sa(min=-0.05, max=0.05), edits=spos(0.2), moveB=slide(0.02))
    add("slider/position_motor_no_limits", S, {"unsaturated"}, args=sa(), edits=spos(0.2), moveB=slide(0.02))
    add("slider/motor_kin_kin", S, {"saturated"}, args=sa(), edits=svel(1.0e-2), kinA=True, kinB=True, moveB=slide(0.02))
    add("slider/translation_error", S, {"beta", "tangents"}, args=sa(), moveB=((0.6, 0.02, -0.03), _IDENT))
    return cases


def far_base(k):
    return v3(2000.0 - 50.0 * k, -2000.0, 2000.0)


_CELLS = sorted(((i, j, l) for i in range(-3, 4) for j in range(-3, 4) for l in range(-3, 4)), key=lambda c: (c[0] * c[0] + c[1] * c[1] + c[2] * c[2], c))


def near_base(k):
    """Pairs 50 m apart on a grid around the origin, nearest cells first: the float32 cancellation in (B.pos + rB) - (A.pos + rA)
    grows with the coordinate, and only the cases tagged for it are meant to see it."""
    return 50.0 * v3(*_CELLS[k])


def groups(cases):
    """Cases by world: one world per (dt, iterations); returns {key: [case, ...]} in battery order."""
    out = {}
    for c in cases:
        out.setdefault((c["dt"], c["iterations"]), []).append(c)
    return out


def place(cases_of_world):
    """Absolute float32 poses, velocities and construction arguments of one world's cases: a list of dicts parallel to the cases."""
    out, near, far = [], 0, 0
    for c in cases_of_world:
        if c["far"]:
            base, far = far_base(far), far + 1
        else:
            base, near = near_base(near), near + 1
        pl = dict(base=base)
        for s in ("A", "B"):
            b = c[s]
            pl[s] = dict(pos0=_f32(base + np.asarray(b["pos"], np.float64)), rot0=_f32(b["rot"]), v=_f32(b["v"]), w=_f32(b["w"]))
            mv = c["move" + s]
            pl[s]["pos"], pl[s]["rot"] = (_f32(base + np.asarray(mv[0], np.float64)), _f32(mv[1])) if mv is not None else (pl[s]["pos0"], pl[s]["rot0"])
        pl["args"] = {k: (_f32(base + np.asarray(v, np.float64)) if k.startswith("anchor") else (_f32(v) if k == "axis" else float(np.float32(v)))) for k, v in c["args"].items()}
        pl["edits"] = {k: (int(v) if k.endswith("Type") else float(np.float32(v))) for k, v in c["edits"].items()}
        out.append(pl)
    return out


def reference(case, pl, massA, massB, constants=None, force=None):
    """joint64 on one placed case.  massA / massB: (invMass, localCOG[3], localInvInertia[9]) as float32 values from the world."""
    pod = derive(case["type"], (pl["A"]["pos0"], pl["A"]["rot0"]), (pl["B"]["pos0"], pl["B"]["rot0"]), pl["args"])
    pod.update(pl["edits"])
    bodies = [Body(pl[s]["pos"], pl[s]["rot"], pl[s]["v"], pl[s]["w"], *m) for s, m in (("A", massA), ("B", massB))]
    r = solve(case["type"], pod, bodies[0], bodies[1], case["dt"], case["iterations"], constants, force)
    r["pod"] = pod
    r["vel"] = np.stack([np.concatenate([b.v, b.w]) for b in bodies])
    r["pose"] = [b.integrate(case["dt"]) for b in bodies]
    r["scale"] = max(1.0, float(np.abs(np.concatenate([pl[s][k] for s in "AB" for k in "vw"])).max()), float(np.abs(r["vel"][np.isfinite(r["vel"])]).max()))
    return r


def classify(case, pl, massA, massB):
    """'clear' or 'tie'; raises for a case that is neither.
    clear: every predicate margin >= MARGIN x its scale.  tie: the unclear predicates are exactly those listed in TIES for the case, and
    each is on its threshold exactly (margin 0), or in rotateFromTo's 1e-6 wide antiparallel band clear of it by more than 4 float32
    ulps of the dot, or (tag indifferent) decided either way with the same result: forcing it the other way moves no velocity by more
    than the floor tolerance."""
    r = reference(case, pl, massA, massB)
    unclear = [(n, d, m) for n, d, m, s in r["preds"] if m < MARGIN * s]
    if not unclear:
        assert case["name"] not in TIES, case["name"] + ": listed as a tie but clear"
        return "clear"
    assert case["name"] in TIES and "tie" in case["tags"], (case["name"], "unclear predicates", unclear)
    assert {n for n, _, _ in unclear} == set(TIES[case["name"]]), (case["name"], unclear)
    if "indifferent" in case["tags"]:
        for n, d, _ in unclear:
            o = reference(case, pl, massA, massB, force={n: not d})
            assert np.abs(o["vel"] - r["vel"]).max() <= FLOOR_ULPS * 2.0 ** -23 * r["scale"], (case["name"], n, np.abs(o["vel"] - r["vel"]).max())
    else:
        assert all(m == 0.0 or (n == "rft_antiparallel" and m > 4 * 2.0 ** -24) for n, _, m in unclear), (case["name"], unclear)
    return "tie"


# ---- the battery as worlds (the same calls build an oracle world and a device world) ----------------------------------------------
GLOBAL_CONSTRUCTORS = ("add_distance_constraint_global", "add_ball_constraint_global", "add_fixed_constraint_global", "add_hinge_constraint_global",
                       "add_cone_twist_constraint_global", "add_slider_constraint_global")


def build_world(world, cases_of_world, placed, contact_far_away=False):
    """Bodies 2k and 2k+1 are A and B of case k (gravity off, no damping: the force integration is the identity, x * 1 / (1 + dt * 0)).
    Returns the joint ids, parallel to the cases.  contact_far_away adds a box resting on a static slab 2 km from every joint, so that
    the step has a pair (the cluster sweep runs) without touching a jointed body."""
    mat = lambda density: (0.1, 0.5, density)
    ids = []
    for c, pl in zip(cases_of_world, placed):
        pair = []
        for s in ("A", "B"):
            b = world.add_body(tuple(pl[s]["pos0"]), tuple(pl[s]["rot0"]), kinematic=c[s]["kinematic"], gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
            ctype, shape, density = c[s]["collider"]
            world.add_collider(b, ctype, shape, mat(density))
            pair.append(b)
        a = pl["args"]
        t = c["type"]
        if t == DISTANCE:
            cid = world.add_distance_constraint_global(pair[0], pair[1], a["anchor_a"], a["anchor_b"])
        elif t in (BALL, FIXED):
            cid = getattr(world, GLOBAL_CONSTRUCTORS[t])(pair[0], pair[1], a["anchor"])
        elif t == CONE_TWIST:
            cid = world.add_cone_twist_constraint_global(pair[0], pair[1], a["anchor"], a["axis"], a["swing"], a["twist"])
        else:
            cid = getattr(world, GLOBAL_CONSTRUCTORS[t])(pair[0], pair[1], a["anchor"], a["axis"], a.get("min", 1.0), a.get("max", -1.0))
        if pl["edits"]:
            pod = world.constraint_get(t, cid, POD_DTYPES[t].itemsize).view(POD_DTYPES[t]).copy()
            for k, v in pl["edits"].items():
                pod[k] = v
            world.constraint_set(t, cid, pod.view(np.uint8))
        ids.append(cid)
    n = 2 * len(cases_of_world)
    tr = np.zeros((n, 7), np.float32); ve = np.zeros((n, 6), np.float32)
    for k, pl in enumerate(placed):
        for j, s in enumerate("AB"):
            tr[2 * k + j, :3], tr[2 * k + j, 3:] = pl[s]["pos"], pl[s]["rot"]
            ve[2 * k + j, :3], ve[2 * k + j, 3:] = pl[s]["v"], pl[s]["w"]
    if contact_far_away:
        world.add_static_collider(4, (0, 0, 0, 1, 0, 0, 0, 2.0, 0.5, 2.0), mat(1000.0), pos=(-2000.0, -0.5, -2000.0))
        box = world.add_body((-2000.0, 0.499, -2000.0))
        world.add_collider(box, 4, (0, 0, 0, 1, 0, 0, 0, 0.5, 0.5, 0.5), mat(1000.0))
        tr = np.concatenate([tr, np.array([[-2000.0, 0.499, -2000.0, 0, 0, 0, 1]], np.float32)]); ve = np.concatenate([ve, np.zeros((1, 6), np.float32)])
    world.write_state(tr, ve)
    return ids


def mass_of(mass_properties, body):
    """(invMass, localCOG, localInvInertia) of one row of World.mass_properties(): {cog3, invMass, invInertia9 (column-major, symmetric)}."""
    m = np.asarray(mass_properties[body], np.float64)
    return m[3], m[0:3], m[4:13].reshape(3, 3).T


def pod_of(world, case, cid):
    return world.constraint_get(case["type"], cid, POD_DTYPES[case["type"]].itemsize).view(POD_DTYPES[case["type"]])[0]


# ---- decoding the device's joint update records (layouts: the comments of csrc/k_joints.hip) ----------------------------------------
def decode_update(jtype, rec):
    """The decisions, signs, motor targets and accumulated impulses of one record, under the names `solve` uses."""
    bits = lambda i: int(np.asarray(rec[i:i + 1], np.float32).view(np.uint32)[0])
    if jtype == HINGE:
        f = bits(34)
        return dict(solveLimit=bool(f & 1), solveMotor=bool(f & 2), limitSign=float(rec[37]), motorVelocity=float(rec[40]), maxMotorImpulse=float(rec[39]),
                    impulses=dict(limit=float(rec[35]), motor=float(rec[38])))
    if jtype == CONE_TWIST:
        f = bits(18)
        return dict(solveSwingLimit=bool(f & 1), solveTwistLimit=bool(f & 2), solveSwingMotor=bool(f & 4), solveTwistMotor=bool(f & 8), twistSign=float(rec[35]),
                    swingMotorVelocity=float(rec[46]), twistMotorVelocity=float(rec[59]), maxSwingMotorImpulse=float(rec[45]), maxTwistMotorImpulse=float(rec[58]),
                    impulses=dict(swing=float(rec[22]), twist=float(rec[34]), swingMotor=float(rec[44]), twistMotor=float(rec[57])))
    if jtype == SLIDER:
        f = bits(36)
        return dict(solveLimit=bool(f & 1), solveMotor=bool(f & 2), limitSign=float(rec[43]), motorVelocity=float(rec[56]), maxMotorImpulse=float(rec[58]),
                    impulses=dict(limit=float(rec[42]), motor=float(rec[57])))
    return dict(impulses={})


def decode_oracle(jtype, rec):
    """One row of OracleWorld.joint_decisions() under the names of decode_update, with what only the oracle keeps: the angles, the
    swing rotation (from which rotateFromTo's branch and sq > 0 follow), the swing motor axis (zero when noz gave up), whether the
    distance joint normalised u, and whether any bias is non-zero (the time step threshold)."""
    f = int(rec[0])
    d = dict(biasNonzero=bool(rec[14]), impulses={})
    if jtype == DISTANCE:
        d["lengthNonzero"] = bool(rec[13])
    if jtype in (HINGE, SLIDER):
        d.update(solveLimit=bool(f & 1), solveMotor=bool(f & 2), limitSign=float(rec[1]), motorVelocity=float(rec[2]), maxMotorImpulse=float(rec[10]),
                 impulses=dict(limit=float(rec[5]), motor=float(rec[7])))
    if jtype == HINGE:
        d["angle"] = float(rec[15])
    if jtype == CONE_TWIST:
        q = np.asarray(rec[17:21], np.float32)
        identity = not q[:3].any() and q[3] == 1.0
        d.update(solveSwingLimit=bool(f & 1), solveTwistLimit=bool(f & 2), solveSwingMotor=bool(f & 4), solveTwistMotor=bool(f & 8), twistSign=float(rec[1]),
                 swingMotorVelocity=float(rec[3]), twistMotorVelocity=float(rec[4]), maxSwingMotorImpulse=float(rec[11]), maxTwistMotorImpulse=float(rec[12]),
                 impulses=dict(swing=float(rec[6]), twist=float(rec[5]), swingMotor=float(rec[8]), twistMotor=float(rec[9])),
                 twistAngle=float(rec[15]), swingAngle=float(rec[16]), swingRotation=q.astype(np.float64),
                 # the antiparallel branch leaves w = cos(pi / 2) in float32 (4e-8); the general one w >= sqrt(2e-6) / 2 = 7e-4
                 rotateFromTo="identity" if identity else ("antiparallel" if abs(q[3]) < 1e-5 else "general"), swingSq=bool(q[:3].any()),
                 swingMotorAxisZero=not np.asarray(rec[21:24]).any())
    return d
