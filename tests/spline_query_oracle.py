"""Plain-Python restatement of the pointwise methods of 10_path_planning_00_cubic_spline_path.py -- CubicSpline1D.calc_position
/ calc_first_derivative / calc_second_derivative (:75-140) and CubicSpline2D.calc_position / calc_yaw / calc_curvature
(:248-310) -- at a parameter of the caller's choosing, one statement per rounding, on the forms of spline_oracle (knots,
coefficients, pow_) and with its three solvers ("thomas", "numpy", or c given as data).

What the reference does with a parameter t is a status:

    Q_OK          answered
    Q_OUTSIDE     t < s[0] or t > s[-1] (+-inf too): calc_position returns None
    Q_REF_RAISES  t == s[-1], or t is NaN: both range tests are false, bisect lands on the last knot, self.b[i] raises
    Q_NO_SPLINE   the spline has two equal consecutive knots (spline_oracle.DEGENERATE)

-0.0 is accepted (-0.0 < 0 is false); there u = -0.0, u ** 2.0 = +0.0 and u ** 3.0 = -0.0 on a numpy double, which
spline_oracle.pow_ (made for sampled parameters k * ds) does not say: u3 takes the sign of u here (math.copysign)."""
import bisect
import math

import numpy as np

import spline_oracle as SO

Q_OK, Q_OUTSIDE, Q_REF_RAISES, Q_NO_SPLINE = 0, 1, 2, 3
NAN = math.nan


def classify(s, t):
    """The status of parameter t on a spline over the knots s (:86-91)"""
    if t < s[0] or t > s[-1]:
        return Q_OUTSIDE
    if not t < s[-1]:
        return Q_REF_RAISES
    return Q_OK


def axis_forms(s, a, b, c, d, t):
    """(position :93-94, first derivative :117, second derivative :139) of one axis at a parameter whose status is Q_OK"""
    i = bisect.bisect(s, t) - 1
    u = t - s[i]
    u2 = SO.pow_(u, 2.0)
    u3 = math.copysign(SO.pow_(u, 3.0), u)
    p = a[i] + b[i] * u + c[i] * u2 + d[i] * u3
    p1 = b[i] + 2.0 * c[i] * u + 3.0 * d[i] * u2
    p2 = 2.0 * c[i] + 6.0 * d[i] * u
    return p, p1, p2


def curvature(x1, y1, x2, y2):
    """calc_curvature :289; a numpy double divides by zero without raising"""
    den = SO.pow_(SO.pow_(x1, 2.0) + SO.pow_(y1, 2.0), 1.5)
    num = y2 * x1 - x2 * y1
    return num / den if den != 0.0 else (NAN if num == 0.0 or num != num else math.copysign(math.inf, num))


def _solve(a, s, solver):
    if isinstance(solver, str):
        return {"thomas": SO.solve_thomas, "numpy": SO.solve_numpy}[solver](a, s)
    c = [float(v) for v in solver]
    assert len(c) == len(a)
    return c


def fit1d(knots, values, solver="thomas"):
    """CubicSpline1D(knots, values): dict(axes=1, status, s, a, b, c, d); solver "thomas", "numpy" or c as data"""
    s, a = [float(v) for v in knots], [float(v) for v in values]
    f = dict(axes=1, status=SO.OK, s=s, a=[a], b=[[]], c=[[0.0] * len(a)], d=[[]])
    if any(s[i + 1] - s[i] == 0.0 for i in range(len(s) - 1)):
        f["status"] = SO.DEGENERATE
        return f
    c = _solve(a, s, solver)
    b, d = SO.coefficients(a, s, c)
    f.update(b=[b], c=[c], d=[d])
    return f


def fit2d(x, y, solver="thomas"):
    """CubicSpline2D(x, y): dict(axes=2, status, s, a, b, c, d) with one list per axis; solver a name or (cx, cy)"""
    x, y = [float(v) for v in x], [float(v) for v in y]
    s = SO.knots(x, y)
    f = dict(axes=2, status=SO.OK, s=s, a=[x, y], b=[[], []], c=[[0.0] * len(x)] * 2, d=[[], []])
    if any(s[i + 1] - s[i] == 0.0 for i in range(len(s) - 1)):
        f["status"] = SO.DEGENERATE
        return f
    cs = [_solve(a, s, solver if isinstance(solver, str) else solver[k]) for k, a in enumerate((x, y))]
    bd = [SO.coefficients(a, s, c) for a, c in zip((x, y), cs)]
    f.update(b=[q[0] for q in bd], c=cs, d=[q[1] for q in bd])
    return f


PLANES = {2: ("x", "y", "yaw", "k", "dx", "dy", "ddx", "ddy"), 1: ("y", "dy", "ddy")}


def query(f, t):
    """(status, dict of the planes of f's axes) of one parameter; every value is NaN unless the status is Q_OK"""
    t = float(t)
    names = PLANES[f["axes"]]
    st = Q_NO_SPLINE if f["status"] == SO.DEGENERATE else classify(f["s"], t)
    if st != Q_OK:
        return st, dict.fromkeys(names, NAN)
    ax = [axis_forms(f["s"], f["a"][k], f["b"][k], f["c"][k], f["d"][k], t) for k in range(f["axes"])]
    if f["axes"] == 1:
        return st, dict(y=ax[0][0], dy=ax[0][1], ddy=ax[0][2])
    (x, x1, x2), (y, y1, y2) = ax
    return st, dict(x=x, y=y, yaw=math.atan2(y1, x1), k=curvature(x1, y1, x2, y2), dx=x1, dy=y1, ddx=x2, ddy=y2)


def batch(fits, q_off, t):
    """The flat form BatchSpline.query returns for a list of fits (all of one kind) and a CSR list of parameters:
    dict(offsets, s, status, and the planes of the fits' axes)"""
    names = PLANES[fits[0]["axes"]] if fits else ()
    out = {k: [] for k in names}
    status = []
    for i, f in enumerate(fits):
        for q in range(int(q_off[i]), int(q_off[i + 1])):
            st, v = query(f, t[q])
            status.append(st)
            for k in names:
                out[k].append(v[k])
    res = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    res.update(offsets=np.asarray(q_off, dtype=np.int64), s=np.asarray(t, dtype=np.float64),
               status=np.array(status, dtype=np.int32))
    return res
