"""Plain-Python restatement of calc_spline_course (10_path_planning_00_cubic_spline_path.py :313-325) and of the classes
under it, one statement per rounding, with the solve of `c` as an argument:

    solver="thomas"   the Thomas recurrence of csrc/rpp_spline.h -- this module is its definition
    solver="numpy"    np.linalg.solve(A, B) on the reference's A and B (:148-173), as the reference runs it on this host
    solver=(cx, cy)   c given as data (the reference's own sx.c, sy.c in the known-answer file)

Everything else is the same for the three: s = [0] + cumsum(np.hypot(diff x, diff y)), B, b and d, the sample parameters
k * ds for k < ceil(s[-1] / ds), bisect_right, the position / derivative forms with ** 2.0 and ** 3.0, math.atan2 and the
curvature with ** 2 and ** (3 / 2).  All values are Python floats (float ** float and a numpy double ** float are both
libm's pow)."""
import bisect
import math

import numpy as np

OK, DEGENERATE, REF_RAISES = 0, 1, 2


def knots(x, y):
    """s of CubicSpline2D.__calc_s as a list of floats: np.hypot per chord, summed left to right"""
    s, acc = [0.0], 0.0
    for i in range(len(x) - 1):
        acc = acc + float(np.hypot(np.float64(x[i + 1] - x[i]), np.float64(y[i + 1] - y[i])))
        s.append(acc)
    return s


def rhs(a, s):
    """B of __calc_B (:165-173)"""
    n = len(a)
    B = [0.0] * n
    for i in range(n - 2):
        B[i + 1] = 3.0 * (a[i + 2] - a[i + 1]) / (s[i + 2] - s[i + 1]) - 3.0 * (a[i + 1] - a[i]) / (s[i + 1] - s[i])
    return B


def solve_thomas(a, s):
    """c by the Thomas recurrence over the interior rows 1 .. n-2: no pivoting, c[0] = c[n-1] = 0.0"""
    n = len(a)
    c = [0.0] * n
    if n <= 2:
        return c
    B = rhs(a, s)
    cp, dp = [0.0] * n, [0.0] * n
    for i in range(1, n - 1):
        sub, sup = s[i] - s[i - 1], s[i + 1] - s[i]
        diag = 2.0 * (sub + sup)
        if i == 1:
            den = diag
            dp[i] = B[i] / den
        else:
            den = diag - sub * cp[i - 1]
            dp[i] = (B[i] - sub * dp[i - 1]) / den
        cp[i] = sup / den
    c[n - 2] = dp[n - 2]
    for i in range(n - 3, 0, -1):
        c[i] = dp[i] - cp[i] * c[i + 1]
    return c


def solve_numpy(a, s):
    """c as the reference makes it: A of __calc_A (:148-163), B, np.linalg.solve"""
    n = len(a)
    h = np.diff(s)
    A = np.zeros((n, n))
    A[0, 0] = 1.0
    for i in range(n - 1):
        if i != (n - 2):
            A[i + 1, i + 1] = 2.0 * (h[i] + h[i + 1])
        A[i + 1, i] = h[i]
        A[i, i + 1] = h[i]
    A[0, 1] = 0.0
    A[n - 1, n - 2] = 0.0
    A[n - 1, n - 1] = 1.0
    B = np.zeros(n)
    for i in range(n - 2):
        B[i + 1] = 3.0 * (a[i + 2] - a[i + 1]) / h[i + 1] - 3.0 * (a[i + 1] - a[i]) / h[i]
    return [float(v) for v in np.linalg.solve(A, B)]


def coefficients(a, s, c):
    """b and d of :68-73 for given c"""
    b, d = [], []
    for i in range(len(a) - 1):
        h = s[i + 1] - s[i]
        d.append((c[i + 1] - c[i]) / (3.0 * h))
        b.append(1.0 / h * (a[i + 1] - a[i]) - h / 3.0 * (2.0 * c[i] + c[i + 1]))
    return b, d


def count(s_end, ds):
    """len(np.arange(0, s_end, ds)): ceil of the rounded quotient"""
    return int(math.ceil(s_end / ds))


def parameters(s_end, ds):
    """np.arange(0, s_end, ds) as a list of floats: numpy fills start + k * delta with delta = (0 + ds) - 0"""
    return [float(k) * ds for k in range(count(s_end, ds))]


def pow_(x, y):
    return 0.0 if x == 0.0 else abs(x) ** y


def spline_course(x, y, ds=0.1, solver="thomas"):
    """dict(status, rx, ry, ryaw, rk, s, cx, cy, knots) of one course; with a status other than OK the lists are empty"""
    x, y = [float(v) for v in x], [float(v) for v in y]
    ds = float(ds)
    n = len(x)
    s = knots(x, y)
    out = dict(status=OK, rx=[], ry=[], ryaw=[], rk=[], s=[], cx=[], cy=[], knots=s)
    if any(s[i + 1] - s[i] == 0.0 for i in range(n - 1)):
        out["status"] = DEGENERATE
        return out
    if isinstance(solver, str):
        fn = {"thomas": solve_thomas, "numpy": solve_numpy}[solver]
        cx, cy = fn(x, s), fn(y, s)
    else:
        cx, cy = [float(v) for v in solver[0]], [float(v) for v in solver[1]]
        assert len(cx) == len(cy) == n
    out["cx"], out["cy"] = cx, cy
    bx, dx = coefficients(x, s, cx)
    by, dy = coefficients(y, s, cy)
    ts = parameters(s[-1], ds)
    if ts and ts[-1] >= s[-1]:
        out["status"] = REF_RAISES   # bisect lands on the last knot: the reference's self.b[i] raises IndexError
        return out
    for t in ts:
        i = bisect.bisect(s, t) - 1
        u = t - s[i]
        u2, u3 = pow_(u, 2.0), pow_(u, 3.0)
        out["rx"].append(x[i] + bx[i] * u + cx[i] * u2 + dx[i] * u3)
        out["ry"].append(y[i] + by[i] * u + cy[i] * u2 + dy[i] * u3)
        x1 = bx[i] + 2.0 * cx[i] * u + 3.0 * dx[i] * u2
        y1 = by[i] + 2.0 * cy[i] * u + 3.0 * dy[i] * u2
        x2 = 2.0 * cx[i] + 6.0 * dx[i] * u
        y2 = 2.0 * cy[i] + 6.0 * dy[i] * u
        out["ryaw"].append(math.atan2(y1, x1))
        den = pow_(pow_(x1, 2.0) + pow_(y1, 2.0), 1.5)
        num = y2 * x1 - x2 * y1
        # a numpy double divides by zero without raising
        out["rk"].append(num / den if den != 0.0 else (math.nan if num == 0.0 or num != num else math.copysign(math.inf, num)))
    out["s"] = ts
    return out


def first_hit(rx, ry, obstacles, robot_radius):
    """check_collision of the pose planners (rrt_05 :1625-1638) as BatchSteer reports it: the first circle of the list
    that any point touches, else -1"""
    for j, (ox, oy, size) in enumerate(obstacles):
        thr = (size + robot_radius) ** 2
        for px, py in zip(rx, ry):
            dx, dy = ox - px, oy - py
            if dx * dx + dy * dy <= thr:
                return j
    return -1


def batch(courses, ds, solver="thomas"):
    """The flat form BatchSpline returns for a list of (x, y) courses: dict(status, n_points, total_length, offsets, x, y,
    yaw, k, s, cx, cy); ds is one value or one per course; solver a name or a list of (cx, cy) per course"""
    res = []
    for i, (x, y) in enumerate(courses):
        d = ds if np.ndim(ds) == 0 else ds[i]
        res.append(spline_course(x, y, d, solver if isinstance(solver, str) else solver[i]))
    off = np.zeros(len(res) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r["s"]) for r in res])

    def cat(key):
        return np.array([v for r in res for v in r[key]], dtype=np.float64)
    return dict(status=np.array([r["status"] for r in res], dtype=np.int32), n_points=np.diff(off),
                total_length=np.array([r["knots"][-1] for r in res]), offsets=off, x=cat("rx"), y=cat("ry"), yaw=cat("ryaw"),
                k=cat("rk"), s=cat("s"), cx=[r["cx"] for r in res], cy=[r["cy"] for r in res], per_course=res)
