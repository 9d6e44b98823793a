"""Plain-Python definition of BatchBSpline (csrc/rpp_bspline.h): interpolating B-spline courses of degree 1 .. 5 through
waypoints, one statement per rounding.  Two scripts of the reference are this one object:

    interpolate_b_spline_path(x, y, n, degree)   10_path_planning_00_bspline_path.py :59-108  -> course(..., param=NORMALISED)
    Spline2D(x, y, kind) and its driver loop      10_path_planning_00_spline_2d.py   :12-55   -> course(..., param=CHORD)

The reference's, restated exactly: the waypoint parameters (`_calc_distance_vector`, `Spline2D.__calc_s`), the knot vector
that FITPACK (s = 0) and make_interp_spline's not-a-knot default both choose, the sample lists (np.linspace, np.arange), the
counts, and interp1d's linear kind.  This module's own definition: the collocation matrix by the Cox-de Boor recurrence, the
banded elimination without pivoting, and the evaluation of value, first and second derivative.  No scipy anywhere.

Operation order (all doubles, no fused multiply-add):
  basis(t, mu, k, x)      N = [1.0]; for j = 1 .. k: left[j] = x - t[mu+1-j], right[j] = t[mu+j] - x, saved = 0.0,
                          for r = 0 .. j-1: temp = N[r] / (right[r+1] + left[j-r]); N[r] = saved + right[r+1] * temp;
                          saved = left[j-r] * temp;  then N[j] = saved.  The rows of degree k-2, k-1 and k are kept.
  derivatives             den[r] = t[mu+1+r] - t[mu-k+1+r]                                   r = 0 .. k-1
                          a1[r] = Nk1[r] / den[r];                 D1[r] = k * (a1[r-1] - a1[r])          r = 0 .. k
                          a2[r] = Nk2[r] / (t[mu+1+r] - t[mu-k+2+r])                         r = 0 .. k-2
                          E[r] = (k-1) * (a2[r-1] - a2[r]);  b[r] = E[r] / den[r]            r = 0 .. k-1
                          D2[r] = k * (b[r-1] - b[r])                                        r = 0 .. k
                          (a term whose index falls outside its range is 0.0; degree 1 has D2 = 0.0)
  dot products            acc = c[mu-k] * w[0]; acc = acc + c[mu-k+r] * w[r] for r = 1 .. k
  fit                     band rows A[i][j] = N_j(u_i), |i - j| <= k; for p = 0 .. m-2: for r = p+1 .. min(p+k, m-1):
                          l = A[r][p] / A[p][p]; A[r][p] = l; A[r][c] = A[r][c] - l * A[p][c] for c = p+1 .. min(p+k, m-1).
                          Per axis: y[r] = y[r] - A[r][p] * y[p] in the same p, r order; then for i = m-1 .. 0:
                          acc = y[i]; acc = acc - A[i][c] * y[c] for c = i+1 .. min(i+k, m-1); y[i] = acc / A[i][i].
"""
import math

import numpy as np

OK, DEGENERATE, TOO_FEW = 0, 1, 2
NORMALISED, CHORD = 0, 1      # the waypoint parameter: bspline_path's u in [0, 1], spline_2d's s in metres
KINDS = {"linear": 1, "quadratic": 2, "cubic": 3}
TWO_THIRDS = 2.0 / 3.0


def parameter(x, y, param):
    """The waypoint parameter as a list of floats: np.hypot per chord, summed left to right; NORMALISED divides every
    entry by the last (`distances /= distances[-1]`, :95)"""
    s, acc = [0.0], 0.0
    for i in range(len(x) - 1):
        acc = acc + float(np.hypot(np.float64(x[i + 1] - x[i]), np.float64(y[i + 1] - y[i])))
        s.append(acc)
    if param == NORMALISED:
        last = s[-1]
        if last != 0.0:      # all waypoints equal: left as zeros, which the caller reports as DEGENERATE
            s = [v / last for v in s]
    return s


def strictly_increasing(u):
    return all(u[i + 1] > u[i] for i in range(len(u) - 1))


def knots(u, k):
    """Clamped ends of multiplicity k + 1; interior: odd k the data sites u[(k+1)/2 .. m-1-(k+1)/2], even k the midpoints
    (u[j] + u[j+1]) / 2 for j = k/2 .. m-2-k/2"""
    m = len(u)
    if k % 2:
        inner = [u[j] for j in range((k + 1) // 2, m - (k + 1) // 2)]
    else:
        inner = [(u[j] + u[j + 1]) / 2.0 for j in range(k // 2, m - 1 - k // 2)]
    return [u[0]] * (k + 1) + inner + [u[-1]] * (k + 1)


def find_span(t, m, k, x):
    """mu in [k, m-1] with t[mu] <= x < t[mu+1]; x at (or past) the last knot gets the last non-empty span m - 1"""
    lo, hi = k, m
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if x < t[mid]:
            hi = mid
        else:
            lo = mid
    return lo


def basis(t, mu, k, x):
    """(Nk, Nk1, Nk2): the non-zero basis functions of degree k, k-1 and k-2 on span mu at x (Nk2 is [] for k = 1)"""
    N = [1.0]
    rows = {0: [1.0]}
    left, right = [0.0] * (k + 1), [0.0] * (k + 1)
    for j in range(1, k + 1):
        left[j] = x - t[mu + 1 - j]
        right[j] = t[mu + j] - x
        saved = 0.0
        for r in range(j):
            temp = N[r] / (right[r + 1] + left[j - r])
            N[r] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        N.append(saved)
        rows[j] = list(N)
    return rows[k], rows[k - 1], rows.get(k - 2, [])


def weights(t, mu, k, x):
    """(N, D1, D2): k + 1 weights each of the coefficients c[mu-k .. mu] for value, first and second derivative"""
    Nk, Nk1, Nk2 = basis(t, mu, k, x)
    den = [t[mu + 1 + r] - t[mu - k + 1 + r] for r in range(k)]
    a1 = [Nk1[r] / den[r] for r in range(k)]
    D1 = [float(k) * ((a1[r - 1] if r >= 1 else 0.0) - (a1[r] if r < k else 0.0)) for r in range(k + 1)]
    if k == 1:
        return Nk, D1, [0.0, 0.0]
    a2 = [Nk2[r] / (t[mu + 1 + r] - t[mu - k + 2 + r]) for r in range(k - 1)]
    E = [float(k - 1) * ((a2[r - 1] if r >= 1 else 0.0) - (a2[r] if r < k - 1 else 0.0)) for r in range(k)]
    b = [E[r] / den[r] for r in range(k)]
    D2 = [float(k) * ((b[r - 1] if r >= 1 else 0.0) - (b[r] if r < k else 0.0)) for r in range(k + 1)]
    return Nk, D1, D2


def dot(c, lo, w):
    acc = c[lo] * w[0]
    for r in range(1, len(w)):
        acc = acc + c[lo + r] * w[r]
    return acc


def fit(u, t, k, ax, ay):
    """(cx, cy): the B-spline coefficients of the two axes"""
    m = len(u)
    A = [[0.0] * (2 * k + 1) for _ in range(m)]     # A[i][j - i + k]
    for i in range(m):
        mu = find_span(t, m, k, u[i])
        Nk = basis(t, mu, k, u[i])[0]
        for r in range(k + 1):
            d = mu - k + r - i + k
            if 0 <= d <= 2 * k:
                A[i][d] = Nk[r]
    for p in range(m - 1):
        piv = A[p][k]
        for r in range(p + 1, min(p + k, m - 1) + 1):
            l = A[r][p - r + k] / piv
            A[r][p - r + k] = l
            for c in range(p + 1, min(p + k, m - 1) + 1):
                A[r][c - r + k] = A[r][c - r + k] - l * A[p][c - p + k]
    out = []
    for a in (ax, ay):
        y = list(a)
        for p in range(m - 1):
            for r in range(p + 1, min(p + k, m - 1) + 1):
                y[r] = y[r] - A[r][p - r + k] * y[p]
        for i in range(m - 1, -1, -1):
            acc = y[i]
            for c in range(i + 1, min(i + k, m - 1) + 1):
                acc = acc - A[i][c - i + k] * y[c]
            y[i] = acc / A[i][k]
        out.append(y)
    return out[0], out[1]


def linspace(stop, n):
    """np.linspace(0.0, stop, n) as a list of floats: k * step with step = (stop - 0.0) / (n - 1), the last entry set to
    stop; n = 1 gives [0.0].  (A step that underflows to zero takes numpy's other branch, k / (n - 1) * stop.)"""
    if n == 1:
        return [0.0]
    div = float(n - 1)
    step = stop / div
    if step == 0.0:
        out = [float(k) / div * stop for k in range(n)]
    else:
        out = [float(k) * step for k in range(n)]
    out[-1] = stop
    return out


def arange(stop, ds):
    """np.arange(0, stop, ds) as a list of floats: ceil(stop / ds) entries k * ds (tests/spline_oracle.py pins the same)"""
    return [float(k) * ds for k in range(int(math.ceil(stop / ds)))]


def div_(num, den):
    """a numpy double divides by zero without raising"""
    if den != 0.0:
        return num / den
    return math.nan if num == 0.0 or num != num else math.copysign(math.inf, num)


def pow_(x, y):
    return 0.0 if x == 0.0 else abs(x) ** y


def point(dx, dy, ddx, ddy):
    """(yaw, k) of _evaluate_spline :104-107 -- the exponent is the script's 2.0 / 3.0, kept as it is"""
    return math.atan2(dy, dx), div_(ddy * dx - ddx * dy, pow_(dx * dx + dy * dy, TWO_THIRDS))


def eval_spline(t, m, k, cx, cy, v):
    """(x, y, yaw, k) at parameter v"""
    mu = find_span(t, m, k, v)
    N, D1, D2 = weights(t, mu, k, v)
    lo = mu - k
    px, py = dot(cx, lo, N), dot(cy, lo, N)
    yaw, kap = point(dot(cx, lo, D1), dot(cy, lo, D1), dot(cx, lo, D2), dot(cy, lo, D2))
    return px, py, yaw, kap


def eval_linear(s, ax, ay, v):
    """interp1d(kind="linear") at v.  For real one-dimensional data interp1d hands the call to np.interp, restated here: j is
    the last waypoint with s[j] <= v; at or past the last waypoint the value is the last waypoint's, on a waypoint exactly
    that waypoint's, else slope * (v - s[j]) + a[j] with slope = (a[j+1] - a[j]) / (s[j+1] - s[j]).  yaw and k, from the
    slopes of that interval (the last interval at the end) and a zero second derivative, are this package's additions."""
    m = len(s)
    lo, hi = 0, m
    while lo < hi:
        mid = (lo + hi) // 2
        if v < s[mid]:
            hi = mid
        else:
            lo = mid + 1
    j = lo - 1
    i = min(max(j, 0), m - 2)
    h = s[i + 1] - s[i]
    sx, sy = (ax[i + 1] - ax[i]) / h, (ay[i + 1] - ay[i]) / h
    if j < 0:
        px, py = ax[0], ay[0]
    elif j >= m - 1:
        px, py = ax[m - 1], ay[m - 1]
    elif s[j] == v:
        px, py = ax[j], ay[j]
    else:
        px, py = sx * (v - s[j]) + ax[j], sy * (v - s[j]) + ay[j]
    yaw, kap = point(sx, sy, 0.0, 0.0)
    return px, py, yaw, kap


def course(x, y, degree=3, param=NORMALISED, n_path_points=None, ds=None, u=None):
    """dict(status, degree, x, y, yaw, k, u, wp_u, knots, cx, cy, length) of one course.  Exactly one of n_path_points
    (np.linspace(0.0, wp_u[-1], n)), ds (np.arange(0, wp_u[-1], ds)) and u (samples as data) is given.  With a status
    other than OK the lists of points, knots and coefficients are empty."""
    x, y = [float(v) for v in x], [float(v) for v in y]
    m, k = len(x), int(degree)
    wp_u = parameter(x, y, param)
    out = dict(status=OK, degree=k, x=[], y=[], yaw=[], k=[], u=[], wp_u=wp_u, knots=[], cx=[], cy=[], length=wp_u[-1])
    if not strictly_increasing(wp_u) or m <= k:
        out["status"] = DEGENERATE if not strictly_increasing(wp_u) else TOO_FEW
        out["length"] = 0.0      # a course without a spline reports no length
        return out
    t = knots(wp_u, k)
    cx, cy = fit(wp_u, t, k, x, y)
    out["knots"], out["cx"], out["cy"] = t, cx, cy
    if u is not None:
        us = [float(v) for v in u]
    elif ds is not None:
        us = arange(wp_u[-1], float(ds))
    else:
        us = linspace(wp_u[-1], int(n_path_points))
    for v in us:
        p = eval_linear(wp_u, x, y, v) if (param == CHORD and k == 1) else eval_spline(t, m, k, cx, cy, v)
        for key, q in zip(("x", "y", "yaw", "k"), p):
            out[key].append(q)
    out["u"] = us
    return out


def first_hit(rx, ry, obstacles, robot_radius):
    """As spline_oracle.first_hit: the first circle of the list that any point touches, else -1"""
    for j, (ox, oy, size) in enumerate(obstacles):
        thr = (size + robot_radius) ** 2
        for px, py in zip(rx, ry):
            dx, dy = ox - px, oy - py
            if dx * dx + dy * dy <= thr:
                return j
    return -1


def batch(courses, degree=3, param=NORMALISED, n_path_points=None, ds=None, u=None):
    """The flat form BatchBSpline returns for a list of (x, y) courses; degree, n_path_points and ds are one value or one
    per course, u a list with a sample list or None per course (None: the course keeps n_path_points / ds)"""
    def per(v, i):
        return None if v is None else (v if np.ndim(v) == 0 else v[i])
    res = []
    for i, (x, y) in enumerate(courses):
        ui = None if u is None else u[i]
        res.append(course(x, y, per(degree, i), param, None if ui is not None else per(n_path_points, i),
                          None if ui is not None else per(ds, i), ui))
    off = np.zeros(len(res) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r["u"]) for r in res])
    koff = np.zeros(len(res) + 1, dtype=np.int64)
    koff[1:] = np.cumsum([len(r["knots"]) for r in res])
    wp_off = np.zeros(len(res) + 1, dtype=np.int64)
    wp_off[1:] = np.cumsum([len(c[0]) for c in courses])

    def cat(key):
        return np.array([v for r in res for v in r[key]], dtype=np.float64)

    def coef(key):
        return np.array([v for r, c in zip(res, courses) for v in (r[key] if r["status"] == OK else [0.0] * len(c[0]))])
    return dict(status=np.array([r["status"] for r in res], dtype=np.int32), degree=np.array([r["degree"] for r in res], dtype=np.int32),
                n_points=np.diff(off), length=np.array([r["length"] for r in res]), offsets=off, x=cat("x"), y=cat("y"),
                yaw=cat("yaw"), k=cat("k"), u=cat("u"), knots=cat("knots"), knot_offsets=koff, cx=coef("cx"), cy=coef("cy"),
                wp_offsets=wp_off, per_course=res)
