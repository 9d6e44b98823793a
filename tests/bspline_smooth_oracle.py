"""Plain-Python definition of BatchBSpline.approximate (csrc/rpp_bspline_smooth.h): the smoothing fit of
approximate_b_spline_path (10_path_planning_00_bspline_path.py :12-56), one statement per rounding.  The script fits
UnivariateSpline(distances, x, k=degree, s=s) and the same for y; that is Dierckx's fpcurf, reached through scipy's fpcurf0
(storage limit max(m // 2, 2 (k + 1))) and, when that limit stops it, once more through fpcurf1 with the full m + k + 1
(DESIGN 5.21).  The discrete part -- which data sites become knots -- is restated exactly; the continuous part -- Givens
rotations, back-substitution, the rational root search on the smoothing parameter -- is this module's own arithmetic in the
order written here, which the C++ header repeats statement for statement.  No scipy anywhere.

Operation order (all doubles, no fused multiply-add):
  givens(piv, ww)     store = |piv|; store >= ww: r = ww / piv, dd = store * sqrt(1.0 + r * r); else r = piv / ww,
                      dd = ww * sqrt(1.0 + r * r);  cos = ww / dd, sin = piv / dd, ww = dd
  rota(cos, sin, a, b)   a' = cos * a - sin * b,  b' = cos * b + sin * a
  least squares       data rows in order; the k + 1 basis values of bspline_oracle.basis; for i = 0 .. k with h[i] != 0.0:
                      givens(h[i], A[j][0]), rota on (yi, z[j]), rota on (h[i1], A[j][i1 - i]) for i1 = i+1 .. k;
                      fp = fp + yi * yi after the row
  back-substitution   c[n-1] = z[n-1] / A[n-1][0]; for i = n-2 .. 0: store = z[i]; store = store - c[i+l] * A[i][l],
                      l = 1 .. min(width - 1, n-1-i); c[i] = store / A[i][0]
  residual            term = c[l0] * q[0] accumulated left to right from 0.0; d = term - y; d * d
  jumps (fpdisc)      fac = nrint / (t[n-k-1] - t[k]); prod = h[j]; prod = prod * h[j+i] * fac, i = 1 .. k;
                      b[row][j] = (t[lp+k+1] - t[lp]) / prod
  smoothing step      pinv = 1.0 / p; the jump rows times pinv rotated into a copy of the band (k + 2 wide)
"""
import math

import numpy as np

import bspline_oracle as B

OK, DEGENERATE, TOO_FEW, SINGULAR = 0, 1, 2, 3
TOL, MAXIT = 0.001, 20
CON1, CON9, CON4 = 0.1, 0.9, 0.04
INT_MIN = -2147483648


def _div(a, b):
    return B.div_(a, b)


def givens(piv, ww):
    """(cos, sin, new ww)"""
    store = abs(piv)
    if store >= ww:
        r = _div(ww, piv)
        dd = store * math.sqrt(1.0 + r * r)
    else:
        r = piv / ww
        dd = ww * math.sqrt(1.0 + r * r)
    return _div(ww, dd), _div(piv, dd), dd


def rota(cos, sin, a, b):
    return cos * a - sin * b, cos * b + sin * a


def back(A, z, n, width, c):
    c[n - 1] = _div(z[n - 1], A[n - 1][0])
    for i in range(n - 2, -1, -1):
        store = z[i]
        for l in range(1, min(width - 1, n - 1 - i) + 1):
            store = store - c[i + l] * A[i][l]
        c[i] = _div(store, A[i][0])


def least_squares(u, y, t, n, k, A, z, q, c):
    """The least-squares spline on the knots t[0 .. n-1]: fills the band A, the rotated right-hand side z, the basis rows q
    and the coefficients c; returns fp"""
    m, k1, nk1 = len(u), k + 1, n - k - 1
    for i in range(nk1):
        z[i] = 0.0
        for j in range(k1):
            A[i][j] = 0.0
    fp = 0.0
    l = k
    for it in range(m):
        xi, yi = u[it], y[it]
        while not (xi < t[l + 1] or l == nk1 - 1):
            l += 1
        h = B.basis(t, l, k, xi)[0]
        for i in range(k1):
            q[it][i] = h[i]
        j = l - k
        for i in range(k1):
            piv = h[i]
            if piv != 0.0:
                cos, sin, A[j][0] = givens(piv, A[j][0])
                yi, z[j] = rota(cos, sin, yi, z[j])
                if i == k:
                    break
                i2 = 0
                for i1 in range(i + 1, k1):
                    i2 += 1
                    h[i1], A[j][i2] = rota(cos, sin, h[i1], A[j][i2])
            j += 1
        fp = fp + yi * yi
    back(A, z, nk1, k1, c)
    return fp


def residual_walk(u, y, t, n, k, q, c, it, lz):
    """The squared residual of data point `it` and the advanced knot cursor: (term, lz, crossed)"""
    nk1 = n - k - 1
    crossed = False
    if not (u[it] < t[lz] or lz > nk1 - 1):
        crossed = True
        lz += 1
    l0 = lz - k - 1
    term = 0.0
    for j in range(k + 1):
        term = term + c[l0 + j] * q[it][j]
    d = term - y[it]
    return d * d, lz, crossed


def interval_sums(u, y, t, n, k, q, c, fpint):
    """fpint[0 .. nrint-1]: the squared residuals per knot interval, a data point on a knot split in halves"""
    nrint = n - 2 * (k + 1) + 1
    fpart, i, lz = 0.0, 0, k + 1
    for it in range(len(u)):
        term, lz, crossed = residual_walk(u, y, t, n, k, q, c, it, lz)
        fpart = fpart + term
        if crossed:
            store = term * 0.5
            fpint[i] = fpart - store
            i += 1
            fpart = store
    fpint[nrint - 1] = fpart


def add_knot(u, t, n, k, fpint, nrdata, nrint):
    """fpknot: one more knot in the interval of the largest fpint that still holds data; returns the new n (n itself when
    no interval qualifies)"""
    fpmax, jbegin, number, maxpt, maxbeg = 0.0, 1, -1, 0, 0
    for j in range(nrint):
        jpoint = nrdata[j]
        if not (fpmax >= fpint[j] or jpoint == 0):
            fpmax, number, maxpt, maxbeg = fpint[j], j, jpoint, jbegin
        jbegin += jpoint + 1
    if number < 0:
        return n
    ihalf = maxpt // 2 + 1
    nrx = maxbeg + ihalf
    nxt = number + 1
    for jj in range(nrint - 1, nxt - 1, -1):
        fpint[jj + 1] = fpint[jj]
        nrdata[jj + 1] = nrdata[jj]
        t[jj + k + 1] = t[jj + k]
    nrdata[number] = ihalf - 1
    nrdata[nxt] = maxpt - ihalf
    am = float(maxpt)
    fpint[number] = fpmax * float(nrdata[number]) / am
    fpint[nxt] = fpmax * float(nrdata[nxt]) / am
    t[nxt + k] = u[nrx - 1]
    return n + 1


def jumps(t, n, k, b):
    """fpdisc: b[0 .. n-2k-3][0 .. k+1], the jumps of the k-th derivative at the interior knots"""
    k1, k2, nk1 = k + 1, k + 2, n - k - 1
    nrint = nk1 - k
    fac = float(nrint) / (t[nk1] - t[k])
    h = [0.0] * (2 * k1)
    for l in range(k1, nk1):
        row = l - k1
        for j in range(k1):
            h[j] = t[l] - t[l + j - k1]
            h[j + k1] = t[l] - t[l + j + 1]
        lp = row
        for j in range(k2):
            prod = h[j]
            for i in range(1, k + 1):
                prod = prod * h[j + i] * fac
            b[row][j] = (t[lp + k1] - t[lp]) / prod
            lp += 1


def rational(p1, f1, p2, f2, p3, f3):
    """fprati: (p, p1, f1, p3, f3)"""
    if p3 > 0.0:
        h1 = f1 * (f2 - f3)
        h2 = f2 * (f3 - f1)
        h3 = f3 * (f1 - f2)
        p = _div(-(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2), p1 * h1 + p2 * h2 + p3 * h3)
    else:
        p = _div(p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1, (f1 - f2) * f3)
    if f2 < 0.0:
        return p, p1, f1, p2, f2
    return p, p2, f2, p3, f3


def smooth_step(u, y, t, n, k, A, z, q, b, p, G, c):
    """One evaluation of f(p) + s: the coefficients c of the smoothing spline with parameter p, and its fp"""
    k1, k2, nk1 = k + 1, k + 2, n - k - 1
    n8 = n - 2 * k1
    pinv = 1.0 / p
    for i in range(nk1):
        c[i] = z[i]
        G[i][k1] = 0.0
        for j in range(k1):
            G[i][j] = A[i][j]
    h = [0.0] * (k2 + 1)
    for it in range(n8):
        for i in range(k2):
            h[i] = b[it][i] * pinv
        yi = 0.0
        for j in range(it, nk1):
            piv = h[0]
            cos, sin, G[j][0] = givens(piv, G[j][0])
            yi, c[j] = rota(cos, sin, yi, c[j])
            if j == nk1 - 1:
                break
            i2 = k1
            if j + 1 > n8:
                i2 = nk1 - j - 1
            for i in range(i2):
                h[i + 1], G[j][i + 1] = rota(cos, sin, h[i + 1], G[j][i + 1])
                h[i] = h[i + 1]
            h[i2] = 0.0
    back(G, c, nk1, k2, c)
    fp, lz = 0.0, k1
    for it in range(len(u)):
        term, lz, _ = residual_walk(u, y, t, n, k, q, c, it, lz)
        fp = fp + term
    return fp


def fit(u, y, k, s, trace=None):
    """One axis: dict(t, c, n, ier, fp, p, rounds, iters, events).  ier: 0, -1 (interpolating), -2 (polynomial), 1 (no
    interval can take a knot: the least-squares spline on the current knots), 2, 3.  trace, a list, receives the nplus of
    every knot round.  events names the paths the fit took (bookkeeping of the tests; no arithmetic depends on it)."""
    events = set()
    m = len(u)
    k1, k2 = k + 1, k + 2
    nmin, nmax = 2 * k1, m + k1
    nest = max(m // 2, nmin)
    acc = TOL * s
    t = [0.0] * (nmax + 1)
    c = [0.0] * (m + 1)
    z = [0.0] * (m + 1)
    A = [[0.0] * k1 for _ in range(m + 1)]
    q = [[0.0] * k1 for _ in range(m)]
    fpint = [0.0] * (m + 1)
    nrdata = [0] * (m + 1)
    n, fpold, nplus, fp0, fp, fpms = nmin, 0.0, 0, 0.0, 0.0, 0.0
    nrdata[0] = m - 2
    ier, rounds, iters = 0, 0, 0
    done = False
    for _ in range(2 * m + 8):
        if n == nmin:
            ier = -2
        nrint, nk1 = n - nmin + 1, n - k1
        for j in range(k1):
            t[j] = u[0]
            t[n - 1 - j] = u[m - 1]
        fp = least_squares(u, y, t, n, k, A, z, q, c)
        rounds += 1
        if ier == -2:
            fp0 = fp
        fpms = fp - s
        if abs(fpms) < acc:
            events.add("accepted_within_acc_in_knot_loop")
            done = True
            break
        if fpms < 0.0:
            break
        if n == nmax:
            events.add("interpolating_with_s_above_0")
            ier = -1
            done = True
            break
        if n == nest:         # the first pass (fpcurf0) returns ier = 1 here; fpcurf1 goes on with the full storage
            events.add("second_stage")
            nest = nmax
            ier = 1
        if ier != 0:
            nplus = 1
            ier = 0
        else:
            npl1 = nplus * 2
            if fpold - fp > acc:
                v = float(nplus) * fpms / (fpold - fp)
                npl1 = int(v) if v < 2147483648.0 else INT_MIN     # the conversion of an x86-64 cvttsd2si
            nplus = min(nplus * 2, max(npl1, nplus // 2, 1))
        fpold = fp
        if trace is not None:
            trace.append(nplus)
        interval_sums(u, y, t, n, k, q, c, fpint)
        for _l in range(nplus):
            n2 = add_knot(u, t, n, k, fpint, nrdata, nrint)
            if n2 == n:       # FITPACK's fpknot is undefined here; this definition: no further knot in this round, and a
                if _l == 0:   # round that adds none ends the fit on the current knots
                    events.add("no_interval_for_a_knot")
                    ier = 1
                    done = True
                break
            n, nrint = n2, nrint + 1
            if n == nmax:
                tk = B.knots(u, k)
                for j in range(n):
                    t[j] = tk[j]
                break
            if n == nest:
                break
        if done:
            break
    nk1 = n - k1
    out = dict(n=n, rounds=rounds, iters=0, p=math.inf, events=events)
    if done or ier == -2:
        out.update(t=t[:n], c=c[:nk1], ier=ier, fp=fp)
        return out
    # the smoothing spline: the root of f(p) = fp(p) - s
    b = [[0.0] * k2 for _ in range(m + 1)]
    G = [[0.0] * k2 for _ in range(m + 1)]
    jumps(t, n, k, b)
    p1, f1, p3, f3 = 0.0, fp0 - s, -1.0, fpms
    p = 0.0
    for i in range(nk1):
        p = p + A[i][0]
    p = float(nk1) / p
    ich1 = ich3 = 0
    ier = 0
    for it in range(1, MAXIT + 1):
        fp = smooth_step(u, y, t, n, k, A, z, q, b, p, G, c)
        iters = it
        fpms = fp - s
        if abs(fpms) < acc:
            break
        if it == MAXIT:
            ier = 3
            break
        p2, f2 = p, fpms
        if ich3 == 0:
            if not (f2 - f3 > acc):      # the initial choice of p is too large
                events.add("p_too_large")
                p3, f3 = p2, f2
                p = p * CON4
                if p <= p1:
                    p = p1 * CON9 + p2 * CON1
                continue
            if f2 < 0.0:
                ich3 = 1
        if ich1 == 0:
            if not (f1 - f2 > acc):      # the initial choice of p is too small
                p1, f1 = p2, f2
                p = p / CON4
                if p3 < 0.0:
                    events.add("p_too_small_unbracketed")
                    continue
                events.add("p_too_small_bracketed")
                if p >= p3:
                    events.add("p_too_small_pulled_back")
                    p = p2 * CON1 + p3 * CON9
                continue
            if f2 > 0.0:
                ich1 = 1
        if f2 >= f1 or f2 <= f3:
            ier = 2
            break
        p, p1, f1, p3, f3 = rational(p1, f1, p2, f2, p3, f3)
    out.update(t=t[:n], c=c[:nk1], ier=ier, fp=fp, p=p, iters=iters)
    return out


def eval_axis(t, n, k, c, v):
    """(value, first, second derivative) of one axis at v"""
    mu = B.find_span(t, n - k - 1, k, v)
    N, D1, D2 = B.weights(t, mu, k, v)
    lo = mu - k
    return B.dot(c, lo, N), B.dot(c, lo, D1), B.dot(c, lo, D2)


def course(x, y, degree=3, s=None, n_path_points=None, u=None):
    """dict(status, degree, length, x, y, yaw, k, u, axes) of approximate_b_spline_path(x, y, n_path_points, degree, s); axes
    holds the two fit() dicts (for s == 0 the interpolating spline of bspline_oracle: ier -1, fp 0.0, no rounds).  With a
    status other than OK there are no points and the axes are empty."""
    x, y = [float(v) for v in x], [float(v) for v in y]
    m, k = len(x), int(degree)
    sv = float(m) if s is None else float(s)
    wp_u = B.parameter(x, y, B.NORMALISED)
    none = dict(t=[], c=[], n=0, ier=0, fp=0.0, p=0.0, rounds=0, iters=0, events=set())
    out = dict(status=OK, degree=k, length=0.0, x=[], y=[], yaw=[], k=[], u=[], axes=[none, none])
    if not B.strictly_increasing(wp_u) or m <= k:
        out["status"] = DEGENERATE if not B.strictly_increasing(wp_u) else TOO_FEW
        return out
    if sv == 0.0:
        t = B.knots(wp_u, k)
        cx, cy = B.fit(wp_u, t, k, x, y)
        axes = [dict(t=t, c=c, n=len(t), ier=-1, fp=0.0, p=math.inf, rounds=0, iters=0, events=set()) for c in (cx, cy)]
    else:
        axes = [fit(wp_u, a, k, sv) for a in (x, y)]
    out["axes"] = axes
    if not all(math.isfinite(v) for a in axes for v in a["c"]):
        out["status"] = SINGULAR
        return out
    out["length"] = wp_u[-1]
    us = [float(v) for v in u] if u is not None else B.linspace(wp_u[-1], int(n_path_points))
    for v in us:
        px, dx, ddx = eval_axis(axes[0]["t"], axes[0]["n"], k, axes[0]["c"], v)
        py, dy, ddy = eval_axis(axes[1]["t"], axes[1]["n"], k, axes[1]["c"], v)
        yaw, kap = B.point(dx, dy, ddx, ddy)
        for key, q in zip(("x", "y", "yaw", "k"), (px, py, yaw, kap)):
            out[key].append(q)
    out["u"] = us
    return out


def batch(courses, n_path_points=None, degree=3, s=None, u=None):
    """The flat form BatchBSpline.approximate returns for a list of (x, y) courses; n_path_points, degree and s are one value
    or one per course (s: None or an entry None means the course's waypoint count), u a list with a sample list or None"""
    def per(v, i):
        return None if v is None else (v if np.ndim(v) == 0 else v[i])
    res = []
    for i, (x, y) in enumerate(courses):
        ui = None if u is None else u[i]
        res.append(course(x, y, per(degree, i), per(s, i), None if ui is not None else per(n_path_points, i), ui))
    off = np.zeros(len(res) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r["u"]) for r in res])

    def cat(key):
        return np.array([v for r in res for v in r[key]], dtype=np.float64)
    out = dict(status=np.array([r["status"] for r in res], dtype=np.int32), degree=np.array([r["degree"] for r in res], dtype=np.int32),
               n_points=np.diff(off), length=np.array([r["length"] for r in res]), offsets=off, x=cat("x"), y=cat("y"),
               yaw=cat("yaw"), k=cat("k"), u=cat("u"), per_course=res)
    for a in (0, 1):        # per axis: (n,) records and CSR knots and coefficients
        ax = [r["axes"][a] for r in res]
        koff = np.zeros(len(res) + 1, dtype=np.int64)
        koff[1:] = np.cumsum([len(q["t"]) for q in ax])
        coff = np.zeros(len(res) + 1, dtype=np.int64)
        coff[1:] = np.cumsum([len(q["c"]) for q in ax])
        out["axis%d" % a] = dict(knots=np.array([v for q in ax for v in q["t"]], dtype=np.float64), knot_offsets=koff,
                                 coefficients=np.array([v for q in ax for v in q["c"]], dtype=np.float64), coef_offsets=coff,
                                 ier=np.array([q["ier"] for q in ax], dtype=np.int32), fp=np.array([q["fp"] for q in ax]),
                                 p=np.array([q["p"] for q in ax]), rounds=np.array([q["rounds"] for q in ax], dtype=np.int32),
                                 iters=np.array([q["iters"] for q in ax], dtype=np.int32))
    return out
