"""Golden generator of BatchBSpline: runs the reference's interpolate_b_spline_path, _calc_distance_vector and _evaluate_spline
(10_path_planning_00_bspline_path.py) and Spline2D (10_path_planning_00_spline_2d.py), loaded through oracle/ref_loader.py (the
file names are added to ref_loader.FILES at run time), and writes tests/golden/bspline_kat.npz.  Build host only: needs the
reference checkout and scipy.

    python tools/gen_golden_bspline.py

Arrays only; 65 courses, the first N_BSP of script 0 (bspline_path), the rest of script 1 (spline_2d).
Courses: script, degree, mode (0 np.linspace, 1 np.arange, 2 samples as data), count (n_path_points), ds -- (n,) each; wp_off
(n + 1,) CSR into wp_x, wp_y (the waypoints), wp_u (the reference's parameter: _calc_distance_vector or Spline2D.s) and cx, cy
(the reference's B-spline coefficients: UnivariateSpline._eval_args / interp1d._spline.c; zeros for the linear kind, which holds
no spline); knot_off (n + 1,) CSR into knots (FITPACK's t / interp1d._spline.t; none for the linear kind); pt_off (n + 1,) CSR
into ru (the sample parameters) and rx, ry, ryaw, rk (what the reference returns; ryaw and rk are NaN for script 1, which
returns (x, y) only).
Degree 1 of script 0: the script's _evaluate_spline raises there (scipy refuses derivative(2) of a k = 1 spline), so x, y and
the heading are taken from the same UnivariateSpline objects directly and the curvature is recorded as 0.0.
Courses whose neighbouring chords differ by more than 1 : 20, or whose speed dx^2 + dy^2 at a sample falls below 1e-6 of its
mean, are rejected and drawn again: conditions on the inputs (ill-conditioning and cusps would inflate the measured gaps).
"""
import os
import sys
import warnings

import numpy as np
import scipy.interpolate as interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["bspline_path"] = "10_path_planning_00_bspline_path.py"
ref_loader.FILES["spline_2d"] = "10_path_planning_00_spline_2d.py"
GOLD = os.path.join(ROOT, "tests", "golden")
KIND = {1: "linear", 2: "quadratic", 3: "cubic"}
LINSPACE, ARANGE, EXPLICIT = 0, 1, 2
rejected = 0


def random_course(rs, n, scale, shift=0.0):
    """n waypoints, chords of about `scale`, headings that wander"""
    th = np.cumsum(rs.uniform(-1.0, 1.0, n)) + rs.uniform(0, 2 * np.pi)
    step = scale * rs.uniform(0.5, 1.5, n)
    x = np.cumsum(step * np.cos(th)) + rs.uniform(-5, 5) + shift
    y = np.cumsum(step * np.sin(th)) + rs.uniform(-5, 5) - shift
    return x.tolist(), y.tolist()


def bsp_record(ref, x, y, degree, mode, count, us):
    u = ref._calc_distance_vector(x, y)
    sx = interpolate.UnivariateSpline(u, x, k=degree, s=0.0)
    sy = interpolate.UnivariateSpline(u, y, k=degree, s=0.0)
    samples = np.linspace(0.0, u[-1], count) if mode == LINSPACE else np.asarray(us, dtype=np.float64)
    dx, dy = sx.derivative(1)(samples), sy.derivative(1)(samples)
    if degree == 1:
        rx, ry, ryaw, rk = np.array(sx(samples)), sy(samples), np.arctan2(dy, dx), np.zeros(len(samples))
    elif mode == LINSPACE:
        rx, ry, ryaw, rk = ref.interpolate_b_spline_path(x, y, count, degree)
    else:
        rx, ry, ryaw, rk = ref._evaluate_spline(samples, sx, sy)
    t, c, k = sx._eval_args
    assert k == degree and len(t) == len(x) + degree + 1
    return dict(wp_u=u, knots=t, cx=c[:len(x)], cy=sy._eval_args[1][:len(x)], ru=samples, rx=rx, ry=ry, ryaw=ryaw, rk=rk,
                speed=dx * dx + dy * dy)


def s2d_record(ref, x, y, degree, mode, ds, us):
    sp = ref.Spline2D(x, y, kind=KIND[degree])
    samples = np.arange(0, sp.s[-1], ds) if mode == ARANGE else np.asarray(us, dtype=np.float64)
    rx, ry = [], []
    for i_s in samples:   # the driver loop :51-54
        ix, iy = sp.calc_position(i_s)
        rx.append(float(ix))
        ry.append(float(iy))
    m = len(x)
    if degree == 1:
        knots, cx, cy = np.zeros(0), np.zeros(m), np.zeros(m)
        speed = np.ones(1)
    else:
        knots, cx, cy = sp.sx._spline.t, sp.sx._spline.c, sp.sy._spline.c
        dx, dy = sp.sx._spline.derivative(1)(samples), sp.sy._spline.derivative(1)(samples)
        speed = dx * dx + dy * dy
    nan = np.full(len(samples), np.nan)
    return dict(wp_u=np.asarray(sp.s, dtype=np.float64), knots=knots, cx=cx, cy=cy, ru=samples, rx=rx, ry=ry, ryaw=nan, rk=nan,
                speed=speed)


def accepted(x, y, rec):
    ch = np.hypot(np.diff(x), np.diff(y))
    if len(ch) > 1 and np.max(np.maximum(ch[1:] / ch[:-1], ch[:-1] / ch[1:])) > 20.0:
        return False
    return bool(np.min(rec["speed"]) >= 1.0e-6 * np.mean(rec["speed"]))


def main():
    global rejected
    os.makedirs(GOLD, exist_ok=True)
    bsp = ref_loader.load("bspline_path")
    s2d = ref_loader.load("spline_2d")
    rs = np.random.RandomState(519)
    scales, counts, steps = [0.3, 2.0, 10.0], [1, 2, 50, 257], [0.05, 0.1, 0.5]
    plan = []   # (script, degree, m or (x, y), scale, mode, count, ds, explicit)
    q = 0
    for k in range(1, 6):           # one polynomial piece, one interior knot, two
        for m in (k + 1, k + 2, k + 3):
            plan.append((0, k, m, scales[q % 3], LINSPACE, counts[q % 4], 0.0, False))
            q += 1
    for m, ks in ((8, (2, 5)), (20, (1, 4)), (64, (3, 2)), (65, (5, 4)), (200, (3, 5))):
        for k in ks:
            plan.append((0, k, m, scales[q % 3], LINSPACE, 50 if m < 200 else 257, 0.0, False))
            q += 1
    plan.append((0, 3, 12, 2.0, LINSPACE, 50, 0.0, "1e4"))
    plan.append((0, 3, ([-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0]), 0.0, LINSPACE, 50, 0.0, False))   # the driver :158-160
    for k in range(1, 6):           # samples as data: both ends, every interior knot, a few between
        plan.append((0, k, 9, 2.0, EXPLICIT, 0, 0.0, True))
    while len(plan) < 40:
        plan.append((0, int(rs.randint(1, 6)), int(rs.randint(6, 41)), scales[q % 3], LINSPACE, 50, 0.0, False))
        q += 1
    n_bsp = len(plan)
    q = 0
    for k in (1, 2, 3):
        for m in (k + 1, k + 2, k + 3):
            plan.append((1, k, m, scales[q % 3], ARANGE, 0, steps[q % 3], False))
            q += 1
    drv = ([-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0], [0.7, -6, -5, -3.5, 0.0, 5.0, -2.0])   # the driver :37-40
    for k in (1, 2, 3):
        plan.append((1, k, drv, 0.0, ARANGE, 0, 0.1, False))
    plan.append((1, 3, ([1.0, 1.3, 1.5, 1.9], [2.0, 2.1, 2.0, 2.2]), 0.0, ARANGE, 0, 5.0, False))   # ds > s[-1]: one point
    plan.append((1, 2, 12, 2.0, ARANGE, 0, 0.1, "1e4"))
    plan.append((1, 1, 64, 0.3, ARANGE, 0, 0.05, False))
    plan.append((1, 2, 65, 2.0, ARANGE, 0, 0.5, False))
    plan.append((1, 3, 200, 0.3, ARANGE, 0, 0.1, False))
    for k in (1, 2, 3):
        plan.append((1, k, 9, 2.0, EXPLICIT, 0, 0.0, True))
    while len(plan) < 65:
        plan.append((1, int(rs.randint(1, 4)), int(rs.randint(6, 41)), scales[q % 3], ARANGE, 0, steps[(q + 1) % 3], False))
        q += 1

    keys = ("wp_x", "wp_y", "wp_u", "cx", "cy", "knots", "ru", "rx", "ry", "ryaw", "rk")
    out = {k: [] for k in keys}
    meta = {k: [] for k in ("script", "degree", "mode", "count", "ds")}
    wp_off, knot_off, pt_off = [0], [0], [0]
    for script, k, shape, scale, mode, count, ds, special in plan:
        while True:
            if isinstance(shape, tuple):
                x, y = [float(v) for v in shape[0]], [float(v) for v in shape[1]]
            else:
                x, y = random_course(rs, shape, scale, 1.0e4 if special == "1e4" else 0.0)
            us = None
            if mode == EXPLICIT:    # the knots depend on the waypoints only: a first pass finds them
                first = (bsp_record(bsp, x, y, k, LINSPACE, 2, None) if script == 0 else s2d_record(s2d, x, y, max(k, 2), ARANGE, 1.0, None))
                t, end = first["knots"], float(first["wp_u"][-1])
                if script == 1 and k == 1:
                    t = np.concatenate([[0.0, 0.0], first["wp_u"][1:-1], [end, end]])
                inner = t[k + 1:len(x)]
                us = np.concatenate([[0.0, end], inner, rs.uniform(0.0, end, 6), 0.5 * (inner[:-1] + inner[1:])])
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                rec = bsp_record(bsp, x, y, k, mode, count, us) if script == 0 else s2d_record(s2d, x, y, k, mode, ds, us)
            if isinstance(shape, tuple) or accepted(x, y, rec):
                break
            rejected += 1
        out["wp_x"] += x
        out["wp_y"] += y
        for key in keys[2:]:
            out[key] += np.asarray(rec[key], dtype=np.float64).ravel().tolist()
        for key, v in zip(("script", "degree", "mode", "count", "ds"), (script, k, mode, count, ds)):
            meta[key].append(v)
        wp_off.append(wp_off[-1] + len(x))
        knot_off.append(knot_off[-1] + len(rec["knots"]))
        pt_off.append(pt_off[-1] + len(rec["ru"]))
    assert len(plan) == 65 and n_bsp == 40

    dst = os.path.join(GOLD, "bspline_kat.npz")
    np.savez_compressed(dst, wp_off=np.array(wp_off, dtype=np.int64), knot_off=np.array(knot_off, dtype=np.int64),
                        pt_off=np.array(pt_off, dtype=np.int64), script=np.array(meta["script"], dtype=np.int32),
                        degree=np.array(meta["degree"], dtype=np.int32), mode=np.array(meta["mode"], dtype=np.int32),
                        count=np.array(meta["count"], dtype=np.int64), ds=np.array(meta["ds"], dtype=np.float64),
                        **{k: np.array(v, dtype=np.float64) for k, v in out.items()})
    print("%d courses (%d bspline_path, %d spline_2d), %d waypoints, %d points, %d rejected and drawn again; %d bytes"
          % (len(plan), n_bsp, len(plan) - n_bsp, wp_off[-1], pt_off[-1], rejected, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
