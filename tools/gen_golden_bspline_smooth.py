"""Golden generator of BatchBSpline.approximate: runs the pieces of the reference's approximate_b_spline_path
(10_path_planning_00_bspline_path.py :12-56: _calc_distance_vector, UnivariateSpline(distances, x, k=degree, s=s) and the same
for y, _evaluate_spline), loaded through oracle/ref_loader.py, and writes tests/golden/bspline_smooth_kat.npz.  Build host only:
needs the reference checkout and scipy.

    python tools/gen_golden_bspline_smooth.py

Arrays only: inputs and recorded outputs.  Per course: degree, s (NaN where the script's default s=None was passed, meaning
the waypoint count), count (n_path_points), kinds (a comma-separated list of what the course is an example of); wp_off (n + 1,)
CSR into wp_x, wp_y.  Per axis a in (x, y): knot_off_a / coef_off_a (n + 1,) CSR into knots_a / coefs_a (UnivariateSpline.
_eval_args), fp_a (get_residual()), warned_a (whether scipy warned on the axis; always False in the file, see below).  pt_off
(n + 1,) CSR into rx, ry, ryaw, rk, the four arrays the script returns.
Degree 1: the script's _evaluate_spline raises there (scipy refuses derivative(2) of a k = 1 spline), so x, y and the heading
are taken from the same UnivariateSpline objects directly and the curvature is recorded as 0.0 (as tools/gen_golden_bspline.py).

The oracle (tests/bspline_smooth_oracle.py) runs beside scipy.  An axis is dropped -- and its course with it -- only if its knot
vector differs from scipy's or scipy warned on it; the number is printed, at most 2 % of the generated axes may be dropped, and
every kind of case listed in KINDS must survive.  Random courses whose neighbouring chords differ by more than 1 : 20, or
whose speed at a sample falls below 1e-6 of its mean, are drawn again: conditions on the inputs, as in gen_golden_bspline.py.
"""
import os
import sys
import warnings

import numpy as np
import scipy.interpolate as interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_loader  # noqa: E402
import bspline_oracle as B  # noqa: E402
import bspline_smooth_oracle as S  # noqa: E402

ref_loader.FILES["bspline_path"] = "10_path_planning_00_bspline_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")
KINDS = ("driver", "s_none", "deg1", "deg2", "deg3", "deg4", "deg5", "m=k+1", "m=k+2", "m=k+3", "axes_differ", "second_stage",
         "nplus>=4", "interp_knots_smoothed", "polynomial", "scale0.3", "scale2", "scale10", "near1e4", "m200")


def random_course(rs, n, scale, shift=0.0):
    """n waypoints, chords of about `scale`, a random-walk heading"""
    th = np.cumsum(rs.normal(0.0, 0.5, n)) + rs.uniform(0, 2 * np.pi)
    step = scale * rs.uniform(0.5, 1.5, n)
    x = np.cumsum(step * np.cos(th)) + rs.uniform(-5, 5) + shift
    y = np.cumsum(step * np.sin(th)) + rs.uniform(-5, 5) - shift
    return x.tolist(), y.tolist()


def record(ref, x, y, degree, s, count):
    u = ref._calc_distance_vector(x, y)
    spl, warned = [], []
    for a in (x, y):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            spl.append(interpolate.UnivariateSpline(u, a, k=degree, s=s))
        warned.append(len(w) > 0)
    samples = np.linspace(0.0, u[-1], count)
    dx, dy = spl[0].derivative(1)(samples), spl[1].derivative(1)(samples)
    if degree == 1:
        rx, ry, ryaw, rk = np.array(spl[0](samples)), spl[1](samples), np.arctan2(dy, dx), np.zeros(count)
    else:
        rx, ry, ryaw, rk = ref._evaluate_spline(samples, spl[0], spl[1])
    axes = []
    for sp in spl:
        t, c, k = sp._eval_args
        assert k == degree
        axes.append(dict(t=np.array(t), c=np.array(c[:len(t) - k - 1]), fp=float(sp.get_residual())))
    return dict(axes=axes, warned=warned, rx=rx, ry=ry, ryaw=ryaw, rk=rk, speed=dx * dx + dy * dy)


def accepted(x, y, rec):
    ch = np.hypot(np.diff(x), np.diff(y))
    if len(ch) > 1 and np.max(np.maximum(ch[1:] / ch[:-1], ch[:-1] / ch[1:])) > 20.0:
        return False
    return bool(np.min(rec["speed"]) >= 1.0e-6 * np.mean(rec["speed"]))


def main():
    os.makedirs(GOLD, exist_ok=True)
    ref = ref_loader.load("bspline_path")
    rs = np.random.RandomState(521)
    scales = [0.3, 2.0, 10.0]
    drv = ([-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0])      # the driver :158-160
    plan = [(3, drv, 0.0, 0.5, 50, "driver"), (3, drv, 0.0, None, 50, "")]   # (degree, m or (x, y), scale, s, count, label)
    q = 0
    for k in range(1, 6):
        for j, m in enumerate((k + 1, k + 2, k + 3)):
            plan.append((k, m, scales[q % 3], [0.05, None, 0.01][(q + k) % 3], [50, 2, 1, 37][q % 4], "m=k+%d" % (j + 1)))
            q += 1
    for k in range(1, 6):                       # small s on a middle-sized course: past the m // 2 stage
        plan.append((k, 24 + 3 * k, scales[k % 3], 0.002, 50, ""))
    for k in range(1, 6):                       # s so small that the knots end as the interpolation knots, then smoothed
        plan.append((k, 10 + k, 2.0, 1.0e-7, 50, ""))
    for k in range(1, 6):                       # s so large that the polynomial is accepted
        plan.append((k, 15, 0.3, 50.0, 50, ""))
    plan.append((3, 200, 2.0, 0.5, 257, "m200"))
    plan.append((5, 200, 0.3, None, 257, "m200"))
    plan.append((2, 120, 10.0, 5.0, 100, ""))
    plan.append((3, 12, 2.0, 0.5, 50, "near1e4"))
    plan.append((4, 40, 2.0, 0.05, 50, "near1e4"))
    while len(plan) < 72:
        m = int(rs.randint(6, 60))
        plan.append((int(rs.randint(1, 6)), m, scales[q % 3], [None, 0.5, 0.05 * m, 2.0, 0.01][q % 5], 50, ""))
        q += 1

    flat = {key: [] for key in ("wp_x", "wp_y", "rx", "ry", "ryaw", "rk", "knots_x", "knots_y", "coefs_x", "coefs_y")}
    meta = {key: [] for key in ("degree", "s", "count", "kinds", "fp_x", "fp_y", "warned_x", "warned_y")}
    offs = {key: [0] for key in ("wp_off", "pt_off", "knot_off_x", "knot_off_y", "coef_off_x", "coef_off_y")}
    axes_made = axes_dropped = redrawn = 0
    for k, shape, scale, s, count, label in plan:
        while True:
            if isinstance(shape, tuple):
                x, y = [float(v) for v in shape[0]], [float(v) for v in shape[1]]
            else:
                x, y = random_course(rs, shape, scale, 1.0e4 if label == "near1e4" else 0.0)
            rec = record(ref, x, y, k, s, count)
            if isinstance(shape, tuple) or accepted(x, y, rec):
                break
            redrawn += 1
        m = len(x)
        u = B.parameter(x, y, B.NORMALISED)
        sv = float(m) if s is None else float(s)
        kinds = {label, "deg%d" % k} - {""}
        if s is None:
            kinds.add("s_none")
        if not isinstance(shape, tuple):
            kinds.add("scale%g" % scale)
        drop = 0
        mine = []
        for a, vals in enumerate((x, y)):
            trace = []
            r = S.fit(u, vals, k, sv, trace)
            mine.append(r)
            axes_made += 1
            t = rec["axes"][a]["t"]
            if rec["warned"][a] or len(t) != r["n"] or not np.array_equal(np.array(r["t"]), t):
                drop += 1
                continue
            if r["n"] > max(m // 2, 2 * k + 2):
                kinds.add("second_stage")
            if trace and max(trace) >= 4:
                kinds.add("nplus>=4")
            if r["n"] == m + k + 1 and r["ier"] == 0 and r["iters"] > 0:
                kinds.add("interp_knots_smoothed")
            if r["ier"] == -2 and m > k + 1:
                kinds.add("polynomial")
        if drop:
            axes_dropped += drop
            print("dropped: degree %d, m %d, s %r (%d axes)" % (k, m, s, drop))
            continue
        if mine[0]["n"] != mine[1]["n"]:
            kinds.add("axes_differ")
        flat["wp_x"] += x
        flat["wp_y"] += y
        for key in ("rx", "ry", "ryaw", "rk"):
            flat[key] += np.asarray(rec[key], dtype=np.float64).ravel().tolist()
        for a, name in enumerate("xy"):
            flat["knots_" + name] += rec["axes"][a]["t"].tolist()
            flat["coefs_" + name] += rec["axes"][a]["c"].tolist()
            offs["knot_off_" + name].append(len(flat["knots_" + name]))
            offs["coef_off_" + name].append(len(flat["coefs_" + name]))
            meta["fp_" + name].append(rec["axes"][a]["fp"])
            meta["warned_" + name].append(rec["warned"][a])
        offs["wp_off"].append(len(flat["wp_x"]))
        offs["pt_off"].append(len(flat["rx"]))
        meta["degree"].append(k)
        meta["s"].append(np.nan if s is None else s)
        meta["count"].append(count)
        meta["kinds"].append(",".join(sorted(kinds)))

    seen = set(",".join(meta["kinds"]).split(","))
    missing = [name for name in KINDS if name not in seen]
    assert not missing, "kinds without a surviving course: %s" % missing
    assert axes_dropped <= 0.02 * axes_made, "%d of %d axes dropped: more than 2 %%" % (axes_dropped, axes_made)
    assert max(np.diff(offs["wp_off"])) == 200
    dst = os.path.join(GOLD, "bspline_smooth_kat.npz")
    np.savez_compressed(dst, degree=np.array(meta["degree"], dtype=np.int32), s=np.array(meta["s"], dtype=np.float64),
                        count=np.array(meta["count"], dtype=np.int64), kinds=np.array(meta["kinds"]),
                        fp_x=np.array(meta["fp_x"]), fp_y=np.array(meta["fp_y"]), warned_x=np.array(meta["warned_x"], dtype=bool),
                        warned_y=np.array(meta["warned_y"], dtype=bool),
                        **{key: np.array(v, dtype=np.int64) for key, v in offs.items()},
                        **{key: np.array(v, dtype=np.float64) for key, v in flat.items()})
    print("%d courses, %d axes generated, %d dropped (%.2f %%), %d courses drawn again; %d waypoints, %d points; %d bytes"
          % (len(meta["degree"]), axes_made, axes_dropped, 100.0 * axes_dropped / axes_made, redrawn, offs["wp_off"][-1],
             offs["pt_off"][-1], os.path.getsize(dst)))
    for name in KINDS:
        print("  %-22s %d courses" % (name, sum(name in v.split(",") for v in meta["kinds"])))


if __name__ == "__main__":
    main()
