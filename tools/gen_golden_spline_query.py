"""Golden generator of BatchSpline.query / fit1d: runs the pointwise methods of the reference's CubicSpline2D and CubicSpline1D
(10_path_planning_00_cubic_spline_path.py :75-140, :248-310), loaded through oracle/ref_loader.py (the file name is added to
ref_loader.FILES at run time), and writes tests/golden/spline_query_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_spline_query.py

Arrays only.
2-D: wp_off (n + 1,) CSR into wp_x, wp_y (the waypoints) and cx, cy (the reference's sx.c, sy.c); q_off (n + 1,) CSR into
q_t (the parameters), q_status (0 answered, 1 calc_position returned (None, None), 2 it raised IndexError) and the answers
rx, ry (calc_position), ryaw (calc_yaw), rk (calc_curvature), rdx, rdy, rddx, rddy (sx / sy.calc_first_derivative,
calc_second_derivative); NaN where the status is not 0.
1-D: k_off CSR into knots, values and c1 (the reference's c); p_off CSR into p_t, p_status, p_y, p_dy, p_ddy.  drv_t, drv_y:
the first driver cell of the script, calc_position of the first spline on np.linspace(0.0, 5.0) (None is NaN).
Per spline the parameters are 0.0, -0.0, every knot and its two neighbours (nextafter), -1e-300, +-inf, NaN and 60 uniform
draws between the first and the last knot.
Prints the gap of the Thomas recurrence (tests/spline_query_oracle.py) to these answers: tests/spline_query_util.py holds 16 x.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_loader  # noqa: E402
from gen_golden_spline import random_course  # noqa: E402

ref_loader.FILES["cubic_spline_path"] = "10_path_planning_00_cubic_spline_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")


def parameters(rs, s):
    """The query list of one spline over the knots s"""
    s = np.asarray(s, dtype=np.float64)
    t = [0.0, -0.0]
    for v in s:
        t += [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]
    t += [-1e-300, float("inf"), float("-inf"), float("nan")]
    t += rs.uniform(s[0], s[-1], 60).tolist()
    return t


def ask(fn, t):
    """(status, value) of one reference method at t: None is 1, IndexError is 2"""
    try:
        v = fn(t)
    except IndexError as e:
        assert str(e) == "list index out of range"
        return 2, None
    return (1, None) if v is None or (isinstance(v, tuple) and v[0] is None) else (0, v)


def main():
    ref = ref_loader.load("cubic_spline_path")
    rs = np.random.RandomState(1914)
    courses = []
    for n, scale in ((2, 2.0), (3, 0.3), (5, 2.0), (12, 10.0), (40, 2.0)):
        courses.append(random_course(rs, n, scale))
    courses.append(([-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0], [0.7, -6, 5, 6.5, 0.0, 5.0, -2.0]))   # the docstring's seven
    x, y = random_course(rs, 12, 2.0)
    courses.append(([v + 1.0e4 for v in x], [v - 1.0e4 for v in y]))                               # near 1e4
    courses.append(([-0.0, 1.0, 2.5, 3.0], [0.0, 0.5, -0.5, 1.0]))                                # first waypoint (-0.0, 0.0)
    courses.append(([0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0]))                                  # knots on integers
    courses.append(random_course(rs, 7, 0.05))                                                     # short chords

    d2 = {k: [] for k in ("wp_x", "wp_y", "cx", "cy", "q_t", "q_status", "rx", "ry", "ryaw", "rk", "rdx", "rdy", "rddx", "rddy")}
    wp_off, q_off = [0], [0]
    nan = float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for x, y in courses:
            sp = ref.CubicSpline2D(x, y)
            d2["wp_x"] += [float(v) for v in x]
            d2["wp_y"] += [float(v) for v in y]
            d2["cx"] += [float(v) for v in sp.sx.c]
            d2["cy"] += [float(v) for v in sp.sy.c]
            ts = parameters(rs, sp.s)
            for t in ts:
                t = np.float64(t)
                st, pos = ask(sp.calc_position, t)
                d2["q_t"].append(float(t))
                d2["q_status"].append(st)
                if st == 0:
                    vals = [pos[0], pos[1], sp.calc_yaw(t), sp.calc_curvature(t), sp.sx.calc_first_derivative(t),
                            sp.sy.calc_first_derivative(t), sp.sx.calc_second_derivative(t), sp.sy.calc_second_derivative(t)]
                else:
                    # the other five methods fail the same way
                    for fn in (sp.sx.calc_first_derivative, sp.sy.calc_first_derivative, sp.sx.calc_second_derivative,
                               sp.sy.calc_second_derivative):
                        assert ask(fn, t)[0] == st
                    for fn in (sp.calc_yaw, sp.calc_curvature):
                        try:
                            fn(t)
                            raise AssertionError("the reference answered")
                        except (TypeError if st == 1 else IndexError):
                            pass
                    vals = [nan] * 8
                for key, v in zip(("rx", "ry", "ryaw", "rk", "rdx", "rdy", "rddx", "rddy"), vals):
                    d2[key].append(float(v))
            wp_off.append(wp_off[-1] + len(x))
            q_off.append(q_off[-1] + len(ts))

    splines = [(np.arange(5), [1.7, -6, 5, 6.5, 0.0]),                                       # the driver cell's
               ([0.0, 0.1, 0.5, 2.75, 3.0, 7.0, 7.125], [1.0, -1.0, 0.25, 4.0, 3.5, -2.0, 0.0]),   # uneven knots
               ([-3.5, -2.0, -0.5, 0.25, 1.0], [0.5, 2.0, -1.0, 0.0, 3.0]),                  # negative knots
               ([1.0, 4.0], [2.0, -1.0])]                                                    # two knots
    d1 = {k: [] for k in ("knots", "values", "c1", "p_t", "p_status", "p_y", "p_dy", "p_ddy")}
    k_off, p_off = [0], [0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for kn, va in splines:
            sp = ref.CubicSpline1D(kn, va)
            d1["knots"] += [float(v) for v in kn]
            d1["values"] += [float(v) for v in va]
            d1["c1"] += [float(v) for v in sp.c]
            ts = parameters(rs, kn)
            for t in ts:
                t = np.float64(t)
                got = [ask(fn, t) for fn in (sp.calc_position, sp.calc_first_derivative, sp.calc_second_derivative)]
                assert len({g[0] for g in got}) == 1
                d1["p_t"].append(float(t))
                d1["p_status"].append(got[0][0])
                for key, g in zip(("p_y", "p_dy", "p_ddy"), got):
                    d1[key].append(nan if g[0] else float(g[1]))
            k_off.append(k_off[-1] + len(kn))
            p_off.append(p_off[-1] + len(ts))

    # the script's first driver cell: the arange(5) spline on np.linspace(0.0, 5.0), None (NaN here) beyond the last knot
    sp = ref.CubicSpline1D(*splines[0])
    drv_t = np.linspace(0.0, 5.0)
    drv = [sp.calc_position(t) for t in drv_t]
    assert drv[-1] is None and drv[0] is not None
    d1["drv_t"] = drv_t.tolist()
    d1["drv_y"] = [nan if v is None else float(v) for v in drv]

    ints = ("q_status", "p_status")
    arrays = {k: np.array(v, dtype=np.int32 if k in ints else np.float64) for k, v in list(d2.items()) + list(d1.items())}
    arrays.update(wp_off=np.array(wp_off, dtype=np.int64), q_off=np.array(q_off, dtype=np.int64),
                  k_off=np.array(k_off, dtype=np.int64), p_off=np.array(p_off, dtype=np.int64))
    for st in (0, 1, 2):
        assert st in arrays["q_status"] and st in arrays["p_status"]
    dst = os.path.join(GOLD, "spline_query_kat.npz")
    np.savez_compressed(dst, **arrays)
    print("%d courses, %d queries; %d splines, %d queries; %d bytes"
          % (len(courses), q_off[-1], len(splines), p_off[-1], os.path.getsize(dst)))

    import spline_query_util as U
    print("gaps of the Thomas recurrence: position %.3e yaw %.3e k %.3e first %.3e second %.3e" % U.gaps_of_thomas())


if __name__ == "__main__":
    main()
