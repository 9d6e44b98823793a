"""Golden generator of BatchSpline: runs the reference's calc_spline_course (10_path_planning_00_cubic_spline_path.py) and
rrt_05's check_collision, loaded through oracle/ref_loader.py (the file name is added to ref_loader.FILES at run time),
and writes tests/golden/spline_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_spline.py

Arrays only.
Courses: wp_off (n + 1,) CSR into wp_x, wp_y (the waypoints) and into cx, cy (the reference's sx.c and sy.c); ds (n,);
pt_off (n + 1,) CSR into rx, ry, ryaw, rk, s (what calc_spline_course returns, concatenated); length (n,) sp.s[-1].
Hit set: hit_courses (m,) indices into the courses, obs (24, 3) circles, rr the robot_radius, hit (m,): the first circle
of the list that any of the reference's points touches by check_collision, else -1.
"""
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["cubic_spline_path"] = "10_path_planning_00_cubic_spline_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")


def random_course(rs, n, scale):
    """n waypoints, chords of about `scale`, headings that wander"""
    th = np.cumsum(rs.uniform(-1.2, 1.2, n))
    step = scale * rs.uniform(0.4, 1.6, n)
    x = np.cumsum(step * np.cos(th)) + rs.uniform(-5, 5)
    y = np.cumsum(step * np.sin(th)) + rs.uniform(-5, 5)
    return x.tolist(), y.tolist()


def main():
    os.makedirs(GOLD, exist_ok=True)
    ref = ref_loader.load("cubic_spline_path")
    m5 = ref_loader.load("rrt_05")
    rs = np.random.RandomState(514)
    courses = []   # (x, y, ds)
    ds_cycle = [0.05, 0.1, 0.5]
    k = 0
    for n in (2, 3, 4, 5, 64, 65, 200):
        for scale in (0.3, 2.0, 10.0):
            if n == 200 and scale == 10.0:
                ds = 0.5   # 2000 m of course: keep the file small
            else:
                ds = ds_cycle[k % 3]
            k += 1
            x, y = random_course(rs, n, scale)
            courses.append((x, y, ds))
    # sample parameters on the knots, s[-1] / ds an integer: arange drops the stop
    courses.append(([0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0], 0.5))
    # ds > s[-1]: one point
    courses.append(([1.0, 1.3, 1.5], [2.0, 2.1, 2.0], 5.0))
    # coordinates near 1e4
    x, y = random_course(rs, 12, 2.0)
    courses.append(([v + 1.0e4 for v in x], [v - 1.0e4 for v in y], 0.1))
    # the reference docstring's seven waypoints
    courses.append(([-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0], [0.7, -6, 5, 6.5, 0.0, 5.0, -2.0], 0.1))
    # the hit set: about 40 short courses in a 20 x 20 field
    first_hit_course = len(courses)
    for i in range(40):
        n = int(rs.randint(3, 9))
        th = np.cumsum(rs.uniform(-0.8, 0.8, n)) + rs.uniform(0, 2 * np.pi)
        step = rs.uniform(1.0, 2.5, n)
        x = np.cumsum(step * np.cos(th)) + rs.uniform(4, 16)
        y = np.cumsum(step * np.sin(th)) + rs.uniform(4, 16)
        courses.append((x.tolist(), y.tolist(), [0.1, 0.2, 0.25][i % 3]))

    wp_off, pt_off = [0], [0]
    out = {k: [] for k in ("wp_x", "wp_y", "cx", "cy", "rx", "ry", "ryaw", "rk", "s", "length", "ds")}
    per_course = []
    for x, y, ds in courses:
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # a division by zero would be garbage: no such course belongs here
            sp = ref.CubicSpline2D(x, y)
            rx, ry, ryaw, rk, s = ref.calc_spline_course(x, y, ds)
        assert len(sp.sx.c) == len(x) and len(rx) == len(s) == len(ryaw) == len(rk)
        out["wp_x"] += [float(v) for v in x]
        out["wp_y"] += [float(v) for v in y]
        out["cx"] += [float(v) for v in sp.sx.c]
        out["cy"] += [float(v) for v in sp.sy.c]
        for key, v in (("rx", rx), ("ry", ry), ("ryaw", ryaw), ("rk", rk), ("s", s)):
            out[key] += [float(q) for q in v]
        out["length"].append(float(sp.s[-1]))
        out["ds"].append(float(ds))
        wp_off.append(wp_off[-1] + len(x))
        pt_off.append(pt_off[-1] + len(s))
        per_course.append((rx, ry))
    i_col = [i for i, c in enumerate(courses) if c[0] == [0.0, 1.0, 2.0, 3.0]][0]
    assert pt_off[i_col + 1] - pt_off[i_col] == 6, "arange keeps the stop on the collinear course"

    # hit set
    hit_courses = list(range(first_hit_course, len(courses)))
    obs = np.stack([rs.uniform(2, 18, 24), rs.uniform(2, 18, 24), rs.uniform(0.3, 0.9, 24)], axis=1)
    rr = 0.2
    # one course that only the last circle touches, and only at a single point: the circle sits beside one sample of a
    # course that is free of the other 23, with a radius that reaches that sample and not its neighbours
    def hits(rx, ry, circles):
        node = types.SimpleNamespace(path_x=list(rx), path_y=list(ry))
        for j, o in enumerate(circles):
            if not m5.RRT.check_collision(node, [tuple(float(v) for v in o)], rr):
                return j
        return -1
    lone = None
    for ci in hit_courses:
        rx, ry = per_course[ci]
        if hits(rx, ry, obs[:23]) == -1 and len(rx) > 20:
            lone = ci
            break
    assert lone is not None
    rx, ry = per_course[lone]
    j = len(rx) // 2
    tx, ty = rx[j + 1] - rx[j - 1], ry[j + 1] - ry[j - 1]
    nrm = float(np.hypot(tx, ty))
    nx, ny = -ty / nrm, tx / nrm
    gap = 1.0
    ox, oy = rx[j] + gap * nx, ry[j] + gap * ny
    d = np.hypot(np.array(rx) - ox, np.array(ry) - oy)
    order = np.sort(d)
    assert int(np.argmin(d)) == j and order[1] > order[0]
    reach = 0.5 * (order[0] + order[1])   # between the nearest sample and the second nearest
    obs[23] = (ox, oy, reach - rr)
    touched = [q for q in range(len(rx)) if (ox - rx[q]) ** 2 + (oy - ry[q]) ** 2 <= (obs[23][2] + rr) ** 2]
    assert touched == [j], touched
    hit = np.array([hits(*per_course[ci], obs) for ci in hit_courses], dtype=np.int32)
    assert hit[hit_courses.index(lone)] == 23
    assert np.sum(hit >= 0) >= 10 and np.sum(hit == -1) >= 10 and np.sum(hit > 0) >= 3, hit.tolist()

    dst = os.path.join(GOLD, "spline_kat.npz")
    np.savez_compressed(dst, wp_off=np.array(wp_off, dtype=np.int64), pt_off=np.array(pt_off, dtype=np.int64),
                        hit_courses=np.array(hit_courses, dtype=np.int32), obs=obs, rr=np.array(rr), hit=hit,
                        lone=np.array([lone, j], dtype=np.int32),
                        **{k: np.array(v, dtype=np.float64) for k, v in out.items()})
    print("%d courses, %d waypoints, %d points; %d hit, %d free, %d with hit > 0; %d bytes"
          % (len(courses), wp_off[-1], pt_off[-1], int(np.sum(hit >= 0)), int(np.sum(hit == -1)), int(np.sum(hit > 0)),
             os.path.getsize(dst)))


if __name__ == "__main__":
    main()
