"""Golden generator of BatchSteer("bezier"): runs the reference's own functions of 10_path_planning_00_bazier_path.py
(calc_4points_bezier_path, calc_bezier_path, bezier_derivatives_control_points, bezier, curvature) and rrt_05's
check_collision, loaded through oracle/ref_loader.py (the file name is added to ref_loader.FILES at run time), and writes
tests/golden/bezier_kat.npz.  Build host only (needs the reference checkout, and the scipy the script imports).

    python tools/gen_golden_bezier.py

Arrays only.  Curves are numbered pose cases first, then control-point cases.
Pose cases: pose (np, 7) rows (sx, sy, syaw, ex, ey, eyaw, offset), pose_cp (np, 4, 2) the reference's control points.
Control-point cases: cp_off (nc + 1,) CSR into cp_xy (rows x, y).
Per curve: n_points (n,), pt_off (n + 1,) CSR into x, y (the path), dx, dy, ddx, ddy (bezier on the derivative control
points) and k (curvature), tag (n,) what the curve is for (TAGS below).
Hit sets: three obstacle lists obs_first, obs_last, obs_none (rows x, y, size), rr the robot_radius, and for every curve
hit_first, hit_last, hit_none: the first circle of the list that any of the reference's points touches by
check_collision, else -1.  lone = (curve A, curve B, circle): the circle of that index in obs_first touches curve A at its
first point only, in obs_last curve B at its last point only, and no earlier circle touches either.
"""
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["bazier_path"] = "10_path_planning_00_bazier_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("driver", "random", "n_points", "same_pose", "axis_yaw", "negative_offset", "far", "signed_zero", "collinear",
        "degree")
N_RANDOM = 85


def main():
    os.makedirs(GOLD, exist_ok=True)
    ref = ref_loader.load("bazier_path")
    m5 = ref_loader.load("rrt_05")
    rs = np.random.RandomState(1962)
    poses = []   # (7 floats, n_points, tag)

    def rand_pose_pair(lo=0.0, hi=20.0):
        return [float(rs.uniform(lo, hi)), float(rs.uniform(lo, hi)), float(rs.uniform(-math.pi, math.pi)),
                float(rs.uniform(lo, hi)), float(rs.uniform(lo, hi)), float(rs.uniform(-math.pi, math.pi)),
                float(rs.uniform(1.0, 5.0))]

    for off in np.arange(1.0, 5.0, 1.0):   # the script's driver pair and its offsets
        poses.append(([10.0, 1.0, float(np.radians(180.0)), -0.0, -3.0, float(np.radians(-45.0)), float(off)], 100, "driver"))
    for _ in range(N_RANDOM):
        poses.append((rand_pose_pair(), 100, "random"))
    for n in (2, 3, 17, 64, 65, 257):
        for _ in range(2):
            poses.append((rand_pose_pair(), n, "n_points"))
    poses.append(([3.0, 4.0, 0.7, 3.0, 4.0, 0.7, 3.0], 100, "same_pose"))   # every control point the same: k is NaN
    for a, b in ((0.0, math.pi), (-math.pi, math.pi / 2), (-math.pi / 2, 0.0), (math.pi / 2, -math.pi), (math.pi, -math.pi / 2)):
        p = rand_pose_pair()
        p[2], p[5] = a, b
        poses.append((p, 100, "axis_yaw"))
    p = rand_pose_pair()
    p[6] = -2.5
    poses.append((p, 100, "negative_offset"))
    p = rand_pose_pair()
    poses.append(([p[0] + 1.0e4, p[1] - 1.0e4, p[2], p[3] + 1.0e4, p[4] - 1.0e4, p[5], p[6]], 100, "far"))
    # y = -0.0 at every control point (sin(-0.0) = -0.0) and x starts at 0.0: np.sum starts from 0.0, so every y of the
    # reference's path is +0.0 (a sum that began with its first product would give -0.0)
    poses.append(([0.0, -0.0, -0.0, 5.0, -0.0, 0.0, 3.0], 100, "signed_zero"))
    poses.append(([1.0, 1.0, math.atan2(1.0, 2.0), 9.0, 5.0, math.atan2(1.0, 2.0), 3.0], 100, "collinear"))

    cps = []   # (array (m, 2), n_points, tag)
    cps.append((np.array([[0.0, 0.0], [1.0, 0.5], [3.0, 1.5], [4.0, 2.0]]), 100, "collinear"))   # exactly on a line: k = 0
    for m in (3, 4, 8, 16):
        for n in (2, 33, 300):
            th = np.cumsum(rs.uniform(-0.9, 0.9, m)) + rs.uniform(0, 2 * np.pi)
            step = rs.uniform(0.5, 3.0, m)
            pts = np.stack([np.cumsum(step * np.cos(th)) + rs.uniform(0, 20), np.cumsum(step * np.sin(th)) + rs.uniform(0, 20)], axis=1)
            cps.append((pts, n, "degree"))

    out = {k: [] for k in ("x", "y", "dx", "dy", "ddx", "ddy", "k")}
    pt_off, n_points, tags, pose_cp, per_curve = [0], [], [], [], []

    def record(cp, n, tag, path):
        assert path.shape == (n, 2)
        w = ref.bezier_derivatives_control_points(cp, 2)
        with np.errstate(all="ignore"):
            for t in np.linspace(0, 1, n):
                d = ref.bezier(t, w[1])
                dd = ref.bezier(t, w[2])
                out["dx"].append(float(d[0])); out["dy"].append(float(d[1]))
                out["ddx"].append(float(dd[0])); out["ddy"].append(float(dd[1]))
                out["k"].append(float(ref.curvature(d[0], d[1], dd[0], dd[1])))
        out["x"] += [float(v) for v in path[:, 0]]
        out["y"] += [float(v) for v in path[:, 1]]
        pt_off.append(pt_off[-1] + n)
        n_points.append(n)
        tags.append(TAGS.index(tag))
        per_curve.append(([float(v) for v in path[:, 0]], [float(v) for v in path[:, 1]]))

    for p, n, tag in poses:
        path, cp = ref.calc_4points_bezier_path(*p)   # the reference's path has 100 points, whatever n
        if n != 100:
            path = ref.calc_bezier_path(cp, n_points=n)
        pose_cp.append(np.array(cp, dtype=np.float64))
        record(cp, n, tag, path)
    cp_off = [0]
    for cp, n, tag in cps:
        record(cp, n, tag, ref.calc_bezier_path(cp, n_points=n))
        cp_off.append(cp_off[-1] + len(cp))
    for i, (p, n, tag) in enumerate(poses):   # the script's own asserts
        a = pt_off[i]
        if tag == "driver":
            assert out["x"][a] == p[0] and out["y"][a] == p[1] and out["x"][a + n - 1] == p[3] and out["y"][a + n - 1] == p[4]
    i0 = [i for i, q in enumerate(poses) if q[2] == "signed_zero"][0]
    ys = np.array(out["y"][pt_off[i0]:pt_off[i0 + 1]])
    assert np.all(ys == 0.0) and not np.any(np.signbit(ys)) and np.all(np.signbit(np.array(pose_cp[i0])[:, 1]))
    i1 = [i for i, q in enumerate(poses) if q[2] == "same_pose"][0]
    assert np.all(np.isnan(out["k"][pt_off[i1]:pt_off[i1 + 1]]))
    ic = len(poses)   # the collinear control-point set
    assert not np.any(np.array(out["k"][pt_off[ic]:pt_off[ic + 1]]))

    # hit sets
    rr = 0.2

    def hits(ci, circles):
        node = types.SimpleNamespace(path_x=per_curve[ci][0], path_y=per_curve[ci][1])
        for j, o in enumerate(circles):
            if not m5.RRT.check_collision(node, [tuple(float(v) for v in o)], rr):
                return j
        return -1

    def touched(ci, o):
        xs, ys_ = per_curve[ci]
        return [q for q in range(len(xs)) if (o[0] - xs[q]) ** 2 + (o[1] - ys_[q]) ** 2 <= (o[2] + rr) ** 2]

    n_curves = len(per_curve)
    field = [i for i in range(n_curves) if tags[i] in (TAGS.index("random"), TAGS.index("n_points"), TAGS.index("degree"))]
    none = []
    while len(none) < 8:   # circles near the curves that touch none of them
        o = (float(rs.uniform(0, 20)), float(rs.uniform(0, 20)), float(rs.uniform(0.05, 0.4)))
        if all(hits(ci, [o]) == -1 for ci in range(n_curves)):
            none.append(o)
    rand = [(float(rs.uniform(2, 18)), float(rs.uniform(2, 18)), float(rs.uniform(0.3, 0.9))) for _ in range(10)]

    def lone_circle(ci, q, q_next):
        """A circle behind point q of curve ci (away from q_next) that reaches q and no other point of the curve"""
        xs, ys_ = per_curve[ci]
        tx, ty = xs[q] - xs[q_next], ys_[q] - ys_[q_next]
        nrm = math.hypot(tx, ty)
        ox, oy = xs[q] + 0.5 * tx / nrm, ys_[q] + 0.5 * ty / nrm
        d = np.sort(np.hypot(np.array(xs) - ox, np.array(ys_) - oy))
        o = (ox, oy, 0.5 * (d[0] + d[1]) - rr)
        assert touched(ci, o) == [q], (ci, touched(ci, o))
        return o

    A = B = None
    for ci in field:   # two curves of 100 points that no decoy circle touches
        if n_points[ci] == 100 and hits(ci, none[:2]) == -1:
            if A is None:
                A = ci
            elif B is None:
                B = ci
    assert A is not None and B is not None
    obs_first = none[:2] + [lone_circle(A, 0, 1)] + rand
    obs_last = none[2:4] + [lone_circle(B, 99, 98)] + rand
    obs_none = none
    hit = {}
    for name, lst in (("first", obs_first), ("last", obs_last), ("none", obs_none)):
        hit[name] = np.array([hits(ci, lst) for ci in range(n_curves)], dtype=np.int32)
    assert hit["first"][A] == 2 and hit["last"][B] == 2 and not np.any(hit["none"] != -1)
    for name in ("first", "last"):
        h = hit[name]
        assert np.sum(h == -1) >= 10 and np.sum(h > 2) >= 10, (name, h.tolist())

    dst = os.path.join(GOLD, "bezier_kat.npz")
    np.savez_compressed(
        dst, pose=np.array([p for p, _, _ in poses], dtype=np.float64), pose_cp=np.array(pose_cp),
        cp_off=np.array(cp_off, dtype=np.int64), cp_xy=np.concatenate([c for c, _, _ in cps]).astype(np.float64),
        n_points=np.array(n_points, dtype=np.int32), pt_off=np.array(pt_off, dtype=np.int64),
        tag=np.array(tags, dtype=np.int32), obs_first=np.array(obs_first), obs_last=np.array(obs_last),
        obs_none=np.array(obs_none), rr=np.array(rr), hit_first=hit["first"], hit_last=hit["last"], hit_none=hit["none"],
        lone=np.array([A, B, 2], dtype=np.int32), **{k: np.array(v, dtype=np.float64) for k, v in out.items()})
    print("%d pose curves, %d control-point curves, %d points; hit_first %d free, hit_last %d free; %d bytes"
          % (len(poses), len(cps), pt_off[-1], int(np.sum(hit["first"] == -1)), int(np.sum(hit["last"] == -1)),
             os.path.getsize(dst)))


if __name__ == "__main__":
    main()
