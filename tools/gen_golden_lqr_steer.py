"""Golden generator of BatchSteer("lqr"): runs the reference's stand-alone LQRPlanner (10_path_planning_00_lqr_path.py)
and rrt_09's sample_path / check_collision, all loaded through oracle/ref_loader.py (the two file names are added to
ref_loader.FILES at run time), and writes tests/golden/lqr_steer_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_lqr_steer.py

Arrays only.
(a) a_pairs (n, 4) rows (sx, sy, gx, gy) with magnitudes from 1e-3 to 1e6, some with start == goal; a_n (n,) len(rx);
    a_rx, a_ry the rollouts of LQRPlanner.lqr_planning, concatenated.  Each rollout is also made with rrt_09's copy of
    the class; the generator stops if the two differ in any bit.
(b) b_pairs (3, 4); b_ctl (6, 2) rows (MAX_TIME, GOAL_DIST); b_n (6, 3) len(rx) per control row and pair; b_rx, b_ry the
    rollouts, concatenated in that order.
(c) c_pairs (m, 4), c_step (m,); c_obs (24, 3) circles, c_rr the robot_radius; c_hit (m,): -1 where rrt_09's
    check_collision returns True for every single-circle list, else the first circle for which it returns False.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["lqr_path"] = "10_path_planning_00_lqr_path.py"
ref_loader.FILES["rrt_09"] = "10_path_planning_01_rrt_09_lqr_rrt_star.py"
GOLD = os.path.join(ROOT, "tests", "golden")

B_PAIRS = [(6.0, 6.0, -50.0, 70.0), (0.0, 0.0, 0.0, 0.0), (1e6, -1e6, -1e6, 1e6)]
B_CTL = [(0.25, 0.1), (0.0, 0.1), (100.0, 0.0), (100.0, 1e-9), (100.0, 5.0), (100.0, -1.0)]
B_EXPECT = [[0, 2, 0], [0, 2, 0], [19, 2, 19], [14, 2, 18], [4, 2, 8], [0, 0, 0]]   # measured when the issue was written


def rollout(planner, pair):
    with contextlib.redirect_stdout(io.StringIO()):
        rx, ry = planner.lqr_planning(*[float(v) for v in pair], show_animation=False)
    return [float(v) for v in rx], [float(v) for v in ry]


def same_bits(a, b):
    return np.array_equal(np.array(a, dtype=np.float64).view(np.uint64), np.array(b, dtype=np.float64).view(np.uint64))


def main():
    os.makedirs(GOLD, exist_ok=True)
    mp = ref_loader.load("lqr_path")
    m9 = ref_loader.load("rrt_09")
    script, inner = mp.LQRPlanner(), m9.LQRPlanner()
    out = {}

    # (a)
    rs = np.random.RandomState(1709)
    pairs = []
    for i in range(200):
        mag = 10.0 ** rs.uniform(-3, 6, 4)
        p = np.clip(rs.choice([-1.0, 1.0], 4) * mag, -1e6, 1e6)
        if i % 25 == 7:
            p[2:] = p[:2]                       # start == goal
        elif i % 25 == 8:
            p[2:] = p[:2] + rs.uniform(-0.2, 0.2, 2)    # within a few GOAL_DIST of each other
        pairs.append(p)
    pairs += [np.array(p) for p in B_PAIRS]
    n, rxs, rys = [], [], []
    for p in pairs:
        rx, ry = rollout(script, p)
        qx, qy = rollout(inner, p)
        assert same_bits(rx, qx) and same_bits(ry, qy), "the script's LQRPlanner and rrt_09's copy differ"
        assert len(rx) >= 2
        n.append(len(rx))
        rxs += rx
        rys += ry
    out.update(a_pairs=np.array(pairs), a_n=np.array(n, dtype=np.int32), a_rx=np.array(rxs), a_ry=np.array(rys))

    # (b)
    bn, rxs, rys = [], [], []
    for (mt, gd), expect in zip(B_CTL, B_EXPECT):
        script.MAX_TIME, script.GOAL_DIST = mt, gd
        row = []
        for p in B_PAIRS:
            rx, ry = rollout(script, p)
            row.append(len(rx))
            rxs += rx
            rys += ry
        assert row == expect, ((mt, gd), row, expect)
        bn.append(row)
    script.MAX_TIME, script.GOAL_DIST = 100.0, 0.1
    out.update(b_pairs=np.array(B_PAIRS), b_ctl=np.array(B_CTL), b_n=np.array(bn, dtype=np.int32), b_rx=np.array(rxs),
               b_ry=np.array(rys))

    # (c)
    rs = np.random.RandomState(31)
    tree = m9.LQRRRTStar([0, 0], [1, 1], [], [-2, 15])
    cp = np.concatenate([rs.uniform(-2, 15, (100, 2)), rs.uniform(-2, 15, (100, 2))], axis=1)
    cp[::10, 2:] = cp[::10, :2] + rs.uniform(-1, 1, (10, 2))     # short edges too
    cstep = np.array([[0.2, 0.1, 0.3, 0.07][i % 4] for i in range(100)])
    obs = np.stack([rs.uniform(-1, 14, 24), rs.uniform(-1, 14, 24), rs.uniform(0.3, 1.0, 24)], axis=1)
    rr = 0.3
    hit = []
    for p, st in zip(cp, cstep):
        wx, wy = rollout(script, p)
        px, py, _ = tree.sample_path(wx, wy, float(st))
        node = types.SimpleNamespace(path_x=px, path_y=py)
        h = -1
        for j, o in enumerate(obs):
            if not m9.LQRRRTStar.check_collision(node, [tuple(float(v) for v in o)], rr):
                h = j
                break
        hit.append(h)
    hit = np.array(hit, dtype=np.int32)
    assert np.sum(hit >= 0) >= 25 and np.sum(hit == -1) >= 25, (int(np.sum(hit >= 0)), int(np.sum(hit == -1)))
    assert np.sum(hit > 0) >= 5
    out.update(c_pairs=cp, c_step=cstep, c_obs=obs, c_rr=np.array(rr), c_hit=hit)

    dst = os.path.join(GOLD, "lqr_steer_kat.npz")
    np.savez_compressed(dst, **out)
    print("(a) %d pairs, rollouts of %d..%d points; (b) %s; (c) %d hit, %d free; %d bytes"
          % (len(pairs), min(n), max(n), bn, int(np.sum(hit >= 0)), int(np.sum(hit == -1)), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
