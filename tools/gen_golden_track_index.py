"""Golden generator of the tracker's obstacle index (BatchTrack(obstacle_index=True), rrtx_tracker_set_obstacle_index):
known-answer vectors of the reference's ClosedLoopRRTStar.check_tracking_path_is_feasible against lists of more circles than
the 64 the lane-per-obstacle check takes.  rrt_10 is loaded exactly as tools/gen_golden_track_batch.py loads it.  Build host
only (needs the reference checkout).

    python tools/gen_golden_track_index.py

Writes tests/golden/track_index_kat.npz:
  the courses   the fields of track_kat.npz (rows, npath, path_x / _y / _yaw goal -> start, start_state; nobs is 0 throughout):
                N_KAT courses of tests/golden/track_kat.npz and N_BATCH of tests/golden/track_batch_kat.npz (preset start
                states, and the 448- and 449-point courses: the last the kernel holds in LDS and the first in its slab), all
                with robot radius RR;
  per list      obs_<m> (m rows x, y, size), out_<m> / last_<m> / sums_<m> (the records of track_kat.npz, one row per course) and
                first_<m>: per course the lowest row of the list that touches a driven point (-1 none), from the reference's
                own x, y -- for m in LISTS.
The circles are spread over the box of the driven trajectories and their radii shrink with the count.  Floors, which the
generator computes from the reference's x, y before it keeps a list (it tries radii and seeds until they hold and exits
non-zero otherwise): at least 4 courses with the collision bit and 4 without, and a blocked course whose lowest touching row
is >= 64, so a check that reads 64 rows only cannot pass."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden_closed_loop import GOLD, load  # noqa: E402
from gen_golden_track_batch import Vectors, feasible  # noqa: E402
from test_track_batch_host import kat_vectors  # noqa: E402

LISTS = (65, 300, 1000)
RR = 0.1
N_KAT, N_BATCH = 14, 8
F_COLL = 8
FLOOR = 4
DEFAULT_BITS = np.array([-0.0, -0.0, 0.0, 0.0]).view(np.uint64)


def pick_courses():
    out = []
    g = np.load(os.path.join(GOLD, "track_kat.npz"))
    vecs = kat_vectors(g)
    out += [vecs[i] for i in range(0, len(vecs), len(vecs) // N_KAT)][:N_KAT]
    g = np.load(os.path.join(GOLD, "track_batch_kat.npz"))
    vecs = kat_vectors(g)
    preset = [v for v in vecs if np.any(np.asarray(v[6], dtype=np.float64).view(np.uint64) != DEFAULT_BITS)]
    out += [next(v for v in vecs if len(v[3]) == n) for n in (448, 449)] + preset[:N_BATCH - 2]
    return out


def first_touch(tx, ty, obs):
    """The lowest row of obs that touches a driven point, the reference's test d^2 <= (size + RR) ** 2; -1 none."""
    dx = obs[:, 0][:, None] - tx[None, :]
    dy = obs[:, 1][:, None] - ty[None, :]
    rows = np.nonzero(np.any(dx * dx + dy * dy <= ((obs[:, 2] + RR) ** 2)[:, None], axis=1))[0]
    return (int(rows[0]) if len(rows) else -1), rows


def make_list(m, traj, box):
    """m circles over `box` for which the floors hold, or None"""
    side = max(box[1] - box[0], box[3] - box[2])
    for scale in (0.35, 0.25, 0.5, 0.18, 0.7, 0.1, 0.05, 0.02):
        for seed in range(40):
            rs = np.random.RandomState(1000 * m + seed)
            size = scale * side / np.sqrt(m)                  # the radii shrink with the count
            obs = np.stack([rs.uniform(box[0], box[1], m), rs.uniform(box[2], box[3], m), rs.uniform(0.5 * size, size, m)], axis=1)
            touched = [first_touch(tx, ty, obs)[1] for tx, ty in traj]
            # a blocked course all of whose touching rows can stand behind row 63: they go to the end of the list
            fits = [t for t in touched if 0 < len(t) <= m - 64]
            if not fits:
                continue
            tail = min(fits, key=len)
            order = [k for k in range(m) if k not in set(tail.tolist())] + tail.tolist()
            obs = obs[order]
            first = [first_touch(tx, ty, obs)[0] for tx, ty in traj]
            blocked = sum(f >= 0 for f in first)
            if blocked >= FLOOR and len(first) - blocked >= FLOOR and max(first) >= 64:
                return obs, first
    return None


def main():
    mod = load()
    courses = pick_courses()
    assert len(courses) >= 16
    V = Vectors()
    traj, presets = [], []
    for params, _, _, cx, cy, cw, start in courses:
        course = [[float(a), float(b), float(c)] for a, b, c in zip(cx, cy, cw)]
        preset = None if np.array_equal(np.asarray(start, dtype=np.float64).view(np.uint64), DEFAULT_BITS) else [float(q) for q in start]
        presets.append(preset)
        rec, out = feasible(mod, course, [], RR, params["target_speed"], params["yaw_th"], params["invalid_travel_ratio"], preset)
        V.add(course, [], RR, params["target_speed"], params["yaw_th"], params["invalid_travel_ratio"], list(start), rec)
        traj.append((np.array(out[1]), np.array(out[2])))
    box = [min(t[0].min() for t in traj), max(t[0].max() for t in traj), min(t[1].min() for t in traj), max(t[1].max() for t in traj)]
    print("courses %d, box of the driven trajectories %s" % (len(courses), np.round(box, 2).tolist()), flush=True)
    extra = {}
    for m in LISTS:
        made = make_list(m, traj, box)
        if made is None:
            print("MISSING: no list of %d circles holds the floors" % m)
            return 1
        obs, first = made
        rows = [tuple(float(q) for q in r) for r in obs]
        outs, lasts, sums = [], [], []
        for i, (params, _, _, cx, cy, cw, start) in enumerate(courses):
            course = [[float(a), float(b), float(c)] for a, b, c in zip(cx, cy, cw)]
            rec, out = feasible(mod, course, rows, RR, params["target_speed"], params["yaw_th"], params["invalid_travel_ratio"], presets[i])
            assert np.array_equal(np.array(out[1]), traj[i][0]) and np.array_equal(np.array(out[2]), traj[i][1])
            assert bool(rec["fail"] & F_COLL) == (first[i] >= 0), "the reference and the floor computation disagree"
            outs.append([int(rec["find"]), rec["n"], rec["fail"]])
            lasts.append([rec["tlast"]] + rec["last"])
            sums.append(rec["sums"])
        extra.update({"obs_%d" % m: obs, "out_%d" % m: np.array(outs, dtype=np.int32), "last_%d" % m: np.array(lasts),
                      "sums_%d" % m: np.array(sums), "first_%d" % m: np.array(first, dtype=np.int32)})
        print("list %4d: size %.3f .. %.3f, blocked %d of %d, first touching rows %s" % (
            m, obs[:, 2].min(), obs[:, 2].max(), sum(f >= 0 for f in first), len(first), first), flush=True)
    out = os.path.join(GOLD, "track_index_kat.npz")
    V.save(out)
    base = dict(np.load(out))
    np.savez_compressed(out, **base, **extra)
    print("track_index_kat: %d courses, %d bytes" % (len(courses), os.path.getsize(out)))
    return 0 if os.path.getsize(out) < 256 * 1024 else 1


if __name__ == "__main__":
    sys.exit(main())
