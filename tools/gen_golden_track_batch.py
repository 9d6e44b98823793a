"""Golden generator of the stand-alone tracker (BatchTrack, rrtx_tracker_run): known-answer vectors of the reference's
ClosedLoopRRTStar.check_tracking_path_is_feasible for the cases tests/golden/track_kat.npz does not hold.  rrt_10 is loaded
exactly as tools/gen_golden_closed_loop.py loads it.  Build host only (needs the reference checkout).

    python tools/gen_golden_track_batch.py

Writes tests/golden/track_batch_kat.npz: the fields of track_kat.npz (the path as the reference receives it, goal -> start)
plus start_state rows (x, y, yaw, v), in this order:
  long    chained Reeds-Shepp legs from the origin, truncated to exactly 3, 448, 449, 700 and 960 points: 448 / 449 are the
          last course the kernel holds in LDS and the first it holds in its global slab, 960 the longest it accepts.  At
          least two per length, and more until a slab course (449 and up) shows a reached goal and another a time-out
          (len(t) == 2002);
  start   vectors built like those of track_kat.npz, rolled out from a preset state instead of State(-0.0, -0.0, 0, 0): the
          loaded module's name `State` is replaced at run time by a callable returning that state;
  obs64   one course with 64 obstacles of which only the last in the list is touched by the driven trajectory (fail & 8),
          and the same course with that obstacle removed (bit 8 clear).
Every kept vector was computed by the reference without raising.  Prints the fail masks and exits non-zero when a wanted
case is missing."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_closed_loop import GOLD, MODEL, load, wrap_feasible  # noqa: E402

LONG_LENGTHS = (3, 448, 449, 700, 960)
SLAB_FROM = 449
N_START = 24
F_COLL = 8
DEFAULT_STATE = [-0.0, -0.0, 0.0, 0.0]


class Vectors:
    def __init__(self):
        self.rows, self.nobs, self.obs, self.npath, self.px, self.py, self.pw = [], [], [], [], [], [], []
        self.out, self.last, self.sums, self.start = [], [], [], []

    def add(self, course, obs, rr, ts, yth, ratio, state, rec):
        path = course[::-1]                       # what check_tracking_path_is_feasible receives: goal -> start
        self.rows.append([rr, ts, yth, ratio])
        self.nobs.append(len(obs))
        self.obs += [list(o) for o in obs]
        self.npath.append(len(path))
        self.px += [float(p[0]) for p in path]
        self.py += [float(p[1]) for p in path]
        self.pw += [float(p[2]) for p in path]
        self.out.append([int(rec["find"]), rec["n"], rec["fail"]])
        self.last.append([rec["tlast"]] + rec["last"])
        self.sums.append(rec["sums"])
        self.start.append(list(state))

    def save(self, path):
        np.savez_compressed(path, model=json.dumps(MODEL), rows=np.array(self.rows), nobs=np.array(self.nobs, dtype=np.int32),
                            obs=np.array(self.obs, dtype=np.float64).reshape(-1, 3), npath=np.array(self.npath, dtype=np.int32),
                            path_x=np.array(self.px), path_y=np.array(self.py), path_yaw=np.array(self.pw),
                            out=np.array(self.out, dtype=np.int32), last=np.array(self.last), sums=np.array(self.sums),
                            start_state=np.array(self.start))


def feasible(mod, course, obs, rr, ts, yth, ratio, state=None):
    """The reference's record for `course` (driving order, rows of [x, y, yaw]); state: the preset start state or None."""
    end = list(course[-1])
    obj = mod.ClosedLoopRRTStar([0.0, 0.0, 0.0], end, obs, [-2, 20], robot_radius=rr, target_speed=ts, yaw_th=yth,
                                invalid_travel_ratio=ratio)
    recs = []
    wrap_feasible(obj, recs)
    orig = mod.State
    if state is not None:
        mod.State = lambda **kw: orig(x=state[0], y=state[1], yaw=state[2], v=state[3])
    try:
        out = obj.check_tracking_path_is_feasible(course[::-1])
    finally:
        mod.State = orig
    return recs[0], out


def legs(mod, rs, pose, count, reach=(-6, 8)):
    """`count` chained Reeds-Shepp legs from `pose` as one polyline (the joints are kept twice, as track_kat.npz keeps them)."""
    pts = []
    while count > 0:
        to = [pose[0] + float(rs.uniform(*reach)), pose[1] + float(rs.uniform(*reach)), float(rs.uniform(-math.pi, math.pi))]
        qx, qy, qw, _, _ = mod.reeds_shepp_path_planning(pose[0], pose[1], pose[2], to[0], to[1], to[2], 1.0, 0.2)
        if not qx:
            continue
        pts += [[float(a), float(b), float(c)] for a, b, c in zip(qx, qy, qw)]
        pose = [qx[-1], qy[-1], qw[-1]]
        count -= 1
    return pts


def long_courses(mod, V):
    rs = np.random.RandomState(21)
    seen = {"reach": False, "timeout": False}
    masks = []
    rounds = 0
    while rounds < 2 or not all(seen.values()):
        if rounds >= 8:
            break
        for n in LONG_LENGTHS:
            pts = []
            while len(pts) < n:
                pts += legs(mod, rs, pts[-1] if pts else [0.0, 0.0, 0.0], 1)
            course = pts[:n]
            ts = float([20.0 / 3.6, 5.0 / 3.6, 10.0 / 3.6][rounds % 3])
            rec, _ = feasible(mod, course, [], 0.0, ts, float(np.deg2rad(3.0)), 5.0)
            V.add(course, [], 0.0, ts, float(np.deg2rad(3.0)), 5.0, DEFAULT_STATE, rec)
            masks.append((n, rec["n"], rec["fail"]))
            if n >= SLAB_FROM:
                seen["reach"] |= not (rec["fail"] & 1)
                seen["timeout"] |= rec["n"] == 2002
        rounds += 1
    print("long: (points, len(t), fail)", masks, flush=True)
    return all(seen.values())


def start_states(mod, V):
    rs = np.random.RandomState(22)
    masks = []
    for i in range(N_START):
        pose = [0.0, 0.0, 0.0] if i % 5 else [float(rs.uniform(-1, 1)), float(rs.uniform(-1, 1)), float(rs.uniform(-1, 1))]
        course = legs(mod, rs, pose, 1 + (i % 2))
        if i % 7 == 0:
            course = course + [[course[-1][0], course[-1][1], course[-1][2] + 0.9]]
        m = int(rs.randint(0, 5))
        obs = [(float(rs.uniform(-4, 8)), float(rs.uniform(-4, 8)), float(rs.uniform(0.2, 1.2))) for _ in range(m)]
        rr = float([0.0, 0.0, 0.3, 0.5][i % 4])
        ts = float([10.0 / 3.6, 5.0 / 3.6, 20.0 / 3.6][i % 3])
        yth = float(np.deg2rad([3.0, 1.0, 6.0][(i // 3) % 3]))
        ratio = float([5.0, 1.0, 1.3, 2.0][(i // 2) % 4])
        s0 = course[0]
        state = [s0[0] + float(rs.uniform(-1, 1)), s0[1] + float(rs.uniform(-1, 1)), s0[2] + float(rs.uniform(-0.5, 0.5)),
                 float([0.0, 1.0, -0.5][i % 3])]
        rec, out = feasible(mod, course, obs, rr, ts, yth, ratio, state)
        assert [out[1][0], out[2][0], out[4][0]] == [state[0], state[1], state[3]], "the preset state was not used"
        V.add(course, obs, rr, ts, yth, ratio, state, rec)
        masks.append(rec["fail"])
    print("start: fail masks", masks, flush=True)
    return len(masks) >= N_START


def obstacles_64(mod, V):
    rs = np.random.RandomState(23)
    course = legs(mod, rs, [0.0, 0.0, 0.0], 1, reach=(4, 8))
    rr, ts, yth, ratio = 0.2, 10.0 / 3.6, float(np.deg2rad(3.0)), 5.0
    _, out = feasible(mod, course, [], rr, ts, yth, ratio)
    tx, ty = np.array(out[1]), np.array(out[2])
    k = len(tx) // 2
    touched = (float(tx[k]), float(ty[k]), 0.1)
    far = []
    while len(far) < 63:    # clear of every driven point by more than the threshold radius
        o = (float(rs.uniform(-6, 14)), float(rs.uniform(-6, 14)), float(rs.uniform(0.2, 1.0)))
        if np.min(np.hypot(tx - o[0], ty - o[1])) > o[2] + rr + 0.25:
            far.append(o)
    with_it, _ = feasible(mod, course, far + [touched], rr, ts, yth, ratio)
    without, _ = feasible(mod, course, far, rr, ts, yth, ratio)
    V.add(course, far + [touched], rr, ts, yth, ratio, DEFAULT_STATE, with_it)
    V.add(course, far, rr, ts, yth, ratio, DEFAULT_STATE, without)
    print("obs64: fail with the 64th obstacle %d, without it %d" % (with_it["fail"], without["fail"]), flush=True)
    return bool(with_it["fail"] & F_COLL) and not (without["fail"] & F_COLL)


def main():
    mod = load()
    V = Vectors()
    ok = {"long (reach and time-out on a slab course)": long_courses(mod, V), "start": start_states(mod, V),
          "obs64": obstacles_64(mod, V)}
    missing = [k for k, v in ok.items() if not v]
    if missing:
        print("MISSING:", missing)
        return 1
    out = os.path.join(GOLD, "track_batch_kat.npz")
    V.save(out)
    o = np.array(V.out)
    print("track_batch_kat: %d vectors, %d points, feasible %d, fail masks %s, %d bytes" % (
        len(o), len(V.px), int(o[:, 0].sum()), sorted(set(o[:, 2].tolist())), os.path.getsize(out)))
    return 0 if os.path.getsize(out) < 256 * 1024 else 1


if __name__ == "__main__":
    sys.exit(main())
