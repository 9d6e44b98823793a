"""Golden generator of BatchPlanner.query_goals: runs the reference's planner classes themselves (loaded through
oracle/ref_loader.py, as tools/gen_golden_steer_all.py does) and writes tests/golden/goal_query_kat.npz.  Build host only
(needs the reference checkout).

    python tools/gen_golden_goal_query.py

Per case: plan with random.seed(s); then, per goal g, set rrt.end (rrt_04: and rrt.goal_node) to g, call
search_best_goal_node() and apply the tail's rule (rrt_04 `is not None`, rrt_05 / rrt_06 `if last_index:`), then
generate_final_course().  Arrays only, keys prefixed by the case name:
  <case>_cfg      the numbers of the case (see CFG_KEYS / POSE_CFG_KEYS), <case>_obstacles, _start, _goal, _rand_area,
                  _play_area (empty: none)
  <case>_goals    (g, 2 | 3)
  <case>_node, _cost (+inf without a node), _n_near (distinct candidates), _n_safe (rrt_04: distinct safe ones; else 0),
  _status (0 found, 1 none), _offsets (g + 1,), _points (sum, 2 | 3): the courses in planning order
  rrt_04 also: _repeats (entries of goal_inds beyond the distinct ones), _play_only (candidates with a free edge that ends
  outside the play area); the pose cases: _n_xy (nodes inside goal_xy_th before the angle check), and, per threshold set,
  the result keys carry the suffix _t0 (the planner's thresholds) / _t1 (the widened ones, <case>_th = [[xy, yaw], ..]);
  rs also _poly_yaw (the yaw of every polyline point, node order): the one tree column the project's CPU oracle does not hand out.
The conditions asserted at the end (and again by tests/test_goal_query_host.py) decided the seeds."""
import contextlib
import io
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DRIVER_OBST = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]   # rrt_04:1498-1500
DUBINS_OBST = DRIVER_OBST[:6]                                                                   # rrt_05:1804-1806
CFG_KEYS = ("seed", "max_iter", "until_max", "sobol", "expand_dis", "path_resolution", "goal_sample_rate", "robot_radius",
            "connect_circle_dist")
POSE_CFG_KEYS = ("seed", "max_iter", "curvature", "robot_radius", "goal_sample_rate", "expand_dis", "connect_circle_dist",
                 "goal_xy_th", "goal_yaw_th", "step_size")
POINT_CASES = (
    ("p0", dict(seed=7, max_iter=300, until_max=1, sobol=0, path_resolution=0.5, play_area=None)),
    ("p1", dict(seed=46, max_iter=300, until_max=0, sobol=0, path_resolution=0.5, play_area=None)),
    ("p2", dict(seed=5, max_iter=400, until_max=1, sobol=1, path_resolution=0.3, play_area=[-2, 12, 0, 14])),
)


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def pack_courses(courses, ncol):
    lens = [0 if c is None else len(c) for c in courses]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    have = [np.asarray(c, dtype=np.float64).reshape(-1, ncol) for c in courses if c is not None]
    return off, (np.concatenate(have) if have else np.zeros((0, ncol)))


# ---- rrt_04 ---------------------------------------------------------------------------------------------------------------
def point_goals(rrt):
    grid = [[float(gx), float(gy)] for gx in range(-2, 16) for gy in range(-2, 16)]            # 18 x 18 over [-2, 15]^2
    mid = rrt.node_list[len(rrt.node_list) // 2]
    special = [[mid.x, mid.y],                  # exactly on a mid-tree node
               [rrt.start.x, rrt.start.y],      # on the start
               [16.0, 8.0],                     # outside rand_area
               [3.0, 8.0],                      # inside an obstacle
               [float("nan"), 5.0],
               [float("inf"), 0.0]]
    return np.array(grid + special, dtype=np.float64)


def point_query(m04, rrt, g):
    """One goal on a planned rrt_04 object: (node, cost, n_near, n_safe, repeats, play_only, course)."""
    rrt.end = rrt.Node(float(g[0]), float(g[1]))
    rrt.goal_node = rrt.Node(float(g[0]), float(g[1]))
    index_of = {id(nd): i for i, nd in enumerate(rrt.node_list)}
    seen = {}                                   # candidate index -> [edge is free, end is inside the play area]
    calls = [0]
    o_cc, o_pa = m04.RRT.check_collision, m04.RRT.check_if_outside_play_area

    def cc_hook(node, ol, rr):
        r = o_cc(node, ol, rr)
        calls[0] += 1
        seen.setdefault(index_of[id(node.parent)], [r, None])
        return r

    def pa_hook(node, pa):
        r = o_pa(node, pa)
        seen[index_of[id(node.parent)]][1] = r
        return r
    rrt.check_collision, rrt.check_if_outside_play_area = cc_hook, pa_hook
    try:
        last = rrt.search_best_goal_node()
        course = rrt.generate_final_course(last) if last is not None else None
    finally:
        del rrt.check_collision, rrt.check_if_outside_play_area
    n_safe = sum(1 for v in seen.values() if v[0] and v[1])
    play_only = sum(1 for v in seen.values() if v[0] and v[1] is False)
    if last is None:
        return -1, math.inf, len(seen), n_safe, calls[0] - len(seen), play_only, None
    nd = rrt.node_list[last]
    return last, nd.cost + rrt.calc_dist_to_goal(nd.x, nd.y), len(seen), n_safe, calls[0] - len(seen), play_only, course


def run_point_case(m04, name, cfg, out):
    ref_loader.reset_sobol(m04)
    random.seed(cfg["seed"])
    full = dict(expand_dis=3.0, goal_sample_rate=5, robot_radius=0.8, connect_circle_dist=50.0)
    full.update(cfg)
    rrt = m04.RRT(start=[0, 0], goal=[6.0, 10.0], obstacle_list=DRIVER_OBST, rand_area=[-2, 15], expand_dis=full["expand_dis"],
                  path_resolution=full["path_resolution"], goal_sample_rate=full["goal_sample_rate"], max_iter=full["max_iter"],
                  play_area=full["play_area"], robot_radius=full["robot_radius"], sobol_sampler=bool(full["sobol"]),
                  connect_circle_dist=full["connect_circle_dist"], search_until_max_iter=bool(full["until_max"]))
    quiet(rrt.planning, animation=False)
    state = random.getstate()
    goals = point_goals(rrt)
    rows = [quiet(point_query, m04, rrt, g) for g in goals]
    assert random.getstate() == state, "a query consumed random numbers"
    off, pts = pack_courses([r[6] for r in rows], 2)
    out.update({name + "_cfg": np.array([float(full[k]) for k in CFG_KEYS]),
                name + "_obstacles": np.array(DRIVER_OBST, dtype=np.float64), name + "_start": np.array([0.0, 0.0]),
                name + "_goal": np.array([6.0, 10.0]), name + "_rand_area": np.array([-2.0, 15.0]),
                name + "_play_area": np.array(full["play_area"] if full["play_area"] is not None else [], dtype=np.float64),
                name + "_n_nodes": np.array(len(rrt.node_list)),
                name + "_goals": goals, name + "_node": np.array([r[0] for r in rows], dtype=np.int32),
                name + "_cost": np.array([r[1] for r in rows]), name + "_n_near": np.array([r[2] for r in rows], dtype=np.int32),
                name + "_n_safe": np.array([r[3] for r in rows], dtype=np.int32),
                name + "_status": np.array([0 if r[0] >= 0 else 1 for r in rows], dtype=np.int32),
                name + "_repeats": np.array([r[4] for r in rows], dtype=np.int32),
                name + "_play_only": np.array([r[5] for r in rows], dtype=np.int32),
                name + "_offsets": off, name + "_points": pts})
    print("%s: %d nodes, %d goals, %d found" % (name, len(rrt.node_list), len(goals), sum(r[0] >= 0 for r in rows)))


# ---- rrt_05 / rrt_06 --------------------------------------------------------------------------------------------------------
def pose_goals(rrt, rng):
    """Node poses shifted by less than the planner's thresholds, the same with the yaw off by more than goal_yaw_th,
    the start pose, a pose far from every node, a NaN."""
    nl = rrt.node_list
    picks = rng.sample(range(1, len(nl)), min(28, len(nl) - 1))
    goals = []
    for i in picks:
        nd = nl[i]
        goals.append([nd.x + rng.uniform(-0.3, 0.3), nd.y + rng.uniform(-0.3, 0.3), nd.yaw + rng.uniform(-0.8, 0.8) * rrt.goal_yaw_th])
    for i in picks[:14]:
        nd = nl[i]
        goals.append([nd.x + rng.uniform(-0.2, 0.2), nd.y + rng.uniform(-0.2, 0.2), nd.yaw + rng.choice((-1, 1)) * rng.uniform(0.05, 0.3)])
    goals.append([rrt.start.x, rrt.start.y, rrt.start.yaw])
    goals.append([40.0, -30.0, 0.0])
    goals.append([float("nan"), 1.0, 0.0])
    return np.array(goals, dtype=np.float64)


def pose_query(rrt, g, ncol):
    rrt.end = rrt.Node(float(g[0]), float(g[1]), float(g[2]))
    n_xy = sum(1 for nd in rrt.node_list if rrt.calc_dist_to_goal(nd.x, nd.y) <= rrt.goal_xy_th)
    n_near = sum(1 for nd in rrt.node_list if rrt.calc_dist_to_goal(nd.x, nd.y) <= rrt.goal_xy_th
                 and abs(nd.yaw - rrt.end.yaw) <= rrt.goal_yaw_th)
    last = rrt.search_best_goal_node()
    if last:
        return last, rrt.node_list[last].cost, n_near, n_xy, np.array(rrt.generate_final_course(last)).reshape(-1, ncol)
    return -1, math.inf, n_near, n_xy, None


def run_pose_case(mod, name, rs, seed, max_iter, out):
    random.seed(seed)
    cfg = dict(seed=seed, max_iter=max_iter, curvature=2.0 if rs else 1.0, robot_radius=0.6 if rs else 0.0, goal_sample_rate=10,
               expand_dis=3.0, connect_circle_dist=50.0, goal_xy_th=0.5, goal_yaw_th=float(np.deg2rad(1.0)),
               step_size=0.1 if rs else 0.0)
    start, goal = [0.0, 0.0, 0.0], ([10.0, 9.0, 0.0] if rs else [10.0, 10.0, 0.0])
    obst = DRIVER_OBST if rs else DUBINS_OBST
    kw = dict(start=start, goal=goal, obstacle_list=obst, rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.5,
              goal_sample_rate=10, max_iter=max_iter, play_area=None, robot_radius=cfg["robot_radius"], sobol_sampler=True,
              connect_circle_dist=50.0, search_until_max_iter=not rs, curvature=cfg["curvature"],
              goal_yaw_th=cfg["goal_yaw_th"], goal_xy_th=0.5)
    if rs:
        kw["step_size"] = 0.1
    rrt = mod.RRT(**kw)                                      # as oracle/gen_golden.py builds the two planners
    quiet(rrt.planning, animation=False)
    state = random.getstate()
    ncol = 3 if rs else 2
    goals = pose_goals(rrt, random.Random(seed + 1000))
    ths = [[cfg["goal_xy_th"], cfg["goal_yaw_th"]], [0.8, 0.5]]
    out.update({name + "_cfg": np.array([float(cfg[k]) for k in POSE_CFG_KEYS]), name + "_obstacles": np.array(obst, dtype=np.float64),
                name + "_start": np.array(start), name + "_goal": np.array(goal), name + "_rand_area": np.array([-2.0, 15.0]),
                name + "_n_nodes": np.array(len(rrt.node_list)), name + "_goals": goals, name + "_th": np.array(ths)})
    if rs:
        out[name + "_poly_yaw"] = np.concatenate([np.asarray(nd.path_yaw, dtype=np.float64).reshape(-1) for nd in rrt.node_list])
    for t, (xy, yw) in enumerate(ths):
        rrt.goal_xy_th, rrt.goal_yaw_th = xy, yw
        rows = [quiet(pose_query, rrt, g, ncol) for g in goals]
        off, pts = pack_courses([r[4] for r in rows], ncol)
        sfx = "_t%d" % t
        out.update({name + "_node" + sfx: np.array([r[0] for r in rows], dtype=np.int32),
                    name + "_cost" + sfx: np.array([r[1] for r in rows]),
                    name + "_n_near" + sfx: np.array([r[2] for r in rows], dtype=np.int32),
                    name + "_n_xy" + sfx: np.array([r[3] for r in rows], dtype=np.int32),
                    name + "_status" + sfx: np.array([0 if r[0] >= 0 else 1 for r in rows], dtype=np.int32),
                    name + "_offsets" + sfx: off, name + "_points" + sfx: pts})
        print("%s%s: %d nodes, %d goals, %d found, %d points" % (name, sfx, len(rrt.node_list), len(goals),
                                                                 sum(r[0] >= 0 for r in rows), len(pts)))
    assert random.getstate() == state, "a query consumed random numbers"


def point_conditions(g):
    """The counts the rrt_04 set must reach (tests/test_goal_query_host.py asserts the same)."""
    c = dict(found=0, unsafe=0, empty=0, repeats=0, play_only=0)
    for name, _ in POINT_CASES:
        st, near = g[name + "_status"], g[name + "_n_near"]
        c["found"] += int((st == 0).sum())
        c["unsafe"] += int(((st != 0) & (near > 0)).sum())
        c["empty"] += int((near == 0).sum())
        c["repeats"] += int((g[name + "_repeats"] > 0).sum())
        c["play_only"] += int(((st != 0) & (g[name + "_play_only"] > 0)).sum())
    return c


def pose_conditions(g):
    c = dict(found=0, yaw_only=0)
    for name in ("d0", "r0"):
        for t in (0, 1):
            st, near, nxy = g[name + "_status_t%d" % t], g[name + "_n_near_t%d" % t], g[name + "_n_xy_t%d" % t]
            c["found"] += int((st == 0).sum())
            c["yaw_only"] += int(((near == 0) & (nxy > 0)).sum())
    return c


POINT_MIN = dict(found=100, unsafe=50, empty=10, repeats=10, play_only=1)
POSE_MIN = dict(found=20, yaw_only=10)


def main():
    out = {}
    m04 = ref_loader.load("rrt_04")
    for name, cfg in POINT_CASES:
        run_point_case(m04, name, cfg, out)
    run_pose_case(ref_loader.load("rrt_05"), "d0", False, 42, 300, out)
    run_pose_case(ref_loader.load("rrt_06"), "r0", True, 42, 200, out)
    pc, qc = point_conditions(out), pose_conditions(out)
    print(pc, qc)
    for k, v in POINT_MIN.items():
        assert pc[k] >= v, (k, pc[k])
    for k, v in POSE_MIN.items():
        assert qc[k] >= v, (k, qc[k])
    path = os.path.join(GOLD, "goal_query_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
