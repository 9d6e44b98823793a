"""BatchPlanner.query_goals in plain Python: the best path to a goal g on a FINISHED tree, as the tail of the planners'
planning() finds it with `end` (rrt_04: and `goal_node`) set to g.  Written from the rules, over arrays:

  rrt_star              tree = (x, y, cost, parent).  dist[i] = hypot(x[i] - gx, y[i] - gy); the candidate list holds, for
                        every i in order with dist[i] <= expand_dis, the FIRST index whose distance equals dist[i]; each
                        is steered to g in steps of path_resolution (the last step snaps onto g when it is within one
                        step) and is safe when no point of that edge lies within size + robot_radius of an obstacle
                        centre and the edge's end lies inside the play area; the answer is the first safe candidate with
                        the lowest cost[i] + dist[i].  Index 0 can answer.  Course: g, then the chain up to the root.
  rrt_star_dubins /     tree = (x, y, yaw, cost, parent), polylines = (plen, px, py[, pyaw]) in node order.  Candidates:
  rrt_star_reeds_shepp  dist[i] <= goal_xy_th and abs(yaw[i] - gyaw) <= goal_yaw_th; the answer is the first candidate
                        with the lowest cost, and index 0 counts as no answer.  Course: g, the reversed polyline of every
                        chain node whose parent is not None ... the start pose.

Status values as _abi.GOALQ_*: 0 found, 1 none.  Every function returns a dict(node, cost, n_near, n_safe, status, course)
with course None or an (n, 2 | 3) array in planning order."""
import math

import numpy as np

OK, NONE = 0, 1


def steer_edge(fx, fy, tx, ty, res):
    """The points of steer(from, to) with an unbounded extend_length (rrt_04:1086-1115) and its end."""
    x, y = fx, fy
    d = math.hypot(tx - x, ty - y)
    theta = math.atan2(ty - y, tx - x)
    px, py = [x], [y]
    for _ in range(math.floor(d / res)):
        x += res * math.cos(theta)
        y += res * math.sin(theta)
        px.append(x)
        py.append(y)
    if math.hypot(tx - x, ty - y) <= res:
        px.append(tx)
        py.append(ty)
        x, y = tx, ty
    return px, py, x, y


def edge_free(px, py, obstacles, robot_radius):
    for (ox, oy, size) in obstacles:
        if min((ox - a) * (ox - a) + (oy - b) * (oy - b) for a, b in zip(px, py)) <= (size + robot_radius) ** 2:
            return False
    return True


def inside(play_area, x, y):
    if play_area is None:
        return True
    return not (x < play_area[0] or x > play_area[1] or y < play_area[2] or y > play_area[3])


def point_candidates(x, y, goal, expand_dis):
    """The candidate list with its repeats, as search_best_goal_node builds it."""
    dist = [math.hypot(float(a) - goal[0], float(b) - goal[1]) for a, b in zip(x, y)]
    return [dist.index(d) for d in dist if d <= expand_dis], dist


def query_rrt_star(tree, goal, expand_dis, path_resolution, obstacles, robot_radius=0.0, play_area=None):
    x, y, cost, parent = tree
    goal = (float(goal[0]), float(goal[1]))
    cand, dist = point_candidates(x, y, goal, expand_dis)
    distinct = sorted(set(cand))
    safe, blocked_by_play_only = [], 0
    for i in distinct:
        px, py, ex, ey = steer_edge(float(x[i]), float(y[i]), goal[0], goal[1], path_resolution)
        free = edge_free(px, py, obstacles, robot_radius)
        if free and inside(play_area, ex, ey):
            safe.append(i)
        elif free:
            blocked_by_play_only += 1
    out = dict(node=-1, cost=math.inf, n_near=len(distinct), n_safe=len(safe), status=NONE, course=None,
               repeats=len(cand) - len(distinct), play_only=blocked_by_play_only)
    if not safe:
        return out
    keys = [float(cost[i]) + dist[i] for i in safe]
    best = safe[keys.index(min(keys))]
    rows, nd = [[goal[0], goal[1]]], best
    while True:
        rows.append([float(x[nd]), float(y[nd])])
        if parent[nd] < 0:
            break
        nd = int(parent[nd])
    out.update(node=best, cost=min(keys), status=OK, course=np.array(rows))
    return out


def query_pose(tree, polylines, goal, start, goal_xy_th, goal_yaw_th, with_yaw):
    x, y, yaw, cost, parent = tree
    plen, cols = polylines[0], polylines[1:]
    goal = [float(v) for v in goal]
    near_xy = [i for i in range(len(x)) if math.hypot(float(x[i]) - goal[0], float(y[i]) - goal[1]) <= goal_xy_th]
    cand = [i for i in near_xy if abs(float(yaw[i]) - goal[2]) <= goal_yaw_th]
    out = dict(node=-1, cost=math.inf, n_near=len(cand), n_safe=0, status=NONE, course=None, n_xy=len(near_xy))
    if not cand:
        return out
    costs = [float(cost[i]) for i in cand]
    best = cand[costs.index(min(costs))]
    if not best:                                   # `if last_index:`
        return out
    ncol = 3 if with_yaw else 2
    off = np.concatenate([[0], np.cumsum(plen)])
    rows, nd = [goal[:ncol]], best
    while parent[nd] >= 0:                         # `while node.parent:` -- the root alone has none
        for q in reversed(range(int(off[nd]), int(off[nd + 1]))):
            rows.append([float(c[q]) for c in cols[:ncol]])
        nd = int(parent[nd])
    rows.append([float(v) for v in start[:ncol]])
    out.update(node=best, cost=min(costs), status=OK, course=np.array(rows))
    return out


def pack(results):
    """A list of query dicts -> the arrays of a GoalQueryResult (one row): node, cost, n_near, n_safe, status, offsets
    and the concatenated course columns (planning order)."""
    node = np.array([r["node"] for r in results], dtype=np.int32)
    cost = np.array([r["cost"] for r in results], dtype=np.float64)
    near = np.array([r["n_near"] for r in results], dtype=np.int32)
    safe = np.array([r["n_safe"] for r in results], dtype=np.int32)
    st = np.array([r["status"] for r in results], dtype=np.int32)
    lens = [0 if r["course"] is None else len(r["course"]) for r in results]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    have = [r["course"] for r in results if r["course"] is not None]
    pts = np.concatenate(have) if have else np.zeros((0, 2))
    return dict(node=node, cost=cost, n_near=near, n_safe=safe, status=st, offsets=off, points=pts)


def reverse_courses(off, pts):
    """The same CSR courses in driving order: every course's rows reversed."""
    out = pts.copy()
    for a, b in zip(off[:-1], off[1:]):
        out[a:b] = pts[a:b][::-1]
    return out
