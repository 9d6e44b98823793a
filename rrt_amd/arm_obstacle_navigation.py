"""Names of 02_arm_obstacle_navigation.py as its driver cell uses them.  The MI355X mirror: get_occupancy_grid and astar_torus
are a batch of one on robotics-path-planning_amd/armnav.py (same arguments, same return types, the script's integers one for
one); no CPU fallback.  NLinkArm, detect_collision, find_neighbors and calc_heuristic_map are a few lines of host arithmetic: one
arm pose, one segment, one cell need no device.  No matplotlib: nothing is drawn while planning (NLinkArm.plot_arm draws an arm
on the pyplot-like object it is handed, after the fact).

astar_torus and find_neighbors read the grid size from a module global M in the script; here astar_torus takes it from
grid.shape, and find_neighbors takes it as a third argument (default: this module's M, 100 as in the script)."""
from math import pi

import numpy as np

from . import armnav as _a

M = 100
_navigator = None


def _nav(m):
    global _navigator
    if _navigator is None:
        _navigator = _a.BatchArmNav(M=m)
    _navigator.M = m
    return _navigator


class NLinkArm(object):
    """A planar arm of len(link_lengths) links: points[k] is the end of link k (points[0] the base at the origin)."""

    def __init__(self, link_lengths, joint_angles):
        if len(link_lengths) != len(joint_angles):
            raise ValueError()
        self.n_links = len(link_lengths)
        self.link_lengths = np.array(link_lengths)
        self.joint_angles = np.array(joint_angles)
        self.points = [[0, 0] for _ in range(self.n_links + 1)]
        self.lim = sum(link_lengths)
        self.update_points()

    def update_joints(self, joint_angles):
        self.joint_angles = joint_angles
        self.update_points()

    def update_points(self):
        for k in range(self.n_links):
            a = np.sum(self.joint_angles[:k + 1])   # fewer angles than links: the later links keep the last sum
            self.points[k + 1][0] = self.points[k][0] + self.link_lengths[k] * np.cos(a)
            self.points[k + 1][1] = self.points[k][1] + self.link_lengths[k] * np.sin(a)
        self.end_effector = np.array(self.points[self.n_links]).T

    def plot_arm(self, myplt, obstacles=[]):  # pragma: no cover
        myplt.cla()
        for ox, oy, size in obstacles:
            myplt.gca().add_patch(myplt.Circle((ox, oy), radius=0.5 * size, fc='k'))
        xs, ys = [p[0] for p in self.points], [p[1] for p in self.points]
        myplt.plot(xs, ys, 'r-')
        myplt.plot(xs, ys, 'k.')
        myplt.xlim([-self.lim, self.lim])
        myplt.ylim([-self.lim, self.lim])
        myplt.draw()


def detect_collision(line_seg, circle):
    """True when the segment line_seg = [[ax, ay], [bx, by]] touches the circle [cx, cy, radius]: the point of the segment
    nearest the centre is no farther from it than the radius."""
    a = np.array([line_seg[0][0], line_seg[0][1]])
    b = np.array([line_seg[1][0], line_seg[1][1]])
    c = np.array([circle[0], circle[1]])
    seg = b - a
    length = np.linalg.norm(seg)
    along = (c - a).dot(seg / length)
    if along <= 0:
        nearest = a
    elif along >= length:
        nearest = b
    else:
        nearest = a + seg * along / length
    return not np.linalg.norm(nearest - c) > circle[2]


def get_occupancy_grid(arm, obstacles, M):
    """The M x M int64 grid over the first two joint angles, from -pi in steps of 2 pi / M: 1 where a link of `arm` touches an
    obstacle [x, y, radius], else 0.  Computed on the device; `arm` is left at the last cell's angles, as the script leaves it."""
    grid = _nav(int(M)).occupancy([float(v) for v in arm.link_lengths], [[list(o) for o in obstacles]])[0]
    first = -M // 2
    last = 2 * (first + M - 1) * pi / M
    arm.update_joints([last, last])
    return grid.astype(np.int64)


def astar_torus(grid, start_node, goal_node):
    """The route, a list of (i, j) tuples from start_node to goal_node ([] when there is none), of the greedy best-first
    search with wrap-around on `grid` (a square ndarray: 0 free, 1 obstacle); `grid` is marked in place as the script marks it
    (2 closed, 3 opened, 4 start, 5 goal, 6 route).  Computed on the device."""
    g = np.asarray(grid)
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError("astar_torus: grid is a square array, not %r" % (g.shape,))
    res = _nav(g.shape[0]).plan([[int(start_node[0]), int(start_node[1])]], [[int(goal_node[0]), int(goal_node[1])]], grids=g)
    grid[...] = res.marks[0]
    route = res.route(0)
    if route:
        print("The route found covers %d grid cells." % len(route))
    else:
        print("No route found.")
    return route


def find_neighbors(i, j, M=None):
    """The cells above, below, left and right of (i, j), in that order, round the edges of the M x M torus."""
    m = globals()["M"] if M is None else M
    return [((i - 1) % m, j), ((i + 1) % m, j), (i, (j - 1) % m), (i, (j + 1) % m)]


def calc_heuristic_map(M, goal_node):
    """The script's heuristic: the Manhattan distance to goal_node, then one row-major in-place pass that takes each cell down to
    what a step over an edge of the grid and the value it finds at the opposite border give.  The pass reads borders that it
    has partly rewritten already, so the result is not the torus distance; it is computed here in the order in which those
    reads become final: cell (0, 0), the rest of row 0 and column 0, the rest."""
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    o = np.abs(j - goal_node[1]) + np.abs(i - goal_node[0])
    h = o.copy()
    h[0, 0] = min(o[0, 0], 1 + o[M - 1, 0], M + o[0, 0], 1 + o[0, M - 1], M + o[0, 0])
    k = np.arange(1, M)
    h[0, 1:] = np.minimum.reduce([o[0, 1:], 1 + o[M - 1, 1:], M + o[0, 1:], k + 1 + o[0, M - 1], M - k + h[0, 0]])
    h[1:, 0] = np.minimum.reduce([o[1:, 0], k + 1 + o[M - 1, 0], M - k + h[0, 0], 1 + o[1:, M - 1], M + o[1:, 0]])
    I, J = i[1:, 1:], j[1:, 1:]
    h[1:, 1:] = np.minimum.reduce([o[1:, 1:], I + 1 + o[M - 1, 1:][None, :], M - I + h[0, 1:][None, :],
                                   J + 1 + o[1:, M - 1][:, None], M - J + h[1:, 0][:, None]])
    return h


__all__ = ['NLinkArm', 'detect_collision', 'get_occupancy_grid', 'astar_torus', 'find_neighbors', 'calc_heuristic_map']
