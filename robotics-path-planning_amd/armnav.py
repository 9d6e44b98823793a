"""Batched arm navigation on the GPU: joint-space occupancy grids of a planar N-link arm among circles, and greedy best-first
searches on the torus grid -- many scenes and many start / goal queries in one call.

    nav = BatchArmNav(M=100)
    grids = nav.occupancy([0.5, 0.5, 0.3, 0.5, 0.1], [obstacles_a, obstacles_b])   # (2, 100, 100) uint8, kept on the device
    res = nav.plan(starts, goals, scene=[0, 1, 1, 0])                               # four queries, each on the grid it names
    res.route(2)                                                                     # the list astar_torus returns

For every scene: what get_occupancy_grid(arm, obstacles, M) of 02_arm_obstacle_navigation.py (:79-110) returns; for every
query: what astar_torus(grid, start_node, goal_node) (:113-184) returns and the marked grid it leaves behind.  Everything is
integers and every integer is the reference's (on the golden host, README): grid cells, route cells, marks 0..6, and the number
of cells the search closed.

As in the reference the grid varies two joint angles: link 1 stands at theta_list[i] and every later link at
theta_list[i] + theta_list[j].

There is no CPU fallback: without a device BatchArmNav raises RrtxError.
"""
import math

import numpy as np

from . import _abi


def _scene_lists(link_lengths, obstacles):
    """(arms, circle lists) one per scene.  link_lengths: one arm (a flat sequence of numbers) or one per scene; obstacles: one
    circle list (x, y, radius) per scene."""
    obstacles = list(obstacles)
    one_arm = len(link_lengths) > 0 and np.ndim(link_lengths[0]) == 0
    arms = [link_lengths] * len(obstacles) if one_arm else list(link_lengths)
    if len(arms) != len(obstacles):
        raise ValueError("BatchArmNav: %d arms for %d obstacle lists" % (len(arms), len(obstacles)))
    return arms, obstacles


def pack_scenes(link_lengths, obstacles):
    """The CSR arrays of rrtx_armnav_occupancy: (link_off, link_len, obs_off, obs_xyr)."""
    arms, obstacles = _scene_lists(link_lengths, obstacles)
    lens = [np.asarray(a, dtype=np.float64).reshape(-1) for a in arms]
    circ = []
    for i, o in enumerate(obstacles):
        c = np.asarray([[float(v) for v in r] for r in o], dtype=np.float64).reshape(-1, 3) if len(o) else np.zeros((0, 3))
        circ.append(c)
    link_off = np.zeros(len(lens) + 1, dtype=np.int64)
    obs_off = np.zeros(len(circ) + 1, dtype=np.int64)
    if lens:
        link_off[1:] = np.cumsum([len(a) for a in lens])
        obs_off[1:] = np.cumsum([len(c) for c in circ])
    link_len = np.ascontiguousarray(np.concatenate(lens) if lens else np.zeros(0), dtype=np.float64)
    obs_xyr = np.ascontiguousarray(np.concatenate(circ) if circ else np.zeros((0, 3)), dtype=np.float64)
    return link_off, link_len, obs_off, obs_xyr


class ArmNavResult:
    """One batch of searches.  Per query: status (ARMNAV_ROUTE, ARMNAV_NO_ROUTE), n_route (cells of the route), pops (cells the
    search closed); offsets (n + 1,) into cells, rows (i, j) int32; marks (n, M, M) uint8 -- the grid each search left behind,
    0 free, 1 obstacle, 2 closed, 3 opened, 4 start, 5 goal, 6 route -- or None when the batch was run with marks=False;
    kernel_ms."""

    def __init__(self, M, status, n_route, pops, offsets, cells, marks, kernel_ms=0.0):
        self.M = int(M)
        self.status, self.n_route, self.pops = status, n_route, pops
        self.offsets, self.cells, self.marks = offsets, cells, marks
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.status)

    @property
    def found(self):
        """Boolean mask of the queries with a route"""
        return self.status == _abi.ARMNAV_ROUTE

    def route(self, i):
        """What astar_torus returns for query i: a list of (i, j) tuples from start to goal, [] when there is no route"""
        return [tuple(c) for c in self.cells[int(self.offsets[i]):int(self.offsets[i + 1])].tolist()]

    def joint_angles(self, i):
        """(theta1, theta2) per cell of route i as the script's animate forms them (:32-33): 2 * pi * node / M - pi"""
        return [(2 * math.pi * a / self.M - math.pi, 2 * math.pi * b / self.M - math.pi) for a, b in self.route(i)]


class BatchArmNav:
    """Occupancy grids and searches for batches of scenes and queries on an M x M joint-space grid (2 <= M <= 128); device
    buffers and the grids of the last occupancy() are kept between calls."""

    def __init__(self, M=100, device=0):
        self.M = int(M)
        self._nav = _abi.ArmNav(device)
        self.n_scenes = 0
        self.grid_ms = 0.0   # HIP-event time of the kernels of the last occupancy()

    def close(self):
        self._nav.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def occupancy(self, link_lengths, obstacles):
        """link_lengths: one arm (1 .. 16 lengths, non-zero, negative allowed) or one arm per scene; obstacles: one list of
        circles (x, y, radius), at most 1024, per scene.  Returns (n_scenes, M, M) uint8 and keeps the grids on the device for
        plan()."""
        packed = pack_scenes(link_lengths, obstacles)
        self._nav.occupancy(self.M, *packed)
        self.n_scenes = len(packed[0]) - 1
        self.grid_ms = self._nav.kernel_ms()[0]
        return self._nav.grids(self.n_scenes, self.M)

    def plan(self, starts, goals, scene=None, grids=None, marks=True):
        """starts, goals: (n, 2) integer cells inside [0, M) -- numpy would wrap a negative index to the other end of the grid;
        this call refuses it.  scene: the grid of each query; default grid 0 when there is one grid, query q on grid q when
        there are as many grids as queries.  grids: (n_scenes, M, M) or (M, M) of 0..6 to search instead of the kept ones (they
        replace them; cells 2..6 are the marks of an earlier search and are searched as astar_torus would).  marks=False: the
        marked grids are not produced."""
        st = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
        go = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        if len(st) != len(go):
            raise ValueError("BatchArmNav: %d starts for %d goals" % (len(st), len(go)))
        if grids is not None:
            g = np.asarray(grids)
            if g.ndim == 2:
                g = g[None]
            if g.ndim != 3 or g.shape[1] != g.shape[2]:
                raise ValueError("BatchArmNav: grids is (n_scenes, M, M), not %r" % (g.shape,))
            if g.size and (g.min() < 0 or g.max() > 6):
                raise ValueError("BatchArmNav: a grid value outside 0..6")
            self._nav.set_grids(np.ascontiguousarray(g, dtype=np.uint8))
            self.n_scenes, self.M = g.shape[0], g.shape[1]
        if scene is None:
            if self.n_scenes > 1 and self.n_scenes != len(st):
                raise ValueError("BatchArmNav: %d grids and %d queries: say which grid each query searches" % (self.n_scenes, len(st)))
            sc = np.arange(len(st), dtype=np.int32) if self.n_scenes > 1 else None
        else:
            sc = np.ascontiguousarray(scene, dtype=np.int32).reshape(-1)
            if len(sc) != len(st):
                raise ValueError("BatchArmNav: %d scene indices for %d queries" % (len(sc), len(st)))
        N = self._nav
        N.search(sc, st, go, marks)
        status, n_route, pops, n_cells = N.counts()
        off, cells = N.routes(len(st), n_cells)
        return ArmNavResult(self.M, status, n_route, pops, off, cells, N.marks(len(st), self.M) if marks else None, N.kernel_ms()[1])
