"""Host-side mirrors of the reference planner classes, driving the HIP library.

Same constructor keywords, entry points, attributes and return shapes as
  rrt_01: /root/reference/src_path_planning/10_path_planning_01_rrt_01_simple.py   class RRT :16-101
  rrt_04: /root/reference/src_path_planning/10_path_planning_01_rrt_04_rrt_star.py class RRT :932-1384
so a driver script written against the reference runs unchanged:

    random.seed(s)
    rrt = RRT(start=..., goal=..., obstacle_list=..., rand_area=..., ...)
    path = rrt.planning(animation=False)      # list of [x, y] goal -> start, or None
    len(rrt.node_list); rrt.node_list[i].path_x; rrt.draw_graph()

`planning()` hands CPython's global `random` state to the device (the kernels
consume the MT19937 stream exactly as random.randint / random.uniform would) and
stores the advanced state back, so code after the call sees the same stream it
would have seen with the reference.  stdout chatter of the reference
("Iter: ...", rrt_04:1045) is not reproduced.  All planning runs on the GPU.
"""
import math
import random

import numpy as np

from . import _abi


class Node:
    """RRT.Node (rrt_04:933-942); path_x/path_y are rebuilt on demand for drawing."""

    def __init__(self, x, y):
        self.x = x
        self.y = y
        self.path_x = []
        self.path_y = []
        self.parent = None
        self.cost = 0.0


class AreaBounds:
    """RRT.AreaBounds (rrt_04:944-949)."""

    def __init__(self, area):
        self.xmin = float(area[0])
        self.xmax = float(area[1])
        self.ymin = float(area[2])
        self.ymax = float(area[3])


def _steer_polyline(fx, fy, tx, ty, extend, res):
    """Polyline of steer() (rrt_04:1086-1115) with CPython's own math, for path_x/path_y."""
    nx, ny = fx, fy
    dx, dy = tx - nx, ty - ny
    d, theta = math.hypot(dx, dy), math.atan2(dy, dx)
    px, py = [nx], [ny]
    if extend > d:
        extend = d
    for _ in range(math.floor(extend / res)):
        nx += res * math.cos(theta)
        ny += res * math.sin(theta)
        px.append(nx)
        py.append(ny)
    if math.hypot(tx - nx, ty - ny) <= res:
        px.append(tx)
        py.append(ty)
    return px, py


def _creation_records(trace, kind, n_nodes):
    """(nearest, sample x, sample y, kind) per NODE from the per-ITERATION trace: iterations that appended a node
    (kind 1 / 2) did so in order, node 0 is the start."""
    rx, ry, nearest, _ = trace
    k = min(len(kind), len(rx))
    it = np.nonzero(kind[:k] > 0)[0]
    if len(it) != n_nodes - 1:      # early exit of a launch chunk etc.: no record rather than a wrong one
        return None
    c_near = np.full(n_nodes, -1, dtype=np.int64)
    c_rx = np.zeros(n_nodes)
    c_ry = np.zeros(n_nodes)
    c_kind = np.zeros(n_nodes, dtype=np.int64)
    c_near[1:], c_rx[1:], c_ry[1:], c_kind[1:] = nearest[it], rx[it], ry[it], kind[it]
    return c_near, c_rx, c_ry, c_kind


class NodeList:
    """Lazy `node_list`: SoA arrays from the device, Node objects made on access.

    Parents are object references as in rrt_01/rrt_04 (the same Node object is
    returned for the same index, so identity comparisons behave).

    `path_x` / `path_y` (what draw_graph plots, rrt_04:1165-1167) are rebuilt on the host with CPython's own math, as
    the reference built them.  A node holds the polyline of the steer() call that produced its current entry in
    node_list:
      * re-pointed by a later rewire (its parent index is larger than its own: `node_list[i] = edge_node`, :1372):
        steer(parent -> node, inf) (:1359);
      * appended as the extension itself (rrt_01:85-96; rrt_04:1066-1067 when choose_parent returned None):
        steer(nearest -> sample, expand_dis) (:1051);
      * appended under a chosen parent: steer(parent -> extension end, inf) (:1279).
    `creation` = (nearest index, sample x, sample y, kind) per node, from the device's per-iteration trace
    (rrtx_get_trace / rrtx_get_trace_kind); without it every node falls back to steer(parent -> node, inf).

    Limit (draw-only data): the polylines are rebuilt from the FINAL coordinates of the nearest / parent node.  When a
    later rewire moved that node (an unsnapped steer with an inexact path_resolution, rrt_04:1372), the reference's stored
    polyline still starts at the old position, and a rewired node's path ends at the pre-move target; path_x / path_y are
    exact only while no nearest node or ancestor has moved (with a binary-fraction resolution such as the C2 map's 0.25 none
    moves).  Tree, costs and the returned path are not affected."""

    def __init__(self, x, y, cost, parent, res, expand_dis=None, creation=None):
        self._x, self._y, self._cost, self._parent, self._res = x, y, cost, parent, res
        self._expand_dis, self._creation = expand_dis, creation
        self._cache = {}

    def __len__(self):
        return len(self._x)

    def _polyline(self, j, pj):
        cr = self._creation
        if cr is not None and pj < j and cr[3][j] > 0:
            ne = int(cr[0][j])
            ex, ey = _steer_polyline(float(self._x[ne]), float(self._y[ne]), float(cr[1][j]), float(cr[2][j]),
                                     self._expand_dis, self._res)
            if cr[3][j] == 1:
                return ex, ey
            return _steer_polyline(float(self._x[pj]), float(self._y[pj]), ex[-1], ey[-1], float("inf"), self._res)
        return _steer_polyline(float(self._x[pj]), float(self._y[pj]), float(self._x[j]), float(self._y[j]),
                               float("inf"), self._res)

    def _make(self, i):
        nd = self._cache.get(i)
        if nd is not None:
            return nd
        # iterative parent chain construction (trees are ~100 deep, but avoid recursion limits)
        chain = []
        j = i
        while j >= 0 and j not in self._cache:
            chain.append(j)
            j = int(self._parent[j])
        for j in reversed(chain):
            n = Node(float(self._x[j]), float(self._y[j]))
            n.cost = float(self._cost[j])
            pj = int(self._parent[j])
            if pj >= 0:
                n.parent = self._cache[pj]
                n.path_x, n.path_y = self._polyline(j, pj)
            self._cache[j] = n
        return self._cache[i]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._make(j) for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._make(i)

    def __iter__(self):
        for i in range(len(self)):
            yield self._make(i)


class _PlannerBase:
    Node = Node
    AreaBounds = AreaBounds
    _ALGO = None

    def _common_init(self, start, goal, obstacle_list, rand_area, expand_dis, path_resolution, goal_sample_rate,
                     max_iter, play_area, robot_radius, device):
        self.start = Node(start[0], start[1])
        self.end = Node(goal[0], goal[1])
        self.min_rand = rand_area[0]
        self.max_rand = rand_area[1]
        self.play_area = AreaBounds(play_area) if play_area is not None else None
        self._play_area_arg = play_area
        self.expand_dis = expand_dis
        self.path_resolution = path_resolution
        self.goal_sample_rate = goal_sample_rate
        self.max_iter = max_iter
        self.obstacle_list = obstacle_list
        self.node_list = []
        self.robot_radius = robot_radius
        self.device = device
        # How planning() hands over obstacle_list (rrt_01 / rrt_02 / rrt_04): None = through the obstacle map when the list
        # has more than 256 circles (rrtx_set_obstacle_map: any number up to 2**20), True = always, False = never, which
        # fails beyond 256.  An attribute, set after construction: the constructors keep the reference's signatures.
        self.obstacle_map = None
        self.stats = None
        self._trace = False
        self.trace = None

    def _run(self, sampler, ccd, until_max):
        h = _abi.Handle(self._ALGO, [self.start.x, self.start.y], [self.end.x, self.end.y],
                        [self.min_rand, self.max_rand], self.expand_dis, self.path_resolution, self.goal_sample_rate,
                        self.max_iter, play_area=self._play_area_arg, robot_radius=self.robot_radius, sampler=sampler,
                        connect_circle_dist=ccd, search_until_max_iter=until_max, n_instances=1, device=self.device)
        try:
            h.load_obstacles(self.obstacle_list, self.obstacle_map)
            st = random.getstate()
            h.set_rng_state(0, st)
            h.enable_trace(0)   # per-iteration (sample, nearest, what was appended): Node.path_x / path_y need it
            h.plan(strict=True)
            random.setstate(h.get_rng_state(0, st[2]))
            x, y, cost, parent = h.get_tree(0)
            trace = h.get_trace()
            self.node_list = NodeList(x, y, cost, parent, self.path_resolution, self.expand_dis,
                                      _creation_records(trace, h.get_trace_kind(), len(x)))
            self.tree = (x, y, cost, parent)
            path = h.get_path(0)
            self.stats = h.get_stats()
            if self._trace:
                self.trace = trace
            if sampler == _abi.SAMPLER_SOBOL:
                self.sobol_inter_ = h.get_sobol_index(0)
        finally:
            h.close()
        if path is None:
            return None
        return [[float(px), float(py)] for px, py in path]

    # drawing helpers of the reference (rrt_04:1155-1194); animation happens after the fact
    def draw_graph(self, rnd=None):  # pragma: no cover
        import matplotlib.pyplot as plt
        plt.clf()
        if rnd is not None:
            plt.plot(rnd.x, rnd.y, "^k")
        for node in self.node_list:
            if node.parent:
                plt.plot(node.path_x, node.path_y, "-g")
        for (ox, oy, size) in self.obstacle_list:
            self.plot_circle(ox, oy, size)
        if self.play_area is not None:
            pa = self.play_area
            plt.plot([pa.xmin, pa.xmax, pa.xmax, pa.xmin, pa.xmin], [pa.ymin, pa.ymin, pa.ymax, pa.ymax, pa.ymin], "-k")
        plt.plot(self.start.x, self.start.y, "xr")
        plt.plot(self.end.x, self.end.y, "xr")
        plt.axis("equal")
        plt.grid(True)

    @staticmethod
    def plot_circle(x, y, size, color="-b"):  # pragma: no cover
        import matplotlib.pyplot as plt
        deg = list(range(0, 360, 5)) + [0]
        plt.plot([x + size * math.cos(np.deg2rad(d)) for d in deg],
                 [y + size * math.sin(np.deg2rad(d)) for d in deg], color)

    def calc_dist_to_goal(self, x, y):
        return math.hypot(x - self.end.x, y - self.end.y)


class RRT(_PlannerBase):
    """Drop-in for rrt_01's `RRT` (10_path_planning_01_rrt_01_simple.py:16-101)."""
    _ALGO = _abi.ALGO_RRT

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, device=0):
        self._common_init(start, goal, obstacle_list, rand_area, expand_dis, path_resolution, goal_sample_rate,
                          max_iter, play_area, robot_radius, device)

    def planning(self, animation=True):
        path = self._run(_abi.SAMPLER_MT, 50.0, False)
        if animation:  # pragma: no cover
            self.draw_graph()
        return path

    plan = planning


class RRTSobol(RRT):
    """Drop-in for rrt_02's `RRT` (10_path_planning_01_rrt_02_sobol_sampler.py:932-1089): rrt_01 whose
    get_random_node draws the 2-D Sobol sequence (:1077-1089)."""

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, device=0):
        super().__init__(start, goal, obstacle_list, rand_area, expand_dis, path_resolution, goal_sample_rate, max_iter,
                         play_area, robot_radius, device)
        self.sobol_inter_ = 0

    def planning(self, animation=True):
        path = self._run(_abi.SAMPLER_SOBOL, 50.0, False)
        if animation:  # pragma: no cover
            self.draw_graph()
        return path

    plan = planning


class RRTStar(_PlannerBase):
    """Drop-in for rrt_04's `RRT` (10_path_planning_01_rrt_04_rrt_star.py:932-1384)."""
    _ALGO = _abi.ALGO_RRT_STAR

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, sobol_sampler=True,
                 connect_circle_dist=50.0, search_until_max_iter=False, device=0):
        self._common_init(start, goal, obstacle_list, rand_area, expand_dis, path_resolution, goal_sample_rate,
                          max_iter, play_area, robot_radius, device)
        self.sobol_sampler = sobol_sampler
        self.sobol_inter_ = 0
        self.connect_circle_dist = connect_circle_dist
        self.goal_node = Node(goal[0], goal[1])
        self.search_until_max_iter = search_until_max_iter

    def planning(self, animation=True):
        path = self._run(_abi.SAMPLER_SOBOL if self.sobol_sampler else _abi.SAMPLER_MT, self.connect_circle_dist,
                         self.search_until_max_iter)
        if animation:  # pragma: no cover
            self.draw_graph()
        return path

    plan = planning


class InformedNode:
    """rrt_07's top-level Node (:1020-1025): integer parent index, no path arrays."""

    def __init__(self, x, y):
        self.x = x
        self.y = y
        self.cost = 0.0
        self.parent = None


def informed_rotation(start_xy, goal_xy):
    """c_min and the rotation-to-world matrix `c`, computed with numpy exactly as rrt_07:1054-1068 does."""
    c_min = math.hypot(start_xy[0] - goal_xy[0], start_xy[1] - goal_xy[1])
    a1 = np.array([[(goal_xy[0] - start_xy[0]) / c_min], [(goal_xy[1] - start_xy[1]) / c_min], [0]])
    id1_t = np.array([1.0, 0.0, 0.0]).reshape(1, 3)
    m = a1 @ id1_t
    u, s, vh = np.linalg.svd(m, True, True)
    c = u @ np.diag([1.0, 1.0, np.linalg.det(u) * np.linalg.det(np.transpose(vh))]) @ vh
    return c_min, c


class InformedRRTStar:
    """Drop-in for rrt_07's `RRT` (10_path_planning_01_rrt_07_informed_rrt_star.py:1027-1285)."""

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=0.5, goal_sample_rate=10, max_iter=200,
                 sobol_sampler=False, device=0):
        self.start = InformedNode(start[0], start[1])
        self.goal = InformedNode(goal[0], goal[1])
        self.min_rand = rand_area[0]
        self.max_rand = rand_area[1]
        self.expand_dis = expand_dis
        self.goal_sample_rate = goal_sample_rate
        self.max_iter = max_iter
        self.obstacle_list = obstacle_list
        self.node_list = None
        self.sobol_sampler = sobol_sampler
        self.sobol_inter_ = 0
        self.device = device
        self.stats = None
        self._trace = False
        self.trace = None

    def informed_rrt_star_search(self, animation=True):
        c_min, c = informed_rotation([self.start.x, self.start.y], [self.goal.x, self.goal.y])
        h = _abi.Handle(_abi.ALGO_INFORMED, [self.start.x, self.start.y], [self.goal.x, self.goal.y],
                        [self.min_rand, self.max_rand], self.expand_dis, 1.0, self.goal_sample_rate, self.max_iter,
                        sampler=_abi.SAMPLER_SOBOL if self.sobol_sampler else _abi.SAMPLER_MT, n_instances=1,
                        device=self.device, informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
        try:
            h.set_obstacles(self.obstacle_list)
            st = random.getstate()
            h.set_rng_state(0, st)
            if self._trace:
                h.enable_trace(0)
            h.plan(strict=True)
            random.setstate(h.get_rng_state(0, st[2]))
            x, y, cost, parent = h.get_tree(0)
            nodes = []
            for i in range(len(x)):
                nd = InformedNode(float(x[i]), float(y[i]))
                nd.cost = float(cost[i])
                nd.parent = None if parent[i] < 0 else int(parent[i])
                nodes.append(nd)
            self.node_list = nodes
            self.tree = (x, y, cost, parent)
            path = h.get_path(0)
            self.stats = h.get_stats()
            if self._trace:
                self.trace = h.get_trace()
            if self.sobol_sampler:
                self.sobol_inter_ = h.get_sobol_index(0)
        finally:
            h.close()
        return None if path is None else [[float(px), float(py)] for px, py in path]

    plan = informed_rrt_star_search

    @staticmethod
    def get_path_len(path):
        return get_path_length(path)


class DubinsNode:
    """rrt_05's RRT.Node (:1336-1349): pose + the sampled polyline of the edge from its parent."""

    def __init__(self, x, y, yaw):
        self.x = x
        self.y = y
        self.path_x = []
        self.path_y = []
        self.parent = None
        self.cost = 0.0
        self.yaw = yaw
        self.path_yaw = []


class RRTStarDubins:
    """Drop-in for rrt_05's `RRT` (10_path_planning_01_rrt_05_rrt_star_dubins_path.py:1335-1795).

    `planning(animation, search_until_max_iter=True)` as the reference's driver calls it; the sampler is always
    pseudo-random (the reference never calls its Sobol variant, :1426) and edge costs are Euclidean (:1777)."""
    Node = DubinsNode
    AreaBounds = AreaBounds

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, sobol_sampler=True,
                 connect_circle_dist=50.0, search_until_max_iter=False, curvature=1.0,
                 goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, device=0):
        self.start = DubinsNode(start[0], start[1], start[2])
        self.end = DubinsNode(goal[0], goal[1], goal[2])
        self.min_rand = rand_area[0]
        self.max_rand = rand_area[1]
        self.play_area = AreaBounds(play_area) if play_area is not None else None
        self.expand_dis = expand_dis
        self.path_resolution = path_resolution
        self.goal_sample_rate = goal_sample_rate
        self.max_iter = max_iter
        self.obstacle_list = obstacle_list
        self.node_list = []
        self.robot_radius = robot_radius
        self.sobol_sampler = sobol_sampler
        self.sobol_inter_ = 0
        self.connect_circle_dist = connect_circle_dist
        self.search_until_max_iter = search_until_max_iter
        self.curvature = curvature
        self.goal_yaw_th = goal_yaw_th
        self.goal_xy_th = goal_xy_th
        self.device = device
        self.stats = None
        self._trace = False
        self.trace = None

    def planning(self, animation=True, search_until_max_iter=True):
        h = self._make_handle(bool(search_until_max_iter))
        try:
            self._load_obstacles(h)
            st = random.getstate()
            h.set_rng_state(0, st)
            if self._trace:
                h.enable_trace(0)
            h.plan(strict=True)
            random.setstate(h.get_rng_state(0, st[2]))
            x, y, cost, parent = h.get_tree(0)
            yaw = h.get_yaw(0)
            plen, px, py = h.get_polylines(0)
            nodes, off = [], 0
            for i in range(len(x)):
                nd = DubinsNode(float(x[i]), float(y[i]), float(yaw[i]))
                nd.cost = float(cost[i])
                nd.path_x = px[off:off + plen[i]]
                nd.path_y = py[off:off + plen[i]]
                off += int(plen[i])
                nodes.append(nd)
            for i, nd in enumerate(nodes):
                nd.parent = nodes[int(parent[i])] if parent[i] >= 0 else None
            self.node_list = nodes
            self.tree = (x, y, cost, parent)
            self.yaw = yaw
            self.polylines = (plen, px, py)
            path = h.get_path(0)
            self.stats = h.get_stats()
            self._after_plan(h)
            if self._trace:
                self.trace = h.get_trace()
        finally:
            h.close()
        return None if path is None else [[float(a), float(b)] for a, b in path]

    plan = planning

    def _make_handle(self, until_max=True):
        return _abi.Handle(_abi.ALGO_DUBINS, [self.start.x, self.start.y, self.start.yaw],
                           [self.end.x, self.end.y, self.end.yaw], [self.min_rand, self.max_rand], self.expand_dis,
                           self.path_resolution, self.goal_sample_rate, self.max_iter, robot_radius=self.robot_radius,
                           connect_circle_dist=self.connect_circle_dist, search_until_max_iter=until_max, n_instances=1,
                           device=self.device, curvature=self.curvature, goal_yaw_th=self.goal_yaw_th,
                           goal_xy_th=self.goal_xy_th)

    def _after_plan(self, h):
        pass

    def _load_obstacles(self, h):
        h.set_obstacles(self.obstacle_list)   # the Dubins planners keep the tile


class RRTDubins(RRTStarDubins):
    """Drop-in for rrt_03's `RRT` (10_path_planning_01_rrt_03_dubins_path.py:1348-1700): RRT whose steer is the whole
    Dubins path to the sample, node cost = Dubins length (:1458-1481).  `sobol_sampler=True` (the driver's setting)
    draws the 3-D Sobol point of :1545-1563.  As shipped that script stops at import (its word table :1030 names
    functions defined later); the behaviour mirrored here is the one its classes define, pinned by goldens generated
    with that one assignment evaluated after the definitions (oracle/ref_loader.py)."""

    def __init__(self, start, goal, obstacle_list, rand_area, goal_sample_rate=10, max_iter=200, play_area=None,
                 robot_radius=0.0, sobol_sampler=False, curvature=1.0, goal_yaw_th=float(np.deg2rad(1.0)),
                 goal_xy_th=0.5, device=0):
        super().__init__(start, goal, obstacle_list, rand_area, goal_sample_rate=goal_sample_rate, max_iter=max_iter,
                         play_area=play_area, robot_radius=robot_radius, sobol_sampler=sobol_sampler,
                         curvature=curvature, goal_yaw_th=goal_yaw_th, goal_xy_th=goal_xy_th, device=device)

    def _make_handle(self, until_max=True):
        return _abi.Handle(_abi.ALGO_RRT_DUBINS, [self.start.x, self.start.y, self.start.yaw],
                           [self.end.x, self.end.y, self.end.yaw], [self.min_rand, self.max_rand], 0.0, 0.5,
                           self.goal_sample_rate, self.max_iter,
                           play_area=None if self.play_area is None else [self.play_area.xmin, self.play_area.xmax,
                                                                          self.play_area.ymin, self.play_area.ymax],
                           robot_radius=self.robot_radius,
                           sampler=_abi.SAMPLER_SOBOL if self.sobol_sampler else _abi.SAMPLER_MT,
                           search_until_max_iter=until_max, n_instances=1, device=self.device, curvature=self.curvature,
                           goal_yaw_th=self.goal_yaw_th, goal_xy_th=self.goal_xy_th)

    def _after_plan(self, h):
        if self.sobol_sampler:
            self.sobol_inter_ = h.get_sobol_index(0)


class RRTStarReedsShepp(RRTStarDubins):
    """Drop-in for rrt_06's `RRT` (10_path_planning_01_rrt_06_rrt_star_reeds_shepp_path.py:1444-1914): RRT* whose steer
    is the whole Reeds-Shepp path to the sample (:1584-1604), with `try_goal_path` (:1572-1582) after every accepted
    node.  `planning(animation, search_until_max_iter=True)` as the driver calls it (:2087: the constructor's
    `search_until_max_iter` is not read by the loop); the sampler is always `get_random_node` (:1539) and edge costs in
    choose_parent / rewire are Euclidean (the last-defined calc_new_cost, :1901).  Returns the three-column course
    `[[x, y, yaw], ...]` of generate_final_course (:1643-1651)."""

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, sobol_sampler=True,
                 connect_circle_dist=50.0, search_until_max_iter=False, curvature=1.0,
                 goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=0.2, device=0):
        super().__init__(start, goal, obstacle_list, rand_area, expand_dis=expand_dis, path_resolution=path_resolution,
                         goal_sample_rate=goal_sample_rate, max_iter=max_iter, play_area=play_area,
                         robot_radius=robot_radius, sobol_sampler=sobol_sampler, connect_circle_dist=connect_circle_dist,
                         search_until_max_iter=search_until_max_iter, curvature=curvature, goal_yaw_th=goal_yaw_th,
                         goal_xy_th=goal_xy_th, device=device)
        self.step_size = step_size
        self.path_yaw = None
        # How planning() hands over obstacle_list (rrt_06, and rrt_10 below): None = through the obstacle map when the list
        # has more than 64 circles, the Reeds-Shepp tile (rrtx_set_obstacle_map: any number up to 2**20), True = always,
        # False = never, which fails beyond 64.  An attribute, set after construction: the constructors keep the
        # reference's signatures.
        self.obstacle_map = None

    def _load_obstacles(self, h):
        h.load_obstacles(self.obstacle_list, _abi.use_obstacle_map(self.obstacle_map, len(self.obstacle_list),
                                                                   _abi.OBSTACLE_TILE_MAX_RS))

    def planning(self, animation=True, search_until_max_iter=True):
        self.path_yaw = None
        path = super().planning(animation, search_until_max_iter)
        if path is None:
            return None
        return [[p[0], p[1], float(w)] for p, w in zip(path, self.path_yaw)]

    plan = planning

    def _make_handle(self, until_max=True):
        return _abi.Handle(_abi.ALGO_RS, [self.start.x, self.start.y, self.start.yaw],
                           [self.end.x, self.end.y, self.end.yaw], [self.min_rand, self.max_rand], self.expand_dis,
                           self.path_resolution, self.goal_sample_rate, self.max_iter, robot_radius=self.robot_radius,
                           connect_circle_dist=self.connect_circle_dist, search_until_max_iter=until_max, n_instances=1,
                           device=self.device, curvature=self.curvature, goal_yaw_th=self.goal_yaw_th,
                           goal_xy_th=self.goal_xy_th, step_size=self.step_size)

    def _after_plan(self, h):
        self.path_yaw = h.get_path_yaw(0)


class ClosedLoopRRTStar(RRTStarReedsShepp):
    """Drop-in for rrt_10's `ClosedLoopRRTStar` (10_path_planning_01_rrt_10_closed_loop_rrt_star.py:1453-1582).

    Tree phase: rrt_10's `RRTStarReedsShepp` (:1005-1207) on the Reeds-Shepp kernel -- always `get_random_node`, no
    `expand_dis` (the near radius is not clamped, :522-531), curvature / goal thresholds fixed at 1.0 / 1 deg / 0.5, and
    choose_parent / rewire / cost propagation with the Reeds-Shepp length of the edge (its calc_new_cost, :1153-1161).
    Closed-loop stage (:1495-1582): every node within xy_th / yaw_th of the goal is tracked by the pure-pursuit / PID
    unicycle on the device (csrc/rrt_track.hip.h) and the feasible roll-out with the smallest end time is returned.
    `planning(animation=True)` returns `flag, x, y, yaw, v, t, a, d` as Python lists, or `(False, None, ...)`.  The model
    constants are module globals in the reference (:1592-1607); here they are optional keywords with those defaults.
    Consumes and leaves CPython's global `random` state exactly as the reference does.  `node_list` holds x, y, yaw,
    cost, parent and path_x / path_y per node; `path_yaw` (which the reference's nodes also carry) is not read back."""

    def __init__(self, start, goal, obstacle_list, rand_area, max_iter=200, connect_circle_dist=50.0, robot_radius=0.0,
                 target_speed=10.0 / 3.6, yaw_th=np.deg2rad(3.0), xy_th=0.5, invalid_travel_ratio=5.0, dt=0.05, L=0.9,
                 steer_max=np.deg2rad(40.0), accel_max=5.0, Kp=2.0, Lf=0.5, T=100.0, goal_dis=0.5, stop_speed=0.5,
                 device=0):
        super().__init__(start, goal, obstacle_list, rand_area, expand_dis=float("inf"), max_iter=max_iter,
                         connect_circle_dist=connect_circle_dist, robot_radius=robot_radius, curvature=1.0,
                         goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=0.2, device=device)
        del self.expand_dis    # rrt_10's class has no such attribute (:1020-1047)
        self.target_speed = target_speed
        self.yaw_th = yaw_th
        self.xy_th = xy_th
        self.invalid_travel_ratio = invalid_travel_ratio
        self.model = dict(dt=dt, L=L, steer_max=steer_max, accel_max=accel_max, Kp=Kp, Lf=Lf, T=T, goal_dis=goal_dis,
                          stop_speed=stop_speed)
        self.candidates = None
        self.records = None
        self.outcome = None

    def _make_handle(self, until_max=True):
        h = _abi.Handle(_abi.ALGO_RS, [self.start.x, self.start.y, self.start.yaw],
                        [self.end.x, self.end.y, self.end.yaw], [self.min_rand, self.max_rand], float("inf"), 0.5, 0,
                        self.max_iter, robot_radius=self.robot_radius, connect_circle_dist=self.connect_circle_dist,
                        search_until_max_iter=True, n_instances=1, device=self.device, curvature=1.0,
                        goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=self.step_size)
        h.set_rs_cost(_abi.RS_COST_PATH)
        return h

    def _track_kwargs(self):
        kw = dict(target_speed=self.target_speed, yaw_th=self.yaw_th, xy_th=self.xy_th,
                  invalid_travel_ratio=self.invalid_travel_ratio)
        kw.update(self.model)
        return kw

    def _after_plan(self, h):
        self.path_yaw = h.get_path_yaw(0)
        rc = h.track_planned(**self._track_kwargs())
        self.outcome = h.get_track_outcome(0)
        if rc == _abi.RRTX_PARTIAL:
            raise _abi.RrtxError("ClosedLoopRRTStar: tracking stopped with status %d (4: a course beyond the device "
                                 "capacity, 32: the reference raises here, 16: outside the arithmetic replicas' domain)"
                                 % self.outcome["status"])
        self.candidates, self.records = h.get_track_records(0)
        self._arrays = h.get_track_arrays(0)

    def planning(self, animation=True):
        self._arrays = None
        RRTStarDubins.planning(self, animation, True)
        if self._arrays is None:
            return False, None, None, None, None, None, None, None
        x, y, yaw, v, t, a, d = ([float(q) for q in arr] for arr in self._arrays)
        return True, x, y, yaw, v, t, a, d

    plan = planning

    def get_goal_indexes(self):
        return [int(i) for i in self.candidates]


class LQRNode:
    """LQRRRTStar.Node (rrt_09:1042-1051)."""

    def __init__(self, x, y):
        self.x = x
        self.y = y
        self.path_x = []
        self.path_y = []
        self.parent = None
        self.cost = 0.0


_lqr_checked = []


def lqr_matmul_check():
    """The device restates numpy's `A @ x` of the LQR model (rrt_09:960) with row 0 fused (csrc/rpp_lqr.h).  Compares
    this host's numpy with that form on a few fixed states, once per process; warns (RrtxParityWarning) on a mismatch:
    the planner then still runs, but matches the reference run on this host only up to those roundings."""
    if _lqr_checked:
        return _lqr_checked[0]
    from fractions import Fraction
    A = np.array([[0.1, 1.0], [0.0, 0.1]])
    bad = 0
    rs = np.random.RandomState(12345)
    for _ in range(64):
        x = rs.uniform(-20.0, 20.0, 2) * (10.0 ** rs.randint(-6, 2, 2))
        got = (A @ x.reshape(2, 1))[0, 0]
        want = float(Fraction(0.1) * Fraction(float(x[0])) + Fraction(float(x[1])))
        bad += got != want
    _lqr_checked.append(bad)
    if bad:
        import warnings
        warnings.warn("this host's numpy rounds the LQR model's A @ x unfused in %d of 64 states; LQRRRTStar matches the "
                      "reference only where it rounds fused (csrc/rpp_lqr.h)" % bad, _abi.RrtxParityWarning)
    return bad


class LQRRRTStar:
    """Drop-in for rrt_09's `LQRRRTStar` (10_path_planning_01_rrt_09_lqr_rrt_star.py:1041-1450): RRT* whose steer is an
    LQR rollout to the target, resampled at `step_size` (csrc/rpp_lqr.h).  `planning(animation, search_until_max_iter=True)`
    as the reference defines it (:1120): the method's keyword, not the constructor's, decides the early exit.
    `node_list` is filled lazily after planning (x, y, cost, parent, path_x / path_y regenerated from each node's edge
    record); `draw_graph` draws after the fact.  Where the reference raises (an LQR rollout that never reaches its
    target: IndexError at :1184) planning raises RrtxError."""
    Node = LQRNode
    AreaBounds = AreaBounds

    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5, goal_sample_rate=10,
                 max_iter=500, play_area=None, robot_radius=0.0, sobol_sampler=True, connect_circle_dist=50.0,
                 search_until_max_iter=False, curvature=1.0, goal_xy_th=0.5, step_size=0.2, device=0):
        self.start = LQRNode(start[0], start[1])
        self.end = LQRNode(goal[0], goal[1])
        self.min_rand = rand_area[0]
        self.max_rand = rand_area[1]
        self.play_area = AreaBounds(play_area) if play_area is not None else None
        self._play_area_arg = play_area
        self.expand_dis = expand_dis
        self.path_resolution = path_resolution
        self.goal_sample_rate = goal_sample_rate
        self.max_iter = max_iter
        self.obstacle_list = obstacle_list
        self.node_list = []
        self.robot_radius = robot_radius
        self.sobol_sampler = sobol_sampler
        self.sobol_inter_ = 0
        self.connect_circle_dist = connect_circle_dist
        self.goal_node = LQRNode(goal[0], goal[1])
        self.search_until_max_iter = search_until_max_iter
        self.curvature = curvature
        self.goal_xy_th = goal_xy_th
        self.step_size = step_size
        self.device = device
        self.stats = None
        self._trace = False
        self.trace = None

    def planning(self, animation=True, search_until_max_iter=True):
        lqr_matmul_check()
        h = _abi.Handle(_abi.ALGO_LQR_RRT_STAR, [self.start.x, self.start.y], [self.end.x, self.end.y],
                        [self.min_rand, self.max_rand], self.expand_dis, self.path_resolution, self.goal_sample_rate,
                        self.max_iter, play_area=self._play_area_arg, robot_radius=self.robot_radius,
                        sampler=_abi.SAMPLER_SOBOL if self.sobol_sampler else _abi.SAMPLER_MT,
                        connect_circle_dist=self.connect_circle_dist,
                        search_until_max_iter=bool(search_until_max_iter), n_instances=1, device=self.device,
                        goal_xy_th=self.goal_xy_th, step_size=self.step_size)
        try:
            h.set_obstacles(self.obstacle_list)
            st = random.getstate()
            h.set_rng_state(0, st)
            if self._trace:
                h.enable_trace(0)
            h.plan(strict=True)
            random.setstate(h.get_rng_state(0, st[2]))
            x, y, cost, parent = h.get_tree(0)
            plen, px, py = h.get_polylines(0)
            self.tree = (x, y, cost, parent)
            self.polylines = (plen, px, py)
            self.node_list = _LQRNodeList(x, y, cost, parent, plen, px, py)
            path = h.get_path(0)
            self.stats = h.get_stats()
            if self.sobol_sampler:
                self.sobol_inter_ = h.get_sobol_index(0)
            if self._trace:
                self.trace = h.get_trace()
        finally:
            h.close()
        if animation:  # pragma: no cover
            self.draw_graph()
        return None if path is None else [[float(a), float(b)] for a, b in path]

    plan = planning

    def draw_graph(self, rnd=None):  # pragma: no cover
        _PlannerBase.draw_graph(self, rnd)

    plot_circle = _PlannerBase.plot_circle

    def calc_dist_to_goal(self, x, y):
        return math.hypot(x - self.end.x, y - self.end.y)


class _LQRNodeList:
    """Lazy node_list of LQRRRTStar: LQRNode objects made on first access, parents as object references."""

    def __init__(self, x, y, cost, parent, plen, px, py):
        self._x, self._y, self._cost, self._parent = x, y, cost, parent
        self._off = np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)
        self._px, self._py = px, py
        self._nodes = None

    def _build(self):
        if self._nodes is None:
            nodes = []
            for i in range(len(self._x)):
                nd = LQRNode(float(self._x[i]), float(self._y[i]))
                nd.cost = float(self._cost[i])
                a, b = int(self._off[i]), int(self._off[i + 1])
                nd.path_x = [float(v) for v in self._px[a:b]]
                nd.path_y = [float(v) for v in self._py[a:b]]
                nodes.append(nd)
            for i, nd in enumerate(nodes):
                nd.parent = nodes[int(self._parent[i])] if self._parent[i] >= 0 else None
            self._nodes = nodes
        return self._nodes

    def __len__(self):
        return len(self._x)

    def __getitem__(self, i):
        return self._build()[i]

    def __iter__(self):
        return iter(self._build())


def path_smoothing(path, max_iter, obstacle_list, device=0):
    """Drop-in for rrt_04's module function `path_smoothing(path, max_iter, obstacle_list)` (:1447-1479): random
    shortcutting of the path `planning()` returned, drawing from CPython's global `random` stream (left exactly where
    the reference would leave it).  Runs on the GPU through the C ABI; see `Handle.smooth_planned` for batches."""
    st = random.getstate()
    out, states, _ = _abi.smooth_paths([path], max_iter, obstacle_list, [(np.array(st[1][:624], dtype=np.uint32), st[1][624])],
                                       device=device)
    w, pos = states[0]
    random.setstate((st[0], tuple(int(v) for v in w) + (int(pos),), st[2]))
    return [[float(a), float(b)] for a, b in out[0]]


def bitstar_rotation(start_xy, goal_xy):
    """cMin and C of rrt_08:189-202, computed with numpy exactly as the reference does."""
    c_min = math.hypot(start_xy[0] - goal_xy[0], start_xy[1] - goal_xy[1]) / 1.5
    a1 = np.array([[(goal_xy[0] - start_xy[0]) / c_min], [(goal_xy[1] - start_xy[1]) / c_min], [0]])
    id1_t = np.array([1.0, 0.0, 0.0]).reshape(1, 3)
    m = np.dot(a1, id1_t)
    u, s, vh = np.linalg.svd(m, True, True)
    c = np.dot(np.dot(u, np.diag([1.0, 1.0, np.linalg.det(u) * np.linalg.det(np.transpose(vh))])), vh)
    return c_min, c


class BITStar:
    """Drop-in for rrt_08's `BITStar` (10_path_planning_01_rrt_08_batch_informed_rrt_star.py:138-566).
    As in the reference, `lowerLimit`, `upperLimit`, `resolution` and `eta` are accepted and ignored (:165-168)."""

    def __init__(self, start, goal, obstacleList, randArea, eta=2.0, maxIter=80, lowerLimit=None, upperLimit=None,
                 resolution=0.01, device=0):
        self.start = start
        self.goal = goal
        self.min_rand = randArea[0]
        self.max_rand = randArea[1]
        self.max_iIter = maxIter
        self.obstacleList = obstacleList
        self.eta = eta
        self.device = device
        self.stats = None
        self.tree_arrays = None
        self._trace = False
        self.trace = None

    def plan(self, animation=True):
        c_min, c = bitstar_rotation(self.start, self.goal)
        h = _abi.Handle(_abi.ALGO_BITSTAR, [self.start[0], self.start[1]], [self.goal[0], self.goal[1]],
                        [self.min_rand, self.max_rand], 2.0, 1.0, 0, self.max_iIter, n_instances=1, device=self.device,
                        informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
        try:
            h.set_obstacles(self.obstacleList)
            st = random.getstate()
            h.set_rng_state(0, st)
            if self._trace:
                h.enable_trace(0)
            h.plan(strict=True)
            random.setstate(h.get_rng_state(0, st[2]))
            self.tree_arrays = h.get_tree(0)
            path = h.get_path(0)
            self.stats = h.get_stats()
            if self._trace:
                self.trace = h.get_trace()
        finally:
            h.close()
        return [] if path is None else [[float(a), float(b)] for a, b in path]


def check_device_courses(n_handles, has_yaw, order):
    """The ValueErrors of BatchPlanner.courses(arrays="device"): what the tracker could not read on the device."""
    if n_handles != 1:
        raise ValueError("BatchPlanner.courses(arrays='device'): the batch is sharded over %d handles, the tracker reads "
                         "one handle's courses" % n_handles)
    if not has_yaw:
        raise ValueError("BatchPlanner.courses(arrays='device'): these courses have no yaw (only the planned courses of "
                         "'rrt_star_reeds_shepp' / 'closed_loop_rrt_star' do), the tracker needs (x, y, yaw)")
    if order != "driving":
        raise ValueError("BatchPlanner.courses(arrays='device'): the tracker drives the course, gather order='driving'")


def get_path_length(path):
    """rrt_04:1391-1399."""
    le = 0
    for i in range(len(path) - 1):
        le += math.hypot(path[i + 1][0] - path[i][0], path[i + 1][1] - path[i][1])
    return le


class PlannerCourses:
    """Every course of a planned batch as one CSR result (BatchPlanner.courses): course i owns rows offsets[i] ..
    offsets[i + 1] - 1 of the flat x, y and yaw (yaw is None unless the planner is "rrt_star_reeds_shepp" /
    "closed_loop_rrt_star" and the courses are the planned ones).  n_points (n,) is np.diff(offsets), found the mask
    n_points > 0, status (n,) 0 for an instance with a course and 1 (as RRTX_STEER_NO_PATH) for one without, kernel_ms the
    HIP-event time of the gather (sharded planners: the slowest handle's).
    With arrays="device" x, y and yaw are None and device_courses names the handle whose device buffers hold them:
    BatchTrack.run reads them there."""

    def __init__(self, offsets, x, y, yaw, order="planning", kernel_ms=0.0, device_courses=None):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.x, self.y, self.yaw = x, y, yaw
        self.order = order
        self.kernel_ms = kernel_ms
        self.n_points = np.diff(self.offsets)
        self.found = self.n_points > 0
        self.status = np.where(self.found, 0, 1).astype(np.int32)
        if device_courses is not None:
            self.device_courses = device_courses

    def __len__(self):
        return len(self.n_points)

    def course(self, i):
        """What BatchPlanner.path(i) returns -- (n, 2), or (n, 3) with the yaw column -- in this result's order, or None."""
        if self.x is None:
            raise ValueError("PlannerCourses.course: made with arrays='device', the points were not fetched")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        if a == b:
            return None
        cols = [self.x[a:b], self.y[a:b]] + ([] if self.yaw is None else [self.yaw[a:b]])
        return np.column_stack(cols)

    def as_csr(self):
        """(offsets, x, y): the waypoint form BatchSpline.run and BatchBSpline accept."""
        if self.x is None:
            raise ValueError("PlannerCourses.as_csr: made with arrays='device', the points were not fetched")
        return self.offsets, self.x, self.y


GOAL_QUERY_ALGOS = ("rrt_star", "rrt_star_dubins", "rrt_star_reeds_shepp")


def goal_query_table(goals, n, pose, goal_yaw):
    """The (g, 3) or (n, g, 3) table of rows (x, y, yaw) rrtx_query_goals reads, from `goals` of shape (g, 2 | 3) or
    (n, g, 2 | 3); a missing yaw column is `goal_yaw`.  Returns (table, per_instance)."""
    g = np.asarray(goals, dtype=np.float64)
    if g.ndim not in (2, 3) or g.shape[-1] not in (2, 3) or g.shape[-2] < 1:
        raise ValueError("BatchPlanner.query_goals: goals has shape (g, 2 | 3) or (n, g, 2 | 3) with g >= 1, got %r"
                         % (g.shape,))
    if g.ndim == 3 and g.shape[0] != n:
        raise ValueError("BatchPlanner.query_goals: per-instance goals for %d instances, the batch has %d" % (g.shape[0], n))
    if g.shape[-1] == 3 and not pose:
        raise ValueError("BatchPlanner.query_goals: 'rrt_star' goals are (x, y)")
    if n * g.shape[-2] > _abi.GOALQ_MAX_QUERIES:
        raise ValueError("BatchPlanner.query_goals: more than %d queries (instances x goals)" % _abi.GOALQ_MAX_QUERIES)
    t = np.empty(g.shape[:-1] + (3,), dtype=np.float64)
    t[..., :g.shape[-1]] = g
    if g.shape[-1] == 2:
        t[..., 2] = float(goal_yaw) if pose else 0.0
    return np.ascontiguousarray(t), g.ndim == 3


class GoalQueryResult:
    """What BatchPlanner.query_goals returns: for instance i and goal j the best path from i's start to goal j that i's
    planned tree holds.  node, cost, n_near, n_safe, status and found are (n, g): the answer node (-1 none), its cost
    ("rrt_star": node cost + distance to the goal; +inf without a node), the number of distinct candidates, of safe ones
    ("rrt_star" only, else 0), _abi.GOALQ_* and status == GOALQ_OK.  With paths, the courses are one CSR result over the
    n * g queries in row-major order: query i * g + j owns rows offsets[q] .. offsets[q + 1] - 1 of the flat x, y and yaw
    (yaw None unless the planner is "rrt_star_reeds_shepp"), in `order`; without, offsets, x, y and yaw are None.
    kernel_ms: HIP-event time of the solve and gather launches (sharded planners: the slowest handle's)."""

    def __init__(self, node, cost, n_near, n_safe, status, offsets=None, x=None, y=None, yaw=None, order="planning",
                 kernel_ms=0.0):
        self.node, self.cost, self.n_near, self.n_safe, self.status = node, cost, n_near, n_safe, status
        self.found = status == _abi.GOALQ_OK
        self.partial = bool(np.any(status == _abi.GOALQ_OVERFLOW))   # rrtx_query_goals returned RRTX_PARTIAL
        self.offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        self.x, self.y, self.yaw = x, y, yaw
        self.order = order
        self.kernel_ms = kernel_ms

    @property
    def shape(self):
        return self.node.shape

    def _need_paths(self, who):
        if self.offsets is None:
            raise ValueError("GoalQueryResult.%s: made with paths=False, the courses were not gathered" % who)

    def course(self, i, j):
        """The course to goal j on instance i's tree, shaped as BatchPlanner.path(i) is, in this result's order, or None."""
        self._need_paths("course")
        n, g = self.node.shape
        if not (-n <= i < n and -g <= j < g):
            raise IndexError((i, j))
        q = (i % n) * g + (j % g)
        a, b = int(self.offsets[q]), int(self.offsets[q + 1])
        if a == b:
            return None
        cols = [self.x[a:b], self.y[a:b]] + ([] if self.yaw is None else [self.yaw[a:b]])
        return np.column_stack(cols)

    def as_csr(self):
        """(offsets, x, y) over the n * g queries: the waypoint form BatchSpline.run and BatchBSpline accept."""
        self._need_paths("as_csr")
        return self.offsets, self.x, self.y


class GoalTrackResult:
    """What BatchPlanner.track_goals returns: for instance i and goal j what the tail of rrt_10's planning() returns on i's
    planned tree with `end` set to goal j.  flag, winner, node, n_cand, len, t_last, status and no_tree are (n, g): whether a
    feasible roll-out exists, the winner's position in the query's candidate list and its node (-1 none), the number of
    candidates, len(t) and t[-1] of the winner (0 and +inf without one), the RRTX_ST_* bits of a refused candidate (such a
    query has no winner) and whether the instance's tree did not finish.
    The candidates of the n * g queries (row major) are one CSR table: query q = i * g + j owns rows cand_offsets[q] ..
    cand_offsets[q + 1] - 1 of cand_node, cand_find, cand_len, cand_fail, cand_ood and cand_t_last (what
    check_tracking_path_is_feasible returned per candidate, _abi.TRACK_RECORD's columns).
    With arrays, a flagged query owns len + 1 entries at arr_offsets[q] of the flat x, y, yaw, v, t, a, d: x, y, yaw fill them
    (the goal pose last), v, t, a, d fill len and leave the last NaN; without, arr_offsets and the seven are None.
    kernel_ms: HIP-event times (list, roll + pick, store) of the launches (sharded planners: the slowest handle's).
    partial: some query carries a status (rrtx_track_goals returned RRTX_PARTIAL)."""
    ARRAYS = ("x", "y", "yaw", "v", "t", "a", "d")

    def __init__(self, outcomes, shape, cand_offsets, cand_node, records, arr_offsets=None, arrays=None, kernel_ms=(0.0, 0.0, 0.0)):
        for k in ("flag", "winner", "node", "n_cand", "len", "t_last", "status", "no_tree"):
            setattr(self, k, np.ascontiguousarray(outcomes[k]).reshape(shape))
        self.flag = self.flag.astype(bool)
        self.no_tree = self.no_tree.astype(bool)
        self.cand_offsets = np.ascontiguousarray(cand_offsets, dtype=np.int64)
        self.cand_node = cand_node
        self.cand_find, self.cand_len, self.cand_fail, self.cand_ood, self.cand_t_last = (
            np.ascontiguousarray(records[k]) for k in ("find_goal", "len", "fail", "ood", "t_last"))
        self._records = records
        self.arr_offsets = None if arr_offsets is None else np.ascontiguousarray(arr_offsets, dtype=np.int64)
        for k, name in enumerate(self.ARRAYS):
            setattr(self, name, None if arrays is None else arrays[k])
        self.kernel_ms = kernel_ms
        self.partial = bool(np.any(self.status != 0))

    @property
    def shape(self):
        return self.flag.shape

    def _query(self, i, j):
        n, g = self.flag.shape
        if not (-n <= i < n and -g <= j < g):
            raise IndexError((i, j))
        return (i % n) * g + (j % g)

    def trajectory(self, i, j):
        """(x, y, yaw, v, t, a, d) of the best feasible roll-out of instance i towards goal j (x, y, yaw one longer: the goal
        pose is appended, rrt_10:1519-1521), or None where the reference returns (False, None, ...)."""
        if self.arr_offsets is None:
            raise ValueError("GoalTrackResult.trajectory: made with arrays=False, the arrays were not stored")
        q = self._query(i, j)
        if not self.flag.reshape(-1)[q]:
            return None
        a, b = int(self.arr_offsets[q]), int(self.arr_offsets[q + 1])
        return tuple(getattr(self, name)[a:b if k < 3 else b - 1] for k, name in enumerate(self.ARRAYS))

    def records(self, i, j):
        """(candidate node indices, records as a TRACK_RECORD array) of query (i, j), in candidate order."""
        q = self._query(i, j)
        a, b = int(self.cand_offsets[q]), int(self.cand_offsets[q + 1])
        return self.cand_node[a:b], self._records[a:b]

    def best_goal(self):
        """Per instance the first goal with the smallest t_last among the flagged ones, -1 if none."""
        return np.where(self.flag.any(axis=1), np.argmin(np.where(self.flag, self.t_last, np.inf), axis=1), -1)


class BatchPlanner:
    """Many independent planning instances (seeds / start-goal pairs) on one GPU or sharded over several.

    This is the throughput form of the same kernels: instance i consumes the stream of
    `random.seed(seeds[i])` and produces exactly the tree the single-instance class would.

    `devices=[d0, d1, ...]` ("one handle per device, driven from one process with N threads"): the batch is cut
    into len(devices) contiguous blocks (`sharding.split_contiguous`), one handle per entry, planned concurrently by
    `rrtx_plan_many` (one native host thread per handle; no torch, no collective -- instances never communicate) and
    read back as ONE batch: every accessor takes the global instance index.  A device may be listed more than once
    (two handles sharing a GPU), which is also how the sharding is tested on a one-GPU box.  Results do not depend on
    the sharding."""

    def __init__(self, algo, seeds, start, goal, obstacle_list, rand_area, expand_dis=3.0, path_resolution=0.5,
                 goal_sample_rate=5, max_iter=500, play_area=None, robot_radius=0.0, sobol_sampler=False,
                 connect_circle_dist=50.0, search_until_max_iter=False, device=0, starts=None, goals=None,
                 curvature=1.0, goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=0.2, devices=None,
                 instance_obstacles=None, obstacle_map=None):
        """algo: "rrt" (rrt_01/02), "rrt_star" (rrt_04), "informed" (rrt_07: expand_dis, goal_sample_rate, max_iter,
        sobol_sampler as in its constructor :1029-1042), "bitstar" (rrt_08: max_iter = maxIter, rand_area = randArea
        :140-168), and the pose planners (start / goal = [x, y, yaw]; curvature, goal thresholds and, for Reeds-Shepp,
        step_size as in their constructors): "rrt_dubins" (rrt_03), "rrt_star_dubins" (rrt_05),
        "rrt_star_reeds_shepp" (rrt_06); "closed_loop_rrt_star" (rrt_10: start / goal poses, max_iter,
        connect_circle_dist, robot_radius as in its constructor :1458-1476; plan() grows the trees, track() runs the
        closed-loop stage); "lqr_rrt_star" (rrt_09: step_size, goal_xy_th; `search_until_max_iter` plays
        the part of planning()'s keyword of the same name, :1120).
        `starts` / `goals`: per-instance [x, y] (pose planners: [x, y, yaw]; a missing yaw keeps `start[2]` /
        `goal[2]`).  For "informed" and "bitstar" the rotation to the world frame and c_min (rrt_07:1054-1068,
        rrt_08:189-202) are computed per instance on the host with numpy, as the reference does per planner object.
        `devices`: HIP device ordinals to shard over (default: [device]).
        `instance_obstacles`: one obstacle list of (x, y, size) per instance, in place of the shared `obstacle_list`
        (which must then be None): a batch over many maps in one launch (rrtx_set_instance_obstacles).
        `obstacle_map` ("rrt", "rrt_star", "rrt_star_reeds_shepp" and "closed_loop_rrt_star" only): None = the shared list
        goes through the obstacle map when it does not fit the planner's tile -- more than 256 circles, 64 for the two
        Reeds-Shepp planners -- (rrtx_set_obstacle_map: any number up to 2**20), True = always, False = never; every shard
        builds its own map.  plan(), track() and track_goals() read it; smooth() and query_goals() are not served with a map."""
        from . import sharding
        a = {"rrt": _abi.ALGO_RRT, "rrt_star": _abi.ALGO_RRT_STAR, "rrt_dubins": _abi.ALGO_RRT_DUBINS,
             "rrt_star_dubins": _abi.ALGO_DUBINS, "rrt_star_reeds_shepp": _abi.ALGO_RS, "informed": _abi.ALGO_INFORMED,
             "bitstar": _abi.ALGO_BITSTAR, "lqr_rrt_star": _abi.ALGO_LQR_RRT_STAR,
             "closed_loop_rrt_star": _abi.ALGO_RS}[algo]
        # rrt_10: the Reeds-Shepp tree with its own cost rule and an unclamped near radius, then track() (closed-loop stage)
        self.closed_loop = algo == "closed_loop_rrt_star"
        if self.closed_loop:
            expand_dis, search_until_max_iter, curvature = float("inf"), True, 1.0
            goal_yaw_th, goal_xy_th, step_size = float(np.deg2rad(1.0)), 0.5, 0.2
        self.tracked = False
        self.seeds = list(seeds)
        if a == _abi.ALGO_LQR_RRT_STAR:
            if not step_size > 0:
                raise ValueError("BatchPlanner(lqr_rrt_star): step_size must be > 0, got %r" % (step_size,))
            if int(max_iter) < 0:
                raise ValueError("BatchPlanner(lqr_rrt_star): max_iter must be >= 0, got %r" % (max_iter,))
            if not self.seeds:
                raise ValueError("BatchPlanner(lqr_rrt_star): no seeds")
            lqr_matmul_check()
        self.pose = a in (_abi.ALGO_RRT_DUBINS, _abi.ALGO_DUBINS, _abi.ALGO_RS)
        self.algo = a
        n = len(self.seeds)
        if instance_obstacles is not None:
            if obstacle_list is not None:
                raise ValueError("BatchPlanner: give either obstacle_list or instance_obstacles, not both")
            instance_obstacles = [list(lst) for lst in instance_obstacles]
            if len(instance_obstacles) != n:
                raise ValueError("BatchPlanner: %d instance_obstacles lists for %d instances"
                                 % (len(instance_obstacles), n))
        self.instance_obstacles = instance_obstacles
        self.obstacle_list = obstacle_list
        self.has_obstacle_map = False
        self.obstacle_tile_max = _abi.OBSTACLE_TILE_MAX_RS if a == _abi.ALGO_RS else _abi.OBSTACLE_TILE_MAX
        if a in _abi.OBSTACLE_MAP_ALGOS and instance_obstacles is None:
            self.has_obstacle_map = _abi.use_obstacle_map(obstacle_map, len(obstacle_list), self.obstacle_tile_max)
        elif obstacle_map:
            raise ValueError("BatchPlanner: obstacle_map serves the shared obstacle_list of \"rrt\", \"rrt_star\", "
                             "\"rrt_star_reeds_shepp\" and \"closed_loop_rrt_star\" only")
        self.devices = [int(device)] if devices is None else [int(d) for d in devices]
        if not self.devices or n < len(self.devices):
            raise ValueError("BatchPlanner: %d instances cannot be sharded over %d handles" % (n, len(self.devices)))
        self.shards = sharding.split_contiguous(n, len(self.devices))
        rot_of = {_abi.ALGO_INFORMED: informed_rotation, _abi.ALGO_BITSTAR: bitstar_rotation}.get(a)
        self.handles = []
        try:
            for dev, (lo, hi) in zip(self.devices, self.shards):
                if a == _abi.ALGO_INFORMED:
                    c_min, c = informed_rotation(start, goal)
                    h = _abi.Handle(a, start, goal, rand_area, expand_dis, 1.0, goal_sample_rate, max_iter,
                                    sampler=_abi.SAMPLER_SOBOL if sobol_sampler else _abi.SAMPLER_MT, n_instances=hi - lo,
                                    device=dev, informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
                elif a == _abi.ALGO_BITSTAR:
                    c_min, c = bitstar_rotation(start, goal)
                    h = _abi.Handle(a, start, goal, rand_area, 2.0, 1.0, 0, max_iter, n_instances=hi - lo, device=dev,
                                    informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
                else:
                    h = _abi.Handle(a, start, goal, rand_area, expand_dis, path_resolution, goal_sample_rate, max_iter,
                                    play_area=play_area, robot_radius=robot_radius,
                                    sampler=_abi.SAMPLER_SOBOL if sobol_sampler else _abi.SAMPLER_MT,
                                    connect_circle_dist=connect_circle_dist, search_until_max_iter=search_until_max_iter,
                                    n_instances=hi - lo, device=dev, curvature=curvature, goal_yaw_th=goal_yaw_th,
                                    goal_xy_th=goal_xy_th, step_size=step_size)
                self.handles.append(h)
                if self.closed_loop:
                    h.set_rs_cost(_abi.RS_COST_PATH)
                if instance_obstacles is None:
                    h.load_obstacles(obstacle_list, self.has_obstacle_map)
                else:
                    h.set_instance_obstacles(instance_obstacles[lo:hi])
                h.seed_instances(self.seeds[lo:hi])
                if starts is not None or goals is not None:
                    for i in range(lo, hi):
                        si = start if starts is None else starts[i]
                        gi = goal if goals is None else goals[i]
                        h.set_instance(i - lo, None if starts is None else si, None if goals is None else gi)
                        if rot_of is not None:
                            cm, ci = rot_of(si, gi)
                            h.set_instance_rotation(i - lo, [ci[0, 0], ci[0, 1], ci[1, 0], ci[1, 1]], cm)
        except Exception:
            self.close()
            raise
        self.h = self.handles[0]      # the single-device form's handle (kept for callers that reach for it)
        self.partial = False

    def _loc(self, i):
        """(handle, local index) of global instance i."""
        if i < 0:
            i += len(self.seeds)
        for h, (lo, hi) in zip(self.handles, self.shards):
            if lo <= i < hi:
                return h, i - lo
        raise IndexError(i)

    def plan(self):
        """Plans every instance; returns (path_cost, n_nodes, status) per instance.  An instance that stopped on a
        capacity limit or where the reference would raise carries the bit in its status word (`failed()` lists
        them); the other instances are complete.  Raises only for errors of the call as a whole."""
        rcs = _abi.plan_many(self.handles)
        self.tracked = False
        self.partial = any(r == _abi.RRTX_PARTIAL for r in rcs)
        return self.results()

    def results(self):
        """(path_cost, n_nodes, status) of the whole batch, shards concatenated in instance order."""
        parts = [h.get_results() for h in self.handles]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))

    def failed(self):
        """Indices of the instances without a result after plan(), with their status words."""
        _, _, st = self.results()
        return [(int(i), int(st[i])) for i in np.nonzero(st & _abi.ST_FAILED)[0]]

    def stats(self):
        """rrtx_stats summed over the shards (times: the slowest shard's; maxima: the largest)."""
        per = [h.get_stats() for h in self.handles]
        if len(per) == 1:
            return per[0]
        out = {}
        for k in per[0]:
            v = [p[k] for p in per]
            out[k] = max(v) if k in ("kernel_ms", "plan_ms", "kernel_ms_main", "near_unique_max", "main_shape", "main_f32") else sum(v)
        out["per_shard"] = per
        return out

    def tree(self, i):
        h, j = self._loc(i)
        return h.get_tree(j)

    def path(self, i):
        """The course `planning()` returns: (n, 2), or (n, 3) with the yaw column for "rrt_star_reeds_shepp"."""
        h, j = self._loc(i)
        p = h.get_path(j)
        if p is not None and self.algo == _abi.ALGO_RS:
            p = np.column_stack([p, h.get_path_yaw(j)])
        return p

    def yaw(self, i):
        h, j = self._loc(i)
        return h.get_yaw(j)

    def polylines(self, i):
        h, j = self._loc(i)
        return h.get_polylines(j)

    def rng_state(self, i):
        h, j = self._loc(i)
        return h.get_rng_state(j)

    def courses(self, which="planned", order="planning", arrays=True):
        """Every course of the batch from one gather per handle on the device (rrtx_gather_courses): a PlannerCourses.
        which: "planned" (what path(i) returns) or "smoothed" (what smooth() returned; after smooth()); order: "planning"
        (goal -> start, as planning() returns it) or "driving" (the same rows reversed, what BatchTrack drives).
        arrays="device": only the counts are fetched and the result carries device_courses for BatchTrack.run -- one
        handle only, and only courses with a yaw in driving order (ValueError otherwise)."""
        w = {"planned": _abi.COURSE_PLANNED, "smoothed": _abi.COURSE_SMOOTHED}.get(which)
        o = {"planning": _abi.ORDER_PLANNING, "driving": _abi.ORDER_DRIVING}.get(order)
        if w is None or o is None:
            raise ValueError("BatchPlanner.courses: which is 'planned' or 'smoothed', order 'planning' or 'driving'")
        device = _abi.on_device(arrays)
        if device:
            check_device_courses(len(self.handles), w == _abi.COURSE_PLANNED and self.algo == _abi.ALGO_RS, order)
        elif arrays is not True:
            raise ValueError("BatchPlanner.courses: arrays is True or 'device'")
        offs, cols, ms, base = [np.zeros(1, dtype=np.int64)], [], 0.0, 0
        for h in self.handles:
            h.gather_courses(w, o)
            off, n, has_yaw, kms = h.get_course_counts()
            offs.append(off[1:] + base)
            base += n
            ms = max(ms, kms)
            if not device:
                cols.append(h.get_courses(n, has_yaw))
        offsets = np.concatenate(offs)
        if device:
            return PlannerCourses(offsets, None, None, None, order, ms, _abi.DeviceCourses(_abi.SRC_PLANNER, self.handles[0]))
        x, y = (np.concatenate([c[k] for c in cols]) for k in range(2))
        yaw = None if cols[0][2] is None else np.concatenate([c[2] for c in cols])
        return PlannerCourses(offsets, x, y, yaw, order, ms)

    def query_goals(self, goals, goal_xy_th=None, goal_yaw_th=None, paths=True, order="planning"):
        """After plan(): the best path from every instance's start to MANY goals, read off the planned trees on the device
        (rrtx_query_goals) -- for instance i and goal g what the tail of the reference's planning() returns on i's
        finished node_list with `end` (rrt_04: and `goal_node`) set to g.  Nothing of the plan changes.
        goals: (g, 2 | 3) shared by all instances, or (n, g, 2 | 3); a missing yaw is the planner's goal yaw.
        goal_xy_th / goal_yaw_th: the pose planners' thresholds for this call (default: the planner's).  paths=False:
        only the records, no gather.  order: "planning" (goal -> start) or "driving".  Returns a GoalQueryResult; a query
        with more than _abi.GOALQ_MAX_CANDIDATES distinct candidates has status GOALQ_OVERFLOW and no node (the
        result's `partial` is then True).  Served for "rrt_star", "rrt_star_dubins" and "rrt_star_reeds_shepp" (ValueError otherwise)."""
        if getattr(self, "has_obstacle_map", False):
            raise ValueError("BatchPlanner.query_goals: not served with an obstacle map (more than %d obstacles, or "
                             "obstacle_map=True): it reads the obstacle tile"
                             % getattr(self, "obstacle_tile_max", _abi.OBSTACLE_TILE_MAX))
        if self.algo not in (_abi.ALGO_RRT_STAR, _abi.ALGO_DUBINS, _abi.ALGO_RS) or getattr(self, "closed_loop", False):
            raise ValueError("BatchPlanner.query_goals: served for %s only (every other planner has another goal rule)"
                             % ", ".join(repr(a) for a in GOAL_QUERY_ALGOS))
        o = {"planning": _abi.ORDER_PLANNING, "driving": _abi.ORDER_DRIVING}.get(order)
        if o is None:
            raise ValueError("BatchPlanner.query_goals: order is 'planning' or 'driving'")
        n = len(self.seeds)
        pose = self.algo != _abi.ALGO_RRT_STAR
        table, per_instance = goal_query_table(goals, n, pose, self.handles[0].params.goal[2] if pose else 0.0)
        recs, offs, cols, ms, base = [], [np.zeros(1, dtype=np.int64)], [], 0.0, 0
        for h, (lo, hi) in zip(self.handles, self.shards):
            rc, g = h.query_goals(table[lo:hi] if per_instance else table, per_instance, goal_xy_th, goal_yaw_th)
            recs.append(h.get_goal_query(g))
            if paths:
                h.gather_goal_courses(o)
                off, x, y, yaw = h.get_goal_courses(g)
                offs.append(off[1:] + base)
                base += int(off[-1])
                cols.append((x, y, yaw))
            ms = max(ms, sum(h.get_goal_query_kernel_ms()))
        node, cost, near, safe, st = (np.concatenate([r[k] for r in recs]) for k in range(5))
        if not paths:
            return GoalQueryResult(node, cost, near, safe, st, order=order, kernel_ms=ms)
        x, y = (np.concatenate([c[k] for c in cols]) for k in range(2))
        yaw = None if cols[0][2] is None else np.concatenate([c[2] for c in cols])
        return GoalQueryResult(node, cost, near, safe, st, np.concatenate(offs), x, y, yaw, order, ms)

    def smooth(self, max_iter):
        """path_smoothing(path, max_iter, obstacle_list) (rrt_04:1447-1479) on every planned path, on the device, each
        instance continuing its own random stream (as the driver does at :1558-1559), against its own obstacle list."""
        if getattr(self, "has_obstacle_map", False):
            raise ValueError("BatchPlanner.smooth: not served with an obstacle map (more than %d obstacles, or "
                             "obstacle_map=True): it reads the obstacle tile"
                             % getattr(self, "obstacle_tile_max", _abi.OBSTACLE_TILE_MAX))
        for h in self.handles:
            h.smooth_planned(max_iter)
        c = self.courses("smoothed")
        return [c.course(i) for i in range(len(self.seeds))]

    def track(self, **kw):
        """"closed_loop_rrt_star" only, after plan(): the closed-loop stage of rrt_10 (:1495-1582) on every planned tree, on
        the device.  Keywords: target_speed, yaw_th, xy_th, invalid_travel_ratio and the model constants (defaults: the
        reference's, _abi.TRACK_DEFAULTS).  Returns the per-instance flags; see trajectory(i) / track_records(i)."""
        if not self.closed_loop:
            raise ValueError("BatchPlanner.track: only for algo=\"closed_loop_rrt_star\"")
        if len(self.handles) == 1:
            self.handles[0].track_planned(**kw)
        else:   # one host thread per shard, as rrtx_plan_many does for the trees (the calls block on their own streams)
            import threading
            errs = []

            def run(h):
                try:
                    h.track_planned(**kw)
                except Exception as e:   # noqa: BLE001 -- re-raised below on the calling thread
                    errs.append(e)
            th = [threading.Thread(target=run, args=(h,)) for h in self.handles]
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errs:
                raise errs[0]
        self.tracked = True
        return np.array([self._loc(i)[0].get_track_outcome(self._loc(i)[1])["flag"] for i in range(len(self.seeds))],
                        dtype=bool)

    def track_goals(self, goals, arrays=True, **kw):
        """"closed_loop_rrt_star" only, after plan(): the closed-loop stage of rrt_10 for MANY goals, read off the planned
        trees on the device (rrtx_track_goals) -- for instance i and goal g what get_goal_indexes() +
        search_best_feasible_path() (:1488-1493) return on i's finished node_list with `end` set to g.  Nothing of the plan
        changes, nor do the answers of track().
        goals: (g, 2 | 3) shared by all instances, or (n, g, 2 | 3); a missing yaw is the planner's goal yaw.  arrays=False:
        records and outcomes only.  Keywords and defaults: those of track() (_abi.TRACK_DEFAULTS); xy_th / yaw_th select the
        candidates.  Returns a GoalTrackResult."""
        if not self.closed_loop:
            raise ValueError("BatchPlanner.track_goals: only for algo=\"closed_loop_rrt_star\"")
        for k in kw:
            if k not in _abi.TRACK_DEFAULTS:
                raise TypeError("BatchPlanner.track_goals: unknown keyword %r" % k)
        n = len(self.seeds)
        table, per_instance = goal_query_table(goals, n, True, self.handles[0].params.goal[2])
        parts = [None] * len(self.handles)

        def run(k, h, lo, hi):
            h.track_goals(table[lo:hi] if per_instance else table, per_instance, arrays=arrays, **kw)
            out, co, ao = h.get_goal_track()
            cand, rec = h.get_goal_track_records(int(co[-1]))
            arr = h.get_goal_track_arrays(int(ao[-1])) if arrays else None
            parts[k] = (out, co, ao, cand, rec, arr, h.get_goal_track_kernel_ms())
        if len(self.handles) == 1:
            run(0, self.handles[0], *self.shards[0])
        else:   # one host thread per shard, as track()
            import threading
            errs = []

            def guarded(*a):
                try:
                    run(*a)
                except Exception as e:   # noqa: BLE001 -- re-raised below on the calling thread
                    errs.append(e)
            th = [threading.Thread(target=guarded, args=(k, h, lo, hi)) for k, (h, (lo, hi)) in enumerate(zip(self.handles, self.shards))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errs:
                raise errs[0]
        out = np.concatenate([p[0] for p in parts])
        cand, rec = np.concatenate([p[3] for p in parts]), np.concatenate([p[4] for p in parts])
        co, ao, cb, ab = [np.zeros(1, dtype=np.int64)], [np.zeros(1, dtype=np.int64)], 0, 0
        for p in parts:
            co.append(p[1][1:] + cb)
            ao.append(p[2][1:] + ab)
            cb += int(p[1][-1])
            ab += int(p[2][-1])
        ms = tuple(max(p[6][k] for p in parts) for k in range(3))
        shape = (n, table.shape[-2])
        if not arrays:
            return GoalTrackResult(out, shape, np.concatenate(co), cand, rec, kernel_ms=ms)
        arr = [np.concatenate([p[5][k] for p in parts]) for k in range(7)]
        return GoalTrackResult(out, shape, np.concatenate(co), cand, rec, np.concatenate(ao), arr, ms)

    def polyline_yaw(self, i):
        """The pose planners on Reeds-Shepp edges: Node.path_yaw of every node of instance i, concatenated as polylines(i)
        concatenates path_x / path_y."""
        h, j = self._loc(i)
        return h.get_polyline_yaw(j)

    def trajectory(self, i):
        """(x, y, yaw, v, t, a, d) of instance i's best feasible roll-out (x, y, yaw one longer: the goal pose is
        appended, rrt_10:1519-1521), or None where planning() returns (False, None, ...)."""
        h, j = self._loc(i)
        return h.get_track_arrays(j)

    def track_outcome(self, i):
        h, j = self._loc(i)
        return h.get_track_outcome(j)

    def track_records(self, i):
        h, j = self._loc(i)
        return h.get_track_records(j)

    def export_npz(self, filename, instances=None):
        """Compact on-disk form of the planned trees for plotting / regression diffs: per instance
        (x, y, cost, parent) as the reference's node_list holds them, the returned path, path cost, seed; with
        `instance_obstacles`, each instance's list as `obstacles_k` ((m, 3): x, y, size)."""
        ids = list(range(len(self.seeds))) if instances is None else list(instances)
        pc, nn, st = self.results()
        paths = self.courses()      # one gather per handle; the yaw column is not part of the file
        out = dict(seeds=np.array([self.seeds[i] for i in ids], dtype=np.int64), path_cost=pc[ids], n_nodes=nn[ids],
                   status=st[ids])
        for k, i in enumerate(ids):
            h, j = self._loc(i)
            x, y, cost, parent = h.get_tree(j)
            p = paths.course(i)
            out["x_%d" % k], out["y_%d" % k], out["cost_%d" % k], out["parent_%d" % k] = x, y, cost, parent
            out["path_%d" % k] = np.zeros((0, 2)) if p is None else np.ascontiguousarray(p[:, :2])
            if self.closed_loop and self.tracked:
                tr = h.get_track_arrays(j)
                out["track_flag_%d" % k] = np.array(tr is not None)
                for name, arr in zip(("x", "y", "yaw", "v", "t", "a", "d"), tr if tr is not None else [np.zeros(0)] * 7):
                    out["track_%s_%d" % (name, k)] = arr
            if self.instance_obstacles is not None:
                out["obstacles_%d" % k] = np.array(self.instance_obstacles[i], dtype=np.float64).reshape(-1, 3)
        np.savez_compressed(filename, **out)
        return filename

    def close(self):
        for h in getattr(self, "handles", []):
            h.close()
