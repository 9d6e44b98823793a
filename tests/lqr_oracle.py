"""Independent pure-Python restatement of LQR-RRT* (rrt_09: 10_path_planning_01_rrt_09_lqr_rrt_star.py, LQRRRTStar
:1041-1450 with LQRPlanner :935-1033) -- TEST INFRASTRUCTURE.

It does not go through csrc/rpp_lqr.h, so a mistake shared with the device cannot hide: the fused row 0 of numpy's
`A @ x` is evaluated exactly with fractions.Fraction, lengths with CPython's own math.hypot, `** 2` with CPython's own
float power, the random stream with the interpreter's own random.Random.  Nodes keep their edge's endpoints
(from x, from y, to x, to y): the polyline of the reference's Node.path_x / path_y is regenerated from them.
"""
import math
import random
from fractions import Fraction

K = (0.0, 0.05)   # the constant dlqr gain of the reference's model (see csrc/rpp_lqr.h)


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def lqr_rollout(sx, sy, gx, gy):
    """lqr_planning :944-986: (rx, ry), or ([], []) when it never gets within GOAL_DIST."""
    rx, ry = [sx], [sy]
    x0, x1 = sx - gx, sy - gy
    time = 0.0
    while time <= 100.0:
        time += 0.1
        u = -(K[0] * x0 + K[1] * x1)
        x0, x1 = fma(0.1, x0, x1) + 0.0 * u, (0.0 * x0 + 0.1 * x1) + u
        rx.append(x0 + gx)
        ry.append(x1 + gy)
        if math.hypot(gx - rx[-1], gy - ry[-1]) <= 0.1:
            return rx, ry
    return [], []


def n_params(step):
    """len(np.arange(0.0, 1.0, step))"""
    return math.ceil(1.0 / step)


def sample_path(wx, wy, step):
    """sample_path :1157-1172"""
    px, py = [], []
    nt = n_params(step)
    for i in range(len(wx) - 1):
        for k in range(nt):
            t = k * step
            px.append(t * wx[i + 1] + (1.0 - t) * wx[i])
            py.append(t * wy[i + 1] + (1.0 - t) * wy[i])
    clen = [math.hypot(px[j + 1] - px[j], py[j + 1] - py[j]) for j in range(len(px) - 1)]
    return px, py, clen


def edge(fx, fy, tx, ty, step):
    wx, wy = lqr_rollout(fx, fy, tx, ty)
    return sample_path(wx, wy, step)


class RefRaises(Exception):
    """The reference raises IndexError at px[-1] in steer (:1184): the rollout never converged."""


class LQROracle:
    def __init__(self, start, goal, obstacle_list, rand_area, expand_dis=3.0, goal_sample_rate=10, max_iter=500,
                 play_area=None, robot_radius=0.0, sobol_sampler=True, connect_circle_dist=50.0, goal_xy_th=0.5,
                 step_size=0.2):
        self.start, self.goal = (start[0], start[1]), (goal[0], goal[1])
        self.min_rand, self.max_rand = rand_area[0], rand_area[1]
        self.expand_dis, self.goal_sample_rate, self.max_iter = expand_dis, goal_sample_rate, max_iter
        self.play_area, self.robot_radius = play_area, robot_radius
        self.sobol_sampler, self.connect_circle_dist = sobol_sampler, connect_circle_dist
        self.goal_xy_th, self.step_size = goal_xy_th, step_size
        self.obstacle_list = [tuple(o) for o in obstacle_list]

    # --- Sobol (dim 2) as i4_sobol(2, index) yields it to the planner: Gray-code steps, 30-bit direction numbers
    def _sobol(self):
        if self.sob_index == 0:
            self.lastq = [0, 0]
        l, n = 1, self.sob_index
        if n:
            while n & 1:
                n >>= 1
                l += 1
        q = [self.lastq[0] / 1073741824.0, self.lastq[1] / 1073741824.0]
        col = l - 1
        raw = 1
        for _ in range(col):
            raw ^= 2 * raw
        self.lastq[0] ^= 1 << (29 - col)
        self.lastq[1] ^= raw << (29 - col)
        self.sob_index += 1
        return q

    def _sample(self):
        if self.rng.randint(0, 100) > self.goal_sample_rate:
            if self.sobol_sampler:
                q = self._sobol()
                return (self.min_rand + q[0] * (self.max_rand - self.min_rand),
                        self.min_rand + q[1] * (self.max_rand - self.min_rand))
            return (self.rng.uniform(self.min_rand, self.max_rand), self.rng.uniform(self.min_rand, self.max_rand))
        return self.goal

    def _steer(self, i, tx, ty):
        """steer(node_list[i], (tx, ty)) :1174-1192 -> (x, y, cost, polyline, course lengths)"""
        fx, fy = self.x[i], self.y[i]
        px, py, cl = edge(fx, fy, tx, ty, self.step_size)
        if not px:
            raise RefRaises()
        return px[-1], py[-1], self.cost[i] + sum([abs(c) for c in cl]), (px, py), (fx, fy, tx, ty)

    def _collision_free(self, poly):
        px, py = poly
        for (ox, oy, size) in self.obstacle_list:
            d = [(ox - x) * (ox - x) + (oy - y) * (oy - y) for x, y in zip(px, py)]
            if min(d) <= (size + self.robot_radius) ** 2:
                return False
        return True

    def _inside(self, x, y):
        pa = self.play_area
        if pa is None:
            return True
        return not (x < float(pa[0]) or x > float(pa[1]) or y < float(pa[2]) or y > float(pa[3]))

    def _new_cost(self, i, tx, ty):
        """calc_new_cost(node_list[i], (tx, ty)) :1432-1442"""
        px, py, cl = edge(self.x[i], self.y[i], tx, ty, self.step_size)
        if not cl:
            return float("inf")
        return self.cost[i] + sum(cl)

    def _near(self, nx, ny):
        nnode = len(self.x) + 1
        r = self.connect_circle_dist * math.sqrt(math.log(nnode) / nnode)
        r = min(r, self.expand_dis)
        dl = [(x - nx) ** 2 + (y - ny) ** 2 for x, y in zip(self.x, self.y)]
        return [dl.index(d) for d in dl if d <= r ** 2]

    def _best_goal(self):
        gx, gy = self.goal
        dl = [math.hypot(x - gx, y - gy) for x, y in zip(self.x, self.y)]
        gi = [dl.index(d) for d in dl if d <= self.goal_xy_th]
        if not gi:
            return None
        mc = min([self.cost[i] for i in gi])
        for i in gi:
            if self.cost[i] == mc:
                return i
        return None

    def _propagate(self, p):
        frontier = [p]
        seen = 0
        while frontier:
            nxt = []
            for q in frontier:
                for j in range(len(self.x)):
                    if self.parent[j] == q:
                        self.cost[j] = self._new_cost(q, self.x[j], self.y[j])
                        nxt.append(j)
                        seen += 1
                        if seen > len(self.x):
                            raise RefRaises()   # a parent cycle: the reference recurses without end
            frontier = nxt

    def polyline(self, i):
        if self.parent[i] < 0:
            return [], []
        fx, fy, tx, ty = self.edges[i]
        px, py, _ = edge(fx, fy, tx, ty, self.step_size)
        return px, py

    def planning(self, rng, search_until_max_iter=True, trace=None):
        """planning(animation=False, search_until_max_iter) :1120-1155 with `rng` as the module's random."""
        self.rng = rng
        self.sob_index, self.lastq = 0, [0, 0]
        self.x, self.y, self.cost, self.parent = [self.start[0]], [self.start[1]], [0.0], [-1]
        self.edges = [(0.0, 0.0, 0.0, 0.0)]
        self.revisits = 0
        for _ in range(self.max_iter):
            rx, ry = self._sample()
            dl = [(x - rx) ** 2 + (y - ry) ** 2 for x, y in zip(self.x, self.y)]
            ni = dl.index(min(dl))
            ex, ey, ecost, poly, _ = self._steer(ni, rx, ry)
            new_node = True
            nnear = -1
            if self._collision_free(poly):
                near = self._near(ex, ey)
                nnear = len(near)
                new_node = self._choose_and_rewire(ex, ey, near)
            if trace is not None:
                trace.append((rx, ry, ni, nnear))
            if (not search_until_max_iter) and new_node:
                gi = self._best_goal()
                if gi:
                    return self._course(gi)
        gi = self._best_goal()
        if gi:
            return self._course(gi)
        return None

    def _choose_and_rewire(self, ex, ey, near):
        if not near:
            return False
        costs = []
        for i in near:
            tx, ty, _, poly, _ = self._steer(i, ex, ey)
            if self._collision_free(poly) and self._inside(tx, ty):
                costs.append(self._new_cost(i, ex, ey))
            else:
                costs.append(float("inf"))
        mc = min(costs)
        if mc == float("inf"):
            return False
        p = near[costs.index(mc)]
        nx, ny, _, _, rec = self._steer(p, ex, ey)
        self.x.append(nx)
        self.y.append(ny)
        self.cost.append(mc)
        self.parent.append(p)
        self.edges.append(rec)
        new = len(self.x) - 1
        moved = set()
        for i in near:
            if i in moved:
                self.revisits += 1
            tx, ty, _, poly, rec = self._steer(new, self.x[i], self.y[i])
            ecost = self._new_cost(new, self.x[i], self.y[i])
            if self._collision_free(poly) and self._inside(tx, ty) and self.cost[i] > ecost:
                self.x[i], self.y[i], self.cost[i], self.parent[i], self.edges[i] = tx, ty, ecost, new, rec
                moved.add(i)
                self._propagate(i)
        return True

    def _course(self, gi):
        path = [[self.goal[0], self.goal[1]]]
        i = gi
        while self.parent[i] >= 0:
            px, py = self.polyline(i)
            for a, b in zip(reversed(px), reversed(py)):
                path.append([a, b])
            i = self.parent[i]
        path.append([self.start[0], self.start[1]])
        self.goal_index = gi
        return path


def get_path_length(path):
    le = 0
    for i in range(len(path) - 1):
        le += math.hypot(path[i + 1][0] - path[i][0], path[i + 1][1] - path[i][1])
    return le
