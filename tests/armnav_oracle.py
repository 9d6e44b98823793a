"""TEST ORACLE of BatchArmNav: a plain-Python restatement of get_occupancy_grid and astar_torus of
02_arm_obstacle_navigation.py (:46-110, :113-233, :257-262) with the arithmetic forms numpy takes written out -- the 2-vector
np.linalg.norm as sqrt(fma(y, y, x * x)), the 2-vector ndarray.dot as fma(a1, b1, a0 * b0), np.cos / np.sin as math.cos /
math.sin -- and the search on integer lists.  No numpy inside the arithmetic; fma is libm's through ctypes (Python 3.10 has no
math.fma).  tests/test_armnav_host.py holds it against the reference's recorded results."""
import ctypes
import ctypes.util
import heapq
import math

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = _libm.fma
PI = math.pi


def theta_list(M):
    """:95, M + 1 entries; a cell uses the first M"""
    return [2 * i * PI / M for i in range(-M // 2, M // 2 + 1)]


def norm2(x, y):
    return math.sqrt(fma(y, y, x * x))


def dot2(a0, a1, b0, b1):
    return fma(a1, b1, a0 * b0)


def detect_collision(ax, ay, bx, by, cx, cy, radius):
    """:46-76"""
    lx, ly = bx - ax, by - ay
    mag = norm2(lx, ly)
    try:
        ux, uy = lx / mag, ly / mag
    except ZeroDivisionError:   # numpy: 0 / 0 = nan, and a NaN distance is "not > radius"
        return True
    proj = dot2(cx - ax, cy - ay, ux, uy)
    if proj <= 0:
        px, py = ax, ay
    elif proj >= mag:
        px, py = bx, by
    else:
        px, py = ax + lx * proj / mag, ay + ly * proj / mag
    return not norm2(px - cx, py - cy) > radius


def arm_points(link_lengths, t1, t2):
    """NLinkArm.update_points :257-262 after update_joints([t1, t2])"""
    pts = [(0.0, 0.0)]
    for k, L in enumerate(link_lengths):
        a = t1 if k == 0 else t1 + t2
        pts.append((pts[-1][0] + float(L) * math.cos(a), pts[-1][1] + float(L) * math.sin(a)))
    return pts


def occupancy_grid(link_lengths, obstacles, M):
    """:79-110 as a list of M lists of 0 / 1"""
    th = theta_list(M)
    grid = [[0] * M for _ in range(M)]
    for i in range(M):
        for j in range(M):
            pts = arm_points(link_lengths, th[i], th[j])
            hit = False
            for k in range(len(pts) - 1):
                for o in obstacles:
                    if detect_collision(pts[k][0], pts[k][1], pts[k + 1][0], pts[k + 1][1], float(o[0]), float(o[1]), float(o[2])):
                        hit = True
                        break
                if hit:
                    break
            grid[i][j] = int(hit)
    return grid


def heuristic_map(M, goal):
    """:221-233, the in-place loop as it is"""
    h = [[abs(j - goal[1]) + abs(i - goal[0]) for j in range(M)] for i in range(M)]
    for i in range(M):
        for j in range(M):
            h[i][j] = min(h[i][j], i + 1 + h[M - 1][j], M - i + h[0][j], j + 1 + h[i][M - 1], M - j + h[i][0])
    return h


def find_neighbors(i, j, M):
    """:187-209"""
    return [(i - 1 if i - 1 >= 0 else M - 1, j), (i + 1 if i + 1 < M else 0, j),
            (i, j - 1 if j - 1 >= 0 else M - 1), (i, j + 1 if j + 1 < M else 0)]


def search(grid, start, goal, h=None):
    """:113-184 on a copy of `grid` (a list of lists or an array of 0..6): (route as a list of (i, j), the marked grid as a list
    of lists, the number of cells closed).  h: heuristic_map(M, goal) when the caller has it already.
    Cells are numbered c = i * M + j.  explored_heuristic_map is a heap of h * M * M + c: a cell is opened at most once before
    it is popped (an opened cell's mark is 3, and only the goal goes back to 5 -- and the goal, the one cell with h = 0, is the
    next pop), so np.argmin's "smallest h, first in row-major order" is the heap's smallest entry."""
    M = len(grid)
    MM = M * M
    g = grid.reshape(-1).tolist() if hasattr(grid, "reshape") else [int(v) for row in grid for v in row]
    if h is None:
        h = heuristic_map(M, goal)
    hf = h.reshape(-1).tolist() if hasattr(h, "reshape") else [v for row in h for v in row]
    s, t = int(start[0]) * M + int(start[1]), int(goal[0]) * M + int(goal[1])
    heap = [hf[s] * MM + s]
    is_open = bytearray(MM)
    is_open[s] = 1
    parent = [-1] * MM
    pops = 0
    for _ in range(MM + 1):
        g[s] = 4
        g[t] = 5
        if not heap:
            break
        cur = heap[0] % MM
        if cur == t:
            break
        heapq.heappop(heap)
        pops += 1
        g[cur] = 2
        is_open[cur] = 0
        i, j = divmod(cur, M)
        for n in ((i - 1 if i else M - 1) * M + j, (i + 1 if i + 1 < M else 0) * M + j,
                  i * M + (j - 1 if j else M - 1), i * M + (j + 1 if j + 1 < M else 0)):   # find_neighbors' order
            if g[n] == 0 or g[n] == 5:
                assert not is_open[n]
                heapq.heappush(heap, hf[n] * MM + n)
                is_open[n] = 1
                parent[n] = cur
                g[n] = 3
    else:
        raise AssertionError("the loop made more than M * M + 1 trips")
    route = []
    if is_open[t]:
        c = t
        while c >= 0:
            route.insert(0, divmod(c, M))
            c = parent[c]
        for c in route[1:]:
            g[c[0] * M + c[1]] = 6
    return route, [g[i * M:(i + 1) * M] for i in range(M)], pops
