"""The obstacle index of BatchSteer / BatchSpline / BatchBSpline restated in Python (the rules added to csrc/rpp_obsgrid.h:
geometry_box, the build over it, point_first_hit and index_reason), for the host and the GPU tests.  Every operation is one
IEEE double operation, as in the header, so the results are compared exactly."""
import math

import numpy as np

import obsmap_util as OM

RUN_MAX, MIN = 4096, 256
AUTO, ON, OFF = 0, 1, 2
REASONS = ("used", "off", "below the threshold", "run too long", "non-finite reach", "empty")


def geometry_box(circles, forced=0):
    """(x0, y0, cell, nx, ny) over the box of the circle centres."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    n = OM.axis_cells(len(c), forced)
    if len(c) == 0:
        return 0.0, 0.0, 1.0, n, n
    xmin, xmax, ymin, ymax = float(c[:, 0].min()), float(c[:, 0].max()), float(c[:, 1].min()), float(c[:, 1].max())
    with np.errstate(over="ignore"):
        cell = float(np.float64(max(np.float64(xmax) - xmin, np.float64(ymax) - ymin)) / float(n))
    if not (cell > 0.0) or not (cell < math.inf):
        cell = 1.0
    return xmin, ymin, cell, n, n


def build(circles, robot_radius=0.0, forced=0):
    """The index as rrtx_steer_get_obstacle_index returns it: (geometry, cell_start[cells + 1], item rows, wide rows)."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    g = geometry_box(c, forced)
    nx, ny = g[3], g[4]
    _, cx0, cx1, cy0, cy1, wide = OM.circle_ranges(g, c, robot_radius)
    per_cell = [[] for _ in range(nx * ny)]
    wide_rows = []
    for i in range(len(c)):
        if wide[i]:
            wide_rows.append(i)
            continue
        for cy in range(cy0[i], cy1[i] + 1):
            for cx in range(cx0[i], cx1[i] + 1):
                per_cell[cy * nx + cx].append(i)
    cell_start = np.zeros(nx * ny + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum([len(p) for p in per_cell])
    rows = np.array([i for p in per_cell for i in p], dtype=np.int64)
    return g, cell_start, rows, np.array(wide_rows, dtype=np.int64)


def reason(circles, robot_radius=0.0, mode=AUTO, forced=0):
    """index_reason of the header for this list, as a word of REASONS."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    if len(c) == 0:
        return "empty"
    if mode == OFF:
        return "off"
    if mode == AUTO and len(c) <= MIN:
        return "below the threshold"
    with np.errstate(over="ignore"):
        thr = np.array([_sq(float(s) + robot_radius) for s in c[:, 2]])
        rho = OM.reach(c[:, 2], robot_radius)
    if not (np.isfinite(thr).all() and np.isfinite(rho).all()):
        return "non-finite reach"
    _, cell_start, _, wide = build(c, robot_radius, forced)
    if max(int(np.diff(cell_start).max()), len(wide)) > RUN_MAX:
        return "run too long"
    return "used"


def _sq(v):
    try:
        return v ** 2
    except OverflowError:          # CPython raises where the C library's pow returns inf
        return math.inf


def first_hit_linear(circles, robot_radius, x, y):
    """rpp::first_hit for arrays of points: the lowest row whose circle holds the point, or -1."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    thr = OM.thresholds(c, robot_radius)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.full(len(x), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(len(c) - 1, -1, -1):
            dx, dy = c[j, 0] - x, c[j, 1] - y
            out[dx * dx + dy * dy <= thr[j]] = j
    return out


def point_first_hit(index, circles, robot_radius, x, y):
    """rppo::point_first_hit for one point on build()'s answer: (the index, records read)."""
    g, cell_start, rows, wide = index
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    thr = OM.thresholds(c, robot_radius)
    cx = int(OM.cell_of(x, g[0], g[2], g[3]))
    cy = int(OM.cell_of(y, g[1], g[2], g[4]))
    k = cy * g[3] + cx
    best, read = -1, 0

    def hits(j):
        dx, dy = c[j, 0] - x, c[j, 1] - y
        return dx * dx + dy * dy <= thr[j]
    for j in rows[cell_start[k]:cell_start[k + 1]]:
        read += 1
        if hits(j):
            best = int(j)
            break
    for j in wide:
        if best >= 0 and j > best:
            break
        read += 1
        if hits(j):
            best = int(j)
            break
    return best, read


def assert_index_equals(steer, circles, robot_radius=0.0, forced=0):
    """The index read back from an _abi.Steer equals the restatement exactly, and its info agrees with it."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    g, cell_start, rows, wide_rows = build(c, robot_radius, forced)
    info, got_start, items, wide = steer.obstacle_index()
    assert info["used"] and info["reason"] == "used"
    assert (info["x0"], info["y0"], info["cell"], info["nx"], info["ny"]) == g
    assert (info["n_circles"], info["n_items"], info["n_wide"]) == (len(c), len(rows), len(wide_rows))
    assert info["build_ms"] >= 0.0
    assert np.array_equal(got_start, cell_start)
    thr = OM.thresholds(c, robot_radius)
    for got, want in ((items, rows), (wide, wide_rows)):
        assert np.array_equal(got["index"], want)
        assert np.array_equal(got["ox"], c[want, 0]) and np.array_equal(got["oy"], c[want, 1])
        assert np.array_equal(got["thr"], thr[want])
    return info
