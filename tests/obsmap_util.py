"""The obstacle map of rrtx_set_obstacle_map restated in Python (the rules of csrc/rpp_obsgrid.h), for the host and the GPU
tests: geometry, cell ranges, the wide rule and the whole CSR.  Every operation is one IEEE double operation, as in the
header, so the results are compared exactly."""
import math

import numpy as np

AXIS_MIN, AXIS_MAX, WIDE_CELLS = 8, 1024, 32
DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations")


def axis_cells(m, forced=0):
    if forced > 0:
        return min(forced, AXIS_MAX)
    k = AXIS_MIN
    while k < AXIS_MAX and k * k < m:
        k += 1
    return k


def geometry(rand_area, m, forced=0):
    """(x0, y0, cell, nx, ny)"""
    lo, hi = min(rand_area[0], rand_area[1]), max(rand_area[0], rand_area[1])
    n = axis_cells(m, forced)
    cell = (hi - lo) / float(n)
    if not (cell > 0.0) or not (cell < math.inf):
        cell = 1.0
    return float(lo), float(lo), cell, n, n


def cell_of(v, origin, cell, n):
    """Vectorised: floor((v - origin) / cell) clamped to [0, n - 1]."""
    q = np.floor((np.asarray(v, dtype=np.float64) - origin) / cell)
    return np.where(q > 0.0, np.minimum(q, float(n - 1)), 0.0).astype(np.int64)


def reach(size, robot_radius):
    a = np.abs(np.asarray(size, dtype=np.float64) + robot_radius)
    return a + a * 2.0 ** -40 + 2.0 ** -500


def range_of(g, xlo, xhi, ylo, yhi):
    x0, y0, cell, nx, ny = g
    return cell_of(xlo, x0, cell, nx), cell_of(xhi, x0, cell, nx), cell_of(ylo, y0, cell, ny), cell_of(yhi, y0, cell, ny)


def circle_ranges(g, circles, robot_radius):
    """(rho, cx0, cx1, cy0, cy1, wide) per circle."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    rho = reach(c[:, 2], robot_radius)
    cx0, cx1, cy0, cy1 = range_of(g, c[:, 0] - rho, c[:, 0] + rho, c[:, 1] - rho, c[:, 1] + rho)
    wide = (cx1 - cx0 + 1) * (cy1 - cy0 + 1) > WIDE_CELLS
    return rho, cx0, cx1, cy0, cy1, wide


def build(rand_area, circles, robot_radius=0.0, forced=0):
    """The map as rrtx_get_obstacle_map returns it: (geometry, cell_start[cells + 1], item rows, wide rows); `rows` are
    circle indices, a cell's in ascending order."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    g = geometry(rand_area, len(c), forced)
    nx, ny = g[3], g[4]
    _, cx0, cx1, cy0, cy1, wide = circle_ranges(g, c, robot_radius)
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


def thresholds(circles, robot_radius):
    """(size + robot_radius) ** 2 as the reference evaluates it (rrt_04:1227): CPython's float ** 2"""
    return np.array([(float(s) + robot_radius) ** 2 for s in np.asarray(circles, dtype=np.float64).reshape(-1, 3)[:, 2]])


def assert_map_equals(handle, rand_area, circles, robot_radius=0.0, forced=0):
    """The handle's map equals the restatement exactly, and its info agrees with it."""
    c = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    g, cell_start, rows, wide_rows = build(rand_area, c, robot_radius, forced)
    info = handle.obstacle_map_info()
    assert (info["x0"], info["y0"], info["cell"], info["nx"], info["ny"]) == g
    assert (info["n_circles"], info["n_items"], info["n_wide"]) == (len(c), len(rows), len(wide_rows))
    assert info["build_ms"] >= 0.0
    got_start, items, wide = handle.obstacle_map()
    assert np.array_equal(got_start, cell_start)
    thr = thresholds(c, robot_radius)
    for got, want in ((items, rows), (wide, wide_rows)):
        assert np.array_equal(got["index"], want)
        assert np.array_equal(got["ox"], c[want, 0]) and np.array_equal(got["oy"], c[want, 1])
        assert np.array_equal(got["thr"], thr[want])
    return info
