"""Forged grazing circles for the tolerance-band verdicts of the rrt_04 and rrt_07 kernels.

The kernels decide a collision verdict from approximate points unless a circle's threshold lies within a tolerance band
of the closest distance**2; then the exact form decides.  On random maps that happens about once per 10^8 (edge, circle)
pairs, so this module BUILDS maps on which it happens all the time: circles tangent, to within a ladder of relative
offsets, to single points of edges the planner is going to test.  Pure Python plus the oracle; deterministic from
(planner, kw, seed, total).

forge() works in rounds.  A round runs the oracle on the map so far with its edge log on, picks a few edges the run
tested and found free -- later in the run than every earlier target, so that what was forged before stays as it is --
rebuilds the points of each edge as the oracle's steer does, picks one point and adds a circle of radius `size` whose
centre is (size + robot_radius) (1 + e) away from it, perpendicular to the edge: the picked point is then the closest.
A circle that would touch an edge the run found free EARLIER is shrunk to a tiny one (it would rewrite the history the
earlier circles were forged on).  The round is kept if the oracle, run again, counts no fewer grazing pairs than before
and the tree keeps at least 80 % of the nodes the unforged run built; otherwise it is tried once more with tiny circles
only, then dropped.  rrt_07: the same on the segments candidate -> new node its oracle logs.
"""
import ctypes as C
import functools
import math

import numpy as np

import oracle

# relative offsets of the centre distance from tangency: 0, the last bits, the band, and far outside it on both sides
LADDER = (0.0, 1e-16, -1e-16, 3e-16, -3e-16, 1e-15, -1e-15, 1e-13, -1e-13, 1e-11, -1e-11, 1e-9, -1e-9, 1e-7, -1e-7,
          1e-5, -1e-5, 1e-2, -1e-2)
# tiny circles leave the rest of the run almost untouched; map-like ones put the threshold where real maps have it
SIZES = (1e-3, 0.3, 1e-3, 1.0, 1e-3, 0.5, 2.0)
TINY = 1e-3
S_EXT_SHORT, S_EXT_LONG, S_CHOOSE, S_REWIRE, S_GOAL = range(5)
SITE_CYCLE = (S_CHOOSE, S_EXT_SHORT, S_REWIRE)
ONE_WAVE_TILE = 56      # circles the one-wave shape of the rrt_04 kernel takes
PER_ROUND = 4           # circles a round adds: free-side ones first, the last one may block its edge

GRAZE_KEYS = tuple(k for k, _ in oracle.Stats._fields_ if k.startswith("graze_"))


def run(planner, kw, seed, obstacles, graze=True, edge_log=False):
    """One oracle run of `planner` ("rrt_star" = rrt_04, "informed" = rrt_07) on kw with `obstacles`."""
    k = dict(kw, obstacles=obstacles)
    if planner == "informed":
        return oracle.plan_informed(seed=seed, graze=graze, edge_log=edge_log, **k)
    return oracle.plan(seed=seed, graze=graze, edge_log=edge_log, **k)


def graze_counts(stats):
    """The grazing-pair counters of one run (or the sum over runs) as a small dict."""
    out = {"in": 0, "out": 0, "exact": 0}
    for kind in ("in", "out", "exact"):
        for s in oracle.GRAZE_SITES:
            v = stats["graze_%s_%s" % (kind, s)]
            out[kind] += v
            if kind != "exact":
                out[s] = out.get(s, 0) + v
    return out


def add_stats(total, stats):
    for k in GRAZE_KEYS:
        total[k] = total.get(k, 0) + stats[k]
    return total


def _polyline(row, res):
    """The points the oracle tested for one edge-log row: rrt_04's steer polyline."""
    L = oracle.lib()
    L.orc_steer_polyline.restype = C.c_int
    L.orc_steer_polyline.argtypes = [C.c_double] * 6 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cap = int(row[7]) + 4
    px = np.zeros(cap)
    py = np.zeros(cap)
    end = np.zeros(2)
    sn = C.c_int(0)
    n = L.orc_steer_polyline(row[2], row[3], row[4], row[5], row[6], res, px.ctypes.data, py.ctypes.data, cap,
                             end.ctypes.data, C.byref(sn))
    assert n == int(row[7]), (n, row)
    return px[:n], py[:n]


def _reach_of_free_edges(edges, before_it, cx, cy):
    """Smallest distance from (cx, cy) to the segments of the edges found free before iteration `before_it`."""
    e = edges[(edges[:, 1] < before_it) & (edges[:, 8] == 1)]
    if not len(e):
        return math.inf
    fx, fy = e[:, 2], e[:, 3]
    dx, dy = e[:, 4] - fx, e[:, 5] - fy
    d = np.hypot(dx, dy)
    cut = np.where(d > 0, np.minimum(1.0, e[:, 6] / np.where(d > 0, d, 1.0)), 0.0)   # steer stops at `extend`
    dx, dy = dx * cut, dy * cut
    l2 = dx * dx + dy * dy
    t = np.clip(((cx - fx) * dx + (cy - fy) * dy) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
    return float(np.hypot(cx - (fx + t * dx), cy - (fy + t * dy)).min())


def _circle(planner, row, res, radius_add, size, e, pick, side):
    """The circle of radius `size` tangent (to within e) to point number `pick` of the edge of `row`."""
    fx, fy, tx, ty = row[2], row[3], row[4], row[5]
    d = math.hypot(tx - fx, ty - fy)
    if d == 0.0:
        return None
    if planner == "informed":
        t = (0.5, 0.25, 0.75, 0.0, 1.0)[pick % 5]          # a point of the segment, the ends included
        qx, qy = fx + t * (tx - fx), fy + t * (ty - fy)
    else:
        px, py = _polyline(row, res)
        n = len(px)
        if pick % 5 == 3:
            i = 0                                          # the edge's first point: a node of the tree
        elif pick % 5 == 4 or n < 3:
            i = n - 1                                      # its last point
        else:
            i = 1 + (pick // 5) % (n - 2)                  # a point of the walk
        qx, qy = float(px[i]), float(py[i])
    ux, uy = -(ty - fy) / d * side, (tx - fx) / d * side
    r = (size + radius_add) * (1.0 + e)
    return (qx + ux * r, qy + uy * r, size)


def _pick_rows(edges, site, after_it, want_points):
    """Rows of the log a circle may be forged on: found free, no grazing circle yet, later than `after_it`."""
    ok = (edges[:, 8] == 1) & (edges[:, 9] == 0) & (edges[:, 1] > after_it)
    rows = edges[ok & (edges[:, 0] == site) & (edges[:, 7] >= want_points)]
    if not len(rows):
        rows = edges[ok & (edges[:, 0] == site)]
    if not len(rows):
        rows = edges[ok & (edges[:, 0] != S_GOAL)]
    return rows


def forge(planner, kw, seed, total=ONE_WAVE_TILE):
    """kw["obstacles"] plus forged circles, `total` circles in all (fewer only if the run offers no more edges)."""
    return list(_forge(planner, _freeze(kw), int(seed), int(total)))


def _freeze(kw):
    return tuple(sorted((k, tuple(tuple(o) for o in v) if k == "obstacles" else (tuple(v) if isinstance(v, list) else v))
                        for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _forge(planner, frozen, seed, total):
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in frozen}
    obstacles = [tuple(float(v) for v in o) for o in kw.pop("obstacles")]
    res = kw.get("path_resolution", 1.0)
    radius_add = kw.get("robot_radius", 0.0) if planner != "informed" else 0.0
    max_iter = kw["max_iter"]
    n_new = total - len(obstacles)
    first_it = max_iter // 12
    r = run(planner, kw, seed, obstacles, edge_log=True)
    have = sum(r["stats"][k] for k in GRAZE_KEYS if "exact" not in k)
    n_nodes = len(r["x"])
    c = seed * 5                         # where this instance starts on the ladder / size / site cycles
    made = 0
    last_it = first_it
    rounds_left = 4 * (n_new // PER_ROUND + 8)
    while made < n_new and rounds_left > 0:
        rounds_left -= 1
        k_round = min(PER_ROUND, n_new - made)
        kept = False
        for tiny_only in (False, True):
            cand, it_cur = [], last_it
            for j in range(k_round):
                cc = c + j
                e = LADDER[cc % len(LADDER)]
                if j < k_round - 1:
                    e = abs(e) if e != 0.0 else 1e-12   # free side: the edge stays, and so does what follows it
                size = TINY if tiny_only else SIZES[cc % len(SIZES)]
                # spread the targets over what is left of the run
                gap = (max_iter - it_cur) // (2 * max(1, (n_new - made - j)))
                rows = _pick_rows(r["edges"], SITE_CYCLE[cc % len(SITE_CYCLE)], it_cur + gap, 3)
                if not len(rows):
                    break
                row = rows[(cc * 7) % min(len(rows), 5)]
                circ = _circle(planner, row, res, radius_add, size, e, cc // len(SITE_CYCLE), 1 if (cc // 2) % 2 else -1)
                if circ is None:
                    continue
                if size != TINY and _reach_of_free_edges(r["edges"], row[1], circ[0], circ[1]) <= (size + radius_add) * 1.01:
                    circ = _circle(planner, row, res, radius_add, TINY, e, cc // len(SITE_CYCLE), 1 if (cc // 2) % 2 else -1)
                cand.append(circ)
                it_cur = int(row[1])
            if not cand:
                break
            r2 = run(planner, kw, seed, obstacles + cand, edge_log=True)
            have2 = sum(r2["stats"][k] for k in GRAZE_KEYS if "exact" not in k)
            # kept: no grazing pair lost, and the tree still grows (a circle that walls the start in grazes every
            # extension edge of the run and tests nothing else)
            if have2 >= have and len(r2["x"]) >= 0.8 * n_nodes:
                obstacles, r, have, kept = obstacles + cand, r2, have2, True
                made += len(cand)
                last_it = it_cur
                break
        c += k_round
        if not kept:
            if not len(_pick_rows(r["edges"], S_CHOOSE, last_it, 0)):
                last_it = first_it   # the run's end is reached: go round again (rows with a grazing circle are skipped)
                if not len(_pick_rows(r["edges"], S_CHOOSE, last_it, 0)):
                    break
            else:
                last_it += max(1, (max_iter - last_it) // 8)
    return tuple(obstacles)


# ---- the scenes tests/test_graze_host.py measures and tests/test_gpu_graze.py plans (same maps, same seeds)
def _arena():
    import util
    kw = dict(util.C2)
    kw.update(goal=[18, 18], rand_area=[0, 20], obstacles=[], max_iter=600)
    return kw


def rrt04_scenes():
    """name -> (kw, seeds, circles per map).  Every map fits the one-wave tile but "arena200"."""
    import util
    arena = _arena()
    drv = dict(util.C2)
    drv.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.1, goal_sample_rate=20,
               max_iter=600, obstacles=[(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)])
    c2 = util.c2_kwargs(1500)
    c2["obstacles"] = c2["obstacles"][:16]
    return {
        # 20 x 20 arena, C2 parameters: dense within ~100 nodes, the libm-free extension edge is the usual one
        "arena": (arena, (1, 2, 3, 4), ONE_WAVE_TILE),
        # thresholds (size + robot_radius) ** 2, steps that do not divide expand_dis
        "arena_res03_rr02": (dict(arena, path_resolution=0.3, robot_radius=0.2), (1, 2, 3, 4), ONE_WAVE_TILE),
        # rewire moves nodes: the backward edges are evaluated again from the winner's end point (eval_edges_back2)
        "moved_nodes": (drv, (1, 2, 3, 4), ONE_WAVE_TILE),
        # 16 circles of the C2 map + 40 forged ones, the benchmark's arena
        "c2_prefix": (c2, (1, 2, 3, 4), ONE_WAVE_TILE),
        # more circles than the one- and two-wave shapes take
        "arena200": (arena, (7,), 200),
    }


def rrt07_scene():
    """(kw, seeds, circles per map): the driver scene of the rrt_07 goldens, 600 iterations."""
    import util
    kw = util.informed_kwargs_from_golden(util.load_golden(util.GOLDEN + "/rrt07_drv_mt_s5_it600.npz"))
    return kw, (1, 2, 3, 4), ONE_WAVE_TILE
