"""Golden generator of BatchArmNav: runs the reference's own get_occupancy_grid, astar_torus and calc_heuristic_map of
02_arm_obstacle_navigation.py, loaded through oracle/ref_loader.py (the file name is added to ref_loader.FILES at run time, the
module global M is set per call, plt and from_levels_and_colors are replaced by do-nothing stubs), and writes
tests/golden/armnav_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_armnav.py

Arrays only.
Scenes (n_s): scene_M, scene_kind (0 an arm among circles: its grid is get_occupancy_grid's; 1 a grid made here as data: walls
that force a route round the torus), link_off / link_len and obs_off / obs_xyr (CSR per scene, empty for kind 1), grid_off
(n_s + 1,) into grids (uint8, row-major cells of every scene).
Queries (n_q): q_scene, q_start (n_q, 2), q_goal (n_q, 2), q_tag (TAGS below), q_pops (calls of find_neighbors: the cells the
search closed), route_off (n_q + 1,) into route_ij (rows i, j), q_marks_off (n_q,) into marks (uint8: the grid astar_torus left
behind, M * M cells), -1 where it is not stored.
Heuristic maps (n_h): h_M, h_goal (n_h, 2), h_off (n_h + 1,) into h_flat (int16).
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["arm_obstacle_navigation"] = "02_arm_obstacle_navigation.py"
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("driver", "same", "goal_on_obstacle", "start_on_obstacle", "walled", "wrap_i", "wrap_j", "wrap_both", "random")
DRIVER_LINKS = [0.5, 0.5, 0.3, 0.5, 0.1]
DRIVER_OBSTACLES = [[1.75, 0.75, 0.6], [0.55, 1.5, 0.5], [0, -1, 0.7], [0, -0.6, 0.4], [-1, 1., 0.3]]
DRIVER_QUERY = ((10, 50), (58, 56))
DATA_M = (3, 5, 8, 16, 17, 33, 64, 65, 128)
MARKS_ALWAYS_UP_TO = 33


class Nothing:
    """plt: every attribute and every call gives it back"""
    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def main():
    os.makedirs(GOLD, exist_ok=True)
    ref = ref_loader.load("arm_obstacle_navigation")
    ref.plt = Nothing()
    ref.from_levels_and_colors = lambda levels, colors: (None, None)
    rs = np.random.RandomState(2002)
    n_closed = [0]
    ref_neighbors = ref.find_neighbors

    def counting_neighbors(i, j):
        n_closed[0] += 1
        return ref_neighbors(i, j)
    ref.find_neighbors = counting_neighbors

    def rand_arm(n, negative=False):
        L = rs.uniform(0.15, 2.2 / n + 0.1, n)
        if negative:
            L[rs.randint(n)] *= -1.0
        return [float(v) for v in L]

    def rand_circles(n, rmin=0.1, rmax=0.5):
        return [[float(rs.uniform(-2.0, 2.0)), float(rs.uniform(-2.0, 2.0)), float(rs.uniform(rmin, rmax))] for _ in range(n)]

    # (M, links, circles)
    arms = [(100, DRIVER_LINKS, DRIVER_OBSTACLES),
            (2, rand_arm(1), rand_circles(1)), (2, rand_arm(2), []),
            (3, rand_arm(2, negative=True), rand_circles(2, 0.4, 0.9)),
            (5, rand_arm(5), rand_circles(1, 0.5, 1.0)), (5, rand_arm(1), rand_circles(3)),
            (8, rand_arm(16), rand_circles(4)),
            (16, rand_arm(5), rand_circles(70, 0.02, 0.12)), (16, rand_arm(2), []),
            (17, rand_arm(2), rand_circles(3)), (17, rand_arm(16, negative=True), rand_circles(2)),
            (33, DRIVER_LINKS, DRIVER_OBSTACLES), (33, rand_arm(1), rand_circles(1, 0.3, 0.5)),
            (64, DRIVER_LINKS, DRIVER_OBSTACLES), (64, rand_arm(2), rand_circles(4)),
            (65, DRIVER_LINKS, DRIVER_OBSTACLES),
            (128, rand_arm(2), rand_circles(3))]
    scenes = []   # dict(M, kind, links, circles, grid)
    for M, links, circles in arms:
        ref.M = M
        arm = ref.NLinkArm(links, [0.0] * len(links))
        grid = ref.get_occupancy_grid(arm, circles, M)
        assert grid.shape == (M, M) and set(np.unique(grid).tolist()) <= {0, 1}
        scenes.append(dict(M=M, kind=0, links=links, circles=circles, grid=grid.astype(np.uint8)))
        print("scene %d: M %d, %d links, %d circles, %d of %d cells occupied" % (len(scenes) - 1, M, len(links), len(circles),
                                                                                 int(grid.sum()), M * M))

    def walls(M, rows, cols):
        """Full walls on the given rows and columns, and a sprinkle of single cells that touches no cell next to a wall"""
        g = np.zeros((M, M), dtype=np.uint8)
        for _ in range(M * M // 12):
            g[rs.randint(M), rs.randint(M)] = 1
        for r in rows:
            g[(r - 1) % M], g[(r + 1) % M] = 0, 0
        for c in cols:
            g[:, (c - 1) % M], g[:, (c + 1) % M] = 0, 0
        for r in rows:
            g[r] = 1
        for c in cols:
            g[:, c] = 1
        return g
    data = {}   # M -> {name: scene index}
    for M in DATA_M:
        mid = M // 2
        data[M] = {}
        for name, rows, cols in (("wrap_i", [mid], []), ("wrap_j", [], [mid]), ("wrap_both", [mid], [mid])):
            data[M][name] = len(scenes)
            scenes.append(dict(M=M, kind=1, links=[], circles=[], grid=walls(M, rows, cols)))

    queries = []   # dict(scene, start, goal, tag, route, pops, marks)

    def run(si, start, goal, tag, keep_marks=False):
        sc = scenes[si]
        M = sc["M"]
        ref.M = M
        g = sc["grid"].astype(np.int64)
        n_closed[0] = 0
        with contextlib.redirect_stdout(io.StringIO()):
            route = ref.astar_torus(g, (int(start[0]), int(start[1])), (int(goal[0]), int(goal[1])))
        route = [(int(c[0]), int(c[1])) for c in route]
        assert int(g.min()) >= 0 and int(g.max()) <= 6
        queries.append(dict(scene=si, start=start, goal=goal, tag=tag, route=route, pops=n_closed[0],
                            marks=g.astype(np.uint8) if (keep_marks or M <= MARKS_ALWAYS_UP_TO) else None))
        return route

    def pick(cells):
        return tuple(int(v) for v in cells[rs.randint(len(cells))])

    for si, sc in enumerate(scenes):
        if sc["kind"] != 0:
            continue
        M, grid = sc["M"], sc["grid"]
        free, occ = np.argwhere(grid == 0), np.argwhere(grid == 1)
        # an obstacle cell whose four neighbours are obstacle cells too: nothing ever opens it
        inner = np.argwhere((grid == 1) & (np.roll(grid, 1, 0) == 1) & (np.roll(grid, -1, 0) == 1) & (np.roll(grid, 1, 1) == 1) &
                            (np.roll(grid, -1, 1) == 1))
        if M >= 64:
            r = run(si, *DRIVER_QUERY, "driver", keep_marks=True)
            if si == 0:
                assert len(r) == 347, len(r)   # "The route found covers 347 grid cells."
        if len(free):
            c = pick(free)
            assert run(si, c, c, "same") == [c]
        if len(occ):
            c = pick(occ)
            assert run(si, c, c, "same") == [c]
        if len(occ) and len(free):
            run(si, pick(free), pick(occ), "goal_on_obstacle", keep_marks=M == 64)
            run(si, pick(occ), pick(free), "start_on_obstacle", keep_marks=M == 65)
        if len(inner) and len(free):
            assert run(si, pick(free), pick(inner), "walled", keep_marks=M == 128) == []
        for k in range(8 if M <= 33 else 6):
            run(si, (rs.randint(M), rs.randint(M)), (rs.randint(M), rs.randint(M)), "random", keep_marks=(M >= 64 and k == 0))

    def jumps(route, axis, M):
        return sum(1 for a, b in zip(route, route[1:]) if abs(a[axis] - b[axis]) == M - 1)
    for M in DATA_M:
        mid = M // 2
        lo, hi = rs.randint(0, mid), rs.randint(mid + 1, M)
        other = lambda: int(rs.randint(M))   # noqa: E731
        for name, start, goal in (("wrap_i", (lo, other()), (hi, other())), ("wrap_j", (other(), lo), (other(), hi)),
                                  ("wrap_both", (lo, lo), (hi, hi))):
            si = data[M][name]
            g = scenes[si]["grid"]
            if name == "wrap_both":   # keep the two corners off the sprinkle
                g[start], g[goal] = 0, 0
            r = run(si, start, goal, name, keep_marks=M in (64, 128) and name == "wrap_both")
            assert r and r[0] == start and r[-1] == goal, (M, name)
            if M > 3:   # (at M = 3 a step of 2 cells is a wrap and a step back at once)
                assert name == "wrap_j" or jumps(r, 0, M) % 2 == 1, (M, name)
                assert name == "wrap_i" or jumps(r, 1, M) % 2 == 1, (M, name)
            if name == "wrap_both":   # wall cells: one next to free cells, and the centre of the cross, walled in
                assert run(si, start, (mid, lo), "goal_on_obstacle") != []
                run(si, (mid, lo), goal, "start_on_obstacle")
                assert run(si, start, (mid, mid), "walled") == []
            for _ in range(2):
                run(si, (rs.randint(M), rs.randint(M)), (rs.randint(M), rs.randint(M)), "random")
    # M = 2: every cell's up and down (left and right) neighbour is the same cell
    for si, sc in enumerate(scenes):
        if sc["M"] == 2:
            for s in range(4):
                for t in range(4):
                    run(si, (s // 2, s % 2), (t // 2, t % 2), "random" if s != t else "same")

    hmaps = []
    for M in (2, 3, 5, 8, 17, 64, 128):
        x = M // 3
        for goal in ((0, x), (M - 1, x), (x, 0), (x, M - 1), (0, 0), (M - 1, M - 1), (0, M - 1), (M - 1, 0), (x, M // 2)):
            hmaps.append((M, goal))
    hmaps.append((100, DRIVER_QUERY[1]))
    hflat = []
    for M, goal in hmaps:
        h = ref.calc_heuristic_map(M, goal)
        assert h.shape == (M, M) and h.min() >= 0 and h.max() <= 2 * M - 2
        hflat.append(h.astype(np.int16).reshape(-1))
    X, Y = np.meshgrid(np.arange(100), np.arange(100))
    closed = np.minimum(np.abs(X - 56), 100 - np.abs(X - 56)) + np.minimum(np.abs(Y - 58), 100 - np.abs(Y - 58))
    print("heuristic M = 100, goal (58, 56): %d cells differ from the torus Manhattan distance"
          % int(np.sum(closed.reshape(-1) != hflat[-1])))

    def csr(lists, width, dtype):
        off = np.zeros(len(lists) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(v) for v in lists])
        flat = np.array([r for v in lists for r in v], dtype=dtype).reshape((-1, width) if width > 1 else (-1,))
        return off, flat
    link_off, link_len = csr([s["links"] for s in scenes], 1, np.float64)
    obs_off, obs_xyr = csr([s["circles"] for s in scenes], 3, np.float64)
    grid_off = np.zeros(len(scenes) + 1, dtype=np.int64)
    grid_off[1:] = np.cumsum([s["M"] ** 2 for s in scenes])
    route_off, route_ij = csr([q["route"] for q in queries], 2, np.int32)
    marks, marks_off, pos = [], [], 0
    for q in queries:
        if q["marks"] is None:
            marks_off.append(-1)
        else:
            marks_off.append(pos)
            marks.append(q["marks"].reshape(-1))
            pos += q["marks"].size
    h_off = np.zeros(len(hmaps) + 1, dtype=np.int64)
    h_off[1:] = np.cumsum([len(h) for h in hflat])
    dst = os.path.join(GOLD, "armnav_kat.npz")
    np.savez_compressed(
        dst, scene_M=np.array([s["M"] for s in scenes], dtype=np.int32), scene_kind=np.array([s["kind"] for s in scenes], dtype=np.int32),
        link_off=link_off, link_len=link_len, obs_off=obs_off, obs_xyr=obs_xyr, grid_off=grid_off,
        grids=np.concatenate([s["grid"].reshape(-1) for s in scenes]).astype(np.uint8),
        q_scene=np.array([q["scene"] for q in queries], dtype=np.int32), q_start=np.array([q["start"] for q in queries], dtype=np.int32),
        q_goal=np.array([q["goal"] for q in queries], dtype=np.int32), q_tag=np.array([TAGS.index(q["tag"]) for q in queries], dtype=np.int32),
        q_pops=np.array([q["pops"] for q in queries], dtype=np.int32), route_off=route_off, route_ij=route_ij,
        q_marks_off=np.array(marks_off, dtype=np.int64), marks=np.concatenate(marks).astype(np.uint8),
        h_M=np.array([m for m, _ in hmaps], dtype=np.int32), h_goal=np.array([g for _, g in hmaps], dtype=np.int32), h_off=h_off,
        h_flat=np.concatenate(hflat).astype(np.int16))
    n_route = np.diff(route_off)
    print("%d scenes, %d queries (%d with a route, longest %d cells, most cells closed %d), %d marked grids, %d heuristic maps; "
          "%d bytes" % (len(scenes), len(queries), int(np.sum(n_route > 0)), int(n_route.max()), max(q["pops"] for q in queries),
                        len(marks), len(hmaps), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
