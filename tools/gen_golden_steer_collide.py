"""Golden generator of BatchSteer's obstacle check: runs the reference's stand-alone curve functions (plan_dubins_path,
reeds_shepp_path_planning) and the reference's own check_collision -- the copy in rrt_05 (:1625-1638) for Dubins rows, the
copy in rrt_06 (:1749-1762) for Reeds-Shepp rows, each cross-checked against the other -- all loaded through
oracle/ref_loader.py, and writes tests/golden/steer_collide_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_steer_collide.py

Arrays only.  Obstacle lists: ob (rows x, y, size of all lists, concatenated) and ob_off (list l is ob[ob_off[l]:ob_off[l + 1]]).
Dubins rows d_*: d_inp = (sx, sy, syaw, gx, gy, gyaw, curvature), d_sel / d_nsel as in steer_kat.npz, d_list the row's
obstacle list, d_rr its robot_radius, d_hit the expected value: -1 check_collision returns True, j >= 0 the shortest
prefix ob[:j + 1] of the list at which it returns False, -2 the reference has no curve; d_tag what the row is for.
Reeds-Shepp rows r_*: the same with r_inp = (..., curvature, step_size).  A grazing pair is two rows that differ in one
obstacle size by one ulp; the generator writes it only after the reference itself gave different answers for the two."""
import contextlib
import io
import math
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["dubins_path"] = "10_path_planning_00_dubins_path.py"
ref_loader.FILES["reeds_shepp_path"] = "10_path_planning_00_reeds_shepp_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")
WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")


def pose(rng):
    return rng.uniform(-2, 15), rng.uniform(-2, 15), rng.uniform(-math.pi, math.pi)


def checker(mod):
    """The reference's check_collision of a planner module (a staticmethod of its planner class)."""
    for v in vars(mod).values():
        if isinstance(v, type) and "check_collision" in vars(v):
            return v.check_collision
    raise RuntimeError("no check_collision in %s" % mod.__file__)


class Gen:
    def __init__(self):
        self.md = ref_loader.load("dubins_path")
        self.mr = ref_loader.load("reeds_shepp_path")
        self.chk = {"d": checker(ref_loader.load("rrt_05")), "r": checker(ref_loader.load("rrt_06"))}
        self.lists = []
        self.rows = {"d": [], "r": []}

    def curve(self, kind, inp, sel=None):
        """(path_x, path_y) as lists of the reference's own values, or None where it has no curve."""
        if kind == "d":
            try:
                px, py, _, _, _ = self.md.plan_dubins_path(*inp, selected_types=sel)
            except TypeError:
                return None
            return list(px), list(py)
        with contextlib.redirect_stdout(io.StringIO()):
            px, py, _, _, _ = self.mr.reeds_shepp_path_planning(*inp)
        return None if px is None else (list(px), list(py))

    def free(self, kind, xy, obs, rr):
        node = types.SimpleNamespace(path_x=xy[0], path_y=xy[1])
        a = self.chk[kind](node, obs, rr)
        b = self.chk["r" if kind == "d" else "d"](node, obs, rr)
        assert a is b or a == b, "the two copies of check_collision disagree"
        return bool(a)

    def hit(self, kind, xy, obs, rr):
        if xy is None:
            return -2
        if self.free(kind, xy, obs, rr):
            return -1
        for j in range(1, len(obs) + 1):   # growing prefixes: the first one the reference refuses
            if not self.chk[kind](types.SimpleNamespace(path_x=xy[0], path_y=xy[1]), obs[:j], rr):
                return j - 1
        raise AssertionError("unreachable")

    def add_list(self, obs):
        self.lists.append([tuple(float(v) for v in o) for o in obs])
        return len(self.lists) - 1

    def add(self, kind, inp, lst, rr, tag, sel=None, expect=None):
        h = self.hit(kind, self.curve(kind, inp, sel), self.lists[lst], rr)
        if expect is not None:
            assert expect(h), (tag, h)
        self.rows[kind].append(dict(inp=inp, lst=lst, rr=rr, hit=h, tag=tag, sel=sel))
        return h


def seeded_map(seed, m=30):
    rng = random.Random(seed)
    return [(rng.uniform(-2, 15), rng.uniform(-2, 15), rng.uniform(0.2, 0.9)) for _ in range(m)]


def dists(xy, ox, oy):
    """d_k as the reference forms it (:1631-1633), Python floats."""
    return [(ox - x) * (ox - x) + (oy - y) * (oy - y) for x, y in zip(xy[0], xy[1])]


def grazing_sizes(d):
    """(largest size with size ** 2 < d, smallest size with size ** 2 >= d), found with math.nextafter."""
    s = math.sqrt(d)
    while s ** 2 >= d:
        s = math.nextafter(s, 0.0)
    while math.nextafter(s, math.inf) ** 2 < d:
        s = math.nextafter(s, math.inf)
    return s, math.nextafter(s, math.inf)


def main():
    os.makedirs(GOLD, exist_ok=True)
    g = Gen()
    rng = random.Random(511)
    base = g.add_list(seeded_map(77))
    curv_of = {"d": (1.0, 0.5, 2.0), "r": (1.0, 0.5, 2.0)}
    step_of = (0.2, 0.05)

    def case(kind, k):
        inp = pose(rng) + pose(rng) + (curv_of[kind][k % 3],)
        return inp + (step_of[k % 2],) if kind == "r" else inp

    for kind in ("d", "r"):
        # the seeded map, robot_radius 0 and 0.35
        got = [g.add(kind, case(kind, k), base, 0.0, "map") for k in range(24)]
        assert sum(h == -1 for h in got) >= 4 and sum(h >= 0 for h in got) >= 4 and sum(h > 0 for h in got) >= 1, got
        for k in range(8):
            g.add(kind, case(kind, k), base, 0.35, "radius")
        # only the radius makes it a hit: a curve the map leaves free, and a radius just past its clearance
        done = 0
        while done < 2:
            inp = case(kind, done)
            xy = g.curve(kind, inp)
            if xy is None or not g.free(kind, xy, g.lists[base], 0.0):
                continue
            gap = min(math.sqrt(min(dists(xy, ox, oy))) - s for ox, oy, s in g.lists[base])
            g.add(kind, inp, base, 0.0, "radius_free", expect=lambda h: h == -1)
            g.add(kind, inp, base, gap + 0.01, "radius_only", expect=lambda h: h >= 0)
            done += 1
        # grazing pairs: one obstacle whose size is one ulp either side of the distance to the curve's nearest point
        done = 0
        while done < 4:
            inp = case(kind, done)
            xy = g.curve(kind, inp)
            if xy is None or len(xy[0]) < 3:
                continue
            k = rng.randrange(len(xy[0]))
            ox, oy = xy[0][k] + rng.uniform(-0.4, 0.4), xy[1][k] + rng.uniform(-0.4, 0.4)
            ds = sorted(dists(xy, ox, oy))
            if not (ds[0] > 0.0 and ds[1] > ds[0]):   # one nearest point, no other as near
                continue
            lo, hi = grazing_sizes(ds[0])
            far = (ox + 40.0, oy + 40.0, 0.5)       # an obstacle in front of it that is never touched: the answer is 1
            if g.free(kind, xy, [far, (ox, oy, lo)], 0.0) and not g.free(kind, xy, [far, (ox, oy, hi)], 0.0):
                g.add(kind, inp, g.add_list([far, (ox, oy, lo)]), 0.0, "graze_free", expect=lambda h: h == -1)
                g.add(kind, inp, g.add_list([far, (ox, oy, hi)]), 0.0, "graze_hit", expect=lambda h: h == 1)
                done += 1
        # 1 000 circles, only the last one touched -- and the same list without it
        while True:
            inp = case(kind, 0)
            xy = g.curve(kind, inp)
            if xy is not None and len(xy[0]) >= 20:
                break
        many = []
        while len(many) < 999:
            o = (rng.uniform(-4, 17), rng.uniform(-4, 17), rng.uniform(0.05, 0.3))
            if min(dists(xy, o[0], o[1])) > (o[2] + 0.05) ** 2:
                many.append(o)
        k = len(xy[0]) // 2
        last = (float(xy[0][k]) + 0.01, float(xy[1][k]) - 0.01, 0.1)
        g.add(kind, inp, g.add_list(many + [last]), 0.0, "many_last", expect=lambda h: h == 999)
        g.add(kind, inp, g.add_list(many), 0.0, "many_free", expect=lambda h: h == -1)

    # pairs without a curve
    g.add("d", (0.0, 0.0, 0.0, 12.0, 3.0, 1.0, 1.0), base, 0.0, "no_word", sel=["RLR", "LRL"], expect=lambda h: h == -2)
    rk = np.load(os.path.join(GOLD, "rs_kat.npz"))
    none_row = [float(v) for v in rk["inp"][int(np.nonzero(rk["n"] == 0)[0][0])]]
    g.add("r", tuple(none_row), base, 0.0, "no_path", expect=lambda h: h == -2)

    out = {"ob": np.array([o for lst in g.lists for o in lst], dtype=np.float64).reshape(-1, 3),
           "ob_off": np.cumsum([0] + [len(lst) for lst in g.lists]).astype(np.int64)}
    for kind in ("d", "r"):
        rows = g.rows[kind]
        out[kind + "_inp"] = np.array([r["inp"] for r in rows], dtype=np.float64)
        out[kind + "_list"] = np.array([r["lst"] for r in rows], dtype=np.int32)
        out[kind + "_rr"] = np.array([r["rr"] for r in rows], dtype=np.float64)
        out[kind + "_hit"] = np.array([r["hit"] for r in rows], dtype=np.int32)
        out[kind + "_tag"] = np.array([r["tag"] for r in rows])
    sel = [[] if r["sel"] is None else [WORDS.index(w) for w in r["sel"]] for r in g.rows["d"]]
    out["d_sel"] = np.array([s + [-1] * (6 - len(s)) for s in sel], dtype=np.int32)
    out["d_nsel"] = np.array([-1 if r["sel"] is None else len(r["sel"]) for r in g.rows["d"]], dtype=np.int32)
    dst = os.path.join(GOLD, "steer_collide_kat.npz")
    np.savez_compressed(dst, **out)
    for kind in ("d", "r"):
        h = out[kind + "_hit"]
        print("%s: %d rows, %d free, %d hit (%d at an index > 0), %d without a curve"
              % (kind, len(h), int(np.sum(h == -1)), int(np.sum(h >= 0)), int(np.sum(h > 0)), int(np.sum(h == -2))))
        print("   ", list(zip(out[kind + "_tag"].tolist(), h.tolist())))
    print("%d obstacle lists, %d rows in all, %d bytes" % (len(g.lists), len(out["ob"]), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
