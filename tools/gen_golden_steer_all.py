"""Golden generator of the candidate lists: runs the reference's calc_paths (10_path_planning_00_reeds_shepp_path.py :483)
itself (loaded through oracle/ref_loader.py, as tools/gen_golden_steer.py does) and writes tests/golden/steer_all_kat.npz.
Build host only (needs the reference checkout).

    python tools/gen_golden_steer_all.py [seed]

Arrays only.  Per pair: inp = (sx, sy, syaw, gx, gy, gyaw, maxc, step_size); n_cand = len(paths), -1 where calc_paths raises
(err then holds the exception's name); cand_off (n + 1,).  Per candidate, in list order: c_mode (Path.ctypes joined), c_nlen,
c_lengths (m, 5) = Path.lengths zero padded, c_L = Path.L, c_off (m + 1,) into the concatenated x, y, yaw (float64) and
directions (int8).  Path.ctypes and Path.lengths are read after calc_paths returns: the divided ones.

The set: raising rows of both exception kinds -- the ZeroDivisionError rows of rs_kat.npz (start = goal) and ValueError
rows drawn here (the goal within 1e-9 .. 1e-4 of the start at the same yaw: math.asin of a quotient that rounding pushes
past 1 in left_right_x_left) --, a pair where generate_path stops at "Step size too large", and a seeded random draw in
the [-2, 15] area over the curvatures 0.1, 0.5, 1, 2, mostly at step 0.5 and 0.2 so that the point arrays stay small.  The conditions asserted below (and again by tests/test_steer_all_host.py) decide the seed."""
import contextlib
import io
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["reeds_shepp_path"] = "10_path_planning_00_reeds_shepp_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 3
N_RANDOM = 66
DRIVER = (-1.0, -4.0, float(np.deg2rad(-20.0)), 5.0, 5.0, float(np.deg2rad(25.0)), 0.1, 0.05)   # the script's driver poses


def pose(rng):
    return rng.uniform(-2, 15), rng.uniform(-2, 15), rng.uniform(-math.pi, math.pi)


def call(mr, inp):
    """(paths or None, exception name, what calc_paths printed)"""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            return mr.calc_paths(*inp), "", out.getvalue()
        except (ZeroDivisionError, ValueError) as e:
            return None, type(e).__name__, out.getvalue()


def conditions(n_cand, err, printed, cand_off, c_L, curv):
    """What the set must hold; shared wording with the CPU test."""
    ties = 0
    for i in range(len(n_cand)):
        L = sorted(c_L[cand_off[i]:cand_off[i + 1]].tolist())
        ties += any(a == b for a, b in zip(L, L[1:]))
    assert sum(1 for v in n_cand if v == 0) >= 3, "pairs with []"
    assert {"ZeroDivisionError", "ValueError"} <= set(err), "both exception kinds"
    assert any("Step size too large" in p for p in printed), "a 'step size too large' pair"
    assert sum(1 for v in n_cand if v >= 10) >= 5, "pairs with >= 10 candidates"
    assert ties >= 10, "pairs holding two candidates of exactly equal L: %d" % ties
    assert set(curv) >= {0.1, 0.5, 1.0, 2.0}, "every curvature"


def main(seed):
    mr = ref_loader.load("reeds_shepp_path")
    kat = np.load(os.path.join(GOLD, "rs_kat.npz"))
    raising = [i for i in range(len(kat["n"])) if int(kat["n"][i]) == -1]
    kinds = {}
    for i in raising:   # two rows of each exception kind
        kinds.setdefault(str(kat["mode"][i]), []).append(i)
    cases = [DRIVER] + [tuple(float(v) for v in kat["inp"][i]) for rows in kinds.values() for i in rows[:2]]
    rng = random.Random(seed)
    n_value = 0
    while n_value < 2:
        s = pose(rng)
        r, a = 10 ** rng.uniform(-9, -4), rng.uniform(-math.pi, math.pi)
        inp = s + (s[0] + r * math.cos(a), s[1] + r * math.sin(a), s[2], 1.0, 0.5)
        if call(mr, inp)[1] == "ValueError":
            cases.append(inp)
            n_value += 1
    too_large = None
    while too_large is None:   # a pair where a segment is shorter than the step but longer than a tenth of the curve
        s = pose(rng)
        g = (s[0] + rng.uniform(-1.5, 1.5), s[1] + rng.uniform(-1.5, 1.5), rng.uniform(-math.pi, math.pi))
        inp = s + g + (1.0, 0.5)
        if "Step size too large" in call(mr, inp)[2]:
            too_large = inp
    cases.append(too_large)
    n_many = 0
    while n_many < 5:   # >= 10 candidates: about 3 % of the pairs at curvature 0.5, none seen at the other curvatures
        inp = pose(rng) + pose(rng) + (0.5, 0.5)
        paths = call(mr, inp)[0]
        if paths is not None and len(paths) >= 10:
            cases.append(inp)
            n_many += 1
    for k in range(N_RANDOM):
        s = pose(rng)
        g = pose(rng) if k % 6 else (s[0] + rng.uniform(-0.3, 0.3), s[1] + rng.uniform(-0.3, 0.3), s[2] + rng.uniform(-0.2, 0.2))
        cases.append(s + g + ((0.1, 0.5, 1.0, 2.0)[k % 4], (0.5, 0.2, 0.5)[k % 3]))

    inp_a, n_cand, err, printed = [], [], [], []
    c_mode, c_nlen, c_len, c_L, c_cnt, xs, ys, yaws, dirs = [], [], [], [], [], [], [], [], []
    for inp in cases:
        paths, e, out = call(mr, inp)
        inp_a.append(inp)
        err.append(e)
        printed.append(out)
        n_cand.append(-1 if paths is None else len(paths))
        for p in paths or []:
            assert isinstance(p.x, list) and isinstance(p.lengths, list) and isinstance(p.directions, list)
            assert all(isinstance(v, float) for v in p.lengths) and set(p.directions) <= {1, -1}
            c_mode.append("".join(p.ctypes))
            c_nlen.append(len(p.lengths))
            c_len.append([float(v) for v in p.lengths] + [0.0] * (5 - len(p.lengths)))
            c_L.append(float(p.L))
            c_cnt.append(len(p.x))
            xs.append(np.asarray(p.x, dtype=np.float64))
            ys.append(np.asarray(p.y, dtype=np.float64))
            yaws.append(np.asarray(p.yaw, dtype=np.float64))
            dirs.append(np.asarray(p.directions, dtype=np.int8))
    cand_off = np.concatenate([[0], np.cumsum([max(v, 0) for v in n_cand])]).astype(np.int64)
    c_L = np.array(c_L, dtype=np.float64)
    conditions(n_cand, err, printed, cand_off, c_L, [c[6] for c in cases])
    dst = os.path.join(GOLD, "steer_all_kat.npz")
    np.savez_compressed(dst, inp=np.array(inp_a, dtype=np.float64), n_cand=np.array(n_cand, dtype=np.int32),
                        err=np.array(err), too_large=np.array(["Step size too large" in p for p in printed]),
                        cand_off=cand_off, c_mode=np.array(c_mode), c_nlen=np.array(c_nlen, dtype=np.int32),
                        c_lengths=np.array(c_len, dtype=np.float64), c_L=c_L,
                        c_off=np.concatenate([[0], np.cumsum(c_cnt)]).astype(np.int64), x=np.concatenate(xs),
                        y=np.concatenate(ys), yaw=np.concatenate(yaws), directions=np.concatenate(dirs))
    size = os.path.getsize(dst)
    print("steer_all_kat: %d pairs, %d candidates (most %d), %d points, %d bytes" % (len(cases), len(c_L), max(n_cand),
                                                                                   int(np.sum(c_cnt)), size))
    assert size < 1000000, size


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
