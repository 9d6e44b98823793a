"""Golden generator of the stand-alone curve solvers: runs the reference's plan_dubins_path
(10_path_planning_00_dubins_path.py :109) and reeds_shepp_path_planning (10_path_planning_00_reeds_shepp_path.py :506)
themselves (loaded through oracle/ref_loader.py, the two files added to ref_loader.FILES at run time) and writes
tests/golden/steer_kat.npz: the cases tests/golden/dubins_kat.npz and rs_kat.npz lack.  Build host only (needs the
reference checkout).

    python tools/gen_golden_steer.py

Arrays only.  Dubins rows d_*: d_inp = (sx, sy, syaw, gx, gy, gyaw, curvature); d_sel = selected_types as indices into
LSL, RSR, LSR, RSL, RLR, LRL padded with -1, d_nsel their number (-1: selected_types=None); d_n points, -1 where the
reference raises TypeError (no word of the list is feasible: b_mode stays None and _generate_local_course zips over it);
d_mode, d_lengths (3), and the concatenated d_x, d_y, d_yaw.  Reeds-Shepp rows r_*: as rs_kat.npz (r_inp carries
curvature and step; r_n 0 = None, -1 = raises, r_mode then the exception's name)."""
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

ref_loader.FILES["dubins_path"] = "10_path_planning_00_dubins_path.py"
ref_loader.FILES["reeds_shepp_path"] = "10_path_planning_00_reeds_shepp_path.py"
GOLD = os.path.join(ROOT, "tests", "golden")
WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")


def pose(rng):
    return rng.uniform(-2, 15), rng.uniform(-2, 15), rng.uniform(-math.pi, math.pi)


def dubins_cases():
    rng = random.Random(50)
    cases = []   # (inp7, selected_types or None)
    for curv in (0.5, 2.0):
        for _ in range(14):
            cases.append((pose(rng) + pose(rng) + (curv,), None))
    for curv in (1.0, 0.5, 2.0):                       # start = goal
        s = pose(rng)
        cases.append((s + s + (curv,), None))
    for k in range(8):                                 # goal within 0.1 of the start
        s = pose(rng)
        g = (s[0] + rng.uniform(-0.1, 0.1), s[1] + rng.uniform(-0.1, 0.1), rng.uniform(-math.pi, math.pi))
        cases.append((s + g + ((1.0, 0.5, 2.0, 1.0)[k % 4],), None))
    for sel in (["RSL", "RSR"], ["RSR", "RSL"], ["LRL", "RLR", "LSL"], ["LRL"], ["LRL", "LSR", "RSL", "RLR", "RSR", "LSL"],
                ["LSL", "LSL", "RSR"], ["RLR", "LRL"]):
        for _ in range(3):
            cases.append((pose(rng) + pose(rng) + (1.0,), sel))
    # lists without a feasible word: LSR / RSL need the two turning circles apart, RLR / LRL need them close
    s = pose(rng)
    cases.append((s + (s[0] + 0.05, s[1] + 0.02, s[2] + 0.3, 1.0), ["LSR", "RSL"]))
    cases.append((s + (s[0] + 0.05, s[1] + 0.02, s[2] + 0.3, 1.0), ["RSL"]))
    cases.append(((0.0, 0.0, 0.0, 12.0, 3.0, 1.0, 1.0), ["RLR", "LRL"]))
    cases.append(((0.0, 0.0, 0.0, 12.0, 3.0, 1.0, 1.0), ["LRL", "LSL"]))   # the same pose with a feasible word after all
    cases.append(((0.0, 0.0, 0.0, 12.0, 3.0, 1.0, 1.0), []))
    return cases


def main():
    os.makedirs(GOLD, exist_ok=True)
    md = ref_loader.load("dubins_path")
    mr = ref_loader.load("reeds_shepp_path")
    d = dict(inp=[], sel=[], nsel=[], n=[], mode=[], lengths=[], x=[], y=[], yaw=[])
    for inp, sel in dubins_cases():
        d["inp"].append(inp)
        idx = [] if sel is None else [WORDS.index(w) for w in sel]
        d["sel"].append(idx + [-1] * (6 - len(idx)))
        d["nsel"].append(-1 if sel is None else len(sel))
        try:
            px, py, pyaw, mode, lengths = md.plan_dubins_path(*inp, selected_types=sel)
        except TypeError:
            d["n"].append(-1)
            d["mode"].append("TypeError")
            d["lengths"].append([0.0, 0.0, 0.0])
            continue
        assert isinstance(px, np.ndarray) and isinstance(pyaw, np.ndarray) and isinstance(mode, list) and isinstance(lengths, list)
        d["n"].append(len(px))
        d["mode"].append("".join(mode))
        d["lengths"].append([float(v) for v in lengths])
        d["x"].append(np.asarray(px, dtype=np.float64))
        d["y"].append(np.asarray(py, dtype=np.float64))
        d["yaw"].append(np.asarray(pyaw, dtype=np.float64))
    rng = random.Random(60)
    r = dict(inp=[], n=[], mode=[], n_len=[], lengths=[], x=[], y=[], yaw=[])
    rcases = [(-1.0, -4.0, float(np.deg2rad(-20.0)), 5.0, 5.0, float(np.deg2rad(25.0)), 0.1, 0.05)]   # the script's driver call
    for k in range(16):
        s = pose(rng)
        g = pose(rng) if k % 4 else (s[0] + rng.uniform(-0.6, 0.6), s[1] + rng.uniform(-0.6, 0.6), rng.uniform(-math.pi, math.pi))
        rcases.append(s + g + (2.0, 0.05))
    for inp in rcases:
        r["inp"].append(inp)
        err, px = "", None
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                px, py, pyaw, mode, lengths = mr.reeds_shepp_path_planning(*inp)
            except (ZeroDivisionError, ValueError) as e:
                err = type(e).__name__
        if err or px is None:
            r["n"].append(-1 if err else 0)
            r["mode"].append(err)
            r["n_len"].append(0)
            r["lengths"].append([0.0] * 5)
            continue
        assert isinstance(px, list) and isinstance(pyaw, list) and isinstance(mode, list) and isinstance(lengths, list)
        r["n"].append(len(px))
        r["mode"].append("".join(mode))
        r["n_len"].append(len(lengths))
        r["lengths"].append([float(v) for v in lengths] + [0.0] * (5 - len(lengths)))
        r["x"].append(np.asarray(px, dtype=np.float64))
        r["y"].append(np.asarray(py, dtype=np.float64))
        r["yaw"].append(np.asarray(pyaw, dtype=np.float64))

    def cat(v):
        return np.concatenate(v) if v else np.zeros(0)
    dst = os.path.join(GOLD, "steer_kat.npz")
    np.savez_compressed(dst, d_inp=np.array(d["inp"], dtype=np.float64), d_sel=np.array(d["sel"], dtype=np.int32),
                        d_nsel=np.array(d["nsel"], dtype=np.int32), d_n=np.array(d["n"], dtype=np.int32),
                        d_mode=np.array(d["mode"]), d_lengths=np.array(d["lengths"], dtype=np.float64),
                        d_x=cat(d["x"]), d_y=cat(d["y"]), d_yaw=cat(d["yaw"]),
                        r_inp=np.array(r["inp"], dtype=np.float64), r_n=np.array(r["n"], dtype=np.int32),
                        r_mode=np.array(r["mode"]), r_n_len=np.array(r["n_len"], dtype=np.int32),
                        r_lengths=np.array(r["lengths"], dtype=np.float64), r_x=cat(r["x"]), r_y=cat(r["y"]), r_yaw=cat(r["yaw"]))
    print("steer_kat: %d Dubins cases (%d without a feasible word, %d points), %d Reeds-Shepp cases (%d points), %d bytes"
          % (len(d["n"]), sum(1 for v in d["n"] if v < 0), sum(v for v in d["n"] if v > 0), len(r["n"]),
             sum(v for v in r["n"] if v > 0), os.path.getsize(dst)))
    print("Dubins no-word rows:", [(i, d["mode"][i]) for i, v in enumerate(d["n"]) if v < 0])
    print("Reeds-Shepp:", list(zip(r["n"], r["mode"])))


if __name__ == "__main__":
    main()
