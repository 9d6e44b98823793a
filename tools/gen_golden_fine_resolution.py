#!/usr/bin/env python3
"""Goldens at fine path resolutions by RUNNING the reference planners (build host only).

Every other rrt01* / rrt04* golden has a path_resolution of 0.05 or more on a map at the origin.  These plans walk 3000
steps to an extension (path_resolution 0.001, expand_dis 3.0), or sit 1000 away from the origin, where the drift of the
reference's sequential additions decides whether a steer ends snapped on its target.  The scenes are
tests/snap_util.py's; the classes are loaded through oracle/ref_loader.py and run by oracle/gen_golden.py's run_rrt04, so the
arrays have the format of every rrt01* / rrt04* golden (300 iterations: the files stay under 20 KB).  Only data is
stored.  The `fineres_` prefix keeps the files out of tests/util.golden_files().

  fineres_rrt04_s5, fineres_rrt04_s7   rrt_04, the fine scene, path_resolution 0.001
  fineres_rrt01_s5                     rrt_01, the same scene
  fineres_rrt04_off1000_s6             rrt_04, rand_area [1000, 1100], path_resolution 0.01

Usage: python tools/gen_golden_fine_resolution.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import gen_golden  # noqa: E402
import ref_loader  # noqa: E402
import snap_util  # noqa: E402


def args(kw, seed):
    return dict(obstacles=kw["obstacles"], start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"],
                expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"], goal_sample_rate=kw["goal_sample_rate"],
                max_iter=kw["max_iter"], play_area=None, robot_radius=0.0, sobol=0, ccd=kw["connect_circle_dist"],
                until_max=bool(kw["search_until_max_iter"]), seed=seed, algo=kw["algo"])


def main():
    m04, m01 = ref_loader.load("rrt_04"), ref_loader.load("rrt_01")
    fine, rrt, off = snap_util.SCENES["fine"][0], snap_util.SCENES["fine_rrt"][0], snap_util.SCENES["offset_1000"][0]
    gen_golden.run_rrt04(m04, "fineres_rrt04_s5", **args(fine, 5))
    gen_golden.run_rrt04(m04, "fineres_rrt04_s7", **args(fine, 7))
    gen_golden.run_rrt04(m01, "fineres_rrt01_s5", **args(rrt, 5))
    gen_golden.run_rrt04(m04, "fineres_rrt04_off1000_s6", **args(off, 6))


if __name__ == "__main__":
    main()
