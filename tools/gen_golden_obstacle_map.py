#!/usr/bin/env python3
"""Goldens of the obstacle map (rrtx_set_obstacle_map) by RUNNING the reference planners (build host only).

The reference's check_collision loops over an obstacle_list of any length; these three plans run it on a list of 1 000
circles, which the planners' 256-circle tile cannot hold.  The classes are loaded through oracle/ref_loader.py and run by
oracle/gen_golden.py's run_rrt04, so the arrays have the format of every rrt01* / rrt04* golden.  Only data is stored.
The `obsmap_` prefix keeps the files out of tests/util.golden_files(), whose parametrised tests hand every rrt01* /
rrt04* golden to rrtx_set_obstacles.

  obsmap_rrt04_m1000_s5        rrt_04, search_until_max_iter on
  obsmap_rrt04_m1000_s5_early  rrt_04, search_until_max_iter off
  obsmap_rrt01_m1000_s5        rrt_01

Usage: python tools/gen_golden_obstacle_map.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402
import ref_loader  # noqa: E402


def main():
    base = gen_golden.synth_map(13, 1000, 0.3, 0.9)
    c2 = dict(obstacles=base, start=[2, 2], goal=[98, 98], rand_area=[0, 100], expand_dis=2.0, path_resolution=0.25,
              goal_sample_rate=5, play_area=None, robot_radius=0.0, ccd=50.0, max_iter=1500, sobol=0, seed=5)
    m04, m01 = ref_loader.load("rrt_04"), ref_loader.load("rrt_01")
    gen_golden.run_rrt04(m04, "obsmap_rrt04_m1000_s5", until_max=True, **c2)
    gen_golden.run_rrt04(m04, "obsmap_rrt04_m1000_s5_early", until_max=False, **c2)
    gen_golden.run_rrt04(m01, "obsmap_rrt01_m1000_s5", until_max=False, algo="rrt", **c2)


if __name__ == "__main__":
    main()
