#!/usr/bin/env python3
"""Goldens of the obstacle map under the Reeds-Shepp planners by RUNNING the reference classes (build host only).

The reference's check_collision loops over an obstacle_list of any length; these plans run it on the 300-circle scene of
tests/rs_obsmap_util.py (scene(13, 300, 0.03, 0.12), robot_radius 0.05), which the 64-circle tile of the Reeds-Shepp kernel
cannot hold.  The classes are loaded through oracle/ref_loader.py; only data is stored.

  obsmap_rs_m300_s<seed>   rrt_06 `RRT` (oracle/gen_golden.py run_rrt06: the format of every rrt06_* golden), curvature 1.0,
                           step_size 0.2, max_iter 150
  obsmap_cl_m300_s<seed>   rrt_10 `ClosedLoopRRTStar` (tools/gen_golden_closed_loop.py run_plan: the format of every rrt10_*
                           golden), max_iter 40 -- the reference's check_collision is O(circles x points) in Python and its
                           closed-loop stage rolls every candidate out, so 150 iterations on 300 circles take too long.
                           A file is only written when the plan shows what it is for: a candidate refused for collision
                           (fail & 8) next to one that is not.

The `obsmap_` prefix keeps the files out of the parametrised tests over rrt06_* / rrt10_* goldens, which hand their lists to
rrtx_set_obstacles.

    python tools/gen_golden_rs_obstacle_map.py              # the seeds below
    python tools/gen_golden_rs_obstacle_map.py rs 0 1       # rrt_06, these seeds
    python tools/gen_golden_rs_obstacle_map.py cl 3 5 7     # rrt_10, these seeds (kept only when they show the branch)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden  # noqa: E402
import gen_golden_closed_loop as gcl  # noqa: E402
import ref_loader  # noqa: E402
import rs_obsmap_util as R  # noqa: E402

# rrt_10: of seeds 0..11 these show the branch -- s1 returns (False, None, ...) with candidates, s7 and s8 a trajectory
RS_SEEDS, CL_SEEDS = [0, 1], [1, 7, 8]
M = 300


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    seeds = [int(v) for v in sys.argv[2:]]
    rmin, rmax, rr = R.SCENES[M]
    circles = R.scene(R.MAP_SEED, M, rmin, rmax)
    if what in ("all", "rs"):
        m06 = ref_loader.load("rrt_06")
        for s in seeds or RS_SEEDS:
            gen_golden.run_rrt06(m06, "obsmap_rs_m%d_s%d" % (M, s), circles, R.START, R.GOAL, R.RAND_AREA, R.MAX_ITER, s,
                                 curvature=1.0, robot_radius=rr, expand_dis=3.0, ccd=R.CCD, step_size=0.2, until_max=True)
    if what in ("all", "cl"):
        mod = gcl.load()
        kw = dict(gcl.DRIVER, obstacle_list=[list(c) for c in circles], max_iter=R.CL_MAX_ITER, robot_radius=rr)
        for s in seeds or CL_SEEDS:
            res = gcl.run_plan(mod, kw, s)
            fails = res["cand_fail"]
            shown = bool(np.any(fails & gcl.F_COLL)) and bool(np.any((fails & gcl.F_COLL) == 0))
            print("cl seed", s, len(res["x"]), "nodes", len(res["cand"]), "candidates, flag", res["flag"], "fail masks",
                  fails.tolist(), "KEPT" if shown else "NOT KEPT (no candidate with and one without the collision bit)",
                  flush=True)
            if shown:
                np.savez_compressed(os.path.join(gcl.GOLD, "obsmap_cl_m%d_s%d.npz" % (M, s)), **res)


if __name__ == "__main__":
    main()
