#!/usr/bin/env python3
"""Diagnostic (GPU box): per-phase cycle shares of the planner kernel from the -DRRTX_PHASE_TIMERS build.
Usage: RRTX_LIB=robotics-path-planning_amd/librrtx_prof.so python tools/phase_profile.py [instances] [max_iter]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402
import rrt_amd  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
it = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
A = rrt_amd._abi
kw = util.c2_kwargs(it)
h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
             kw["goal_sample_rate"], it, robot_radius=0.0, connect_circle_dist=50.0, search_until_max_iter=True,
             n_instances=B)
h.set_obstacles(kw["obstacles"])
h.seed_instances(list(range(1, B + 1)))
h.plan()
s = h.get_stats()
ph = h.get_phase_cycles()
names = {0: "loop+sample", 1: "nearest scan", 2: "ext steer", 3: "ext collision", 4: "near scan", 5: "exact+dedup",
         6: "choose edges", 7: "choose cost/min", 8: "rewire edges", 13: "rewire seq: pick+links",
         14: "rewire seq: propagate", 9: "rewire seq: tail+append", 11: "bookkeeping"}
# every slot named above is a disjoint span of the iteration; 10 counts lane walks, 12 and 15 the obstacle cull
tot = float(sum(ph[k] for k in names))
print("instances", B, "max_iter", it, "kernel_ms", s["kernel_ms"], "alg GB/s", s["algorithmic_bytes"] / 1e6 / s["kernel_ms"])
for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 9, 11):
    print("  %-30s %6.2f%%  %.1f cycles/iter/inst" % (names[k], 100.0 * ph[k] / tot if tot else 0, ph[k] / max(s["iterations"], 1)))
rw = ph[9] + ph[13] + ph[14]
print("  %-30s %6.2f%%  %.1f cycles/iter/inst" % ("(rewire seq+propagate+append)", 100.0 * rw / tot if tot else 0,
                                                  rw / max(s["iterations"], 1)))
print("  total cycles/iter/inst %.1f" % (tot / max(s["iterations"], 1)))
print("lane walks finished", int(ph[10]) & ((1 << 40) - 1), "pending list full", int(ph[10]) >> 40)
# slots 12 and 15 hold the obstacle-cull counts only when the iteration kernel (rrt_star_v2) ran the whole plan, and the two
# halves of slot 15 are whole only while the iterations of all instances stay below 2^32
if os.environ.get("RRTX_KERNEL") == "v1" or s["replanned"] or s["main_shape"] not in (64, 128, 256):
    print("obstacle cull: no counts (slots 12 and 15 are phase cycles of the general kernel)")
elif s["iterations"] >= 1 << 32:
    print("obstacle cull: no counts (%d iterations: the packed halves of slot 15 may have carried)" % s["iterations"])
else:
    ev, empty, pop = int(ph[15]) & 0xffffffff, int(ph[15]) >> 32, int(ph[12])
    print("obstacle cull: edge evaluations under a mask", ev, "empty masks", empty, "(%.4f)" % (empty / ev if ev else 0.0),
          "popcount sum", pop, "(mean %.4f)" % (pop / ev if ev else 0.0))
print({k: s[k] for k in ("iterations", "edges_unique", "near_unique", "rewires", "propagated", "exact_rescans")})
