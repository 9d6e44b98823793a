// rrt_star_v2_body.inc -- latency-lean RRT* iteration kernel (rrt_04 semantics, search_until_max_iter=True).
//
// Same algorithm, results and HBM layout as rrt_kernels.hip.h (which stays the general path: rrt_01, early-exit
// RRT*, the final goal search), restructured around one measurement: with ~1000 instances streaming their node
// arrays, a dependent global load costs several thousand cycles, and the v1 iteration had ~19 of them on its
// critical path.  Here everything an iteration decides on is carried in LDS / registers:
//   * the scan captures the coordinates of what it finds (nearest node, near-ball hits), so nothing is read back;
//   * each distinct near candidate becomes an LDS record {idx, x, y, cost, first_child, d2, hypot, flags}, filled
//     once (cost / first_child loads overlap the edge evaluation), used by choose_parent, rewire and as the root
//     of the cost propagation;
//   * the cost propagation (rrt_04:1379-1384) walks child lists level by level with frontier entries
//     {idx, cost, x, y, first_child} in LDS: one global round trip per level and sibling, and it refreshes the
//     LDS cost of later rewire candidates it passes, so the sequential rewire order (:1357-1373) needs no re-read;
//   * the nearest-node query of iteration i+1 rides on the near-ball pass of iteration i (see scan_fused in v1).
// What is left on the critical path per iteration: ~1 round trip per successful rewire (sibling links) plus
// ~1 per propagated tree level.  One piece per concern, in dependency order (DESIGN.md 5.1.0 maps them and the phases):
namespace RRT2_NS {
#include "rrt_star_v2_shapes.inc"   // shape constants, the LDS layout Sh2, block reductions
#include "rrt_star_v2_scan64.inc"   // f64 streaming pass (scan2, hit_at2)
#include "rrt_star_v2_q16.inc"      // 16-bit stage: qdist, scan2q_slot, scan2q, the Spec* records
#include "rrt_star_v2_grid.inc"     // grid index of the 16-bit mirror: GridS ... scan2g
#include "rrt_star_v2_cand.inc"     // near candidates and candidate edges: resolve_group ... eval_edges_back2
#include "rrt_star_v2_walk.inc"     // scalar-path tree walks and cost propagation
#include "rrt_star_v2_kernel.inc"   // rrt_star_kernel_v2
}  // namespace RRT2_NS
