// rpp_node.h -- the per-node records of the tree kernels (rrt_kernels.hip.h, rrt_star_v2_body.inc).  Plain layout, no device
// code: the host checks of tests/native compile it as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rppk {

// What a tree walk reads of a node, in one 16-byte record (four to a 64-byte line): its first child, its next sibling
// and elen = hypot(node - its parent), exactly the value calc_new_cost (rrt_04:1375-1377) would compute now.  elen is
// kept by the rrt_04 iteration kernel only (Ctx::has_elen), so cost propagation needs no coordinates and no hypot.
struct alignas(16) Kid {
  int32_t first_child, next_sib;
  double elen;
};
static_assert(sizeof(Kid) == 16 && alignof(Kid) == 16, "one node record is one aligned 16-byte load");
// Everything the hot phases of the rrt_04 iteration kernel read or write of a node, in ONE 64-byte line (Ctx::node; the
// working format of a launch: built from the arrays in its prologue, written back to them in its epilogue).  First half:
// the walk record, then what a hop writes (cost) and what a rewire re-points (parent, prev_sib) -- a hop is one 16-byte
// load and one 8-byte store, the link reads of a rewire one 32-byte scalar load.  Second half: what the candidate gather
// reads (x, y: one 16-byte load) and the 16-bit mirror entry.
struct alignas(64) Node {
  Kid k;
  double cost;
  int32_t parent, prev_sib;
  double x, y;
  uint32_t xq;
  uint32_t pad[3];
};
static_assert(sizeof(Node) == 64 && alignof(Node) == 64, "one node is one 64-byte line");
static_assert(offsetof(Node, k) == 0, "the walk record is the first 16 bytes of the line");
static_assert(offsetof(Node, cost) == 16 && offsetof(Node, parent) == 24 && offsetof(Node, prev_sib) == 28,
              "cost and the links share the walk record's 32-byte half");
static_assert(offsetof(Node, x) == 32 && offsetof(Node, y) == 40 && offsetof(Node, xq) == 48,
              "x, y are one aligned 16-byte load in the other half");

}  // namespace rppk
