// csrc/rpp_node.h on the host: the header carries its own static_asserts (size, alignment, the offsets the kernel's loads
// rely on), so compiling this file is the check; the run repeats them against a real array of records.
#include <cstdint>
#include <cstdio>

#include "rpp_node.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  using rppk::Kid;
  using rppk::Node;
  static_assert(sizeof(Node) == 64 && alignof(Node) == 64, "one 64-byte line per node");
  static_assert(offsetof(Node, k) == 0 && sizeof(Kid) == 16, "the walk record is the first 16 bytes");
  static_assert(offsetof(Node, prev_sib) + sizeof(int32_t) == 32, "walk record, cost and links fill the first half");
  static_assert(offsetof(Node, x) % 16 == 0 && offsetof(Node, y) == offsetof(Node, x) + 8, "x, y: one 16-byte load");
  static_assert(offsetof(Node, xq) + sizeof(uint32_t) <= 64, "the mirror entry is inside the line");
  static Node nd[3];
  for (int i = 0; i < 3; i++) CHECK(reinterpret_cast<uintptr_t>(&nd[i]) % 64 == 0);
  // what the 32-byte link load of a rewire decodes: dwords 1, 6, 7
  nd[1].k = Kid{11, 22, 1.5};
  nd[1].cost = 2.5;
  nd[1].parent = 33;
  nd[1].prev_sib = 44;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&nd[1]);
  CHECK(w[0] == 11u && w[1] == 22u && w[6] == 33u && w[7] == 44u);
  std::printf("ok\n");
  return 0;
}
