// obsgrid_host_check.cpp -- csrc/rpp_obsgrid.h on the CPU (tests/test_obstacle_map_host.py): the geometry of a map, every
// circle's reach, cell range and wide flag, the cell ranges of query boxes, and the whole CSR as the build kernels of
// obstacle_map.hip.h lay it out (count, exclusive sum, fill in ascending circle index, the wide list behind the last cell).
//   in : rand_min rand_max robot_radius forced_cells m nq | m x (ox oy size) | nq x (xlo xhi ylo yhi)       (doubles)
//   out: x0 y0 cell nx ny | m x (rho cx0 cx1 cy0 cy1 wide) | nq x (cx0 cx1 cy0 cy1) | cells + 2 starts | the records' circle rows
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rpp_obsgrid.h"

static std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  double buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<double> in = read_all(argv[1]);
  if (in.size() < 6) return 3;
  const double rand_min = in[0], rand_max = in[1], rr = in[2];
  const int32_t forced = (int32_t)in[3];
  const int64_t m = (int64_t)in[4], nq = (int64_t)in[5];
  if (in.size() != (size_t)(6 + 3 * m + 4 * nq)) return 4;
  const double* circ = in.data() + 6;
  const double* box = circ + 3 * m;
  std::vector<double> out;
  const rppo::Geom g = rppo::geometry(rand_min, rand_max, m, forced);
  out.insert(out.end(), {g.x0, g.y0, g.cell, (double)g.nx, (double)g.ny});
  const int64_t cells = (int64_t)g.nx * g.ny;
  std::vector<int64_t> count((size_t)cells + 1, 0);
  std::vector<rppo::Range> rng((size_t)m);
  for (int64_t i = 0; i < m; i++) {
    const double rho = rppo::reach(circ[3 * i + 2], rr);
    const rppo::Range r = rppo::circle_range(g, circ[3 * i], circ[3 * i + 1], rho);
    rng[i] = r;
    const bool wide = rppo::is_wide(r);
    out.insert(out.end(), {rho, (double)r.cx0, (double)r.cx1, (double)r.cy0, (double)r.cy1, wide ? 1.0 : 0.0});
    if (wide) {
      count[cells]++;
      continue;
    }
    for (int32_t cy = r.cy0; cy <= r.cy1; cy++)
      for (int32_t cx = r.cx0; cx <= r.cx1; cx++) count[rppo::cell_id(g, cx, cy)]++;
  }
  for (int64_t q = 0; q < nq; q++) {
    const rppo::Range r = rppo::range_of(g, box[4 * q], box[4 * q + 1], box[4 * q + 2], box[4 * q + 3]);
    out.insert(out.end(), {(double)r.cx0, (double)r.cx1, (double)r.cy0, (double)r.cy1});
  }
  std::vector<int64_t> start((size_t)cells + 2, 0);
  for (int64_t k = 0; k <= cells; k++) start[k + 1] = start[k] + count[k];
  std::vector<int64_t> cursor(start.begin(), start.end() - 1);
  std::vector<double> rows((size_t)start[cells + 1], -1.0);
  for (int64_t i = 0; i < m; i++) {
    const rppo::Range& r = rng[i];
    if (rppo::is_wide(r)) {
      rows[cursor[cells]++] = (double)i;
      continue;
    }
    for (int32_t cy = r.cy0; cy <= r.cy1; cy++)
      for (int32_t cx = r.cx0; cx <= r.cx1; cx++) rows[cursor[rppo::cell_id(g, cx, cy)]++] = (double)i;
  }
  for (int64_t k = 0; k < cells + 2; k++) out.push_back((double)start[k]);
  out.insert(out.end(), rows.begin(), rows.end());
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 5;
  fwrite(out.data(), sizeof(double), out.size(), f);
  fclose(f);
  return 0;
}
