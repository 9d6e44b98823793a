// obsindex_host_check.cpp -- the obstacle index of the curve objects on the CPU (tests/test_obstacle_index_host.py): the grid
// of rppo::geometry_box built from the rules of csrc/rpp_obsgrid.h as the build kernels of obstacle_map.hip.h lay it out, and
// rppo::point_first_hit on it against the linear loop rpp::first_hit (csrc/rpp_collide.h), which must agree for every point.
//   obsindex_host_check                  the built-in cases; prints one line per case, exit 1 at the first disagreement
//   obsindex_host_check job.bin out.bin  one map of the caller's:
//     in : robot_radius forced_cells mode m np | m x (ox oy size) | np x (x y)                                      (doubles)
//     out: x0 y0 cell nx ny | reason longest_run | np x (index answer, linear answer) | cells + 2 starts | the records' rows
//          (the starts and the rows are left out when the circles' thresholds or reaches are not all finite)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rpp_collide.h"
#include "rpp_obsgrid.h"

static double (*volatile libm_pow)(double, double) = pow;   // (size + robot_radius) ** 2 as the host API makes it
static double py_sq(double x) { return x == 0.0 ? 0.0 : libm_pow(std::fabs(x), 2.0); }

struct Built {
  rppo::Geom g;
  bool finite = true;
  int64_t longest = 0;
  std::vector<double> rows3;          // the linear rows (ox, oy, thr)
  std::vector<int32_t> start;         // cells + 2
  std::vector<rppo::Item> items;
  rppo::Map map() const { return rppo::Map{g, start.data(), items.data()}; }
};

// count, exclusive sum, fill in ascending circle index; the wide list behind the last cell
static Built build(const double* circ, int64_t m, double rr, int32_t forced) {
  Built B;
  std::vector<double> rho((size_t)m);
  double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
  for (int64_t i = 0; i < m; i++) {
    const double ox = circ[3 * i], oy = circ[3 * i + 1], thr = py_sq(circ[3 * i + 2] + rr);
    B.rows3.insert(B.rows3.end(), {ox, oy, thr});
    rho[i] = rppo::reach(circ[3 * i + 2], rr);
    B.finite = B.finite && std::isfinite(thr) && std::isfinite(rho[i]);
    if (i == 0) lo[0] = hi[0] = ox, lo[1] = hi[1] = oy;
    lo[0] = ox < lo[0] ? ox : lo[0], hi[0] = ox > hi[0] ? ox : hi[0];
    lo[1] = oy < lo[1] ? oy : lo[1], hi[1] = oy > hi[1] ? oy : hi[1];
  }
  B.g = rppo::geometry_box(lo[0], hi[0], lo[1], hi[1], m, forced);
  if (!B.finite) return B;
  const rppo::Geom& g = B.g;
  const int64_t cells = (int64_t)g.nx * g.ny;
  std::vector<int64_t> count((size_t)cells + 1, 0);
  std::vector<rppo::Range> rng((size_t)m);
  for (int64_t i = 0; i < m; i++) {
    rng[i] = rppo::circle_range(g, circ[3 * i], circ[3 * i + 1], rho[i]);
    if (rppo::is_wide(rng[i])) {
      count[cells]++;
      continue;
    }
    for (int32_t cy = rng[i].cy0; cy <= rng[i].cy1; cy++)
      for (int32_t cx = rng[i].cx0; cx <= rng[i].cx1; cx++) count[rppo::cell_id(g, cx, cy)]++;
  }
  B.start.assign((size_t)cells + 2, 0);
  for (int64_t k = 0; k <= cells; k++) {
    B.start[k + 1] = B.start[k] + (int32_t)count[k];
    B.longest = count[k] > B.longest ? count[k] : B.longest;
  }
  std::vector<int32_t> cursor(B.start.begin(), B.start.end() - 1);
  B.items.resize((size_t)B.start[cells + 1]);
  for (int64_t i = 0; i < m; i++) {
    const rppo::Item it = {circ[3 * i], circ[3 * i + 1], B.rows3[3 * i + 2], i};
    if (rppo::is_wide(rng[i])) {
      B.items[cursor[cells]++] = it;
      continue;
    }
    for (int32_t cy = rng[i].cy0; cy <= rng[i].cy1; cy++)
      for (int32_t cx = rng[i].cx0; cx <= rng[i].cx1; cx++) B.items[cursor[rppo::cell_id(g, cx, cy)]++] = it;
  }
  return B;
}

// ---- the built-in cases ---------------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uni(double a, double b) {   // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return a + (b - a) * ((double)(z >> 11) * 0x1p-53);
}

struct Tally {
  int64_t points = 0, hits = 0;
};

static bool same(const Built& B, int64_t m, double x, double y, Tally& t, const char* what) {
  const int32_t want = rpp::first_hit(B.rows3.data(), m, x, y), got = rppo::point_first_hit(B.map(), x, y);
  t.points++;
  t.hits += want >= 0;
  if (want == got) return true;
  printf("MISMATCH %s: point (%.17g, %.17g): index %d, linear %d\n", what, x, y, got, want);
  return false;
}

static bool run_case(const char* name, const std::vector<double>& circ, double rr, int32_t forced, int n_random, double lo,
                     double hi, int32_t want_reason = rppo::WHY_USED) {
  const int64_t m = (int64_t)circ.size() / 3;
  const Built B = build(circ.data(), m, rr, forced);
  const int32_t reason = rppo::index_reason(rppo::IDX_ON, m, B.finite, B.longest);
  if (reason != want_reason) {
    printf("MISMATCH %s: reason %d, expected %d\n", name, reason, want_reason);
    return false;
  }
  if (reason != rppo::WHY_USED) {
    printf("ok %-28s m %6lld: the linear loop serves it (reason %d)\n", name, (long long)m, reason);
    return true;
  }
  Tally t;
  for (int i = 0; i < n_random; i++)
    if (!same(B, m, uni(lo, hi), uni(lo, hi), t, name)) return false;
  // forged: on every circle's boundary along both axes and the diagonal, and one ulp either side
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t j = 0; j < m; j++) {
    const double ox = circ[3 * j], oy = circ[3 * j + 1], a = std::fabs(circ[3 * j + 2] + rr), d = a * 0.7071067811865476;
    const double px[6] = {ox + a, ox - a, ox, ox, ox + d, ox - d}, py[6] = {oy, oy, oy + a, oy - a, oy + d, oy - d};
    for (int q = 0; q < 6; q++) {
      const double xs[3] = {std::nextafter(px[q], -inf), px[q], std::nextafter(px[q], inf)};
      const double ys[3] = {std::nextafter(py[q], -inf), py[q], std::nextafter(py[q], inf)};
      for (int u = 0; u < 3; u++)   // along x, along y, along the diagonal
        if (!same(B, m, q == 2 || q == 3 ? px[q] : xs[u], q < 2 ? py[q] : ys[u], t, name)) return false;
    }
  }
  // special values and points far outside the box
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double sp[] = {-0.0, 0.0, nan, inf, -inf, 1e300, -1e300, 1e6, -1e6, 5e-324};
  for (double sx : sp)
    for (double sy : sp)
      if (!same(B, m, sx, sy, t, name)) return false;
  for (int64_t j = 0; j < m && j < 64; j++)
    for (double s : sp)
      if (!same(B, m, circ[3 * j], s, t, name) || !same(B, m, s, circ[3 * j + 1], t, name)) return false;
  const int64_t cells = (int64_t)B.g.nx * B.g.ny;
  printf("ok %-28s m %6lld cells %4d^2 wide %5d longest run %5lld: %lld points, %lld hits\n", name, (long long)m, B.g.nx,
         B.start[cells + 1] - B.start[cells], (long long)B.longest, (long long)t.points, (long long)t.hits);
  return true;
}

static std::vector<double> random_map(int64_t m, double lo, double hi, double smin, double smax) {
  std::vector<double> c;
  for (int64_t i = 0; i < m; i++) c.insert(c.end(), {uni(lo, hi), uni(lo, hi), uni(smin, smax)});
  return c;
}

static int selftest() {
  bool ok = true;
  const int N = 100000;
  ok = ok && run_case("1000 circles", random_map(1000, 0, 100, 0.3, 0.9), 0.1, 0, N, -5, 105);
  {
    std::vector<double> c = random_map(1000, 0, 100, 0.3, 0.9);   // wide circles with a lower and a higher index than a cell hit
    c[3 * 0 + 2] = 40.0, c[3 * 500 + 2] = 25.0, c[3 * 999 + 2] = 60.0;
    ok = ok && run_case("1000 + three wide, rr 0.25", c, 0.25, 0, N, -20, 120);
  }
  ok = ok && run_case("5000 small circles", random_map(5000, 0, 100, 0.01, 0.4), 0.0, 0, N, -1, 101);
  ok = ok && run_case("257 sizes -1.5 .. 3", random_map(257, 0, 100, -1.5, 3.0), 0.0, 0, N, -5, 105);
  ok = ok && run_case("negative size + radius", random_map(300, 0, 100, -2.0, -0.5), 0.25, 0, N, -5, 105);
  ok = ok && run_case("offset map", random_map(1000, 1000, 1100, 0.3, 0.9), 0.1, 0, N, 990, 1110);
  ok = ok && run_case("m = 1", {3.0, 4.0, 1.5}, 0.5, 0, N, -2, 9);
  ok = ok && run_case("m = 0", {}, 0.5, 0, 0, 0, 1, rppo::WHY_EMPTY);
  {
    std::vector<double> c;   // a box of zero width: all centres equal (a short run: below RUN_MAX)
    for (int i = 0; i < 300; i++) c.insert(c.end(), {7.0, -3.0, 0.01 * (i % 17)});
    ok = ok && run_case("zero-width box", c, 0.1, 0, N, 6, 8);
  }
  {
    std::vector<double> c = random_map(500, 0, 100, 0.3, 0.9);   // zero width along one axis only
    for (int i = 0; i < 500; i++) c[3 * i + 1] = 2.5;
    ok = ok && run_case("zero-height box", c, 0.0, 0, N, -5, 105);
  }
  ok = ok && run_case("forced = 1", random_map(1000, 0, 100, 0.3, 0.9), 0.1, 1, N / 10, -5, 105);
  ok = ok && run_case("forced = 7", random_map(1000, 0, 100, 0.3, 0.9), 0.1, 7, N, -5, 105);
  {
    std::vector<double> c;   // coincident circles: a run longer than RUN_MAX
    for (int i = 0; i < 5000; i++) c.insert(c.end(), {1.0, 2.0, 0.5});
    ok = ok && run_case("5000 coincident", c, 0.0, 0, 0, 0, 1, rppo::WHY_RUN_TOO_LONG);
  }
  {
    std::vector<double> c = random_map(300, 0, 100, 0.3, 0.9);
    c[3 * 100 + 2] = 1e200;   // (size + r) ** 2 = inf
    ok = ok && run_case("size 1e200", c, 0.0, 0, 0, 0, 1, rppo::WHY_NOT_FINITE);
  }
  return ok ? 0 : 1;
}

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
  if (argc == 1) return selftest();
  if (argc != 3) return 2;
  const std::vector<double> in = read_all(argv[1]);
  if (in.size() < 5) return 3;
  const double rr = in[0];
  const int32_t forced = (int32_t)in[1], mode = (int32_t)in[2];
  const int64_t m = (int64_t)in[3], np = (int64_t)in[4];
  if (in.size() != (size_t)(5 + 3 * m + 2 * np)) return 4;
  const double* circ = in.data() + 5;
  const double* pts = circ + 3 * m;
  const Built B = build(circ, m, rr, forced);
  std::vector<double> out = {B.g.x0, B.g.y0, B.g.cell, (double)B.g.nx, (double)B.g.ny};
  out.push_back((double)rppo::index_reason(mode, m, B.finite, B.longest));
  out.push_back((double)B.longest);
  for (int64_t q = 0; q < np; q++) {
    const double x = pts[2 * q], y = pts[2 * q + 1];
    out.push_back(B.finite && m > 0 ? (double)rppo::point_first_hit(B.map(), x, y) : -3.0);
    out.push_back((double)rpp::first_hit(B.rows3.data(), m, x, y));
  }
  if (B.finite) {
    for (int32_t s : B.start) out.push_back((double)s);
    for (const rppo::Item& it : B.items) out.push_back((double)it.index);
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 5;
  fwrite(out.data(), sizeof(double), out.size(), f);
  fclose(f);
  return 0;
}
