// Host unit test of robotics-path-planning_amd/csrc/rpp_bspline.h, used as the two B-spline kernels use it: per course
// bspline_parameter, bspline_knots and bspline_fit on a band workspace of strided planes, then bspline_sample and bspline_eval
// for every point on its own, by index, last point first.
// Reads courses as raw doubles [m, degree, param, mode, count, ds, n_us, x[m], y[m], us[n_us]] and writes per course
// [status, points, length, n_knots, knots.., cx[m], cy[m], x.., y.., yaw.., k.., u..] as raw doubles.
// tests/test_bspline_host.py compares with tests/bspline_oracle.py.  Built plainly and with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>
#include "rpp_bspline.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s courses.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  double head[7];
  while (fread(head, sizeof(double), 7, fi) == 7) {
    const int m = (int)head[0], k = (int)head[1], param = (int)head[2], mode = (int)head[3];
    const int64_t count = (int64_t)head[4], n_us = (int64_t)head[6];
    const double ds = head[5];
    if (m < 2 || k < 1 || k > rpp::kBsplineMaxDegree) return 5;
    std::vector<double> x(m), y(m), us((size_t)n_us);
    if (fread(x.data(), sizeof(double), m, fi) != (size_t)m || fread(y.data(), sizeof(double), m, fi) != (size_t)m) return 3;
    if (n_us && fread(us.data(), sizeof(double), (size_t)n_us, fi) != (size_t)n_us) return 3;
    // exactly the sizes the kernels are given: m parameters, m + k + 1 knots, 2 k + 1 band planes, m coefficients per axis
    const int64_t stride = m + 3;
    std::vector<double> u(m), t((size_t)m + k + 1), ab((size_t)(2 * k + 1) * stride), cx(m, 0.0), cy(m, 0.0);
    int st = rpp::bspline_parameter(x.data(), y.data(), m, param, u.data());
    if (st == rpp::kBsplineOk && m <= k) st = rpp::kBsplineTooFew;
    int64_t cnt = 0;
    double length = 0.0;
    if (st == rpp::kBsplineOk) {
      rpp::bspline_knots(u.data(), m, k, t.data());
      rpp::bspline_fit(u.data(), t.data(), m, k, x.data(), y.data(), ab.data(), stride, cx.data(), cy.data());
      length = u[m - 1];
      cnt = mode == rpp::kBsplineLinspace ? count : mode == rpp::kBsplineArange ? rpp::arange_count(length, ds) : n_us;
    } else {
      t.clear();
    }
    const double rec[4] = {(double)st, (double)cnt, length, (double)t.size()};
    fwrite(rec, sizeof(double), 4, fo);
    if (!t.empty()) fwrite(t.data(), sizeof(double), t.size(), fo);
    fwrite(cx.data(), sizeof(double), m, fo);
    fwrite(cy.data(), sizeof(double), m, fo);
    std::vector<double> out(5 * (size_t)cnt);
    for (int64_t i = cnt - 1; i >= 0; i--) {
      const double v = rpp::bspline_sample(mode, length, cnt, ds, us.data(), i);
      double p[4];
      rpp::bspline_eval(u.data(), x.data(), y.data(), t.data(), cx.data(), cy.data(), m, k, param, v, p);
      for (int q = 0; q < 4; q++) out[q * cnt + i] = p[q];
      out[4 * cnt + i] = v;
    }
    if (!out.empty()) fwrite(out.data(), sizeof(double), out.size(), fo);
  }
  fclose(fo);
  fclose(fi);
  return 0;
}
