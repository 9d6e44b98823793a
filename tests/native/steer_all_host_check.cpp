// Host check of the candidate lists (rpp_rs.h rs_calc_paths, rs_course, rs_point, rs_point_dir) and of the choice among
// free candidates (rpp_collide.h pick_free).  Flat binary files written and read by tests/test_steer_all_host.py and
// tests/test_gpu_steer_all.py (no numpy on this side).
//   kat <blob>          every golden row of tests/golden/steer_all_kat.npz, bit for bit
//   pick                the selection rule on forged key / hit vectors
//   print <in> <out>    the candidates of the pairs in <in> (rows of 8 doubles), for the GPU sweep
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rpp_collide.h"
#include "rpp_rs.h"

struct Cand {
  int32_t variant, nl, npts;
  char modes[8];
  double seglen[5], length, key;
  std::vector<double> x, y, yaw;
  std::vector<int8_t> dir;
};

// status 0 / 1 (no candidates) / 2 (ZeroDivisionError) / 3 (ValueError), as RRTX_STEER_*
static int candidates(const double* inp, std::vector<Cand>& out) {
  static rpp::RsPaths S;
  out.clear();
  rpp::rs_calc_paths(inp[0], inp[1], inp[2], inp[3], inp[4], inp[5], inp[6], inp[7], &S);
  if (S.np < 0) return S.np == -3 ? 2 : 3;
  if (S.np == 0) return 1;
  const double maxc = inp[6];
  for (int i = 0; i < S.np; i++) {
    const int k = S.kept[i];
    Cand c;
    memset(c.modes, 0, 8);
    c.variant = k;
    c.nl = S.n[k];
    c.length = 0.0;
    for (int j = 0; j < 5; j++) {
      c.seglen[j] = j < c.nl ? S.d[k][j] / maxc : 0.0;
      c.length += rpp::dabs(c.seglen[j]);
      if (j < c.nl) c.modes[j] = S.ct[k][j];
    }
    c.key = rpp::dabs(S.L[i] / maxc);
    rpp::RsCourse C;
    rpp::rs_course(S.d[k], S.ct[k], c.nl, inp[0], inp[1], inp[2], maxc, inp[7], &C);
    c.npts = C.total;
    c.x.resize(C.total), c.y.resize(C.total), c.yaw.resize(C.total), c.dir.resize(C.total);
    for (int q = 0; q < C.total; q++) {
      rpp::rs_point(C, q, &c.x[q], &c.y[q], &c.yaw[q]);
      c.dir[q] = (int8_t)rpp::rs_point_dir(C, q);
    }
    out.push_back(c);
  }
  return 0;
}

static int run_kat(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  long bad = 0, cases = 0, cands = 0;
  std::vector<Cand> got;
  for (;;) {
    double inp[8];
    int32_t hdr[2];   // n_cand (-1: raises), status expected
    if (fread(inp, 8, 8, f) != 8 || fread(hdr, 4, 2, f) != 2) break;
    const int st = candidates(inp, got);
    bool ok = st == hdr[1] && (int)got.size() == (hdr[0] > 0 ? hdr[0] : 0);
    for (int i = 0; i < hdr[0]; i++) {
      char mode[8];
      int32_t h2[2];   // n_len, points
      double len[5], L;
      if (fread(mode, 1, 8, f) != 8 || fread(h2, 4, 2, f) != 2 || fread(len, 8, 5, f) != 5 || fread(&L, 8, 1, f) != 1) return 2;
      const size_t n = (size_t)h2[1];
      std::vector<double> x(n), y(n), yaw(n);
      std::vector<int8_t> dir(n);
      if (fread(x.data(), 8, n, f) != n || fread(y.data(), 8, n, f) != n || fread(yaw.data(), 8, n, f) != n ||
          fread(dir.data(), 1, n, f) != n)
        return 2;
      cands++;
      if (!ok || i >= (int)got.size()) continue;
      const Cand& c = got[i];
      ok = c.nl == h2[0] && c.npts == h2[1] && !memcmp(c.modes, mode, 8) && !memcmp(c.seglen, len, 40) && !memcmp(&c.key, &L, 8) &&
           !memcmp(c.x.data(), x.data(), 8 * n) && !memcmp(c.y.data(), y.data(), 8 * n) && !memcmp(c.yaw.data(), yaw.data(), 8 * n) &&
           !memcmp(c.dir.data(), dir.data(), n);
      if (!ok) printf("case %ld candidate %d: word %s vs %s, points %d vs %d\n", cases, i, c.modes, mode, c.npts, h2[1]);
    }
    if (!ok && bad++ < 5) printf("case %ld: status %d vs %d, candidates %zu vs %d\n", cases, st, hdr[1], got.size(), hdr[0]);
    cases++;
  }
  fclose(f);
  printf("steer_all cases %ld candidates %ld mismatches %ld\n", cases, cands, bad);
  return bad || cases == 0;
}

static int run_pick() {
  struct Case {
    int n;
    double key[6];
    int32_t hit[6];
    int chosen, rank, nfree;
  };
  const Case cases[] = {
      {1, {2.0}, {-1}, 0, 0, 1},                                   // one candidate, free
      {1, {2.0}, {4}, 0, 0, 0},                                    // one candidate, blocked: the planner's row
      {3, {3.0, 1.0, 2.0}, {-1, -1, -1}, 1, 0, 3},                 // all free: the planner's own choice
      {3, {3.0, 1.0, 2.0}, {-1, 0, -1}, 2, 1, 2},                  // the shortest blocked: the next by key
      {3, {3.0, 1.0, 2.0}, {-1, 7, 2}, 0, 2, 1},                   // the first free is the longest
      {3, {3.0, 1.0, 2.0}, {5, 7, 2}, 1, 0, 0},                    // none free: the shortest with its hit
      {4, {1.0, 1.0, 1.0, 1.0}, {-1, -1, -1, -1}, 0, 0, 4},        // ties: the first in list order
      {4, {1.0, 1.0, 1.0, 1.0}, {3, -1, -1, 0}, 1, 1, 2},          // ties, the first blocked: the first free of the equals
      {4, {2.0, 1.0, 2.0, 1.0}, {-1, 3, -1, 3}, 0, 2, 2},          // equal keys among the free ones, after two shorter equals
      {5, {2.0, 3.0, 2.0, 1.0, 2.0}, {9, -1, 9, 9, -1}, 4, 3, 2},  // the first free (index 1) is not the shortest free
      {6, {5.0, 4.0, 3.0, 2.0, 1.0, 0.5}, {-1, 1, 1, 1, 1, 1}, 0, 5, 1},
      {3, {1.0, 1.0, 0.5}, {2, 2, 2}, 2, 0, 0},                    // none free, the minimum is the last
  };
  int bad = 0;
  for (const Case& c : cases) {
    int ch = -9, rk = -9, nf = -9;
    rpp::pick_free(c.key, c.hit, c.n, &ch, &rk, &nf);
    if (ch != c.chosen || rk != c.rank || nf != c.nfree) {
      printf("pick case %ld: chosen %d rank %d n_free %d, expected %d %d %d\n", (long)(&c - cases), ch, rk, nf, c.chosen, c.rank, c.nfree);
      bad++;
    }
  }
  printf("pick cases %zu mismatches %d\n", sizeof(cases) / sizeof(cases[0]), bad);
  return bad != 0;
}

static int run_print(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  double inp[8];
  std::vector<Cand> got;
  while (fread(inp, 8, 8, f) == 8) {
    const int32_t hdr[2] = {candidates(inp, got), (int32_t)got.size()};
    fwrite(hdr, 4, 2, o);
    for (const Cand& c : got) {
      const int32_t h2[3] = {c.variant, c.nl, c.npts};
      fwrite(h2, 4, 3, o);
      fwrite(c.modes, 1, 8, o);
      fwrite(c.seglen, 8, 5, o);
      fwrite(&c.length, 8, 1, o);
      fwrite(&c.key, 8, 1, o);
      fwrite(c.x.data(), 8, c.x.size(), o);
      fwrite(c.y.data(), 8, c.y.size(), o);
      fwrite(c.yaw.data(), 8, c.yaw.size(), o);
      fwrite(c.dir.data(), 1, c.dir.size(), o);
    }
  }
  fclose(f);
  return fclose(o) ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "kat")) return run_kat(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "pick")) return run_pick();
  if (argc == 4 && !strcmp(argv[1], "print")) return run_print(argv[2], argv[3]);
  return 2;
}
