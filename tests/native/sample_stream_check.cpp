// Host check of rrt_samples.hip.h: the lane-parallel twist and the walk / emit split of the sample-stream kernel against
// the serial generator (rpp::mt_twist, rpp::mt_next, and draw_sample's statements restated below).
//   sample_stream_check            -> runs the checks, prints "ok", exit status 0
//   sample_stream_check dump SEED[,SEED...] RATE SAMPLER COUNT RAND_MIN RAND_MAX GX GY -> the serial stream, one "x y" per line as hex
//                                     bit patterns (the GPU test compares rrtx_get_sample_stream with it)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rrt_samples.hip.h"

// rppk::draw_sample (rrt_kernels.hip.h), statement for statement, on a serial state
static void draw_serial(rpp::MT* rng, rpp::Sobol* sob, int goal_sample_rate, int sampler, double rand_min, double rand_max,
                        double gx, double gy, double* ox, double* oy) {
  double rx, ry;
  if (rpp::mt_randint_0_100(rng) > goal_sample_rate) {
    if (sampler == 1) {
      double q[2];
      rpp::sobol_next(sob, q);
      rx = rand_min + q[0] * (rand_max - rand_min);
      ry = rand_min + q[1] * (rand_max - rand_min);
    } else {
      rx = rpp::mt_uniform(rng, rand_min, rand_max);
      ry = rpp::mt_uniform(rng, rand_min, rand_max);
    }
  } else {
    rx = gx;
    ry = gy;
  }
  *ox = rx;
  *oy = ry;
}

// rrt_sample_stream_kernel's rounds with the lanes run one after another
struct Emu {
  uint32_t raw[2][rppss::MTN], tw[2 * rppss::MTN];
  double lq[rppss::LCAP][2];
  int32_t lkind[rppss::LCAP];
  void regenerate() {
    for (int third = 0; third < 3; third++)
      for (int lane = 63; lane >= 0; lane--) rppss::mt_twist_lane(raw[0], raw[1], third, lane, 64);   // any lane order
    for (int i = 0; i < rppss::MTN; i++) tw[rppss::MTN + i] = rpp::mt_temper(raw[1][i]);
  }
  void run(rpp::MT* rng, rpp::Sobol* sob_io, int max_iter, int rate, int sampler, double rand_min, double rand_max, double gx,
           double gy, double* out) {
    for (int i = 0; i < rppss::MTN; i++) {
      raw[0][i] = rng->mt[i];
      tw[i] = rpp::mt_temper(rng->mt[i]);
    }
    rpp::Sobol sob = *sob_io;
    int pos = rng->pos, cnt = 0;
    regenerate();
    while (cnt < max_iter) {
      rppss::MTWin w = {tw, pos, 2 * rppss::MTN};
      int nl = 0;
      while (w.pos < rppss::MTN && nl < rppss::LCAP && cnt + nl < max_iter) {
        lkind[nl] = rppss::sample_walk(&w, rate, sampler, &sob, lq[nl]);
        nl++;
      }
      pos = w.pos;
      for (int j = nl - 1; j >= 0; j--)
        rppss::sample_emit(tw, 2 * rppss::MTN, lkind[j], lq[j], rand_min, rand_max, gx, gy, &out[2 * (cnt + j)],
                           &out[2 * (cnt + j) + 1]);
      cnt += nl;
      if (cnt < max_iter && pos >= rppss::MTN) {
        memcpy(raw[0], raw[1], sizeof(raw[0]));
        memcpy(tw, tw + rppss::MTN, sizeof(uint32_t) * rppss::MTN);
        regenerate();
        pos -= rppss::MTN;
      }
    }
    const int half = pos <= rppss::MTN ? 0 : 1;
    memcpy(rng->mt, raw[half], sizeof(raw[0]));
    rng->pos = pos - half * rppss::MTN;
    *sob_io = sob;
  }
};

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

int main(int argc, char** argv) {
  if (argc >= 10 && !strcmp(argv[1], "dump")) {
    const int rate = atoi(argv[3]), sampler = atoi(argv[4]), count = atoi(argv[5]);
    const double lo = atof(argv[6]), hi = atof(argv[7]), gx = atof(argv[8]), gy = atof(argv[9]);
    for (char* tok = strtok(argv[2], ","); tok; tok = strtok(nullptr, ",")) {
      rpp::MT rng;
      rpp::Sobol sob;
      memset(&sob, 0, sizeof(sob));
      rpp::mt_seed_u64(&rng, strtoull(tok, nullptr, 10));
      for (int k = 0; k < count; k++) {
        double x, y;
        draw_serial(&rng, &sob, rate, sampler, lo, hi, gx, gy, &x, &y);
        printf("%016llx %016llx\n", (unsigned long long)bits(x), (unsigned long long)bits(y));
      }
    }
    return 0;
  }
  // 1. the twist in thirds, out of place, against mt_twist in place; several generations per seed
  for (uint64_t seed = 1; seed <= 8; seed++) {
    rpp::MT a;
    rpp::mt_seed_u64(&a, seed * 7919u);
    std::vector<uint32_t> o(a.mt, a.mt + 624), w(624, 0u);
    for (int gen = 0; gen < 5; gen++) {
      rpp::mt_twist(a.mt);
      for (int third = 0; third < 3; third++)
        for (int lane = 0; lane < 64; lane++) rppss::mt_twist_lane(o.data(), w.data(), third, (lane * 29) & 63, 64);
      CHECK(!memcmp(a.mt, w.data(), 624 * 4), "twist: seed %llu generation %d differs", (unsigned long long)seed, gen);
      o = w;
    }
  }
  // 2. the stream and the end state: 8 seeds x 2000 samples, goal_sample_rate 0 / 5 / 100, MT and Sobol samplers
  const int N = 2000;
  static Emu emu;
  std::vector<double> par(2 * N);
  int regen_min = 1 << 30;
  for (int sampler = 0; sampler < 2; sampler++)
    for (int rate : {0, 5, 100})
      for (uint64_t seed = 0; seed < 8; seed++) {
        rpp::MT s0, s1;
        rpp::mt_seed_u64(&s0, seed * 1000003u + 17u);
        if (seed == 3) {   // a staged state in the middle of a block, and one on its last word
          for (int k = 0; k < 700; k++) rpp::mt_next(&s0);
        }
        if (seed == 4) {
          for (int k = 0; k < 623; k++) rpp::mt_next(&s0);
        }
        s1 = s0;
        rpp::Sobol b0, b1;
        memset(&b0, 0, sizeof(b0));
        b1 = b0;
        const double lo = -2.0, hi = 15.0, gx = 6.0, gy = 10.0;
        // the serial end state and the words the run consumes
        long words = 0;
        for (int k = 0; k < N; k++) {
          double x, y;
          const int p0 = s0.pos;
          draw_serial(&s0, &b0, rate, sampler, lo, hi, gx, gy, &x, &y);
          words += s0.pos > p0 ? s0.pos - p0 : s0.pos - p0 + 624;
          par[2 * k] = par[2 * k + 1] = 0.0;
        }
        // the serial stream once more, compared sample by sample with the emulated kernel
        rpp::MT s2 = s1;
        rpp::Sobol b2 = b1;
        emu.run(&s1, &b1, N, rate, sampler, lo, hi, gx, gy, par.data());
        for (int k = 0; k < N; k++) {
          double x, y;
          draw_serial(&s2, &b2, rate, sampler, lo, hi, gx, gy, &x, &y);
          CHECK(bits(x) == bits(par[2 * k]) && bits(y) == bits(par[2 * k + 1]), "sampler %d rate %d seed %llu sample %d differs",
                sampler, rate, (unsigned long long)seed, k);
        }
        CHECK(s1.pos == s0.pos && !memcmp(s1.mt, s0.mt, 624 * 4), "sampler %d rate %d seed %llu: end state differs (pos %d vs %d)",
              sampler, rate, (unsigned long long)seed, s1.pos, s0.pos);
        CHECK(b1.index == b0.index && b1.lastq[0] == b0.lastq[0] && b1.lastq[1] == b0.lastq[1],
              "sampler %d rate %d seed %llu: Sobol end state differs", sampler, rate, (unsigned long long)seed);
        if (sampler == 0 && rate != 100 && (int)(words / 624) < regen_min) regen_min = (int)(words / 624);
      }
  CHECK(regen_min >= 14, "only %d regenerations in a run: samples must straddle the 624-word boundary often", regen_min);
  // 3. a plan of no iterations leaves the staged state alone
  {
    rpp::MT s0, s1;
    rpp::mt_seed_u64(&s0, 5u);
    s1 = s0;
    rpp::Sobol b;
    memset(&b, 0, sizeof(b));
    emu.run(&s1, &b, 0, 5, 0, -2.0, 15.0, 6.0, 10.0, par.data());
    CHECK(s1.pos == s0.pos && !memcmp(s1.mt, s0.mt, 624 * 4), "max_iter 0: state changed");
  }
  if (fails) {
    printf("FAILED: %d checks\n", fails);
    return 1;
  }
  printf("ok (at least %d regenerations per MT run)\n", regen_min);
  return 0;
}
