// Stand-alone host check of the gradient-norm launcher's host code (csrc/grad_norm_plan.h): the
// argument checks and the launch arithmetic, replayed index by index as grad_sumsq_kernel walks
// them.  No HIP, no GPU; meant to be built with host sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icsrc csrc/tools/grad_norm_host_check.cpp -o grad_norm_host_check && ./grad_norm_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grad_norm_plan.h"

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// every float of [0, n) is read exactly once, nothing at or past n
static void cover(long long n) {
  const GradNormPlan p = grad_norm_plan(n);
  CHECK(p.n4 * 4 + p.tail == n && p.tail >= 0 && p.tail < 4);
  CHECK(p.blocks >= 1 && p.blocks <= GN_CAP);
  std::vector<unsigned char> seen((size_t)n + 8, 0);      // 8 guard bytes behind n
  const long long stride = (long long)p.blocks * GN_NT * GN_U;
  int trips = 0;
  for (int b = 0; b < p.blocks; ++b) {
    int t = 0;
    for (long long base = (long long)b * GN_NT * GN_U; base < p.n4; base += stride, ++t)
      for (int u = 0; u < GN_U; ++u)
        for (int tid = 0; tid < GN_NT; ++tid) {
          const long long i = base + u * GN_NT + tid;
          if (i < p.n4)
            for (int k = 0; k < 4; ++k) ++seen[(size_t)(4 * i + k)];
        }
    if (t > trips) trips = t;
  }
  for (long long j = p.n4 * 4; j < n; ++j) ++seen[(size_t)j];
  CHECK(trips == p.trips);
  bool once = true;
  for (long long j = 0; j < n; ++j) once = once && seen[(size_t)j] == 1;
  for (int j = 0; j < 8; ++j) once = once && seen[(size_t)n + j] == 0;
  CHECK(once);
}

int main() {
  const long long bs = (long long)GN_NT * GN_U * 4, gs = bs * GN_CAP;
  const long long sizes[] = {1, 2, 3, 4, 5, 7, bs - 1, bs, bs + 1, bs + 4, gs - 1, gs, gs + 4,
                             2 * gs + 7, 11173976, 25557032};
  for (long long n : sizes) cover(n);

  alignas(16) static float g[64];
  static float mx[1], rec[2], ws[GN_CAP];
  const uintptr_t G = (uintptr_t)g, M = (uintptr_t)mx, R = (uintptr_t)rec, W = (uintptr_t)ws;
  CHECK(!throws([&] { grad_norm_check(G, 64, M, R, W, GN_CAP); }));
  CHECK(!throws([&] { grad_norm_check(G, 1, M, R, W, 1); }));
  CHECK(throws([&] { grad_norm_check(G, 0, M, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, -5, M, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(0, 64, M, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, 64, 0, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, 64, M, 0, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, 64, M, R, 0, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G + 4, 60, M, R, W, GN_CAP); }));    // 4-aligned, not 16
  CHECK(throws([&] { grad_norm_check(G + 8, 60, M, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, 64, M + 1, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, gs, M, R, W, GN_CAP - 1); }));    // too few partials
  CHECK(!throws([&] { grad_norm_check(G, gs, M, R, W, GN_CAP); }));
  CHECK(throws([&] { grad_norm_check(G, bs + 4, M, R, W, 1); }));          // two blocks
  // a trip count past int: refused, and nothing overflows on the way there
  CHECK(throws([&] { grad_norm_check(G, 0x7fffffffffffffffLL, M, R, W, GN_CAP); }));
  std::printf(fails ? "grad_norm_host_check: %d failure(s)\n" : "grad_norm_host_check: ok\n",
              fails);
  return fails ? 1 : 0;
}
