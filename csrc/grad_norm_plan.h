// Launch arithmetic and argument checks of the gradient-norm pass (csrc/optim.hip
// grad_sumsq_kernel / grad_norm_finish_kernel).  Plain host C++ with no HIP in it, so a
// stand-alone program can run it under host sanitizers; mercury_amd/ops/optim.py
// grad_norm_plan mirrors it line by line (the tests compare the two).
#pragma once
#include <cstdint>
#include <stdexcept>

constexpr int GN_NT = 256;        // threads per block
constexpr int GN_U = 2;           // float4 loads per thread per trip
constexpr int GN_CAP = 1024;      // grid cap: 4 blocks per CU, 32 KB of loads in flight per CU

struct GradNormPlan {
  long long n4;                   // whole float4s, swept by the grid-stride loop
  int tail;                       // n % 4 trailing floats (block 0, thread 0)
  int blocks;                     // grid of the sum-of-squares launch (= partials written)
  int trips;                      // grid-stride trips of the busiest block
};

inline GradNormPlan grad_norm_plan(long long n) {
  if (n < 1) throw std::invalid_argument("grad_norm: n must be >= 1");
  GradNormPlan p;
  p.n4 = n / 4;
  p.tail = (int)(n - p.n4 * 4);
  const long long per_block = (long long)GN_NT * GN_U;
  long long b = (p.n4 + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > GN_CAP) b = GN_CAP;
  p.blocks = (int)b;
  const long long span = b * per_block;
  const long long t = (p.n4 + span - 1) / span;
  if (t > 0x7fffffffLL) throw std::invalid_argument("grad_norm: n too large");
  p.trips = (int)t;
  return p;
}

// The launcher's argument checks: a null pointer, a misaligned base (the float4 loads need 16
// bytes) or a workspace shorter than the grid's partials is an error, never a silent fallback.
inline GradNormPlan grad_norm_check(uintptr_t g, long long n, uintptr_t max_norm, uintptr_t rec,
                                    uintptr_t ws, long long ws_floats) {
  const GradNormPlan p = grad_norm_plan(n);
  if (!g || !max_norm || !rec || !ws) throw std::invalid_argument("grad_norm: null pointer");
  if (g & 15) throw std::invalid_argument("grad_norm: g must be 16-byte aligned");
  if ((max_norm | rec | ws) & 3)
    throw std::invalid_argument("grad_norm: max_norm / record / workspace must be 4-byte aligned");
  if (ws_floats < p.blocks)
    throw std::invalid_argument("grad_norm: workspace holds fewer floats than the grid's partials");
  return p;
}
