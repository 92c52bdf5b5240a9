// Attention pooling over time for the BiLSTM speech model, gfx950 (CDNA4).
//
//   s[b,t] = x[t,b,:] . w      r = max(s, 0)      a[b,t] = softmax over t < len_b of r
//   rep[b,:] = sum_{t < len_b} a[b,t] x[t,b,:]
//
// Memory-bound, no MFMA: the forward reads x once, the backward reads x once and writes dx
// once.  A wave owns whole rows of D: lane l holds the 16-byte chunks l, l + 64, ... of a row
// (NCH of them, so D <= NCH * 64 * E with E = 4 fp32 or 8 bf16 elements per chunk; lanes past D
// idle), the dot product is one cross-lane sum per frame, and G frames are in flight per trip.
// A block is ATTN_BLOCK_WAVES waves on one batch row, each walking its own share of T.
//
// Forward: online softmax per wave -- running max m, denominator l and accumulator acc[D] in
// registers.  r >= 0, so m starts at 0 and no -inf is ever formed; an empty share leaves
// (0, 0, 0), which merges as nothing.  The block's waves merge through LDS in wave order into
// one partial (m, l, acc) per block; attn_pool_combine merges the partials of a row in block
// order, normalises rep, and turns the r the waves parked in attn[] into a.  Frames at
// t >= len_b are never loaded.
//
// Backward: c_b = sum_t a da is taken as g_b . rep_b (rep is the forward's own output; the sum
// it replaces has the same terms), so one pass suffices: da = g . x per frame, ds, dx written
// (zeros past the length), dw accumulated per lane, merged over the block's waves in LDS and
// left as one partial row per block; attn_pool_dw_reduce sums the rows in a fixed order.
//
// No atomics: every output element has one writer and every sum a fixed order, so two runs are
// bit-equal.  Launchers neither allocate nor synchronise.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kWaves = ATTN_BLOCK_WAVES;
constexpr int kThreads = 64 * kWaves;
constexpr int kRedRows = 16;            // row groups of attn_pool_dw_reduce (x 64 columns)
// elements per lane from which the backward keeps 2 frames in flight instead of 4: at 16
// (D = 1024 fp32) 2 frames take 130 VGPRs against 172 and the B = 320 backward 106 us against
// 120 (bf16: 56 against 78), B = 32 unchanged (builds with -DATTN_BWD_WIDE=32)
#ifndef ATTN_BWD_WIDE
#define ATTN_BWD_WIDE 16
#endif

template <typename XT> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int E = 4;
  static MA_DEV void load(const float* p, float (&v)[4]) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  static MA_DEV void store(float* p, const float (&v)[4]) {
    f32x4 q;
    q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    *reinterpret_cast<f32x4*>(p) = q;
  }
};
template <> struct Chunk<bf16> {
  static constexpr int E = 8;
  static MA_DEV void load(const bf16* p, float (&v)[8]) {
    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bf2f(q[e]);
  }
  static MA_DEV void store(bf16* p, const float (&v)[8]) {
    bf16x8 q;
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = f2bf(v[e]);
    *reinterpret_cast<bf16x8*>(p) = q;
  }
};

MA_DEV void load_f32(const float* p, float* v, int n) {   // n = 4 or 8, p 16-byte aligned
  for (int e = 0; e < n; e += 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + e);
    v[e] = q.x; v[e + 1] = q.y; v[e + 2] = q.z; v[e + 3] = q.w;
  }
}

MA_DEV int row_len(const int* lengths, int b, int T) {
  const int len = lengths ? min(max(lengths[b], 0), T) : T;
  return __builtin_amdgcn_readfirstlane(len);
}

template <typename XT, int NCH>
__global__ __launch_bounds__(kThreads) void attn_pool_fwd_kernel(AttnFwdArgs a, int share, int nsb) {
  constexpr int E = Chunk<XT>::E, DP = NCH * 64 * E, G = NCH * E >= 32 ? 2 : 4;
  __shared__ __attribute__((aligned(16))) float red[kWaves][DP];
  __shared__ float ml[kWaves][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
  const int len = row_len(a.lengths, b, a.T);
  const int t0 = (blockIdx.x * kWaves + wv) * share, t1 = min(t0 + share, len);
  const XT* xb = static_cast<const XT*>(a.x) + (size_t)b * a.sb;
  float* attn = a.attn + (size_t)b * a.T;
  float* score = a.score ? a.score + (size_t)b * a.T : nullptr;

  bool act[NCH];
  float wr[NCH][E], acc[NCH][E];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int col = (k * 64 + lane) * E;
    act[k] = col < a.D;
#pragma unroll
    for (int e = 0; e < E; ++e) wr[k][e] = acc[k][e] = 0.f;
    if (act[k]) load_f32(a.w + col, wr[k], E);
  }
  float m = 0.f, l = 0.f;
  for (int t = t0; t < t1; t += G) {
    float xv[G][NCH][E], s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool valid = t + g < t1;
      const XT* row = xb + (size_t)(t + g) * a.st;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        if (valid && act[k]) {
          Chunk<XT>::load(row + (k * 64 + lane) * E, xv[g][k]);
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) xv[g][k][e] = 0.f;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float p = 0.f;
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) p += xv[g][k][e] * wr[k][e];
      s[g] = p;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = wave_sum(s[g]);
    float mn = m;
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (t + g < t1) mn = fmaxf(mn, fmaxf(s[g], 0.f));
    const float keep = expf(m - mn);
    m = mn;
    l *= keep;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[k][e] *= keep;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool valid = t + g < t1;
      const float r = fmaxf(s[g], 0.f);
      const float p = valid ? expf(r - mn) : 0.f;
      l += p;
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[k][e] += p * xv[g][k][e];
      if (valid && lane == 0) {
        attn[t + g] = r;                 // parked for attn_pool_combine
        if (score) score[t + g] = s[g];
      }
    }
  }

  // the block's waves, in wave order
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < E; ++e) red[wv][(k * 64 + lane) * E + e] = acc[k][e];
  if (lane == 0) {
    ml[wv][0] = m;
    ml[wv][1] = l;
  }
  __syncthreads();
  float M = 0.f, f[kWaves];
#pragma unroll
  for (int i = 0; i < kWaves; ++i) M = fmaxf(M, ml[i][0]);
#pragma unroll
  for (int i = 0; i < kWaves; ++i) f[i] = expf(ml[i][0] - M);
  const size_t part = (size_t)b * nsb + blockIdx.x;
  float* pa = a.ws + part * a.D;
  for (int d = threadIdx.x; d < a.D; d += kThreads) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) v += f[i] * red[i][d];
    pa[d] = v;
  }
  if (threadIdx.x == 0) {
    float L = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) L += f[i] * ml[i][1];
    float* pm = a.ws + (size_t)a.B * nsb * a.D + part * 2;
    pm[0] = M;
    pm[1] = L;
  }
}

// grid (ceil(max(D, T) / kThreads), B): thread i of a row finishes rep[b][i] and attn[b][i]
__global__ __launch_bounds__(kThreads) void attn_pool_combine_kernel(AttnFwdArgs a, int nsb) {
  const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const int len = row_len(a.lengths, b, a.T);
  const float* pm = a.ws + (size_t)a.B * nsb * a.D + (size_t)b * nsb * 2;
  float M = 0.f, L = 0.f;
  for (int j = 0; j < nsb; ++j) M = fmaxf(M, pm[2 * j]);
  for (int j = 0; j < nsb; ++j) L += pm[2 * j + 1] * expf(pm[2 * j] - M);
  const float inv = L > 0.f ? 1.f / L : 0.f;
  if (i < a.D) {
    const float* pa = a.ws + (size_t)b * nsb * a.D + i;
    float v = 0.f;
    for (int j = 0; j < nsb; ++j) v += pa[(size_t)j * a.D] * expf(pm[2 * j] - M);
    a.rep[(size_t)b * a.D + i] = v * inv;
  }
  if (i < a.T) {
    const size_t o = (size_t)b * a.T + i;
    if (i < len) {
      a.attn[o] = expf(a.attn[o] - M) * inv;
    } else {
      a.attn[o] = 0.f;
      if (a.score) a.score[o] = 0.f;
    }
  }
}

template <typename XT, int NCH>
__global__ __launch_bounds__(kThreads) void attn_pool_bwd_kernel(AttnBwdArgs a, int share, int nsb) {
  constexpr int E = Chunk<XT>::E, DP = NCH * 64 * E, G = NCH * E >= ATTN_BWD_WIDE ? 2 : 4;
  __shared__ __attribute__((aligned(16))) float red[kWaves][DP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
  const int len = row_len(a.lengths, b, a.T);
  const int t0 = (blockIdx.x * kWaves + wv) * share;
  const int t1 = min(t0 + share, len), tend = min(t0 + share, a.T);
  const XT* xb = static_cast<const XT*>(a.x) + (size_t)b * a.sb;
  XT* dxb = static_cast<XT*>(a.dx) + (size_t)b * a.dsb;
  const float* attn = a.attn + (size_t)b * a.T;
  const float* score = a.score + (size_t)b * a.T;

  bool act[NCH];
  float wr[NCH][E], gr[NCH][E], dwa[NCH][E];
  float cp = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int col = (k * 64 + lane) * E;
    act[k] = col < a.D;
#pragma unroll
    for (int e = 0; e < E; ++e) wr[k][e] = gr[k][e] = dwa[k][e] = 0.f;
    if (act[k]) {
      float rp[E];
      load_f32(a.w + col, wr[k], E);
      load_f32(a.g + (size_t)b * a.D + col, gr[k], E);
      load_f32(a.rep + (size_t)b * a.D + col, rp, E);
#pragma unroll
      for (int e = 0; e < E; ++e) cp += gr[k][e] * rp[e];
    }
  }
  const float c = wave_sum(cp);
  for (int t = t0; t < tend; t += G) {
    float xv[G][NCH][E], da[G], av[G], sv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool valid = t + g < t1;
      const XT* row = xb + (size_t)(t + g) * a.st;
      av[g] = valid ? attn[t + g] : 0.f;
      sv[g] = valid ? score[t + g] : 0.f;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        if (valid && act[k]) {
          Chunk<XT>::load(row + (k * 64 + lane) * E, xv[g][k]);
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) xv[g][k][e] = 0.f;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float p = 0.f;
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) p += xv[g][k][e] * gr[k][e];
      da[g] = p;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) da[g] = wave_sum(da[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (t + g >= tend) break;
      const bool valid = t + g < t1;
      const float ds = valid && sv[g] > 0.f ? av[g] * (da[g] - c) : 0.f;
      XT* row = dxb + (size_t)(t + g) * a.dst;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        float o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          o[e] = valid ? av[g] * gr[k][e] + ds * wr[k][e] : 0.f;
          dwa[k][e] += ds * xv[g][k][e];
        }
        if (act[k]) Chunk<XT>::store(row + (k * 64 + lane) * E, o);
      }
    }
  }

#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < E; ++e) red[wv][(k * 64 + lane) * E + e] = dwa[k][e];
  __syncthreads();
  float* pa = a.ws + ((size_t)b * nsb + blockIdx.x) * a.D;
  for (int d = threadIdx.x; d < a.D; d += kThreads) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) v += red[i][d];
    pa[d] = v;
  }
}

// dw[d] = sum over the `rows` partial rows: grid D / 64, block 64 columns x kRedRows row groups;
// group q adds rows q, q + kRedRows, ... in order, then column d adds the groups in order
__global__ __launch_bounds__(64 * kRedRows) void attn_pool_dw_reduce_kernel(const float* ws,
                                                                            float* dw, int rows,
                                                                            int D) {
  __shared__ float red[kRedRows][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6, d = blockIdx.x * 64 + c;
  float v = 0.f;
  for (int r = q; r < rows; r += kRedRows) v += ws[(size_t)r * D + d];
  red[q][c] = v;
  __syncthreads();
  if (q == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kRedRows; ++i) t += red[i][c];
    dw[d] = t;
  }
}

struct Geom {
  int share, nsb, nch;
};

Geom check_geom(const char* what, int T, int B, int D, int bf16_x, long long st, long long sb,
                const void* x) {
  const std::string w(what);
  if (D < 64 || D % 64 != 0 || D > ATTN_MAX_D)
    throw std::invalid_argument(w + ": D must be a multiple of 64 in [64, " +
                                std::to_string(ATTN_MAX_D) + "]");
  if (B < 1 || T < 1) throw std::invalid_argument(w + ": B and T must be >= 1");
  if (B > 65535) throw std::invalid_argument(w + ": B exceeds a grid dimension");
  if ((long long)B * T > 0x7fffffffLL)
    throw std::invalid_argument(w + ": B * T exceeds a 32-bit index");
  const int epc = bf16_x ? 8 : 4;
  if (st < 0 || sb < 0 || st % epc || sb % epc || reinterpret_cast<uintptr_t>(x) % 16)
    throw std::invalid_argument(w + ": rows must be 16-byte aligned with non-negative strides");
  if ((long long)(T - 1) * st + (long long)(B - 1) * sb + D > (1LL << 40))
    throw std::invalid_argument(w + ": tensor extent out of range");
  Geom g;
  attn_pool_split(T, B, &g.share, &g.nsb);
  const int chunks = (D / epc + 63) / 64;
  g.nch = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 8;
  return g;
}

}  // namespace

void attn_pool_split(int T, int B, int* share, int* nsb) {
  int want = (ATTN_TARGET_WAVES + B - 1) / B;
  want = want < 1 ? 1 : want > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : want;
  int sh = (T + want - 1) / want;
  if (sh < ATTN_WAVE_FRAMES) sh = ATTN_WAVE_FRAMES;
  const int ns = (T + sh - 1) / sh;
  *share = sh;
  *nsb = (ns + ATTN_BLOCK_WAVES - 1) / ATTN_BLOCK_WAVES;
}

#define ATTN_DISPATCH(kernel, ...)                                                     \
  do {                                                                                 \
    if (a.bf16_x) {                                                                    \
      if (g.nch == 1) kernel<bf16, 1><<<grid, kThreads, 0, st>>>(__VA_ARGS__);         \
      else if (g.nch == 2) kernel<bf16, 2><<<grid, kThreads, 0, st>>>(__VA_ARGS__);    \
      else kernel<bf16, 4><<<grid, kThreads, 0, st>>>(__VA_ARGS__);                    \
    } else {                                                                           \
      if (g.nch == 1) kernel<float, 1><<<grid, kThreads, 0, st>>>(__VA_ARGS__);        \
      else if (g.nch == 2) kernel<float, 2><<<grid, kThreads, 0, st>>>(__VA_ARGS__);   \
      else if (g.nch == 4) kernel<float, 4><<<grid, kThreads, 0, st>>>(__VA_ARGS__);   \
      else kernel<float, 8><<<grid, kThreads, 0, st>>>(__VA_ARGS__);                   \
    }                                                                                  \
  } while (0)

void attn_pool_fwd_launch(const AttnFwdArgs& a, hipStream_t st) {
  const Geom g = check_geom("attn_pool_fwd", a.T, a.B, a.D, a.bf16_x, a.st, a.sb, a.x);
  if (!a.x || !a.w || !a.rep || !a.attn || !a.ws)
    throw std::invalid_argument("attn_pool_fwd: null operand");
  if (a.ws_floats < (long long)a.B * g.nsb * (a.D + 2))
    throw std::invalid_argument("attn_pool_fwd: workspace too small");
  const dim3 grid(g.nsb, a.B);
  ATTN_DISPATCH(attn_pool_fwd_kernel, a, g.share, g.nsb);
  const int n = a.D > a.T ? a.D : a.T;
  attn_pool_combine_kernel<<<dim3((n + kThreads - 1) / kThreads, a.B), kThreads, 0, st>>>(a, g.nsb);
  HIP_LAUNCH_CHECK();
}

void attn_pool_bwd_launch(const AttnBwdArgs& a, hipStream_t st) {
  const Geom g = check_geom("attn_pool_bwd", a.T, a.B, a.D, a.bf16_x, a.st, a.sb, a.x);
  check_geom("attn_pool_bwd (dx)", a.T, a.B, a.D, a.bf16_x, a.dst, a.dsb, a.dx);
  if (!a.x || !a.w || !a.g || !a.rep || !a.attn || !a.score || !a.dx || !a.dw || !a.ws)
    throw std::invalid_argument("attn_pool_bwd: null operand");
  if (a.ws_floats < (long long)a.B * g.nsb * a.D)
    throw std::invalid_argument("attn_pool_bwd: workspace too small");
  const dim3 grid(g.nsb, a.B);
  ATTN_DISPATCH(attn_pool_bwd_kernel, a, g.share, g.nsb);
  attn_pool_dw_reduce_kernel<<<a.D / 64, 64 * kRedRows, 0, st>>>(a.ws, a.dw, a.B * g.nsb, a.D);
  HIP_LAUNCH_CHECK();
}
