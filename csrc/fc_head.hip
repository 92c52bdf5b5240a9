// The speech LSTM's classifier head: Linear(K, N) + BatchNorm1d(N) + ReLU +
// Linear(N, C) with the two dropouts of MyLSTM.forward around it, forward and backward.
//
//   zd = bf16(z * m0)            y = zd . bf16(W1)^T + b1                       [B][N] fp32
//   mean, var over the B rows (training) or the running pair (eval); rstd = rsqrt(var + eps)
//   a2 = bf16(relu(gamma * (y - mean) * rstd + beta) * m1)                      [B][N]
//   logits = a2 . bf16(W2)^T + b2                                               [B][C] fp32
//
// m0 / m1 are uint8 keep-masks ([B][K] / [B][N], null = keep all) and ``scale`` = 1 / (1 - p) the
// value of a kept element; they are applied in the operand loads and epilogues, nothing draws a
// random number here.  Every GEMM operand is rounded to bf16 (RNE) in registers, every sum and
// all BN arithmetic is fp32, and the weights are read as the modules' own fp32 tensors.
//
// BatchNorm1d needs per-column statistics over the whole batch and B is small, so the unit of
// work is a STRIP OF 16 COLUMNS OF N FOR ALL B ROWS.  With the weights as the MFMA "A" input of
// v_mfma_f32_16x16x32_bf16 (as lstm.hip / lstm_proj.hip) a lane's accumulator is row
// m = lane & 15 of a 16-row tile and 4 consecutive columns 4 (lane >> 4) + 0..3, so a column's
// statistics are a sum over the lane's RT row tiles plus a reduction over the 16 lanes of its
// group: no second pass over y, no atomics, nothing shared between workgroups.  The kernels are
// templates on RT, the number of 16-row tiles held (2, 4, 8 or 20: B <= 320); rows past B are
// clamped loads (a B-operand column only reaches its own output column) and guarded stores.
//
//   fc_bn_fwd_kernel<RT, NW>  a block of NW waves per strip.  Wave w takes the 32-deep K-chunks
//     w, w + NW, ...: one W1 fragment (two 16-byte fp32 loads, rounded in registers) against RT
//     z fragments.  Waves 1.. leave their accumulators in LDS; wave 0 adds them in wave order,
//     adds b1, forms mean and the CENTRED variance from the y it holds in registers, and stores
//     y (when a backward will follow), mean, rstd, a2 and, in training, the running statistics
//     of its 16 columns (unbiased variance) -- block 0 also counts the batch.
//   fc_out_kernel  one 16 (rows) x 16 (classes) tile of the logits per block; its 8 waves split
//     the reduction over N and merge in LDS in wave order.  A class row past C is the clamped
//     row C - 1: an A-operand row only reaches its own output row, which is not stored.
//   fc_bn_bwd_kernel<RT>  the forward's strips, 8 waves.  Row tile i belongs to wave i % 8:
//     da2 = bf16(dlogits) . bf16(W2[:, strip]) on the MFMA, dh = da2 * m1 * (a2 > 0), the lane
//     sums of dh and dh * xhat; the waves' 16-lane sums meet in LDS and are added in wave order
//     (dbeta, dgamma), then dy = gamma * rstd * (dh - dbeta / B - xhat * dgamma / B) (eval:
//     gamma * rstd * dh) goes out as bf16 [B][N] for fc_dz_kernel and into LDS, and its fp32
//     column sum is db1.  From the strip's dy and a2 in LDS the block then writes
//     dW2[:, strip] = bf16(dlogits)^T . a2 (class tiles over the waves; block 0 also db2) and
//     its 16 rows of dW1 = dy^T . zd (16-column tiles of K over the waves, reduction over B).
//   fc_dz_kernel<RT>  dz = (dy . bf16(W1)) * m0.  A block owns 32 columns of K for all rows; its
//     8 waves are RG row groups x NS splits of the reduction over N.  A wave loads its 32 (n) x
//     32 (k) tile of W1 along K (128-byte rows), rounds it and stages it in LDS as it lies in
//     memory with rows padded to 72 bytes, so the transposed fragment reads (8 n of one k) of
//     the four 16-lane groups fall in distinct banks; the splits merge in LDS in order.
//
// Every output element has one writer and every reduction a fixed order: two runs are bit-equal.
// No launcher allocates or synchronises; dy is the caller's workspace.
#include <stdexcept>
#include <string>

#include "bn_math.h"
#include "common.h"
#include "kernels.h"

namespace {

MA_DEV f32x4 fc_zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
MA_DEV bf16x8 fc_cvt8(f32x4 lo, f32x4 hi) {
  return bf16x8{f2bf(lo[0]), f2bf(lo[1]), f2bf(lo[2]), f2bf(lo[3]),
                f2bf(hi[0]), f2bf(hi[1]), f2bf(hi[2]), f2bf(hi[3])};
}
MA_DEV bf16x8 fc_zero8() { return fc_cvt8(fc_zero(), fc_zero()); }
// byte e of four keep-mask bytes as the factor of a kept / dropped element
MA_DEV float fc_keep(uint32_t word, int e, float scale) {
  return ((word >> (8 * e)) & 0xffu) ? scale : 0.f;
}
MA_DEV f32x4 fc_keep4(const uint8_t* m, size_t off, float scale) {
  if (!m) return f32x4{1.f, 1.f, 1.f, 1.f};
  const uint32_t word = *(const uint32_t*)(m + off);
  return f32x4{fc_keep(word, 0, scale), fc_keep(word, 1, scale), fc_keep(word, 2, scale),
               fc_keep(word, 3, scale)};
}
// sum over the 16 lanes of a group (the rows of a tile)
MA_DEV float fc_rows_sum(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
MA_DEV f32x4 fc_rows_sum4(f32x4 v) {
  return f32x4{fc_rows_sum(v[0]), fc_rows_sum(v[1]), fc_rows_sum(v[2]), fc_rows_sum(v[3])};
}
MA_DEV f32x4 fc_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------------------ forward
template <int RT, int NW>
__global__ __launch_bounds__(NW * 64) void fc_bn_fwd_kernel(FcHeadFwdArgs g) {
  __shared__ f32x4 part[(NW - 1) * RT * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int B = g.B, K = g.K, N = g.N;
  const int n0 = blockIdx.x * 16;

  f32x4 acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = fc_zero();

  const float* wrow = g.w1 + (size_t)(n0 + li) * K + 8 * q;
  for (int k = w * 32; k < K; k += NW * 32) {
    const bf16x8 fw = fc_cvt8(*(const f32x4*)(wrow + k), *(const f32x4*)(wrow + k + 4));
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const size_t off = (size_t)min(16 * i + li, B - 1) * K + k + 8 * q;
      const f32x4 lo = *(const f32x4*)(g.z + off) * fc_keep4(g.m0, off, g.scale);
      const f32x4 hi = *(const f32x4*)(g.z + off + 4) * fc_keep4(g.m0, off + 4, g.scale);
      acc[i] = fc_mfma(fw, fc_cvt8(lo, hi), acc[i]);
    }
  }

  if (w > 0) {
#pragma unroll
    for (int i = 0; i < RT; ++i) part[((w - 1) * RT + i) * 64 + lane] = acc[i];
  }
  __syncthreads();
  if (w > 0) return;
  for (int p = 0; p < NW - 1; ++p) {
#pragma unroll
    for (int i = 0; i < RT; ++i) acc[i] += part[(p * RT + i) * 64 + lane];
  }

  // wave 0: lane holds y[16 i + li][nb .. nb + 3]
  const int nb = n0 + 4 * q;
  const f32x4 bias = *(const f32x4*)(g.b1 + nb);
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] += bias;

  f32x4 mean, rstd;
  if (g.train) {
    // y is in registers, so the variance is the centred sum: no E[y^2] - mean^2 cancellation
    const float invB = 1.f / (float)B;
    f32x4 s = fc_zero();
#pragma unroll
    for (int i = 0; i < RT; ++i)
      if (16 * i + li < B) s += acc[i];
    mean = fc_rows_sum4(s) * invB;
    f32x4 v = fc_zero();
#pragma unroll
    for (int i = 0; i < RT; ++i)
      if (16 * i + li < B) v += (acc[i] - mean) * (acc[i] - mean);
    const f32x4 var = fc_rows_sum4(v) * invB;
#pragma unroll
    for (int j = 0; j < 4; ++j) rstd[j] = rsqrtf(var[j] + g.eps);
    if (g.run_mean && li == 0) {
      const float unb = (float)B / (float)(B - 1), mo = g.momentum;
      const f32x4 rm = *(const f32x4*)(g.run_mean + nb), rv = *(const f32x4*)(g.run_var + nb);
      *(f32x4*)(g.run_mean + nb) = rm * (1.f - mo) + mean * mo;
      *(f32x4*)(g.run_var + nb) = rv * (1.f - mo) + var * (unb * mo);
    }
    if (g.batches && blockIdx.x == 0 && lane == 0) *g.batches += 1;
  } else {
    mean = *(const f32x4*)(g.run_mean + nb);
    const f32x4 var = *(const f32x4*)(g.run_var + nb);
#pragma unroll
    for (int j = 0; j < 4; ++j) rstd[j] = rsqrtf(var[j] + g.eps);
  }
  if (li == 0) {
    *(f32x4*)(g.mean + nb) = mean;
    *(f32x4*)(g.rstd + nb) = rstd;
  }
  const f32x4 sc = *(const f32x4*)(g.gamma + nb) * rstd, beta = *(const f32x4*)(g.beta + nb);
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int m = 16 * i + li;
    if (m >= B) continue;
    const size_t off = (size_t)m * N + nb;
    if (g.y) *(f32x4*)(g.y + off) = acc[i];
    const f32x4 keep = fc_keep4(g.m1, off, g.scale);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = f2bf(act_fwd((acc[i][j] - mean[j]) * sc[j] + beta[j], 1) * keep[j]);
    *(bf16x4*)(g.a2 + off) = o;
  }
}

constexpr int OUT_NW = 8;

__global__ __launch_bounds__(OUT_NW * 64) void fc_out_kernel(FcHeadFwdArgs g) {
  __shared__ f32x4 part[(OUT_NW - 1) * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int B = g.B, N = g.N, C = g.C;
  const int c0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const float* wp = g.w2 + (size_t)min(c0 + li, C - 1) * N;
  const bf16* ap = g.a2 + (size_t)min(r0 + li, B - 1) * N;

  f32x4 acc = fc_zero();
  for (int k = w * 32; k < N; k += OUT_NW * 32) {
    const bool ok = k + 8 * q < N;                 // N % 16 == 0: the last chunk may be half
    const int kk = ok ? k + 8 * q : 0;
    const bf16x8 fw = fc_cvt8(*(const f32x4*)(wp + kk), *(const f32x4*)(wp + kk + 4));
    const bf16x8 fa = ok ? *(const bf16x8*)(ap + kk) : fc_zero8();
    acc = fc_mfma(fw, fa, acc);
  }
  if (w > 0) part[(w - 1) * 64 + lane] = acc;
  __syncthreads();
  if (w > 0) return;
  for (int p = 0; p < OUT_NW - 1; ++p) acc += part[p * 64 + lane];

  const int m = r0 + li;
  if (m >= B) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + 4 * q + j;
    if (c < C) g.logits[(size_t)m * C + c] = acc[j] + g.b2[c];
  }
}

// ------------------------------------------------------------------------------ backward
constexpr int BWD_NW = 8;

template <int RT>
__global__ __launch_bounds__(BWD_NW * 64) void fc_bn_bwd_kernel(FcHeadBwdArgs g) {
  static_assert(RT % 2 == 0, "the reductions over B walk 32 rows a step");
  constexpr int TPW = (RT + BWD_NW - 1) / BWD_NW;       // row tiles per wave
  __shared__ __attribute__((aligned(16))) bf16 dyS[RT * 16 * 16];     // [row][strip column]
  __shared__ __attribute__((aligned(16))) bf16 a2S[RT * 16 * 16];
  __shared__ __attribute__((aligned(16))) float red[BWD_NW * 3 * 16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int B = g.B, K = g.K, N = g.N, C = g.C;
  const int n0 = blockIdx.x * 16, nb = n0 + 4 * q;

  const f32x4 mean = *(const f32x4*)(g.mean + nb), rstd = *(const f32x4*)(g.rstd + nb);
  const f32x4 sc = *(const f32x4*)(g.gamma + nb) * rstd;

  // ---- da2, dh and the two sums over the batch
  f32x4 dh[TPW], xh[TPW];
  f32x4 s1 = fc_zero(), s2 = fc_zero();
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int i = w + BWD_NW * t;                       // wave-uniform
    dh[t] = xh[t] = fc_zero();
    if (i >= RT) continue;
    const int m = 16 * i + li, mc = min(m, B - 1);
    f32x4 acc = fc_zero();
    for (int c0 = 0; c0 < C; c0 += 32) {
      float fw[8], fd[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + 8 * q + e, cc = min(c, C - 1);
        const float wv = g.w2[(size_t)cc * N + n0 + li];
        fw[e] = c < C ? wv : 0.f;                       // the reduction index is padded with zeros
        fd[e] = g.dlogits[(size_t)mc * C + cc];
      }
      acc = fc_mfma(fc_cvt8(f32x4{fw[0], fw[1], fw[2], fw[3]}, f32x4{fw[4], fw[5], fw[6], fw[7]}),
                    fc_cvt8(f32x4{fd[0], fd[1], fd[2], fd[3]}, f32x4{fd[4], fd[5], fd[6], fd[7]}),
                    acc);
    }
    const size_t off = (size_t)mc * N + nb;
    const f32x4 y = *(const f32x4*)(g.y + off);
    const bf16x4 a2 = *(const bf16x4*)(g.a2 + off);
    const f32x4 keep = fc_keep4(g.m1, off, g.scale);
    const bool valid = m < B;
    bf16x4 a2z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dh[t][j] = valid ? acc[j] * keep[j] * act_mask(bf2f(a2[j]), 1) : 0.f;
      xh[t][j] = (y[j] - mean[j]) * rstd[j];
      a2z[j] = valid ? a2[j] : f2bf(0.f);
    }
    *(bf16x4*)(a2S + m * 16 + 4 * q) = a2z;
    s1 += dh[t];
    s2 += dh[t] * xh[t];
  }
  s1 = fc_rows_sum4(s1);
  s2 = fc_rows_sum4(s2);
  if (li == 0) {
    *(f32x4*)(red + (w * 3 + 0) * 16 + 4 * q) = s1;
    *(f32x4*)(red + (w * 3 + 1) * 16 + 4 * q) = s2;
  }
  __syncthreads();
  f32x4 S1 = fc_zero(), S2 = fc_zero();
  for (int p = 0; p < BWD_NW; ++p) {
    S1 += *(const f32x4*)(red + (p * 3 + 0) * 16 + 4 * q);
    S2 += *(const f32x4*)(red + (p * 3 + 1) * 16 + 4 * q);
  }

  // ---- dy: bf16 to the workspace and to LDS; its fp32 column sum is db1
  const float invB = 1.f / (float)B;
  f32x4 s3 = fc_zero();
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int i = w + BWD_NW * t;
    if (i >= RT) continue;
    const int m = 16 * i + li;
    const bool valid = m < B;
    f32x4 dy;
    if (g.train) dy = sc * (dh[t] - S1 * invB - xh[t] * (S2 * invB));
    else dy = sc * dh[t];
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dy[j] = valid ? dy[j] : 0.f;
      o[j] = f2bf(dy[j]);
    }
    s3 += dy;
    *(bf16x4*)(dyS + m * 16 + 4 * q) = o;
    if (valid) *(bf16x4*)(g.dy + (size_t)m * N + nb) = o;
  }
  s3 = fc_rows_sum4(s3);
  if (li == 0) *(f32x4*)(red + (w * 3 + 2) * 16 + 4 * q) = s3;
  __syncthreads();                                      // dyS, a2S and the third sum are complete
  if (w == 0 && li == 0) {
    f32x4 S3 = fc_zero();
    for (int p = 0; p < BWD_NW; ++p) S3 += *(const f32x4*)(red + (p * 3 + 2) * 16 + 4 * q);
    *(f32x4*)(g.dbeta + nb) = S1;
    *(f32x4*)(g.dgamma + nb) = S2;
    *(f32x4*)(g.db1 + nb) = S3;
  }

  // ---- dW2[c][strip] = sum_m bf16(dlogits[m][c]) * a2[m][strip]; lane holds 4 strip columns
  for (int ct = w; ct * 16 < C; ct += BWD_NW) {
    const int c = ct * 16 + li, cc = min(c, C - 1);
    f32x4 acc = fc_zero();
#pragma unroll 2
    for (int r0 = 0; r0 < RT * 16; r0 += 32) {
      bf16x8 fa;
      float fd[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = r0 + 8 * q + e;
        fa[e] = a2S[m * 16 + li];                       // zero at m >= B
        fd[e] = g.dlogits[(size_t)min(m, B - 1) * C + cc];
      }
      acc = fc_mfma(fa, fc_cvt8(f32x4{fd[0], fd[1], fd[2], fd[3]}, f32x4{fd[4], fd[5], fd[6], fd[7]}),
                    acc);
    }
    if (c < C) *(f32x4*)(g.dw2 + (size_t)c * N + nb) = acc;
  }
  if (blockIdx.x == 0) {
    for (int c = tid; c < C; c += BWD_NW * 64) {
      float s = 0.f;
      for (int m = 0; m < B; ++m) s += g.dlogits[(size_t)m * C + c];
      g.db2[c] = s;
    }
  }

  // ---- dW1[strip row][k] = sum_m dy[m][row] * zd[m][k]; zd is the "A" input, so a lane holds 4
  // consecutive k of row n0 + li
  for (int kt = w; kt * 16 < K; kt += BWD_NW) {
    f32x4 acc = fc_zero();
#pragma unroll 2
    for (int r = 0; r < RT / 2; ++r) {
      bf16x8 fa, fb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = 32 * r + 8 * q + e;
        const size_t off = (size_t)min(m, B - 1) * K + kt * 16 + li;
        float v = g.z[off];
        if (g.m0) v *= g.m0[off] ? g.scale : 0.f;
        fa[e] = f2bf(v);                                // (rows past B meet dy = 0)
        fb[e] = dyS[m * 16 + li];
      }
      acc = fc_mfma(fa, fb, acc);
    }
    *(f32x4*)(g.dw1 + (size_t)(n0 + li) * K + kt * 16 + 4 * q) = acc;
  }
}

constexpr int DZ_NW = 8;
constexpr int DZ_BK = 32;               // columns of K per block
constexpr int DZ_LD = 36;               // bf16 per staged W1 row: 72 bytes
constexpr int dz_rg(int RT) { return RT >= 16 ? 4 : (RT >= 4 ? 2 : 1); }
constexpr int dz_max(int a, int b) { return a > b ? a : b; }

template <int RT>
__global__ __launch_bounds__(DZ_NW * 64) void fc_dz_kernel(FcHeadBwdArgs g) {
  constexpr int RG = dz_rg(RT), NS = DZ_NW / RG, TPW = RT / RG;
  static_assert(RT % RG == 0, "row tiles divide over the row groups");
  constexpr int TILE_BYTES = DZ_NW * 32 * DZ_LD * 2;
  constexpr int PART_BYTES = (NS - 1) * RG * TPW * 2 * 64 * 16;
  // the staged W1 tiles and, after the loop, the splits' accumulators
  __shared__ __attribute__((aligned(16))) char smem[dz_max(TILE_BYTES, PART_BYTES)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int rg = w % RG, ns = w / RG;
  const int B = g.B, K = g.K, N = g.N;
  const int k0 = blockIdx.x * DZ_BK;
  bf16* tile = (bf16*)smem + w * 32 * DZ_LD;
  const int lr = lane >> 3, lc = 4 * (lane & 7);        // loader: row (+ 8 a pass), 4 columns

  f32x4 acc[TPW][2];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t][0] = acc[t][1] = fc_zero();

  const int nchunks = (N + 31) / 32, steps = (nchunks + NS - 1) / NS;
  for (int s = 0; s < steps; ++s) {
    const int nbase = (ns + NS * s) * 32;               // may lie past N: zeros
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int n = nbase + lr + 8 * p;
      f32x4 v = *(const f32x4*)(g.w1 + (size_t)min(n, N - 1) * K + k0 + lc);
      if (n >= N) v = fc_zero();
      *(bf16x4*)(tile + (lr + 8 * p) * DZ_LD + lc) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    }
    __syncthreads();
    bf16x8 fa[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 8; ++e) fa[h][e] = tile[(8 * q + e) * DZ_LD + 16 * h + li];
    const int col = nbase + 8 * q;
    const bool ok = col < N;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int m = min(16 * (rg * TPW + t) + li, B - 1);
      const bf16x8 fd = ok ? *(const bf16x8*)(g.dy + (size_t)m * N + col) : fc_zero8();
      acc[t][0] = fc_mfma(fa[0], fd, acc[t][0]);
      acc[t][1] = fc_mfma(fa[1], fd, acc[t][1]);
    }
    __syncthreads();
  }

  f32x4* part = (f32x4*)smem;
  if (ns > 0) {
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        part[((((ns - 1) * RG + rg) * TPW + t) * 2 + h) * 64 + lane] = acc[t][h];
  }
  __syncthreads();
  if (ns > 0) return;
  for (int p = 0; p < NS - 1; ++p) {
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[t][h] += part[(((p * RG + rg) * TPW + t) * 2 + h) * 64 + lane];
  }
  // lane holds dz[16 i + li][k0 + 16 h + 4 q .. + 3]
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int m = 16 * (rg * TPW + t) + li;
    if (m >= B) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t off = (size_t)m * K + k0 + 16 * h + 4 * q;
      *(f32x4*)(g.dz + off) = acc[t][h] * fc_keep4(g.m0, off, g.scale);
    }
  }
}

void check_geom(const char* what, int B, int K, int N, int C) {
  const std::string s(what);
  if (B < 1 || B > FC_HEAD_MAX_B)
    throw std::invalid_argument(s + ": B must be in [1, " + std::to_string(FC_HEAD_MAX_B) + "]");
  if (N < 16 || N % 16 != 0) throw std::invalid_argument(s + ": N must be a positive multiple of 16");
  if (K < 32 || K % 32 != 0) throw std::invalid_argument(s + ": K must be a positive multiple of 32");
  if (C < 1 || C > FC_HEAD_MAX_C)
    throw std::invalid_argument(s + ": classes must be in [1, " + std::to_string(FC_HEAD_MAX_C) + "]");
  if ((double)N * K >= 2147483648.0)
    throw std::invalid_argument(s + ": W1 has 2^31 elements or more");
}

int row_tiles(int B) { return B <= 32 ? 2 : (B <= 64 ? 4 : (B <= 128 ? 8 : 20)); }

}  // namespace

void fc_head_fwd_launch(const FcHeadFwdArgs& a, hipStream_t st) {
  check_geom("fc_head_fwd", a.B, a.K, a.N, a.C);
  if (!a.z || !a.w1 || !a.b1 || !a.gamma || !a.beta || !a.w2 || !a.b2 || !a.mean || !a.rstd ||
      !a.a2 || !a.logits)
    throw std::invalid_argument("fc_head_fwd: null operand");
  if (a.train && a.B < 2)
    throw std::invalid_argument("fc_head_fwd: batch statistics need B >= 2");
  if (!a.train && (!a.run_mean || !a.run_var))
    throw std::invalid_argument("fc_head_fwd: the eval form needs the running statistics");
  if ((a.run_mean == nullptr) != (a.run_var == nullptr))
    throw std::invalid_argument("fc_head_fwd: run_mean and run_var come together");
  const dim3 grid(a.N / 16);
  switch (row_tiles(a.B)) {
    case 2: fc_bn_fwd_kernel<2, 8><<<grid, 512, 0, st>>>(a); break;
    case 4: fc_bn_fwd_kernel<4, 8><<<grid, 512, 0, st>>>(a); break;
    case 8: fc_bn_fwd_kernel<8, 4><<<grid, 256, 0, st>>>(a); break;
    default: fc_bn_fwd_kernel<20, 4><<<grid, 256, 0, st>>>(a); break;
  }
  fc_out_kernel<<<dim3((a.C + 15) / 16, (a.B + 15) / 16), OUT_NW * 64, 0, st>>>(a);
  HIP_LAUNCH_CHECK();
}

void fc_head_bwd_launch(const FcHeadBwdArgs& a, hipStream_t st) {
  check_geom("fc_head_bwd", a.B, a.K, a.N, a.C);
  if (!a.dlogits || !a.z || !a.w1 || !a.w2 || !a.gamma || !a.y || !a.mean || !a.rstd || !a.a2 ||
      !a.dy || !a.dz || !a.dw1 || !a.db1 || !a.dgamma || !a.dbeta || !a.dw2 || !a.db2)
    throw std::invalid_argument("fc_head_bwd: null operand");
  const dim3 strips(a.N / 16), cols(a.K / DZ_BK);
  switch (row_tiles(a.B)) {
    case 2:
      fc_bn_bwd_kernel<2><<<strips, BWD_NW * 64, 0, st>>>(a);
      fc_dz_kernel<2><<<cols, DZ_NW * 64, 0, st>>>(a);
      break;
    case 4:
      fc_bn_bwd_kernel<4><<<strips, BWD_NW * 64, 0, st>>>(a);
      fc_dz_kernel<4><<<cols, DZ_NW * 64, 0, st>>>(a);
      break;
    case 8:
      fc_bn_bwd_kernel<8><<<strips, BWD_NW * 64, 0, st>>>(a);
      fc_dz_kernel<8><<<cols, DZ_NW * 64, 0, st>>>(a);
      break;
    default:
      fc_bn_bwd_kernel<20><<<strips, BWD_NW * 64, 0, st>>>(a);
      fc_dz_kernel<20><<<cols, DZ_NW * 64, 0, st>>>(a);
      break;
  }
  HIP_LAUNCH_CHECK();
}
