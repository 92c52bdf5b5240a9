// Time-batched GEMMs of the bidirectional LSTM layer: the input projection, the
// input gradient and the weight / bias gradients around the recurrence of lstm.hip, reading and
// writing the layouts its step kernels use, so nothing is permuted, biased, sliced or widened in
// a pass of its own.
//
//   lstm_proj_kernel<PJ_FWD>  pre[t][d][b][j] = sum_k xb[(t,b)][k] * w_ih[(d,j)][k] + b[d][j]
//   lstm_proj_kernel<PJ_DX>   dx[(t,b)][c]    = sum_d sum_j dG[t][d][b][j] * w_ihT[d][c][j]
//   lstm_wgrad_kernel         dW_ih[d][n][c]  = sum_(t,b) dG[t][d][b][n] * xb[t][b][c]
//                             dW_hh[d][n][c]  = sum_(t,b) dG[t][d][b][n] * h_prev(t, b, c)
//                             db[d][n]        = sum_(t,b) dG[t][d][b][n]
//
// ---- lstm_proj_kernel: OUT[m][n] = sum_k A[m][k] * W[n][k], both operands K-contiguous bf16.
// A 256-thread block (four waves, 2 x 2) owns a 128 (m) x 128 (n) output tile and walks K in
// 32-deep steps; a wave owns 64 x 64 of it as 4 x 4 v_mfma_f32_16x16x32_bf16 accumulators (64
// VGPRs).  The weights are the MFMA "A" input and the rows (t, b) the "B" input, so a lane's
// accumulator is 4 CONSECUTIVE n of one row m: every pre store is one contiguous 16 bytes at
// pre[t][d][b][j .. j+3] with the bias added in registers, and a dx store is 16 bytes where F
// is a multiple of 4 (four dwords where it is not: rows of 101 floats are 4-byte aligned).
//   * Both operand tiles of a step (128 rows x 64 bytes each) go HBM -> registers by 16-byte
//     buffer loads (two per operand per thread) -> LDS, and every wave reads its fragments from
//     the shared tile: a fragment is fetched from HBM once per block, not once per wave.
//   * LDS rows are one K-step (64 bytes); chunk c of row r lives at chunk c ^ ((r >> 1) & 3)
//     (pgemm.hip's permutation: conflict-free ds_read_b128 fragment reads for the four 16-lane
//     groups); LDS is double-buffered and TWO steps are in flight in registers, so the loads of
//     step s + 2 are issued before the MFMAs of step s and stay in flight across the barrier
//     that publishes step s + 1.  The loop has whole trips only and the last one or two steps
//     are straight-line code behind it (wgrad_body.h's exit-free form: hipcc keeps its counted
//     vmcnt waits).
//   * Edges cost no branch: a row past M, a weight row past N and a 16-byte chunk past the K
//     tail get a byte offset beyond the buffer resource's range, which loads zeros; a store to
//     such an offset is dropped.  K is walked in chunks of 8, so the operands' rows are padded to
//     ld = K rounded up to 8 with ZERO columns (the caller builds them so).
//   * DX reads dG in place: K = 2 * 4H runs over the two directions' segments of row (t, b), at
//     ((t * 2 + d) * B + b) * 4H, against w_ihT[d]; a 32-deep step never straddles the segments
//     (4H % 128 == 0), the segment is a wave-uniform add, and both directions land in the same
//     accumulators.
//   Tile and grid: at the preset shape (M = 161 * 320 = 51 520, N = 8H = 4096, K = 101 or 1024)
//   the kernel is MFMA-bound at K = 1024 (432 GFLOP against a 844 MB store) and store-bound at
//   K = 101; 128 x 128 x 32 gives 16 MFMAs per 8 fragment reads per wave and step, 32 KB of LDS
//   and ~130 VGPRs, so two blocks share a CU and one block's barrier hides behind the other's
//   MFMAs.  The grid is one block per tile, n fastest (12 896 blocks: the A panel of an m tile
//   is re-read by its 32 n tiles from L2, the 8 MB of weights stay in L2 / MALL).  At B = 32
//   (M = 5152: 1312 tiles, five per CU) neither the matrix cores nor HBM are saturated -- the
//   launch is ~35 GFLOP and an 84 MB store, a few tens of microseconds -- so the same tile is
//   kept: a smaller one would only raise the tile count, not the rate.
//
// ---- lstm_wgrad_kernel: both operands have the reduction index r = (t, b) as their SLOW
// dimension.  A block owns 128 (n) x 64 (c) of one direction's dW_ih | dW_hh and walks all T * B
// rows in slabs of 64: the slab of dG (64 x 128) and of the column operand (64 x 64) are staged
// in LDS as they lie in memory and the fragments are formed with the hardware transpose
// ds_read_b64_tr_b16, in wgrad_body.h's row permutation (conflict-free, the same relabelling of
// the summation index on both operands).  Column tiles [0, ceil(F / 64)) read xb[r]; the tiles
// after them read out[r -+ B] at the direction's half of the 2H row -- h_prev of (t, b) is the
// other operand's row shifted by one frame, i.e. by B rows -- and a row without that frame
// (t = 0 forward, t = T-1 reverse) is an out-of-range offset, so it adds zeros: T = 1 writes an
// all-zero dW_hh.  Blocks of column tile 0 also multiply their dG fragments with a fragment of
// bf16 ones (four more MFMAs per 32 rows in two of the four waves), which is db: one read of
// dG, no reduction launch, no fp32 copy.  Two slabs are in flight in registers, as above.
//   No split of the T * B reduction: at H = 512 a layer has 2 x 16 x (2 + 8) = 320 tiles
//   (F = 101) or 2 x 16 x (16 + 8) = 768 (F = 1024) for 256 CUs with two blocks resident per
//   CU, so every CU is busy without one; each output element then has exactly one writer that
//   sums in a fixed order -- no atomics, no workspace, two runs are bit-equal.
//
// Neither kernel takes lengths: dG, out and xb are exact zeros at padded frames.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int PJ_FWD = 0, PJ_DX = 1;
constexpr int PJ_BM = 128, PJ_BN = 128;        // output rows (t, b) / columns per tile
constexpr int PJ_NT = 256;
constexpr int PJ_STAGE = (PJ_BM + PJ_BN) * 64;  // bytes of one K-step in LDS
constexpr unsigned PJ_OOB = 0xFFFFFF00u;        // byte offset past every tensor: zeros / dropped

MA_DEV __amdgpu_buffer_rsrc_t pj_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}
MA_DEV u32x4 pj_load16(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

template <int MODE>
__global__ __launch_bounds__(PJ_NT, 2) void lstm_proj_kernel(LstmProjArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * PJ_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int B = g.B, H4 = 4 * g.H, F = g.F;
  const int M = g.T * B;
  const int N = MODE == PJ_FWD ? 2 * H4 : F;
  const int KS = MODE == PJ_FWD ? (F + 31) / 32 : 2 * H4 / 32;     // K-steps
  const int K8 = MODE == PJ_FWD ? (F + 7) / 8 : 2 * H4 / 8;        // 16-byte chunks per row
  const int ntn = (N + PJ_BN - 1) / PJ_BN;
  const int mt = blockIdx.x / ntn, nt = blockIdx.x - mt * ntn;
  const int m0 = mt * PJ_BM, n0 = nt * PJ_BN;

  // FWD: A = xb [M][ld], W = w_ih [8H][ld].  DX: A = dG [T][2][B][4H], W = w_ihT [2][F][4H].
  const unsigned a_bytes = MODE == PJ_FWD ? (unsigned)M * g.ld * 2u : (unsigned)M * 2u * H4 * 2u;
  const unsigned w_bytes = MODE == PJ_FWD ? 2u * H4 * g.ld * 2u : 2u * F * H4 * 2u;
  const unsigned o_bytes = MODE == PJ_FWD ? (unsigned)M * 2u * H4 * 4u : (unsigned)M * F * 4u;
  const auto rs_a = pj_rsrc(g.a, a_bytes);
  const auto rs_w = pj_rsrc(g.w, w_bytes);
  const auto rs_o = pj_rsrc(g.out, o_bytes);

  // loader roles: row tid >> 2 (and + 64), logical chunk tid & 3 of the 64-byte K-step
  const int prow = tid >> 2, lc = tid & 3;
  const int sts = prow * 64 + 16 * (lc ^ ((prow >> 1) & 3));          // (row + 64: same swizzle)
  unsigned aoff[2], woff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + prow + 64 * i, n = n0 + prow + 64 * i;
    if constexpr (MODE == PJ_FWD) {
      aoff[i] = m < M ? ((unsigned)m * g.ld + lc * 8) * 2u : PJ_OOB;
      woff[i] = n < N ? ((unsigned)n * g.ld + lc * 8) * 2u : PJ_OOB;
    } else {
      const int t = m / B, b = m - t * B;
      aoff[i] = m < M ? (((unsigned)t * 2u * B + b) * H4 + lc * 8) * 2u : PJ_OOB;
      woff[i] = n < N ? ((unsigned)n * H4 + lc * 8) * 2u : PJ_OOB;
    }
  }
  // a step past KS or a chunk past the K tail loads zeros, so every trip issues the same loads
  auto load_step = [&](int ks, u32x4 (&ra)[2], u32x4 (&rw)[2]) {
    const bool ok = ks < KS && ks * 4 + lc < K8;
    unsigned ka, kw;
    if constexpr (MODE == PJ_FWD) {
      ka = kw = (unsigned)ks * 64u;
    } else {
      const int k = ks * 32, d = k >= H4 ? 1 : 0;          // wave-uniform
      const unsigned kk = (unsigned)(k - d * H4);
      ka = ((unsigned)d * B * H4 + kk) * 2u;
      kw = ((unsigned)d * F * H4 + kk) * 2u;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = pj_load16(rs_a, ok && aoff[i] != PJ_OOB ? aoff[i] + ka : PJ_OOB);
      rw[i] = pj_load16(rs_w, ok && woff[i] != PJ_OOB ? woff[i] + kw : PJ_OOB);
    }
  };
  auto store_step = [&](int buf, const u32x4 (&ra)[2], const u32x4 (&rw)[2]) {
    char* sa = smem + buf * PJ_STAGE;
    char* sw = sa + PJ_BM * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(u32x4*)(sa + sts + i * 64 * 64) = ra[i];
      *(u32x4*)(sw + sts + i * 64 * 64) = rw[i];
    }
  };

  f32x4 acc[4][4];                                       // [m subtile][n subtile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read: row lane & 15 of a 16-row subtile, logical chunk lane >> 4
  const int fl = (lane & 15) * 64 + 16 * ((lane >> 4) ^ ((lane >> 1) & 3));
  auto mma = [&](int buf) {
    const char* sa = smem + buf * PJ_STAGE + (wm * 64) * 64 + fl;
    const char* sw = smem + buf * PJ_STAGE + PJ_BM * 64 + (wn * 64) * 64 + fl;
    bf16x8 fa[4], fw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa[i] = *(const bf16x8*)(sa + i * 16 * 64);
      fw[i] = *(const bf16x8*)(sw + i * 16 * 64);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j], fa[i], acc[i][j], 0, 0, 0);
  };

  {
    u32x4 ra0[2], rw0[2], ra1[2], rw1[2];
    load_step(0, ra0, rw0);
    store_step(0, ra0, rw0);
    load_step(1, ra1, rw1);              // past KS for a one-step K: zeros, never stored
    __syncthreads();
    int ks = 0;
    for (; ks + 2 < KS; ks += 2) {
      load_step(ks + 2, ra0, rw0);       // LDS 0 holds step ks, ra1 step ks + 1
      mma(0);
      store_step(1, ra1, rw1);
      __syncthreads();
      load_step(ks + 3, ra1, rw1);       // LDS 1 holds step ks + 1, ra0 step ks + 2
      mma(1);
      store_step(0, ra0, rw0);
      __syncthreads();
    }
    mma(0);                              // LDS 0 holds step ks, ra1 step ks + 1 if there is one
    if (ks + 1 < KS) {
      store_step(1, ra1, rw1);
      __syncthreads();
      mma(1);
    }
  }

  // epilogue: lane holds n = nb + 16 j + 0 .. 3 of row m0 + 64 wm + 16 i + (lane & 15)
  const int nb = n0 + wn * 64 + 4 * (lane >> 4);
  if constexpr (MODE == PJ_FWD) {
    const int d = n0 >= H4 ? 1 : 0;                      // (4H % 128 == 0: a tile has one d)
    f32x4 bias[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bias[j] = *(const f32x4*)(g.bias + nb + 16 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + 16 * i + (lane & 15);
      const int t = m / B, b = m - t * B;
      const unsigned row = (((unsigned)t * 2u + d) * B + b) * H4 + (nb - d * H4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = acc[i][j] + bias[j];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_o,
                                               m < M ? (row + 16 * j) * 4u : PJ_OOB, 0, 0);
      }
    }
  } else {
    const bool vec = (F & 3) == 0;                       // kernel-uniform
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + 16 * i + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = nb + 16 * j;
        const unsigned off = ((unsigned)m * F + c) * 4u;
        if (vec) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rs_o,
                                                 m < M && c < F ? off : PJ_OOB, 0, 0);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = acc[i][j][r];        // (a bit_cast of the element itself reads [0])
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs_o,
                                                  m < M && c + r < F ? off + 4u * r : PJ_OOB, 0, 0);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------ wgrad
constexpr int WG_BM = 128, WG_BN = 64;         // n rows / c columns per tile
constexpr int WG_BKR = 64;                     // reduction rows per slab
constexpr int WG_LDA = WG_BM + 16, WG_LDB = WG_BN + 16;   // bf16 per LDS row (+16: 8 banks a row)
constexpr int WG_STAGE = WG_BKR * (WG_LDA + WG_LDB);      // bf16 elements
constexpr int WG_AR = WG_BKR * (WG_BM / 8) / PJ_NT;       // 16-byte loads per thread and slab
constexpr int WG_BR = WG_BKR * (WG_BN / 8) / PJ_NT;

typedef short pj_short4 __attribute__((ext_vector_type(4)));
MA_DEV bf16x4 pj_tr_read(const bf16* p) {
  pj_short4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pj_short4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}

__global__ __launch_bounds__(PJ_NT, 2) void lstm_wgrad_kernel(LstmWgradArgs g) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * WG_STAGE];
  constexpr int TM = WG_BM / 32, TN = WG_BN / 32;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int B = g.B, H = g.H, H4 = 4 * g.H, F = g.F, d = blockIdx.y;
  const int M = g.T * B;
  const int ctf = (F + WG_BN - 1) / WG_BN, cth = (H + WG_BN - 1) / WG_BN;
  const int mt = blockIdx.x / (ctf + cth), ct = blockIdx.x - mt * (ctf + cth);
  const bool isx = ct < ctf;                               // xb columns, else h_prev columns
  const int m0 = mt * WG_BM, c0 = (isx ? ct : ct - ctf) * WG_BN;
  const bool with_db = ct == 0 && wn == 0;                 // wave-uniform
  const int nslab = (M + WG_BKR - 1) / WG_BKR;

  const auto rs_g = pj_rsrc(g.dG, (unsigned)M * 2u * H4 * 2u);
  const auto rs_x = pj_rsrc(g.xb, (unsigned)M * g.ld * 2u);
  const auto rs_h = pj_rsrc(g.out, (unsigned)M * 2u * H * 2u);
  const float rcpB = 1.f / (float)B;

  // dG slab: 16 chunks a row, 16 rows a pass; column slab: 8 chunks a row, 32 rows a pass
  const int ach = tid & 15, arow = tid >> 4;
  const int bch = tid & 7, brow = tid >> 3;
  const int cb = c0 + bch * 8;                             // this thread's first column
  const bool cok = isx ? cb < g.ld : cb < H;               // (ld, H % 8 == 0: a chunk is in or out)
  auto load_slab = [&](int sl, u32x4 (&ra)[WG_AR], u32x4 (&rb)[WG_BR]) {
    const bool live = sl < nslab;
#pragma unroll
    for (int i = 0; i < WG_AR; ++i) {
      const int r = sl * WG_BKR + arow + 16 * i;
      const int t = udiv24(r, B, rcpB);                    // dG row of (t, b): r + (t + d) B
      const unsigned off = (((unsigned)r + (unsigned)(t + d) * B) * H4 + m0 + ach * 8) * 2u;
      ra[i] = pj_load16(rs_g, live && r < M ? off : PJ_OOB);
    }
#pragma unroll
    for (int i = 0; i < WG_BR; ++i) {
      const int r = sl * WG_BKR + brow + 32 * i;
      unsigned off;
      bool ok = live && cok;
      if (isx) {
        ok = ok && r < M;
        off = ((unsigned)r * g.ld + cb) * 2u;
      } else {
        // h_prev(t, b): out[t - 1][b][c] (d = 0), out[t + 1][b][H + c] (d = 1): row r -+ B
        const int rh = d ? r + B : r - B;
        ok = ok && rh >= 0 && rh < M;
        off = ((unsigned)rh * 2u * H + d * H + cb) * 2u;
      }
      rb[i] = pj_load16(isx ? rs_x : rs_h, ok ? off : PJ_OOB);
    }
  };
  auto store_slab = [&](int buf, const u32x4 (&ra)[WG_AR], const u32x4 (&rb)[WG_BR]) {
    bf16* a = smem + buf * WG_STAGE;
    bf16* b = a + WG_BKR * WG_LDA;
#pragma unroll
    for (int i = 0; i < WG_AR; ++i) *(u32x4*)(a + (arow + 16 * i) * WG_LDA + ach * 8) = ra[i];
#pragma unroll
    for (int i = 0; i < WG_BR; ++i) *(u32x4*)(b + (brow + 32 * i) * WG_LDB + bch * 8) = rb[i];
  };

  f32x4 acc[TM][TN], accb[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bf16 one = f2bf(1.f);
  const bf16x8 ones = {one, one, one, one, one, one, one, one};

  const int g4 = lane >> 4, li = lane & 15;
  const int tq = li >> 2, tp = li & 3;
  auto mma = [&](int buf) {
    const bf16* a = smem + buf * WG_STAGE;
    const bf16* b = a + WG_BKR * WG_LDA;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = kk * 32 + 16 * h + 4 * g4 + tq;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          const bf16x4 v = pj_tr_read(a + row * WG_LDA + wm * (WG_BM / 2) + tm * 16 + 4 * tp);
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[tm][4 * h + e] = v[e];
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          const bf16x4 v = pj_tr_read(b + row * WG_LDB + wn * (WG_BN / 2) + tn * 16 + 4 * tp);
#pragma unroll
          for (int e = 0; e < 4; ++e) fb[tn][4 * h + e] = v[e];
        }
      }
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[tm], fb[tn], acc[tm][tn], 0, 0, 0);
      if (with_db) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          accb[tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[tm], ones, accb[tm], 0, 0, 0);
      }
    }
  };

  {
    u32x4 ra0[WG_AR], rb0[WG_BR], ra1[WG_AR], rb1[WG_BR];
    load_slab(0, ra0, rb0);
    store_slab(0, ra0, rb0);
    load_slab(1, ra1, rb1);              // past nslab for a one-slab range: zeros, never stored
    __syncthreads();
    int sl = 0;
    for (; sl + 2 < nslab; sl += 2) {
      load_slab(sl + 2, ra0, rb0);
      mma(0);
      store_slab(1, ra1, rb1);
      __syncthreads();
      load_slab(sl + 3, ra1, rb1);
      mma(1);
      store_slab(0, ra0, rb0);
      __syncthreads();
    }
    mma(0);
    if (sl + 1 < nslab) {
      store_slab(1, ra1, rb1);
      __syncthreads();
      mma(1);
    }
  }

  // lane holds rows n = .. + 4 g4 + 0 .. 3 of column c = .. + li
  const int C = isx ? F : H;
  float* dw = isx ? g.dw_ih + (size_t)d * H4 * F : g.dw_hh + (size_t)d * H4 * H;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int c = c0 + wn * (WG_BN / 2) + tn * 16 + li;
    if (c >= C) continue;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = m0 + wm * (WG_BM / 2) + tm * 16 + g4 * 4 + j;   // (4H % 128 == 0: n < 4H)
        dw[(size_t)n * C + c] = acc[tm][tn][j];
      }
  }
  if (with_db && li == 0) {              // every column of accb is the row sum; column 0 stores
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
      *(f32x4*)(g.db + (size_t)d * H4 + m0 + wm * (WG_BM / 2) + tm * 16 + g4 * 4) = accb[tm];
  }
}

// every tensor is addressed with 32-bit byte offsets through a buffer resource, and PJ_OOB has to
// lie past all of them
void check_bytes(const char* what, const char* name, double bytes) {
  if (bytes >= (double)PJ_OOB)
    throw std::invalid_argument(std::string(what) + ": " + name + " is 2^32 bytes or more");
}

void check_geom(const char* what, int T, int B, int F, int H, int ld) {
  if (H < 32 || H % 32 != 0)
    throw std::invalid_argument(std::string(what) + ": H must be a positive multiple of 32");
  if (T < 1 || B < 1 || F < 1)
    throw std::invalid_argument(std::string(what) + ": T, B and F must be >= 1");
  if (ld % 8 != 0 || ld < F || ld >= F + 8)
    throw std::invalid_argument(std::string(what) + ": ld must be F rounded up to a multiple of 8");
  const double M = (double)T * B;
  check_bytes(what, "pre / dG", M * 8.0 * H * 4.0);
  check_bytes(what, "xb", M * ld * 2.0);
  check_bytes(what, "dx", M * F * 4.0);
  check_bytes(what, "w_ih", 8.0 * H * ld * 2.0);
}

}  // namespace

void lstm_proj_launch(const LstmProjArgs& a, hipStream_t st) {
  const char* what = a.dx ? "lstm_proj_dx" : "lstm_proj_fwd";
  check_geom(what, a.T, a.B, a.F, a.H, a.ld);
  if (!a.a || !a.w || !a.out || (!a.dx && !a.bias))
    throw std::invalid_argument(std::string(what) + ": null operand");
  const long long M = (long long)a.T * a.B;
  const int N = a.dx ? a.F : 8 * a.H;
  const long long tiles = ((M + PJ_BM - 1) / PJ_BM) * ((N + PJ_BN - 1) / PJ_BN);
  if (tiles > 0x7fffffffLL) throw std::invalid_argument(std::string(what) + ": too many tiles");
  if (a.dx) lstm_proj_kernel<PJ_DX><<<dim3((unsigned)tiles), PJ_NT, 0, st>>>(a);
  else lstm_proj_kernel<PJ_FWD><<<dim3((unsigned)tiles), PJ_NT, 0, st>>>(a);
  HIP_LAUNCH_CHECK();
}

void lstm_wgrad_launch(const LstmWgradArgs& a, hipStream_t st) {
  check_geom("lstm_proj_wgrad", a.T, a.B, a.F, a.H, a.ld);
  if (!a.dG || !a.xb || !a.out || !a.dw_ih || !a.dw_hh || !a.db)
    throw std::invalid_argument("lstm_proj_wgrad: null operand");
  const int ct = (a.F + WG_BN - 1) / WG_BN + (a.H + WG_BN - 1) / WG_BN;
  lstm_wgrad_kernel<<<dim3((unsigned)(4 * a.H / WG_BM * ct), 2), PJ_NT, 0, st>>>(a);
  HIP_LAUNCH_CHECK();
}
