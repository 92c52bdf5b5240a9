// Shared epilogue of the MFMA convolution kernels (igemm.hip, hconv.hip).
//
// The accumulator layout both main loops produce (swapped-operand 16x16x32 MFMA: lane l holds
// output pixel l&15 and four consecutive channels), the fused epilogue (bias, bf16 round,
// ghost-BN statistics, BN-backward sums, coalesced row stores) and the in-launch split-K
// reduction by the last-arriving slice.  Included into each kernel TU; everything is in an
// anonymous namespace.
#pragma once
#include "bn_math.h"
#include "igemm.h"

namespace {

constexpr int BK = 64;          // k elements per stage (8 chunks of 8)
constexpr int NT = 256;         // threads

#ifdef MERCURY_STAMPS
// Diagnostic build only (-DMERCURY_STAMPS): per-block s_memtime at the phase boundaries of the
// register-staged body -- entry, first stage staged, main loop done, epilogue done -- written
// by thread 0 into a buffer no other code reads (bench/stamp_conv.py).
__device__ unsigned long long g_stamps[8192][12];   // [8..10]: epilogue sub-phases
#define MA_STAMP(i)                                                                         \
  do {                                                                                      \
    if (threadIdx.x == 0) {                                                                 \
      const int b_ = blockIdx.x + blockIdx.y * gridDim.x;                                   \
      if (b_ < 8192) g_stamps[b_][i] = __builtin_amdgcn_s_memtime();                       \
    }                                                                                       \
  } while (0)
// per-phase cycle sums over the main loop (thread 0): [4] load issue, [5] MFMA phase,
// [6] stage store (incl. the wait for its loads), [7] barrier
#define MA_LAP(slot, t)                                                                     \
  do {                                                                                      \
    const unsigned long long n_ = __builtin_amdgcn_s_memtime();                            \
    lap[slot] += n_ - t;                                                                    \
    t = n_;                                                                                 \
  } while (0)
#else
#define MA_STAMP(i) (void)0
#define MA_LAP(slot, t) (void)0
#endif

// XCD-aware tile order.  The dispatcher places workgroup b on XCD b % 8 and each XCD has its
// own 4 MB L2, so with tile = blockIdx.x, neighbouring output tiles -- which share the 3x3
// halo rows of their input and, across N tiles, the same input rows entirely -- land on
// different L2s.  Renumber so XCD x runs one contiguous range of tiles (bijective on [0, n)).
MA_DEV int xcd_tile(int b, int n) {
  const int per = n >> 3, rem = n & 7, x = b & 7;
  return x * per + min(x, rem) + (b >> 3);
}

template <int BM, int BN>
struct Smem {
  static constexpr int STAGE = (BM + BN) * BK;              // bf16 elements
  static constexpr int RED_BYTES = 16 * BN * 4 + BM * (BN + 8) * 2;  // stats + staged tile
  static constexpr int bytes(int stages) {
    return stages * STAGE * 2 > RED_BYTES ? stages * STAGE * 2 : RED_BYTES;
  }
};

// DPP sum over the 16 lanes of a row (quad xor1, quad xor2, half-mirror, mirror)
MA_DEV float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}

// ---------------------------------------------------------------- epilogue
// (BN-backward mean / rstd and the activation bounds: bn_math.h, shared with bn.hip so fused and
// standalone reductions agree)

// Waves are laid out WM x WN (WM * WN = 4): 2 x 2 for the LDS-staged loops, 4 x 1 for the
// direct-A loop.  acc[tm][tn][j] =
//   OUT[m0 + wm*(BM/WM) + tm*16 + (lane&15)][n0 + wn*(BN/WN) + tn*16 + 4*(lane>>4) + j]
template <int BM, int BN, int WM>
using AccT = f32x4[BM / (16 * WM)][BN * WM / 64];

// output row of GEMM row ``row`` (identity unless a stride-2 dgrad parity class, EpiParams.rm_*)
MA_DEV int phys_row(const EpiParams& e, int row) {
  if (e.rm_hc == 0) return row;
  const int per = e.rm_hc * e.rm_wc;
  const int n = udiv24(row, per, 1.f / (float)per), rem = row - n * per;
  const int i = udiv24(rem, e.rm_wc, 1.f / (float)e.rm_wc), j = rem - i * e.rm_wc;
  return (n * e.rm_h + 2 * i + e.rm_ph) * e.rm_w + 2 * j + e.rm_pw;
}

// ---------------------------------------------------------------- prefetched row operands
// What the row loop of a dgrad epilogue reads besides the accumulators -- the old dst of an
// accumulating dgrad, the BN-backward operands (bw_out, bw_y, bw_y2) and the BN statistics --
// was final before the launch started and a thread's (row, chunk) pairs are fixed at block
// entry, so igemm_nt_body requests all of it in front of its last MFMA phases and the epilogue
// finds it in registers instead of paying up to five dependent memory round trips behind the
// last MFMA.  Every operand goes through a buffer resource based at the tile's first output
// row: a row >= M or a chunk column >= N takes the offset EPI_OOB (loads zeros, stores
// nothing), an absent operand a resource of zero bytes -- no branch round any load or store,
// so the counted vmcnt waits stay exact.
constexpr unsigned EPI_OOB = 0x80000000u;
constexpr int EPI_RSRC_FLAGS = 0x00020000;    // raw buffer
constexpr int EPI_RANGE = 0x7fffffff;

// K-split launches: every block of a tile requests the operands in front of its tail, though
// only the last arriver uses them.  Measured against requesting them in the block that wins the
// tile's ticket, under its slab reads (-DMERCURY_EPI_PF_WINNER, bench/build_variant.py; same
// box, interleaved, ResNet-18 step): 1.1868 / 1.1848 ms against 1.1939 / 1.1924 / 1.1920, parent
// 1.2158 / 1.2141 / 1.2137 (profiles/r10/dgrad_epi/bench_ab.json) -- the losers' requests mostly
// hit L2 lines the winner then finds there, the winner's own come a ticket round trip later.
#ifdef MERCURY_EPI_PF_WINNER
constexpr bool EPI_PF_ALL = false;
#else
constexpr bool EPI_PF_ALL = true;
#endif

MA_DEV u32x4 epi_load16(__amdgpu_buffer_rsrc_t rs, unsigned byte_off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 0));
}

// EARLY (the 64 x 64 two-stage kernels, igemm_nt_body): both trips of the row loop are requested
// in front of the last MFMA phases, and the tile's statistics as ONE dword per thread (wave w
// loads row w of [sum, sumsq, shortcut sum, shortcut sumsq] x 64 columns), handed round through
// LDS in the epilogue -- as 16-byte chunks per thread they were 32 more registers across the
// tail, a block per CU.  Otherwise the loads go out at the top of the row loop: two trips at a
// time, or one where a second set would cost the 64 x 64 one-stage kernels a block per CU.
template <int BM, int BN, bool EARLY>
struct EpiPf {
  static constexpr bool EARLY_ = EARLY;
  static constexpr int CPR = BN / 8, TRIPS = BM * CPR / NT;
  static constexpr int G = EARLY || TRIPS > 2 ? 2 : 1;   // trips held in registers at a time
  static_assert(NT % CPR == 0 && TRIPS * NT == BM * CPR && TRIPS % G == 0, "row loop shape");
  static_assert(!EARLY || (BN * 4 == NT && TRIPS == 2), "EARLY: 64 x 64 tiles");
  unsigned off[TRIPS];   // byte offset of the thread's chunk in trip t from the tile's first
                         // output row, or EPI_OOB
  u32x4 old[G], ao[G], ay[G], ay2[G];
  unsigned sv;           // EARLY: the thread's statistics dword

  MA_DEV void init(const EpiParams& e, int M, int N, int m0, int n0) {
    const int tid = threadIdx.x, colc = n0 + (tid % CPR) * 8;
    const int pr0 = phys_row(e, m0);
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int row = m0 + tid / CPR + t * (NT / CPR);
      const bool ok = row < M && colc < N;
      const int d = phys_row(e, ok ? row : m0) - pr0;
      off[t] = ok ? (unsigned)(d * e.ldo + colc) * 2u : EPI_OOB;
    }
  }
};

// The tile's resources: out / bw_out / bw_y / bw_y2 from the tile's first output row (32-bit
// offsets inside a tile whatever the tensor's size), a statistics row with its exact range.
// Each is built where it is used (four scalar registers each; all at once spilled some).
MA_DEV __amdgpu_buffer_rsrc_t epi_rsrc(const void* p, bool on, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(on ? p : nullptr), 0, on ? bytes : 0,
                                           EPI_RSRC_FLAGS);
}
MA_DEV size_t epi_base(const EpiParams& e, int m0) { return (size_t)phys_row(e, m0) * e.ldo; }

// request trips [g * G, g * G + G) of the row loop; every thread issues the same 4 * G loads
template <class P>
MA_DEV void epi_load_rows(P& pf, const EpiParams& e, int m0, int g) {
  constexpr int G = P::G;
  const size_t base = epi_base(e, m0);
  const bool bw = e.bw_sums != nullptr, two = bw && e.bw_y2 != nullptr;
  const auto ro = epi_rsrc(e.out + base, e.accumulate != 0, EPI_RANGE);
#pragma unroll
  for (int u = 0; u < G; ++u) pf.old[u] = epi_load16(ro, pf.off[g * G + u]);
  const auto ra = epi_rsrc(e.bw_out + base, bw, EPI_RANGE);
#pragma unroll
  for (int u = 0; u < G; ++u) pf.ao[u] = epi_load16(ra, pf.off[g * G + u]);
  const auto ry = epi_rsrc(e.bw_y + base, bw, EPI_RANGE);
#pragma unroll
  for (int u = 0; u < G; ++u) pf.ay[u] = epi_load16(ry, pf.off[g * G + u]);
  const auto ry2 = epi_rsrc(e.bw_y2 + base, two, EPI_RANGE);
#pragma unroll
  for (int u = 0; u < G; ++u) pf.ay2[u] = epi_load16(ry2, pf.off[g * G + u]);
}

// the prefetch: (EARLY) the thread's statistics dword, then the first G trips
template <class P>
MA_DEV void epi_prefetch(P& pf, const EpiParams& e, int m0, int n0, int N) {
  if constexpr (P::EARLY_) {
    const bool bw = e.bw_sums != nullptr, two = bw && e.bw_y2 != nullptr;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // statistics row
    const float* row = (w < 2 ? e.bw_stats : e.bw_stats2) + (w & 1) * e.ldo;
    const auto rs = epi_rsrc(row, bw && (w < 2 || two), e.ldo * 4);
    const int col = n0 + (threadIdx.x & 63);
    pf.sv = __builtin_amdgcn_raw_buffer_load_b32(rs, col < N ? (unsigned)col * 4u : EPI_OOB, 0, 0);
  }
  epi_load_rows(pf, e, m0, 0);
}

// Sums over the lanes that differ in bit 4 and in bit 5 without the LDS pipe.  The swaps
// exchange whole rows / halves between TWO registers, so each step also packs two partial sums
// into one register: v_permlane16_swap a, b leaves a = [a.r0 b.r0 a.r2 b.r2] and
// b = [a.r1 b.r1 a.r3 b.r3] (rows of 16 lanes), their sum holds a's pair sums in rows 0 / 2 and
// b's in rows 1 / 3; v_permlane32_swap does the same with the halves.  Four registers come out
// as one whose row r holds the total of register r -- the same pairs in the same order as the
// xor-16 / xor-32 butterfly.
MA_DEV float swap16_sum(float a, float b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a),
                                                  __builtin_bit_cast(unsigned, b), false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
}
MA_DEV float swap32_sum(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a),
                                                  __builtin_bit_cast(unsigned, b), false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
}
// v + (lane ^ 8's v): DPP row_ror:8
MA_DEV float ror8_sum(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128,
                                                                0xF, 0xF, false));
}

// Row loop of the dgrad epilogues, fully unrolled, on prefetched operands.  MODE 0: stores
// only; 1: + BN-backward sums; 2: + the shortcut BN's sum.  MODE and ACC are block-uniform and
// resolved outside (epilogue), so the element code has no branch: the activation mask is two
// compares and a select.
template <int BM, int BN, bool EARLY, int MODE, bool ACC>
MA_DEV void epi_rows(EpiPf<BM, BN, EARLY>& pf, const bf16* tile, float* red, const EpiParams& e,
                     int m0, int n0, int N) {
  using P = EpiPf<BM, BN, EARLY>;
  constexpr int CPR = P::CPR, TRIPS = P::TRIPS, G = P::G, LDT = BN + 8;
  const int tid = threadIdx.x, lane = tid & 63, ch = tid % CPR;
  const auto rso = epi_rsrc(e.out + epi_base(e, m0), true, EPI_RANGE);
  float mean[8], rstd[8], mean2[8], rstd2[8], sdz[8], sx[8], sx2[8];
  float alo, ahi;
  bn_act_bounds(e.bw_act, alo, ahi);
  const bool pass = e.bw_act == 0;
  if constexpr (MODE >= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sdz[k] = sx[k] = sx2[k] = 0.f;
    if constexpr (EARLY) {   // the statistics rows the epilogue staged behind the sums
      const float* sl = red + 8 * BN + ch * 8;
      mean_rstd8(sl, BN, e.bw_inv_count, e.bw_eps, mean, rstd);
      if constexpr (MODE == 2)
        mean_rstd8(sl + 2 * BN, BN, e.bw_inv_count, e.bw_eps, mean2, rstd2);
    } else {
      const int colc = n0 + ch * 8, cc = colc < N ? colc : 0;
      mean_rstd8(e.bw_stats + cc, e.ldo, e.bw_inv_count, e.bw_eps, mean, rstd);
      if constexpr (MODE == 2)
        mean_rstd8(e.bw_stats2 + cc, e.ldo, e.bw_inv_count, e.bw_eps, mean2, rstd2);
    }
  }
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int u = t % G;
    if (u == 0 && t > 0) epi_load_rows(pf, e, m0, t / G);
    const int rl = tid / CPR + t * (NT / CPR);
    bf16x8 v = *(const bf16x8*)(tile + rl * LDT + ch * 8);
    if constexpr (ACC) {
      const bf16x8 o = __builtin_bit_cast(bf16x8, pf.old[u]);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = f2bf(bf2f(v[k]) + bf2f(o[k]));
    }
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rso, pf.off[t], 0, 0);
    if constexpr (MODE >= 1) {
      const bool valid = pf.off[t] != EPI_OOB;
      const bf16x8 ao = __builtin_bit_cast(bf16x8, pf.ao[u]);
      const bf16x8 ay = __builtin_bit_cast(bf16x8, pf.ay[u]);
      const bf16x8 ay2 = __builtin_bit_cast(bf16x8, pf.ay2[u]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float ok = bf2f(ao[k]);
        const bool keep = valid & (pass | ((ok > alo) & (ok < ahi)));
        const float dz = keep ? bf2f(v[k]) : 0.f;
        sdz[k] += dz;
        sx[k] += dz * (bf2f(ay[k]) - mean[k]) * rstd[k];
        if constexpr (MODE == 2) sx2[k] += dz * (bf2f(ay2[k]) - mean2[k]) * rstd2[k];
      }
    }
  }
  if constexpr (MODE >= 1) {
    // lanes ch, ch + CPR, ... of a wave share the chunk: sum them pairwise in the butterfly's
    // order (xor 8 by DPP where CPR == 8, then the packed xor 16 / xor 32 steps above), which
    // leaves the total of register 4 q + r in row r of packed register q; then one LDS atomic
    // per (wave, column), then one global atomic per column per block
    constexpr int NV = MODE == 2 ? 24 : 16;
    float vals[NV];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      vals[k] = sdz[k];
      vals[8 + k] = sx[k];
      if constexpr (MODE == 2) vals[16 + k] = sx2[k];
    }
    if constexpr (CPR == 8) {
#pragma unroll
      for (int i = 0; i < NV; ++i) vals[i] = ror8_sum(vals[i]);
    }
    static_assert(CPR == 8 || CPR == 16, "chunks per row");
    const int r = lane >> 4;
    const bool first = CPR == 16 || (lane & 8) == 0;
#pragma unroll
    for (int q = 0; q < NV / 4; ++q) {
      const float s = swap32_sum(swap16_sum(vals[4 * q], vals[4 * q + 1]),
                                 swap16_sum(vals[4 * q + 2], vals[4 * q + 3]));
      const int idx = 4 * q + r;
      if (first) atomicAdd(&red[(idx >> 3) * BN + ch * 8 + (idx & 7)], s);
    }
    __syncthreads();
    // replica (row tile % SUMS_R) of the [SUMS_R][3][ldo] sums (igemm.h)
    float* sums = e.bw_sums + (size_t)((m0 / BM) % SUMS_R) * 3 * e.ldo;
    for (int i = tid; i < BN; i += NT) {
      const int col = n0 + i;
      if (col < N) {
        atomicAdd(sums + col, red[i]);
        atomicAdd(sums + e.ldo + col, red[BN + i]);
        if constexpr (MODE == 2) atomicAdd(sums + 2 * e.ldo + col, red[2 * BN + i]);
      }
    }
  }
}

// BWT: a dgrad instantiation (igemm_nt_body) -- its row loop runs on operands prefetched into
// ``pf``; every other instantiation carries no BN-backward code at all.
template <int BM, int BN, int WM = 2, bool BWT = false, bool EARLY = false>
MA_DEV void epilogue(AccT<BM, BN, WM>& acc, char* smem, const EpiParams& e, int M, int N,
                     int m0, int n0, EpiPf<BM, BN, EARLY>* pf = nullptr) {
  constexpr int WN = 4 / WM, TM = BM / (16 * WM), TN = BN / (16 * WN), LDT = BN + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / WN, wn = w % WN;
  const bool stats = e.stats != nullptr;
  const bool bw = e.bw_sums != nullptr;
  // stats: [WM][4][BN] per-wave-row partials (sum | sumsq | group-2 sum | group-2 sumsq),
  // each slot written by exactly one lane -- no LDS atomics, no zeroing; bw: [3][BN] sums
  float* red = (float*)smem;
  bf16* tile = (bf16*)(smem + 16 * BN * 4);        // [BM][LDT] staged output
  if (bw) {
    for (int i = tid; i < 3 * BN; i += NT) red[i] = 0.f;
  }
  // ghost-BN groups: a tile may straddle ONE group boundary (groups are >= BM rows), e.g. when
  // the per-image pixel count is odd (speech VGG 101x161); rows >= bnd go to group g + 1
  const int g0 = stats ? m0 / e.group_rows : 0;
  const int bnd = stats ? (g0 + 1) * e.group_rows : 0;
  const bool straddle = stats && bnd < m0 + BM && bnd < M;
  float4 bias[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) bias[tn] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e.bias) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int nb = n0 + wn * (BN / WN) + tn * 16 + 4 * (lane >> 4);
      bias[tn] = *(const float4*)(e.bias + (nb < N ? nb : N - 4));
    }
  }
  __syncthreads();
  MA_STAMP(8);
  const int mrow = m0 + wm * (BM / WM) + (lane & 15);
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int nl = wn * (BN / WN) + tn * 16 + 4 * (lane >> 4);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
    float s2[4] = {0.f, 0.f, 0.f, 0.f}, ss2[4] = {0.f, 0.f, 0.f, 0.f};
    const float bb[4] = {bias[tn].x, bias[tn].y, bias[tn].z, bias[tn].w};
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int ml = wm * (BM / WM) + tm * 16 + (lane & 15);
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(acc[tm][tn][j] + bb[j]);
      *(bf16x4*)(tile + ml * LDT + nl) = o;   // one 8-byte LDS write per lane
      const int row = mrow + tm * 16;
      if (stats) {
        if (!straddle) {
          // rows past M masked by a multiply, not an exec-mask branch per fragment
          const float msk = row < M ? 1.f : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float f = bf2f(o[j]) * msk;
            s[j] += f;
            ss[j] += f * f;
          }
        } else if (row < M) {
          if (row < bnd) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float f = bf2f(o[j]);
              s[j] += f;
              ss[j] += f * f;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float f = bf2f(o[j]);
              s2[j] += f;
              ss2[j] += f * f;
            }
          }
        }
      }
    }
    if (stats) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = row16_sum(s[j]);
        ss[j] = row16_sum(ss[j]);
      }
      if (straddle) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s2[j] = row16_sum(s2[j]);
          ss2[j] = row16_sum(ss2[j]);
        }
      }
      if ((lane & 15) == 0) {
        float* r = red + wm * 4 * BN + nl;
        *(float4*)r = make_float4(s[0], s[1], s[2], s[3]);
        *(float4*)(r + BN) = make_float4(ss[0], ss[1], ss[2], ss[3]);
        if (straddle) {
          *(float4*)(r + 2 * BN) = make_float4(s2[0], s2[1], s2[2], s2[3]);
          *(float4*)(r + 3 * BN) = make_float4(ss2[0], ss2[1], ss2[2], ss2[3]);
        }
      }
    }
  }
  if constexpr (BWT && EARLY) {
    // the prefetched statistics dwords -> red[8 BN ..): sum, sumsq, shortcut sum, shortcut sumsq
    if (bw) red[8 * BN + tid] = __builtin_bit_cast(float, pf->sv);
  }
  MA_STAMP(9);
  __syncthreads();
  if (stats) {
    for (int gi = 0; gi < (straddle ? 2 : 1); ++gi) {
      float* dst = MA_SPREAD(e.stats + (size_t)(g0 + gi) * 2 * e.stats_ld);
      for (int i = tid; i < BN; i += NT) {
        const int col = n0 + i;
        if (col < N) {
          float a = 0.f, b = 0.f;
#pragma unroll
          for (int q = 0; q < WM; ++q) {
            a += red[(q * 4 + 2 * gi) * BN + i];
            b += red[(q * 4 + 2 * gi + 1) * BN + i];
          }
          atomicAdd(dst + col, a);
          atomicAdd(dst + e.stats_ld + col, b);
        }
      }
    }
  }
  // coalesced 16-byte row stores from the staged tile.  NT is a multiple of CPR, so every
  // thread keeps ONE 8-column chunk for the whole loop (its BN constants load once).
  MA_STAMP(10);
  if constexpr (BWT) {
    // dgrad: unrolled row loop on the prefetched operands; the block-uniform options select one
    // of six straight-line instances here, outside the element code
    static_assert(WM == 2, "the prefetched row loop serves igemm_nt_body");
    if constexpr (!EARLY) {
      // not requested ahead of the MFMA tail (igemm_nt_body): request here, where the
      // accumulators are dead -- the first two trips and the statistics in one round trip
      pf->init(e, M, N, m0, n0);
      epi_prefetch(*pf, e, m0, n0, N);
    }
    const bool two = bw && e.bw_y2 != nullptr;
    if (!bw) {
      if (e.accumulate) epi_rows<BM, BN, EARLY, 0, true>(*pf, tile, red, e, m0, n0, N);
      else epi_rows<BM, BN, EARLY, 0, false>(*pf, tile, red, e, m0, n0, N);
    } else if (!two) {
      if (e.accumulate) epi_rows<BM, BN, EARLY, 1, true>(*pf, tile, red, e, m0, n0, N);
      else epi_rows<BM, BN, EARLY, 1, false>(*pf, tile, red, e, m0, n0, N);
    } else {
      if (e.accumulate) epi_rows<BM, BN, EARLY, 2, true>(*pf, tile, red, e, m0, n0, N);
      else epi_rows<BM, BN, EARLY, 2, false>(*pf, tile, red, e, m0, n0, N);
    }
    return;
  }
  constexpr int CPR = BN / 8;
  const int ch = tid % CPR;
  const int colc = n0 + ch * 8;
  float mean[8], rstd[8], mean2[8], rstd2[8], sdz[8], sx[8], sx2[8];
  const bool two = bw && e.bw_y2 != nullptr;
  float alo, ahi;
  bn_act_bounds(e.bw_act, alo, ahi);
  const bool pass = e.bw_act == 0;
  if (bw) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sdz[k] = sx[k] = sx2[k] = mean2[k] = 0.f, rstd2[k] = 1.f;
    const int cc = colc < N ? colc : 0;
    mean_rstd8(e.bw_stats + cc, e.ldo, e.bw_inv_count, e.bw_eps, mean, rstd);
    if (two) mean_rstd8(e.bw_stats2 + cc, e.ldo, e.bw_inv_count, e.bw_eps, mean2, rstd2);
  }
  for (int i = tid; i < BM * CPR; i += NT) {
    const int rl = i / CPR;
    const int row = m0 + rl, col = colc;
    if (row >= M || col >= N) continue;
    bf16x8 v = *(const bf16x8*)(tile + rl * LDT + ch * 8);
    const size_t off = (size_t)phys_row(e, row) * e.ldo + col;
    bf16* dst = e.out + off;
    if (e.accumulate) {
      const bf16x8 o = *(const bf16x8*)dst;
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = f2bf(bf2f(v[k]) + bf2f(o[k]));
    }
    *(bf16x8*)dst = v;
    if (bw) {
      const bf16x8 ao = *(const bf16x8*)(e.bw_out + off);
      const bf16x8 ay = *(const bf16x8*)(e.bw_y + off);
      bf16x8 ay2;
      if (two) ay2 = *(const bf16x8*)(e.bw_y2 + off);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float ok = bf2f(ao[k]);
        const float dz = (pass || (ok > alo && ok < ahi)) ? bf2f(v[k]) : 0.f;
        sdz[k] += dz;
        sx[k] += dz * (bf2f(ay[k]) - mean[k]) * rstd[k];
        if (two) sx2[k] += dz * (bf2f(ay2[k]) - mean2[k]) * rstd2[k];
      }
    }
  }
  if (bw) {
    // lanes ch, ch+CPR, ... of a wave share the chunk: butterfly, then one LDS atomic per
    // (wave, column), then one global atomic per column per block
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1) {
        sdz[k] += __shfl_xor(sdz[k], o, 64);
        sx[k] += __shfl_xor(sx[k], o, 64);
        if (two) sx2[k] += __shfl_xor(sx2[k], o, 64);
      }
    }
    if (lane < CPR) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        atomicAdd(&red[ch * 8 + k], sdz[k]);
        atomicAdd(&red[BN + ch * 8 + k], sx[k]);
        if (two) atomicAdd(&red[2 * BN + ch * 8 + k], sx2[k]);
      }
    }
    __syncthreads();
    // replica (row tile % SUMS_R) of the [SUMS_R][3][ldo] sums (igemm.h)
    float* sums = e.bw_sums + (size_t)((m0 / BM) % SUMS_R) * 3 * e.ldo;
    for (int i = tid; i < BN; i += NT) {
      const int col = n0 + i;
      if (col < N) {
        atomicAdd(sums + col, red[i]);
        atomicAdd(sums + e.ldo + col, red[BN + i]);
        if (two) atomicAdd(sums + 2 * e.ldo + col, red[2 * BN + i]);
      }
    }
  }
}

// Split-K: every K-slice block writes its fp32 partial tile (fragment order, 16 B per lane,
// fully coalesced) behind the slab's tile-counter header; the LAST block to arrive on a tile
// sums all slices and runs the epilogue in the same launch (no reducer kernel, no extra launch
// in the step graph).  Hand-off (cdna_hip_programming.md §6 Guideline 16, R1 form): partials are
// stored write-through (buffer store, sc1) and drained by every wave before the workgroup
// barrier, one lane takes a relaxed agent-scope ticket; the last arriver reads the other slices
// with sc1 loads only -- no L2 write-back fence per block, correct for any XCD placement.  The
// counter is reset by the last arriver (slabs are zero-initialised at allocation).
constexpr int SEM_INTS = 1024;   // tile counters at the head of the slab (4 KB)

template <int BM, int BN, int WM = 2, bool BWT = false, bool EARLY = false>
MA_DEV void finish(AccT<BM, BN, WM>& acc, char* smem, const EpiParams& e, int M, int N,
                   int m0, int n0, int bx, int by, int gx, int gy,
                   EpiPf<BM, BN, EARLY>* pf = nullptr) {
  constexpr int TM = BM / (16 * WM), TN = BN * WM / 64;
  if (e.slab) {
    const int ntiles = gx;
    const int splits = gy;
    int* sem = (int*)e.slab;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(e.slab + SEM_INTS), 0, 0x7fffffff,
                                                      0x00020000);
    const int tile_bytes = TM * TN * NT * 16;
    const int mine = (by * ntiles + bx) * tile_bytes + threadIdx.x * 16;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[tm][tn]), rs,
                                               mine + (tm * TN + tn) * NT * 16, 0, 16 /*sc1*/);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains
    int* flag = (int*)smem;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(&sem[bx], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == splits - 1;
      if (last) __hip_atomic_store(&sem[bx], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      flag[0] = last;
    }
    __syncthreads();
    if (!flag[0]) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // keep the sc1 loads below the ticket
    // (EPI_PF_WINNER builds) the epilogue's operands, requested by the one block that will use
    // them, in flight under the slab reads
    if constexpr (BWT && EARLY && !EPI_PF_ALL) epi_prefetch(*pf, e, m0, n0, N);
    for (int sp = 0; sp < splits; ++sp) {
      if (sp == by) continue;
      const int base = (sp * ntiles + bx) * tile_bytes + threadIdx.x * 16;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] += __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, base + (tm * TN + tn) * NT * 16, 0,
                                                           16 /*sc1*/));
    }
    __syncthreads();   // flag read by every wave before the epilogue reuses smem
  }
  epilogue<BM, BN, WM, BWT, EARLY>(acc, smem, e, M, N, m0, n0, pf);
}

}  // namespace
