// Log-mel and MFCC pools from raw clips (WaveRecipe with mel > 0, mercury_amd/data/augment.py):
// pool_wave.hip's front end with a mel filter bank, and optionally a DCT, between the power and
// the store, all three GEMMs on v_mfma_f32_16x16x4_f32 in one launch.
//
// pool_wave_mel : shard [Ns][L] -> shift, gain, noise mix, reflect padding (pool_wave_slot.h) ->
//                 windowed DFT -> p[t][k] = re^2 + im^2 -> mel[t][m] = sum_k p[t][k] fb[k][m] ->
//                 lm = ln(mel + eps) -> [c[t][j] = sum_m lm[t][m] D[m][j]] -> a * . + b -> masks
//                 -> bf16 channel 0 of the NHWC8 pool [P][R][T][8], R = dct ? dct : mel rows.
//
// Why a kernel of its own: in pool_wave_kernel a wave owns 16 bins for all frames, so nothing
// crosses lanes after the DFT.  A mel band sums over bins, that is over waves, so the power goes
// through LDS and the block is re-split for the second GEMM.
//
// Grid (slot, frame chunk), the chunk rule of pool_wave.hip with the panels added to the LDS need.
// LDS, in fp32 words:
//   [0, lds_words)                      the waveform stretch (phase 1's A operand); dead after
//                                       phase 1, so the log-mel panel of phase 3 lies over it
//   [panel_off, + 16 tiles * PP)        power panel [frame][bin], pitch PP = F16 + 4
//   [0, 16 tiles * LP)  (DCT only)      log-mel panel [frame][band], pitch LP = M16 + 4
//   [panel_off, + src_words + 65 * 33)  (SPEED) the resampler's source panel and table
//                                       (pool_wave_slot.h), over the power panel: dead once
//                                       the stretch is staged, before phase 1 writes the power
// Pitch.  An accumulator lane (col = lane % 16, kq = lane / 16) holds frames 4 kq + i, i < 4, of
// column col, so store i of a wave goes to word (r0 + 4 kq + i) * PP + c0 + col: bank
// 4 kq PP + col + const (mod 64).  The next GEMM's A operand of K step k is the word
// (r0 + col) * PP + 4 k + kq: bank col PP + kq + const.  With PP = 4 (mod 16), PP = 4 q, q odd:
// 4 kq PP = 16 q kq runs over {0, 16, 32, 48} and col < 16 fills each quarter; col PP = 4 (q col
// mod 16) runs over the 16 multiples of 4 and kq < 4 fills the gaps.  Both touch 64 distinct
// banks.  F16 and M16 are multiples of 16, so + 4 is the smallest such pitch.
//
// Phase 1 (DFT) is pool_wave_kernel's table-stationary loop: a wave owns a 16-bin tile, holds
// its 2 * NK table fragments in registers and walks the chunk's 16-frame tiles; each lane writes
// re^2 + im^2 of its 4 frames into the power panel.  The padding bins (>= F) are written too:
// their table columns are zero, so they are the exact zeros the mel GEMM's padding rows expect.
// Phase 2 (mel) is [frames x F16] . [F16 x M16]: the waves take (frame tile, band tile) pairs
// round-robin, A from the panel, B from mel_tab in global memory (at most 272 x 128 floats, L2).
// The bank is banded: krange (kernel argument, checked by the launcher) gives each band tile's
// first and last 4-bin K step with a nonzero, and the K loop runs only those; the skipped
// products are exact zeros.  Without DCT the log, the affine, the masks and the 16-byte pixel
// stores follow in registers (4 consecutive frames of one band: 64 contiguous bytes).
// Phase 3 (DCT): ln(mel + eps) goes to the log-mel panel instead -- padding bands as ln(eps),
// which dct_tab's zero rows >= M cancel -- and after a barrier [frames x M16] . [M16 x C16]
// against dct_tab, then affine, masks, store.
// No atomics, fixed K order: launches are bit-equal and capturable.
//
// Delta rows (DELTA = true, WaveRecipe.delta = 1 | 2, half-window N = dwin): rows R + r and
// 2 R + r of the pool hold a * d1[r] and a * d2[r],
//   d1[r][t] = sum_{n <= N} n (v[r][clamp(t + n)] - v[r][clamp(t - n)]) / (2 sum n^2),
// clamp(u) = min(max(u, 0), T - 1), d2 the same operator on d1, v the feature before the affine.
// A difference over +-N frames crosses the lane's 4 frames, the wave's tile and the block's
// chunk, so the features go through LDS once more and the chunk gets a frame halo:
//   a block OWNS output frames [o0, o1), its tiles clipped to T, and computes features for the
//   WINDOW [w0, w1) = [o0 - h, o1 + h) clipped to [0, T), h = delta * N <= 8, in whole 16-frame
//   tiles counted from w0 (no longer a multiple of 16): at most one tile more than it owns.
// wave_stage stages from sample w0 * hop and phases 1 to 3 walk the window's tiles as they are.
// Instead of storing, phase 2 (no DCT) keeps ln(mel + eps) in the log-mel panel and phase 3
// writes the coefficients into a panel of their own over the power panel, dead after phase 2:
//   feature panel [window frames][FP], FP = R16 + 4: at 0 without DCT, at panel_off with it
//   d1 panel (order 2) [o0 - N, o1 + N) clipped, pitch FP: over the other dead panel -- the power
//   panel without DCT, the log-mel panel with it.
// Phase 4, after a barrier: a lane is (row r = 16 rt + lane % 16, frames tb + i, tb = o0 + 16 ft
// + 4 (lane / 16)), the accumulator's mapping, over (owned frame tile, row tile) pairs.  It
// reads panel[(clamp(t +- n) - w0) * FP + r]: bank 4 (lane / 16) FP + lane % 16 + const, the
// store pattern above, conflict-free; in a tile that touches a clip end the clamp breaks the
// 4-frame spacing and two words can share a bank (bench/wave_bench.py banks).  Order 2 first
// fills the d1 panel in the same mapping from its first frame, barriers, and runs the stencil
// again on it.  Then 4 frames of the static row and of each delta row go out through mel_store4
// (64 contiguous bytes per row).  Every output element is the same fixed sequence of fp32
// operations on panel values that do not depend on where the window starts (an MFMA row's
// result does not depend on its row index), so pools built with different chunk counts are
// bit-equal.
//
// Feature-out form (FEAT = true, WaveRecipe.cmvn; always with DELTA = false, also for delta > 0):
// per-utterance CMVN needs statistics over all T frames of a row, and no block of this grid sees
// a whole row.  So phase 2 (no DCT) or phase 3 (DCT) stores the lane's 4 consecutive frames of
// the RAW feature -- ln(mel + eps) or the coefficient: no affine, no mask, no rounding -- as one
// 16-byte fp32 store into the workspace feat[slot][r][Tp], Tp = T rounded up to 4 (mel_store4's
// mapping: 64 contiguous bytes per row and 16-lane group).  Frames >= T of a row's last 4 may
// hold anything; nobody reads them.  pool_cmvn_kernel (pool_cmvn.hip), launched right behind on
// the same stream, normalises, takes the delta rows and writes the pool.  No halo, no window
// DFT computed twice, and the LDS of the DELTA = false kernel.
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"
#include "pool_wave_slot.h"

namespace {

constexpr int PANEL_PAD = 4;     // pitch = width + 4 = 4 (mod 16), see above

// Frames tb..tb+3 of pool row `row`: y = log_a * v + log_b (a delta row, DIFF: y = log_a * v, the
// difference of an affine feature carries no offset), fill where masked (frequency bands by the
// feature row `frow` the pool row derives from), one bf16 rounding into channel 0 of the 16-byte
// pixel, channels 1..7 +0.
template <bool DIFF = false>
MA_DEV void mel_store4(const PoolWaveArgs& a, const WaveSlot& s, int slot, int row, int frow,
                       int tb, const float v[4]) {
  const int T = a.b.W;
  const bf16 fill = f2bf(a.fill), zero = f2bf(0.f);
  const bool rmasked = (frow >= s.f0[0] && frow < s.f0[0] + s.fw[0]) ||
                       (frow >= s.f0[1] && frow < s.f0[1] + s.fw[1]);
  bf16* o = a.b.pool + (((size_t)slot * a.b.H + row) * T + tb) * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int tt = tb + i;
    if (tt >= T) break;
    const bool masked = rmasked || (tt >= s.t0[0] && tt < s.t0[0] + s.tw[0]) ||
                        (tt >= s.t0[1] && tt < s.t0[1] + s.tw[1]);
    bf16x8 px;
    px[0] = masked ? fill : f2bf(DIFF ? a.log_a * v[i] : a.log_a * v[i] + a.log_b);
#pragma unroll
    for (int c = 1; c < 8; ++c) px[c] = zero;
    *(bf16x8*)(o + (size_t)i * 8) = px;
  }
}

// Frames tb..tb+3 (tb a multiple of 4) of raw feature row `row` into the cmvn workspace.
MA_DEV void feat_store4(const PoolWaveArgs& a, int slot, int row, int tb, const float v[4]) {
  if (tb >= a.b.W) return;
  const f32x4 q = {v[0], v[1], v[2], v[3]};
  *(f32x4*)(a.feat + ((size_t)slot * a.rows + row) * a.feat_tp + tb) = q;
}

// One 16 x 16 output tile of [rows x K] . [K x N]: A rows r0.. of an LDS panel of pitch lda, B
// columns n0.. of a global table of pitch ldb, K steps k0..k1 (inclusive) of 4.
MA_DEV f32x4 panel_gemm(const float* panel, int lda, int r0, const float* tab, int ldb, int n0,
                        int k0, int k1, int col, int kq) {
  const float* ap = panel + (r0 + col) * lda + kq;
  const float* bp = tab + (size_t)kq * ldb + n0 + col;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = k0; k <= k1; ++k)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * k], bp[(size_t)(4 * k) * ldb], acc, 0, 0, 0);
  return acc;
}

// d[i] = dinv * sum_{n <= N} n (x[clamp(t0 + i + n)] - x[clamp(t0 + i - n)]), i < 4, down one
// column `x` of a panel of pitch `pitch` whose row 0 is frame p0; frames >= tend give 0 and read
// nothing.  One fused multiply-add per n in a fixed order, then one multiply.
MA_DEV void delta4(const float* x, int pitch, int p0, int t0, int tend, int T, int N, float dinv,
                   float d[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + i;
    float acc = 0.f;
    if (t < tend)
      for (int n = 1; n <= N; ++n)
        acc = fmaf((float)n, x[(min(t + n, T - 1) - p0) * pitch] - x[(max(t - n, 0) - p0) * pitch],
                   acc);
    d[i] = acc * dinv;
  }
}

template <typename S, int NK, bool DCT, bool DELTA, bool SPEED = false, bool FEAT = false>
__global__ __launch_bounds__(NK > 64 ? 256 : 448) void pool_wave_mel_kernel(PoolWaveArgs a) {
  extern __shared__ float lds[];
  const PoolBuildArgs& b = a.b;
  const int slot = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int T = b.W;
  if (b.zero && blockIdx.y == 0)
    for (int j = slot * nthr + tid; j < b.nzero; j += gridDim.x * nthr) b.zero[j] = 0.f;
  int64_t gb;
  int t;
  const uint32_t src = pool_src(b, slot, gb, t);
  const WaveSlot s = wave_slot_draws<DELTA || FEAT, SPEED>(a, gb, t);
  if (tid == 0 && blockIdx.y == 0) wave_slot_header<SPEED>(a, slot, src, s);
  const int ntiles = (T + 15) >> 4;
  const int tile0 = blockIdx.y * a.tiles_per_chunk;
  const int nown = min(a.tiles_per_chunk, ntiles - tile0);      // owned tiles
  // owned frames [o0, o1), window [w0, w1) in `ntile` tiles from w0 (without DELTA: the same)
  const int o0 = tile0 * 16, o1 = min(o0 + nown * 16, T);
  const int halo = DELTA ? a.delta * a.dwin : 0;
  const int w0 = DELTA ? max(o0 - halo, 0) : o0;
  const int ntile = DELTA ? (min(o1 + halo, T) - w0 + 15) >> 4 : nown;
  wave_stage_slot<S, SPEED>(a, s, a.rev_on ? (uint32_t)slot : src, w0 * a.hop, lds, tid, nthr);
  __syncthreads();

  // ---- phase 1: DFT, table stationary, frames streaming; power into the panel
  const int lane = tid & 63, nw = nthr >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kq = lane >> 4;
  const int ldt = 2 * a.F16, nbt = a.F16 >> 4, PP = a.panel_pitch;
  float* panel = lds + a.panel_off;
  for (int bt = wave; bt < nbt; bt += nw) {
    float bc[NK], bs[NK];
    const float* tp = a.tab + (size_t)kq * ldt + bt * 16 + col;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      bc[k] = tp[(size_t)(4 * k) * ldt];
      bs[k] = tp[(size_t)(4 * k) * ldt + a.F16];
    }
    for (int ft = 0; ft < ntile; ++ft) {
      const float* fp = lds + (ft * 16 + col) * a.hop + kq;
      f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float av = fp[4 * k];
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bc[k], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bs[k], im, 0, 0, 0);
      }
      float* pw = panel + (ft * 16 + kq * 4) * PP + bt * 16 + col;
#pragma unroll
      for (int i = 0; i < 4; ++i) pw[i * PP] = re[i] * re[i] + im[i] * im[i];
    }
  }
  __syncthreads();

  // ---- phase 2: mel bands, (frame tile, band tile) pairs round-robin over the waves
  const int nmt = a.M16 >> 4, LP = a.lm_pitch;
  for (int p = wave; p < nmt * ntile; p += nw) {
    const int ft = p / nmt, mt = p - ft * nmt;
    const int k0 = max(a.krange[2 * mt], 0), k1 = min(a.krange[2 * mt + 1], (a.F16 >> 2) - 1);
    const f32x4 acc = panel_gemm(panel, PP, ft * 16, a.mel_tab, a.M16, mt * 16, k0, k1, col, kq);
    const int band = mt * 16 + col;
    float lm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) lm[i] = __logf(acc[i] + a.eps);
    if (DCT || DELTA) {
      float* lp = lds + (ft * 16 + kq * 4) * LP + band;
#pragma unroll
      for (int i = 0; i < 4; ++i) lp[i * LP] = lm[i];
    } else if (band < a.mel) {
      if (FEAT)
        feat_store4(a, slot, band, (tile0 + ft) * 16 + kq * 4, lm);
      else
        mel_store4(a, s, slot, band, band, (tile0 + ft) * 16 + kq * 4, lm);
    }
  }
  if constexpr (!DCT && !DELTA) return;
  __syncthreads();

  // ---- phase 3: cepstral coefficients
  if constexpr (DCT) {
    const int nct = a.C16 >> 4;
    for (int p = wave; p < nct * ntile; p += nw) {
      const int ft = p / nct, ct = p - ft * nct;
      const f32x4 acc = panel_gemm(lds, LP, ft * 16, a.dct_tab, a.C16, ct * 16, 0,
                                   (a.M16 >> 2) - 1, col, kq);
      const int coef = ct * 16 + col;
      const float c[4] = {acc[0], acc[1], acc[2], acc[3]};
      if (DELTA) {            // the coefficient panel, over the power panel (padding columns: 0)
        float* cp = panel + (ft * 16 + kq * 4) * a.feat_pitch + coef;
#pragma unroll
        for (int i = 0; i < 4; ++i) cp[i * a.feat_pitch] = c[i];
      } else if (coef < a.dct) {
        if (FEAT)
          feat_store4(a, slot, coef, (tile0 + ft) * 16 + kq * 4, c);
        else
          mel_store4(a, s, slot, coef, coef, (tile0 + ft) * 16 + kq * 4, c);
      }
    }
    if constexpr (!DELTA) return;
    __syncthreads();
  }

  // ---- phase 4: time differences of the feature panel, static and delta rows out
  if constexpr (DELTA) {
    const int R = a.rows, FP = a.feat_pitch, N = a.dwin;
    const int nrt = (R + 15) >> 4;
    const float* feat = lds + a.feat_off;
    float* d1p = lds + a.d1_off;
    const int e0 = max(o0 - N, 0), e1 = min(o1 + N, T);         // frames of the d1 panel
    if (a.delta == 2) {
      for (int p = wave; p < nrt * ((e1 - e0 + 15) >> 4); p += nw) {
        const int ft = p / nrt, r = (p - ft * nrt) * 16 + col;
        const int tb = e0 + ft * 16 + kq * 4;
        if (r >= R) continue;
        float d[4];
        delta4(feat + r, FP, w0, tb, e1, T, N, a.dinv, d);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (tb + i < e1) d1p[(tb + i - e0) * FP + r] = d[i];
      }
      __syncthreads();
    }
    for (int p = wave; p < nrt * nown; p += nw) {
      const int ft = p / nrt, r = (p - ft * nrt) * 16 + col;
      const int tb = o0 + ft * 16 + kq * 4;
      if (r >= R || tb >= o1) continue;
      float v[4], d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = feat[(min(tb + i, T - 1) - w0) * FP + r];
      mel_store4(a, s, slot, r, r, tb, v);
      if (a.delta == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = d1p[(min(tb + i, T - 1) - e0) * FP + r];
      } else {
        delta4(feat + r, FP, w0, tb, o1, T, N, a.dinv, d);
      }
      mel_store4<true>(a, s, slot, R + r, r, tb, d);
      if (a.delta == 2) {
        delta4(d1p + r, FP, e0, tb, o1, T, N, a.dinv, d);
        mel_store4<true>(a, s, slot, 2 * R + r, r, tb, d);
      }
    }
  }
}

template <typename S, bool DCT, bool DELTA, bool SPEED, bool FEAT = false>
void launch_nk(const PoolWaveArgs& a, int nk, dim3 grid, int threads, size_t lds, hipStream_t st) {
  const dim3 blk(threads);
#define MEL_LAUNCH(NK) \
  hipLaunchKernelGGL((pool_wave_mel_kernel<S, NK, DCT, DELTA, SPEED, FEAT>), grid, blk, lds, st, a)
  switch (nk) {
    case 16: MEL_LAUNCH(16); break;
    case 32: MEL_LAUNCH(32); break;
    case 50: MEL_LAUNCH(50); break;
    case 64: MEL_LAUNCH(64); break;
    default: MEL_LAUNCH(128);
  }
#undef MEL_LAUNCH
}

template <typename S, bool SPEED>
void launch_stages(const PoolWaveArgs& a, int nk, dim3 grid, int threads, size_t lds,
                   hipStream_t st) {
  if (a.cmvn)
    a.dct ? launch_nk<S, true, false, SPEED, true>(a, nk, grid, threads, lds, st)
          : launch_nk<S, false, false, SPEED, true>(a, nk, grid, threads, lds, st);
  else if (a.delta)
    a.dct ? launch_nk<S, true, true, SPEED>(a, nk, grid, threads, lds, st)
          : launch_nk<S, false, true, SPEED>(a, nk, grid, threads, lds, st);
  else
    a.dct ? launch_nk<S, true, false, SPEED>(a, nk, grid, threads, lds, st)
          : launch_nk<S, false, false, SPEED>(a, nk, grid, threads, lds, st);
}

template <typename S>
void launch_typed(const PoolWaveArgs& a, int nk, dim3 grid, int threads, size_t lds,
                  hipStream_t st) {
  a.src_words ? launch_stages<S, true>(a, nk, grid, threads, lds, st)
              : launch_stages<S, false>(a, nk, grid, threads, lds, st);
}

}  // namespace

void pool_mel_launch(PoolWaveArgs a, int nk, hipStream_t st) {
  const PoolBuildArgs& b = a.b;
  if (a.mel < 8 || a.mel > 128)
    throw std::invalid_argument("pool_wave: mel must be 0 or 8..128");
  if (a.dct < 0 || a.dct > a.mel)
    throw std::invalid_argument("pool_wave: dct must be 0..mel");
  if (a.dct && a.fmask_n)
    throw std::invalid_argument("pool_wave: dct with a frequency mask (bands of cepstral "
                                "coefficients) is refused");
  if (a.M16 != ((a.mel + 15) & ~15) || a.C16 != ((a.dct + 15) & ~15))
    throw std::invalid_argument("pool_wave: M16 and C16 are mel and dct rounded up to 16");
  if (!a.mel_tab || a.mel_floats != (long long)a.F16 * a.M16)
    throw std::invalid_argument("pool_wave: the mel table holds F16 rows of M16 floats");
  if (a.dct && (!a.dct_tab || a.dct_floats != (long long)a.M16 * a.C16))
    throw std::invalid_argument("pool_wave: the dct table holds M16 rows of C16 floats");
  const int nmt = a.M16 / 16, ksteps = a.F16 / 4;
  if (a.krange_n != 2 * nmt)
    throw std::invalid_argument("pool_wave: krange holds (first, last) per 16-band tile");
  for (int m = 0; m < nmt; ++m)
    if (a.krange[2 * m] < 0 || a.krange[2 * m + 1] >= ksteps)
      throw std::invalid_argument("pool_wave: krange steps must lie in 0..F16/4-1");
  a.panel_pitch = a.F16 + PANEL_PAD;
  a.lm_pitch = a.M16 + PANEL_PAD;
  a.rows = a.dct ? a.dct : a.mel;
  a.feat_pitch = (a.dct ? a.C16 : a.M16) + PANEL_PAD;
  a.dinv = 0.f;
  for (int n = 1; a.delta && n <= a.dwin; ++n) a.dinv += 2.f * n * n;
  if (a.delta) a.dinv = 1.f / a.dinv;
  if (a.cmvn) pool_cmvn_check(a);
  // With cmvn the first launch is the DELTA = false kernel whatever a.delta is: the rows are
  // differenced by pool_cmvn_kernel, and this kernel needs neither halo nor delta panels.
  const int delta = a.cmvn ? 0 : a.delta;
  const int ntiles = (b.W + 15) / 16;
  // A block that owns `tiles` tiles computes a window of one tile more (a halo of delta * dwin
  // <= 8 frames on each side, in whole tiles from its first frame), the clip's length at most.
  auto window = [&](int tiles) { return delta ? std::min(tiles + 1, ntiles) : tiles; };
  auto d1 = [&](int tiles) {       // the d1 panel: owned frames and dwin on each side
    return delta == 2 ? (long long)(16 * tiles + 2 * a.dwin) * a.feat_pitch : 0;
  };
  // LDS is two regions, each as long as the longest of what lies in it over the phases:
  // [0, panel_off) the stretch, the log-mel panel and (DCT) the d1 panel; then the power panel,
  // (DCT) the coefficient panel and (no DCT) the d1 panel.
  auto stretch = [&](int tiles) {
    const int wt = window(tiles);
    const long long lm = (a.dct || delta) ? (long long)16 * wt * a.lm_pitch : 0;
    return std::max({wave_stretch_words(wt, a.hop, nk), lm, a.dct ? d1(tiles) : 0LL});
  };
  // Speed perturbation: the resampler's source panel and table lie over the power panel, dead
  // until phase 1, and cost LDS only where they are the longest tenant of that region.
  const bool speed = wave_speed_on(a);
  auto panels = [&](int tiles) {
    const int wt = window(tiles);
    const long long coef = (a.dct && delta) ? (long long)16 * wt * a.feat_pitch : 0;
    const long long rs =
        speed ? wave_speed_words(wave_stretch_words(wt, a.hop, nk), a.rq_hi) : 0;
    return std::max({(long long)16 * wt * a.panel_pitch, coef, a.dct ? 0LL : d1(tiles), rs});
  };
  a.tiles_per_chunk = wave_tiles_per_chunk(a.chunks, b.P, ntiles, [&](int tiles) {
    return (stretch(tiles) + panels(tiles)) * 4;
  });
  const int chunks = (ntiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk;   // (no empty chunk)
  a.lds_words = (int)wave_stretch_words(window(a.tiles_per_chunk), a.hop, nk);
  a.panel_off = (int)stretch(a.tiles_per_chunk);
  a.feat_off = a.dct ? a.panel_off : 0;
  a.d1_off = a.dct ? 0 : a.panel_off;
  a.src_off = a.panel_off;
  a.src_words = speed ? (int)wave_src_words(a.lds_words, a.rq_hi) : 0;
  const size_t lds = ((size_t)a.panel_off + (size_t)panels(a.tiles_per_chunk)) * 4;
  const int threads = 64 * std::min(a.F16 / 16, nk > 64 ? 4 : 7);
  const dim3 grid(b.P, chunks);
  if (a.rev_on) pool_reverb_launch(a, st);
  if (a.f32)
    launch_typed<float>(a, nk, grid, threads, lds, st);
  else
    launch_typed<int16_t>(a, nk, grid, threads, lds, st);
  if (a.cmvn) pool_cmvn_launch(a, st);
}

