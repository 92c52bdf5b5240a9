// Per-utterance cepstral mean and variance normalisation of the log-mel / MFCC pools
// (WaveRecipe.cmvn, mercury_amd/data/augment.py): the second launch of a cmvn recipe, behind
// pool_wave_mel_kernel<.., FEAT = true> (pool_mel.hip) on the same stream.
//
// pool_cmvn : feat [P][R][Tp] fp32, the raw features v[r][t] (Tp = T rounded up to 4; frames
//             >= T are never read) ->
//               mu_r  = mean_t v[r][t]
//               var_r = mean_t (v[r][t] - mu_r)^2                      (biased, Kaldi's apply-cmvn)
//               z     = v - mu_r                                       (cmvn = 1)
//               z     = (v - mu_r) / sqrt(var_r + CMVN_VAR_FLOOR)      (cmvn = 2)
//             -> y[r] = a z + b, y[R + r] = a d1(z), y[2R + r] = a d2(z) (pool_mel.hip's difference
//             operator, delta4's arithmetic, on the normalised row) -> masks -> one bf16 rounding
//             into channel 0 of the NHWC8 pool [P][(1 + delta) R][T][8].
//
// Why a kernel of its own: the first launch splits a clip into frame chunks over grid.y, so no
// block of it sees a whole row, and the statistics must come from the fp32 features, not from
// the bf16 pool.
//
// Grid (slot, ceil(R / 4)), 256 threads.  WAVE w OWNS FEATURE ROW r = 4 blockIdx.y + w for the
// whole clip: no reduction crosses a wave, no atomic, no second workspace.  LDS, fp32 words, one
// or two private rows per wave:
//   [w * Tp, + T)              the row: v, then z in place
//   [(4 + w) * Tp, + T)        (delta = 2) d1(z), from which d2 is taken
// so Tp <= CMVN_TP_MAX = 2048 keeps the block inside 64 KB.  The block's barriers only order a
// wave's own LDS writes before its own reads of other lanes' words; a wave past the last row
// (R % 4 != 0) does nothing between them.
//   1. lane l loads v[l], v[l + 64], ... (coalesced along t), parks them, and sums them in index
//      order; wave_sum's fixed xor tree adds the 64 partial sums (every lane gets the same bits,
//      fp32 addition commutes); mu = sum / T.
//   2. the lane's own elements again: c = v - mu, ss = fma(c, c, ss) in index order, the same
//      tree, rs = 1 / sqrtf(ss / T + floor) (cmvn = 1: rs = 1), and z = c * rs goes back into the
//      row.  Two passes on purpose: E[v^2] - mu^2 in fp32 loses everything for log features near
//      -14 with a spread of 0.1.  T = 1: mu = v exactly, z = 0, y = b.
//   3. output, one frame per lane and trip: y = a z + b, masks, rounding, the 16-byte pixel; the
//      wave writes 1 KiB contiguous per trip.  With delta the first difference of the row is
//      taken from LDS (clamped ends, one fma per n in ascending n, one multiply by dinv), written
//      as row R + r and (delta = 2) parked; after a barrier the same operator on the parked row
//      gives row 2R + r.
// Every value is a fixed sequence of fp32 operations on the workspace row, which does not depend
// on the first launch's chunk count (pool_mel.hip): pools built with different chunk counts are
// bit-equal, and so are two runs.  No atomics; capturable.
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"
#include "pool_wave_slot.h"

namespace {

constexpr int CMVN_WAVES = 4;

// frame t of pool row `row`: fill where masked, else y, one rounding; channels 1..7 +0
MA_DEV void cmvn_store(const PoolWaveArgs& a, const WaveSlot& s, int slot, int row, bool rmasked,
                       int t, float y) {
  const bool masked = rmasked || (t >= s.t0[0] && t < s.t0[0] + s.tw[0]) ||
                      (t >= s.t0[1] && t < s.t0[1] + s.tw[1]);
  const bf16 zero = f2bf(0.f);
  bf16x8 px;
  px[0] = masked ? f2bf(a.fill) : f2bf(y);
#pragma unroll
  for (int c = 1; c < 8; ++c) px[c] = zero;
  *(bf16x8*)(a.b.pool + (((size_t)slot * a.b.H + row) * a.b.W + t) * 8) = px;
}

// dinv * sum_{n <= N} n (x[clamp(t + n)] - x[clamp(t - n)]): delta4's arithmetic on an LDS row
MA_DEV float cmvn_delta(const float* x, int t, int T, int N, float dinv) {
  float acc = 0.f;
  for (int n = 1; n <= N; ++n) acc = fmaf((float)n, x[min(t + n, T - 1)] - x[max(t - n, 0)], acc);
  return acc * dinv;
}

__global__ __launch_bounds__(64 * CMVN_WAVES) void pool_cmvn_kernel(PoolWaveArgs a) {
  extern __shared__ float lds[];
  const PoolBuildArgs& b = a.b;
  const int slot = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = b.W, Tp = a.feat_tp, R = a.rows, N = a.dwin;
  const int r = blockIdx.y * CMVN_WAVES + wave;
  const bool live = r < R;
  float* row = lds + wave * Tp;
  float* d1p = lds + (CMVN_WAVES + wave) * Tp;       // (delta = 2 only: the launcher's LDS size)
  float rs = 1.f;
  if (live) {
    const float* v = a.feat + ((size_t)slot * R + r) * Tp;
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
      const float x = v[t];
      row[t] = x;
      sum += x;
    }
    const float mu = wave_sum(sum) / (float)T;
    float ss = 0.f;
    for (int t = lane; t < T; t += 64) {             // (the lane's own words: no barrier yet)
      const float c = row[t] - mu;
      ss = fmaf(c, c, ss);
    }
    if (a.cmvn == 2) rs = 1.f / sqrtf(wave_sum(ss) / (float)T + CMVN_VAR_FLOOR);
    for (int t = lane; t < T; t += 64) row[t] = (row[t] - mu) * rs;
  }
  __syncthreads();
  int64_t gb;
  int bt;
  pool_src(b, slot, gb, bt);
  const WaveSlot s = wave_slot_draws<true>(a, gb, bt);   // the first launch's masks (a speed
                                                            // recipe's rate is a draw of its own)
  const bool rmasked = (r >= s.f0[0] && r < s.f0[0] + s.fw[0]) ||
                       (r >= s.f0[1] && r < s.f0[1] + s.fw[1]);
  if (live)
    for (int t = lane; t < T; t += 64) {
      cmvn_store(a, s, slot, r, rmasked, t, a.log_a * row[t] + a.log_b);
      if (a.delta) {
        const float d = cmvn_delta(row, t, T, N, a.dinv);
        if (a.delta == 2) d1p[t] = d;
        cmvn_store(a, s, slot, R + r, rmasked, t, a.log_a * d);
      }
    }
  if (a.delta != 2) return;
  __syncthreads();
  if (live)
    for (int t = lane; t < T; t += 64)
      cmvn_store(a, s, slot, 2 * R + r, rmasked, t, a.log_a * cmvn_delta(d1p, t, T, N, a.dinv));
}

}  // namespace

void pool_cmvn_check(PoolWaveArgs& a) {
  const int R = a.dct ? a.dct : a.mel;
  a.feat_tp = (a.b.W + 3) & ~3;
  if (a.feat_tp > CMVN_TP_MAX)
    throw std::invalid_argument("pool_wave: cmvn keeps a clip's row in LDS: T rounded up to 4 "
                                "must stay within 2048 frames");
  const long long want = (long long)a.b.P * R * a.feat_tp;
  if (!a.feat || ((uintptr_t)a.feat & 15) || a.feat_floats != want)
    throw std::invalid_argument("pool_wave: the cmvn workspace holds P * R rows of T rounded up "
                                "to 4 floats, 16-byte aligned");
  if (want * 4 >= (1LL << 32))
    throw std::invalid_argument("pool_wave: the cmvn workspace must stay below 2^32 bytes");
}

void pool_cmvn_launch(const PoolWaveArgs& a, hipStream_t st) {
  const dim3 grid(a.b.P, (a.rows + CMVN_WAVES - 1) / CMVN_WAVES), blk(64 * CMVN_WAVES);
  const size_t lds = (size_t)CMVN_WAVES * (a.delta == 2 ? 2 : 1) * a.feat_tp * 4;
  hipLaunchKernelGGL(pool_cmvn_kernel, grid, blk, lds, st, a);
}
