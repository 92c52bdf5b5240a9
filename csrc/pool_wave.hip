// Waveform front end of the speech path: the presample pool straight from an HBM-resident shard
// of raw clips (WaveRecipe, mercury_amd/data/augment.py).
//
// pool_wave : shard [Ns][L] (int16 PCM read as x / 32768, or float32 as is) -> shift, gain and
//             background-noise mix on the waveform -> reflect centre padding -> windowed DFT on
//             the fp32 matrix cores -> a * ln(re^2 + im^2 + eps) + b -> frequency / time masks ->
//             bf16 channel 0 of the NHWC8 pool [P][F][T][8], F = W/2 + 1 bins (rows), T = 1 + L/hop
//             frames (columns).  Channels 1..7 are +0.
//
// The DFT is a GEMM [T frames x W] . [W x 2F] against a table Python builds once in fp64
// (ops.pool_wave_table): tab[4*NK][2*F16] fp32, columns [0, F) = w[n] cos(2 pi k n / W), columns
// [F16, F16 + F) = -w[n] sin(2 pi k n / W), w the periodic Hann window, F16 = F rounded up to 16,
// rows >= W and the padding columns zero.  The kernel evaluates no trigonometric function and
// never multiplies by the window.
//
// Work split.  Grid (slot, frame chunk).  A block stages its chunk's stretch of the augmented,
// reflect-padded waveform in LDS once, in fp32: shift, gain, noise mix and the reflect index map
// all happen in that loop, frames are never materialised.  A wave owns one tile of 16 bins -- the
// cos tile and the sin tile of the same bins -- loads those 2 * NK B fragments of
// v_mfma_f32_16x16x4_f32 into registers once (table stationary) and walks the chunk's tiles of 16
// frames (frames streaming).  Frames are the MFMA rows: the A operand of K step k is the single
// LDS word lds[(f0 + lane % 16) * hop + 4 k + lane / 16], so overlapping frames cost no extra
// bytes; the LDS row is flat (no pitch padding), a hop whose residue mod 64 collides takes the
// bank conflicts (hop = 100: 16 frames land on 16 distinct multiples of 4, conflict-free).  Real
// and imaginary accumulators of one (frame, bin) share lane and register index, so the power,
// the log and the affine need no cross-lane traffic; a lane holds 4 consecutive frames of one
// bin = four 16-byte pixel stores, 64 contiguous bytes.  With more bin tiles than waves a wave
// takes tiles wave, wave + nw, ... and reloads its fragments for each.
//
// NK (K steps held in registers) is a template parameter; W is padded up to 4 * NK with zero
// table rows (and the LDS stretch is zero past the padded signal).  A padded K step multiplies
// a zero table entry by the samples that follow the frame, which is an exact zero for finite
// data: a float32 shard must be finite, an Inf or NaN sample would also reach the frames
// before it as 0 * Inf.  No atomics, fixed K order: two launches are bit-equal.
//
// Draws per slot: Philox on the image kernels' counter (gb, t), stream words 0x5bec8..b:
//   0x5bec8: .x shift     .y gain      .z noise on   .w noise clip
//   0x5bec9: .x noise off .y noise vol .z width fa   .w start fa
//   0x5beca: .x width fb  .y start fb  .z width ta   .w start ta
//   0x5becb: .x width tb  .y start tb
// shift = x % (2 S + 1) - S; gain = fma(hi - lo, u01, lo); noise on iff u01 < p; clip = r % Nn;
// off = r % (Ln - L + 1); vol = vol_max u01; masks as pool_spec_kernel; augment = 0 draws the
// identity.  Augmented sample: xa[j] = gain * x[j - s] (0 outside the clip), then one fused
// multiply-add fmaf(vol, noise[clip][off + j], .) when noise is on.
//
// SPEED = true (WaveRecipe.speed): stream word 0x5becc .x draws a resampling rate and the stretch
// is staged through the polyphase resampler of pool_wave_slot.h, whose source panel and table
// lie behind the stretch in LDS ([lds_words, + src_words + 65 * 33)).  SPEED = false is the
// kernel as it was.
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"
#include "pool_wave_slot.h"

namespace {

template <typename S, int NK, bool SPEED = false>
__global__ __launch_bounds__(NK > 64 ? 256 : 448) void pool_wave_kernel(PoolWaveArgs a) {
  extern __shared__ float lds[];
  const PoolBuildArgs& b = a.b;
  const int slot = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int F = b.H, T = b.W;
  if (b.zero && blockIdx.y == 0)
    for (int j = slot * nthr + tid; j < b.nzero; j += gridDim.x * nthr) b.zero[j] = 0.f;
  int64_t gb;
  int t;
  const uint32_t src = pool_src(b, slot, gb, t);
  const WaveSlot s = wave_slot_draws<false, SPEED>(a, gb, t);
  if (tid == 0 && blockIdx.y == 0) wave_slot_header<SPEED>(a, slot, src, s);
  const int ntiles = (T + 15) >> 4;
  const int tile0 = blockIdx.y * a.tiles_per_chunk;
  const int ntile = min(a.tiles_per_chunk, ntiles - tile0);
  wave_stage_slot<S, SPEED>(a, s, a.rev_on ? (uint32_t)slot : src, tile0 * 16 * a.hop, lds, tid,
                            nthr);
  __syncthreads();

  // ---- table stationary, frames streaming
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int ldt = 2 * a.F16, nbt = a.F16 >> 4;
  const bf16 fill = f2bf(a.fill), zero = f2bf(0.f);
  for (int bt = wave; bt < nbt; bt += nw) {
    float bc[NK], bs[NK];
    const float* tp = a.tab + (size_t)kq * ldt + bt * 16 + col;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      bc[k] = tp[(size_t)(4 * k) * ldt];
      bs[k] = tp[(size_t)(4 * k) * ldt + a.F16];
    }
    const int bin = bt * 16 + col;
    const bool fmasked = (bin >= s.f0[0] && bin < s.f0[0] + s.fw[0]) ||
                         (bin >= s.f0[1] && bin < s.f0[1] + s.fw[1]);
    for (int ft = 0; ft < ntile; ++ft) {
      const float* fp = lds + (ft * 16 + col) * a.hop + kq;
      f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float av = fp[4 * k];
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bc[k], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bs[k], im, 0, 0, 0);
      }
      if (bin >= F) continue;         // (the tail tile's padding bins)
      const int tb = (tile0 + ft) * 16 + kq * 4;
      bf16* o = b.pool + (((size_t)slot * F + bin) * T + tb) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tt = tb + i;
        if (tt >= T) break;
        const float pw = re[i] * re[i] + im[i] * im[i] + a.eps;
        const bool masked = fmasked || (tt >= s.t0[0] && tt < s.t0[0] + s.tw[0]) ||
                            (tt >= s.t0[1] && tt < s.t0[1] + s.tw[1]);
        bf16x8 px;
        px[0] = masked ? fill : f2bf(a.log_a * __logf(pw) + a.log_b);
#pragma unroll
        for (int c = 1; c < 8; ++c) px[c] = zero;
        *(bf16x8*)(o + (size_t)i * 8) = px;
      }
    }
  }
}

template <typename S, bool SPEED>
void launch_nk(const PoolWaveArgs& a, int nk, dim3 grid, int threads, size_t lds, hipStream_t st) {
  const dim3 blk(threads);
#define WAVE_LAUNCH(NK) \
  hipLaunchKernelGGL((pool_wave_kernel<S, NK, SPEED>), grid, blk, lds, st, a)
  switch (nk) {
    case 16: WAVE_LAUNCH(16); break;
    case 32: WAVE_LAUNCH(32); break;
    case 50: WAVE_LAUNCH(50); break;
    case 64: WAVE_LAUNCH(64); break;
    default: WAVE_LAUNCH(128);
  }
#undef WAVE_LAUNCH
}

template <typename S>
void launch_typed(const PoolWaveArgs& a, bool speed, int nk, dim3 grid, int threads, size_t lds,
                  hipStream_t st) {
  speed ? launch_nk<S, true>(a, nk, grid, threads, lds, st)
        : launch_nk<S, false>(a, nk, grid, threads, lds, st);
}

}  // namespace

int pool_wave_ksteps(int n_fft) {
  for (int nk : {16, 32, 50, 64, 128})
    if (n_fft <= 4 * nk) return nk;
  return 0;
}

void pool_wave_launch(const PoolWaveArgs& a0, hipStream_t st) {
  PoolWaveArgs a = a0;
  const PoolBuildArgs& b = a.b;
  const int W = a.n_fft, L = a.L;
  if (W < 16 || W > 512 || (W & 1))
    throw std::invalid_argument("pool_wave: n_fft must be even, 16..512");
  if (a.hop < 1 || a.hop > W)
    throw std::invalid_argument("pool_wave: hop must be 1..n_fft");
  if (L <= W / 2)
    throw std::invalid_argument("pool_wave: L must exceed n_fft/2 (reflect padding)");
  if (b.Ns < 1 || b.P < 1 || b.batch < 1)
    throw std::invalid_argument("pool_wave: Ns, P and batch must be positive");
  if (a.mel < 0 || a.dct < 0 || (a.dct && !a.mel))
    throw std::invalid_argument("pool_wave: mel and dct are >= 0, dct needs mel");
  if (a.delta < 0 || a.delta > 2)
    throw std::invalid_argument("pool_wave: delta must be 0..2");
  if (a.delta && (a.dwin < 1 || a.dwin > 4))
    throw std::invalid_argument("pool_wave: dwin must be 1..4");
  if (a.delta && !a.mel)
    throw std::invalid_argument("pool_wave: delta needs mel (no delta rows on the linear bins)");
  if (a.cmvn < 0 || a.cmvn > 2)
    throw std::invalid_argument("pool_wave: cmvn must be 0..2");
  if (a.cmvn && !a.mel)
    throw std::invalid_argument("pool_wave: cmvn needs mel (no CMVN on the linear bins)");
  const int F = W / 2 + 1, T = 1 + L / a.hop;
  const int R = a.dct ? a.dct : a.mel ? a.mel : F;      // feature rows; the masks' row count
  if (b.H != (1 + a.delta) * R || b.W != T || a.F16 != ((F + 15) & ~15))
    throw std::invalid_argument("pool_wave: the pool is [P][(1 + delta) * (n_fft/2+1 | mel | "
                                "dct)][1+L/hop][8]");
  if (a.noise && (a.Nn < 1 || a.Ln < L))
    throw std::invalid_argument("pool_wave: the noise bank needs Nn >= 1 clips of Ln >= L samples");
  if (a.noise && (long long)a.Ln - L >= (1 << 24))
    throw std::invalid_argument("pool_wave: Ln - L must stay below 2^24");
  const long long es = a.f32 ? 4 : 2, lim = 1LL << 32;
  if ((long long)b.Ns * L * es >= lim || (a.noise && (long long)a.Nn * a.Ln * es >= lim) ||
      (long long)b.P * b.H * T * 16 >= lim)
    throw std::invalid_argument("pool_wave: every tensor must stay below 2^32 bytes");
  if (!(a.eps > 0.f))
    throw std::invalid_argument("pool_wave: eps must be positive");
  if (a.shift < 0 || a.fmask_n < 0 || a.fmask_n > 2 || a.fmask_max < 0 || a.fmask_max > R ||
      a.tmask_n < 0 || a.tmask_n > 2 || a.tmask_max < 0 || a.tmask_max > T)
    throw std::invalid_argument("pool_wave: shift >= 0, masks are (n <= 2, max <= size)");
  const int nk = pool_wave_ksteps(W);
  if (a.tab_floats != (long long)4 * nk * 2 * a.F16)
    throw std::invalid_argument("pool_wave: the table holds 4*ksteps rows of 2*F16 floats");
  const bool speed = wave_speed_on(a);
  pool_reverb_check(a);          // (with the pre-pass on: a.b.shard is its workspace from here)
  if (a.mel) return pool_mel_launch(a, nk, st);
  const int ntiles = (T + 15) / 16;
  // the stretch, and behind it the resampler's source panel and table
  auto words = [&](int tiles) { return wave_stretch_words(tiles, a.hop, nk); };
  auto need = [&](int tiles) {
    return words(tiles) + (speed ? wave_speed_words(words(tiles), a.rq_hi) : 0);
  };
  a.tiles_per_chunk = wave_tiles_per_chunk(a.chunks, b.P, ntiles,
                                           [&](int tiles) { return need(tiles) * 4; });
  const int chunks = (ntiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk;   // (no empty chunk)
  a.lds_words = (int)words(a.tiles_per_chunk);
  a.src_off = a.lds_words;
  a.src_words = speed ? (int)wave_src_words(a.lds_words, a.rq_hi) : 0;
  const size_t lds = (size_t)need(a.tiles_per_chunk) * 4;
  const int waves = std::min(a.F16 / 16, nk > 64 ? 4 : 7);
  const dim3 grid(b.P, chunks);
  if (a.rev_on) pool_reverb_launch(a, st);
  if (a.f32)
    launch_typed<float>(a, speed, nk, grid, waves * 64, lds, st);
  else
    launch_typed<int16_t>(a, speed, nk, grid, waves * 64, lds, st);
}
