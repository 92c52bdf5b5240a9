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
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"

namespace {

constexpr int WAVE_LDS_MAX = 64 * 1024;    // dynamic LDS of one block

MA_DEV float wave_sample(const int16_t* p, int i) { return (float)p[i] * (1.f / 32768.f); }
MA_DEV float wave_sample(const float* p, int i) { return p[i]; }

template <typename S, int NK>
__global__ __launch_bounds__(NK > 64 ? 256 : 448) void pool_wave_kernel(PoolWaveArgs a) {
  extern __shared__ float lds[];
  const PoolBuildArgs& b = a.b;
  const int slot = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int F = b.H, T = b.W, L = a.L, W = a.n_fft;
  if (b.zero && blockIdx.y == 0)
    for (int j = slot * nthr + tid; j < b.nzero; j += gridDim.x * nthr) b.zero[j] = 0.f;
  int64_t gb;
  int t;
  const uint32_t src = pool_src(b, slot, gb, t);
  int shift = 0, noise_on = 0, clip = 0, off = 0;
  float gain = 1.f, vol = 0.f;
  int f0[2] = {0, 0}, fw[2] = {0, 0}, t0[2] = {0, 0}, tw[2] = {0, 0};
  if (b.augment) {
    const u32x4 r0 = pool_draw(gb, t, DRAW_WAVE, b.seed);
    const u32x4 r1 = pool_draw(gb, t, DRAW_WAVE + 1, b.seed);
    const u32x4 r2 = pool_draw(gb, t, DRAW_WAVE + 2, b.seed);
    const u32x4 r3 = pool_draw(gb, t, DRAW_WAVE + 3, b.seed);
    shift = (int)(r0.x % (uint32_t)(2 * a.shift + 1)) - a.shift;
    gain = fmaf(a.gain_hi - a.gain_lo, u01(r0.y), a.gain_lo);   // (one rounding, by contract)
    if (a.noise && u01(r0.z) < a.noise_p) {
      noise_on = 1;
      clip = (int)(r0.w % (uint32_t)a.Nn);
      off = (int)(r1.x % (uint32_t)(a.Ln - L + 1));
      vol = a.vol_max * u01(r1.y);
    }
    const uint32_t wr[4] = {r1.z, r2.x, r2.z, r3.x}, sr[4] = {r1.w, r2.y, r2.w, r3.y};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < a.fmask_n) {
        fw[k] = (int)(wr[k] % (uint32_t)(a.fmask_max + 1));
        f0[k] = (int)(sr[k] % (uint32_t)(F - fw[k] + 1));
      }
      if (k < a.tmask_n) {
        tw[k] = (int)(wr[2 + k] % (uint32_t)(a.tmask_max + 1));
        t0[k] = (int)(sr[2 + k] % (uint32_t)(T - tw[k] + 1));
      }
    }
  }
  if (tid == 0 && blockIdx.y == 0) {
    pool_slot_header(b, slot, src);
    if (a.params) {
      float* p = a.params + (size_t)slot * 16;
      p[0] = (float)shift;
      p[1] = gain;
      p[2] = (float)noise_on;
      p[3] = (float)clip;
      p[4] = (float)off;
      p[5] = vol;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        p[6 + 2 * k] = (float)f0[k];
        p[7 + 2 * k] = (float)fw[k];
        p[10 + 2 * k] = (float)t0[k];
        p[11 + 2 * k] = (float)tw[k];
      }
      p[14] = p[15] = 0.f;
    }
  }

  // ---- stage the chunk's stretch of the padded signal: LDS word i is padded sample q0 + i
  const int ntiles = (T + 15) >> 4;
  const int tile0 = blockIdx.y * a.tiles_per_chunk;
  const int ntile = min(a.tiles_per_chunk, ntiles - tile0);
  const int q0 = tile0 * 16 * a.hop, half = W >> 1;
  const S* x = (const S*)b.shard + (size_t)src * L;
  const S* nz = (const S*)a.noise + (size_t)clip * a.Ln + off;
  for (int i = tid; i < a.lds_words; i += nthr) {
    const int q = q0 + i;
    float v = 0.f;
    if (q < L + W) {
      int j = q - half;               // reflect: one fold suffices since L > W / 2
      j = j < 0 ? -j : j;
      j = j >= L ? 2 * (L - 1) - j : j;
      const int js = j - shift;
      v = gain * ((js >= 0 && js < L) ? wave_sample(x, js) : 0.f);
      if (noise_on) v = fmaf(vol, wave_sample(nz, j), v);
    }
    lds[i] = v;
  }
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
    const bool fmasked = (bin >= f0[0] && bin < f0[0] + fw[0]) || (bin >= f0[1] && bin < f0[1] + fw[1]);
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
        const bool masked = fmasked || (tt >= t0[0] && tt < t0[0] + tw[0]) ||
                            (tt >= t0[1] && tt < t0[1] + tw[1]);
        bf16x8 px;
        px[0] = masked ? fill : f2bf(a.log_a * __logf(pw) + a.log_b);
#pragma unroll
        for (int c = 1; c < 8; ++c) px[c] = zero;
        *(bf16x8*)(o + (size_t)i * 8) = px;
      }
    }
  }
}

template <typename S>
void launch_typed(const PoolWaveArgs& a, int nk, dim3 grid, int threads, size_t lds,
                  hipStream_t st) {
  switch (nk) {
    case 16: hipLaunchKernelGGL((pool_wave_kernel<S, 16>), grid, dim3(threads), lds, st, a); break;
    case 32: hipLaunchKernelGGL((pool_wave_kernel<S, 32>), grid, dim3(threads), lds, st, a); break;
    case 50: hipLaunchKernelGGL((pool_wave_kernel<S, 50>), grid, dim3(threads), lds, st, a); break;
    case 64: hipLaunchKernelGGL((pool_wave_kernel<S, 64>), grid, dim3(threads), lds, st, a); break;
    default: hipLaunchKernelGGL((pool_wave_kernel<S, 128>), grid, dim3(threads), lds, st, a);
  }
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
  const int F = W / 2 + 1, T = 1 + L / a.hop;
  if (b.H != F || b.W != T || a.F16 != ((F + 15) & ~15))
    throw std::invalid_argument("pool_wave: the pool is [P][n_fft/2+1][1+L/hop][8]");
  if (a.noise && (a.Nn < 1 || a.Ln < L))
    throw std::invalid_argument("pool_wave: the noise bank needs Nn >= 1 clips of Ln >= L samples");
  if (a.noise && (long long)a.Ln - L >= (1 << 24))
    throw std::invalid_argument("pool_wave: Ln - L must stay below 2^24");
  const long long es = a.f32 ? 4 : 2, lim = 1LL << 32;
  if ((long long)b.Ns * L * es >= lim || (a.noise && (long long)a.Nn * a.Ln * es >= lim) ||
      (long long)b.P * F * T * 16 >= lim)
    throw std::invalid_argument("pool_wave: every tensor must stay below 2^32 bytes");
  if (!(a.eps > 0.f))
    throw std::invalid_argument("pool_wave: eps must be positive");
  if (a.shift < 0 || a.fmask_n < 0 || a.fmask_n > 2 || a.fmask_max < 0 || a.fmask_max > F ||
      a.tmask_n < 0 || a.tmask_n > 2 || a.tmask_max < 0 || a.tmask_max > T)
    throw std::invalid_argument("pool_wave: shift >= 0, masks are (n <= 2, max <= size)");
  const int nk = pool_wave_ksteps(W);
  if (a.tab_floats != (long long)4 * nk * 2 * a.F16)
    throw std::invalid_argument("pool_wave: the table holds 4*ksteps rows of 2*F16 floats");
  // Frame chunks per slot, by measurement (README, "Waveform front end": 4 of 2..11 win at P = 320
  // with 11 tiles, 6 at P = 32): about 1024 blocks in all, never fewer than two 16-frame tiles per
  // block, and then as many more as the LDS stretch [0, (16 tiles - 1) * hop + 4 nk) words needs.
  const int ntiles = (T + 15) / 16;
  auto words = [&](int tiles) { return (long long)(16 * tiles - 1) * a.hop + 4 * nk; };
  int chunks = a.chunks;
  if (chunks < 0 || chunks > ntiles)
    throw std::invalid_argument("pool_wave: chunks must be 0..number of 16-frame tiles");
  if (!chunks)
    for (chunks = std::max(1, std::min((1024 + b.P - 1) / b.P, (ntiles + 1) / 2));
         chunks < ntiles && words((ntiles + chunks - 1) / chunks) * 4 > WAVE_LDS_MAX;)
      ++chunks;
  a.tiles_per_chunk = (ntiles + chunks - 1) / chunks;
  chunks = (ntiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk;   // (no empty chunk)
  if (words(a.tiles_per_chunk) * 4 > WAVE_LDS_MAX)
    throw std::invalid_argument("pool_wave: the chunk's waveform stretch exceeds the LDS limit");
  a.lds_words = (int)words(a.tiles_per_chunk);
  const int waves = std::min(a.F16 / 16, nk > 64 ? 4 : 7);
  const dim3 grid(b.P, chunks);
  if (a.f32)
    launch_typed<float>(a, nk, grid, waves * 64, (size_t)a.lds_words * 4, st);
  else
    launch_typed<int16_t>(a, nk, grid, waves * 64, (size_t)a.lds_words * 4, st);
}
