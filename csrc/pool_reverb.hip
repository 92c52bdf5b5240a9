// Room-impulse reverberation of the waveform pools (WaveRecipe.reverb, mercury_amd/data/
// augment.py): the pre-pass of a reverb recipe, launched by pool_wave_launch on the same stream
// in front of pool_wave_kernel / pool_wave_mel_kernel.
//
// pool_reverb : shard [Ns][L] (int16 read as x / 32768, or float32), bank rir [Nr][K] fp32 ->
//               rev [P][L] fp32, indexed by SLOT:
//                 rev[slot][i] = sum_{k <= min(K - 1, i)} h[k] x[i - k]     (reverb drawn on)
//                 rev[slot][i] = x[i] converted to fp32, bit for bit        (drawn off)
//               x the slot's clip, h = rir[r.y % Nr], on iff u01(r.x) < p, r the Philox word of
//               stream DRAW_WAVE + 5 on the slot counter (gb, t).  params[slot][15] = 1 + rir
//               when on, else 0.  The wave kernels then run in their float32 form with rev as
//               the shard and the slot as the clip index (PoolWaveArgs.rev_on).
//
// The convolution as a GEMM on v_mfma_f32_16x16x4_f32.  A tile is 256 consecutive outputs
// i = i0 + 16 r + c, r, c in 0..15.  With k = u + c,
//   y[i0 + 16 r + c] = sum_u h[u + c] x[i0 + 16 r - u],      u = -16 .. U - 1,  U = K up to 16,
// a product [16 x (U + 16)] . [(U + 16) x 16] of a Hankel operand from the response and a
// Toeplitz operand from the clip; h outside [0, K) and x outside [0, L) are staged as zeros.  Of
// each instruction's 1024 multiply-adds K / (U + 16) are useful.  The response takes the A role:
// lane (c = lane % 16, kk = lane / 16) of K step u0 reads h[u0 + kk + c], 19 consecutive words of
// which equal ones broadcast.  The clip takes the B role: lane (r = lane % 16, kk) reads
// x[i0 + 16 r - u0 - kk].  The accumulator of lane (r, q = lane / 16) is then outputs i0 + 16 r +
// 4 q + 0..3: one 16-byte store per lane, and the wave's store covers the tile's 1 KiB.
//
// Work split.  Grid (slot, output chunk), 256 threads.  A block owns `rev_tiles` consecutive
// tiles [i_first, i_last], i_first a multiple of 256, and stages once, in fp32:
//   hs   [0, U + 32)                 word j is h[j - 16]; zero margins of 16 on each side
//   pan  [U + 32, + 20 (16 nt + U / 16))   the clip range [i_first - U + 1, i_first + 256 nt],
//                                    logical word w = g - (i_first - U + 1) at w + 4 (w >> 4)
// Its tiles are dealt to the 4 waves in runs of ceil(nt / 4) <= 4 consecutive tiles (16 tiles at
// a time when a forced chunk holds more): a wave keeps up to 4 independent accumulator chains
// and one A fragment read serves up to 4 MFMAs.
//
// The panel pitch.  Lane (r, kk) reads logical word 256 tt + 16 r + q, q = U + 15 - 16 so - 4 si -
// kk for K step u0 = -16 + 16 so + 4 si.  U is a multiple of 16, so the four kk of a step stay
// inside one 16-word group and the physical word is 320 tt + 20 (r + U / 16 - so) + 15 - 4 si - kk.
// On a flat row the 16 r would land on banks 16 r % 64: 4 distinct groups, 4 lanes per bank.
// With 4 pad words per 16 the r land on 20 r % 64 = the 16 multiples of 4, and the four kk fill
// the gaps: one lane per bank.  One pad word per 16 (pitch 17) leaves 2 lanes on three banks
// (bench/wave_bench.py banks); the 4-word pad costs 6 KB at the preset and keeps 4 blocks per CU.
//
// Order and determinism.  Every tile runs u0 ascending from -16, so the summation order of an
// output depends on i % 16 alone, not on its tile's place in a block or chunk: pools built with
// different chunk counts are bit-equal.  A wave stops at the last 16-step group that can still
// touch sample 0 or later of its LAST tile: what it drops, and what an earlier tile of the run
// adds beyond its own last group, are products with staged +0 clip words, and an accumulator
// that starts at +0 is never -0 under round-to-nearest, so adding +-0 leaves its bits (a finite
// bank, as a float32 shard must be finite).  No atomics, nothing allocated; capturable.
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"
#include "pool_wave_slot.h"

namespace {

constexpr int REV_TILE = 256;                 // outputs of one 16 x 16 tile
constexpr int REV_WAVES = 4, REV_RUN = 4;     // waves of a block, tiles of a wave's run
constexpr int REV_GROUP = 16, REV_PITCH = 20; // clip panel: 16 words at a pitch of 20
constexpr int REV_MARGIN = 16;                // zero words on each side of the response in LDS
constexpr uint32_t DRAW_REVERB = DRAW_WAVE + 5;

// CNT tiles from tile `tt` of the block (first output i0): so_end groups of 4 K steps
template <int CNT>
MA_DEV void reverb_run(const float* hs, const float* pan, int U, int tt, int so_end, int i0,
                       int L, bool vec, float* y, int lane) {
  const int r = lane & 15, kk = lane >> 4;
  const float* hp = hs + kk + r;                          // (A: c = lane % 16)
  const float* xp = pan + (REV_PITCH * REV_GROUP) * tt + REV_PITCH * (r + (U >> 4)) + 15 - kk;
  f32x4 acc[CNT];
#pragma unroll
  for (int j = 0; j < CNT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int so = 0; so < so_end; ++so) {
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      const float av = hp[16 * so + 4 * si];
#pragma unroll
      for (int j = 0; j < CNT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av, xp[(REV_PITCH * REV_GROUP) * j - REV_PITCH * so - 4 * si], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
    const int i = i0 + REV_TILE * j + 16 * r + 4 * kk;
    if (vec && i + 3 < L) {
      *(f32x4*)(y + i) = acc[j];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < L) y[i + e] = acc[j][e];
    }
  }
}

template <typename S>
__global__ __launch_bounds__(64 * REV_WAVES) void pool_reverb_kernel(PoolWaveArgs a) {
  extern __shared__ float lds[];
  const PoolBuildArgs& b = a.b;
  const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L, K = a.rir_k, U = a.rev_u;
  int64_t gb;
  int t;
  const uint32_t src = pool_src(b, slot, gb, t);
  const u32x4 rw = pool_draw(gb, t, DRAW_REVERB, b.seed);
  const bool on = u01(rw.x) < a.reverb_p;
  const int rir = (int)(rw.y % (uint32_t)a.Nr);
  if (tid == 0 && blockIdx.y == 0 && a.params)
    a.params[(size_t)slot * 16 + 15] = on ? (float)(1 + rir) : 0.f;
  const S* x = (const S*)a.rev_src + (size_t)src * L;
  float* y = a.rev + (size_t)slot * L;
  const int ntiles = (L + REV_TILE - 1) / REV_TILE;
  const int tile0 = blockIdx.y * a.rev_tiles;
  const int nt = min(a.rev_tiles, ntiles - tile0);
  const int i_first = tile0 * REV_TILE;
  if (!on) {                                   // (slot-uniform) the clip itself, converted
    const int i_end = min(i_first + nt * REV_TILE, L);
    for (int i = i_first + tid; i < i_end; i += 64 * REV_WAVES) y[i] = wave_sample(x, i);
    return;
  }
  // ---- stage the response with its margins and the block's clip range
  float* hs = lds;
  float* pan = lds + U + 2 * REV_MARGIN;
  const float* h = a.rir + (size_t)rir * K;
  for (int j = tid; j < U + 2 * REV_MARGIN; j += 64 * REV_WAVES) {
    const int k = j - REV_MARGIN;
    hs[j] = (k >= 0 && k < K) ? h[k] : 0.f;
  }
  const int base = i_first - U + 1, nlog = nt * REV_TILE + U;
  for (int w = tid; w < nlog; w += 64 * REV_WAVES) {
    const int g = base + w;
    pan[w + (REV_PITCH - REV_GROUP) * (w >> 4)] = (g >= 0 && g < L) ? wave_sample(x, g) : 0.f;
  }
  __syncthreads();
  // ---- the tiles, 16 at a time, in runs of consecutive tiles per wave
  const bool vec = (L & 3) == 0;
  const int groups = (U + 16) >> 4;            // groups of 4 K steps: u0 = -16 .. U - 4
  for (int g0 = 0; g0 < nt; g0 += REV_WAVES * REV_RUN) {
    const int ng = min(REV_WAVES * REV_RUN, nt - g0);
    const int per = (ng + REV_WAVES - 1) / REV_WAVES;
    const int tt = g0 + wave * per;
    const int cnt = min(per, ng - wave * per);
    if (cnt <= 0) continue;
    const int i0 = i_first + tt * REV_TILE;
    // the last group with a clip word at or after sample 0 of the run's last tile:
    // -16 + 16 so <= i0_last + 240
    const int so_end = min(groups, (i0 + (cnt - 1) * REV_TILE) / 16 + 17);
    switch (cnt) {
      case 1: reverb_run<1>(hs, pan, U, tt, so_end, i0, L, vec, y, lane); break;
      case 2: reverb_run<2>(hs, pan, U, tt, so_end, i0, L, vec, y, lane); break;
      case 3: reverb_run<3>(hs, pan, U, tt, so_end, i0, L, vec, y, lane); break;
      default: reverb_run<4>(hs, pan, U, tt, so_end, i0, L, vec, y, lane);
    }
  }
}

// LDS bytes of a block of `tiles` tiles at U padded taps
long long reverb_lds_bytes(int tiles, int U) {
  return 4LL * (U + 2 * REV_MARGIN + REV_PITCH * ((long long)tiles * REV_TILE + U) / REV_GROUP);
}

}  // namespace

bool pool_reverb_check(PoolWaveArgs& a) {
  a.rev_on = 0;
  if (a.reverb_p == 0.f && !a.rir && !a.rev) return false;
  const PoolBuildArgs& b = a.b;
  if (!(a.reverb_p > 0.f && a.reverb_p <= 1.f))
    throw std::invalid_argument("pool_wave: reverb p must lie in (0, 1]");
  if (a.rir_k < 1 || a.rir_k > REVERB_K_MAX || a.Nr < 1)
    throw std::invalid_argument("pool_wave: the RIR bank is [Nr >= 1][K], 1 <= K <= 4096");
  if (!a.rir || ((uintptr_t)a.rir & 3) || a.rir_floats != (long long)a.Nr * a.rir_k)
    throw std::invalid_argument("pool_wave: the RIR bank holds Nr rows of K floats");
  const long long want = (long long)b.P * a.L;
  if (!a.rev || ((uintptr_t)a.rev & 15) || a.rev_floats != want)
    throw std::invalid_argument("pool_wave: the reverb workspace holds P rows of L floats, "
                                "16-byte aligned");
  if (want * 4 >= (1LL << 32) || a.rir_floats * 4 >= (1LL << 32))
    throw std::invalid_argument("pool_wave: the reverb workspace and the RIR bank must stay "
                                "below 2^32 bytes");
  if (a.noise && !a.f32 && (!a.noise_f32 || (long long)a.Nn * a.Ln * 4 >= (1LL << 32)))
    throw std::invalid_argument("pool_wave: reverb on an int16 shard needs the noise bank's "
                                "float32 copy, below 2^32 bytes");
  // Chunk rule: about 1024 blocks in all, never fewer than 4 tiles per block (one per wave),
  // then as many more chunks as the block's LDS need takes to fit; rev_chunks > 0 forces it.
  const int ntiles = (a.L + REV_TILE - 1) / REV_TILE;
  a.rev_u = (a.rir_k + 15) & ~15;
  int chunks = a.rev_chunks;
  if (chunks < 0 || chunks > ntiles)
    throw std::invalid_argument("pool_wave: reverb chunks must be 0..number of 256-sample tiles");
  if (!chunks)
    for (chunks = std::max(1, std::min((1024 + b.P - 1) / b.P, (ntiles + 3) / 4));
         chunks < ntiles &&
         reverb_lds_bytes((ntiles + chunks - 1) / chunks, a.rev_u) > WAVE_LDS_MAX;)
      ++chunks;
  a.rev_tiles = (ntiles + chunks - 1) / chunks;
  if (reverb_lds_bytes(a.rev_tiles, a.rev_u) > WAVE_LDS_MAX)
    throw std::invalid_argument("pool_wave: the reverb chunk's LDS need (clip panel and "
                                "response) exceeds the LDS limit");
  if (!b.augment) return false;          // the identity draws: today's route, no pre-pass
  // the wave kernels read the workspace as a float32 shard indexed by slot
  a.rev_src = b.shard;
  a.rev_src_f32 = a.f32;
  a.b.shard = (const uint8_t*)a.rev;
  if (a.noise && !a.f32) a.noise = a.noise_f32;
  a.f32 = 1;
  a.rev_on = 1;
  return true;
}

void pool_reverb_launch(const PoolWaveArgs& a, hipStream_t st) {
  const int ntiles = (a.L + REV_TILE - 1) / REV_TILE;
  const dim3 grid(a.b.P, (ntiles + a.rev_tiles - 1) / a.rev_tiles), blk(64 * REV_WAVES);
  const size_t lds = (size_t)reverb_lds_bytes(a.rev_tiles, a.rev_u);
  if (a.rev_src_f32)
    hipLaunchKernelGGL(pool_reverb_kernel<float>, grid, blk, lds, st, a);
  else
    hipLaunchKernelGGL(pool_reverb_kernel<int16_t>, grid, blk, lds, st, a);
}
