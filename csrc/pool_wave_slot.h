// The slot prologue shared by the waveform pool kernels (pool_wave.hip, pool_mel.hip): the
// slot's draws, its params row, and the LDS staging of the augmented, reflect-padded stretch.
// The draws, their stream words and the sample formula are documented at the top of
// pool_wave.hip; the frequency masks are drawn on the pool's row count b.H.
#pragma once
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "pool_geom.h"

constexpr int WAVE_LDS_MAX = 64 * 1024;    // dynamic LDS of one block

MA_DEV float wave_sample(const int16_t* p, int i) { return (float)p[i] * (1.f / 32768.f); }
MA_DEV float wave_sample(const float* p, int i) { return p[i]; }

struct WaveSlot {
  int shift = 0, noise_on = 0, clip = 0, off = 0;
  float gain = 1.f, vol = 0.f;
  int f0[2] = {0, 0}, fw[2] = {0, 0}, t0[2] = {0, 0}, tw[2] = {0, 0};
};

// FEAT_ROWS: the frequency masks are drawn on a.rows, the R feature rows of a pool with delta
// rows, not on the pool's row count b.H
template <bool FEAT_ROWS = false>
MA_DEV WaveSlot wave_slot_draws(const PoolWaveArgs& a, int64_t gb, int t) {
  const PoolBuildArgs& b = a.b;
  WaveSlot s;
  if (b.augment) {
    const u32x4 r0 = pool_draw(gb, t, DRAW_WAVE, b.seed);
    const u32x4 r1 = pool_draw(gb, t, DRAW_WAVE + 1, b.seed);
    const u32x4 r2 = pool_draw(gb, t, DRAW_WAVE + 2, b.seed);
    const u32x4 r3 = pool_draw(gb, t, DRAW_WAVE + 3, b.seed);
    s.shift = (int)(r0.x % (uint32_t)(2 * a.shift + 1)) - a.shift;
    s.gain = fmaf(a.gain_hi - a.gain_lo, u01(r0.y), a.gain_lo);   // (one rounding, by contract)
    if (a.noise && u01(r0.z) < a.noise_p) {
      s.noise_on = 1;
      s.clip = (int)(r0.w % (uint32_t)a.Nn);
      s.off = (int)(r1.x % (uint32_t)(a.Ln - a.L + 1));
      s.vol = a.vol_max * u01(r1.y);
    }
    const uint32_t wr[4] = {r1.z, r2.x, r2.z, r3.x}, sr[4] = {r1.w, r2.y, r2.w, r3.y};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < a.fmask_n) {
        s.fw[k] = (int)(wr[k] % (uint32_t)(a.fmask_max + 1));
        s.f0[k] = (int)(sr[k] % (uint32_t)((FEAT_ROWS ? a.rows : b.H) - s.fw[k] + 1));
      }
      if (k < a.tmask_n) {
        s.tw[k] = (int)(wr[2 + k] % (uint32_t)(a.tmask_max + 1));
        s.t0[k] = (int)(sr[2 + k] % (uint32_t)(b.W - s.tw[k] + 1));
      }
    }
  }
  return s;
}

// the slot's label, shard index and params row (one thread per slot calls this)
MA_DEV void wave_slot_header(const PoolWaveArgs& a, int slot, uint32_t src, const WaveSlot& s) {
  pool_slot_header(a.b, slot, src);
  if (a.params) {
    float* p = a.params + (size_t)slot * 16;
    p[0] = (float)s.shift;
    p[1] = s.gain;
    p[2] = (float)s.noise_on;
    p[3] = (float)s.clip;
    p[4] = (float)s.off;
    p[5] = s.vol;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      p[6 + 2 * k] = (float)s.f0[k];
      p[7 + 2 * k] = (float)s.fw[k];
      p[10 + 2 * k] = (float)s.t0[k];
      p[11 + 2 * k] = (float)s.tw[k];
    }
    p[14] = p[15] = 0.f;
  }
}

// stage the chunk's stretch of the padded signal: LDS word i is padded sample q0 + i
template <typename S>
MA_DEV void wave_stage(const PoolWaveArgs& a, const WaveSlot& s, uint32_t src, int q0, float* lds,
                       int tid, int nthr) {
  const int L = a.L, W = a.n_fft, half = W >> 1;
  const S* x = (const S*)a.b.shard + (size_t)src * L;
  const S* nz = (const S*)a.noise + (size_t)s.clip * a.Ln + s.off;
  for (int i = tid; i < a.lds_words; i += nthr) {
    const int q = q0 + i;
    float v = 0.f;
    if (q < L + W) {
      int j = q - half;               // reflect: one fold suffices since L > W / 2
      j = j < 0 ? -j : j;
      j = j >= L ? 2 * (L - 1) - j : j;
      const int js = j - s.shift;
      v = s.gain * ((js >= 0 && js < L) ? wave_sample(x, js) : 0.f);
      if (s.noise_on) v = fmaf(s.vol, wave_sample(nz, j), v);
    }
    lds[i] = v;
  }
}

// ---- host side: the launchers' frame-chunk rule
// LDS words of a block's waveform stretch: 16 * tiles frames at `hop`, 4 * nk samples each
inline long long wave_stretch_words(int tiles, int hop, int nk) {
  return (long long)(16 * tiles - 1) * hop + 4 * nk;
}

// Tiles of 16 frames per block.  Frame chunks per slot, by measurement on pool_wave_kernel
// (README, "Waveform front end": 4 of 2..11 win at P = 320 with 11 tiles, 6 at P = 32): about
// 1024 blocks in all, never fewer than two 16-frame tiles per block, and then as many more as
// lds_bytes(tiles), the block's whole LDS need, takes to fit WAVE_LDS_MAX.  `chunks` > 0 forces
// the count; a forced count that does not fit throws.
template <typename Fn>
inline int wave_tiles_per_chunk(int chunks, int P, int ntiles, Fn lds_bytes) {
  if (chunks < 0 || chunks > ntiles)
    throw std::invalid_argument("pool_wave: chunks must be 0..number of 16-frame tiles");
  if (!chunks)
    for (chunks = std::max(1, std::min((1024 + P - 1) / P, (ntiles + 1) / 2));
         chunks < ntiles && lds_bytes((ntiles + chunks - 1) / chunks) > WAVE_LDS_MAX;)
      ++chunks;
  const int tiles = (ntiles + chunks - 1) / chunks;
  if (lds_bytes(tiles) > WAVE_LDS_MAX)
    throw std::invalid_argument("pool_wave: the chunk's LDS need (waveform stretch and panels) "
                                "exceeds the LDS limit");
  return tiles;
}
