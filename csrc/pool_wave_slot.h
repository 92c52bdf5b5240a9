// The slot prologue shared by the waveform pool kernels (pool_wave.hip, pool_mel.hip): the
// slot's draws, its params row, and the LDS staging of the augmented, reflect-padded stretch.
// The draws, their stream words and the sample formula are documented at the top of
// pool_wave.hip; the frequency masks are drawn on the pool's row count b.H.
//
// Speed perturbation (SPEED = true; WaveRecipe.speed): one more Philox word, stream 0x5becc, .x
// draws a 16.16 rate rq = rq_lo + x % (rq_hi - rq_lo + 1) (augment = 0: 65536), and step 1 of the
// slot reads the clip through a polyphase resampler anchored at the clip's centre c = L >> 1:
//   pos = (c << 16) + (js - c) * rq (int64), i0 = pos >> 16, p = (pos & 0xffff) >> 10,
//   mu = (pos & 1023) / 1024, w_k = fma(mu, h[p + 1][k] - h[p][k], h[p][k]),
//   xs = sum_{k < 32} w_k x[i0 + k - 15], fmaf in ascending k, x = 0 outside [0, L),
// for js = j - shift in [0, L) (else 0, as without speed), then gain and noise as before.  h is
// WaveRecipe.speed_table(): 64 phases of a 32-tap Kaiser-windowed sinc and the wrap row 64.
// A slot that drew rq = 65536 takes wave_stage's x[js] itself (a slot-uniform branch).
//
// wave_stage_speed.  The padded indices q0 .. q0 + lds_words of a block fold to ONE contiguous
// range of j (the fold moves by +-1 per step), so to one range js0..js1 of clip positions and,
// pos being monotone, one range i0(js0) - 15 .. i0(js1) + 16 of source samples, at most
// (lds_words - 1) rq / 65536 + 33 long.  The block stages that range once, converted to fp32
// and zero outside the clip, into the LDS source panel, copies the table behind it, barriers,
// and every thread then runs the 32-tap FIR for its stretch words out of LDS:
//   source panel  [src_off, + src_words)        word i is source sample base + i
//   table         [src_off + src_words, + 65 * 33)   row pitch 33
// Lanes of a wave read source words i0 + k about `rate` apart: unit stride at rate 1, pairs on
// one word (a broadcast) at 0.5, stride 2 (two lanes per bank) at 2.  Their table rows differ
// (the phase walks by frac(rate) per lane), and with the odd pitch 33 rows p = 0..63 start on 64
// distinct banks, so lanes on different rows never collide and lanes on one row broadcast; at
// the table's own pitch of 32 every row would start on bank 0 or 32.
// A value depends on (js, rq) and the clip alone, never on q0: pools built with different
// chunk counts are bit-equal.
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
  int rq = 65536;                // SPEED: the 16.16 resampling rate
};

constexpr int SPEED_NT = 32, SPEED_PH = 64;          // taps, phases (the table has PH + 1 rows)
constexpr int SPEED_PITCH = SPEED_NT + 1;            // LDS row pitch of the table, odd
constexpr int SPEED_TAB_WORDS = (SPEED_PH + 1) * SPEED_PITCH;

// FEAT_ROWS: the frequency masks are drawn on a.rows, the R feature rows of a pool with delta
// rows, not on the pool's row count b.H
template <bool FEAT_ROWS = false, bool SPEED = false>
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
    if (SPEED) {
      const u32x4 r4 = pool_draw(gb, t, DRAW_WAVE + 4, b.seed);
      s.rq = a.rq_lo + (int)(r4.x % (uint32_t)(a.rq_hi - a.rq_lo + 1));
    }
  }
  return s;
}

// the slot's label, shard index and params row (one thread per slot calls this)
template <bool SPEED = false>
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
    p[14] = SPEED ? (float)(s.rq - 65536) : 0.f;
    if (!a.rev_on) p[15] = 0.f;        // (a reverb pre-pass wrote 1 + rir, pool_reverb.hip)
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

// source sample i0 and 16-bit fraction of clip position js at rate rq, about the centre c
MA_DEV int speed_pos(int js, int c, int rq, int& frac) {
  const long long pos = ((long long)c << 16) + (long long)(js - c) * rq;
  frac = (int)(pos & 0xffff);
  return (int)(pos >> 16);       // (arithmetic: floor)
}

// wave_stage with the slot's stretch read through the resampler (see the top of this file)
template <typename S>
MA_DEV void wave_stage_speed(const PoolWaveArgs& a, const WaveSlot& s, uint32_t src, int q0,
                             float* lds, int tid, int nthr) {
  const int L = a.L, W = a.n_fft, half = W >> 1, c = L >> 1;
  const S* x = (const S*)a.b.shard + (size_t)src * L;
  const S* nz = (const S*)a.noise + (size_t)s.clip * a.Ln + s.off;
  float* pan = lds + a.src_off;
  float* tab = pan + a.src_words;
  auto fold = [&](int j) {
    j = j < 0 ? -j : j;
    return j >= L ? 2 * (L - 1) - j : j;
  };
  // ---- the block's source range: q0 .. q1 -> j0 .. j1 -> js0 .. js1 -> base .. base + n
  const int e0 = q0 - half, e1 = min(q0 + a.lds_words, L + W) - 1 - half;
  int j0 = min(fold(e0), fold(e1)), j1 = max(fold(e0), fold(e1));
  if (e0 <= 0 && e1 >= 0) j0 = 0;                    // the stretch crosses the front fold
  if (e0 <= L - 1 && e1 >= L - 1) j1 = L - 1;        // ... the back fold
  const int js0 = max(j0 - s.shift, 0), js1 = min(j1 - s.shift, L - 1);
  int base = 0, n = 0, fr;
  if (js0 <= js1) {
    base = speed_pos(js0, c, s.rq, fr) - (SPEED_NT / 2 - 1);
    n = speed_pos(js1, c, s.rq, fr) + SPEED_NT / 2 + 1 - base;
  }
  n = min(n, a.src_words);       // (never binds: the launcher sized the panel for rq_hi)
  for (int i = tid; i < n; i += nthr) {
    const int g = base + i;
    pan[i] = (g >= 0 && g < L) ? wave_sample(x, g) : 0.f;
  }
  for (int i = tid; i < (SPEED_PH + 1) * SPEED_NT; i += nthr)
    tab[(i / SPEED_NT) * SPEED_PITCH + i % SPEED_NT] = a.speed_tab[i];
  __syncthreads();
  // ---- the FIR, one stretch word per thread and pass
  for (int i = tid; i < a.lds_words; i += nthr) {
    const int q = q0 + i;
    float v = 0.f;
    if (q < L + W) {
      const int j = fold(q - half);
      const int js = j - s.shift;
      float xs = 0.f;
      if (js >= 0 && js < L) {
        int frac;
        const int i0 = speed_pos(js, c, s.rq, frac);
        const float mu = (float)(frac & 1023) * (1.f / 1024.f);
        const float* h = tab + (frac >> 10) * SPEED_PITCH;
        const float* sp = pan + (i0 - (SPEED_NT / 2 - 1) - base);
#pragma unroll
        for (int k = 0; k < SPEED_NT; ++k)
          xs = fmaf(fmaf(mu, h[SPEED_PITCH + k] - h[k], h[k]), sp[k], xs);
      }
      v = s.gain * xs;
      if (s.noise_on) v = fmaf(s.vol, wave_sample(nz, j), v);
    }
    lds[i] = v;
  }
}

// the slot's staging: the resampler when the slot drew a rate other than 1.  `src` is the clip's
// row in a.b.shard: the shard index, or the slot when the shard is a reverb pre-pass's workspace
template <typename S, bool SPEED>
MA_DEV void wave_stage_slot(const PoolWaveArgs& a, const WaveSlot& s, uint32_t src, int q0,
                            float* lds, int tid, int nthr) {
  if (SPEED && s.rq != 65536)
    wave_stage_speed<S>(a, s, src, q0, lds, tid, nthr);
  else
    wave_stage<S>(a, s, src, q0, lds, tid, nthr);
}

// ---- host side: the launchers' frame-chunk rule
// LDS words of a block's waveform stretch: 16 * tiles frames at `hop`, 4 * nk samples each
inline long long wave_stretch_words(int tiles, int hop, int nk) {
  return (long long)(16 * tiles - 1) * hop + 4 * nk;
}

// Speed perturbation: checks the new arguments (rq_hi = 0: off) and returns whether it is on
inline bool wave_speed_on(const PoolWaveArgs& a) {
  if (!a.rq_hi && !a.rq_lo) return false;
  if (a.rq_lo < 32768 || a.rq_hi > 131072 || a.rq_lo > a.rq_hi)
    throw std::invalid_argument("pool_wave: speed is 32768 <= rq_lo <= rq_hi <= 131072 (16.16)");
  if (!a.speed_tab || a.speed_floats != (long long)(SPEED_PH + 1) * SPEED_NT)
    throw std::invalid_argument("pool_wave: the speed table holds 65 rows of 32 floats");
  return true;
}
// LDS words of the source panel behind a stretch of `words` at the fastest rate, and of the
// panel and the table together
inline long long wave_src_words(long long words, int rq_hi) {
  return (words * rq_hi + 65535) / 65536 + SPEED_NT + 2;
}
inline long long wave_speed_words(long long words, int rq_hi) {
  return wave_src_words(words, rq_hi) + SPEED_TAB_WORDS;
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
