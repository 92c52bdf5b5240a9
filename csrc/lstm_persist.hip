// Persistent bidirectional LSTM recurrence: ONE launch for all T steps of both directions of a
// layer (lstm.hip pays a launch per step).  Same arithmetic and saved layouts as the step kernels:
// bf16 operands, fp32 accumulation, h rounded to bf16 once per step, gates / dG in bf16, c in fp32,
// so either family can consume what the other wrote.  No h0 / c0.
//
// Work split.  A block is (direction, 16 hidden units) and owns ALL B batch rows of its slice for
// the whole sequence; the grid is 2 * H / 16 blocks of 4 waves (64 blocks at H = 512) and must be
// resident at once.  The forward block's slice is the 4 x 16 gate rows of W_hh[d] ([64][H]), the
// backward block's slice is 16 rows of the transposed copy W_hh^T ([16][4H]): 64 KB of bf16 at
// H = 512 either way.  The slice is loaded ONCE, before step 0, as ready MFMA "A" fragments in
// REGISTERS: K is dealt to the four waves in 32-deep chunks round-robin (chunk ch belongs to wave
// ch % 4), so a wave holds at most 16 fragments = 64 VGPRs and the MFMAs read their weights with
// no LDS or cache traffic at all.  (LDS would hold the slice too, but every MFMA would then pay an
// LDS read per step for data that never changes; with one block per CU the registers are free.)
//
// Per step a wave multiplies its K share against the rows of up to four 16-row batch tiles
// (v_mfma_f32_16x16x32_bf16, weights as "A", batch rows as "B": lane l holds row l & 15 and four
// consecutive units 4 * (l >> 4) .. +3 -- the step kernels' fragment layout), writes its partial
// accumulators to LDS, and wave w then finishes tile w of the pass: it sums the four partials in
// wave order (a fixed order, no atomics on data: two runs are bit-equal, though not bit-equal to
// the step kernels, whose K order is another), adds the fp32 pre[t] / dout[t], does the cell or
// gate-derivative update in registers and stores h_t into out[t] (8 bytes per lane) or dG[t]
// (4 x 8 bytes).  B > 64 rows loops over passes (B = 320: 5).  c (forward) and dc (backward) of the
// block's units live in LDS for the whole sequence, one f32x4 per (tile, lane), touched only by
// the lane that owns them.  The operands of the first pass that do not depend on other blocks
// (pre; dout, gates, c) are loaded BEFORE the barrier wait.  The exchange buffer between steps is
// out / dG itself.
//
// Barrier.  One arrival counter per direction (the directions never wait for each other), in a
// caller-owned workspace that a one-wave kernel clears in front of every launch (a kernel, not a
// memset node, so a captured graph clears it on every replay like any other launch).  After its
// stores of step s every thread issues an agent-scope release fence, the block synchronises and
// one lane adds 1 to the counter (agent-scope atomic).  Before step s + 1 one lane spins on an
// agent-scope atomic load until the counter reaches nblk * (s + 1); the block synchronises and
// every thread issues an agent-scope acquire fence.  All of it is __hip_atomic_* / fence builtins
// in plain C++ (the compiler emits the L2 write-back / invalidate cross-XCD visibility needs);
// there is no inline assembly and nothing is written to memory except by vector stores and those
// atomics.
//
// NO UNBOUNDED WAIT.  Every spin is bounded by SPIN_BUDGET ticks of wall_clock64() (100 MHz: 2 s,
// against legitimate waits of microseconds -- or, when blocks queue behind another stream's
// kernels, of that kernel's length).  On expiry the block ORs a nonzero code into the status word,
// waits for nothing for the rest of the sequence and runs to its end: a broken barrier shows as a
// wrong result plus a status code within about one budget, never as a hang.
//
// Lengths (<true> instantiations): lens is clamped to [0, T]; a padded (t, row) is taken by a
// branch, reads none of pre / dout / gates and stores exact zeros (h = +0, c = 0, dG = 0, dc = 0).
// Every block arrives at every barrier whatever its rows are.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int NW = 4, NT = 64 * NW;      // waves / threads per block
constexpr int UB = 16;                   // units (forward) or dh columns (backward) per block
constexpr int G = NW;                    // row tiles per pass: wave w finishes tile w of the pass
constexpr int KCF = LSTM_SEQ_MAX_H / 32 / NW;        // forward chunks per wave (x 4 gates)
constexpr int KCB = 4 * LSTM_SEQ_MAX_H / 32 / NW;    // backward chunks per wave (K = 4H)
constexpr long long SPIN_BUDGET = 200000000;         // wall_clock64 ticks (100 MHz): 2 s
constexpr size_t FWD_PART = (size_t)G * NW * 4 * 64 * sizeof(f32x4);   // 64 KB
constexpr size_t BWD_PART = (size_t)G * NW * 64 * sizeof(f32x4);       // 16 KB

MA_DEV float sigm(float x) { return 1.f / (1.f + expf(-x)); }
MA_DEV f32x4 ldf4(const float* p) { return *(const f32x4*)p; }
MA_DEV f32x4 ldb4(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
}
MA_DEV void stb4(bf16* p, f32x4 v) {
  *(bf16x4*)p = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}
MA_DEV bool frame_valid(const int* lens, int T, int B, int t, int b) {
  return t < min(max(lens[min(b, B - 1)], 0), T);
}

// ---- the grid barrier of one direction (both kernels) ----
// this block's stores of the step are done: publish them, then count the block in
MA_DEV void grid_arrive(int* ws, int d) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(ws + LSTM_WS_CTR * d, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// wait until `target` blocks-times-steps have arrived; `dead` (meaningful in thread 0 only) is
// set once a wait ran out of budget, and then nothing waits any more
MA_DEV void grid_wait(int* ws, int d, int target, bool& dead) {
  if (threadIdx.x == 0 && !dead) {
    int* ctr = ws + LSTM_WS_CTR * d;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (wall_clock64() - t0 > SPIN_BUDGET) {
        __hip_atomic_fetch_or(ws + LSTM_WS_STATUS, 1 + (int)(blockIdx.x << 1), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
        dead = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__global__ __launch_bounds__(64) void lstm_seq_clear_kernel(int* ws) {
  if (threadIdx.x < 2) ws[LSTM_WS_CTR * threadIdx.x] = 0;
}

template <bool LENS>
__global__ __launch_bounds__(NT) void lstm_seq_fwd_kernel(LstmSeqFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x4* part = (f32x4*)smem;                          // [G][NW][4 gates][64 lanes]
  f32x4* cst = (f32x4*)(smem + FWD_PART);              // [tiles][64 lanes]: c of this block's units
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int H = a.H, B = a.B, T = a.T;
  const int nblk = H / UB, d = blockIdx.x / nblk, u0 = (blockIdx.x % nblk) * UB;
  const int ntiles = (B + 15) / 16, nch = H / 32;
  const int r = lane & 15, kq = 8 * (lane >> 4), u = u0 + 4 * (lane >> 4);
  bool dead = false;

  // the resident slice: this wave's chunks of the four gates' rows, as MFMA A fragments
  bf16x8 fw[KCF][4];
#pragma unroll
  for (int j = 0; j < KCF; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = j * NW + w;
      fw[j][g] = bf16x8{};
      if (ch < nch)
        fw[j][g] = *(const bf16x8*)(a.whh + ((uint32_t)d * 4 * H + (uint32_t)g * H + u0 + r) * H +
                                    ch * 32 + kq);
    }

  int len0 = T;                      // the clamped length of the row this lane finishes in pass 0
  if constexpr (LENS) len0 = min(max(a.lens[min(w * 16 + r, B - 1)], 0), T);

  for (int s = 0; s < T; ++s) {
    const int t = d ? T - 1 - s : s, tp = d ? t + 1 : t - 1;
    // pre[t] of the tile this wave finishes in pass 0 depends on no other block: load it first
    f32x4 gp[4];
    {
      const int b = w * 16 + r;
      bool ok = w < ntiles && b < B;
      if constexpr (LENS) ok = ok && t < len0;
      if (ok) {
        const size_t grow = ((uint32_t)(t * 2 + d) * B + b) * 4 * H + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) gp[g] = ldf4(a.pre + grow + (uint32_t)g * H);
      }
    }
    if (s) grid_wait(a.ws, d, nblk * s, dead);
    const bf16* hp = a.out + (uint32_t)tp * B * 2 * H + (uint32_t)d * H + kq;

    for (int t0 = 0; t0 < ntiles; t0 += G) {
      if (s) {
        if (t0) __syncthreads();            // the previous pass's partials have been read
        bf16x8 fh[G][KCF];
#pragma unroll
        for (int m = 0; m < G; ++m)
#pragma unroll
          for (int j = 0; j < KCF; ++j) {
            // a chunk past H is read as chunk nch - 1 of the same row and meets a zero fw
            fh[m][j] = *(const bf16x8*)(hp + (uint32_t)min((t0 + m) * 16 + r, B - 1) * 2 * H +
                                        min(j * NW + w, nch - 1) * 32);
          }
#pragma unroll
        for (int m = 0; m < G; ++m) {
          if (t0 + m >= ntiles) continue;
          f32x4 acc[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < KCF; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
              acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j][g], fh[m][j], acc[g], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) part[((m * NW + w) * 4 + g) * 64 + lane] = acc[g];
        }
        __syncthreads();
      }
      // wave w finishes tile t0 + w: partials summed in wave order, then the cell update
      const int tile = t0 + w, b = tile * 16 + r;
      if (tile >= ntiles || b >= B) continue;
      float* ctp = a.c + ((uint32_t)(t * 2 + d) * B + b) * H + u;      // c[t] (training form)
      bf16* hout = a.out + ((uint32_t)t * B + b) * 2 * H + (uint32_t)d * H + u;
      if constexpr (LENS) {
        if (!(t0 ? frame_valid(a.lens, T, B, t, b) : t < len0)) {     // padded frame: h = +0, c = 0
          cst[tile * 64 + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
          *(short4v*)hout = short4v{0, 0, 0, 0};
          if (a.train) *(f32x4*)ctp = f32x4{0.f, 0.f, 0.f, 0.f};
          else if (s == T - 1)
            *(f32x4*)(a.c + ((uint32_t)d * B + b) * H + u) = f32x4{0.f, 0.f, 0.f, 0.f};
          continue;
        }
      }
      const size_t grow = ((uint32_t)(t * 2 + d) * B + b) * 4 * H + u;
      f32x4 gt[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        gt[g] = t0 ? ldf4(a.pre + grow + (uint32_t)g * H) : gp[g];
        if (s) {
#pragma unroll
          for (int ww = 0; ww < NW; ++ww) gt[g] += part[((w * NW + ww) * 4 + g) * 64 + lane];
        }
      }
      f32x4 cp = {0.f, 0.f, 0.f, 0.f};
      if (s) cp = cst[tile * 64 + lane];
      f32x4 ct, ht;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        gt[0][q] = sigm(gt[0][q]);
        gt[1][q] = sigm(gt[1][q]);
        gt[2][q] = tanhf(gt[2][q]);
        gt[3][q] = sigm(gt[3][q]);
        ct[q] = gt[1][q] * cp[q] + gt[0][q] * gt[2][q];
        ht[q] = gt[3][q] * tanhf(ct[q]);
      }
      cst[tile * 64 + lane] = ct;
      stb4(hout, ht);
      if (a.train) {
        *(f32x4*)ctp = ct;
#pragma unroll
        for (int g = 0; g < 4; ++g) stb4(a.gates + grow + (uint32_t)g * H, gt[g]);
      } else if (s == T - 1) {              // the inference form leaves the final running c
        *(f32x4*)(a.c + ((uint32_t)d * B + b) * H + u) = ct;
      }
    }
    grid_arrive(a.ws, d);
  }
}

template <bool LENS>
__global__ __launch_bounds__(NT) void lstm_seq_bwd_kernel(LstmSeqBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x4* part = (f32x4*)smem;                          // [G][NW][64 lanes]
  f32x4* dcst = (f32x4*)(smem + BWD_PART);             // [tiles][64 lanes]: dc of this block's units
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int H = a.H, B = a.B, T = a.T, K = 4 * H;
  const int nblk = H / UB, d = blockIdx.x / nblk, u0 = (blockIdx.x % nblk) * UB;
  const int ntiles = (B + 15) / 16, nch = K / 32;
  const int r = lane & 15, kq = 8 * (lane >> 4), u = u0 + 4 * (lane >> 4);
  bool dead = false;

  // the resident slice: this wave's chunks of 16 rows of W_hh^T
  bf16x8 fw[KCB];
#pragma unroll
  for (int j = 0; j < KCB; ++j) {
    const int ch = j * NW + w;
    fw[j] = bf16x8{};
    if (ch < nch) fw[j] = *(const bf16x8*)(a.whhT + ((uint32_t)d * H + u0 + r) * K + ch * 32 + kq);
  }

  int len0 = T;                      // the clamped length of the row this lane finishes in pass 0
  if constexpr (LENS) len0 = min(max(a.lens[min(w * 16 + r, B - 1)], 0), T);

  for (int s = 0; s < T; ++s) {
    const int t = d ? s : T - 1 - s;
    const int tn = d ? t - 1 : t + 1;      // the step whose dG this one multiplies
    const int tc = d ? t + 1 : t - 1;      // the step whose c is this step's c_prev
    const bool last = s == T - 1;
    // what pass 0's tile needs from the forward and from upstream depends on no other block
    f32x4 pdh, pg[4], pct, pcp = {0.f, 0.f, 0.f, 0.f};
    {
      const int b = w * 16 + r;
      bool ok = w < ntiles && b < B;
      if constexpr (LENS) ok = ok && t < len0;
      if (ok) {
        const size_t grow = ((uint32_t)(t * 2 + d) * B + b) * K + u;
        pdh = ldf4(a.dout + ((uint32_t)t * B + b) * 2 * H + (uint32_t)d * H + u);
#pragma unroll
        for (int g = 0; g < 4; ++g) pg[g] = ldb4(a.gates + grow + (uint32_t)g * H);
        pct = ldf4(a.c + ((uint32_t)(t * 2 + d) * B + b) * H + u);
        if (!last) pcp = ldf4(a.c + ((uint32_t)(tc * 2 + d) * B + b) * H + u);
      }
    }
    if (s) grid_wait(a.ws, d, nblk * s, dead);
    const bf16* gp = a.dG + (uint32_t)(tn * 2 + d) * B * K + kq;

    for (int t0 = 0; t0 < ntiles; t0 += G) {
      if (s) {
        if (t0) __syncthreads();
#pragma unroll
        for (int m = 0; m < G; ++m) {
          if (t0 + m >= ntiles) continue;
          const bf16* grow = gp + (uint32_t)min((t0 + m) * 16 + r, B - 1) * K;
          bf16x8 fg[KCB];
#pragma unroll
          for (int j = 0; j < KCB; ++j)     // a chunk past 4H: see the forward
            fg[j] = *(const bf16x8*)(grow + min(j * NW + w, nch - 1) * 32);
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < KCB; ++j)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j], fg[j], acc, 0, 0, 0);
          part[(m * NW + w) * 64 + lane] = acc;
        }
        __syncthreads();
      }
      const int tile = t0 + w, b = tile * 16 + r;
      if (tile >= ntiles || b >= B) continue;
      const size_t grow = ((uint32_t)(t * 2 + d) * B + b) * K + u;
      float* dcout = a.dc + ((uint32_t)d * B + b) * H + u;
      if constexpr (LENS) {
        if (!(t0 ? frame_valid(a.lens, T, B, t, b) : t < len0)) {     // padded frame: dG[t] = 0, dc = 0
#pragma unroll
          for (int g = 0; g < 4; ++g) *(short4v*)(a.dG + grow + (uint32_t)g * H) = short4v{0, 0, 0, 0};
          dcst[tile * 64 + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (last) *(f32x4*)dcout = f32x4{0.f, 0.f, 0.f, 0.f};
          continue;
        }
      }
      f32x4 dh = pdh, gi = pg[0], gf = pg[1], gg = pg[2], go = pg[3], ct = pct, cp = pcp;
      if (t0) {
        dh = ldf4(a.dout + ((uint32_t)t * B + b) * 2 * H + (uint32_t)d * H + u);
        gi = ldb4(a.gates + grow), gf = ldb4(a.gates + grow + H);
        gg = ldb4(a.gates + grow + 2 * (uint32_t)H), go = ldb4(a.gates + grow + 3 * (uint32_t)H);
        ct = ldf4(a.c + ((uint32_t)(t * 2 + d) * B + b) * H + u);
        if (!last) cp = ldf4(a.c + ((uint32_t)(tc * 2 + d) * B + b) * H + u);
      }
      f32x4 dcn = {0.f, 0.f, 0.f, 0.f};
      if (s) {
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) dh += part[(w * NW + ww) * 64 + lane];
        dcn = dcst[tile * 64 + lane];
      }
      f32x4 di, df, dg, dgo, dcprev;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float th = tanhf(ct[q]);
        const float dc = dcn[q] + dh[q] * go[q] * (1.f - th * th);
        dgo[q] = dh[q] * th * go[q] * (1.f - go[q]);
        di[q] = dc * gg[q] * gi[q] * (1.f - gi[q]);
        df[q] = dc * cp[q] * gf[q] * (1.f - gf[q]);
        dg[q] = dc * gi[q] * (1.f - gg[q] * gg[q]);
        dcprev[q] = dc * gf[q];
      }
      stb4(a.dG + grow, di);
      stb4(a.dG + grow + H, df);
      stb4(a.dG + grow + 2 * (uint32_t)H, dg);
      stb4(a.dG + grow + 3 * (uint32_t)H, dgo);
      dcst[tile * 64 + lane] = dcprev;
      if (last) *(f32x4*)dcout = dcprev;
    }
    grid_arrive(a.ws, d);
  }
}

void check_shape(const char* what, int T, int B, int H) {
  const std::string w(what);
  if (H < 32 || H % 32 != 0) throw std::invalid_argument(w + ": H must be a positive multiple of 32");
  if (H > LSTM_SEQ_MAX_H)
    throw std::invalid_argument(w + ": H above " + std::to_string(LSTM_SEQ_MAX_H) +
                                " (the resident weight slice is sized for it)");
  if (B < 1 || T < 1) throw std::invalid_argument(w + ": B and T must be >= 1");
  if (B > LSTM_SEQ_MAX_B)
    throw std::invalid_argument(w + ": B above " + std::to_string(LSTM_SEQ_MAX_B) +
                                " (the resident c / dc state is sized for it)");
  if ((unsigned long long)T * 2 * B * 4 * H * 4 >= (1ull << 32))    // 32-bit element indices
    throw std::invalid_argument(w + ": pre / dG of 2^32 bytes or more");
}

// all blocks must be resident together: the grid fits the CUs and a block fits a CU.  Asked of
// the runtime once per instantiation, with the largest LDS a launch can take (as the other
// launchers set their LDS attribute once), so a later launch inside a capture makes no such call.
constexpr size_t STATE_MAX = (size_t)(LSTM_SEQ_MAX_B / 16) * 64 * sizeof(f32x4);
struct Resident { int cus = 0, per_cu = 0; };
void check_resident(const char* what, const void* kernel, Resident& r, int grid, size_t lds_max) {
  const std::string w(what);
  if (!r.cus) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      throw std::invalid_argument(w + ": no HIP device");
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, NT, lds_max) != hipSuccess)
      per_cu = 0;
    r.per_cu = per_cu;
    r.cus = cus;
  }
  if (grid > r.cus)
    throw std::invalid_argument(w + ": " + std::to_string(grid) + " blocks on " +
                                std::to_string(r.cus) + " CUs cannot be resident together");
  if (r.per_cu < 1)
    throw std::invalid_argument(w + ": a block with " + std::to_string(lds_max) +
                                " bytes of LDS does not fit a CU");
}

}  // namespace

void lstm_seq_fwd_launch(const LstmSeqFwdArgs& a, hipStream_t st) {
  check_shape("lstm_seq_fwd", a.T, a.B, a.H);
  if (!a.pre || !a.whh || !a.out || !a.c || !a.ws || (a.train && !a.gates))
    throw std::invalid_argument("lstm_seq_fwd: null operand");
  const int grid = 2 * a.H / UB;
  const size_t lds = FWD_PART + (size_t)((a.B + 15) / 16) * 64 * sizeof(f32x4);
  static Resident res[2];
  const void* k = a.lens ? (const void*)lstm_seq_fwd_kernel<true>
                         : (const void*)lstm_seq_fwd_kernel<false>;
  check_resident("lstm_seq_fwd", k, res[a.lens != nullptr], grid, FWD_PART + STATE_MAX);
  lstm_seq_clear_kernel<<<1, 64, 0, st>>>(a.ws);
  if (a.lens) lstm_seq_fwd_kernel<true><<<grid, NT, lds, st>>>(a);
  else lstm_seq_fwd_kernel<false><<<grid, NT, lds, st>>>(a);
  HIP_LAUNCH_CHECK();
}

void lstm_seq_bwd_launch(const LstmSeqBwdArgs& a, hipStream_t st) {
  check_shape("lstm_seq_bwd", a.T, a.B, a.H);
  if (!a.dout || !a.gates || !a.c || !a.whhT || !a.dG || !a.dc || !a.ws)
    throw std::invalid_argument("lstm_seq_bwd: null operand");
  const int grid = 2 * a.H / UB;
  const size_t lds = BWD_PART + (size_t)((a.B + 15) / 16) * 64 * sizeof(f32x4);
  static Resident res[2];
  const void* k = a.lens ? (const void*)lstm_seq_bwd_kernel<true>
                         : (const void*)lstm_seq_bwd_kernel<false>;
  check_resident("lstm_seq_bwd", k, res[a.lens != nullptr], grid, BWD_PART + STATE_MAX);
  lstm_seq_clear_kernel<<<1, 64, 0, st>>>(a.ws);
  if (a.lens) lstm_seq_bwd_kernel<true><<<grid, NT, lds, st>>>(a);
  else lstm_seq_bwd_kernel<false><<<grid, NT, lds, st>>>(a);
  HIP_LAUNCH_CHECK();
}
