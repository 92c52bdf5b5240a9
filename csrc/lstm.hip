// Bidirectional LSTM recurrence (MyLSTM's two nn.LSTM(bidirectional=True, num_layers=1) layers,
// `pytorch_model.py:156-242`): the sequential half of the cell as one launch per
// time step, both directions in the same launch (blockIdx.z; direction 1 walks t = T-1 .. 0).
// The time-batched GEMMs (x . W_ih^T, dW, dx) stay with the caller; stream order is the only
// dependency between steps -- no persistent kernel, no grid barrier.
//
// forward step   gates = pre[t] + h_prev . W_hh^T   (i, f, g, o as torch orders them)
//                c_t = f * c_prev + i * g,  h_t = o * tanh(c_t)
// backward step  dh = dout[t] + dG[t_next] . W_hh  (read through the transposed copy W_hh^T),
//                then the gate derivatives from the saved gates, c_t, c_prev and dc_next.
//
// Both GEMMs issue v_mfma_f32_16x16x32_bf16 with the weights as the "A" input and the batch rows
// as "B" (as igemm.hip does), so the accumulator comes out transposed: lane l holds batch row
// l & 15 and FOUR CONSECUTIVE hidden units 4 * (l >> 4) .. +3.  The forward keeps one accumulator
// per gate for the same (row, units), so the cell update runs in registers and every store is a
// contiguous 8 or 16 bytes; nothing goes through LDS.  Both operands are K-contiguous in HBM
// (h_prev is the previous step's slice of out[], dG and the weight copies are row-major), so a
// lane's 16-byte load is exactly its MFMA fragment.  One wave per block: 16 units x 16 * MB batch
// rows; rows past B read row B-1 (their MFMA columns are independent) and are never stored.
// No atomics: every output element has one writer, so two runs are bit-equal.
//
// Lengths (the <.., true> instantiations, args.lens != null): frame (t, b) is valid iff
// t < len_b = clamp(lens[b], 0, T) -- packed-sequence semantics by per-row masking.  A lane whose
// row is padded at this step's t reads none of pre / dout / gates and stores exact zeros: h = +0
// and c = 0 in the forward, dG[t] = 0 and dc = 0 in the backward (a select by branch, never a
// multiply, so a NaN in the padding reaches nothing).  That alone makes both directions right:
// the reverse pass of row b first becomes valid at t = len_b - 1 and finds the zero h and c an
// earlier launch stored at len_b; the backward's first valid step finds dG[len_b] = 0 and dc = 0.
// A wave whose rows are all padded at this step (rows past B count as padded) skips the K loop:
// no weight, h_prev or dG loads, only its zero stores.  Without lens the kernels are the
// <.., false> instantiations: the code they were before lengths existed.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace {

MA_DEV float sigm(float x) { return 1.f / (1.f + expf(-x)); }

MA_DEV f32x4 ldf4(const float* p) { return *(const f32x4*)p; }
MA_DEV f32x4 ldb4(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
}
MA_DEV void stb4(bf16* p, f32x4 v) {
  *(bf16x4*)p = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}

// The backward's K = 4H loop is latency-bound (few waves, one 16-byte load per fragment straight
// from L2/HBM), so it is written in groups of U 32-deep chunks -- the group's loads are all
// issued in the source before its MFMAs, which lets the scheduler run loads well ahead of the
// MFMAs that use them (it does not keep all 16 chunks live: the kernels take 68-76 VGPRs) -- and
// a chunk-by-chunk tail takes what 4H % (32 U) leaves.  U and the tiles per wave can be set at
// build time for A/B builds (bench/build_variant.py with -DLSTM_BWD_U=.. -DLSTM_TILES_PER_WAVE=..)
// and bench/lstm_step_probe.py times the step kernels alone (profiles/r8/lstm/step_probe.jsonl).
// Backward, us per step at H = 512 with two tiles per wave, U = 1 / 4 / 8 / 16: B = 32 20.0 / 16.8 /
// 15.2 / 12.9, B = 320 26.6 / 27.1 / 25.4 / 23.7 (the shipped B = 32 path uses one tile: 8.8).
// The forward has four weight fragments per chunk already; grouping its chunks the same way
// measured slower in a one-off variant that was not kept (12.2 us per step plain, 13.3 at 2, 14.1
// at 4; H = 512, B = 32, two tiles per wave).
#ifndef LSTM_BWD_U
#define LSTM_BWD_U 16
#endif
constexpr int BWD_U = LSTM_BWD_U;

template <int MB, int U>
MA_DEV void bwd_chunks(const bf16* w, const bf16* const (&grow)[MB], int k0, f32x4 (&acc)[MB]) {
  bf16x8 fw[U], fg[U][MB];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    fw[j] = *(const bf16x8*)(w + 32 * j);
#pragma unroll
    for (int m = 0; m < MB; ++m) fg[j][m] = *(const bf16x8*)(grow[m] + k0 + 32 * j);
  }
#pragma unroll
  for (int j = 0; j < U; ++j)
#pragma unroll
    for (int m = 0; m < MB; ++m)
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j], fg[j][m], acc[m], 0, 0, 0);
}

// valid[m]: this lane's row of tile m is a real row and t is inside its sequence; returns whether
// any lane of the wave has a valid row in any tile (wave-uniform)
template <int MB>
MA_DEV bool row_valid(const int* lens, int T, int B, int t, int b0, int lane, bool (&valid)[MB]) {
  bool any = false;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int b = b0 + 16 * m + (lane & 15);
    valid[m] = b < B && t < min(max(lens[min(b, B - 1)], 0), T);
    any |= valid[m];
  }
#ifdef LSTM_NO_WAVE_SKIP
  return true;                         // A/B builds only: what skipping all-padded waves buys
#else
  return __ballot(any) != 0;
#endif
}

template <int MB, bool LENS>
__global__ __launch_bounds__(64) void lstm_step_fwd_kernel(LstmFwdArgs a) {
  const int lane = threadIdx.x, d = blockIdx.z;
  const int H = a.H, B = a.B;
  const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16 * MB;
  const int t = d ? a.T - 1 - a.s : a.s, tp = d ? t + 1 : t - 1;
  const bool first = a.s == 0;
  // h_prev: the previous step's half of out[] (row stride 2H), or h0 [2][B][H], or zero
  const bf16* hp = first ? (a.h0 ? a.h0 + (size_t)d * B * H : nullptr)
                         : a.out + (size_t)tp * B * 2 * H + (size_t)d * H;
  const int ldh = first ? H : 2 * H;
  bool valid[MB], work = true;
  if constexpr (LENS) work = row_valid<MB>(a.lens, a.T, B, t, b0, lane, valid);

  f32x4 acc[MB][4];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (hp && work) {
    const int kq = 8 * (lane >> 4);
    const bf16* wrow = a.whh + ((size_t)d * 4 * H + u0 + (lane & 15)) * H + kq;
    const bf16* hrow[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
      hrow[m] = hp + (size_t)min(b0 + 16 * m + (lane & 15), B - 1) * ldh + kq;
    for (int k0 = 0; k0 < H; k0 += 32) {
      bf16x8 fw[4], fh[MB];
#pragma unroll
      for (int g = 0; g < 4; ++g) fw[g] = *(const bf16x8*)(wrow + (size_t)g * H * H + k0);
#pragma unroll
      for (int m = 0; m < MB; ++m) fh[m] = *(const bf16x8*)(hrow[m] + k0);
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[m][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[g], fh[m], acc[m][g], 0, 0, 0);
    }
  }

  // cell update in registers: this lane owns units u .. u+3 of row b, all four gates
  const int u = u0 + 4 * (lane >> 4);
  const size_t cd = (size_t)d * B * H;                 // direction offset inside a [2][B][H] state
  const float* cprev = first ? (a.c0 ? a.c0 + cd : nullptr)
                             : a.c + (a.train ? (size_t)tp * 2 * B * H : 0) + cd;
  float* cout = a.c + (a.train ? (size_t)t * 2 * B * H : 0) + cd;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int b = b0 + 16 * m + (lane & 15);
    if (b >= B) continue;
    if constexpr (LENS) {
      if (!valid[m]) {               // padded frame: h = +0, c = 0, pre not read, gates not written
        *(f32x4*)(cout + (size_t)b * H + u) = f32x4{0.f, 0.f, 0.f, 0.f};
        *(short4v*)(a.out + ((size_t)t * B + b) * 2 * H + (size_t)d * H + u) = short4v{0, 0, 0, 0};
        continue;
      }
    }
    const size_t grow = ((size_t)(t * 2 + d) * B + b) * 4 * H + u;
    f32x4 gt[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) gt[g] = ldf4(a.pre + grow + (size_t)g * H) + acc[m][g];
    f32x4 cp = {0.f, 0.f, 0.f, 0.f};
    if (cprev) cp = ldf4(cprev + (size_t)b * H + u);
    f32x4 ct, ht;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gt[0][r] = sigm(gt[0][r]);
      gt[1][r] = sigm(gt[1][r]);
      gt[2][r] = tanhf(gt[2][r]);
      gt[3][r] = sigm(gt[3][r]);
      ct[r] = gt[1][r] * cp[r] + gt[0][r] * gt[2][r];
      ht[r] = gt[3][r] * tanhf(ct[r]);
    }
    *(f32x4*)(cout + (size_t)b * H + u) = ct;
    stb4(a.out + ((size_t)t * B + b) * 2 * H + (size_t)d * H + u, ht);
    if (a.train) {
#pragma unroll
      for (int g = 0; g < 4; ++g) stb4(a.gates + grow + (size_t)g * H, gt[g]);
    }
  }
}

template <int MB, bool LENS>
__global__ __launch_bounds__(64) void lstm_step_bwd_kernel(LstmBwdArgs a) {
  const int lane = threadIdx.x, d = blockIdx.z;
  const int H = a.H, B = a.B;
  const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16 * MB;
  const int t = d ? a.s : a.T - 1 - a.s;
  const int tn = d ? t - 1 : t + 1;      // the step the previous launch wrote dG for
  const int tc = d ? t + 1 : t - 1;      // the step whose c is this step's c_prev
  const bool first = a.s == 0, last = a.s == a.T - 1;
  bool valid[MB], work = true;
  if constexpr (LENS) work = row_valid<MB>(a.lens, a.T, B, t, b0, lane, valid);

  f32x4 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (!first && work) {    // dh_rec = dG[tn] . W_hh, K = 4H over the rows of W_hh^T
    const int kq = 8 * (lane >> 4);
    const int K = 4 * H;
    const bf16* wrow = a.whhT + ((size_t)d * H + u0 + (lane & 15)) * K + kq;
    const bf16* grow[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
      grow[m] = a.dG + ((size_t)(tn * 2 + d) * B + min(b0 + 16 * m + (lane & 15), B - 1)) * K + kq;
    int k0 = 0;
    for (; k0 + 32 * BWD_U <= K; k0 += 32 * BWD_U) bwd_chunks<MB, BWD_U>(wrow + k0, grow, k0, acc);
    for (; k0 < K; k0 += 32) bwd_chunks<MB, 1>(wrow + k0, grow, k0, acc);
  }

  const int u = u0 + 4 * (lane >> 4);
  const size_t cd = (size_t)d * B * H;
  // the forward starts from a zero state and nothing flows into the last step from beyond it
  const float* cprev = last ? nullptr : a.c + (size_t)tc * 2 * B * H + cd;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int b = b0 + 16 * m + (lane & 15);
    if (b >= B) continue;
    if constexpr (LENS) {
      if (!valid[m]) {               // padded frame: dG[t] = 0, dc = 0, dout and gates not read
        bf16* z = a.dG + ((size_t)(t * 2 + d) * B + b) * 4 * H + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) *(short4v*)(z + (size_t)g * H) = short4v{0, 0, 0, 0};
        *(f32x4*)(a.dc + cd + (size_t)b * H + u) = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
    }
    const size_t grow = ((size_t)(t * 2 + d) * B + b) * 4 * H + u;
    const f32x4 dh = ldf4(a.dout + ((size_t)t * B + b) * 2 * H + (size_t)d * H + u) + acc[m];
    const f32x4 gi = ldb4(a.gates + grow), gf = ldb4(a.gates + grow + H),
                gg = ldb4(a.gates + grow + 2 * (size_t)H), go = ldb4(a.gates + grow + 3 * (size_t)H);
    const f32x4 ct = ldf4(a.c + (size_t)t * 2 * B * H + cd + (size_t)b * H + u);
    f32x4 cp = {0.f, 0.f, 0.f, 0.f}, dcn = {0.f, 0.f, 0.f, 0.f};
    if (cprev) cp = ldf4(cprev + (size_t)b * H + u);
    float* dcp = a.dc + cd + (size_t)b * H + u;
    if (!first) dcn = ldf4(dcp);
    f32x4 di, df, dg, dgo, dcprev;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float th = tanhf(ct[r]);
      const float dc = dcn[r] + dh[r] * go[r] * (1.f - th * th);
      dgo[r] = dh[r] * th * go[r] * (1.f - go[r]);
      di[r] = dc * gg[r] * gi[r] * (1.f - gi[r]);
      df[r] = dc * cp[r] * gf[r] * (1.f - gf[r]);
      dg[r] = dc * gi[r] * (1.f - gg[r] * gg[r]);
      dcprev[r] = dc * gf[r];
    }
    stb4(a.dG + grow, di);
    stb4(a.dG + grow + H, df);
    stb4(a.dG + grow + 2 * (size_t)H, dg);
    stb4(a.dG + grow + 3 * (size_t)H, dgo);
    *(f32x4*)dcp = dcprev;
  }
}

// 16-row batch tiles per wave.  Two reuse each weight fragment, one leaves twice the waves in
// flight, and the step is latency-bound until the waves cover the chip: one tile measured faster
// at B = 32 and two at B = 320 (H = 512, bench/lstm_step_probe.py, forward / backward us per
// step: B = 32 one 8.6 / 8.8, two 11.5 / 12.9; B = 320 one 18.7 / 25.1, two 17.6 / 23.7).
int tiles_per_wave(int B) {
#ifdef LSTM_TILES_PER_WAVE
  return LSTM_TILES_PER_WAVE;          // A/B builds only: 1 or 2
#endif
  return B > 128 ? 2 : 1;
}

void check_shape(const char* what, int T, int B, int H, int s) {
  if (H < 32 || H % 32 != 0)
    throw std::invalid_argument(std::string(what) + ": H must be a positive multiple of 32");
  if (B < 1 || T < 1) throw std::invalid_argument(std::string(what) + ": B and T must be >= 1");
  if (s < 0 || s >= T) throw std::invalid_argument(std::string(what) + ": step outside [0, T)");
  if ((B + 15) / 16 > 65535) throw std::invalid_argument(std::string(what) + ": B too large");
}

}  // namespace

void lstm_step_fwd_launch(const LstmFwdArgs& a, hipStream_t st) {
  check_shape("lstm_step_fwd", a.T, a.B, a.H, a.s);
  if (!a.pre || !a.whh || !a.out || !a.c || (a.train && !a.gates))
    throw std::invalid_argument("lstm_step_fwd: null operand");
  if (a.lens && (a.h0 || a.c0))
    throw std::invalid_argument("lstm_step_fwd: lens with h0 / c0 is not supported");
  const int mb = tiles_per_wave(a.B);
  const dim3 grid(a.H / 16, (a.B + 16 * mb - 1) / (16 * mb), 2);
  if (a.lens) {
    if (mb == 1) lstm_step_fwd_kernel<1, true><<<grid, 64, 0, st>>>(a);
    else lstm_step_fwd_kernel<2, true><<<grid, 64, 0, st>>>(a);
  } else {
    if (mb == 1) lstm_step_fwd_kernel<1, false><<<grid, 64, 0, st>>>(a);
    else lstm_step_fwd_kernel<2, false><<<grid, 64, 0, st>>>(a);
  }
  HIP_LAUNCH_CHECK();
}

void lstm_step_bwd_launch(const LstmBwdArgs& a, hipStream_t st) {
  check_shape("lstm_step_bwd", a.T, a.B, a.H, a.s);
  if (!a.dout || !a.gates || !a.c || !a.whhT || !a.dG || !a.dc)
    throw std::invalid_argument("lstm_step_bwd: null operand");
  const int mb = tiles_per_wave(a.B);
  const dim3 grid(a.H / 16, (a.B + 16 * mb - 1) / (16 * mb), 2);
  if (a.lens) {
    if (mb == 1) lstm_step_bwd_kernel<1, true><<<grid, 64, 0, st>>>(a);
    else lstm_step_bwd_kernel<2, true><<<grid, 64, 0, st>>>(a);
  } else {
    if (mb == 1) lstm_step_bwd_kernel<1, false><<<grid, 64, 0, st>>>(a);
    else lstm_step_bwd_kernel<2, false><<<grid, 64, 0, st>>>(a);
  }
  HIP_LAUNCH_CHECK();
}
