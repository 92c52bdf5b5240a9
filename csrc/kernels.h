// Host-visible argument blocks + launchers for the non-GEMM kernels.
// Every launcher is stream-ordered, allocation-free and graph-capturable.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "igemm.h"

// ------------------------------------------------------------------ batch norm
struct BnApplyArgs {
  const bf16* y;
  const float* stats;            // [G][2][C]
  const float* gamma;
  const float* beta;
  const float* rmean;            // eval mode
  const float* rvar;
  int use_running;
  int res_mode;                  // 0 none, 1 identity (+res), 2 BN'd shortcut (+bn2(res))
  const bf16* res;
  const float* stats2;
  const float* gamma2;
  const float* beta2;
  const float* rmean2;
  const float* rvar2;
  bf16* out;
  int M, C, group_rows, act;     // act: 0 none, 1 relu, 2 relu6
  float eps;
};
void bn_apply_launch(const BnApplyArgs& a, hipStream_t st);
void bn_configure(long long nt_min_bytes);

struct BnBwdArgs {
  const bf16* dout;              // grad of the activation output
  const bf16* out;               // activation output (mask)
  const bf16* y;                 // conv output (pre-BN)
  const float* stats;            // [2][C]
  const float* gamma;
  const bf16* y2;                // optional shortcut conv output sharing dz
  const float* stats2;
  const float* gamma2;
  float* sums;                   // workspace [SUMS_R][3][C] (replicas, igemm.h SUMS_R)
  bf16* dy;                      // grad wrt y
  bf16* dy2;                     // grad wrt y2
  bf16* dz;                      // optional: grad wrt pre-activation (identity residual)
  float* dgamma;
  float* dbeta;
  float* dgamma2;
  float* dbeta2;
  int M, C, act;
  float eps;
  int phases;                    // 1 reduce, 2 apply, 3 both (reduce fused upstream -> 2)
};
void bn_bwd_launch(const BnBwdArgs& a, hipStream_t st);

struct BnRunEntry {
  float* rmean;
  float* rvar;
  const float* stats_train;      // [n_train][2][C]
  const float* stats_score;      // [n_score][2][C]
  long long* nbt;                // num_batches_tracked (int64) or null
  int C, n_train, n_score;
  float cnt_train, cnt_score;
};
void bn_running_launch(const BnRunEntry* tab, int nlayers, int maxC, float momentum,
                       hipStream_t st);

// ------------------------------------------------------------------ head (pool + fc + loss)
struct HeadArgs {
  const bf16* act;               // [B][HW][C] final activation
  const float* w;                // fc weight [classes][C] (fp32 master)
  const float* b;                // fc bias [classes]
  const int* label;              // [B]
  const float* isw;              // [B] importance weights N*p (train) or null (score / uniform)
  float* pooled;                 // [B][C] workspace (saved for backward)
  float* logits;                 // [B][classes] workspace
  float* dlogits;                // [B][classes] (train) or null
  float* losses;                 // [B] per-sample CE (score) or null
  float* meters;                 // [0]+=sum(w-loss)*... see head.hip
  int B, HW, C, classes, mode;   // mode 0 score, 1 train, 2 eval
  int log_softmax_input;         // logits are already log-probs (VGG) -> NLL
  int score_kind;                // losses[] holds 0: CE loss, 1: classifier-layer grad norm
  int logits_ready;              // (set by head_fwd_launch) pooled/logits already computed
  // final BatchNorm (+ identity residual) + activation applied while pooling (scoring / eval:
  // nothing else reads the last block's output): act is then the raw conv output y and
  // pooled = mean_hw(act(bn(y) [+ bn_res])) -- no bn_apply pass over the last activation
  const bf16* bn_res = nullptr;  // [B][HW][C] identity residual or null
  const float* bn_stats = nullptr;   // [G][2][C] ghost-group sums (or null: running stats)
  const float* bn_rmean = nullptr;
  const float* bn_rvar = nullptr;
  const float* bn_gamma = nullptr;   // non-null: the BN prologue is on
  const float* bn_beta = nullptr;
  float bn_inv_count = 0.f;
  float bn_eps = 0.f;
  int bn_group_imgs = 1;
  int bn_act = 0;                // 0 none, 1 relu, 2 relu6
  int pooled_ready = 0;          // (set by head_fwd_launch) pooled[] already written
  // train mode only: F.cross_entropy's label_smoothing in [0, 1) -- dlogits and meters[0] are the
  // smoothed loss's; losses[] (and score / eval mode as a whole) stay plain CE
  float smooth = 0.f;
  // train / eval: k >= 1 adds the samples whose label ranks below k (lower index wins a tie, so
  // k = 1 is the argmax count) to meters[5]; 0 = off
  int topk = 0;
};
// throws std::invalid_argument: smooth outside [0, 1) or non-zero outside train mode, topk
// outside [0, classes] (the launchers call it before they enqueue anything)
void head_check_extras(const HeadArgs& a, const char* who);
void head_fwd_launch(const HeadArgs& a, hipStream_t st);
void head_loss_launch(const HeadArgs& a, hipStream_t st);

struct HeadBwdArgs {
  const float* pooled;           // [B][C]
  const float* dlogits;          // [B][classes]
  const float* w;                // [classes][C]
  float* dw;                     // [classes][C] fp32 grad
  float* db;                     // [classes]
  bf16* dact;                    // [B][HW][C] grad of final activation
  int B, HW, C, classes;
  // optional: also reduce the BN-backward sums of the final BN (+ shortcut BN) whose activation
  // the head read -- as a dgrad epilogue does (EpiParams bw_*): dz = dact * act'(bw_out),
  // sums[0] += dz, [1] += dz * xhat(bw_y), [2] += dz * xhat(bw_y2); [SUMS_R][3][C] replicas
  const bf16* bw_out = nullptr;
  const bf16* bw_y = nullptr;
  const float* bw_stats = nullptr;
  const bf16* bw_y2 = nullptr;
  const float* bw_stats2 = nullptr;
  float* bw_sums = nullptr;
  float bw_inv_count = 0.f, bw_eps = 0.f;
  int bw_act = 0;
};
void mlp_head_fwd_launch(const bf16* x, const bf16* w1, const float* b1, const float* w2,
                         const float* b2, float* h1, float* logits, int B, int F, int H1, int K,
                         int splits, hipStream_t st);
void mlp_head_bwd_launch(const float* dlogits, const float* h1, const bf16* x, const bf16* w1,
                         const float* w2, float* dh1, float* dw1, float* db1, float* dw2,
                         float* db2, bf16* dx, int B, int F, int H1, int K, hipStream_t st);
// returns 1 when the BN-backward sums (a.bw_sums) were reduced (the per-sample path)
int head_bwd_launch(const HeadBwdArgs& a, hipStream_t st);

// ------------------------------------------------------------------ importance sampling
struct PoolBuildArgs {
  const uint8_t* shard;          // [Ns][H][W][3] uint8 HWC
  const int64_t* labels;         // [Ns]
  const int64_t* ctrl;           // [0] pool counter (pools built so far)
  bf16* pool;                    // [P][H][W][8] bf16 normalised, channels 3..7 zero
  int* pool_label;               // [P]
  int* pool_index;               // [P] shard-local index (the dataset index the reference returns)
  int Ns, H, W, P, batch, pad, flip, augment, shuffle;
  uint32_t seed;
  float mean[3], inv_std[3];
  int prebuilt;                  // shard is already NHWC bf16 [Ns][H][W][8]: plain gather
  float* zero;                   // optional buffer zeroed by the launch (the pass's BN stats)
  int nzero;
};
void pool_build_launch(const PoolBuildArgs& a, hipStream_t st);

// Image recipe (AugmentRecipe, mercury_amd/data/augment.py; pool_recipe.hip): geometry -> flip ->
// [ColorJitter] -> /255 -> Normalize -> Cutout, evaluated per output pixel in fp32 with no
// rounding between the stages.  The geometry is Resize -> RandomCrop(pad) -> RandomAffine
// (rotation, isotropic scale; bilinear, zeros outside) or RandomResizedCrop (a drawn box of the
// source, bilinear to b.H x b.W, no antialiasing).
struct PoolRecipeArgs {
  PoolBuildArgs b;               // b.shard is [Ns][Hs][Ws][3]; b.H, b.W are the OUTPUT size
  int Hs, Ws;                    // source image size
  int resize;                    // 0: off (Hr, Wr = Hs, Ws); else the shorter side's new length
  int Hr, Wr;                    // size the crop is taken from (transforms.Resize's formula)
  float degrees;                 // rotation drawn from [-degrees, degrees)
  float scale_lo, scale_hi;      // isotropic scale drawn from [lo, hi) (lo = hi = 1: unset)
  int cutout;                    // side of the zeroed square (0: off)
  int affine;                    // rotation / scale stage on
  int rrc;                       // RandomResizedCrop replaces Resize / RandomCrop / RandomAffine:
                                 // b.pad = 0, no resize, no affine, (Hr, Wr) = (Hs, Ws)
  float area_lo, area_hi;        // box area as a fraction of the source, drawn from [lo, hi)
  float ratio_lo, ratio_hi;      // box aspect w / h, log-uniform in [lo, hi)
  float log_ratio_lo, log_ratio_hi;
  float jitter[4];               // brightness, contrast, saturation, hue strengths (0: off)
  float* params;                 // optional [P][8]: dy, dx, flip, angle_deg, scale, cut_y, cut_x, 0
                                 // (rrc: top, left, flip, 0, 1, cut_y, cut_x, attempt); with rrc
                                 // or jitter [P][16]: then box h, w, fb, fc, fs, fh, order code,
                                 // grey mean used by contrast.  The row length is a constant of
                                 // the instantiation the launcher picks from rrc and jitter.
};
void pool_recipe_launch(const PoolRecipeArgs& p, hipStream_t st);

// Spectrogram recipe (mercury_amd/data/augment.py, SpecRecipe): time shift -> gain -> frequency
// and time masks in output coordinates, from a PLANAR bf16 shard to the NHWC8 pool.
struct PoolSpecArgs {
  PoolBuildArgs b;               // b.shard is bf16 [Ns][C][H][W]; b.H frequency rows, b.W frames
  int C;                         // stored channels, 1..8 (pool channels C..7 are +0)
  int shift;                     // time shift drawn from [-shift, shift]
  int fmask_n, fmask_max;        // frequency masks: how many (0..2), widths drawn from [0, max]
  int tmask_n, tmask_max;        // time masks likewise
  float gain_lo, gain_hi;        // gain drawn from [lo, hi) (lo = hi = 1: unset, exactly 1.0f)
  float fill;                    // value of masked / shifted-in pixels (rounded to bf16 once)
  float* params;                 // optional [P][12]: shift, gain, f0a, fwa, f0b, fwb, t0a, twa,
                                 //                   t0b, twb, 0, 0
  int chunks;                    // blocks per slot (grid.y); 0: the launcher's choice
};
void pool_spec_launch(const PoolSpecArgs& a, hipStream_t st);

struct IsSampleArgs {
  const float* losses;           // [P]
  float* ema;                    // [0] value, [1] initialised flag (device-resident EMAverage)
  int64_t* ctrl;                 // [0] pool counter (incremented), [1] draw counter
  int* idx;                      // [B] drawn pool slots
  float* w;                      // [B] N * p[idx]
  float* meters;                 // [3] pool mean out, [4] ema out
  int P, B, group, importance;   // importance=0 -> uniform draws, w = 1
  float alpha, ema_alpha;
  uint32_t seed;
  int alias;                     // 1: Walker alias table in LDS + O(1) draws; 0: inverse CDF
  const float* gl;               // [W][P] all ranks' pool scores (global EMA) or null
  int W;
};
void is_sample_launch(const IsSampleArgs& a, hipStream_t st);
size_t is_sample_lds(int P, int alias);   // dynamic LDS bytes (<= 128 KB: alias up to P ~ 4k)

struct GatherArgs {
  const bf16* pool;              // [P][pix*8]
  const int* pool_label;
  const int* pool_index;
  const int* idx;                // [B]
  bf16* batch;                   // [B][pix*8]
  int* batch_label;
  int* batch_index;
  int B, chunks_per_img;         // 16-byte chunks per image
};
void gather_launch(const GatherArgs& a, hipStream_t st);

// global importance table in HBM (Groupwise sampler, K2/K11) -- csrc/table.hip
struct TableScatterArgs {
  float* imp;                    // [N] importance
  int* grp;                      // [N] group stamp
  const float* losses;           // [n]
  const int* index;              // [n] table positions, or null -> start + i
  const int64_t* stamp;          // device group id (graph-replay safe) or null -> gi
  int start, n, N, gi;
};
void table_scatter_launch(const TableScatterArgs& a, hipStream_t st);

struct TableScalars {
  float mean, count;             // group mean importance, member count
  double total;                  // sum of w = imp + mean over members
  int64_t counter;               // draw-counter snapshot used by this batch of draws
};
struct TableSampleArgs {
  const float* imp;
  const int* grp;
  int N, gi;
  const int64_t* gi_dev;         // device group id or null -> gi
  float2* part;                  // workspace [table_num_segments(N)]
  double* prefix;                // workspace [table_num_segments(N) + 1]
  TableScalars* sc;              // workspace / result scalars
  int64_t* counter;              // device draw counter (bumped once per launch) or null
  int ndraw;
  uint32_t seed;
  int64_t* out;                  // [ndraw] drawn table positions (int64) or null
  int* out32;                    // [ndraw] same as int32 or null
};
int table_num_segments(int N);
void table_sample_launch(const TableSampleArgs& a, hipStream_t st);
void table_weights_launch(const int* pos, int ndraw, const float* imp, const void* sc,
                          const int* pool_index, int Ns, int P, int* idx, float* isw,
                          float* meters, hipStream_t st);

// ------------------------------------------------------------------ optimizer
struct OptSeg {
  long long off;                 // element offset in the flat buffer (multiple of 4)
  int numel;
  int kind;                      // 0 plain, 1 conv weight (also write bf16 copies)
  int K, R, S, C, Cpad;
  bf16* w_krsc;                  // [K][R][S][Cpad] bf16 (forward / wgrad)
  bf16* w_crsk;                  // [C][R][S][K] bf16 (dgrad) or null
};
struct OptArgs {
  float* p;
  float* g;
  float* m;
  float* v;
  const OptSeg* segs;
  int nsegs;
  long long total;               // end of the swept range (padded flat length for a full step)
  const float* hyper;            // device: [0] lr [1] beta1 [2] beta2 [3] eps [4] wd
  const int64_t* step;           // device step counter (t, already incremented)
  int algo;                      // 0 adam (L2 in the gradient), 1 sgd(momentum), 2 adamw
  int zero_grad;
  long long start;               // first element of the swept range (4-aligned segment start)
  const float* gscale;           // device clip coefficient the gradient is multiplied by before
                                 // weight decay (grad_norm_launch's record[1]); null: no clipping
};
// L2 norm of g[0, n) and the clip coefficient min(1, *max_norm / (norm + 1e-6)) into
// rec[0], rec[1] (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False).  Two launches on
// `st`: per-block fp32 partial sums of squares into ws[0, plan.blocks), then one block that
// combines them in fp64.  Fixed summation order, no atomics: bit-equal from run to run.
// Throws std::invalid_argument (grad_norm_plan.h grad_norm_check); allocates and syncs nothing.
void grad_norm_launch(const float* g, long long n, const float* max_norm, float* rec, float* ws,
                      long long ws_floats, hipStream_t st);
void optimizer_launch(const OptArgs& a, hipStream_t st);
// full step in one launch: tile jobs (conv segments with a dgrad copy, C % 4 == 0) write both
// bf16 copies; ew ([n][2] start, numel) / ewp ([n+1] float4 prefix) cover everything else
void optimizer_fused_launch(const OptArgs& a, const int* jobs, int njobs, const long long* ew,
                            const long long* ewp, int new_, long long ew4, hipStream_t st);
void step_begin_launch(int64_t* ctrl, float* z0, int n0, float* z1, int n1, hipStream_t st);
// jobs: [njobs][4] = (segment index, r*S+s, k0, c0) -> one 64x64 tile each
void transpose_weights_launch(const OptSeg* segs, const int* jobs, int njobs, hipStream_t st);
void pack_weights_launch(const float* p, const OptSeg* segs, int nsegs, long long total,
                         hipStream_t st);

// ------------------------------------------------------------------ misc
void quantize_launch(const float* x, float* out, float* absmax_ws, long long n, uint32_t seed,
                     uint64_t counter, hipStream_t st);
void tern_pack_launch(const float* x, long long n, float* absmax_ws, uint32_t seed,
                      uint64_t counter, const long long* dctr, uint32_t* words, hipStream_t st);
void tern_unpack_launch(const uint32_t* msgs, int W, long long n, float scale, float* out,
                        hipStream_t st);
struct PoolArgs {                 // max-pool / avg-pool NHWC bf16
  const bf16* x;
  bf16* y;
  uint8_t* argmax;               // [N*P*Q*C] window tap r*k+s of the max, for backward, or null
  int N, H, W, C, P, Q, k, stride, pad, is_max;
  // optional BN (+ activation) of x applied per tap before pooling: x is then the raw conv
  // output, normalised from ghost-group sums ``stats`` [G][2][C] (G = N / group_imgs) or from
  // running statistics (rmean/rvar) -- the scoring pass's ImageNet stem, no bn_apply pass
  const float* stats;
  const float* gamma;
  const float* beta;
  const float* rmean;
  const float* rvar;
  int group_imgs, act;
  float eps;
};
void pool2d_fwd_launch(const PoolArgs& a, hipStream_t st);
void maxpool2d_bwd_launch(const PoolArgs& geom, const bf16* dy, bf16* dx, hipStream_t st);
struct DwArgs {                   // depthwise 3x3 conv NHWC bf16
  const bf16* x;
  const float* w;                // [C][3][3] fp32 master
  bf16* y;
  float* stats;                  // BN sums [G][2][C] or null
  int N, H, W, C, P, Q, stride, pad, group_rows;
  // input prologue (pro_gamma != null): x is the producer's raw output, act(bn(x)) is applied
  // to every loaded input chunk (padding stays zero); keep (optional) receives the activation,
  // each element written once by the thread whose strip owns it
  const float* pro_stats;        // [G][2][C] producer sums, or null -> running statistics
  const float* pro_rmean;
  const float* pro_rvar;
  const float* pro_gamma;
  const float* pro_beta;
  bf16* keep;
  float pro_inv_count, pro_eps;
  int pro_act, pro_group_imgs;
};
void dwconv_fwd_launch(const DwArgs& a, hipStream_t st);
struct StemArgs {                 // first conv: <= 4 input channels packed densely into k (stem.hip)
  const bf16* x;                  // [N][H][W][8] (channels >= C zero)
  const bf16* w;                  // [K][R][R][8] bf16 weights (channels >= C zero)
  const float* bias;              // [K] or null
  bf16* y;                        // [N][P][Q][K]
  float* stats;                   // BN sums [G][2][K] or null
  int N, H, W, K, R, stride, pad, P, Q, group_imgs;
  int tpb, blocks_per_img;        // set by the launcher
};
int stem_fwd_launch(StemArgs a, hipStream_t st);
struct DwBw {                      // BN-backward reduce fused into the depthwise dgrad
  const bf16* out;                 // activation act(bn(y)) of the BN feeding the dw conv (mask)
  const bf16* y;                   // that BN's input
  const float* stats;              // its batch sums [2][C]
  float* sums;                     // += (sum dz, sum dz * xhat) [SUMS_R][3][C] (zeroed)
  float inv_count, eps;
  int act;
};
// The dw conv's OUTPUT BatchNorm backward applied to dy as it is loaded (no bn_bwd_apply pass,
// no materialised dy): dy = A * dz + B * y + Cc per channel, dz = dout * act'(out), with
//   A = gamma * rstd, B = -A * rstd * mean(dz*xhat), Cc = A * (rstd * mean * mean(dz*xhat) -
//   mean(dz)) -- bn.hip bn_bwd_apply's arithmetic rearranged; the sums come complete from the
// producing dgrad's epilogue.  Block 0 writes that BN's dgamma / dbeta.
void dwconv_dgrad_launch(const bf16* dy, const float* w, bf16* dx, int N, int H, int W, int C,
                         int P, int Q, int stride, int pad, hipStream_t st,
                         const DwBw* bw = nullptr);
// slab (optional, >= dwconv_wgrad_slab_floats): per-block partials + a reduce kernel
size_t dwconv_wgrad_slab_floats(int N, int P, int Q, int C);
// dgrad (+ fused BN-backward sums bw) and slab wgrad of a depthwise conv in one launch; the
// partials reduce follows unless ``reduce`` is false (then dwconv_wgrad_reduce_batch_launch
// sums this layer's slab later, e.g. once for every layer at the end of the backward)
constexpr int DW_RED_MAX = 24;
int dwconv_wgrad_blocks(int N, int P, int Q, int C);
void dwconv_bwd_launch(const bf16* dy, const bf16* x, const float* w, bf16* dx, float* dw, int N,
                       int H, int W, int C, int P, int Q, int stride, int pad, float* slab,
                       const DwBw* bw, bool reduce, hipStream_t st);
void dwconv_wgrad_reduce_batch_launch(const float* const* slabs, float* const* dws, const int* Cs,
                                      const int* nblks, int n, hipStream_t st);
void dwconv_wgrad_launch(const bf16* dy, const bf16* x, float* dw, int N, int H, int W, int C,
                         int P, int Q, int stride, int pad, hipStream_t st, float* slab = nullptr,
                         size_t slab_floats = 0);
void nchw_to_nhwc8_launch(const float* x, bf16* y, int N, int C, int H, int W, int Cpad,
                          hipStream_t st);
// bidirectional LSTM recurrence, one launch per time step, both directions per launch (lstm.hip).
// Step s handles t = s for direction 0 and t = T-1-s for direction 1 (the backward walks the
// other way: t = T-1-s and t = s).
struct LstmFwdArgs {
  const float* pre;               // [T][2][B][4H] x . W_ih^T + b_ih + b_hh, gates i, f, g, o
  const bf16* whh;                // [2][4H][H]
  bf16* out;                      // [T][B][2H]; h_t at column dir*H, read back as the next h_prev
  float* c;                       // train: [T][2][B][H] every c_t; else [2][B][H], updated in place
  bf16* gates;                    // train: [T][2][B][4H] post-activation gates; else null
  const bf16* h0;                 // [2][B][H] initial state, or null = zero
  const float* c0;                // [2][B][H], or null = zero
  int T, B, H, s, train;
  const int* lens = nullptr;      // [B] or null: frame (t, b) is valid iff t < clamp(lens[b], 0, T);
                                  // padded frames get h = +0 and c = 0.  Not with h0 / c0.
};
void lstm_step_fwd_launch(const LstmFwdArgs& a, hipStream_t st);
struct LstmBwdArgs {                // of a forward that started from a zero state
  const float* dout;              // [T][B][2H] upstream gradient of out
  const bf16* gates;              // saved by the forward
  const float* c;                 // [T][2][B][H] saved by the forward
  const bf16* whhT;               // [2][H][4H] = W_hh transposed
  bf16* dG;                       // [T][2][B][4H] pre-activation gradients; step s reads step s-1's
  float* dc;                      // [2][B][H] dc_next in, dc_prev out (in place); step 0 reads zero
  int T, B, H, s;
  const int* lens = nullptr;      // as the forward's; padded frames get dG[t] = 0 and dc = 0
};
void lstm_step_bwd_launch(const LstmBwdArgs& a, hipStream_t st);
// attention pooling over time (attn.hip): s = x . w, a = masked softmax_t(relu(s)),
// rep = sum_t a x.  x / dx are addressed by element strides for t and b with the D row
// contiguous; a block of ATTN_BLOCK_WAVES waves takes one batch row and that many shares of
// T (attn_pool_split) and leaves one partial; a second launch merges the partials in order.
constexpr int ATTN_WAVE_FRAMES = 8;     // smallest share of T one wave walks
constexpr int ATTN_BLOCK_WAVES = 4;
constexpr int ATTN_MAX_SPLITS = 32;     // most wave shares T is cut into
constexpr int ATTN_TARGET_WAVES = 2048; // T is cut until B * shares reaches this
constexpr int ATTN_MAX_D = 2048;
// share: frames per wave; nsb: blocks (partials) per batch row
void attn_pool_split(int T, int B, int* share, int* nsb);
struct AttnFwdArgs {
  const void* x;                  // fp32 or bf16 (bf16_x), element (t, b) at x + t*st + b*sb
  const float* w;                 // [D]
  const int* lengths;             // [B], clamped to [0, T] here; null = T
  float* rep;                     // [B][D]
  float* attn;                    // [B][T]
  float* score;                   // [B][T] s before the relu (training), or null
  float* ws;                      // >= B * nsb * (D + 2) floats
  long long ws_floats;
  long long st, sb;
  int T, B, D, bf16_x;
};
void attn_pool_fwd_launch(const AttnFwdArgs& a, hipStream_t st);
struct AttnBwdArgs {
  const void* x;                  // as the forward read it
  const float* w;                 // [D]
  const float* g;                 // [B][D] upstream gradient of rep
  const float* rep;               // [B][D] forward output: c_b = g_b . rep_b
  const float* attn;              // [B][T] forward output
  const float* score;             // [B][T] saved s: ds is zero where s <= 0
  const int* lengths;             // as the forward's
  void* dx;                       // x's dtype, element (t, b) at dx + t*dst + b*dsb; every frame
                                  // is written, frames past the length with zeros
  float* dw;                      // [D]
  float* ws;                      // >= B * nsb * D floats: per-block partials of dw
  long long ws_floats;
  long long st, sb, dst, dsb;
  int T, B, D, bf16_x;
};
void attn_pool_bwd_launch(const AttnBwdArgs& a, hipStream_t st);
