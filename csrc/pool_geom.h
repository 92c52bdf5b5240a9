// Device helpers shared by the pool-build kernels (importance.hip, pool_recipe.hip): which shard
// sample fills a pool slot, its Philox draws, the launch's zeroed slice, and the per-pixel
// geometry of the image recipes (PoolRecipeArgs).
#pragma once
#include "common.h"
#include "kernels.h"

// Which shard sample fills pool slot `slot` (epoch permutation, drop_last batches), and the
// global batch number gb that seeds its augmentation.
MA_DEV uint32_t pool_src(const PoolBuildArgs& a, int slot, int64_t& gb, int& t) {
  const int j = slot / a.batch;
  t = slot - j * a.batch;
  const int64_t pc = a.ctrl[0];
  const int per_pool = a.P / a.batch;
  const int nb = max(1, a.Ns / a.batch);
  gb = pc * per_pool + j;
  const uint32_t epoch = (uint32_t)(gb / nb);
  const int bi = (int)(gb % nb);
  // (% Ns only matters for a shard smaller than one batch: the batch cycles the shard)
  const uint32_t pos = (uint32_t)((bi * a.batch + t) % a.Ns);
  return a.shuffle ? permute_index(pos, (uint32_t)a.Ns, a.seed, epoch)
                   : (uint32_t)((gb * a.batch + t) % a.Ns);
}

// Stream words of the per-slot draws: the last counter word of pool_draw.
constexpr uint32_t DRAW_CROP = 0x5eedu;     // .x dy  .y dx  .z flip
constexpr uint32_t DRAW_AFFINE = 0x5eeeu;   // .x angle  .y scale  .z cut_y  .w cut_x
constexpr uint32_t DRAW_BOX = 0x5ef0u;      // + 0..4: two RandomResizedCrop box attempts each
constexpr uint32_t DRAW_BOX_AT = 0x5ef5u;   // .x top  .y left of the accepted box
constexpr uint32_t DRAW_COLOUR = 0x5ef8u;   // ColorJitter's four factors
constexpr uint32_t DRAW_ORDER = 0x5ef9u;    // .x ColorJitter's order code
constexpr uint32_t DRAW_SPEC = 0x5bec0u;    // + 0..2: pool_spec_kernel's shift, gain and masks

// Slot (gb, t)'s four random words of stream `word`.
MA_DEV u32x4 pool_draw(int64_t gb, int t, uint32_t word, uint32_t seed) {
  return philox4x32(u32x4{(uint32_t)gb, (uint32_t)(gb >> 32), (uint32_t)t, word}, seed,
                    0xA5A5A5A5u);
}

// The slot's label and shard index (one thread per slot calls this).
MA_DEV void pool_slot_header(const PoolBuildArgs& b, int slot, uint32_t src) {
  b.pool_label[slot] = (int)b.labels[src];
  b.pool_index[slot] = (int)src;
}

MA_DEV void zero_slice(const PoolBuildArgs& a) {
  for (int j = blockIdx.x * 256 + threadIdx.x; j < a.nzero; j += gridDim.x * 256) a.zero[j] = 0.f;
}

// Tap (y, x) of the cropped view, 0 <= y < H, 0 <= x < W: undo the flip, move into the padded
// resized image, zero in the padding; the resized image itself is torch's bilinear with
// align_corners=False over the uint8 source, every source index clamped into the image.
template <bool RESIZE>
MA_DEV void aug_tap(const PoolRecipeArgs& a, const uint8_t* img, int y, int x, int dy, int dx,
                    int flip, float ry, float rx, float v[3]) {
  const int xc = flip ? (a.b.W - 1 - x) : x;
  const int ys = y + dy - a.b.pad, xs = xc + dx - a.b.pad;
  v[0] = v[1] = v[2] = 0.f;
  if (ys < 0 || xs < 0 || ys >= a.Hr || xs >= a.Wr) return;
  if (!RESIZE) {               // (Hr, Wr) == (Hs, Ws), checked by the binding
    const uint8_t* p = img + ((size_t)ys * a.Ws + xs) * 3;
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
    return;
  }
  const float fy = fmaxf((ys + 0.5f) * ry - 0.5f, 0.f), fx = fmaxf((xs + 0.5f) * rx - 0.5f, 0.f);
  const int y0 = min((int)fy, a.Hs - 1), x0 = min((int)fx, a.Ws - 1);
  const int y1 = min(y0 + 1, a.Hs - 1), x1 = min(x0 + 1, a.Ws - 1);
  const float ly = fy - y0, lx = fx - x0;
  const uint8_t* p0 = img + (size_t)y0 * a.Ws * 3;
  const uint8_t* p1 = img + (size_t)y1 * a.Ws * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = p0[x0 * 3 + c] * (1.f - lx) + p0[x1 * 3 + c] * lx;
    const float bot = p1[x0 * 3 + c] * (1.f - lx) + p1[x1 * 3 + c] * lx;
    v[c] = top * (1.f - ly) + bot * ly;
  }
}

// Output pixel (i, j) of the Resize -> RandomCrop(pad) -> flip -> [RandomAffine] chain, in
// uint8 levels (0..255, float): with AFFINE, affine_grid + grid_sample (bilinear, zeros
// padding, align_corners=False) over aug_tap; cs, sn are cos / scale and sin / scale.
template <bool AFFINE, bool RESIZE>
MA_DEV void aug_pixel(const PoolRecipeArgs& a, const uint8_t* img, int H, int W, int i, int j,
                      int dy, int dx, int flip, float ry, float rx, float cs, float sn,
                      float v[3]) {
  if (AFFINE) {
    const float xn = (2 * j + 1) / (float)W - 1.f, yn = (2 * i + 1) / (float)H - 1.f;
    const float gx = cs * xn - sn * yn, gy = sn * xn + cs * yn;
    const float fx = ((gx + 1.f) * W - 1.f) * 0.5f, fy = ((gy + 1.f) * H - 1.f) * 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);   // (floorf: fx, fy can be negative)
    const float lx = fx - x0f, ly = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    v[0] = v[1] = v[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = y0 + (k >> 1), x = x0 + (k & 1);
      if (y < 0 || x < 0 || y >= H || x >= W) continue;
      const float wt = ((k >> 1) ? ly : 1.f - ly) * ((k & 1) ? lx : 1.f - lx);
      float tv[3];
      aug_tap<RESIZE>(a, img, y, x, dy, dx, flip, ry, rx, tv);
      v[0] += wt * tv[0];
      v[1] += wt * tv[1];
      v[2] += wt * tv[2];
    }
  } else {
    aug_tap<RESIZE>(a, img, i, j, dy, dx, flip, ry, rx, v);
  }
}
