// Image augmentation recipes on the GPU (PoolRecipeArgs; every AugmentRecipe,
// mercury_amd/data/augment.py, that does not take pool_build_kernel): one block per pool slot
// builds
//
//     geometry -> [flip] -> [ColorJitter] -> /255 -> [Normalize] -> [Cutout]
//
// per output pixel from the HBM-resident uint8 shard into the NHWC8 bf16 pool, fp32 between the
// stages.  The geometry is the Resize -> RandomCrop(pad) -> [RandomAffine] chain (pool_geom.h)
// or RandomResizedCrop.  The crop / flip draw is pool_build_kernel's (importance.hip) word for
// word: a crop-and-flip recipe on a shard of the output size gives the same bits from either
// kernel.
//
// Draws per slot: Philox on the counter (gb, t) (pool_draw).  Stream word 0x5eed holds dy, dx,
// flip and 0x5eee angle, scale, cut_y, cut_x -- flip is r.z & 1 of the 0x5eed call for both
// geometries.  The photographic recipes (`rrc`, `jitter`) add:
//   0x5ef0..0x5ef4: the box attempts, two per call: attempt 2k   takes .x (area) and .y (aspect),
//                                                   attempt 2k+1 takes .z (area) and .w (aspect)
//                   of word 0x5ef0 + k
//   0x5ef5:         .x top, .y left of the accepted box
//   0x5ef8:         .x fb  .y fc  .z fs  .w fh   (brightness, contrast, saturation, hue factors)
//   0x5ef9:         .x order code = x % 24
// Box (torchvision RandomResizedCrop.get_params): target = Hs*Ws * (slo + (shi - slo) * u),
// aspect = exp(log rlo + (log rhi - log rlo) * u'), w = rint(sqrt(target * aspect)),
// h = rint(sqrt(target / aspect)); the first of ten attempts with 1 <= w <= Ws, 1 <= h <= Hs is
// taken, top = x % (Hs - h + 1), left = y % (Ws - w + 1); else (attempt 10) the whole image
// clipped to the ratio range, centred.  augment = 0 takes that fallback box, and the identity
// factors (1, 1, 1, 0) in order 0.
// Output pixel (i, j): fy = max((i + .5) * h / H - .5, 0), rows y0 = min(floor(fy), h - 1) and
// min(y0 + 1, h - 1) RELATIVE TO THE BOX (indices clamp at the box edge), columns likewise from
// jx = flip ? W - 1 - j : j; the four taps are read at (top + y, left + x).
//
// ColorJitter (torchvision's tensor path on [0, 1] values): the order code is the Lehmer code of
// the order of (0 brightness, 1 contrast, 2 saturation, 3 hue): from the list [0, 1, 2, 3] take
// element code / 6, then element (code % 6) / 2 of the rest, then element code % 2, then what is
// left; code 0 is brightness, contrast, saturation, hue.  An operation of strength 0 is skipped
// in place.  Contrast needs the mean grey level of the slot's image as it stands at that point:
// a first sweep evaluates geometry and the operations before contrast and sums the grey level
// (per thread in pixel order px = tid, tid + 256, ...; then the xor-shuffle tree of wave_sum and
// the four wave totals added in wave order: no atomics, the same bits every run), a second
// sweep recomputes and finishes.  Without contrast there is one sweep.
#include "common.h"
#include "kernels.h"
#include "pool_geom.h"

namespace {

constexpr int OP_BRIGHT = 0, OP_CONTRAST = 1, OP_SAT = 2, OP_HUE = 3, OP_SKIP = 4;

MA_DEV float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
MA_DEV float grey(const float x[3]) { return 0.299f * x[0] + 0.587f * x[1] + 0.114f * x[2]; }
MA_DEV float uni_f(float x) {      // a block-uniform value read from LDS, into an SGPR
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// adjust_hue: RGB -> HSV, h <- (h + fh) mod 1, HSV -> RGB (torchvision _rgb2hsv / _hsv2rgb)
MA_DEV void hue_shift(float x[3], float fh) {
  const float r = x[0], g = x[1], b = x[2];
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const float cr = maxc - minc;
  const bool eq = cr == 0.f;
  const float s = cr * __builtin_amdgcn_rcpf(eq ? 1.f : maxc);
  const float icr = __builtin_amdgcn_rcpf(eq ? 1.f : cr);
  const float rc = (maxc - r) * icr, gc = (maxc - g) * icr, bc = (maxc - b) * icr;
  float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
  h = h * (1.f / 6.f) + 1.f;
  h -= floorf(h);
  h += fh;
  h -= floorf(h);
  const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
  int i = (int)fi;
  if (i >= 6) i -= 6;                       // (h can round up to 1.0)
  const float v = maxc;
  const float p = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - f * s));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  x[0] = (i == 0 || i == 5) ? v : i == 1 ? q : (i == 2 || i == 3) ? p : t;
  x[1] = (i == 1 || i == 2) ? v : i == 3 ? q : (i == 4 || i == 5) ? p : t;
  x[2] = (i == 3 || i == 4) ? v : i == 5 ? q : (i == 0 || i == 1) ? p : t;
}

// The slot's colour operations on one [0, 1] pixel, in the order `seq` holds (one nibble per
// position).  UNTIL_CONTRAST: stop in front of contrast (the first sweep).
template <bool UNTIL_CONTRAST>
MA_DEV void jitter_pixel(float x[3], int seq, const float f[4], float m) {
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int op = (seq >> (4 * k)) & 15;       // uniform: scalar branches
    if (op == OP_BRIGHT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp01(x[c] * f[0]);
    } else if (op == OP_CONTRAST) {
      if (UNTIL_CONTRAST) return;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp01(f[1] * x[c] + (1.f - f[1]) * m);
    } else if (op == OP_SAT) {
      const float gr = grey(x);
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp01(f[2] * x[c] + (1.f - f[2]) * gr);
    } else if (op == OP_HUE) {
      hue_shift(x, f[3]);
    }
  }
}

struct PhotoBox {
  int top, left, h, w;
};

// One tap set of the resized box, in uint8 levels (header comment).
MA_DEV void rrc_pixel(const uint8_t* img, int Ws, const PhotoBox& bx, int i, int jx, float ry,
                      float rx, float v[3]) {
  const float fy = fmaxf((i + 0.5f) * ry - 0.5f, 0.f), fx = fmaxf((jx + 0.5f) * rx - 0.5f, 0.f);
  const int y0 = min((int)fy, bx.h - 1), x0 = min((int)fx, bx.w - 1);
  const int y1 = min(y0 + 1, bx.h - 1), x1 = min(x0 + 1, bx.w - 1);
  const float ly = fy - y0, lx = fx - x0;
  const uint8_t* p0 = img + ((size_t)(bx.top + y0) * Ws + bx.left) * 3;
  const uint8_t* p1 = img + ((size_t)(bx.top + y1) * Ws + bx.left) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = p0[x0 * 3 + c] * (1.f - lx) + p0[x1 * 3 + c] * lx;
    const float bot = p1[x0 * 3 + c] * (1.f - lx) + p1[x1 * 3 + c] * lx;
    v[c] = top * (1.f - ly) + bot * ly;
  }
}

// The slot's box, by one thread (header comment).  Returns the accepted attempt, 10: fallback.
MA_DEV int rrc_box(const PoolRecipeArgs& p, int64_t gb, int t, PhotoBox& bx) {
  const PoolBuildArgs& b = p.b;
  const int Hs = p.Hs, Ws = p.Ws;
  if (b.augment) {
    const float area = (float)Hs * (float)Ws;
    for (int k = 0; k < 5; ++k) {
      const u32x4 r = pool_draw(gb, t, DRAW_BOX + (uint32_t)k, b.seed);
      for (int e = 0; e < 2; ++e) {
        const float target = area * (p.area_lo + (p.area_hi - p.area_lo) * u01(e ? r.z : r.x));
        const float aspect = expf(p.log_ratio_lo +
                                  (p.log_ratio_hi - p.log_ratio_lo) * u01(e ? r.w : r.y));
        const float w = rintf(sqrtf(target * aspect)), h = rintf(sqrtf(target / aspect));
        if (w >= 1.f && w <= (float)Ws && h >= 1.f && h <= (float)Hs) {
          const u32x4 q = pool_draw(gb, t, DRAW_BOX_AT, b.seed);
          bx.h = (int)h;
          bx.w = (int)w;
          bx.top = (int)(q.x % (uint32_t)(Hs - bx.h + 1));
          bx.left = (int)(q.y % (uint32_t)(Ws - bx.w + 1));
          return 2 * k + e;
        }
      }
    }
  }
  const float in_ratio = (float)Ws / (float)Hs;
  bx.h = Hs;
  bx.w = Ws;
  if (in_ratio < p.ratio_lo)
    bx.h = min(max((int)rintf((float)Ws / p.ratio_lo), 1), Hs);
  else if (in_ratio > p.ratio_hi)
    bx.w = min(max((int)rintf((float)Hs * p.ratio_hi), 1), Ws);
  bx.top = (Hs - bx.h) / 2;
  bx.left = (Ws - bx.w) / 2;
  return 10;
}

// params[0..7] of a slot's row: the draws every recipe has.
MA_DEV void dump_draws(float* o, int dy, int dx, int flip, float angle, float scale, int cut_y,
                       int cut_x, int attempt) {
  o[0] = (float)dy;
  o[1] = (float)dx;
  o[2] = (float)flip;
  o[3] = angle;
  o[4] = scale;
  o[5] = (float)cut_y;
  o[6] = (float)cut_x;
  o[7] = (float)attempt;
}

// GEOM 0..3: the Resize -> RandomCrop -> [RandomAffine] chain, AFFINE << 1 | RESIZE; GEOM 4:
// RandomResizedCrop.  PHOTO (a drawn box or colour factors): thread 0 draws them and hands them
// to the block through LDS, and the params row has 16 floats; without, there is no LDS, no
// barrier and the row has 8.
template <int GEOM, bool JIT>
__global__ __launch_bounds__(256) void pool_recipe_kernel(PoolRecipeArgs p) {
  constexpr bool RRC = GEOM == 4, AFFINE = (GEOM & 2) != 0, RESIZE = (GEOM & 1) != 0;
  constexpr bool PHOTO = RRC || JIT;
  constexpr int PARAMS_LD = PHOTO ? 16 : 8;      // floats of a slot's params row
  const PoolBuildArgs& b = p.b;
  const int slot = blockIdx.x;
  if (b.zero) zero_slice(b);
  int64_t gb;
  int t;
  const uint32_t src = pool_src(b, slot, gb, t);
  const int H = b.H, W = b.W;
  int dy = 0, dx = 0, flip = 0;
  if (!RRC) {
    dy = (p.Hr + 2 * b.pad - H) / 2;
    dx = (p.Wr + 2 * b.pad - W) / 2;
  }
  float angle = 0.f, scale = 1.f;
  int cut_y = 0, cut_x = 0, cut = 0;
  if (b.augment) {
    const u32x4 r = pool_draw(gb, t, DRAW_CROP, b.seed);
    if (!RRC) {
      dy = r.x % (p.Hr + 2 * b.pad - H + 1);
      dx = r.y % (p.Wr + 2 * b.pad - W + 1);
    }
    flip = b.flip ? (r.z & 1) : 0;
    const u32x4 q = pool_draw(gb, t, DRAW_AFFINE, b.seed);
    if (!RRC) {
      angle = -p.degrees + 2.f * p.degrees * u01(q.x);
      scale = p.scale_lo + (p.scale_hi - p.scale_lo) * u01(q.y);
    }
    cut_y = q.z % H;
    cut_x = q.w % W;
    cut = p.cutout;
  }
  PhotoBox bx{0, 0, 0, 0};
  float f[4] = {1.f, 1.f, 1.f, 0.f};
  int seq = OP_SKIP * 0x1111;
  if constexpr (PHOTO) {
    // the box search and the colour draws run once, in thread 0, and reach the block through LDS
    __shared__ float sh_f[4];
    __shared__ int sh_i[6];
    if (threadIdx.x == 0) {
      int attempt = 0, code = 0;
      if (RRC) attempt = rrc_box(p, gb, t, bx);
      if (JIT && b.augment) {
        const u32x4 r = pool_draw(gb, t, DRAW_COLOUR, b.seed);
        const uint32_t w[3] = {r.x, r.y, r.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float lo = fmaxf(0.f, 1.f - p.jitter[k]), hi = 1.f + p.jitter[k];
          f[k] = lo + (hi - lo) * u01(w[k]);
        }
        f[3] = -p.jitter[3] + 2.f * p.jitter[3] * u01(r.w);
        code = (int)(pool_draw(gb, t, DRAW_ORDER, b.seed).x % 24u);
      }
      if (JIT) {                        // (augment = 0: identity factors in order 0)
        const int pick[3] = {code / 6, (code % 6) >> 1, code & 1};
        int list = 0x3210;
        seq = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int s4 = k < 3 ? 4 * pick[k] : 0;
          const int op = (list >> s4) & 15;
          list = (list & ((1 << s4) - 1)) | ((list >> (s4 + 4)) << s4);
          seq |= (p.jitter[op] > 0.f ? op : OP_SKIP) << (4 * k);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sh_f[k] = f[k];
      sh_i[0] = bx.top;
      sh_i[1] = bx.left;
      sh_i[2] = bx.h;
      sh_i[3] = bx.w;
      sh_i[4] = seq;
      pool_slot_header(b, slot, src);
      if (p.params) {
        float* o = p.params + (size_t)slot * PARAMS_LD;
        dump_draws(o, RRC ? bx.top : dy, RRC ? bx.left : dx, flip, angle, scale, cut_y, cut_x,
                   attempt);
        o[8] = (float)bx.h;
        o[9] = (float)bx.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[10 + k] = f[k];
        o[14] = (float)code;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = uni_f(sh_f[k]);
    bx.top = __builtin_amdgcn_readfirstlane(sh_i[0]);
    bx.left = __builtin_amdgcn_readfirstlane(sh_i[1]);
    bx.h = __builtin_amdgcn_readfirstlane(sh_i[2]);
    bx.w = __builtin_amdgcn_readfirstlane(sh_i[3]);
    seq = __builtin_amdgcn_readfirstlane(sh_i[4]);
  } else if (threadIdx.x == 0) {
    pool_slot_header(b, slot, src);
    if (p.params)
      dump_draws(p.params + (size_t)slot * PARAMS_LD, dy, dx, flip, angle, scale, cut_y, cut_x,
                 0);
  }

  // Cutout.__call__: [clip(c - L/2, 0, n), clip(c + L/2, 0, n)) in both axes (empty when off)
  const int ch = cut / 2;
  const int cy0 = cut ? max(cut_y - ch, 0) : 0, cy1 = cut ? min(cut_y + ch, H) : 0;
  const int cx0 = cut ? max(cut_x - ch, 0) : 0, cx1 = cut ? min(cut_x + ch, W) : 0;
  const float ry = RRC ? (float)bx.h / (float)H : (float)p.Hs / (float)p.Hr;
  const float rx = RRC ? (float)bx.w / (float)W : (float)p.Ws / (float)p.Wr;
  float cs = 1.f, sn = 0.f;
  if (AFFINE) {
    const float rad = angle * 0.017453292519943295f;
    cs = cosf(rad) / scale;
    sn = sinf(rad) / scale;
  }
  const uint8_t* img = b.shard + (size_t)src * p.Hs * p.Ws * 3;
  bf16* out = b.pool + (size_t)slot * H * W * 8;
  const int npx = H * W;

  auto geometry = [&](int px, int& i, int& j, float v[3]) {   // uint8 levels, float
    i = px / W;
    j = px - i * W;
    if (RRC)
      rrc_pixel(img, p.Ws, bx, i, flip ? W - 1 - j : j, ry, rx, v);
    else
      aug_pixel<AFFINE, RESIZE>(p, img, H, W, i, j, dy, dx, flip, ry, rx, cs, sn, v);
  };

  float m = 0.f;                      // params[15]: written with the 16-float row only
  if constexpr (JIT) {
    __shared__ float red[16];
    const bool contrast = ((seq & 15) == OP_CONTRAST) | (((seq >> 4) & 15) == OP_CONTRAST) |
                          (((seq >> 8) & 15) == OP_CONTRAST) | (((seq >> 12) & 15) == OP_CONTRAST);
    if (contrast) {                   // uniform over the block
      float acc = 0.f;
      for (int px = threadIdx.x; px < npx; px += 256) {
        int i, j;
        float v[3];
        geometry(px, i, j, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] *= 1.f / 255.f;
        jitter_pixel<true>(v, seq, f, 0.f);
        acc += grey(v);
      }
      m = block_sum(acc, red) / (float)npx;
    }
    if (threadIdx.x == 0 && p.params) p.params[(size_t)slot * PARAMS_LD + 15] = m;
  } else if (PHOTO && threadIdx.x == 0 && p.params) {
    p.params[(size_t)slot * PARAMS_LD + 15] = 0.f;
  }

  for (int px = threadIdx.x; px < npx; px += 256) {
    int i, j;
    float v[3];
    geometry(px, i, j, v);
    const bool hole = i >= cy0 && i < cy1 && j >= cx0 && j < cx1;
    bf16x8 o;
    if (JIT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] *= 1.f / 255.f;
      jitter_pixel<false>(v, seq, f, m);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = f2bf(hole ? 0.f : (v[c] - b.mean[c]) * b.inv_std[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[c] = f2bf(hole ? 0.f : (v[c] * (1.f / 255.f) - b.mean[c]) * b.inv_std[c]);
    }
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = f2bf(0.f);
    *(bf16x8*)(out + (size_t)px * 8) = o;
  }
}

}  // namespace

template <int GEOM>
static void recipe_launch(const PoolRecipeArgs& p, bool jit, hipStream_t st) {
  if (jit)
    hipLaunchKernelGGL((pool_recipe_kernel<GEOM, true>), dim3(p.b.P), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((pool_recipe_kernel<GEOM, false>), dim3(p.b.P), dim3(256), 0, st, p);
}

void pool_recipe_launch(const PoolRecipeArgs& p, hipStream_t st) {
  const bool jit = p.jitter[0] > 0.f || p.jitter[1] > 0.f || p.jitter[2] > 0.f || p.jitter[3] > 0.f;
  switch (p.rrc ? 4 : (p.affine ? 2 : 0) | (p.resize ? 1 : 0)) {
    case 4: recipe_launch<4>(p, jit, st); break;
    case 3: recipe_launch<3>(p, jit, st); break;
    case 2: recipe_launch<2>(p, jit, st); break;
    case 1: recipe_launch<1>(p, jit, st); break;
    default: recipe_launch<0>(p, jit, st); break;
  }
}
