// The BatchNorm scale / shift, mean / rstd and activation arithmetic of every kernel in csrc/.
//
// Fused consumers of a BN (the conv prologues, the pool, the head, the depthwise conv, pgemm /
// pwconv and the halo conv) must agree with bn.hip to the bit -- the tests compare them with
// torch.equal -- so the arithmetic is written down here once and every site passes it the values
// it has loaded.  Each site keeps its own loads and pointer selection; only values come in.
#pragma once
#include "common.h"

MA_DEV float act_fwd(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return fminf(fmaxf(v, 0.f), 6.f);
  return v;
}
// derivative from the activation OUTPUT
MA_DEV float act_mask(float out, int act) {
  if (act == 1) return out > 0.f ? 1.f : 0.f;
  if (act == 2) return (out > 0.f && out < 6.f) ? 1.f : 0.f;
  return 1.f;
}
// act'(out) != 0  <=>  act == none, or lo < out < hi: bounds from the uniform act once, so the
// per-element test is two compares, one uniform OR and one select -- a runtime act switch inside
// the unrolled element loop was if-converted into every activation form plus selects.  act ==
// none passes EVERY value (NaN and +-inf included), exactly like act_mask, so a diverging run is
// not hidden from the health checks by a fused reduction.
MA_DEV void bn_act_bounds(int act, float& lo, float& hi) {
  lo = act == 0 ? -__builtin_huge_valf() : 0.f;
  hi = act == 2 ? 6.f : __builtin_huge_valf();
}
// Forward clamp bounds: act == none clamps against NaN, which v_max/v_min_f32 ignore (they
// return the non-NaN operand), so the clamp is the identity and a NaN input stays NaN as in
// act_fwd; relu / relu6 clamp as act_fwd does.
MA_DEV void act_clamp_bounds(int act, float& lo, float& hi) {
  lo = act == 0 ? __builtin_nanf("") : 0.f;
  hi = act == 2 ? 6.f : (act == 0 ? __builtin_nanf("") : __builtin_huge_valf());
}

// The single definition of the BN arithmetic.  Every fused and standalone path computes, in
// this expression order and from values the site has loaded,
//   mean = sum * inv_count;  var = max(sumsq * inv_count - mean * mean, 0)   (or the running pair)
//   scale = gamma * rsqrt(var + eps);  shift = beta - mean * scale           (forward)
//   rstd = rsqrt(var + eps)                                                  (backward)
// The three steps are separate so that a site whose loads sit between them -- the statistics in
// an ``if (stats) ... else ...``, beta behind the store of the scale -- keeps its loads and its
// branch where they are: bn_scale_shift's run-time flag compiles to selects, which is the code
// of the sites that load everything up front, not of those.
MA_DEV void bn_mean_var(float s, float ss, float inv_count, float& mean, float& var) {
  mean = s * inv_count;
  var = fmaxf(ss * inv_count - mean * mean, 0.f);
}
MA_DEV float bn_scale(float gamma, float var, float eps) { return gamma * rsqrtf(var + eps); }
MA_DEV float bn_shift(float beta, float mean, float sc) { return beta - mean * sc; }
// (a, b): the batch sums (sum, sumsq) over 1 / inv_count elements when from_sums, else the
// running (mean, var)
MA_DEV void bn_scale_shift(float a, float b, bool from_sums, float inv_count, float eps,
                           float gamma, float beta, float& sc, float& sh) {
  float mean = a, var = b;
  if (from_sums) bn_mean_var(a, b, inv_count, mean, var);
  sc = bn_scale(gamma, var, eps);
  sh = bn_shift(beta, mean, sc);
}
// BN backward: (mean, rstd) of a channel from its batch sums
MA_DEV void bn_mean_rstd(float s, float ss, float inv_count, float eps, float& mean, float& rstd) {
  float var;
  bn_mean_var(s, ss, inv_count, mean, var);
  rstd = rsqrtf(var + eps);
}

MA_DEV void load8(const float* p, float (&v)[8]) {     // 8 floats as two 16-byte loads
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// scale/shift for 8 channels: from batch sums (sum, sumsq) or running (mean, var).
MA_DEV void scale_shift8(const float* mean_or_sum, const float* var_or_sq, bool running,
                         float inv_cnt, float eps, const float* gamma, const float* beta,
                         float (&sc)[8], float (&sh)[8]) {
  float a[8], b[8], g[8], be[8];
  load8(mean_or_sum, a);
  load8(var_or_sq, b);
  load8(gamma, g);
  load8(beta, be);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    bn_scale_shift(a[k], b[k], !running, inv_cnt, eps, g[k], be[k], sc[k], sh[k]);
}

// mean / rstd for 8 channels from sums at ``stats`` and sums of squares at ``stats + ld``
MA_DEV void mean_rstd8(const float* stats, int ld, float inv_cnt, float eps, float (&mean)[8],
                       float (&rstd)[8]) {
  float s[8], ss[8];
  load8(stats, s);
  load8(stats + ld, ss);
#pragma unroll
  for (int k = 0; k < 8; ++k) bn_mean_rstd(s[k], ss[k], inv_cnt, eps, mean[k], rstd[k]);
}
