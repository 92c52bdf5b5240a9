"""Draw-by-draw tests of the pool sampler (``csrc/importance.hip`` is_sample_kernel), both paths.

Every draw is ``philox4x32(ctrl[1], d, stream word; seed, k1)``; ``sampler_oracles`` replays the
generator, so each test knows the uniforms behind every one of its 2**20 draws and says which
sample draw ``d`` had to be -- one launch per case, no statistics.

Exact cases (``exact_losses``: dyadic, mean 1, every fp32 operation of the kernel exact; alpha 0):
``idx`` must equal the pick of ``alias_closed_form`` (alias path) or of the exact CDF search
(inverse-CDF path) for every draw, and ``w`` must equal ``p[idx] / total * P`` bit for bit.  The
same for ``importance=False``, for the silent fall-back to the inverse CDF above the LDS limit
(P = 4096) and for a draw counter at or above 2**32.

Random cases (``skewed_losses``, alpha 0.5, the EMA read back from ``ema[0]``), against fp64:

* inverse CDF: ``cdf64[k-1] - eps*total <= u01*total64 < cdf64[k] + eps*total`` for k = idx[d],
  ``eps = 2 * (seg + 12) * 2**-24`` (``pool_eps``): all terms are positive, a prefix carries at
  most seg + 6 + 4 fp32 additions, ``u01 * total`` one more rounding, doubled.
* alias: the table is recovered from (bin, u_y, idx) alone (``recover_alias_table``): the alias
  of a bucket must be unique, and the bracket it gives for every item must hold
  ``lo_i - tol <= P p_i <= hi_i + U + tol`` with ``tol = eps * max(1, total deficit)`` (the
  deficit and excess scans) and U, the mass of the buckets that never moved, below 0.5 % of P.
* weights: ``P p64[idx] / total64`` within eps relative plus 2 ulp.

Observed on the MI355X, in units of the bound (the CPU fp32 emulation of
``test_sampler_oracles`` gives the same figures):

* inverse CDF, P = 320 / 1056 / 2048 / 4096: the worst draw lies 0.046 / 0.051 / 0.094 / 0.073 of
  the bound outside its fp64 interval (1.2e-5 / 2.6e-5 / 9.3e-5 / 1.3e-4 of the draws lie outside
  it at all, each by one neighbour); weights 0.088 / 0.088 / 0.058 / 0.053 of their bound.
* alias, P = 320 / 1056 / 2048: no item leaves its bracket (worst -0.003 / -0.002 / -0.001 tol,
  negative = inside), U = 2.9e-4 / 7.3e-3 / 1.1e-2 over 1 / 3 / 4 buckets, mean bracket 0.0012 /
  0.0041 / 0.0079 of a uniform share; weights 0.088 / 0.088 / 0.058 of their bound.
* equal losses 0.3, P = 320 / 1056: inside the bracket by 0.77 / 0.71 tol, no bucket ever moved
  (U = 0.097 / 1.13, bound 1.6 / 5.3), every w within 4 ulp of 1.
* the exact cases, ``importance=False``, the fall-back and the 64-bit counter: 0 draws differ.

The weight bound found a defect: the inverse-CDF path took the weight from the CDF difference
``p[k] - p[k-1]``, which carries the prefix's rounding -- 53 / 239 / 480 / 836 times the bound
(1e-4 .. 1.7e-3 relative) at P = 320 .. 4096.  The kernel now forms it from the item's own p.

Each test is one launch (two or three for the fall-back and the counter) plus numpy work; the
slowest took 0.15 s on the MI355X (0.3 s for whichever runs first and loads the extension),
below the 0.38 s of the parent's slowest chi-square test there.

Blocks of 0.25 x3 and 1.75 x1 have P / total = 1.6, no power of two, so the exact block case is
the sibling with deficits of 0.25 (0.75 x3, 1.75 x1, mean 1) and the 0.25 vector is held to the
bracket (``test_quarter_blocks_...``).  "One heavy" is 0.5 everywhere and
(P + 1) / 2 once: a power of two there cannot make the mean a power of two for these P.
"""
import functools

import numpy as np
import pytest
import torch

import sampler_oracles as so

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = np.float32
NDRAW = 1 << 20
SEED = 1


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _run(losses, P, group, alias, B=NDRAW, dc=0, pc=0, alpha=0.5, importance=True):
    """One is_sample launch -> (idx int64, w fp32, the EMA the weights used, ctrl after)."""
    ops = _ops()
    l = torch.from_numpy(np.ascontiguousarray(losses, dtype=F32)).to(DEV)
    ema = torch.zeros(2, device=DEV)
    ctrl = torch.tensor([pc, dc, 0, 0], dtype=torch.int64, device=DEV)
    idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    w = torch.full((B,), float('nan'), device=DEV)
    ops.is_sample(l, ema, ctrl, idx, w, P, B, group, alpha=alpha, ema_alpha=0.9, seed=SEED,
                  importance=importance, alias=alias)
    return (idx.cpu().numpy().astype(np.int64), w.cpu().numpy(), F32(ema[0].item()),
            ctrl.cpu().tolist())


@functools.lru_cache(maxsize=4)
def _uniforms(dc, alias, P, B=NDRAW):
    return so.pool_draw_uniforms(dc, SEED, B, alias, P=P)


@functools.lru_cache(maxsize=None)
def _closed_form(kind, P):
    q, alias = so.alias_closed_form(so.exact_losses(kind, P))
    return np.array([float(x) for x in q], F32), np.array(alias, np.int64)


def _exact_pick(v, kind, P, alias, dc=0, B=NDRAW):
    """The sample every draw has to be on an exact vector (fp32 sums exact, total = fp32)."""
    total = F32(v.astype(np.float64).sum())
    if alias:
        q, al = _closed_form(kind, P)
        bins, uy = _uniforms(dc, True, P, B)
        return np.where(uy < q[bins], bins, al[bins]), total
    cdf = np.cumsum(v.astype(np.float64)).astype(F32)          # exact
    u = _uniforms(dc, False, None, B) * total                  # one fp32 multiply, as the kernel
    return np.minimum(np.searchsorted(cdf, u, side='right'), P - 1), total


def _assert_exact(idx, w, ref, v, total, P):
    bad = np.nonzero(idx != ref)[0]
    assert bad.size == 0, '%d draws differ, first d=%d: got %d want %d' % (
        bad.size, bad[0], idx[bad[0]], ref[bad[0]])
    wref = v[ref] / total * F32(P)
    assert wref.dtype == F32 and np.array_equal(w, wref)


@pytest.mark.parametrize('alias', [True, False], ids=['alias', 'cdf'])
@pytest.mark.parametrize('P,group', so.EXACT_SHAPES)
@pytest.mark.parametrize('kind', so.EXACT_KINDS)
def test_exact_vectors_every_draw(kind, P, group, alias):
    v = so.exact_losses(kind, P)
    idx, w, _, _ = _run(v, P, group, alias, alpha=0.0)
    ref, total = _exact_pick(v, kind, P, alias)
    _assert_exact(idx, w, ref, v, total, P)


@pytest.mark.parametrize('alias', [True, False], ids=['alias', 'cdf'])
@pytest.mark.parametrize('P,group', so.EXACT_SHAPES)
def test_importance_off_draws_uniformly(P, group, alias):
    """importance=False: every bucket keeps 1, so an alias draw is its own bin and an inverse-CDF
    draw is floor(u01 * P) (one fp32 multiply); w is exactly 1.  The losses are ignored."""
    idx, w, _, _ = _run(so.skewed_losses(P), P, group, alias, importance=False)
    if alias:
        ref = _uniforms(0, True, P)[0]
    else:
        ref = np.minimum((_uniforms(0, False, None) * F32(P)).astype(np.int64), P - 1)
    assert np.array_equal(idx, ref)
    assert np.all(w == F32(1))


def test_fallback_above_the_lds_limit_is_the_inverse_cdf():
    """P = 4096: alias=True runs the inverse-CDF path (stream word 0xd1a5), bit for bit."""
    P = 4096
    l = so.skewed_losses(P)
    ia, wa, ea, _ = _run(l, P, 32, True)
    ic, wc, ec, _ = _run(l, P, 32, False)
    assert np.array_equal(ia, ic) and np.array_equal(wa.view(np.int32), wc.view(np.int32))
    assert ea == ec
    v = so.exact_losses('alternating', P)
    idx, w, _, _ = _run(v, P, 32, True, alpha=0.0)
    ref, total = _exact_pick(v, 'alternating', P, False)
    _assert_exact(idx, w, ref, v, total, P)


@pytest.mark.parametrize('alias', [True, False], ids=['alias', 'cdf'])
def test_draw_counter_is_64_bit_and_advances(alias):
    P, B, kind = 320, 1 << 16, 'alternating'
    v = so.exact_losses(kind, P)
    hi, lo = 2 ** 32 + 5, 5
    idx_hi, w, _, ctrl = _run(v, P, 32, alias, B=B, dc=hi, pc=7, alpha=0.0)
    assert ctrl[:2] == [8, hi + 1]
    ref_hi, total = _exact_pick(v, kind, P, alias, dc=hi, B=B)
    ref_lo, _ = _exact_pick(v, kind, P, alias, dc=lo, B=B)
    assert not np.array_equal(ref_hi, ref_lo)
    _assert_exact(idx_hi, w, ref_hi, v, total, P)
    idx_lo, w, _, ctrl = _run(v, P, 32, alias, B=B, dc=lo, alpha=0.0)
    assert ctrl[:2] == [1, lo + 1]
    _assert_exact(idx_lo, w, ref_lo, v, total, P)


def _p64(l, ema, alpha=0.5):
    return l.astype(np.float64) + alpha * float(ema)


@pytest.mark.parametrize('P', [320, 1056, 2048, 4096])
def test_skewed_inverse_cdf_every_draw_within_bound(P):
    l = so.skewed_losses(P)
    idx, w, ema, _ = _run(l, P, 32, False)
    assert abs(float(ema) - float(so.ema_replay(l, 32))) < 1e-5
    assert idx.min() >= 0 and idx.max() < P
    p64, eps = _p64(l, ema), so.pool_eps(P)
    below, above, outside = so.cdf_draw_violation(idx, _uniforms(0, False, None), p64, eps)
    wv = so.weight_violation(w, idx, p64, eps)
    print('\ncdf P %d: below %.3f above %.3f of the bound, %.2e of draws outside the fp64 '
          'interval; weights %.3f' % (P, below, above, outside, wv))
    assert below < 1 and above < 1
    assert wv < 1


def _alias_case(l, P, alpha=0.5):
    idx, w, ema, _ = _run(l, P, 32, True, alpha=alpha)
    assert idx.min() >= 0 and idx.max() < P
    bins, uy = _uniforms(0, True, P)
    p64 = _p64(l, ema, alpha)
    unique, worst, U, unknown, width = so.alias_draw_violation(bins, uy, idx, p64)
    print('\nalias P %d: worst %.3f tol, U %.2e over %d buckets, mean bracket %.4f'
          % (P, worst, U, unknown, width))
    assert unique, 'a bucket sent its draws to more than one alias'
    assert worst < 1
    assert U < 0.005 * P
    return idx, w, p64


@pytest.mark.parametrize('P', [320, 1056, 2048])
def test_skewed_alias_table_recovered_from_the_draws(P):
    idx, w, p64 = _alias_case(so.skewed_losses(P), P)
    wv = so.weight_violation(w, idx, p64, so.pool_eps(P))
    print('weights %.3f' % wv)
    assert wv < 1


@pytest.mark.parametrize('P', [320, 1056])
def test_equal_losses_draw_uniformly(P):
    """All losses 0.3: rounding decides which buckets are light, and the numerically-all-light
    fall-back may run.  The implied distribution is uniform within tol; every w is 1 within
    4 ulp."""
    idx, w, _ = _alias_case(np.full(P, 0.3, F32), P)
    assert so.ulps32(w, np.ones_like(w)).max() <= 4
    counts = np.bincount(idx, minlength=P)
    assert counts.min() > 0


def test_quarter_blocks_alias_table_recovered_from_the_draws():
    """Blocks of 0.25 x3 and 1.75 x1: P / total = 1.6 is no power of two, so the build rounds
    and the vector is held to the bracket, not bit for bit (``exact_losses('blocks')`` is its
    exact sibling, deficits of 0.25)."""
    P = 320
    idx, w, p64 = _alias_case(np.tile(np.array([0.25, 0.25, 0.25, 1.75], F32), P // 4), P, alpha=0.0)
    assert so.weight_violation(w, idx, p64, so.pool_eps(P)) < 1
