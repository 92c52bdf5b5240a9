"""CPU evidence for ``sampler_oracles`` (no GPU needed): the Philox replica reproduces the
Random123 known-answer vectors, the alias closed form stands exactly for ``v / sum(v)``, and an
fp32 emulation of is_sample's two paths (the kernel's scan order) stays inside the bounds that
``test_sampler_draws_gpu`` holds the kernel to -- so a failing GPU test cannot be the
reference's own rounding.

fp32 emulation against the bounds (2**20 draws, alpha 0.5, ``skewed_losses``):

    inverse CDF, P = 320 / 1056 / 2048 / 4096: worst distance outside the fp64 interval 0.046 /
    0.051 / 0.094 / 0.073 of the bound; weights ``p[pick] / total * P`` 0.074 / 0.088 / 0.058 /
    0.053 of the bound.  (The CDF difference ``(cdf[k] - cdf[k-1]) / total * P`` that the kernel
    used before is at 57 / 239 / 480 / 836 times the bound: a cancellation, see the README.)
    alias, P = 320 / 1056 / 2048: the table's implied P * p is within 0.086 / 0.139 / 0.110 tol
    of fp64, and no item leaves the bracket recovered from the draws.
"""
from fractions import Fraction

import numpy as np
import pytest

import sampler_oracles as so

F32 = np.float32
NDRAW = 1 << 20


def _hex(r):
    return ' '.join('%08x' % int(x) for x in r)


def test_philox_known_answers():
    """The three Random123 vectors of philox4x32_10."""
    assert _hex(so.philox4x32((0, 0, 0, 0), 0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    ones = 0xffffffff
    assert _hex(so.philox4x32((ones,) * 4, ones, ones)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    pi = (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)
    assert _hex(so.philox4x32(pi, 0xa4093822, 0x299f31d0)) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_philox_is_vectorised_over_draws():
    r = so.philox4x32((5, 1, np.arange(4), 0xa11a), 9, so.POOL_K1)
    for d in range(4):
        one = so.philox4x32((5, 1, d, 0xa11a), 9, so.POOL_K1)
        assert [int(x[d]) for x in r] == [int(x) for x in one]


def test_uniforms():
    assert so.u01(0xffffffff) == F32(1 - 2.0 ** -24) and so.u01(0xff) == 0
    b, uy = so.pool_draw_uniforms(7, 3, 4096, True, P=320)
    assert b.min() >= 0 and b.max() < 320 and uy.dtype == F32 and uy.max() < 1
    assert so.pool_draw_uniforms(7, 3, 16, False).dtype == F32
    # the high word of the counter reaches the generator
    assert not np.array_equal(so.pool_draw_uniforms(5, 3, 16, False),
                              so.pool_draw_uniforms(2 ** 32 + 5, 3, 16, False))
    rx, ry = so.table_draw_uniforms(2 ** 32 + 3, 1, 1000)
    u = so.table_u(rx, ry, 10.0)
    assert u.min() >= 0 and u.max() < 10.0
    ones = np.array([0xffffffff], np.uint64)
    assert so.table_u(ones, ones, 10.0)[0] == 10.0 * (1 - 1e-12)      # the clamp below total


@pytest.mark.parametrize('kind', so.EXACT_KINDS + ('uniform',))
@pytest.mark.parametrize('P,group', so.EXACT_SHAPES)
def test_closed_form_is_the_distribution_exact_vectors(kind, P, group):
    """(q_i + sum_{alias_j == i} (1 - q_j)) / P == v_i / sum(v) in Fraction, and every q is an
    fp32 number, as are P / total and every partial sum: the kernel's fp32 build is exact."""
    v = so.exact_losses(kind, P)
    q, alias = so.alias_closed_form(v)
    tot = sum(Fraction(float(x)) for x in v)
    assert so.implied_distribution(q, alias) == [Fraction(float(x)) / tot for x in v]
    assert all(Fraction(float(F32(float(x)))) == x for x in q)
    scale = Fraction(P) / tot
    assert scale.numerator == 1 or scale.denominator == 1
    assert (scale.numerator & (scale.numerator - 1)) == 0
    assert (scale.denominator & (scale.denominator - 1)) == 0
    assert float(np.cumsum(v.astype(np.float64))[-1]) < 2 ** 13 and np.all(v * 4 == np.round(v * 4))
    # the fp32 emulation reproduces the closed form bit for bit on these vectors
    q32, a32, t32 = so.alias_fp32_emulation(v)
    assert np.array_equal(q32, np.array([float(x) for x in q], F32))
    assert np.array_equal(a32, np.array(alias)) and Fraction(float(t32)) == tot


def test_exact_vectors_have_the_structure_the_cases_name():
    q, alias = so.alias_closed_form(so.exact_losses('alternating', 32))
    assert alias[0] == 1 and alias[2] == 1 and alias[1] == 3      # two lights share heavy 1
    q, alias = so.alias_closed_form(so.exact_losses('blocks', 32))
    assert alias[0] == alias[1] == alias[2] == 3
    q, alias = so.alias_closed_form(so.exact_losses('one_heavy', 32))
    assert all(alias[i] == 10 for i in range(32)) and q[10] == 1


def _p(P):
    """(fp32 weights as the kernel forms them, the same in fp64) for the random cases."""
    l = so.skewed_losses(P)
    ema = so.ema_replay(l, 32)
    return (l + F32(0.5) * ema).astype(F32), l.astype(np.float64) + 0.5 * float(ema)


@pytest.mark.parametrize('P', [320, 1056, 2048])
def test_closed_form_is_the_distribution_random_vectors(P):
    p32, _ = _p(P)
    v = [Fraction(float(x)) for x in p32]
    q, alias = so.alias_closed_form(v)
    tot = sum(v)
    assert so.implied_distribution(q, alias) == [x / tot for x in v]


@pytest.mark.parametrize('P', [320, 1056, 2048, 4096])
def test_fp32_inverse_cdf_is_within_the_gpu_bounds(P):
    p32, p64 = _p(P)
    cdf, total = so.cdf_fp32_emulation(p32)
    u = so.pool_draw_uniforms(0, 1, NDRAW, False)
    pick = np.minimum(np.searchsorted(cdf, u * total, side='right'), P - 1)
    eps = so.pool_eps(P)
    below, above, outside = so.cdf_draw_violation(pick, u, p64, eps)
    w = p32[pick] / total * F32(P)
    wv = so.weight_violation(w, pick, p64, eps)
    print('P %d  below %.3f above %.3f outside %.2e  weights %.3f' % (P, below, above, outside, wv))
    assert below < 1 and above < 1 and wv < 1
    # the neighbour's boundary rule (p[mid] >= u) is NOT what the bound hides: it moves a draw
    # only where u equals a CDF entry, so the exact cases of the GPU module hold it, not this one


@pytest.mark.parametrize('P', [320, 1056, 2048])
def test_fp32_alias_build_is_within_the_gpu_bounds(P):
    p32, p64 = _p(P)
    q, alias, total = so.alias_fp32_emulation(p32)
    x = P * p64 / p64.sum()
    tol = so.alias_tol(p64, P)
    implied = q.astype(np.float64)
    np.add.at(implied, alias, np.where(alias != np.arange(P), 1.0 - q.astype(np.float64), 0.0))
    direct = float(np.abs(implied - x).max()) / tol
    bins, uy = so.pool_draw_uniforms(0, 1, NDRAW, True, P=P)
    idx = np.where(uy < q[bins], bins, alias[bins])
    unique, worst, U, unknown, width = so.alias_draw_violation(bins, uy, idx, p64)
    print('P %d  table %.3f tol  draws %.3f tol  U %.2e (%d buckets)  bracket %.4f'
          % (P, direct, worst, U, unknown, width))
    assert unique and direct < 1 and worst < 1 and U < 0.005 * P
    w = p32[idx] / total * F32(P)
    assert so.weight_violation(w, idx, p64, so.pool_eps(P)) < 1


def test_recovery_sees_a_wrong_table():
    """One bucket's kept share off by a percent, and one member that is never drawn: both leave
    the bracket by many tol (a chi-square at this sample size sees neither)."""
    P = 320
    p32, p64 = _p(P)
    q, alias, _ = so.alias_fp32_emulation(p32)
    bins, uy = so.pool_draw_uniforms(0, 1, NDRAW, True, P=P)
    j = int(np.argmin(np.abs(q - 0.5)))
    bad = q.copy()
    bad[j] = bad[j] * F32(1.01)
    assert so.alias_draw_violation(bins, uy, np.where(uy < bad[bins], bins, alias[bins]), p64)[1] > 5
    idx = np.where(uy < q[bins], bins, alias[bins])
    idx[idx == j] = alias[j]
    assert so.alias_draw_violation(bins, uy, idx, p64)[1] > 5
