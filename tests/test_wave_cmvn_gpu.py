"""Per-utterance CMVN pools (``pool_wave_mel_kernel<.., FEAT>`` + ``pool_cmvn_kernel``): every element
against ``WaveRecipe.reference`` in fp64, fed with the dumped draws.  Bound: with ``E_r = 2e-3 S_r``
(``tests/test_wave_mel_gpu.py``'s bound on the feature ``v``) and ``s_r = sqrt(var_r + floor)`` (1 for
``cmvn=1``), an error of at most ``E_r`` in every ``v`` moves mean and standard deviation by at most
``E_r`` each, so to first order ``|dz| <= (2 + |z|) E_r / s_r``: the pool is within ``2^-8 |ref| + |a|
(2 + |z|) E_r / s_r``, times ``g^k``, ``g = 3 / (2N + 1)``, on order-k rows.  The clips are the mel
tests' noise, tone and quiet clips under a gain decaying from 1 to 1/32, which keeps the identity
cases' least ``s_r`` at 0.27 or more on the first four shapes (README, "Per-utterance CMVN"); T = 2
cannot meet 0.25, so the least ``s_r`` is printed, not asserted.  Rows constant by construction (a
filter with no bin under it, T = 1) have ``s_r = sqrt(floor)``: there the formula is loose."""
import dataclasses
import math

import pytest
import torch

from test_wave_mel_gpu import DEV, SEED, SENTINEL, _clips

pytestmark = pytest.mark.gpu

P = 5
# (n_fft, hop, L, mel, dct, preemph): T = 34, R = 13: the last block has one live wave | the same,
# pre-emphasised | T = 161: three lane trips, the last partial | odd hop, dct = mel | T = 2: every
# clamp active | T = 1
SHAPES = [(200, 100, 3300, 80, 13, 0.0), (200, 100, 3300, 80, 13, 0.97), (200, 100, 16000, 40, 0, 0.0),
          (30, 7, 300, 8, 8, 0.0), (16, 16, 24, 8, 0, 0.0), (16, 16, 12, 8, 0, 0.0)]
FULL = dict(gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), fill=-1.5)


def _recipe(shape, full, **kw):
    from mercury_amd.data.augment import WaveRecipe
    W, hop, L, mel, dct, pre = shape
    if full:
        kw.update(FULL, shift=W, tmask=(2, min(3, 1 + L // hop)), fmask=(0, 0) if dct else (2, 3))
    return WaveRecipe(n_fft=W, hop=hop, mel=mel, dct=dct, preemph=pre, **kw)


def _build(L, dtype, recipe, chunks=0):
    """One pool of the 5 decaying clips between two guard slots -> (pool, params, x, bank)"""
    from mercury_amd.ops.importance import _pool_wave
    x, bank, labels = _clips(L, dtype)
    x = x[[0, 1, 3, 4, 5]].double() * 32.0 ** (-torch.arange(L, dtype=torch.float64) / L)
    x, labels = (x.round() if dtype == torch.int16 else x).to(dtype), labels[:P]
    big = torch.full((P + 2, *recipe.out_hw(L), 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.full((P,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    params = torch.full((P, 16), -99.0, device=DEV)
    _pool_wave(x.to(DEV), bank.to(DEV) if recipe.noise else None, labels.to(DEV),
               torch.zeros(4, dtype=torch.int64, device=DEV), big[1:P + 1], pl, pi, P, P, SEED,
               True, False, None, recipe, params, chunks=chunks)
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    assert pi.tolist() == list(range(P))                     # (unshuffled: slot i holds clip i)
    return big[1:P + 1], params.cpu(), x, bank


@pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
@pytest.mark.parametrize('full', [False, True], ids=['identity', 'full'])
@pytest.mark.parametrize('delta', [0, 2])
@pytest.mark.parametrize('cmvn', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%dx%dx%dx%g' % s)
def test_pool_matches_reference(shape, cmvn, delta, full, dtype):
    from mercury_amd.data.augment import CMVN_VAR_FLOOR
    r = _recipe(shape, full, cmvn=cmvn, delta=delta)
    raw = dataclasses.replace(r, cmvn=0, delta=0, norm=None)
    pool, params, x, bank = _build(shape[2], dtype, r)
    assert bool((pool[..., 1:].contiguous().view(torch.int16) == 0).all())      # +0
    s = r._mel_fb().sum(0).clamp(min=1.0)
    E = 2e-3 * ((r._dct_mat().abs() * s.view(-1, 1)).sum(0) if r.dct else s).view(-1, 1)
    worst, smin = -math.inf, math.inf
    for i in range(P):
        p = params[i].tolist()
        ref = r.reference(x[i], bank, p, dtype=torch.float64)[:, :, 0]
        v = raw.reference(x[i], bank, p[:6] + [0.0] * 10, dtype=torch.float64)[:, :, 0]
        var = v.var(1, unbiased=False, keepdim=True)
        sr = (var + CMVN_VAR_FLOOR).sqrt() if cmvn == 2 else torch.ones_like(var)
        z = (v - v.mean(1, keepdim=True)) / sr
        bound = abs(r.affine()[0]) * (2 + z.abs()) * E / sr
        bound = 2.0 ** -8 * ref.abs() + torch.cat([bound * (3.0 / (2 * r.dwin + 1)) ** k for k in range(delta + 1)])
        worst = max(worst, float(((pool[i, :, :, 0].double() - ref).abs() - bound).max()))
        smin = min([smin] + (var + CMVN_VAR_FLOOR).sqrt()[var > 1e-20].tolist())
    print('%s cmvn=%d delta=%d full=%d %s: worst err - bound = %.3g, least s_r = %.3g'
          % (shape, cmvn, delta, full, dtype, worst, smin))
    assert worst <= 0


def test_chunk_counts_and_runs_are_bit_equal_and_the_graph_replays():
    from mercury_amd import ops
    shape = (200, 100, 16000, 40, 13, 0.0)
    r = _recipe(shape, True, cmvn=2, delta=2)
    want, _, x, bank = _build(16000, torch.int16, r, chunks=11)       # one tile per block
    for chunks in (0, 3, 11):       # the rule's 11 tiles in 6 | the fewest chunks that fit | again
        got = _build(16000, torch.int16, r, chunks=chunks)[0]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), chunks
    pool = torch.zeros(P, *r.out_hw(16000), 8, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.zeros(P, dtype=torch.int32, device=DEV) for _ in range(2))
    xd, bd = x.to(DEV), bank.to(DEV)
    ld, ctrl = (torch.zeros(n, dtype=torch.int64, device=DEV) for n in (P, 4))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pool_build(xd, ld, ctrl, pool, pl, pi, P, P, SEED, shuffle=False, recipe=r, noise=bd)
    for _ in range(3):
        pool.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pool.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('bad, msg', [
    (dict(cmvn=3), 'cmvn must be'), (dict(cmvn=-1), 'cmvn must be'),
    (dict(mel=0, mel_tab=0, mel_floats=0, krange=[]), 'cmvn needs mel'),
    (dict(feat_floats=5 * 8 * 2048 - 1), 'workspace holds'), (dict(feat=0), 'workspace holds'),
    (dict(P=1 << 16), r'below 2\^32 bytes'), (dict(L=16 * 2048, Ns=1), 'within 2048 frames')])
def test_launcher_refusals_launch_nothing(bad, msg):
    from mercury_amd import ops
    from mercury_amd.ops import importance, ptr
    r = _recipe((16, 16, 32704, 8, 0, 0.0), False, cmvn=2)    # T = 2045 frames: Tp = 2048, the most
    xd = torch.zeros(2, 32784, dtype=torch.int16, device=DEV)
    pool = torch.full((P, 8, 2050, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    feat = torch.full((P, 8, 2052), SENTINEL, device=DEV)
    z = torch.zeros(2, P, dtype=torch.int32, device=DEV)
    ld, ctrl = (torch.zeros(n, dtype=torch.int64, device=DEV) for n in (2, 4))
    tab = importance.pool_wave_table(r, DEV)
    mtab, _, krange = importance.pool_mel_tables(r, DEV)
    kw = dict(shard=ptr(xd), tab=ptr(tab), tab_floats=tab.numel(), labels=ptr(ld), ctrl=ptr(ctrl),
              pool=ptr(pool), pool_label=ptr(z[0]), pool_index=ptr(z[1]), stream=0, f32=0, Ns=2,
              L=32704, n_fft=16, hop=16, P=P, batch=P, augment=1, shuffle=1, seed=1, eps=1e-6,
              mel=8, mel_tab=ptr(mtab), mel_floats=mtab.numel(), krange=krange, cmvn=2,
              feat=ptr(feat), feat_floats=P * 8 * 2048)
    with pytest.raises(ValueError, match=msg):
        ops.lib().pool_wave(**dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all()) and bool((feat == SENTINEL).all())
