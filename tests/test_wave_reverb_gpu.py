"""Room-impulse reverberation in the waveform pools (``pool_reverb_kernel``, ``csrc/pool_reverb.hip``,
and the slot-indexed route of the wave kernels behind it): the pre-pass's workspace against the
fp64 convolution under the derived bound ``gamma_n (|h| conv |x|)[i]``, ``n = K + 16``, ``u =
2^-24``, which holds for any summation order; the pool as the exact composition of the workspace
and the recipe without reverb; the pool against ``WaveRecipe.reference`` under the unchanged
bounds of ``test_wave_gpu.py``, ``test_wave_mel_gpu.py`` and ``test_wave_delta_gpu.py`` (``2^-8
|ref| + 2e-3 |a| S_r g^k``; ``test_wave_reverb.py`` carries them over); bit-equality over chunk
counts, runs and graph replays, and the launcher's refusals."""
import dataclasses
import math

import pytest
import torch

from test_wave_reverb import NS, clips, rirs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 7.0
P, B, SEED = 48, 8, 11
DTYPES = pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
FULL = dict(shift=200, gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), tmask=(2, 3), fill=-1.5)
# (n_fft, hop, L, K, recipe fields)
ROUTES = {'linear': (200, 100, 3300, 257, dict(shift=200)),
          'mfcc-delta': (200, 100, 3300, 257, dict(shift=200, mel=80, dct=13, delta=2)),
          'w30-speed': (30, 7, 300, 5, dict(shift=30, mel=8, dct=8, speed=(0.9, 1.1))),
          'cmvn': (200, 100, 3300, 257, dict(mel=80, cmvn=2)),
          'full': (200, 100, 3300, 257, dict(FULL, fmask=(2, 3)))}


def _recipe(route, reverb=0.5):
    from mercury_amd.data.augment import WaveRecipe
    W, hop, L, K, kw = ROUTES[route]
    return WaveRecipe(n_fft=W, hop=hop, reverb=reverb, **kw), L, K


def _build(x, bank, labels, recipe, rir=None, augment=True, rev_chunks=0):
    """One pool build between two guard slots -> (pool, indices, params, workspace) on the host."""
    from mercury_amd.ops.importance import _pool_wave, pool_reverb_workspace
    L = x.shape[1]
    ctrl = torch.tensor([4, 0, 0, 0], device=DEV)      # batches 24..29 of 8 per epoch: one epoch
    big = torch.full((P + 2, *recipe.out_hw(L), 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.full((P,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    params = torch.full((P, 16), -99.0, device=DEV)
    _pool_wave(x.to(DEV), bank.to(DEV) if recipe.noise else None, labels.to(DEV), ctrl,
               big[1:P + 1], pl, pi, P, B, SEED, augment, True, None, recipe, params,
               rir=None if rir is None else rir.to(DEV), rev_chunks=rev_chunks)
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    rev = pool_reverb_workspace(P, L, DEV).cpu() if recipe.reverb and augment else None
    return big[1:P + 1], pi.cpu(), params.cpu(), rev


def _f32(t):
    return t.float() / 32768 if t.dtype == torch.int16 else t


@DTYPES
@pytest.mark.parametrize('L, K', [(300, 5), (3300, 257), (2048, 4096)])
def test_workspace_matches_fp64_convolution(L, K, dtype):
    from mercury_amd.data.augment import WaveRecipe, reverb_convolve
    x, bank, labels = clips(L, dtype)
    h = rirs(K)
    _, pi, params, rev = _build(x, bank, labels, WaveRecipe(n_fft=30, hop=7, reverb=0.5), h)
    on = params[:, 15]
    assert bool((on == 0).any()) and len(set(on[on > 0].tolist())) > 1 and float(on.max()) <= 3
    gamma = (K + 16) * 2.0 ** -24 / (1 - (K + 16) * 2.0 ** -24)
    worst = -math.inf
    for i in range(P):
        xi = _f32(x[int(pi[i])])
        if on[i] == 0:
            assert torch.equal(rev[i].view(torch.int32), xi.view(torch.int32))
            continue
        hk = h[int(on[i]) - 1]
        err = (rev[i].double() - reverb_convolve(xi, hk)).abs()
        worst = max(worst, float((err - gamma * reverb_convolve(xi.abs(), hk.abs())).max()))
    print('L=%d K=%d %s: worst err - bound = %.3g' % (L, K, dtype, worst))
    assert worst <= 0


@DTYPES
@pytest.mark.parametrize('route', list(ROUTES))
def test_pool_is_the_recipe_without_reverb_on_the_workspace(route, dtype):
    r, L, K = _recipe(route)
    x, bank, labels = clips(L, dtype)
    pool, pi, params, rev = _build(x, bank, labels, r, rirs(K))
    assert len(set(pi.tolist())) == P                     # distinct sources: one row per slot
    shard = torch.zeros(NS, L)
    shard[pi.long()] = rev
    want = _build(shard, _f32(bank), labels, dataclasses.replace(r, reverb=0.0))
    assert torch.equal(pool.view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(pi, want[1]) and torch.equal(params[:, :15], want[2][:, :15])
    assert bool((params[:, 15] > 0).any()) and bool((want[2][:, 15] == 0).all())


@DTYPES
@pytest.mark.parametrize('route', ['linear', 'mfcc-delta'])
def test_pool_matches_reference(route, dtype):
    r, L, K = _recipe(route)
    r = dataclasses.replace(r, **FULL)
    x, bank, labels = clips(L, dtype)
    h = rirs(K)
    pool, pi, params, _ = _build(x, bank, labels, r, h)
    scale = torch.ones(r.out_hw(L)[0], dtype=torch.float64)
    if r.mel:
        scale = (r._dct_mat().abs() * r._mel_fb().sum(0).clamp(min=1.0).view(-1, 1)).sum(0)
        scale = torch.cat([scale * (3.0 / (2 * r.dwin + 1)) ** k for k in range(r.delta + 1)])
    worst = -math.inf
    for i in range(P):
        ref = r.reference(x[int(pi[i])], bank, params[i].tolist(), dtype=torch.float64,
                          rir=h)[:, :, 0]
        err = (pool[i, :, :, 0].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2e-3 * abs(r.affine()[0]) * scale.view(-1, 1)
        worst = max(worst, float((err - bound).max()))
    print('%s %s: worst err - bound = %.3g' % (route, dtype, worst))
    assert bool((params[:, 15] > 0).any()) and worst <= 0


def test_chunk_counts_runs_and_graph_replays_are_bit_equal():
    from mercury_amd.ops.importance import _pool_wave, pool_noise_f32, pool_reverb_workspace
    r, L, K = _recipe('full')
    x, bank, labels = clips(L, torch.int16)
    h = rirs(K)
    pool, pi, params, rev = _build(x, bank, labels, r, h)
    for n in (0, 1, 2, 5, 13):                            # 13 tiles: 13, 7, 3 and 1 per block
        got = _build(x, bank, labels, r, h, rev_chunks=n)
        assert torch.equal(got[3].view(torch.int32), rev.view(torch.int32)), n
        assert torch.equal(got[0].view(torch.int16), pool.view(torch.int16)), n
    off = _build(x, bank, labels, r, h, augment=False)
    want = _build(x, bank, labels, dataclasses.replace(r, reverb=0.0), augment=False)
    assert torch.equal(off[0].view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(off[2], want[2])
    ctrl = torch.tensor([4, 0, 0, 0], device=DEV)
    out = torch.zeros(P, *r.out_hw(L), 8, dtype=torch.bfloat16, device=DEV)
    pl, pd = (torch.zeros(P, dtype=torch.int32, device=DEV) for _ in range(2))
    xd, bd, ld, hd = x.to(DEV), bank.to(DEV), labels.to(DEV), h.to(DEV)
    ws = pool_reverb_workspace(P, L, DEV)
    pool_noise_f32(bd)                                    # (made outside the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _pool_wave(xd, bd, ld, ctrl, out, pl, pd, P, B, SEED, True, True, None, r, None, rir=hd)
    for _ in range(3):
        out.fill_(SENTINEL)
        ws.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int16), pool.view(torch.int16))
        assert torch.equal(ws.cpu().view(torch.int32), rev.view(torch.int32))


@pytest.mark.parametrize('bad, msg', [
    (dict(rev=0), 'workspace holds'), (dict(rev_floats=P * 3300 - 1), 'workspace holds'),
    (dict(rev=8), 'workspace holds'), (dict(rir=0), 'RIR bank holds'),
    (dict(rir_floats=3 * 257 + 1), 'RIR bank holds'), (dict(rir_k=4097), 'K <= 4096'),
    (dict(rir_k=0), 'K <= 4096'), (dict(reverb_p=0.0), r'p must lie'),
    (dict(reverb_p=1.5), r'p must lie'), (dict(rev_chunks=14), 'reverb chunks'),
    (dict(Nr=1 << 18, rir_k=4096, rir_floats=1 << 30), r'below 2\^32 bytes'),
    (dict(L=32000, Ns=1, rev_floats=P * 32000, rir_k=4096, rir_floats=3 * 4096, rev_chunks=1),
     'LDS')])
def test_launcher_refusals_launch_nothing(bad, msg):
    from mercury_amd import ops
    from mercury_amd.ops import importance, ptr
    r, L, K = _recipe('linear')
    xd = torch.zeros(10, 3300, dtype=torch.int16, device=DEV)     # (room for L = 32000, Ns = 1)
    pool = torch.full((P, 101, 321, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    rev = torch.full((P, 32000), SENTINEL, device=DEV)
    hd = torch.zeros(3, 4096, device=DEV)
    z = torch.zeros(2, P, dtype=torch.int32, device=DEV)
    ld, ctrl = (torch.zeros(n, dtype=torch.int64, device=DEV) for n in (10, 4))
    tab = importance.pool_wave_table(r, DEV)
    kw = dict(shard=ptr(xd), tab=ptr(tab), tab_floats=tab.numel(), labels=ptr(ld), ctrl=ptr(ctrl),
              pool=ptr(pool), pool_label=ptr(z[0]), pool_index=ptr(z[1]), stream=0, f32=0, Ns=10,
              L=L, n_fft=200, hop=100, P=P, batch=B, augment=1, shuffle=1, seed=1, eps=1e-6,
              reverb_p=0.5, rir=ptr(hd), rir_floats=3 * K, Nr=3, rir_k=K, rev=ptr(rev),
              rev_floats=P * L)
    with pytest.raises(ValueError, match=msg):
        ops.lib().pool_wave(**dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all()) and bool((rev == SENTINEL).all())
