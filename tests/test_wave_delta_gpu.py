"""Delta and delta-delta rows of the log-mel / MFCC pools (``pool_wave_mel_kernel<.., DELTA>``):
the pool's bf16 value against ``WaveRecipe.reference`` in fp64, fed with the dumped draws.
Tolerance: the static rows keep ``tests/test_wave_mel_gpu.py``'s bound ``2^-8 |ref| + 2e-3 |a|
S_r``; a delta row is a linear combination of static values whose weights sum in magnitude to ``g
= sum_n 2n / (2 sum_n n^2) = 3 / (2N + 1)``, so rows of order k get ``2^-8 |ref| + 2e-3 |a| g^k
S_r``."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_wave_mel_gpu import B, DEV, NS, P, SEED, SENTINEL, _clips, _Loader      # the helpers

pytestmark = pytest.mark.gpu

# (n_fft, hop, L, mel, dct): MFCC, 3 frame tiles with a 2-frame tail | log-mel with frequency
# masks | one wave, odd hop, dct = mel | T = 2: every clamp active
SHAPES = [(200, 100, 3300, 80, 13), (200, 100, 3300, 40, 0), (30, 7, 300, 8, 8), (16, 16, 24, 8, 0)]


def _recipe(shape, full, **kw):
    from mercury_amd.data.augment import WaveRecipe
    W, hop, L, mel, dct = shape
    if full:
        kw.update(shift=W, gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), fill=-1.5,
                  tmask=(2, min(3, 1 + L // hop)), fmask=(0, 0) if dct else (2, 3),
                  lifter=22 if dct else 0)
    return WaveRecipe(n_fft=W, hop=hop, mel=mel, dct=dct, **kw)


def _build(x, bank, labels, recipe, pc=0, chunks=0):
    """One pool build between two guard slots -> (pool, indices, params) on the host."""
    from mercury_amd.ops.importance import _pool_wave
    R, T = recipe.out_hw(x.shape[1])
    ctrl = torch.tensor([pc, 0, 0, 0], device=DEV)
    big = torch.full((P + 2, R, T, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.full((P,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    params = torch.full((P, 16), -99.0, device=DEV)
    _pool_wave(x.to(DEV), bank.to(DEV) if recipe.noise else None, labels.to(DEV), ctrl,
               big[1:P + 1], pl, pi, P, B, SEED, True, True, None, recipe, params, chunks=chunks)
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    return big[1:P + 1], pi.cpu(), params.cpu()


@pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
@pytest.mark.parametrize('full', [False, True], ids=['identity', 'full'])
@pytest.mark.parametrize('N', [1, 2])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%dx%dx%d' % s)
def test_pool_matches_reference(shape, order, N, full, dtype):
    r = _recipe(shape, full, delta=order, dwin=N)
    x, bank, labels = _clips(shape[2], dtype)
    pool, pi, params = _build(x, bank, labels, r, pc=2)
    assert set(pi.tolist()) >= {1, 2, 3}
    assert bool((pool[..., 1:].contiguous().view(torch.int16) == 0).all())      # +0
    assert torch.equal(params, torch.tensor(r.identity_params()).expand(P, 16)) != full
    s = r._mel_fb().sum(0).clamp(min=1.0)                                       # max(1, s_m)
    scale = (r._dct_mat().abs() * s.view(-1, 1)).sum(0) if r.dct else s
    scale = torch.cat([scale * (3.0 / (2 * N + 1)) ** k for k in range(order + 1)])
    worst = -math.inf
    for i in range(P):
        ref = r.reference(x[int(pi[i])], bank, params[i].tolist(), dtype=torch.float64)[:, :, 0]
        err = (pool[i, :, :, 0].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2e-3 * abs(r.affine()[0]) * scale.view(-1, 1)
        worst = max(worst, float((err - bound).max()))
    print('%s delta=%d N=%d full=%d %s: worst err - bound = %.3g'
          % (shape, order, N, full, dtype, worst))
    assert worst <= 0


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]], ids=lambda s: '%dx%dx%dx%dx%d' % s)
def test_pools_of_different_chunk_counts_are_bit_equal(shape):
    """one block per slot, the rule's choice (two), and one owned tile per block (three)"""
    r = _recipe(shape, True, delta=2, dwin=2)
    x, bank, labels = _clips(shape[2], torch.int16)
    want = _build(x, bank, labels, r, pc=1, chunks=1)[0].view(torch.int16)
    assert (r.out_hw(shape[2])[1] + 15) // 16 == 3
    for chunks in (0, 3):
        got = _build(x, bank, labels, r, pc=1, chunks=chunks)[0].view(torch.int16)
        assert torch.equal(got, want), chunks


def test_delta_off_determinism_and_graph_replay():
    from mercury_amd import ops
    from mercury_amd.data.augment import WaveRecipe
    shape = SHAPES[0]
    x, bank, labels = _clips(shape[2], torch.int16)
    old = WaveRecipe(n_fft=200, hop=100, mel=80, dct=13, shift=200, tmask=(2, 3))
    new = _recipe(shape, False, shift=200, tmask=(2, 3), delta=0, dwin=3)
    a, b = _build(x, bank, labels, old, pc=1), _build(x, bank, labels, new, pc=1)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[2], b[2])
    full = _recipe(shape, True, delta=2, dwin=2)
    eager, again = _build(x, bank, labels, full, pc=1), _build(x, bank, labels, full, pc=1)
    assert torch.equal(eager[0].view(torch.int16), again[0].view(torch.int16))
    static = _build(x, bank, labels, _recipe(shape, True), pc=1)[0]    # the delta = 0 pool
    assert torch.equal(eager[0][:, :13].contiguous().view(torch.int16), static.view(torch.int16))
    ctrl = torch.tensor([1, 0, 0, 0], device=DEV)
    pool = torch.zeros(P, *full.out_hw(shape[2]), 8, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.zeros(P, dtype=torch.int32, device=DEV) for _ in range(2))
    xd, bd, ld = x.to(DEV), bank.to(DEV), labels.to(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pool_build(xd, ld, ctrl, pool, pl, pi, P, B, SEED, recipe=full, noise=bd)
    for _ in range(2):
        pool.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pool.cpu().view(torch.int16), eager[0].view(torch.int16))
        assert torch.equal(pi.cpu(), eager[1])


@pytest.mark.parametrize('bad, msg', [
    (dict(delta=3), 'delta must be'), (dict(delta=-1), 'delta must be'),
    (dict(delta=1, dwin=0), 'dwin must be'), (dict(delta=1, dwin=5), 'dwin must be'),
    (dict(delta=1, mel=0, mel_tab=0, mel_floats=0, krange=[]), 'delta needs mel'),
    (dict(delta=2, chunks=1), 'LDS')])
def test_launcher_refusals_launch_nothing(bad, msg):
    from mercury_amd.data.augment import WaveRecipe
    from mercury_amd import ops
    from mercury_amd.ops import importance, ptr
    r = WaveRecipe(n_fft=200, hop=100, mel=80)
    x, _, labels = _clips(16000, torch.int16)            # T = 161: one chunk of 11 tiles > 64 KB
    xd, ld = x.to(DEV), labels.to(DEV)
    pool = torch.full((P, 3 * 101, 161, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(2, P, dtype=torch.int32, device=DEV)
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    tab = importance.pool_wave_table(r, DEV)
    mtab, _, krange = importance.pool_mel_tables(r, DEV)
    kw = dict(shard=ptr(xd), tab=ptr(tab), tab_floats=tab.numel(), labels=ptr(ld), ctrl=ptr(ctrl),
              pool=ptr(pool), pool_label=ptr(z[0]), pool_index=ptr(z[1]), stream=0, f32=0, Ns=NS,
              L=16000, n_fft=200, hop=100, P=P, batch=B, augment=1, shuffle=1, seed=1, eps=1e-6,
              mel=80, mel_tab=ptr(mtab), mel_floats=mtab.numel(), krange=krange)
    with pytest.raises(ValueError, match=msg):
        ops.lib().pool_wave(**dict(kw, **bad))
    with pytest.raises(ValueError, match='pool must be'):                # rows != (1 + delta) R
        ops.pool_build(xd, ld, ctrl, pool[:, :160], z[0], z[1], P, B, SEED,
                       recipe=WaveRecipe(n_fft=200, hop=100, mel=80, delta=2))
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all())


def test_trainer_takes_a_delta_recipe():
    from mercury_amd.collab import make_trainer
    from mercury_amd.config import Config
    from mercury_amd.engine.native import NativeTrainer
    from mercury_amd.models.vgg import VGG
    g = torch.Generator().manual_seed(5)
    x = (0.3 * torch.randn(64, 16000, generator=g) * 32767).round().to(torch.int16).numpy()
    y = (np.arange(64) * 7) % 30
    torch.manual_seed(0)
    net = VGG('VGG11', 30, in_features=512 * (39 // 32) * (161 // 32)).to(DEV)
    loader = _Loader(batch_size=32, dataset=SimpleNamespace(data=x, target=y, noise=None,
                                                           transform=None))
    cfg = Config(print_every=0, eval_every=0, use_graphs=False, presample_batches=2,
                 augment='wave:nfft=200,hop=100,mel=40,dct=13,delta=2,shift=1600,tmask=2x20')
    tr = make_trainer(cfg, net, torch.optim.Adam(net.parameters(), lr=1e-3), loader, loader,
                      loader, DEV)
    try:
        assert isinstance(tr, NativeTrainer)
        e = tr.engine
        assert (e.H, e.W) == (39, 161) and e.augment.delta == 2
        e.prime()
        e.step()
        torch.cuda.synchronize()
        m = e.read_meters()
        assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
    finally:
        tr.engine.close()
