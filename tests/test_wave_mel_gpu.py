"""Log-mel and MFCC pools on the GPU (``pool_wave_mel_kernel``): the pool's bf16 value against
``WaveRecipe.reference`` in fp64, fed with the dumped draws.  Tolerance: the linear kernel's ``2^-8
|ref| + 2e-3 |a|`` means ``|dp_k| <= 2e-3 (p_k + eps)`` per bin; a band sums non-negative terms
against one ``eps`` and the DCT weighs bands by ``|D[m][j]|``, so ``2e-3 |a|`` is scaled by ``max(1,
s_m)``, ``s_m = sum_k fb[k][m]``, for log-mel and by ``sum_m |D[m][j]| max(1, s_m)`` for MFCC."""
import dataclasses
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 7.0
P, B, NS, SEED = 48, 8, 20, 11
# (n_fft, hop, L, mel, dct): 5-bin tail tile, 8-band mel tail, two chunks with a partial last |
# 13-column DCT tail, K ranges that skip | empty low bands: ln(eps) | largest K, 17 bin tiles on
# 4 waves, widest panel | W % 4 != 0, one tile of everything, dct = mel
SHAPES = [(200, 100, 3300, 40, 0), (200, 100, 3300, 80, 13), (64, 16, 512, 20, 0),
          (512, 128, 2048, 128, 40), (30, 7, 300, 8, 8)]
FULL = dict(shift=1, gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), tmask=(2, 3), fill=-1.5)
_CLIPS = {}


def _recipe(shape, full):
    from mercury_amd.data.augment import WaveRecipe
    W, hop, _, mel, dct = shape
    kw = dict(FULL, shift=W, fmask=(0, 0) if dct else (2, 3)) if full else {}
    return WaveRecipe(n_fft=W, hop=hop, mel=mel, dct=dct, **kw)


def _clips(L, dtype):
    """(shard, noise bank, labels): white noise, clip 1 a full-scale off-bin tone, 2 zero, 3 1e-3"""
    if (L, dtype) not in _CLIPS:
        g = torch.Generator().manual_seed(L)
        x = 0.3 * torch.randn(NS, L, generator=g)
        x[1] = 0.999 * torch.sin(2 * math.pi * 0.1037 * torch.arange(L))
        x[2] = 0
        x[3] *= 1e-3 / 0.3
        bank = 0.3 * torch.randn(3, L + 37, generator=g)
        if dtype == torch.int16:
            x, bank = ((t.clamp(-1, 1) * 32767).round().to(torch.int16) for t in (x, bank))
        _CLIPS[L, dtype] = (x, bank, (torch.arange(NS) * 7) % 30)
    return _CLIPS[L, dtype]


def _build(x, bank, labels, recipe, pc=0, **kw):
    """One pool build between two guard slots -> (pool, labels, indices, params) on the host."""
    from mercury_amd import ops
    R, T = recipe.out_hw(x.shape[1])
    ctrl = torch.tensor([pc, 0, 0, 0], device=DEV)
    big = torch.full((P + 2, R, T, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.full((P,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    params = torch.full((P + 2, 16), -99.0, device=DEV)
    ops.pool_build(x.to(DEV), labels.to(DEV), ctrl, big[1:P + 1], pl, pi, P, B, SEED,
                      recipe=recipe, params=params[1:P + 1],
                      noise=bank.to(DEV) if recipe.noise else None, **kw)
    torch.cuda.synchronize()
    big, params = big.cpu(), params.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    assert bool((params[0] == -99).all()) and bool((params[-1] == -99).all())
    return big[1:P + 1], pl.cpu(), pi.cpu(), params[1:P + 1]


@pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
@pytest.mark.parametrize('full', [False, True], ids=['identity', 'full'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%dx%dx%d' % s)
def test_pool_matches_reference(shape, full, dtype):
    r = _recipe(shape, full)
    x, bank, labels = _clips(shape[2], dtype)
    pool, pl, pi, params = _build(x, bank, labels, r, pc=2)
    assert torch.equal(pl.long(), labels[pi.long()]) and set(pi.tolist()) >= {1, 2, 3}
    assert bool((pool[..., 1:].contiguous().view(torch.int16) == 0).all())      # +0
    row = torch.tensor(r.identity_params()).expand(P, 16)
    assert torch.equal(_build(x, bank, labels, r, pc=2, augment=False)[3], row)
    assert torch.equal(params, row) != full
    s = r._mel_fb().sum(0).clamp(min=1.0)                                       # max(1, s_m)
    scale = (r._dct_mat().abs() * s.view(-1, 1)).sum(0) if r.dct else s
    worst = -math.inf
    for i in range(P):
        ref = r.reference(x[int(pi[i])], bank, params[i].tolist(), dtype=torch.float64)[:, :, 0]
        err = (pool[i, :, :, 0].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2e-3 * abs(r.affine()[0]) * scale.view(-1, 1)
        worst = max(worst, float((err - bound).max()))
    print('%s full=%d %s: worst err - bound = %.3g' % (shape, full, dtype, worst))
    assert worst <= 0


@pytest.mark.parametrize('shape', SHAPES[:2], ids=lambda s: '%dx%dx%dx%dx%d' % s)
def test_identity_determinism_and_graph_replay(shape):
    from mercury_amd import ops
    x, bank, labels = _clips(shape[2], torch.int16)
    full = _recipe(shape, True)
    ident = dataclasses.replace(full, shift=0, gain=None, noise=None, fmask=(0, 0), tmask=(0, 0))
    off, want = _build(x, bank, labels, full, augment=False), _build(x, bank, labels, ident)
    assert torch.equal(off[0].view(torch.int16), want[0].view(torch.int16))
    assert all(torch.equal(a, b) for a, b in zip(off[1:], want[1:]))
    eager, again = _build(x, bank, labels, full, pc=1), _build(x, bank, labels, full, pc=1)
    assert torch.equal(eager[0].view(torch.int16), again[0].view(torch.int16))
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
        assert torch.equal(pi.cpu(), eager[2])


@pytest.mark.parametrize('bad, msg', [
    (dict(mel_floats=272 * 128 - 1), 'mel table holds'), (dict(mel=7), 'mel must be'),
    (dict(mel=129), 'mel must be'), (dict(dct=129, dct_tab=8, dct_floats=128 * 144), 'dct must be'),
    (dict(chunks=1), 'LDS')])
def test_launcher_refusals_launch_nothing(bad, msg):
    from mercury_amd.data.augment import WaveRecipe
    from mercury_amd import ops
    from mercury_amd.ops import importance, ptr
    r = WaveRecipe(n_fft=512, hop=128, mel=128)
    x, _, labels = _clips(4096, torch.int16)             # T = 33: 3 frame tiles, one chunk = 79 KB
    xd, ld = x.to(DEV), labels.to(DEV)
    pool = torch.full((P, 129, 33, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(2, P, dtype=torch.int32, device=DEV)
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    tab = importance.pool_wave_table(r, DEV)
    mtab, _, krange = importance.pool_mel_tables(r, DEV)
    kw = dict(shard=ptr(xd), tab=ptr(tab), tab_floats=tab.numel(), labels=ptr(ld), ctrl=ptr(ctrl),
              pool=ptr(pool), pool_label=ptr(z[0]), pool_index=ptr(z[1]), stream=0, f32=0, Ns=NS,
              L=4096, n_fft=512, hop=128, P=P, batch=B, augment=1, shuffle=1, seed=1, eps=1e-6,
              mel=128, mel_tab=ptr(mtab), mel_floats=mtab.numel(), krange=krange)
    with pytest.raises(ValueError, match=msg):
        ops.lib().pool_wave(**dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all())


class _Loader(SimpleNamespace):
    def __len__(self):
        return 1


def test_trainer_takes_a_mel_recipe():
    from mercury_amd.collab import make_trainer
    from mercury_amd.config import Config
    from mercury_amd.engine.native import NativeTrainer
    from mercury_amd import ops
    from mercury_amd.models.vgg import VGG
    g = torch.Generator().manual_seed(5)
    x = (0.3 * torch.randn(64, 16000, generator=g) * 32767).round().to(torch.int16).numpy()
    y = (np.arange(64) * 7) % 30
    torch.manual_seed(0)
    net = VGG('VGG11', 30, in_features=5120).to(DEV)
    loader = _Loader(batch_size=32, dataset=SimpleNamespace(data=x, target=y, noise=None,
                                                           transform=None))
    cfg = Config(print_every=0, eval_every=0, use_graphs=False, presample_batches=2,
                 augment='wave:nfft=200,hop=100,mel=64,shift=1600,gain=0.8:1.2,tmask=2x20')
    tr = make_trainer(cfg, net, torch.optim.Adam(net.parameters(), lr=1e-3), loader, loader,
                      loader, DEV)
    try:
        assert isinstance(tr, NativeTrainer)
        e = tr.engine
        assert (e.H, e.W) == (64, 161) and e.augment.mel == 64
        e.prime()
        torch.cuda.synchronize()
        sm = e.score_mode
        ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
        pool, pl, pi = (torch.empty_like(t) for t in (sm.input, sm.label, sm.index))
        ops.pool_build(e.shard, e.shard_labels, ctrl, pool, pl, pi, 64, 32, e.seed,
                          recipe=e.augment)
        assert torch.equal(pool.view(torch.int16), sm.input.view(torch.int16))
        assert torch.equal(pi, sm.index) and len(set(e.aug_params[:, 0].tolist())) > 1
        e.step()
        torch.cuda.synchronize()
        m = e.read_meters()
        assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
        out = tr.evaluate()
        assert math.isfinite(out[2].average) and out[2].count == 64
    finally:
        tr.engine.close()
