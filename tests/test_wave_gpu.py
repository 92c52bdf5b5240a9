"""Waveform pools on the GPU (``pool_wave_kernel``) against ``WaveRecipe.reference`` (fp64, one
rounding to bf16) fed with the draws the kernel dumped and the shard indices it wrote.  The pool's bf16 value is
compared with the reference's fp64 value, so the pool's one rounding is inside the bound.

Tolerance, every element: ``2^-8 |ref| + 2e-3 |a|`` -- one bf16 ulp of the stored value plus the
fp32 accumulation of the DFT ahead of the log (``a = 1/std``)."""
import dataclasses
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sampler_oracles import philox4x32, u01

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 7.0
P, B, NS, SEED = 48, 8, 20, 11
# T = 11, a 5-bin tail tile | a 2-frame tail | a one-bin tail tile | the largest K | W % 4 != 0;
# at P = 48 the launcher gives the 2nd, 3rd and 5th shape two frame chunks, the last one partial
SHAPES = [(200, 100, 1000), (200, 100, 3300), (64, 16, 512), (512, 128, 2048), (30, 7, 300)]
RECIPES = {        # name -> (recipe fields but n_fft / hop (shift in units of W), Ln - L or None)
    'identity': (dict(), None),
    'shiftgain': (dict(shift=1, gain=(0.5, 2.0)), None),
    'noise0': (dict(noise=(0.7, 0.5)), 0),
    'noise37': (dict(noise=(0.7, 0.5)), 37),
    'full': (dict(shift=1, gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), fmask=(2, 3),
                  tmask=(2, 3), fill=-1.5), 37),
}


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _recipe(W, hop, name):
    from mercury_amd.data.augment import WaveRecipe
    kw = dict(RECIPES[name][0])
    kw['shift'] = kw.get('shift', 0) * W
    return WaveRecipe(n_fft=W, hop=hop, **kw)


_CLIPS = {}


def _clips(L, dtype, extra):
    """(shard [NS][L], noise bank [3][L + extra] or None, labels): white noise, a full-scale
    off-bin tone (clip 1), an all-zero clip (2), a 1e-3-scale clip (3); made once, never
    written."""
    key = (L, dtype, extra)
    if key not in _CLIPS:
        g = torch.Generator().manual_seed(L)
        x = 0.3 * torch.randn(NS, L, generator=g)
        x[1] = 0.999 * torch.sin(2 * math.pi * 0.1037 * torch.arange(L))
        x[2] = 0
        x[3] *= 1e-3 / 0.3
        bank = None if extra is None else 0.3 * torch.randn(3, L + extra, generator=g)
        if dtype == torch.int16:
            x, bank = ((None if t is None else (t.clamp(-1, 1) * 32767).round().to(torch.int16))
                       for t in (x, bank))
        _CLIPS[key] = (x, bank, (torch.arange(NS) * 7) % 30)
    return _CLIPS[key]


def _build(x, bank, labels, recipe, pc=0, **kw):
    """One pool build between two guard slots -> (pool, labels, indices, params) on the host."""
    ops = _ops()
    F, T = recipe.out_hw(x.shape[1])
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = pc
    big = torch.full((P + 2, F, T, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pi = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    params = torch.full((P + 2, 16), -99.0, device=DEV)
    ops.pool_build(x.to(DEV), labels.to(DEV), ctrl, big[1:P + 1], pl, pi, P, B, SEED,
                   recipe=recipe, params=params[1:P + 1],
                   noise=None if bank is None else bank.to(DEV), **kw)
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    params = params.cpu()
    assert bool((params[0] == -99).all()) and bool((params[-1] == -99).all())
    return big[1:P + 1], pl.cpu(), pi.cpu(), params[1:P + 1]


def _replay(r, pc, L, bank):
    """[P][16] fp32: the documented stream words 0x5bec8..b of every slot, drawn as the class
    docstring says (gain is one fused multiply-add: product and sum are multiples of 2^-25 below
    4 for these recipes, so exact in fp64, then rounded once)."""
    slot = np.arange(P)
    gb = pc * (P // B) + slot // B
    w = [philox4x32((gb & 0xffffffff, gb >> 32, slot % B, 0x5bec8 + i), SEED, 0xA5A5A5A5)
         for i in range(4)]
    F, T = r.out_hw(L)
    out = np.zeros((P, 16), np.float32)
    out[:, 0] = (w[0][0] % np.uint64(2 * r.shift + 1)).astype(np.int64) - r.shift
    lo, hi = (np.float32(v) for v in (r.gain or (1.0, 1.0)))
    out[:, 1] = (np.float64(hi - lo) * u01(w[0][1]).astype(np.float64) + np.float64(lo))
    if r.noise is not None:
        on = u01(w[0][2]) < np.float32(r.noise[0])
        out[:, 2] = on
        out[:, 3] = np.where(on, w[0][3] % np.uint64(bank.shape[0]), 0)
        out[:, 4] = np.where(on, w[1][0] % np.uint64(bank.shape[1] - L + 1), 0)
        out[:, 5] = np.where(on, np.float32(r.noise[1]) * u01(w[1][1]), 0)
    wr, sr = (w[1][2], w[2][0], w[2][2], w[3][0]), (w[1][3], w[2][1], w[2][3], w[3][1])
    for m, ((n, mx), size) in enumerate(((r.fmask, F), (r.tmask, T))):
        for k in range(n):
            width = wr[2 * m + k] % np.uint64(mx + 1)
            out[:, 6 + 4 * m + 2 * k] = sr[2 * m + k] % (np.uint64(size + 1) - width)
            out[:, 7 + 4 * m + 2 * k] = width
    return torch.from_numpy(out)


@pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
@pytest.mark.parametrize('name', list(RECIPES))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_pool_matches_reference(shape, name, dtype):
    W, hop, L = shape
    r = _recipe(W, hop, name)
    x, bank, labels = _clips(L, dtype, RECIPES[name][1])
    pool, pl, pi, params = _build(x, bank, labels, r, pc=2)
    assert torch.equal(params, _replay(r, 2, L, bank))
    assert torch.equal(pl.long(), labels[pi.long()]) and set(pi.tolist()) >= {1, 2, 3}
    assert bool((pool[..., 1:].contiguous().view(torch.int16) == 0).all())      # +0
    if r.shift:     # the reflect padding mirrors shifted-in zeros in at least one slot
        assert bool((params[:, 0].abs() >= W // 2).any())
    if r.noise:
        assert 0 < int(params[:, 2].sum()) < P
    a = r.affine()[0]
    worst = -math.inf
    for s in range(P):
        # (the reference before its own rounding: against the rounded one a correct pool value
        # that rounds the other way is a whole ulp off, 2^-7 |ref| low in a binade)
        ref = r.reference(x[int(pi[s])], bank, params[s].tolist(), dtype=torch.float64)[:, :, 0]
        err = (pool[s, :, :, 0].double() - ref).abs()
        worst = max(worst, float((err - (2.0 ** -8 * ref.abs() + 2e-3 * abs(a))).max()))
    print('%s %s %s: worst err - bound = %.3g' % (shape, name, dtype, worst))
    assert worst <= 0


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]], ids=lambda s: '%dx%dx%d' % s)
def test_identity_determinism_and_graph_replay(shape):
    W, hop, L = shape
    x, bank, labels = _clips(L, torch.int16, 37)
    full = _recipe(W, hop, 'full')
    ident = dataclasses.replace(full, shift=0, gain=None, noise=None, fmask=(0, 0), tmask=(0, 0))
    off = _build(x, bank, labels, full, augment=False)
    want = _build(x, None, labels, ident)
    row = torch.zeros(P, 16)
    row[:, 1] = 1
    assert torch.equal(off[3], row) and torch.equal(want[3], row)
    assert torch.equal(off[0].view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(off[1], want[1]) and torch.equal(off[2], want[2])
    eager = _build(x, bank, labels, full, pc=1)
    again = _build(x, bank, labels, full, pc=1)
    assert torch.equal(eager[0].view(torch.int16), again[0].view(torch.int16))
    # captured: the same launch recorded once and replayed three times
    ops = _ops()
    F, T = full.out_hw(L)
    xd, bd, ld = x.to(DEV), bank.to(DEV), labels.to(DEV)
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = 1
    pool = torch.zeros(P, F, T, 8, dtype=torch.bfloat16, device=DEV)
    pl = torch.zeros(P, dtype=torch.int32, device=DEV)
    pi = torch.zeros(P, dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pool_build(xd, ld, ctrl, pool, pl, pi, P, B, SEED, recipe=full, noise=bd)
    for _ in range(3):
        pool.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pool.cpu().view(torch.int16), eager[0].view(torch.int16))
        assert torch.equal(pi.cpu(), eager[2])


def test_refusals_launch_nothing():
    from mercury_amd.data.augment import WaveRecipe
    ops = _ops()
    x, bank, labels = _clips(300, torch.int16, 37)

    def build(recipe, shard=x, noise=None, **kw):
        F, T = recipe.out_hw(shard.shape[1])
        pool = torch.full((P, F, T, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
        z = torch.zeros(P, dtype=torch.int32, device=DEV)
        ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
        try:
            ops.pool_build(shard, labels.to(DEV), ctrl, pool, z, z.clone(), P, B, SEED,
                           recipe=recipe, noise=noise, **kw)
        finally:
            torch.cuda.synchronize()
            assert bool((pool == SENTINEL).all())

    xd = x.to(DEV)
    with pytest.raises(ValueError, match='n_fft'):
        WaveRecipe(n_fft=31)
    with pytest.raises(ValueError, match='n_fft'):
        build(WaveRecipe(n_fft=512, hop=128), xd[:, :256].contiguous())              # L <= W / 2
    with pytest.raises(ValueError, match='noise'):
        build(WaveRecipe(n_fft=64, hop=16, noise=(1, 0.5)), xd)         # no bank
    with pytest.raises(ValueError, match='noise bank'):
        build(WaveRecipe(n_fft=64, hop=16, noise=(1, 0.5)), xd, bank.to(DEV)[:, :299].contiguous())
    with pytest.raises(ValueError, match='device'):
        build(WaveRecipe(n_fft=64, hop=16), x)                          # a CPU shard
    with pytest.raises(ValueError, match='WaveRecipe'):
        build(WaveRecipe(n_fft=64, hop=16), xd.double())
    # the launcher's own checks, reached past the Python ones (null pointers: nothing may launch)
    kw = dict(shard=8, tab=8, tab_floats=0, labels=8, ctrl=8, pool=8, pool_label=8, pool_index=8,
              stream=0, f32=0, Ns=4, L=300, n_fft=64, hop=16, P=P, batch=B, augment=1, shuffle=1,
              seed=1, eps=1e-6)
    for bad, msg in ((dict(n_fft=31), 'n_fft'), (dict(n_fft=1024), 'n_fft'),
                     (dict(L=32), 'L must exceed'), (dict(noise=8, Nn=1, Ln=299), 'noise bank'),
                     (dict(L=2 ** 29, Ns=8), '2\\^32'), (dict(), 'table'),
                     (dict(tab_floats=4 * 16 * 2 * 48, chunks=1, L=2 ** 20), 'LDS')):
        with pytest.raises(ValueError, match=msg):
            ops.lib().pool_wave(**dict(kw, **bad))


class _Loader(object):
    batch_size = 32

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return 1


def test_trainer_takes_a_waveform_dataset():
    """VGG11, 30 classes, 64 int16 clips of 16000 samples: 101 x 161 spectrograms."""
    from mercury_amd.collab import make_trainer
    from mercury_amd.config import Config
    from mercury_amd.data.augment import WaveRecipe
    from mercury_amd.data.transforms import WaveSpectrogram
    from mercury_amd.engine.native import NativeTrainer
    from mercury_amd.models import build_model
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = (0.3 * torch.randn(64, 16000, generator=g) * 32767).round().to(torch.int16).numpy()
    bank = (0.3 * torch.randn(3, 16037, generator=g) * 32767).round().to(torch.int16).numpy()
    y = (np.arange(64) * 7) % 30
    spec = 'wave:nfft=200,hop=100,shift=1600,gain=0.8:1.2,noise=0.8x0.1,norm=-5:4,fmask=2x10,' \
           'tmask=2x20'

    def trainer(transform=None, noise=bank, **kw):
        torch.manual_seed(0)
        net = build_model('vgg11', 30).to(DEV)
        train = _Loader(SimpleNamespace(data=x, target=y, noise=noise, transform=transform))
        test = _Loader(SimpleNamespace(data=x[:32], target=y[:32], transform=None))
        cfg = Config(print_every=0, eval_every=0, use_graphs=False, presample_batches=2, **kw)
        return make_trainer(cfg, net, torch.optim.Adam(net.parameters(), lr=1e-3), train, train,
                            test, DEV)

    with pytest.raises(ValueError, match='wave recipe'):
        trainer()                                   # [N][L] without a wave recipe
    with pytest.raises(ValueError, match='noise'):
        trainer(noise=None, augment=spec)           # a noise= recipe without a bank
    for transform, kw in ((None, dict(augment=spec)),
                          (WaveSpectrogram(spec, noise=bank), dict(augment='dataset'))):
        tr = trainer(transform, bank if transform is None else None, **kw)   # (or its transform's)
        try:
            assert isinstance(tr, NativeTrainer)
            e = tr.engine
            assert e.augment == WaveRecipe.parse(spec) and (e.H, e.W) == (101, 161)
            assert e.shard.dtype == torch.int16 and tuple(e.shard.shape) == (64, 16000)
            assert e.aug_params.shape == (64, 16)
            if transform is not None:
                continue
            e.prime()
            torch.cuda.synchronize()
            sm = e.score_mode
            ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
            pool = torch.empty_like(sm.input)
            pl, pi = torch.empty_like(sm.label), torch.empty_like(sm.index)
            ops.pool_build(e.shard, e.shard_labels, ctrl, pool, pl, pi, 64, 32, e.seed,
                           recipe=e.augment, noise=e.noise)
            assert torch.equal(pool.view(torch.int16), sm.input.view(torch.int16))
            assert torch.equal(pi, sm.index) and len(set(e.aug_params[:, 0].tolist())) > 1
            e.step()
            torch.cuda.synchronize()
            m = e.read_meters()
            assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
            out = tr.evaluate()
            assert math.isfinite(out[2].average) and out[2].count == 32
        finally:
            tr.engine.close()
