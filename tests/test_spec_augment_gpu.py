"""Spectrogram recipes on the GPU (``pool_spec_kernel``) against ``SpecRecipe.reference``, fed
with the draws the kernel dumped and the shard indices it wrote -- never with the kernel's own
pixels.  Every operation is a select or one fp32 multiply rounded once to bf16, so every
comparison here is exact: 0 ulp, on int16 views of the bf16 bits."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 7.0            # the pool's content before a build: 7 is never a result of these inputs

# (C, H, W); 1x101x161 is 16261 pixels: 63 full 256-pixel trips and a 133-pixel tail
SHAPES = [(1, 5, 19), (3, 4, 7), (8, 3, 33), (1, 101, 161)]
FULL = dict(shift=3, fmask=(2, 2), tmask=(2, 6), gain=(0.5, 2.0), fill=-1.5)
RECIPES = {
    'full': FULL,
    'shift': dict(shift=3, fill=-1.5),
    'masks': dict(fmask=(2, 2), tmask=(2, 6), fill=-1.5),
    'gain': dict(gain=(0.5, 2.0)),
}


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _recipe(**kw):
    from mercury_amd.data.augment import SpecRecipe
    return SpecRecipe(**kw)


_SHARDS = {}


def _shard(Ns, C, H, W):
    """(float [Ns][C][H][W] on the host, labels): made once per shape and never written."""
    key = (Ns, C, H, W)
    if key not in _SHARDS:
        g = torch.Generator().manual_seed(17 + Ns + H)
        _SHARDS[key] = (torch.randn(Ns, C, H, W, generator=g), (torch.arange(Ns) * 7) % 30)
    return _SHARDS[key]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _build(x, labels, recipe, P, B, seed=11, pc=0, dump=True, **kw):
    """One pool build from the planar bf16 shard -> (pool, labels, indices, params) on the host."""
    ops = _ops()
    H, W = x.shape[2:]
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = pc
    pool = torch.full((P, H, W, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pi = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    params = torch.full((P, 12), -99.0, device=DEV) if dump else None
    ops.pool_build(x.to(DEV).bfloat16(), labels.to(DEV), ctrl, pool, pl, pi, P, B, seed,
                   recipe=recipe, params=params, **kw)
    torch.cuda.synchronize()
    return pool.cpu(), pl.cpu(), pi.cpu(), params.cpu() if dump else None


def _take(x, labels, P, B, seed=11, pc=0):
    """Today's path: the same samples as an NHWC8 shard, gathered with no recipe."""
    ops = _ops()
    N, C, H, W = x.shape
    nhwc = torch.empty(N, H, W, 8, dtype=torch.bfloat16, device=DEV)
    ops.nchw_to_nhwc8(x.to(DEV).contiguous(), nhwc)
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = pc
    pool = torch.full((P, H, W, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pi = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    ops.pool_build(nhwc, labels.to(DEV), ctrl, pool, pl, pi, P, B, seed)
    torch.cuda.synchronize()
    return pool.cpu(), pl.cpu(), pi.cpu()


def _check(pool, params, index, x, recipe):
    """Every element of every slot, channels C..7 included, equals the reference's bits."""
    for s in range(pool.shape[0]):
        ref = recipe.reference(x[int(index[s])], params[s].tolist())
        bad = _bits(pool[s]) != _bits(ref)
        assert not bool(bad.any()), 'slot %d: %d elements differ, first at %s' % (
            s, int(bad.sum()), bad.nonzero()[0].tolist())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('Ns', [24, 7])
def test_identity_is_the_plain_gather(shape, Ns):
    """SpecRecipe() -- and any recipe with augment=False -- on the planar shard gives the bits,
    labels and indices of pool_take_kernel on the NHWC8 shard (Ns = 7 < B: a cycled shard)."""
    C, H, W = shape
    x, labels = _shard(Ns, C, H, W)
    for pc in (0, 3):
        want = _take(x, labels, 16, 8, pc=pc)
        got = _build(x, labels, _recipe(), 16, 8, pc=pc)
        off = _build(x, labels, _recipe(**FULL), 16, 8, pc=pc, augment=False)
        nodump = _build(x, labels, _recipe(), 16, 8, pc=pc, dump=False)
        for g in (got, off, nodump):
            assert torch.equal(_bits(g[0]), _bits(want[0]))
            assert torch.equal(g[1], want[1]) and torch.equal(g[2], want[2])
        ident = torch.zeros(16, 12)
        ident[:, 1] = 1
        assert torch.equal(got[3], ident) and torch.equal(off[3], ident)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('name', sorted(RECIPES))
def test_recipe_matches_reference(name, shape):
    C, H, W = shape
    r = _recipe(**RECIPES[name])
    x, labels = _shard(24, C, H, W)
    for pc in (0, 3):
        pool, pl, pi, params = _build(x, labels, r, 16, 8, pc=pc)
        assert int(pi.min()) >= 0 and int(pi.max()) < 24
        assert torch.equal(pl.long(), labels[pi.long()])
        assert bool((params[:, 10:] == 0).all())
        _check(pool, params, pi, x, r)
        assert bool((_bits(pool[..., C:]) == 0).all())          # +0, not the sentinel, not -0
        if r.gain is None:
            assert bool((params[:, 1] == 1).all())
        if not r.shift:
            assert bool((params[:, 0] == 0).all())
        if name in ('shift', 'gain'):
            assert bool((params[:, 2:10] == 0).all())


def test_masks_fill_their_bands_and_nothing_else():
    C, H, W = 3, 12, 40
    x, labels = _shard(24, C, H, W)
    kw = dict(shift=3, fmask=(2, 4), tmask=(2, 9), gain=(0.5, 2.0), fill=-1.5)
    masked = _build(x, labels, _recipe(**kw), 16, 8, pc=1)
    # the same draws, the bands emptied by hand: the reference with widths 0 is the unmasked build
    plain = _build(x, labels, _recipe(shift=3, gain=(0.5, 2.0), fill=-1.5), 16, 8, pc=1)
    assert torch.equal(masked[3][:, :2], plain[3][:, :2]) and torch.equal(masked[2], plain[2])
    fill = _bits(torch.tensor(-1.5).bfloat16())
    union = 0
    for s in range(16):
        p = masked[3][s].long().tolist()
        band = torch.zeros(H, W, dtype=torch.bool)
        for f0, fw in ((p[2], p[3]), (p[4], p[5])):
            assert 0 <= f0 and f0 + fw <= H and 0 <= fw <= 4
            band[f0:f0 + fw, :] = True
        for t0, tw in ((p[6], p[7]), (p[8], p[9])):
            assert 0 <= t0 and t0 + tw <= W and 0 <= tw <= 9
            band[:, t0:t0 + tw] = True
        union += int(band.sum())
        a, b = _bits(masked[0][s, :, :, :C]), _bits(plain[0][s, :, :, :C])
        assert bool((a[band] == fill).all())
        assert torch.equal(a[~band], b[~band])
        # noise never equals the fill, so the two builds differ exactly on the bands, except
        # where the shift already filled the unmasked build
        differs = (a != b).any(dim=-1)
        shifted_in = (b == fill).all(dim=-1)
        assert torch.equal(differs, band & ~shifted_in)
    assert union > 0


def test_parameter_draws():
    """8 pools of 256 slots: ranges, coverage, the gain's mean (5 sigma), determinism."""
    r = _recipe(**FULL)
    H, W = 4, 9
    x, labels = _shard(64, 1, H, W)
    runs = [_build(x, labels, r, 256, 32, seed=5, pc=pc) for pc in range(8)]
    p = torch.cat([q[3] for q in runs])
    n = p.shape[0]
    assert n == 2048
    assert sorted(set(p[:, 0].tolist())) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    for k, size, mx in ((2, H, 2), (4, H, 2), (6, W, 6), (8, W, 6)):
        assert sorted(set(p[:, k + 1].tolist())) == [float(v) for v in range(mx + 1)]
        assert float(p[:, k].min()) >= 0 and bool((p[:, k] + p[:, k + 1] <= size).all())
    assert float(p[:, 1].min()) >= 0.5 and float(p[:, 1].max()) < 2.0
    assert abs(float(p[:, 1].mean()) - 1.25) <= 5 * (1.5 / math.sqrt(12)) / math.sqrt(n)
    assert bool((p[:, 10:] == 0).all())
    again = _build(x, labels, r, 256, 32, seed=5, pc=3)
    assert torch.equal(_bits(again[0]), _bits(runs[3][0])) and torch.equal(again[3], runs[3][3])
    assert not torch.equal(runs[4][3], runs[3][3])
    assert not torch.equal(_bits(runs[4][0]), _bits(runs[3][0]))
    other = _build(x, labels, r, 256, 32, seed=6, pc=3)
    assert not torch.equal(other[3], runs[3][3])
    assert not torch.equal(_bits(other[0]), _bits(runs[3][0]))


def test_chunked_grid_gives_the_same_bits():
    """Blocks per slot (the launcher picks it from P) never change a bit."""
    from mercury_amd.ops.importance import _pool_spec
    r = _recipe(**FULL)
    x, labels = _shard(24, 1, 101, 161)
    want = _build(x, labels, r, 16, 8, pc=2)
    shard, lab = x.to(DEV).bfloat16(), labels.to(DEV)
    for chunks in (1, 3, 64, 1000):
        ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctrl[0] = 2
        pool = torch.full((16, 101, 161, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
        pl = torch.full((16,), -1, dtype=torch.int32, device=DEV)
        pi = torch.full((16,), -1, dtype=torch.int32, device=DEV)
        params = torch.full((16, 12), -99.0, device=DEV)
        _pool_spec(shard, lab, ctrl, pool, pl, pi, 16, 8, 11, True, True, None, r, params,
                   chunks=chunks)
        torch.cuda.synchronize()
        assert torch.equal(_bits(pool.cpu()), _bits(want[0])) and torch.equal(params.cpu(), want[3])
        assert torch.equal(pl.cpu(), want[1]) and torch.equal(pi.cpu(), want[2])


def test_refusals():
    ops = _ops()
    from mercury_amd.data.augment import AugmentRecipe
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    pool = torch.zeros(4, 5, 19, 8, dtype=torch.bfloat16, device=DEV)
    planar = torch.zeros(4, 1, 5, 19, dtype=torch.bfloat16, device=DEV)
    nhwc8 = torch.zeros(4, 5, 19, 8, dtype=torch.bfloat16, device=DEV)
    u8 = torch.zeros(4, 5, 19, 3, dtype=torch.uint8, device=DEV)

    def build(shard, recipe, pool=pool, **kw):
        ops.pool_build(shard, lab, lab, pool, i, i.clone(), 4, 4, 0, recipe=recipe, **kw)

    with pytest.raises(ValueError, match='shard is uint8'):
        build(u8, _recipe())
    with pytest.raises(ValueError, match=r'shard is \(4, 5, 19, 8\).*NHWC8'):
        build(nhwc8, _recipe())
    with pytest.raises(ValueError, match=r'shard is \(4, 9, 5, 19\)'):         # C > 8
        build(torch.zeros(4, 9, 5, 19, dtype=torch.bfloat16, device=DEV), _recipe())
    with pytest.raises(ValueError, match='needs the uint8 image shard'):
        build(planar, AugmentRecipe.cifar())
    with pytest.raises(ValueError, match='planar'):
        build(planar, None)
    with pytest.raises(ValueError, match='pool must be'):
        build(planar, _recipe(), pool=pool.view(-1))
    with pytest.raises(ValueError, match='params too small'):
        build(planar, _recipe(), params=torch.zeros(4, 8, device=DEV))
    with pytest.raises(ValueError, match='shift'):
        build(planar, _recipe(shift=19))
    with pytest.raises(ValueError, match='fmask'):
        build(planar, _recipe(fmask=(1, 6)))
    with pytest.raises(ValueError, match='tmask'):
        build(planar, _recipe(tmask=(1, 20)))
    with pytest.raises(ValueError, match='force_augment_kernel'):
        build(planar, _recipe(), force_augment_kernel=True)

    # the binding's own checks, with null pointers: they must refuse before any launch
    def raw(Ns=4, C=1, H=5, W=19, P=4, batch=4, shift=0, fn=0, fm=0, tn=0, tm=0, lo=1.0, hi=1.0,
            fill=0.0, chunks=0):
        ops.lib().pool_spec(0, 0, 0, 0, 0, 0, Ns, C, H, W, P, batch, 1, 1, 0, 0, 0, 0, shift, fn,
                            fm, tn, tm, lo, hi, fill, 0, chunks)

    for kw, field in ((dict(Ns=0), 'Ns'), (dict(C=0), 'C must'), (dict(C=9), 'C must'),
                      (dict(H=1 << 15, W=1 << 15, P=2), r'H\*W\*P'),
                      (dict(shift=-1), 'shift'), (dict(shift=19), 'shift'),
                      (dict(fn=3), 'fmask'), (dict(fn=1, fm=6), 'fmask'), (dict(fm=-1), 'fmask'),
                      (dict(tn=3), 'tmask'), (dict(tn=1, tm=20), 'tmask'), (dict(tn=-1), 'tmask'),
                      (dict(lo=2.0, hi=1.0), 'gain'), (dict(hi=float('inf')), 'gain'),
                      (dict(lo=float('nan')), 'gain'), (dict(fill=float('nan')), 'fill'),
                      (dict(chunks=-1), 'chunks')):
        with pytest.raises(RuntimeError, match=field):
            raw(**kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- engine and trainer
HW = (101, 161)


def _speech(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 1, HW[0], HW[1], generator=g).numpy(), (np.arange(n) * 7) % 30


def _engine(augment, x, y):
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    torch.manual_seed(0)
    eng = NativeEngine(build_model('vgg11', 30).to(DEV), DEV, 32, 2, image_hw=HW, seed=3,
                       augment=augment, use_graphs=False)
    eng.set_shard(x, y)
    return eng


def test_engine_trains_on_a_recipe():
    """VGG11, 30 classes, 1x101x161, B = 32, two pool batches, a 64-sample float shard."""
    r = _recipe(**FULL)
    x, y = _speech(64, 21)
    xe, ye = _speech(32, 22)
    state = {}
    for name, aug in (('none', None), ('identity', _recipe()), ('full', r)):
        eng = _engine(aug, x, y)
        try:
            if aug is None:
                assert eng.aug_params is None and tuple(eng.shard.shape) == (64, 101, 161, 8)
            else:
                assert tuple(eng.shard.shape) == (64, 1, 101, 161)
                assert eng.shard.dtype == torch.bfloat16 and eng.shard.is_contiguous()
                assert eng.aug_params.shape == (64, 12) and eng.eval_augment is None
            ev = eng.evaluate_arrays(xe, ye) + (eng.modes['eval32'].input.cpu(),)
            eng.prime()
            torch.cuda.synchronize()
            sm = eng.score_mode
            state[name] = (sm.input.view(64, 101, 161, 8).cpu(), sm.label.cpu(), sm.index.cpu(), ev)
            if name == 'full':
                params = eng.aug_params.cpu()
                assert torch.equal(sm.label.cpu().long(), torch.as_tensor(y)[sm.index.cpu().long()])
                _check(state[name][0], params, state[name][2], torch.as_tensor(x), r)
                assert len(set(params[:, 0].tolist())) > 1          # the recipe did draw
                for _ in range(3):
                    eng.step()
                torch.cuda.synchronize()
                m = eng.read_meters()
                assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
        finally:
            eng.close()
    none, ident, full = state['none'], state['identity'], state['full']
    assert torch.equal(_bits(ident[0]), _bits(none[0]))
    assert torch.equal(ident[1], none[1]) and torch.equal(ident[2], none[2])
    assert torch.equal(full[1], none[1]) and torch.equal(full[2], none[2])
    # evaluation takes the NHWC8 conversion and the plain gather whatever the train recipe: the
    # same input bits, count and accuracy.  The mean loss is an fp32 atomic sum of the 32
    # per-sample losses in block arrival order (and split-K convs move single losses by an ulp),
    # with or without a recipe, so two calls agree to the reordering bound n * 2^-24 * sum|l|,
    # not to the bit.
    for other in (ident[3], full[3]):
        assert torch.equal(_bits(other[3]), _bits(none[3][3]))
        assert other[1:3] == none[3][1:3]
        print('eval loss %.9g vs %.9g' % (other[0], none[3][0]))
        assert abs(other[0] - none[3][0]) <= 32 * 2.0 ** -24 * abs(none[3][0])
    assert none[3][2] == 32 and math.isfinite(none[3][0])


def test_engine_refuses_what_a_spec_recipe_cannot_take():
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    net = build_model('vgg11', 30).to(DEV)
    with pytest.raises(ValueError, match='eval_augment'):
        NativeEngine(net, DEV, 32, 2, image_hw=HW, eval_augment=_recipe())
    with pytest.raises(ValueError, match='shift'):
        NativeEngine(net, DEV, 32, 2, image_hw=HW, augment=_recipe(shift=161))
    eng = NativeEngine(net, DEV, 32, 2, image_hw=HW, augment=_recipe(shift=4), use_graphs=False)
    try:
        with pytest.raises(ValueError, match='float shard'):
            eng.set_shard(np.zeros((4, 101, 161, 3), np.uint8), np.zeros(4, np.int64))
        with pytest.raises(ValueError, match='float shard'):
            eng.set_shard(np.zeros((4, 1, 100, 161), np.float32), np.zeros(4, np.int64))
    finally:
        eng.close()


class _Set(object):
    def __init__(self, data, target, transform=None):
        self.data, self.target, self.transform = data, target, transform


class _Loader(object):
    batch_size = 32

    def __init__(self, dataset, steps=1):
        self.dataset, self.steps = dataset, steps

    def __len__(self):
        return self.steps


def test_trainer_takes_a_float_dataset():
    from mercury_amd.collab import make_trainer
    from mercury_amd.config import Config
    from mercury_amd.data.transforms import SpecAugment
    from mercury_amd.engine.native import NativeTrainer
    from mercury_amd.models import build_model
    x, y = _speech(64, 23)
    want = _recipe(shift=4, tmask=(1, 8))

    def trainer(transform, **kw):
        torch.manual_seed(0)
        net = build_model('vgg11', 30).to(DEV)
        train = _Loader(_Set(x, y, transform))
        test = _Loader(_Set(x[:32], y[:32]))
        cfg = Config(print_every=0, eval_every=0, use_graphs=False, presample_batches=2, **kw)
        return make_trainer(cfg, net, torch.optim.Adam(net.parameters(), lr=1e-3), train, train,
                            test, DEV)

    for transform, kw in ((None, dict(augment='spec:shift=4,tmask=1x8')),
                          (SpecAugment(want), dict(augment='dataset'))):
        tr = trainer(transform, **kw)
        try:
            assert isinstance(tr, NativeTrainer)
            e = tr.engine
            assert e.augment == want and e.eval_augment is None
            assert (e.H, e.W) == HW and tuple(e.shard.shape) == (64, 1, 101, 161)
            assert e.aug_params.shape == (64, 12)
        finally:
            tr.engine.close()
    tr = trainer(None)                      # the default: no recipe, today's NHWC8 shard
    try:
        assert tr.engine.augment is None and tuple(tr.engine.shard.shape) == (64, 101, 161, 8)
    finally:
        tr.engine.close()
