"""Augmentation recipes on the GPU (``pool_recipe_kernel``) against ``AugmentRecipe.reference``
in fp64, fed with the draws the kernel dumped and the shard indices it wrote -- never with the
kernel's own pixels.

Tolerance, every element: |gpu - ref| <= 2^-8 |ref| + 1e-3.  The first term is one bf16 ulp;
the second covers the fp32 coordinates (about 4e-6 px times at most 255 levels/px is 1e-3
level, 2e-5 after Normalize) and sits about 15x below one uint8 level (1/255/std ~ 1.6e-2),
so an off-by-one pixel or level, a wrong flip or a half-pixel shift fail on noise images."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _recipe(**kw):
    from mercury_amd.data.augment import AugmentRecipe
    return AugmentRecipe(**kw)


def _noise(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def _build(shard, labels, recipe, P, B, seed=11, pc=0, dump=True, params=None, **kw):
    """One pool build -> (pool, labels, indices, params), everything on the host.  ``params``:
    the device buffer to dump into, in the place of a fresh [P][8] one."""
    ops = _ops()
    H, W = recipe.out_hw
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = pc
    pool = torch.full((P, H, W, 8), 7.0, dtype=torch.bfloat16, device=DEV)   # 7: never a result
    pl = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pi = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    if params is None and dump:
        params = torch.full((P, 8), -99.0, device=DEV)
    dump = params is not None
    ops.pool_build(shard.to(DEV), labels.to(DEV), ctrl, pool, pl, pi, P, B, seed, recipe=recipe,
                   params=params, **kw)
    torch.cuda.synchronize()
    return pool.cpu(), pl.cpu(), pi.cpu(), params.cpu() if dump else None


def _check(pool, params, index, shard, recipe):
    """Every element of every slot against the fp64 reference."""
    worst = -math.inf
    for s in range(pool.shape[0]):
        ref = recipe.reference(shard[int(index[s])], params[s].tolist())
        err = (pool[s, :, :, :3].double() - ref).abs()
        bound = ref.abs() * 2.0 ** -8 + 1e-3
        worst = max(worst, float((err - bound).max()))
        assert bool((err <= bound).all()), 'slot %d: max err %g over the bound by %g' % (
            s, float(err.max()), float((err - bound).max()))
    assert float(pool[..., 3:].abs().max()) == 0
    return worst


def test_legacy_recipe_is_bit_identical():
    """AugmentRecipe.cifar() takes today's kernel; forced through the recipe kernel it gives the
    same bits (same draws, crop, flip, normalisation)."""
    ops = _ops()
    from mercury_amd.data.augment import AugmentRecipe
    Ns, P, B = 40, 32, 16
    shard, labels = _noise(Ns, 32, 32, 1), torch.arange(Ns) % 10
    r = AugmentRecipe.cifar()
    for pc in (0, 2):
        ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctrl[0] = pc
        pool = torch.empty(P, 32, 32, 8, dtype=torch.bfloat16, device=DEV)
        pl = torch.empty(P, dtype=torch.int32, device=DEV)
        pi = torch.empty(P, dtype=torch.int32, device=DEV)
        ops.pool_build(shard.to(DEV), labels.to(DEV), ctrl, pool, pl, pi, P, B, 11)
        torch.cuda.synchronize()
        a = _build(shard, labels, r, P, B, pc=pc, dump=False)
        f = _build(shard, labels, r, P, B, pc=pc, dump=False, force_augment_kernel=True)
        d = _build(shard, labels, r, P, B, pc=pc)                   # dumping the draws: same kernel
        for got in (a, f, d):
            assert torch.equal(got[0].view(torch.int16), pool.cpu().view(torch.int16))
            assert torch.equal(got[1], pl.cpu()) and torch.equal(got[2], pi.cpu())
        # ... and the dumped draws explain the pixels
        _check(d[0], d[3], d[2], shard, r)
        assert set(d[3][:, 0].tolist()) <= set(range(9)) and set(d[3][:, 2].tolist()) == {0.0, 1.0}
        assert bool((d[3][:, 3] == 0).all()) and bool((d[3][:, 4] == 1).all())


# the binding called directly: a 16x16 source, a 32x32 crop, pad 4, no rrc, no jitter
RAW_16_TO_32 = dict(shard=0, labels=0, ctrl=0, pool=0, pool_label=0, pool_index=0, stream=0, Ns=4,
                    Hs=16, Ws=16, H=32, W=32, P=4, batch=4, pad=4, flip=1, augment=1, shuffle=1,
                    seed=0, mean=[0.0] * 3, inv_std=[1.0] * 3, Hr=16, Wr=16)


def test_recipe_needs_the_uint8_shard():
    ops = _ops()
    from mercury_amd.data.augment import AugmentRecipe
    z = torch.zeros(4, 32, 32, 8, dtype=torch.bfloat16, device=DEV)
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='uint8'):
        ops.pool_build(z, lab, lab, z.clone(), i, i.clone(), 4, 4, 0, recipe=AugmentRecipe.cifar())
    small = torch.zeros(4, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='does not fit'):
        ops.pool_build(small, lab, lab, z.clone(), i, i.clone(), 4, 4, 0,
                       recipe=AugmentRecipe.cifar())
    with pytest.raises(RuntimeError, match='empty crop range'):      # the binding's own check
        ops.lib().pool_recipe(**RAW_16_TO_32)


FULL = dict(resize=35, crop=(32, 32), flip=True, degrees=10.0, scale=(0.9, 1.1))
CASES = {
    'full': ((24, 32, 32), 16, 8, FULL),
    'nonsquare_cutout': ((24, 24, 32), 16, 8, dict(
        resize=27, crop=(24, 24), pad=2, flip=True, degrees=10.0, scale=(0.9, 1.1), cutout=8,
        mean=[0.49139968, 0.48215827, 0.44653124], std=[0.24703233, 0.24348505, 0.26158768])),
    'crop_only': ((24, 40, 40), 16, 8, dict(crop=(32, 32), flip=True)),
}


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('pc', [0, 3])
def test_recipe_matches_reference(case, pc):
    (Ns, Hs, Ws), P, B, kw = CASES[case]
    r = _recipe(**kw)
    shard, labels = _noise(Ns, Hs, Ws, 2), (torch.arange(Ns) * 7) % 10
    pool, pl, pi, params = _build(shard, labels, r, P, B, pc=pc)
    assert int(pi.min()) >= 0 and int(pi.max()) < Ns
    assert torch.equal(pl.long(), labels[pi.long()])
    assert bool((params[:, 7] == 0).all())
    worst = _check(pool, params, pi, shard, r)
    print('%s pc=%d: worst err - bound = %.3g' % (case, pc, worst))
    Hr, Wr = r.resized_hw(Hs, Ws)
    assert float(params[:, 0].max()) <= Hr + 2 * r.pad - r.crop[0]
    assert float(params[:, 1].max()) <= Wr + 2 * r.pad - r.crop[1]
    if not r.affine:
        assert bool((params[:, 3] == 0).all()) and bool((params[:, 4] == 1).all())


def _case(case):
    (Ns, Hs, Ws), P, B, kw = CASES[case]
    return _noise(Ns, Hs, Ws, 2), (torch.arange(Ns) * 7) % 10, _recipe(**kw), P, B


@pytest.mark.parametrize('case', ['crop_only', 'full'])
def test_params_row_is_eight_floats(case):
    """A recipe without rrc / jitter dumps 8 floats per slot: P slots fill the first P * 8 floats
    of a longer buffer with what a [P][8] buffer of its own receives, and touch nothing behind
    them (a 16-float stride, or the 16-float row's grey-mean word [15], would)."""
    shard, labels, r, P, B = _case(case)
    want = _build(shard, labels, r, P, B, pc=1)
    big = torch.full((P * 16 + 16,), -99.0, device=DEV)
    got = _build(shard, labels, r, P, B, pc=1, params=big[:P * 8])
    big = big.cpu()
    assert bool((big[P * 8:] == -99.0).all())
    assert torch.equal(big[:P * 8].view(torch.int32), want[3].reshape(-1).view(torch.int32))
    assert bool((want[3] != -99.0).all()) and bool((want[3][:, 7] == 0).all())
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))


@pytest.mark.parametrize('case', ['crop_only', 'full'])
def test_dump_does_not_change_pixels(case):
    """With and without a params buffer: the same pool, labels and indices, bit for bit."""
    shard, labels, r, P, B = _case(case)
    plain = _build(shard, labels, r, P, B, pc=1, dump=False, force_augment_kernel=True)
    dumped = _build(shard, labels, r, P, B, pc=1, force_augment_kernel=True)
    assert plain[3] is None and bool((dumped[3] != -99.0).all())
    assert torch.equal(plain[0].view(torch.int16), dumped[0].view(torch.int16))
    assert torch.equal(plain[1], dumped[1]) and torch.equal(plain[2], dumped[2])
    assert int(plain[2].min()) >= 0 and not bool((plain[0][..., :3] == 7.0).any())


def test_cutout_zeroes_its_square_and_nothing_else():
    kw = dict(CASES['nonsquare_cutout'][3])
    shard, labels = _noise(24, 24, 32, 3), torch.arange(24) % 10
    cut = _build(shard, labels, _recipe(**kw), 16, 8, pc=1)
    kw['cutout'] = 0
    plain = _build(shard, labels, _recipe(**kw), 16, 8, pc=1)
    assert torch.equal(cut[3], plain[3]) and torch.equal(cut[2], plain[2])
    H, W = 24, 24
    holes = 0
    for s in range(16):
        cy, cx = int(cut[3][s, 5]), int(cut[3][s, 6])
        assert 0 <= cy < H and 0 <= cx < W
        y1, y2 = int(np.clip(cy - 8 // 2, 0, H)), int(np.clip(cy + 8 // 2, 0, H))
        x1, x2 = int(np.clip(cx - 8 // 2, 0, W)), int(np.clip(cx + 8 // 2, 0, W))
        hole = torch.zeros(H, W, dtype=torch.bool)
        hole[y1:y2, x1:x2] = True
        holes += int(hole.sum())
        a, b = cut[0][s].view(torch.int16), plain[0][s].view(torch.int16)
        assert bool((a[hole] == 0).all())
        assert torch.equal(a[~hole], b[~hole])
    assert holes > 0


def test_parameter_draws():
    """8 pools of 256 slots: ranges, coverage, moments (5 sigma), determinism."""
    r = _recipe(**FULL)
    shard, labels = _noise(64, 8, 8, 4), torch.arange(64) % 10
    runs = [_build(shard, labels, r, 256, 32, seed=5, pc=pc) for pc in range(8)]
    p = torch.cat([x[3] for x in runs])
    n = p.shape[0]
    assert n == 2048
    for k in (0, 1):
        assert sorted(set(p[:, k].tolist())) == [0.0, 1.0, 2.0, 3.0]
    assert set(p[:, 2].tolist()) == {0.0, 1.0}
    assert float(p[:, 3].min()) >= -10 and float(p[:, 3].max()) < 10
    assert float(p[:, 4].min()) >= 0.9 and float(p[:, 4].max()) < 1.1
    assert abs(float(p[:, 2].mean()) - 0.5) <= 5 * 0.5 / math.sqrt(n)
    assert abs(float(p[:, 3].mean())) <= 5 * (20 / math.sqrt(12)) / math.sqrt(n)
    assert float(p[:, 5].min()) >= 0 and float(p[:, 5].max()) <= 31
    assert float(p[:, 6].min()) >= 0 and float(p[:, 6].max()) <= 31
    again = _build(shard, labels, r, 256, 32, seed=5, pc=3)
    assert torch.equal(again[0].view(torch.int16), runs[3][0].view(torch.int16))
    assert torch.equal(again[3], runs[3][3])
    assert not torch.equal(runs[4][3], runs[3][3])
    assert not torch.equal(runs[4][0].view(torch.int16), runs[3][0].view(torch.int16))
    other = _build(shard, labels, r, 256, 32, seed=6, pc=3)
    assert not torch.equal(other[3], runs[3][3])


ENGINE_CASES = {
    'crop_flip_40': ((40, 40), dict(crop=(32, 32), flip=True)),
    'full_32': ((32, 32), FULL),
}


@pytest.mark.parametrize('case', sorted(ENGINE_CASES))
def test_engine_trains_on_a_recipe(case):
    """ResNet-18, B = 32, 10 pool batches, graphs on: the scored pool is the recipe's."""
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import ResNet18
    (Hs, Ws), kw = ENGINE_CASES[case]
    r = _recipe(**kw)
    ev = _recipe(resize=33, crop=(32, 32))
    shard = _noise(640, Hs, Ws, 6)
    labels = torch.arange(640) % 10
    torch.manual_seed(0)
    eng = NativeEngine(ResNet18(10).to(DEV), DEV, 32, 10, image_hw=(32, 32), augment=r,
                       eval_augment=ev, use_graphs=True)
    try:
        eng.set_shard(shard.numpy(), labels.numpy())      # without recipes: "must be [N][32][32][3]"
        assert eng.aug_params.shape == (320, 8)
        eng.prime()
        eng.step()
        eng.build_graphs()
        eng.step()
        eng.step()
        torch.cuda.synchronize()
        sm = eng.score_mode
        pool = sm.input.view(320, 32, 32, 8).cpu()
        index = sm.index.cpu()
        assert torch.equal(sm.label.cpu().long(), labels[index.long()])
        _check(pool, eng.aug_params.cpu(), index, shard, r)
        m = eng.read_meters()
        assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
        # evaluation under the Resize(33) + RandomCrop(32) recipe: same views, same numbers on a
        # second call.  500 images = one eval batch whose convs run without split-K; a smaller
        # batch takes split-K plans whose atomic partial sums move single losses by an ulp from
        # call to call, with or without a recipe.
        x = _noise(500, 32, 32, 8).numpy()
        y = (np.arange(500) % 10)
        first = eng.evaluate_arrays(x, y)
        views = eng.modes['eval500'].input.clone()
        second = eng.evaluate_arrays(x, y)
        assert torch.equal(views.view(torch.int16), eng.modes['eval500'].input.view(torch.int16))
        assert first == second and first[2] == 500
        assert math.isfinite(first[0]) and 0.0 <= first[1] <= 1.0
    finally:
        eng.close()


class _Set(object):
    def __init__(self, data, target, transform):
        self.data, self.target, self.transform = data, target, transform


class _Loader(object):
    batch_size = 32

    def __init__(self, dataset, steps=1):
        self.dataset, self.steps = dataset, steps

    def __len__(self):
        return self.steps


def test_trainer_reads_the_dataset_transform():
    from mercury_amd.collab import make_trainer
    from mercury_amd.config import Config
    from mercury_amd.data import transforms as T
    from mercury_amd.engine.native import NativeTrainer
    from mercury_amd.models import ResNet18
    x, y = _noise(640, 32, 32, 9).numpy(), np.arange(640) % 10
    train = _Loader(_Set(x, y, T.affine_train_transform()))
    test = _Loader(_Set(x[:64], y[:64], T.affine_test_transform()))

    def trainer(**kw):
        torch.manual_seed(0)
        net = ResNet18(10).to(DEV)
        cfg = Config(print_every=0, eval_every=0, use_graphs=False, **kw)
        return make_trainer(cfg, net, torch.optim.Adam(net.parameters(), lr=1e-3), train, train,
                            test, DEV)

    tr = trainer(augment='dataset')
    try:
        assert isinstance(tr, NativeTrainer)
        assert tr.engine.augment == _recipe(**FULL)
        assert tr.engine.eval_augment == _recipe(resize=33, crop=(32, 32))
        assert (tr.engine.H, tr.engine.W) == (32, 32)
        loss, acc, _ = tr.train()
        torch.cuda.synchronize()
        assert tr.step == 2 and math.isfinite(loss.average)
        e = tr.engine
        _check(e.score_mode.input.view(320, 32, 32, 8).cpu()[:32], e.aug_params.cpu()[:32],
               e.score_mode.index.cpu()[:32], torch.as_tensor(x), e.augment)
    finally:
        tr.engine.close()
    tr = trainer(augment='cifar')
    try:
        assert tr.engine.augment is None and tr.engine.eval_augment is None
        assert tr.engine.aug_params is None
    finally:
        tr.engine.close()
