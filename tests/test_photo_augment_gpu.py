"""RandomResizedCrop and ColorJitter recipes on the GPU (``pool_recipe_kernel`` with a box or
colour draw, ``csrc/pool_recipe.hip``) against ``AugmentRecipe.reference`` in fp64, fed with the
draws the kernel dumped and the shard indices it wrote -- never with the kernel's own pixels --
and the draws themselves against the Philox replay of ``photo_oracles``.

Tolerance, every element: |gpu - ref| <= 2^-8 |ref| + 1e-3, the bound ``test_augment_gpu``
derives (one bf16 ulp, plus fp32 coordinates and weights: about 1e-5 after Normalize).  The
colour stages are Lipschitz with a small constant, so the bound keeps its factor of 15 below one
uint8 level.  The grey mean: the fp32 tree's error is at most (pixels per thread + 8) * 2^-24
(below 1e-6 at these sizes); 1e-4 is a factor of 40 below one uint8 level.

Shapes are the smallest at which each mechanism can go wrong: 32x32 (four pixels per thread),
24x20 (480 pixels, no multiple of 256), 12x12 (fewer pixels than threads), boxes smaller and
larger than the output and boxes on the image's edge.  Seeds are chosen on the CPU with the
Philox replay; every test asserts what it chose them for."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import photo_oracles as po
from test_augment_gpu import CASES as OLD_CASES, RAW_16_TO_32

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED = 1
HS, WS = 40, 48
RRC_A = (0.08, 1.0, 0.75, 4.0 / 3.0)
RRC_UP = (0.02, 0.1, 0.5, 2.0)
JIT = (0.4, 0.4, 0.4, 0.1)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


_SHARDS = {}


def _shard(n, h, w):
    if (n, h, w) not in _SHARDS:
        _SHARDS[n, h, w] = (_noise(n, h, w, 2), (torch.arange(n) * 7) % 10)
    return _SHARDS[n, h, w]


def _build(shard, labels, recipe, P, B, seed=SEED, pc=0, dump=True, **kw):
    """One pool build -> (pool, labels, indices, params), everything on the host."""
    ops = _ops()
    H, W = recipe.out_hw
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    ctrl[0] = pc
    pool = torch.full((P, H, W, 8), 7.0, dtype=torch.bfloat16, device=DEV)   # 7: never a result
    pl = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pi = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    n = 16 if recipe.photo else 8
    params = torch.full((P, n), -99.0, device=DEV) if dump else None
    ops.pool_build(shard.to(DEV), labels.to(DEV), ctrl, pool, pl, pi, P, B, seed, recipe=recipe,
                   params=params, **kw)
    torch.cuda.synchronize()
    return pool.cpu(), pl.cpu(), pi.cpu(), params.cpu() if dump else None


def _check(pool, params, index, shard, recipe):
    """Every element of every slot against the fp64 reference; the grey mean too."""
    worst, worst_mean = -math.inf, 0.0
    for s in range(pool.shape[0]):
        info = {}
        ref = recipe.reference(shard[int(index[s])], params[s].tolist(), info=info)
        err = (pool[s, :, :, :3].double() - ref).abs()
        bound = ref.abs() * 2.0 ** -8 + 1e-3
        worst = max(worst, float((err - bound).max()))
        assert bool((err <= bound).all()), 'slot %d: max err %g over the bound by %g' % (
            s, float(err.max()), float((err - bound).max()))
        dm = abs(float(params[s, 15]) - info.get('grey_mean', 0.0))
        worst_mean = max(worst_mean, dm)
        assert dm <= 1e-4, 'slot %d: grey mean %r, reference %r' % (s, float(params[s, 15]), info)
    assert float(pool[..., 3:].abs().max()) == 0
    return worst, worst_mean


def _inside(params):
    top, left, h, w = (params[:, k] for k in (0, 1, 8, 9))
    assert bool(((top >= 0) & (left >= 0) & (h >= 1) & (w >= 1)).all())
    assert bool(((top + h <= HS) & (left + w <= WS)).all())


GEOMETRY = {'flip': dict(rrc=RRC_A, flip=True),
            'norm': dict(rrc=RRC_A, flip=True, mean=MEAN, std=STD),
            'upsampled': dict(rrc=RRC_UP)}


@pytest.mark.parametrize('kind', sorted(GEOMETRY))
@pytest.mark.parametrize('out', [(32, 32), (24, 20), (12, 12)])
def test_rrc_matches_reference(out, kind):
    P, B = 16, 8
    r = _recipe(crop=out, **GEOMETRY[kind])
    shard, labels = _shard(24, HS, WS)
    seen = []
    for pc in (0, 3):
        pool, pl, pi, params = _build(shard, labels, r, P, B, pc=pc)
        assert int(pi.min()) >= 0 and int(pi.max()) < 24
        assert torch.equal(pl.long(), labels[pi.long()])
        _inside(params)
        worst, _ = _check(pool, params, pi, shard, r)
        print('rrc %s %dx%d pc=%d: worst err - bound = %.3g' % (kind, out[0], out[1], pc, worst))
        assert bool((params[:, 3] == 0).all()) and bool((params[:, 4] == 1).all())
        assert bool((params[:, 10:13] == 1).all()) and bool((params[:, 13:] == 0).all())
        assert set(params[:, 2].tolist()) <= ({0.0, 1.0} if r.flip else {0.0})
        assert torch.equal(params[:, 2].long(), torch.as_tensor(po.flips(SEED, pc, P, B))
                           * int(r.flip))
        seen += [(int(p[7]), int(p[0]), int(p[1]), int(p[8]), int(p[9]), False) for p in params]
    small, large, edge = po.box_coverage(seen, out[0], out[1], HS, WS)
    if kind == 'upsampled':
        if out != (12, 12):
            assert all(h <= out[0] and w <= out[1] for _, _, _, h, w, _ in seen)
    else:
        # (a box below 12x12 has less than scale_lo of the image's area)
        assert large and edge and (small or out == (12, 12))


def test_box_draws_match_the_philox_replay():
    P, B = 64, 8
    r = _recipe(crop=(12, 12), rrc=RRC_A, flip=True)
    shard, labels = _shard(24, HS, WS)
    want = po.boxes(SEED, 0, P, B, HS, WS, RRC_A)
    assert sum(b[5] for b in want) <= 2                  # the seed's own property, on the CPU
    assert len({b[0] for b in want}) > 1                 # some slot needed a second attempt
    _, _, _, params = _build(shard, labels, r, P, B)
    words = po.slot_words(SEED, 0, P, B, po.W_POS)
    loose = 0
    for s in range(P):
        got = tuple(int(params[s, k]) for k in (7, 0, 1, 8, 9))
        if got == want[s][:5]:
            continue
        assert want[s][5], 'slot %d: %r, replay %r' % (s, got, want[s])
        loose += 1
        att, top, left, h, w = got
        assert att == want[s][0] and abs(h - want[s][3]) <= 1 and abs(w - want[s][4]) <= 1
        assert top == int(words[0, s]) % (HS - h + 1) and left == int(words[1, s]) % (WS - w + 1)
    assert loose <= 2


def test_whole_image_box_equals_crop_and_flip_bit_for_bit():
    """rrc = (1, 1, Ws/Hs, Ws/Hs) to the source size: the box is the image, the bilinear weights
    are exactly 0 and 1, the flip bit is the same word -- the crop + flip recipe's bits."""
    P, B = 16, 8
    shard, labels = _shard(24, HS, WS)
    a = _recipe(crop=(HS, WS), rrc=(1, 1, WS / HS, WS / HS), flip=True, mean=MEAN, std=STD)
    b = _recipe(crop=(HS, WS), flip=True, mean=MEAN, std=STD)
    for pc in (0, 3):
        got = _build(shard, labels, a, P, B, pc=pc)
        want = _build(shard, labels, b, P, B, pc=pc, force_augment_kernel=True)
        assert bool((got[3][:, 7] == 0).all())
        assert torch.equal(got[3][:, [0, 1, 8, 9]], torch.tensor([[0., 0., HS, WS]] * P))
        assert torch.equal(got[3][:, 2], want[3][:, 2]) and set(got[3][:, 2].tolist()) == {0., 1.}
        assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize('ratio, box', [((0.5, 1.0), (0, 4, 40, 40)), ((1.5, 2.0), (4, 0, 32, 48)),
                                        ((0.75, 4 / 3), (0, 0, 40, 48))])
def test_fallback_box(ratio, box):
    P, B = 16, 8
    r = _recipe(crop=(24, 20), rrc=(4, 4) + ratio, flip=True)
    shard, labels = _shard(24, HS, WS)
    pool, _, pi, params = _build(shard, labels, r, P, B)
    assert bool((params[:, 7] == 10).all())
    assert torch.equal(params[:, [0, 1, 8, 9]], torch.tensor([[float(v) for v in box]] * P))
    worst, _ = _check(pool, params, pi, shard, r)
    print('fallback %r: worst err - bound = %.3g' % (ratio, worst))


JITTER = {
    'full': (OLD_CASES['full'][0], dict(OLD_CASES['full'][3], jitter=JIT)),
    'nonsquare_cutout': (OLD_CASES['nonsquare_cutout'][0],
                         dict(OLD_CASES['nonsquare_cutout'][3], jitter=JIT)),
    'rrc': ((24, HS, WS), dict(crop=(24, 20), rrc=RRC_A, flip=True, jitter=JIT, mean=MEAN, std=STD,
                               cutout=6)),
    'brightness': ((24, HS, WS), dict(crop=(24, 20), rrc=RRC_A, jitter=(0.8, 0, 0, 0))),
    'contrast': ((24, HS, WS), dict(crop=(24, 20), rrc=RRC_A, jitter=(0, 0.8, 0, 0))),
    'saturation': ((24, HS, WS), dict(crop=(24, 20), rrc=RRC_A, jitter=(0, 0, 0.8, 0))),
    'hue': ((24, HS, WS), dict(crop=(24, 20), rrc=RRC_A, jitter=(0, 0, 0, 0.5))),
    'pad_contrast': ((24, 32, 32), dict(crop=(32, 32), pad=4, flip=True, jitter=(0, 0.8, 0, 0))),
}


@pytest.mark.parametrize('case', sorted(JITTER))
def test_jitter_matches_reference(case):
    P, B = 64, 8
    (Ns, Hs, Ws), kw = JITTER[case]
    r = _recipe(**kw)
    shard, labels = _shard(Ns, Hs, Ws)
    pool, pl, pi, params = _build(shard, labels, r, P, B)
    assert torch.equal(pl.long(), labels[pi.long()])
    worst, worst_mean = _check(pool, params, pi, shard, r)
    print('jitter %s: worst err - bound = %.3g, worst grey-mean error = %.3g'
          % (case, worst, worst_mean))
    # the draws are the replay's
    want = po.jitter_draws(SEED, 0, P, B, r.jitter)
    got = params[:, 10:15].double().numpy()
    assert np.abs(got[:, :4] - np.array([w[:4] for w in want])).max() <= 1e-6
    assert got[:, 4].astype(int).tolist() == [w[4] for w in want]
    lo = [max(0.0, 1 - s) for s in r.jitter[:3]]
    for k in range(3):
        assert got[:, k].min() >= lo[k] and got[:, k].max() <= 1 + r.jitter[k]
        assert (got[:, k].max() > got[:, k].min()) == (r.jitter[k] > 0)
    assert np.abs(got[:, 3]).max() <= r.jitter[3]
    ran = r.jitter[1] > 0
    assert bool((params[:, 15] > 0).all()) if ran else bool((params[:, 15] == 0).all())
    if all(r.jitter):
        pos, before = po.contrast_coverage(want)
        assert pos == {0, 1, 2, 3} and before == {0, 2, 3}
    if r.rrc is None:
        # the old geometry draws what the same recipe draws without jitter
        plain = _build(shard, labels, _recipe(**dict(kw, jitter=None)), P, B)
        assert torch.equal(plain[3][:, :7], params[:, :7]) and torch.equal(plain[2], pi)
        assert bool((params[:, 7:10] == 0).all())
        assert not torch.equal(plain[0].view(torch.int16), pool.view(torch.int16))


def test_deterministic_identity_and_cutout():
    P, B = 16, 8
    shard, labels = _shard(24, HS, WS)
    kw = dict(crop=(24, 20), rrc=(0.08, 1.0, 1.5, 2.0), flip=True, jitter=JIT, mean=MEAN, std=STD,
              cutout=8)
    r = _recipe(**kw)
    one = _build(shard, labels, r, P, B, pc=1)
    two = _build(shard, labels, r, P, B, pc=1)
    assert torch.equal(one[0].view(torch.int16), two[0].view(torch.int16))
    assert torch.equal(one[3].view(torch.int32), two[3].view(torch.int32))
    assert not torch.equal(one[3], _build(shard, labels, r, P, B, pc=2)[3])
    # augment=False: identity factors, order 0, no flip, the fallback box, no hole
    off = _build(shard, labels, r, P, B, pc=1, augment=False)
    want = torch.tensor([[4., 0., 0., 0., 1., 0., 0., 10., 32., 48., 1., 1., 1., 0., 0.]] * P)
    assert torch.equal(off[3][:, :15], want)
    worst, _ = _check(off[0], off[3], off[2], shard, dataclasses.replace(r, cutout=0))
    print('augment=False: worst err - bound = %.3g' % worst)
    # Cutout: its square is zero, nothing else changes
    plain = _build(shard, labels, _recipe(**dict(kw, cutout=0)), P, B, pc=1)
    assert torch.equal(plain[3], one[3])
    H, W = 24, 20
    holes = 0
    for s in range(P):
        cy, cx = int(one[3][s, 5]), int(one[3][s, 6])
        y1, y2 = int(np.clip(cy - 4, 0, H)), int(np.clip(cy + 4, 0, H))
        x1, x2 = int(np.clip(cx - 4, 0, W)), int(np.clip(cx + 4, 0, W))
        hole = torch.zeros(H, W, dtype=torch.bool)
        hole[y1:y2, x1:x2] = True
        holes += int(hole.sum())
        a, b = one[0][s].view(torch.int16), plain[0][s].view(torch.int16)
        assert bool((a[hole] == 0).all()) and torch.equal(a[~hole], b[~hole])
    assert holes > 0


def test_argument_checks():
    ops = _ops()
    shard, labels = _shard(24, HS, WS)
    r = _recipe(crop=(24, 20), rrc=RRC_A, jitter=JIT)
    z = torch.zeros(16, 24, 20, 8, dtype=torch.bfloat16, device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)
    lab = labels.to(DEV)
    ctrl = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='params'):          # the 8-value buffer of other recipes
        ops.pool_build(shard.to(DEV), lab, ctrl, z, i, i.clone(), 16, 8, 0, recipe=r,
                       params=torch.zeros(16, 8, device=DEV))
    with pytest.raises(ValueError, match='uint8'):
        ops.pool_build(torch.zeros(24, HS, WS, 8, dtype=torch.bfloat16, device=DEV), lab, ctrl, z,
                       i, i.clone(), 16, 8, 0, recipe=r)
    with pytest.raises(ValueError, match='kernel of its own'):
        ops.pool_build(shard.to(DEV), lab, ctrl, z, i, i.clone(), 16, 8, 0, recipe=r,
                       force_augment_kernel=True)
    base = dict(shard=0, labels=0, ctrl=0, pool=0, pool_label=0, pool_index=0, stream=0, Ns=24,
                Hs=HS, Ws=WS, H=24, W=20, P=16, batch=8, augment=1, shuffle=1, seed=0, flip=1,
                mean=[0.0] * 3, inv_std=[1.0] * 3, Hr=HS, Wr=WS)
    photo = ops.lib().pool_recipe
    bad = [(dict(rrc=list(RRC_A), jitter=[0.4, 0.4, 0.4, 0.6]), 'hue'),
           (dict(rrc=list(RRC_A), jitter=[-0.1, 0, 0, 0]), '>= 0'),
           (dict(rrc=list(RRC_A), params=8, params_floats=16 * 8), 'P \\* 16'),
           (dict(rrc=[0.0, 1.0, 0.75, 1.33]), 'scale_lo'),
           (dict(rrc=[0.08, 1.0, 1.5, 0.75]), 'ratio_lo'),
           (dict(rrc=list(RRC_A), pad=4), 'replaces'),
           (dict(rrc=list(RRC_A), H=0), 'positive'),
           (dict(params=8, params_floats=16 * 16), 'P \\* 8'),   # neither field: the 8-float row
           (dict(jitter=list(JIT), Hr=16, Wr=16), 'resized size'),
           (dict(jitter=list(JIT), H=64, W=64), 'empty crop range')]
    for kw, word in bad:
        with pytest.raises(RuntimeError, match=word):
            photo(**dict(base, **kw))
    with pytest.raises(TypeError):                            # keyword arguments only
        photo(0, 0, 0, 0, 0, 0)
    # a recipe with neither field set meets the same geometry checks
    with pytest.raises(RuntimeError, match='empty crop range'):
        photo(**RAW_16_TO_32)


class _Set(object):
    def __init__(self, transform):
        self.transform = transform


class _Loader(object):
    def __init__(self, transform):
        self.dataset = _Set(transform)


def test_engine_trains_on_a_photo_recipe():
    """ResNet-18, B = 32, 10 pool batches, graphs on: the scored pool is the recipe's."""
    from mercury_amd.config import Config
    from mercury_amd.data import transforms as T
    from mercury_amd.engine.native import NativeEngine, _config_recipes
    from mercury_amd.models import ResNet18
    r = _recipe(crop=(32, 32), rrc=RRC_A, flip=True, jitter=JIT, mean=MEAN, std=STD)
    tf = T.Compose([T.ToPILImage(), T.RandomResizedCrop(32), T.RandomHorizontalFlip(),
                    T.ColorJitter(*JIT), T.ToTensor(), T.Normalize(MEAN, STD)])
    ev = T.Compose([T.ToPILImage(), T.Resize(32), T.RandomCrop(32), T.ToTensor(),
                    T.Normalize(MEAN, STD)])
    aug, ev_aug = _config_recipes(Config(augment='dataset'), _Loader(tf), _Loader(ev))
    assert aug == r and ev_aug == _recipe(resize=32, crop=32, mean=MEAN, std=STD)
    aug, ev_aug = _config_recipes(Config(augment=r.spec()), None, None)
    assert aug == r and ev_aug == _recipe(crop=(32, 32), rrc=RRC_A, mean=MEAN, std=STD)
    shard = _noise(640, 40, 40, 6)
    labels = torch.arange(640) % 10
    torch.manual_seed(0)
    eng = NativeEngine(ResNet18(10).to(DEV), DEV, 32, 10, image_hw=(32, 32), augment=r,
                       eval_augment=ev_aug, use_graphs=True)
    try:
        eng.set_shard(shard.numpy(), labels.numpy())
        assert eng.aug_params.shape == (320, 16)
        eng.prime()
        eng.step()
        eng.build_graphs()
        eng.step()
        torch.cuda.synchronize()
        sm = eng.score_mode
        pool = sm.input.view(320, 32, 32, 8).cpu()
        index = sm.index.cpu()
        assert torch.equal(sm.label.cpu().long(), labels[index.long()])
        params = eng.aug_params.cpu()
        worst, _ = _check(pool[:64], params[:64], index[:64], shard, r)
        print('engine: worst err - bound = %.3g' % worst)
        assert len(set(params[:, 14].tolist())) > 8 and float(params[:, 8].min()) >= 1
        m = eng.read_meters()
        assert all(math.isfinite(v) for v in m.values()) and m['count'] > 0
        # evaluation under the rrc recipe (it simply runs): finite, and the same on a second call
        x, y = _noise(500, 40, 40, 8).numpy(), np.arange(500) % 10
        first = eng.evaluate_arrays(x, y)
        assert first == eng.evaluate_arrays(x, y) and first[2] == 500
        assert math.isfinite(first[0])
    finally:
        eng.close()
    torch.manual_seed(0)
    eng = NativeEngine(ResNet18(10).to(DEV), DEV, 32, 10, image_hw=(32, 32),
                       augment=_recipe(crop=(32, 32), flip=True), use_graphs=False)
    try:
        eng.set_shard(shard.numpy(), labels.numpy())
        assert eng.aug_params.shape == (320, 8)
    finally:
        eng.close()
