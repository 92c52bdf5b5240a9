"""Speed perturbation in the waveform pools (``wave_stage_speed``, the ``SPEED`` instantiations
of ``pool_wave_kernel`` and ``pool_wave_mel_kernel``): every element of every slot against
``WaveRecipe.reference`` in fp64, fed with the kernel's own params row.  The bounds are those of
``test_wave_gpu.py``, ``test_wave_mel_gpu.py`` and ``test_wave_delta_gpu.py`` for the same kind
of recipe: ``2^-8 |ref| + 2e-3 |a| S_r g^k``, ``S_r`` = 1 (linear), ``max(1, s_m)`` (log-mel),
``sum_m |D[m][j]| max(1, s_m)`` (MFCC), ``g = 3 / (2 N + 1)`` per delta order k.  The FIR's own
fp32 error, about ``32 * 2^-23 max|x| sum|w|`` per sample, is far below ``eps``'s share."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 7.0
P, B, NS, SEED = 48, 8, 20, 11
# (n_fft, hop, L, recipe fields): linear, two chunks | both folds and both clip ends in one
# block | the largest K and the widest panel | MFCC with delta rows (a frame halo)
SHAPES = [(200, 100, 3300, {}), (30, 7, 300, dict(mel=8, dct=8)), (512, 128, 2048, dict(mel=128)),
          (200, 100, 3300, dict(mel=80, dct=13, delta=2))]
IDS = ['linear', 'w30mfcc', 'w512mel', 'delta']
_CLIPS = {}


def _clips(L, dtype):
    """(shard [NS][L], noise bank [3][L + 37], labels) of uniform noise; made once."""
    if (L, dtype) not in _CLIPS:
        g = torch.Generator().manual_seed(L)
        x, bank = (torch.rand(n, m, generator=g) - 0.5 for n, m in ((NS, L), (3, L + 37)))
        if dtype == torch.int16:
            x, bank = ((t * 65534).round().to(torch.int16) for t in (x, bank))
        _CLIPS[L, dtype] = (x, bank, (torch.arange(NS) * 7) % 30)
    return _CLIPS[L, dtype]


def _recipe(shape, speed, full=False):
    from mercury_amd.data.augment import WaveRecipe
    W, hop, _, kw = shape
    kw = dict(kw, shift=W, speed=speed)
    if full:
        kw.update(gain=(0.5, 2.0), noise=(0.7, 0.5), norm=(-5.0, 4.0), tmask=(2, 3), fill=-1.5,
                  fmask=(0, 0) if kw.get('dct') else (2, 3))
    return WaveRecipe(n_fft=W, hop=hop, **kw)


def _build(x, bank, labels, recipe, augment=True, chunks=0):
    """One pool build between two guard slots -> (pool, indices, params) on the host; a forced
    chunk count goes past ``ops.pool_build``, which leaves the count to the launcher."""
    from mercury_amd import ops
    from mercury_amd.ops.importance import _pool_wave
    R, T = recipe.out_hw(x.shape[1])
    ctrl = torch.tensor([2, 0, 0, 0], device=DEV)
    big = torch.full((P + 2, R, T, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pl, pi = (torch.full((P,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    params = torch.full((P, 16), -99.0, device=DEV)
    noise = bank.to(DEV) if recipe.noise else None
    if chunks:
        _pool_wave(x.to(DEV), noise, labels.to(DEV), ctrl, big[1:P + 1], pl, pi, P, B, SEED,
                   augment, True, None, recipe, params, chunks=chunks)
    else:
        ops.pool_build(x.to(DEV), labels.to(DEV), ctrl, big[1:P + 1], pl, pi, P, B, SEED,
                       recipe=recipe, params=params, noise=noise, augment=augment)
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all())
    return big[1:P + 1], pi.cpu(), params.cpu()


@pytest.mark.parametrize('speed, full, dtype', [
    ((0.9, 1.1), False, torch.int16), ((0.9, 1.1), False, torch.float32),
    ((0.5, 0.5), False, torch.int16), ((0.5, 0.5), False, torch.float32),
    ((2.0, 2.0), False, torch.int16), ((2.0, 2.0), False, torch.float32),
    ((0.9, 1.1), True, torch.int16)], ids=lambda v: str(v).replace('torch.', ''))
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pool_matches_reference(shape, speed, full, dtype):
    r = _recipe(shape, speed, full)
    x, bank, labels = _clips(shape[2], dtype)
    pool, pi, params = _build(x, bank, labels, r)
    lo, hi = r.speed_rq()
    rate = params[:, 14]
    assert bool(((rate >= lo - 65536) & (rate <= hi - 65536)).all()) and bool((rate != 0).any())
    assert len(set(rate.tolist())) > 1 or lo == hi
    assert bool((params[:, 0] != 0).any()) and bool((params[:, 15] == 0).all())
    if r.mel:
        scale = r._mel_fb().sum(0).clamp(min=1.0)
        if r.dct:
            scale = (r._dct_mat().abs() * scale.view(-1, 1)).sum(0)
        scale = torch.cat([scale * (3.0 / (2 * r.dwin + 1)) ** k for k in range(r.delta + 1)])
    else:
        scale = torch.ones(r.out_hw(shape[2])[0], dtype=torch.float64)
    worst = -math.inf
    for i in range(P):
        ref = r.reference(x[int(pi[i])], bank, params[i].tolist(), dtype=torch.float64)[:, :, 0]
        err = (pool[i, :, :, 0].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2e-3 * abs(r.affine()[0]) * scale.view(-1, 1)
        worst = max(worst, float((err - bound).max()))
    print('%s speed=%s full=%d %s: worst err - bound = %.3g' % (shape, speed, full, dtype, worst))
    assert worst <= 0


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_augment_off_is_the_pool_without_speed(shape):
    x, bank, labels = _clips(shape[2], torch.int16)
    off = _build(x, bank, labels, _recipe(shape, (0.9, 1.1), True), augment=False)
    want = _build(x, bank, labels, _recipe(shape, None, True), augment=False)
    assert bool((off[2][:, 14] == 0).all()) and torch.equal(off[2], want[2])
    assert torch.equal(off[0].view(torch.int16), want[0].view(torch.int16))


@pytest.mark.parametrize('shape, counts', [(SHAPES[0], (2, 3)), (SHAPES[3], (2, 3))],
                         ids=[IDS[0], IDS[3]])
def test_pools_of_different_chunk_counts_are_bit_equal(shape, counts):
    x, bank, labels = _clips(shape[2], torch.int16)
    r = _recipe(shape, (0.9, 1.1), True)
    a, b = (_build(x, bank, labels, r, chunks=n)[0].view(torch.int16) for n in counts)
    assert torch.equal(a, b)
    big = _clips(16000, torch.int16)        # two chunks of 6 tiles: 39 KB alone, 125 KB at rate 2
    _build(*big, _recipe((200, 100, 16000, {}), None), chunks=2)
    with pytest.raises(ValueError, match='LDS'):
        _build(*big, _recipe((200, 100, 16000, {}), (2, 2)), chunks=2)
