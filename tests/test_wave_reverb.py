"""``WaveRecipe.reverb`` on the CPU: ``reference`` with an RIR bank against ``conv1d`` in fp64, the
unit impulse, the spec round trip and the refusals, and the precedent check that carries the wave
pools' bounds over to reverberant clips.  ``clips`` and ``rirs`` are also the inputs of
``test_wave_reverb_gpu.py``."""
import pytest
import torch
import torch.nn.functional as F

from mercury_amd.data.augment import WaveRecipe, reverb_convolve
from mercury_amd.data.transforms import WaveSpectrogram

NS = 64
_MADE = {}


def clips(L, dtype):
    """(shard [NS][L], noise bank [3][L + 37], labels) of uniform noise in +-1/64; made once.
    Quiet on purpose: the workspace rounds every reverberant sample to fp32, about 2^-24 of the
    clip's level at every bin, which only ``eps`` bounds against a bin in a spectral null."""
    if (L, dtype) not in _MADE:
        g = torch.Generator().manual_seed(L)
        x, bank = ((torch.rand(n, m, generator=g) - 0.5) / 32 for n, m in ((NS, L), (3, L + 37)))
        if dtype == torch.int16:
            x, bank = ((t * 65534).round().to(torch.int16) for t in (x, bank))
        _MADE[L, dtype] = (x, bank, (torch.arange(NS) * 7) % 30)
    return _MADE[L, dtype]


def rirs(K):
    """[3][K] float32: white noise under an exponential decay (60 dB over K taps), h[0] = 1."""
    if K not in _MADE:
        g = torch.Generator().manual_seed(K)
        h = 0.3 * torch.randn(3, K, generator=g) * torch.exp(-6.9 * torch.arange(K) / K)
        h[:, 0] = 1.0
        _MADE[K] = h.float().contiguous()
    return _MADE[K]


@pytest.mark.parametrize('L, K', [(300, 5), (3300, 257), (700, 1024)])
def test_reference_matches_conv1d(L, K):
    x, h = clips(L, torch.int16)[0][3], rirs(K)
    r0, r = WaveRecipe(n_fft=30, hop=7), WaveRecipe(n_fft=30, hop=7, reverb=0.5)
    p = r.identity_params()
    p[15] = 3.0                                                     # response 2
    xd = x.double() / 32768
    y = F.conv1d(F.pad(xd, (K - 1, 0)).view(1, 1, -1), h[2].double().flip(0).view(1, 1, -1)).view(-1)
    assert y.shape[0] == L and float((reverb_convolve(xd, h[2]) - y).abs().max()) <= 1e-9
    want = r0.reference(y, None, r0.identity_params(), dtype=torch.float64)
    got = r.reference(x, None, p, dtype=torch.float64, rir=h)
    assert float((got - want).abs().max()) <= 1e-9


def test_unit_impulse_and_reverb_off_are_the_clip():
    x = clips(300, torch.float32)[0][0]
    h = torch.zeros(2, 9)
    h[:, 0] = 1.0
    r0, r = WaveRecipe(n_fft=30, hop=7, shift=4), WaveRecipe(n_fft=30, hop=7, shift=4, reverb=1.0)
    p = r.identity_params()
    p[0] = 3.0
    want = r0.reference(x, None, p, dtype=torch.float64)
    assert torch.equal(r.reference(x, None, p, dtype=torch.float64, rir=h), want)    # drawn off
    p[15] = 2.0
    assert torch.equal(r.reference(x, None, p, dtype=torch.float64, rir=h), want)
    t = WaveSpectrogram(r, rir=h, generator=torch.Generator().manual_seed(1))
    t(x)
    assert t.last[15] in (1.0, 2.0) and WaveSpectrogram(r, rir=h, augment=False)(x).shape[0] == 1


def test_spec_round_trip_and_old_recipes_unchanged():
    r = WaveRecipe(n_fft=64, hop=16, mel=20, cmvn=2, preemph=0.97, reverb=0.5)
    assert r.spec().endswith('cmvn=2,preemph=0.97,reverb=0.5') and WaveRecipe.parse(r.spec()) == r
    assert WaveRecipe(reverb=0.0) == WaveRecipe() and not r.identity
    assert WaveRecipe().spec() == 'wave:nfft=200,hop=100,shift=0,eps=1e-06,fmask=0x0,tmask=0x0,fill=0.0'
    assert r.out_hw(3300) == WaveRecipe(n_fft=64, hop=16, mel=20).out_hw(3300)


@pytest.mark.parametrize('reverb, shape', [(0.5, None), (0.0, (2, 8)), (0.5, (2, 0)),
                                           (0.5, (2, 4097)), (0.5, (0, 8)), (0.5, (8,))])
def test_refusals(reverb, shape):
    with pytest.raises(ValueError):
        WaveRecipe(reverb=reverb).check(3300, None, shape)
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            WaveRecipe(reverb=bad)
    with pytest.raises(ValueError):
        WaveSpectrogram(WaveRecipe(reverb=0.5), rir=torch.zeros(2, 8, dtype=torch.float64))


@pytest.mark.parametrize('dtype', [torch.int16, torch.float32], ids=['int16', 'float32'])
def test_fp32_convolution_carries_the_pool_bounds(dtype):
    """The GPU test's clips under its responses: an fp32 convolution fed to the fp64 front end
    moves each bin's power by at most ``2e-4 (p_k + eps)``, a tenth of the linear kernel's per-bin
    bound ``2e-3 (p_k + eps)`` (``test_wave_gpu.py``), so the wave pools' bounds carry over."""
    L, K = 3300, 257
    x, h = clips(L, dtype)[0], rirs(K)
    x32 = x.float() / 32768 if dtype == torch.int16 else x
    r = WaveRecipe(n_fft=200, hop=100)
    worst = 0.0
    for i in range(NS):
        hk = h[i % 3]
        y32 = F.conv1d(F.pad(x32[i], (K - 1, 0)).view(1, 1, -1), hk.flip(0).view(1, 1, -1)).view(-1)
        ln = [r.reference(y, None, r.identity_params(), dtype=torch.float64)[:, :, 0]
              for y in (y32.double(), reverb_convolve(x32[i], hk))]
        worst = max(worst, float(torch.expm1(ln[0] - ln[1]).abs().max()))    # |dp| / (p + eps)
    print('%s: worst |dp| / (p + eps) = %.3g' % (dtype, worst))
    assert worst <= 2e-4
