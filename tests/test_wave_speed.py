"""``WaveRecipe.speed`` on the CPU: the polyphase resampler of ``reference`` against analytic
tones, the identity rate, and the recipe's strings and refusals."""
import math

import pytest
import torch

from mercury_amd.data.augment import SPEED_NT, WaveRecipe, speed_resample


@pytest.mark.parametrize('rate', [0.9, 1.05, 1.1])
@pytest.mark.parametrize('f', [0.01, 0.1, 0.2, 0.3])
def test_tones_through_the_resampler(f, rate):
    """Bound 5e-4: the Kaiser ripple at beta 8 (8.6e-5) plus the phase interpolation's
    (pi / 64)^2 / 8 = 3.0e-4, with margin; fp64 evaluation of the formulas gives 1.57e-4 at
    f = 0.3."""
    L, rq = 4000, int(round(rate * 65536))
    c = L >> 1
    x = torch.sin(2 * math.pi * f * torch.arange(L, dtype=torch.float64) + 0.3)
    js = torch.arange(L)
    got = speed_resample(x, js, rq, WaveRecipe(speed=(0.9, 1.1)).speed_table())
    at = c + (js - c).double() * rq / 65536
    keep = (at >= SPEED_NT) & (at <= L - 1 - SPEED_NT)
    assert int(keep.sum()) > L // 2
    err = (got - torch.sin(2 * math.pi * f * at + 0.3)).abs()[keep].max()
    print('f = %g rate = %g: worst error %.3g' % (f, rate, err))
    assert err <= 5e-4


def test_identity_rate_is_the_recipe_without_speed():
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3300, generator=g) * 2 - 1).mul(32767).round().to(torch.int16)
    kw = dict(n_fft=200, hop=100, shift=150, gain=(0.5, 2.0), tmask=(2, 3), mel=40)
    old, new = WaveRecipe(**kw), WaveRecipe(speed=(1, 1), **kw)
    p = new.draw(3300, generator=g)
    assert p[14] == 0 and p[0] != 0 and new.speed_rq() == (65536, 65536)
    assert torch.equal(new.reference(x, None, p, torch.float64),
                       old.reference(x, None, p, torch.float64))
    q = WaveRecipe(speed=(0.9, 1.1), **kw).draw(3300, generator=g)
    assert 58982 - 65536 <= q[14] <= 72090 - 65536


def test_strings_and_refusals():
    old = 'wave:nfft=200,hop=100,shift=1600,eps=1e-06,fmask=0x0,tmask=0x0,fill=0.0'
    assert WaveRecipe(shift=1600).spec() == old and WaveRecipe.parse(old).speed is None
    r = WaveRecipe.parse(old + ',speed=0.9:1.1')
    assert r.speed == (0.9, 1.1) and r.spec() == old + ',speed=0.9:1.1'
    assert WaveRecipe.parse(r.spec()) == r and r != WaveRecipe.parse(old)
    assert r.out_hw(16000) == (101, 161) and not r.identity and WaveRecipe(speed=(1, 1)).identity
    assert tuple(r.speed_table().shape) == (65, 32) and r.speed_table().dtype == torch.float32
    assert torch.equal(r.speed_table()[64, 1:], r.speed_table()[0, :-1])      # the wrap row
    for bad in ((0.4, 1.0), (1.1, 0.9), (1.0, 2.5), (float('nan'), 1.0), (1.0,)):
        with pytest.raises(ValueError, match='speed'):
            WaveRecipe(speed=bad)
    with pytest.raises(ValueError, match='speed'):
        WaveRecipe.parse('wave:speed=0.9')
    with pytest.raises(ValueError, match='speed'):
        WaveRecipe().speed_table()
    with pytest.raises(ValueError, match='speed'):
        WaveRecipe().reference(torch.zeros(300), None, [0.0, 1.0] + [0.0] * 12 + [5.0, 0.0])
