"""``WaveRecipe`` delta rows and liftering on the CPU: ``reference`` against the operator written
out with ``F.pad(mode='replicate')`` + ``F.conv1d`` on the ``delta = 0`` reference, the lifter
against its formula, the spec round trip, and the refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

from mercury_amd.data.augment import WaveRecipe

BASE = dict(n_fft=64, hop=16, mel=20, dct=13, tmask=(1, 2), fill=-3.0)


def _delta(v, N):
    """torchaudio's compute_deltas(mode='replicate') on [R][T], fp64"""
    k = torch.arange(-N, N + 1, dtype=torch.float64).view(1, 1, -1)
    pad = F.pad(v.unsqueeze(1), (N, N), mode='replicate')
    return F.conv1d(pad, k).squeeze(1) / (2 * sum(n * n for n in range(1, N + 1)))


@pytest.mark.parametrize('L', [200, 40], ids=['T13', 'T3'])        # T = 3 < 2N + 1 for N >= 2
@pytest.mark.parametrize('N', [1, 2, 4])
@pytest.mark.parametrize('order', [1, 2])
def test_reference_matches_the_written_out_operator(order, N, L):
    x = 0.3 * torch.randn(L, generator=torch.Generator().manual_seed(L + N))
    r0 = WaveRecipe(**BASE)
    r = WaveRecipe(**BASE, norm=(-5.0, 4.0), delta=order, dwin=N)
    p = r.identity_params()
    p[10:12] = [1.0, 1.0]                                          # a time band at frame 1
    R, T = r0.out_hw(L)
    assert r.out_hw(L) == ((1 + order) * R, T)
    v = r0.reference(x, None, r0.identity_params(), dtype=torch.float64)[:, :, 0]
    want, d = [v / 4.0 + 1.25], v
    for _ in range(order):
        d = _delta(d, N)
        want.append(d / 4.0)
    want = torch.cat(want)
    want[:, 1] = -3.0
    got = r.reference(x, None, p, dtype=torch.float64)
    assert got.shape == ((1 + order) * R, T, 8) and bool((got[:, :, 1:] == 0).all())
    assert float((got[:, :, 0] - want).abs().max()) <= 1e-9


def test_frequency_band_fills_the_row_of_every_block():
    r = WaveRecipe(n_fft=64, hop=16, mel=20, fmask=(1, 3), fill=9.0, delta=2)
    p = r.identity_params()
    p[6:8] = [4.0, 2.0]
    y = r.reference(torch.randn(200), None, p, dtype=torch.float64)[:, :, 0]
    filled = (y == 9.0).all(1)
    assert torch.nonzero(filled).view(-1).tolist() == [4, 5, 24, 25, 44, 45]


def test_lifter_scales_the_dct_columns():
    r0, r = WaveRecipe(**BASE), WaveRecipe(**BASE, lifter=22)
    j = torch.arange(13, dtype=torch.float64)
    want = r0._dct_mat() * (1 + 11.0 * torch.sin(math.pi * j / 22))
    assert float((r._dct_mat() - want).abs().max()) <= 1e-12
    assert torch.equal(r.dct_table()[:20, :13], want.float())


def test_spec_round_trip_and_old_recipes_unchanged():
    r = WaveRecipe(**BASE, delta=2, dwin=3, lifter=22)
    assert r.spec().endswith('dct=13,delta=2,dwin=3,lifter=22')
    assert WaveRecipe.parse(r.spec()) == r
    assert WaveRecipe.parse('wave:nfft=64,hop=16,mel=20,delta=1') == \
        WaveRecipe(n_fft=64, hop=16, mel=20, delta=1, dwin=2)
    old = WaveRecipe(**BASE)
    assert old.spec() == ('wave:nfft=64,hop=16,shift=0,eps=1e-06,fmask=0x0,tmask=1x2,fill=-3.0,'
                          'mel=20,sr=16000,fmin=0.0,dct=13')
    assert old.out_hw(200) == (13, 13) and WaveRecipe().out_hw(16000) == (101, 161)


@pytest.mark.parametrize('kw', [
    dict(delta=1), dict(mel=20, delta=3), dict(mel=20, delta=-1), dict(mel=20, delta=1, dwin=0),
    dict(mel=20, delta=1, dwin=5), dict(mel=20, lifter=22), dict(mel=20, dct=13, lifter=-1)])
def test_refusals(kw):
    with pytest.raises(ValueError):
        WaveRecipe(**kw)


def test_check_refuses_a_mask_wider_than_one_block():
    with pytest.raises(ValueError, match='fmask'):
        WaveRecipe(n_fft=64, hop=16, mel=20, delta=2, fmask=(1, 21)).check(200)
