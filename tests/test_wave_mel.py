"""``WaveRecipe`` with ``mel`` / ``dct`` on the CPU: tables against their formulas, ``reference``
against ``torch.stft`` pushed through them, spec round trip, refusals, ``WaveSpectrogram``."""
import math

import pytest
import torch

from mercury_amd.data.augment import WaveRecipe
from mercury_amd.data.transforms import WaveSpectrogram

MEL = [dict(n_fft=200, hop=100, mel=80), dict(n_fft=64, hop=16, mel=20),
       dict(n_fft=512, hop=128, mel=128, sr=22050, fmin=60.0, fmax=7600.0),
       dict(n_fft=30, hop=7, mel=8, sr=8000)]


@pytest.mark.parametrize('kw', MEL, ids=lambda k: '%dx%d' % (k['n_fft'], k['mel']))
def test_mel_table_is_the_htk_triangles(kw):
    r = WaveRecipe(**kw)
    F, M = r.n_fft // 2 + 1, r.mel
    tab = r.mel_table()
    assert tab.dtype == torch.float32 and tab.shape == ((F + 15) // 16 * 16, (M + 15) // 16 * 16)
    assert not tab[F:].any() and not tab[:, M:].any()

    def mel(f):
        return 2595.0 * math.log10(1.0 + f / 700.0)
    top = r.sr / 2 if r.fmax is None else r.fmax
    lo, hi = mel(r.fmin), mel(top)
    f = [700.0 * (10.0 ** ((lo + (hi - lo) * i / (M + 1)) / 2595.0) - 1.0) for i in range(M + 2)]
    for k in range(F):
        g = k * (r.sr / 2) / (F - 1)
        for m in range(M):
            up, down = (g - f[m]) / (f[m + 1] - f[m]), (f[m + 2] - g) / (f[m + 2] - f[m + 1])
            want = max(0.0, min(up, down))
            assert abs(float(tab[k, m]) - want) <= 1e-6, (k, m)


@pytest.mark.parametrize('M, C', [(80, 13), (128, 40), (8, 8)])
def test_dct_is_orthonormal(M, C):
    r = WaveRecipe(mel=M, dct=C)
    D = WaveRecipe(mel=M, dct=M)._dct_mat()
    assert (D.t() @ D - torch.eye(M, dtype=torch.float64)).abs().max() < 1e-12
    tab = r.dct_table()
    assert tab.dtype == torch.float32 and tab.shape == ((M + 15) // 16 * 16, (C + 15) // 16 * 16)
    assert not tab[M:].any() and not tab[:, C:].any()
    assert (tab[:M, :C].double() - D[:, :C]).abs().max() < 1e-7


@pytest.mark.parametrize('dct', [0, 13])
def test_reference_is_torch_stft_through_the_tables(dct):
    r = WaveRecipe(n_fft=200, hop=100, mel=40, dct=dct, norm=(-5.0, 4.0), fmin=20.0, fmax=7000.0)
    L = 3300
    x = torch.randn(L, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    X = torch.stft(x, 200, 100, 200, torch.hann_window(200, dtype=torch.float64), center=True,
                   pad_mode='reflect', return_complex=True)
    y = torch.log((X.real ** 2 + X.imag ** 2).t() @ r._mel_fb() + r.eps)
    if dct:
        y = y @ r._dct_mat()
    a, b = r.affine()
    got = r.reference(x, None, r.identity_params(), dtype=torch.float64)
    assert got.shape == (dct or 40, 34, 8) and not got[:, :, 1:].any()
    assert (got[:, :, 0] - (a * y + b).t()).abs().max() < 1e-9


def test_spec_round_trip_and_old_recipes_unchanged():
    r = WaveRecipe.parse('wave:nfft=200,hop=100,mel=80,sr=16000,fmin=0,fmax=8000,dct=13')
    assert r == WaveRecipe(mel=80, sr=16000, fmin=0.0, fmax=8000.0, dct=13)
    assert WaveRecipe.parse(r.spec()) == r and r.out_hw(16000) == (13, 161)
    r = WaveRecipe(n_fft=64, hop=16, mel=20, sr=8000, fmin=50.0, fmask=(2, 5))
    assert WaveRecipe.parse(r.spec()) == r and r.fmax is None and r.out_hw(512) == (20, 33)
    with pytest.raises(ValueError, match='fmask'):      # checked against the rows, not the bins
        WaveRecipe(mel=40, fmask=(1, 41)).check(1000)
    old = WaveRecipe(shift=1600, gain=(0.8, 1.2), norm=(-5, 4), fmask=(2, 10), tmask=(2, 20))
    assert old.spec() == 'wave:nfft=200,hop=100,shift=1600,gain=0.8:1.2,eps=1e-06,' \
                         'norm=-5.0:4.0,fmask=2x10,tmask=2x20,fill=0.0'
    assert old.out_hw(16000) == (101, 161) and old == WaveRecipe.parse(old.spec())
    assert WaveRecipe(sr=8000).spec() == WaveRecipe().spec()


@pytest.mark.parametrize('kw, field', [
    (dict(mel=7), 'mel'), (dict(mel=129), 'mel'), (dict(mel=40, fmin=-1.0), 'fmin'),
    (dict(mel=40, fmin=4000.0, fmax=4000.0), 'fmin'), (dict(mel=40, fmax=8000.5), 'fmax'),
    (dict(mel=40, sr=8000, fmax=4001.0), 'fmax'), (dict(mel=40, dct=41), 'dct'),
    (dict(dct=13), 'dct'), (dict(mel=40, dct=-1), 'dct'),
    (dict(mel=40, dct=13, fmask=(1, 4)), 'fmask')])
def test_refusals_name_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        WaveRecipe(**kw)


def test_the_eager_transform_follows():
    r = WaveRecipe(n_fft=64, hop=16, mel=20, dct=10, shift=40, gain=(0.8, 1.2), tmask=(2, 5))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(512, generator=g)
    tf = WaveSpectrogram(r.spec(), generator=g)
    y = tf(x)
    assert y.shape == (1, 10, 33) and y.dtype == torch.float32
    assert torch.equal(y[0], r.reference(x, None, tf.last, dtype=torch.float32)[:, :, 0])
