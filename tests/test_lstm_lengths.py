"""CPU tests of lengths in the native BiLSTM cell's arithmetic: ``ops.lstm.emulate(x, lstm, lens)``
implements the masking rules of the step kernels (``csrc/lstm.hip``) in plain torch -- a padded
frame stores ``h = +0``, ``c = 0``, ``dG = 0`` and ``dc = 0`` by a select -- no GPU needed.

It is held to fp64 packed ``nn.LSTM`` with bf16 packed ``nn.LSTM`` as the yardstick
(``lstm_packed_oracles``, the project's factor 2.5) on all ten tensors, with a finite and with a
NaN upstream gradient at the padded frames.
"""
import pytest
import torch

import lstm_oracles as lo
import lstm_packed_oracles as po
from mercury_amd.ops import lstm as L
from test_lstm_packed import SHAPES as PACKED_SHAPES

# the four shapes of test_lstm_packed.py, and one whose rows past the first 16-row tile are short:
# a tile that is fully valid, then padded, at the same step
SHAPES = list(PACKED_SHAPES) + [(9, 40, 40, 64, tuple([9] * 16 + [1] * 8 + [4] * 16))]
IDS = ['T%d_B%d_F%d_H%d' % s[:4] for s in SHAPES]


def _emu(m, x, lens):
    return L.emulate(x, m, lens)


def _same(a, b, what=''):
    for n, u, v in zip(lo.NAMES, a, b):
        assert torch.equal(u, v), '%s %s' % (what, n)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_emulate_with_lengths_vs_packed_fp64(shape):
    T, B, F, H, lens = shape
    lstm, x, gout, ref, tb = po.case(*shape)
    pad = po.padded(T, lens)
    got = po.run(_emu, lstm, x, gout, list(lens))
    lo.assert_vs_bf16(got, ref, tb, 'emulate lengths %r' % (shape[:4],))
    assert bool((got[0][pad] == 0).all()) and bool((got[1][pad] == 0).all())
    # NaN in the padded upstream gradient: pack / unpack drops it, so the references are the same
    gn = gout.clone()
    gn[pad] = float('nan')
    nan = po.run(_emu, lstm, x, gn, list(lens))
    lo.assert_vs_bf16(nan, ref, tb, 'emulate lengths, NaN gradient %r' % (shape[:4],))


@pytest.mark.parametrize('shape', SHAPES[:2] + SHAPES[4:], ids=IDS[:2] + IDS[4:])
def test_padding_has_no_influence(shape):
    T, B, F, H, lens = shape
    lstm = lo.make_lstm(F, H, 0)
    lens = list(lens)
    pad = po.padded(T, lens)
    x0, g0 = po.make_io(T, B, F, H, lens, pad_x=0.0, pad_g=0.0)
    want = po.run(_emu, lstm, x0, g0, lens)
    assert bool((want[0][pad] == 0).all()) and bool((want[1][pad] == 0).all())
    _, gn = po.make_io(T, B, F, H, lens, pad_g=float('nan'))
    xn, _ = po.make_io(T, B, F, H, lens, pad_x=float('nan'))
    assert bool(torch.isnan(gn).any()) and bool(torch.isnan(xn).any())
    for what, xi, gi in (('NaN gradient', x0, gn), ('NaN x', xn, g0), ('both', xn, gn)):
        got = po.run(_emu, lstm, xi, gi, lens)
        for n, v in zip(lo.NAMES, got):
            assert bool(torch.isfinite(v).all()), '%s %s' % (what, n)
        _same(want, got, what)


def test_forms_of_lengths():
    T, B, F, H = 5, 4, 40, 32
    lstm = lo.make_lstm(F, H, 0)
    x, gout = lo.make_io(T, B, F, H, 0)
    full = lo.run(L.emulate, lstm, x, gout)
    _same(full, po.run(_emu, lstm, x, gout, [T] * B), 'None vs [T]*B')
    _same(full, po.run(_emu, lstm, x, gout, None), 'None')
    want = po.run(_emu, lstm, x, gout, [5, 1, 3, 5])
    assert not torch.equal(want[0], full[0])
    for lens in (torch.tensor([5, 1, 3, 5]), torch.tensor([5, 1, 3, 5], dtype=torch.int32),
                 [5, 1, 3, 9], torch.tensor([99, 1, 3, 5], dtype=torch.int64)):   # above T: clamped
        _same(want, po.run(_emu, lstm, x, gout, lens), repr(lens))


def test_length_zero_row():
    T, B, F, H = 5, 4, 40, 32
    lstm = lo.make_lstm(F, H, 0)
    x, gout = lo.make_io(T, B, F, H, 0)
    zero = po.run(_emu, lstm, x, gout, [5, 0, 3, 2])
    one = po.run(_emu, lstm, x, gout, [5, 1, 3, 2])
    assert bool((zero[0][:, 1] == 0).all()) and bool((zero[1][:, 1] == 0).all())
    assert bool((one[0][0, 1] != 0).any())
    keep = [0, 2, 3]
    assert torch.equal(zero[0][:, keep], one[0][:, keep])
    # negative values are clamped to 0, and all rows may be empty
    _same(zero, po.run(_emu, lstm, x, gout, [5, -3, 3, 2]), 'negative')
    none = po.run(_emu, lstm, x, gout, [0] * B)
    for n, v in zip(lo.NAMES, none):
        assert bool((v == 0).all()), n


def test_refusals():
    T, B, F, H = 5, 4, 40, 32
    lstm = lo.make_lstm(F, H, 0)
    x, _ = lo.make_io(T, B, F, H, 0)
    with pytest.raises(TypeError, match='lengths'):
        L.emulate(x, lstm, torch.tensor([5.0, 1.0, 3.0, 2.0]))
    with pytest.raises(TypeError, match='lengths'):
        L.emulate(x, lstm, torch.tensor([True, True, False, True]))
    with pytest.raises(ValueError, match='lengths'):
        L.emulate(x, lstm, [5, 1, 3])
    with pytest.raises(ValueError, match='lengths'):
        L.emulate(x, lstm, torch.tensor([[5, 1, 3, 2]]))
    # the native cell still refuses a CPU input, lengths or not
    with pytest.raises(ValueError, match='HIP device'):
        L.bilstm(x, lstm, [5, 1, 3, 2])
    # step level: device int32 only, and not together with an initial state
    with pytest.raises(ValueError, match='lengths'):
        L.lstm_step_fwd(None, None, None, None, T=T, B=B, H=H, lengths=torch.tensor([5, 1, 3, 2]))
    with pytest.raises(ValueError, match='lengths'):
        L.lstm_step_bwd(None, None, None, None, None, None, T=T, B=B, H=H,
                        lengths=torch.tensor([5, 1, 3, 2], dtype=torch.int32))


def test_eight_parameter_call_still_valid():
    T, B, F, H = 3, 4, 40, 32
    lstm = lo.make_lstm(F, H, 0)
    x, gout = lo.make_io(T, B, F, H, 0)
    params = [getattr(lstm, n) for n in L._PARAMS]
    xr = x.clone().requires_grad_()
    out = L.BiLSTMFunction.apply(False, True, xr, *params)
    out.backward(gout)
    assert torch.equal(out, L.emulate(x, lstm)) and xr.grad is not None
    assert 'MEASURED_NATIVE_PACKED' in dir(L) and isinstance(L.MEASURED_NATIVE_PACKED, frozenset)
