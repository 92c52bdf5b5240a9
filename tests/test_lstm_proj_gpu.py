"""GPU tests of the BiLSTM layer's native GEMMs (``csrc/lstm_proj.hip``) and of
``ops.lstm.bilstm(..., proj='native')``.

The three kernels are held to fp64 ``einsum`` references of the same bf16-valued inputs with the
elementwise criterion of ``kernel_oracles``: ``|got - ref| <= K * mag``, K = 1e-5, ``mag`` = the
sum of |terms| (with ``|b|`` for ``pre``); every output is pre-filled with NaN, so an element
that is not written fails.  The layer is held to ``lstm_oracles`` (2.5 x the error of CPU bf16
``nn.LSTM`` against fp64 ``nn.LSTM``) and, with lengths, to exact zeros and bit-equality.

Printed on an MI355X (largest KNEED over the cases; K is 1e-5): lstm_proj_fwd 1.0e-07,
lstm_proj_dx 9.9e-08, lstm_proj_wgrad_dw_ih 1.0e-07, lstm_proj_wgrad_dw_hh 8.6e-08,
lstm_proj_wgrad_db 4.9e-09.  RATIO (error / torch-bf16 error, bound 2.5) over the two sequence
shapes: out 0.86-0.89, dx 0.79, parameter gradients 0.74-0.89.
"""
import pytest
import torch

import lstm_oracles as lo
from kernel_oracles import BF16, F64, assert_within, record

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')

# (T, B, F, H): one live row; K < 32 and an ld tail with rows under 16; M across a tile edge with
# B no multiple of 16 and 8H = 768; 32 K-steps
SHAPES = [(1, 1, 8, 32), (3, 5, 101, 32), (7, 37, 101, 96), (2, 16, 1024, 32)]
SEQ_SHAPES = [(5, 33, 40, 96), (4, 32, 101, 512)]


def _L():
    from mercury_amd.ops import lstm as L
    return L


def _inputs(T, B, F, H):
    """bf16-valued operands in the kernels' layouts (CPU): xb [T*B][ld] and w_ih [2][4H][ld] with
    zero columns past F, b, dG [T][2][B][4H], out [T][B][2H]."""
    g = torch.Generator().manual_seed(T * 100003 + B * 1009 + F * 31 + H)
    ld = _L().proj_ld(F)
    xb = torch.zeros(T * B, ld, dtype=BF16)
    xb[:, :F] = torch.randn(T * B, F, generator=g)
    w = torch.zeros(2, 4 * H, ld, dtype=BF16)
    w[:, :, :F] = torch.randn(2, 4 * H, F, generator=g) / F ** 0.5
    b = torch.randn(2, 4 * H, generator=g)
    dG = torch.randn(T, 2, B, 4 * H, generator=g).to(BF16)
    out = torch.randn(T, B, 2 * H, generator=g).to(BF16)
    return xb, w, b, dG, out


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


@pytest.mark.parametrize('T,B,F,H', SHAPES)
def test_proj_fwd(T, B, F, H):
    xb, w, b, _, _ = _inputs(T, B, F, H)
    pre = _nan(T, 2, B, 4 * H)
    _L().lstm_proj_fwd(xb.to(DEV), w.to(DEV), b.to(DEV), pre, T=T, B=B, F=F, H=H)
    x64, w64 = xb.to(F64).view(T, B, -1), w.to(F64)
    ref = torch.einsum('tbk,dnk->tdbn', x64, w64) + b.to(F64)[None, :, None, :]
    mag = torch.einsum('tbk,dnk->tdbn', x64.abs(), w64.abs()) + b.to(F64).abs()[None, :, None, :]
    record('lstm_proj_fwd', assert_within(pre.cpu(), ref, mag, what='pre %r' % ((T, B, F, H),)))


@pytest.mark.parametrize('T,B,F,H', SHAPES)
def test_proj_dx(T, B, F, H):
    _, w, _, dG, _ = _inputs(T, B, F, H)
    wT = w[:, :, :F].transpose(1, 2).contiguous()                     # [2][F][4H]
    dx = _nan(T * B, F)
    _L().lstm_proj_dx(dG.to(DEV), wT.to(DEV), dx, T=T, B=B, F=F, H=H)
    g64, w64 = dG.to(F64), wT.to(F64)
    ref = torch.einsum('tdbj,dcj->tbc', g64, w64).reshape(T * B, F)
    mag = torch.einsum('tdbj,dcj->tbc', g64.abs(), w64.abs()).reshape(T * B, F)
    record('lstm_proj_dx', assert_within(dx.cpu(), ref, mag, what='dx %r' % ((T, B, F, H),)))


def _wgrad(T, B, F, H, ops):
    xb, _, _, dG, out = ops
    dw_ih, dw_hh, db = _nan(2, 4 * H, F), _nan(2, 4 * H, H), _nan(2, 4 * H)
    _L().lstm_proj_wgrad(dG.to(DEV), xb.to(DEV), out.to(DEV), dw_ih, dw_hh, db, T=T, B=B, F=F, H=H)
    return dw_ih.cpu(), dw_hh.cpu(), db.cpu()


@pytest.mark.parametrize('T,B,F,H', SHAPES + [(2, 3, 40, 32)])
def test_proj_wgrad(T, B, F, H):
    ops = _inputs(T, B, F, H)
    xb, _, _, dG, out = ops
    dw_ih, dw_hh, db = _wgrad(T, B, F, H, ops)
    g64, x64, o64 = dG.to(F64), xb.to(F64).view(T, B, -1)[:, :, :F], out.to(F64)
    hp = torch.zeros(T, 2, B, H, dtype=F64)           # h_prev: out[t-1] forward, out[t+1] reverse
    hp[1:, 0], hp[:-1, 1] = o64[:-1, :, :H], o64[1:, :, H:]
    what = ' %r' % ((T, B, F, H),)
    for name, got, ref, mag in (
            ('dw_ih', dw_ih, torch.einsum('tdbn,tbc->dnc', g64, x64),
             torch.einsum('tdbn,tbc->dnc', g64.abs(), x64.abs())),
            ('dw_hh', dw_hh, torch.einsum('tdbn,tdbc->dnc', g64, hp),
             torch.einsum('tdbn,tdbc->dnc', g64.abs(), hp.abs())),
            ('db', db, g64.sum((0, 2)), g64.abs().sum((0, 2)))):
        record('lstm_proj_wgrad_' + name, assert_within(got, ref, mag, what=name + what))
    if T == 1:
        assert not bool(dw_hh.any())


def test_proj_wgrad_is_deterministic():
    ops = _inputs(7, 37, 101, 96)
    for a, b in zip(_wgrad(7, 37, 101, 96, ops), _wgrad(7, 37, 101, 96, ops)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ the layer
def _native(x, m, lengths=None):
    return _L().bilstm(x, m, lengths, proj='native')


@pytest.mark.parametrize('T,B,F,H', SEQ_SHAPES)
def test_layer_against_fp64(T, B, F, H):
    lstm, x, gout, ref, tb = lo.case(T, B, F, H)
    lo.assert_vs_bf16(lo.run(_native, lstm, x, gout, DEV), ref, tb, 'proj native %r' % ((T, B, F, H),))


@pytest.mark.parametrize('T,B,F,H', SEQ_SHAPES)
def test_layer_lengths_keep_padding_out(T, B, F, H):
    lstm, x, gout = lo.case(T, B, F, H)[:3]
    lens = ([T, 1, 0, T // 2] * B)[:B]
    pad = torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]             # [T][B]
    fn = lambda a, m: _native(a, m, lens)
    zero = lo.run(fn, lstm, x.masked_fill(pad[:, :, None], 0.), gout.masked_fill(pad[:, :, None], 0.), DEV)
    got = lo.run(fn, lstm, x.masked_fill(pad[:, :, None], NAN), gout.masked_fill(pad[:, :, None], NAN), DEV)
    assert not bool(got[1][pad].any()), 'dx at padded frames'
    for n, g, z in zip(lo.NAMES, got, zero):
        assert bool(torch.isfinite(g).all()), n
        assert torch.equal(g, z), n


@pytest.mark.parametrize('T,B,F,H', SEQ_SHAPES)
def test_proj_torch_is_the_default(T, B, F, H):
    L = _L()
    lstm, x, gout = lo.case(T, B, F, H)[:3]
    want = lo.run(L.bilstm, lstm, x, gout, DEV)
    got = lo.run(lambda a, m: L.bilstm(a, m, proj='torch'), lstm, x, gout, DEV)
    for n, g, w in zip(lo.NAMES, got, want):
        assert torch.equal(g, w), n
