"""GPU tests of lengths in the BiLSTM step kernels (``csrc/lstm.hip``) and in what is built on
them: ``ops.lstm.bilstm(x, lstm, lengths)`` and ``MyLSTM(packed=True, cell='native')``.

Step kernels, exact.  Batch rows are independent MFMA columns, so a row of length L must come out
of the kernels with lengths bit-equal to the same row out of the no-lengths kernels run with
``T = L`` on the time-major prefixes (``pre[:L]``, ``dout[:L]``, ...): the forward's ``out[:L]``,
``c[:L]`` and ``gates[:L]`` in the training and the inference form, the backward's ``dG[:L]`` and
``dc``.  One point needs care: ``dc`` is one running buffer per direction and a padded lane stores
``dc = 0``.  Direction 0 ends at t = 0, which is valid for every L >= 1, so its final ``dc`` is
compared as it is.  Direction 1 walks t = 0 .. T-1, so for L < T the value its last valid step
(t = L-1) left is overwritten with zeros by the padded steps after it; the backward is therefore
run in segments that end at every distinct L, ``dc`` of direction 1 is compared right after step
L-1, and the final ``dc`` of those rows is required to be exactly 0.

The layer and the model are held to fp64 packed ``nn.LSTM`` with the bf16 yardstick of
``lstm_oracles`` (factor 2.5) and, for ``out``, to ``emulate`` on the device.
"""
import copy

import pytest
import torch

import lstm_oracles as lo
import lstm_packed_oracles as po
from test_lstm_packed import SHAPES as PACKED_SHAPES

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF16 = torch.bfloat16
NAN = float('nan')


def _L():
    from mercury_amd.ops import lstm as L
    return L


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev_lens(lens):
    return torch.tensor(list(lens), dtype=torch.int32, device=DEV)


# One wave takes 16 rows up to B = 128 and 32 rows (two tiles) above.
# (5, 33, 96): rows 0-15 always valid (7 > T is clamped), rows 16-31 mixed (with 0 and a negative
# value), row 32 alone in the last, partial tile: that wave is all padded from t = 2.
# (4, 130, 32): rows 0-31 always valid, 32-63 mixed, 64-95 all padded from t = 2 (both tiles),
# 96-127 one tile full and one tile of length 1 (the wave must not skip), 128-129 the partial wave.
LENS_33 = [5] * 8 + [7] * 8 + [5, 1, 0, -3, 3, 2, 4, 9, 1, 1, 0, 5, 3, 3, 2, 4] + [2]
LENS_130 = ([4] * 16 + [6] * 16 + [4, 1, 0, -1, 3, 2, 9, 1] * 4 + [2] * 32 + [4] * 16 + [1] * 16
            + [3, 0])
STEP_CASES = [(6, 4, 32, [6, 1, 0, -2]), (5, 33, 96, LENS_33), (4, 130, 32, LENS_130)]
STEP_IDS = ['T%d_B%d_H%d' % c[:3] for c in STEP_CASES]


def _bits_zero(t):
    """Every element is +0 (bit pattern 0), not merely == 0."""
    ints = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return bool((t.contiguous().view(ints) == 0).all())


@pytest.mark.parametrize('T,B,H,lens', STEP_CASES, ids=STEP_IDS)
def test_step_kernels_rowwise_equal_to_the_prefix_runs(T, B, H, lens):
    L = _L()
    assert len(lens) == B
    g = _gen(T * 1000 + B + H)
    eff = torch.tensor(lens).clamp(0, T)                                  # [B]
    pad = po.padded(T, lens)                                              # [T][B]
    pre = torch.randn(T, 2, B, 4 * H, generator=g).to(DEV)
    whh = ((torch.rand(2, 4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(BF16).to(DEV)
    whhT = whh.transpose(1, 2).contiguous()
    dout_f = torch.randn(T, B, 2 * H, generator=g)
    dout = dout_f.clone()
    dout[pad] = NAN
    dout, dout_f = dout.to(DEV), dout_f.to(DEV)
    ld = _dev_lens(lens)

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, NAN, dtype=dtype, device=DEV)

    # ---- forward with lengths: training form and inference form, every output prefilled with NaN
    out, c, gates = nan(T, B, 2 * H, dtype=BF16), nan(T, 2, B, H), nan(T, 2, B, 4 * H, dtype=BF16)
    L.lstm_step_fwd(pre, whh, out, c, gates, T=T, B=B, H=H, lengths=ld)
    out_i, c_i = nan(T, B, 2 * H, dtype=BF16), nan(1, 2, B, H)
    L.lstm_step_fwd(pre, whh, out_i, c_i, None, T=T, B=B, H=H, lengths=ld)
    # ---- backward with lengths, in segments that end at every distinct L (see the docstring)
    dG, dc = nan(T, 2, B, 4 * H, dtype=BF16), nan(2, B, H)
    ends = sorted({int(v) for v in eff if v >= 1} | {T})
    dc1_after, prev = {}, 0
    for e in ends:
        L.lstm_step_bwd(dout, gates, c, whhT, dG, dc, T=T, B=B, H=H, s0=prev, s1=e, lengths=ld)
        dc1_after[e] = dc[1].clone()
        prev = e
    torch.cuda.synchronize()

    assert torch.equal(out_i, out)
    padd = pad.to(DEV)
    assert _bits_zero(out[padd]) and _bits_zero(c.transpose(1, 2)[padd])
    assert _bits_zero(dG.transpose(1, 2)[padd])
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(c).any())
    assert not bool(torch.isnan(dG).any()) and not bool(torch.isnan(dc).any())
    empty = (eff == 0).to(DEV)
    if bool(empty.any()):
        assert _bits_zero(dc[:, empty]) and _bits_zero(c_i[0][:, empty])

    for Lr in sorted({int(v) for v in eff if v >= 1}):
        rows = (eff == Lr).to(DEV)
        ro, rc, rg = nan(Lr, B, 2 * H, dtype=BF16), nan(Lr, 2, B, H), nan(Lr, 2, B, 4 * H, dtype=BF16)
        L.lstm_step_fwd(pre[:Lr], whh, ro, rc, rg, T=Lr, B=B, H=H)
        ro_i, rc_i = nan(Lr, B, 2 * H, dtype=BF16), nan(1, 2, B, H)
        L.lstm_step_fwd(pre[:Lr], whh, ro_i, rc_i, None, T=Lr, B=B, H=H)
        rdG, rdc = nan(Lr, 2, B, 4 * H, dtype=BF16), nan(2, B, H)
        L.lstm_step_bwd(dout_f[:Lr].contiguous(), rg, rc, whhT, rdG, rdc, T=Lr, B=B, H=H)
        torch.cuda.synchronize()
        what = 'rows of length %d' % Lr
        assert torch.equal(out[:Lr, rows], ro[:, rows]), what
        assert torch.equal(out_i[:Lr, rows], ro_i[:, rows]), what
        assert torch.equal(c[:Lr][:, :, rows], rc[:, :, rows]), what
        assert torch.equal(gates[:Lr][:, :, rows], rg[:, :, rows]), what
        assert torch.equal(dG[:Lr][:, :, rows], rdG[:, :, rows]), what
        assert torch.equal(dc[0][rows], rdc[0][rows]), what
        assert torch.equal(dc1_after[Lr][rows], rdc[1][rows]), what
        # the running c of the inference form: direction 1 ends at t = 0 like the prefix run;
        # direction 0 was zeroed by the padded steps after L-1
        assert torch.equal(c_i[0, 1][rows], rc_i[0, 1][rows]), what
        if Lr < T:
            assert _bits_zero(dc[1][rows]) and _bits_zero(c_i[0, 0][rows]), what
        else:
            assert torch.equal(c_i[0, 0][rows], rc_i[0, 0][rows]), what


# ------------------------------------------------------------------------------------- layer
# the waves of LENS_130 with lengths the oracle can pack (1 .. T)
LAYER_LENS_130 = [4] * 32 + [4, 1, 3, 2] * 8 + [2] * 32 + [4] * 16 + [1] * 16 + [3, 1]
LAYER_SHAPES = list(PACKED_SHAPES) + [(9, 40, 40, 64, tuple([9] * 16 + [1] * 8 + [4] * 16)),
                                      (4, 130, 24, 32, tuple(LAYER_LENS_130))]
LAYER_IDS = ['T%d_B%d_F%d_H%d' % s[:4] for s in LAYER_SHAPES]


def _run(lstm, x, gout, lens, fn=None):
    """The ten tensors of ``bilstm(x, lstm, lens)`` on the device, on private copies."""
    L = _L()
    m = copy.deepcopy(lstm).to(DEV)
    x = x.detach().clone().to(DEV).requires_grad_()
    out = (fn or L.bilstm)(x, m, lens)
    out.backward(gout.to(DEV))
    return lo._collect(m, x, out)


def _same(a, b, what=''):
    for n, u, v in zip(lo.NAMES, a, b):
        assert torch.equal(u, v), '%s %s' % (what, n)


@pytest.mark.parametrize('shape', LAYER_SHAPES, ids=LAYER_IDS)
def test_layer_vs_packed_fp64(shape):
    L = _L()
    T, B, F, H, lens = shape
    lstm, x, gout, ref, tb = po.case(*shape)
    lens = list(lens)
    pad = po.padded(T, lens)
    got = _run(lstm, x, gout, lens)
    lo.assert_vs_bf16(got, ref, tb, 'native lengths %r' % (shape[:4],))
    assert bool((got[0][pad] == 0).all()) and bool((got[1][pad] == 0).all())
    with torch.no_grad():
        emu = L.emulate(x.to(DEV), copy.deepcopy(lstm).to(DEV), lens)
    assert bool((emu.cpu()[pad] == 0).all())
    lo.assert_close_to_emulate(got[0], emu, 'native lengths %r' % (shape[:4],))
    # whatever the padding holds, the bits are those of zero padding
    x0, g0 = po.make_io(T, B, F, H, lens, pad_x=0.0, pad_g=0.0)
    want = _run(lstm, x0, g0, lens)
    _same(want, got, 'PAD_X and PAD_G against zero padding')
    _, gn = po.make_io(T, B, F, H, lens, pad_g=NAN)
    xn, _ = po.make_io(T, B, F, H, lens, pad_x=NAN)
    if bool(pad.any()):
        assert bool(torch.isnan(gn).any()) and bool(torch.isnan(xn).any())
    _same(want, _run(lstm, x0, gn, lens), 'NaN gradient')
    _same(want, _run(lstm, xn, g0, lens), 'NaN x')


def test_forms_of_lengths_and_determinism():
    L = _L()
    T, B, F, H = 7, 33, 40, 96
    lens = [min(v, 5) for v in po.seeded_lens(T, B)]            # max 5 < T: host lengths trim
    lens[3] = 0
    lstm = lo.make_lstm(F, H, 0)
    x, gout = po.make_io(T, B, F, H, lens)
    want = _run(lstm, x, gout, lens)
    _same(want, _run(lstm, x, gout, lens), 'second run')
    for form in (torch.tensor(lens), torch.tensor(lens, dtype=torch.int32),
                 torch.tensor(lens, device=DEV), _dev_lens(lens)):
        _same(want, _run(lstm, x, gout, form), '%s on %s' % (form.dtype, form.device))
    full = lo.run(L.bilstm, lstm, x, gout, DEV)
    _same(full, _run(lstm, x, gout, [T] * B), 'None against [T]*B')
    _same(full, _run(lstm, x, gout, _dev_lens([T + 2] * B)), 'None against device [T+2]*B')
    assert not torch.equal(full[0], want[0])
    none = _run(lstm, x, gout, [0] * B)                          # nothing is launched
    for n, v in zip(lo.NAMES, none):
        assert bool((v == 0).all()), n
    _same(none, _run(lstm, x, gout, _dev_lens([0] * B)), 'all empty, device lengths')


def test_host_lengths_trim_the_launches(monkeypatch):
    # a list's maximum is free: the kernels get T = max(len_b); a device tensor costs no sync and
    # runs all T steps.  Under no_grad neither passes a gates buffer.
    L = _L()
    seen = []
    real_f, real_b = L.lstm_step_fwd, L.lstm_step_bwd

    def spy_f(pre, whh, out, c, gates=None, *a, **kw):
        seen.append(('fwd', kw['T'], gates is None, kw.get('lengths') is not None))
        return real_f(pre, whh, out, c, gates, *a, **kw)

    def spy_b(*a, **kw):
        seen.append(('bwd', kw['T'], False, kw.get('lengths') is not None))
        return real_b(*a, **kw)

    monkeypatch.setattr(L, 'lstm_step_fwd', spy_f)
    monkeypatch.setattr(L, 'lstm_step_bwd', spy_b)
    T, B, F, H = 6, 4, 40, 32
    lstm = lo.make_lstm(F, H, 0)
    x, gout = po.make_io(T, B, F, H, [4, 1, 3, 2])
    m = copy.deepcopy(lstm).to(DEV)
    with torch.no_grad():
        a = L.bilstm(x.to(DEV), m, [4, 1, 3, 2])
        b = L.bilstm(x.to(DEV), m, _dev_lens([4, 1, 3, 2]))
        L.bilstm(x.to(DEV), m, [0, 0, 0, 0])
    assert seen == [('fwd', 4, True, True), ('fwd', 6, True, True)]
    assert torch.equal(a, b) and bool((a[4:] == 0).all())
    del seen[:]
    _run(lstm, x, gout, [4, 1, 3, 2])
    assert seen == [('fwd', 4, False, True), ('bwd', 4, False, True)]


# ----------------------------------------------------------------------------- graph capture
def test_graph_capture_with_device_lengths():
    L = _L()
    T, B, F, H = 5, 33, 40, 96
    lstm, x, _, _, _ = lo.case(T, B, F, H)
    m = copy.deepcopy(lstm).to(DEV)
    xs = x.to(DEV)
    first, second = po.seeded_lens(T, B, 1), po.seeded_lens(T, B, 2)
    assert first != second
    ld = _dev_lens(first)
    with torch.no_grad():
        eager = [L.bilstm(xs, m, _dev_lens(v)).clone() for v in (first, second)]
        assert not torch.equal(eager[0], eager[1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            L.bilstm(xs, m, ld)                    # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = L.bilstm(xs, m, ld)
        for want, lens in zip(eager, (first, second)):
            ld.copy_(_dev_lens(lens))
            cap.fill_(NAN)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap, want)


# --------------------------------------------------------------------------------- the model
MODEL_LENS = [25, 1, 10, 25]


def _model_case():
    from mercury_amd.models import MyLSTM
    torch.manual_seed(11)
    base = MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell='torch')
    with torch.no_grad():
        for p in base.parameters():
            p.copy_(lo.rbf(p))
    g = _gen(12)
    x = lo.rbf(torch.randn(4, 1, 40, 25, generator=g))
    gl = lo.rbf(torch.randn(4, 12, generator=g))
    return base, x, gl


def _model_run(base, cell, x, gl, dtype, device):
    from mercury_amd.models import MyLSTM
    m = MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell=cell, packed=True)
    m.load_state_dict(base.state_dict())
    m = m.to(device=device, dtype=dtype).train()
    logits = m(x.to(device=device, dtype=dtype), MODEL_LENS)
    logits.backward(gl.to(device=device, dtype=dtype))
    names = [n for n, _ in m.named_parameters()]
    return names, [logits.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()]


def test_packed_model_native_vs_torch_cell():
    base, x, gl = _model_case()
    names, ref = _model_run(base, 'torch', x, gl, torch.float64, 'cpu')
    _, tb = _model_run(base, 'torch', x, gl, BF16, 'cpu')
    _, got = _model_run(base, 'native', x, gl, torch.float32, DEV)
    lo.assert_vs_bf16(got, ref, tb, 'MyLSTM packed native', ['logits'] + names)
    # 7.0 written into the padding changes no bit of the logits or of any parameter gradient
    x2 = x.clone()
    x2.permute(0, 3, 1, 2)[po.padded(25, MODEL_LENS).t()] = 7.0
    assert not torch.equal(x, x2)
    _, got2 = _model_run(base, 'native', x2, gl, torch.float32, DEV)
    for n, u, v in zip(['logits'] + names, got, got2):
        assert torch.equal(u, v), n


def test_auto_cell_follows_the_packed_table(monkeypatch):
    from mercury_amd.models import MyLSTM
    L = _L()
    base, x, _ = _model_case()

    def logits(cell):
        m = MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell=cell, packed=True)
        m.load_state_dict(base.state_dict())
        with torch.no_grad():
            return m.to(DEV).eval()(x.to(DEV), MODEL_LENS)

    assert (4, 32) not in L.MEASURED_NATIVE_PACKED
    assert torch.equal(logits('auto'), logits('torch'))
    monkeypatch.setattr(L, 'MEASURED_NATIVE_PACKED', frozenset({(4, 32)}))
    assert torch.equal(logits('auto'), logits('native'))
    assert not torch.equal(logits('auto'), logits('torch'))


# --------------------------------------------------------------------------------- refusals
def test_refusals():
    L = _L()
    T, B, H = 3, 4, 32
    pre = torch.zeros(T, 2, B, 4 * H, device=DEV)
    whh = torch.zeros(2, 4 * H, H, dtype=BF16, device=DEV)
    out = torch.zeros(T, B, 2 * H, dtype=BF16, device=DEV)
    c = torch.zeros(1, 2, B, H, device=DEV)
    ok = _dev_lens([3, 1, 2, 0])
    for bad in (torch.tensor([3, 1, 2, 0], dtype=torch.int32), torch.tensor([3, 1, 2, 0], device=DEV),
                _dev_lens([3, 1, 2]), _dev_lens([3, 1, 2, 0, 1])):
        with pytest.raises(ValueError, match='lengths'):
            L.lstm_step_fwd(pre, whh, out, c, T=T, B=B, H=H, lengths=bad)
        with pytest.raises(ValueError, match='lengths'):
            L.lstm_step_bwd(None, None, None, None, None, None, T=T, B=B, H=H, lengths=bad)
    h0 = torch.zeros(2, B, H, dtype=BF16, device=DEV)
    c0 = torch.zeros(2, B, H, device=DEV)
    with pytest.raises(ValueError, match='h0'):
        L.lstm_step_fwd(pre, whh, out, c, None, h0, T=T, B=B, H=H, lengths=ok)
    with pytest.raises(ValueError, match='h0'):
        L.lstm_step_fwd(pre, whh, out, c, None, None, c0, T=T, B=B, H=H, lengths=ok)
    # the launcher refuses it on its own (std::invalid_argument), before any launch
    before = out.clone()
    with pytest.raises(ValueError, match='h0'):
        L.lib().lstm_step_fwd(pre.data_ptr(), whh.data_ptr(), out.data_ptr(), c.data_ptr(), 0,
                              h0.data_ptr(), 0, ok.data_ptr(), T, B, H, 0, T, 0,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    L.lstm_step_fwd(pre, whh, out, c, T=T, B=B, H=H, lengths=ok)       # and takes it without h0
    torch.cuda.synchronize()
