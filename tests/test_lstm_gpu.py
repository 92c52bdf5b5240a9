"""GPU tests of the BiLSTM step kernels (``csrc/lstm.hip``) and of the cell built on them.

Single steps are held to fp64 oracles written here with the elementwise criterion of
``kernel_oracles`` (k = K = 1e-5, ``mag`` = the sum of |terms|):

* forward: with ``pm_x = |pre_x| + sum_k |h_k w_xk|`` the magnitude of gate x's pre-activation,
  ``c_t`` (fp32) uses ``|f c_prev| + |i g| + 2 max(pm_i, pm_f, pm_g)`` -- the activations'
  derivatives are at most 1 (sigmoid: 1/4) and |c_prev| <= 2, so a pre-activation error d moves
  c_t by at most (|c_prev|/4 + 1/4 + 1) d <= 1.75 d < 2 d; ``h_t`` (bf16) adds ``pm_o / 2``
  (|tanh c| sigmoid' <= 1/4, with the same factor-2 slack); each saved gate (bf16) uses its own
  ``pm_x``.
* backward: ``mag_dh = |dout| + sum_k |dG_k w_k|``; ``dc = dc_next + dh o (1 - tanh^2 c)`` uses
  ``mag_dc = |dc_next| + mag_dh |o| (1 - tanh^2 c) + |dh o|`` (the last term carries tanh's own
  error through the cancelling ``1 - tanh^2``); ``dc_prev`` (fp32) and the four ``dG`` (bf16) are
  products of dc (or dh) with exactly representable factors and scale ``mag`` by those factors.

Sequences are held to ``lstm_oracles``: 2.5 x the error of CPU bf16 ``nn.LSTM`` against fp64
``nn.LSTM``, and ``out`` to 2 bf16 ulps of ``emulate`` on the device for >= 99 % of elements.

Printed on an MI355X (largest KNEED over the four shapes, both states / both directions; K is
1e-5): lstm_fwd_c 4.8e-08, lstm_fwd_h 1.0e-09, lstm_fwd_gates 0, lstm_bwd_dG 1.7e-08,
lstm_bwd_dc 1.1e-07.  RATIO (error / torch-bf16 error, bound 2.5) over the five sequence shapes:
out 0.84-0.98, dx 0.79-0.83, parameter gradients 0.60-0.92; the model: logits 0.11, parameter
gradients 0.00-1.00.  EMU: every shape 1.0000 of the elements within 2 bf16 ulps of emulate.
"""
import copy

import pytest
import torch

import lstm_oracles as lo
from kernel_oracles import BF16, F64, K, assert_within, record

pytestmark = pytest.mark.gpu
DEV = 'cuda'

STEP_SHAPES = [(4, 32), (33, 96), (32, 512), (320, 64)]       # (B, H)
SEQ_SHAPES = [(1, 4, 40, 32), (3, 4, 40, 32), (5, 33, 40, 96), (25, 4, 40, 32), (4, 32, 101, 512)]


def _L():
    from mercury_amd.ops import lstm as L
    return L


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _whh(H, g):
    return ((torch.rand(2, 4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(BF16)


# ------------------------------------------------------------------------------ forward step
@pytest.mark.parametrize('given', [False, True], ids=['zero_state', 'given_state'])
@pytest.mark.parametrize('B,H', STEP_SHAPES)
def test_forward_step(B, H, given):
    L = _L()
    g = _gen(B * 1000 + H + given)
    pre = torch.randn(1, 2, B, 4 * H, generator=g)
    whh = _whh(H, g)
    h0 = (torch.rand(2, B, H, generator=g) * 2 - 1).to(BF16) if given else None
    c0 = (torch.rand(2, B, H, generator=g) * 4 - 2) if given else None
    out = torch.full((1, B, 2 * H), float('nan'), dtype=BF16, device=DEV)
    c = torch.full((1, 2, B, H), float('nan'), device=DEV)
    gates = torch.full((1, 2, B, 4 * H), float('nan'), dtype=BF16, device=DEV)
    dv = lambda t: None if t is None else t.to(DEV)
    L.lstm_step_fwd(pre.to(DEV), whh.to(DEV), out, c, gates, dv(h0), dv(c0), T=1, B=B, H=H)
    # the inference form (running state in place, nothing saved) gives the same h and c
    out2 = torch.empty_like(out)
    c2 = torch.empty(2, B, H, device=DEV)
    L.lstm_step_fwd(pre.to(DEV), whh.to(DEV), out2, c2, None, dv(h0), dv(c0), T=1, B=B, H=H)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(c2, c[0])

    w = whh.to(F64)
    h = h0.to(F64) if given else torch.zeros(2, B, H, dtype=F64)
    cp = c0.to(F64) if given else torch.zeros(2, B, H, dtype=F64)
    p = pre[0].to(F64)
    G = p + torch.einsum('dbk,dnk->dbn', h, w)
    pm = p.abs() + torch.einsum('dbk,dnk->dbn', h.abs(), w.abs())
    i, f, gg, o = (torch.sigmoid(G[..., :H]), torch.sigmoid(G[..., H:2 * H]),
                   torch.tanh(G[..., 2 * H:3 * H]), torch.sigmoid(G[..., 3 * H:]))
    pmi, pmf, pmg, pmo = pm[..., :H], pm[..., H:2 * H], pm[..., 2 * H:3 * H], pm[..., 3 * H:]
    ct = f * cp + i * gg
    ht = o * torch.tanh(ct)
    mag_c = (f * cp).abs() + (i * gg).abs() + 2 * torch.maximum(torch.maximum(pmi, pmf), pmg)
    tag = 'B%d_H%d_%s' % (B, H, 'given' if given else 'zero')
    kc = assert_within(c[0].cpu(), ct, mag_c, K, 'c_t ' + tag)
    hk = out[0].cpu().view(B, 2, H).permute(1, 0, 2)
    kh = assert_within(hk, ht, mag_c + 0.5 * pmo, K, 'h_t ' + tag)
    kg = assert_within(gates[0].cpu(), torch.cat([i, f, gg, o], dim=-1), pm, K, 'gates ' + tag)
    record('lstm_fwd_c ' + tag, kc)
    record('lstm_fwd_h ' + tag, kh)
    record('lstm_fwd_gates ' + tag, kg)


# ----------------------------------------------------------------------------- backward step
# T = 3, step 1: both directions sit at t = 1, read dG of one neighbour (t = 2 / t = 0) and c of
# the other; T = 1, step 0: the first backward step (no recurrent term, dc_next zero), which is
# also the last (c_prev is the initial state: zero)
@pytest.mark.parametrize('first', [False, True], ids=['recurrent', 'first_step'])
@pytest.mark.parametrize('B,H', STEP_SHAPES)
def test_backward_step(B, H, first):
    L = _L()
    g = _gen(B * 1000 + H + 17 + first)
    T, s = (1, 0) if first else (3, 1)
    whh = _whh(H, g)
    whhT = whh.transpose(1, 2).contiguous()
    gates = torch.randn(T, 2, B, 4 * H, generator=g)
    gates = torch.cat([torch.sigmoid(gates[..., :2 * H]), torch.tanh(gates[..., 2 * H:3 * H]),
                       torch.sigmoid(gates[..., 3 * H:])], dim=-1).to(BF16)
    c = torch.rand(T, 2, B, H, generator=g) * 4 - 2
    dout = torch.randn(T, B, 2 * H, generator=g)
    dG0 = (torch.randn(T, 2, B, 4 * H, generator=g) * 0.1).to(BF16)
    dc0 = torch.randn(2, B, H, generator=g)
    dG = dG0.to(DEV)
    dc = dc0.to(DEV)
    L.lstm_step_bwd(dout.to(DEV), gates.to(DEV), c.to(DEV), whhT.to(DEV), dG, dc, T=T, B=B, H=H,
                    s0=s, s1=s + 1)
    torch.cuda.synchronize()
    dG, dc = dG.cpu(), dc.cpu()

    w = whh.to(F64)
    t = 0 if first else 1
    for d in (0, 1):
        tn, tc = (t + 1, t - 1) if d == 0 else (t - 1, t + 1)
        dh = dout[t, :, d * H:(d + 1) * H].to(F64)
        mag_dh = dh.abs()
        if first:
            dcn = torch.zeros(B, H, dtype=F64)
            cp = torch.zeros(B, H, dtype=F64)
        else:
            dgn = dG0[tn, d].to(F64)
            dh = dh + dgn @ w[d]
            mag_dh = mag_dh + dgn.abs() @ w[d].abs()
            dcn = dc0[d].to(F64)
            cp = c[tc, d].to(F64)
        i, f, gg, o = gates[t, d].to(F64).split(H, dim=1)
        th = torch.tanh(c[t, d].to(F64))
        dcv = dcn + dh * o * (1 - th * th)
        mag_dc = dcn.abs() + mag_dh * o.abs() * (1 - th * th) + (dh * o).abs()
        ref = torch.cat([dcv * gg * i * (1 - i), dcv * cp * f * (1 - f), dcv * i * (1 - gg * gg),
                         dh * th * o * (1 - o)], dim=1)
        mag = torch.cat([mag_dc * (gg * i * (1 - i)).abs(), mag_dc * (cp * f * (1 - f)).abs(),
                         mag_dc * (i * (1 - gg * gg)).abs(),
                         mag_dh * (th * o * (1 - o)).abs() + (dh * o * (1 - o)).abs()], dim=1)
        tag = 'B%d_H%d_%s_d%d' % (B, H, 'first' if first else 'rec', d)
        record('lstm_bwd_dG ' + tag, assert_within(dG[t, d], ref, mag, K, 'dG ' + tag))
        record('lstm_bwd_dc ' + tag,
               assert_within(dc[d], dcv * f, mag_dc * f.abs(), K, 'dc_prev ' + tag))
    # only step t of dG was written
    keep = [u for u in range(T) if u != t]
    assert torch.equal(dG[keep], dG0[keep])


# --------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize('shape', SEQ_SHAPES)
def test_sequence_forward_backward(shape):
    L = _L()
    lstm, x, gout, ref, tb = lo.case(*shape)
    got = lo.run(L.bilstm, lstm, x, gout, DEV)
    lo.assert_vs_bf16(got, ref, tb, 'native %r' % (shape,))
    with torch.no_grad():
        emu = L.emulate(x.to(DEV), copy.deepcopy(lstm).to(DEV))
    lo.assert_close_to_emulate(got[0], emu, 'native %r' % (shape,))


def test_long_sequence_forward():
    L = _L()
    shape = (161, 8, 101, 128)
    lstm, x, _, ref, tb = lo.case(*shape)
    m = copy.deepcopy(lstm).to(DEV)
    with torch.no_grad():
        out = L.bilstm(x.to(DEV), m)
        emu = L.emulate(x.to(DEV), m)
    lo.assert_vs_bf16([out.double().cpu()], ref[:1], tb[:1], 'native fwd %r' % (shape,), lo.NAMES[:1])
    lo.assert_close_to_emulate(out, emu, 'native fwd %r' % (shape,))


def test_reverse_direction_is_reversed():
    # x is zero except at t = 0: the reverse direction reaches t = 0 last, so its output at T-1
    # is its FIRST step, taken from a zero state on a zero input; the forward half has seen x[0]
    L = _L()
    T, B, F, H = 6, 4, 40, 32
    lstm = lo.make_lstm(F, H, 5).to(DEV)
    x = torch.zeros(T, B, F, device=DEV)
    x[0] = torch.randn(B, F, generator=_gen(9)).to(DEV)
    with torch.no_grad():
        out = L.bilstm(x, lstm)
        one = L.bilstm(torch.zeros(1, B, F, device=DEV), lstm)
    assert torch.equal(out[T - 1, :, H:], one[0, :, H:])
    assert not torch.equal(out[T - 1, :, :H], one[0, :, :H])


def test_no_grad_forward_takes_the_inference_form(monkeypatch):
    # under no_grad (the Trainer's scoring pass) the kernels get no gates buffer and one running c
    L = _L()
    seen = []
    real = L.lstm_step_fwd

    def spy(pre, whh, out, c, gates=None, *a, **kw):
        seen.append((gates is None, tuple(c.shape)))
        return real(pre, whh, out, c, gates, *a, **kw)

    monkeypatch.setattr(L, 'lstm_step_fwd', spy)
    lstm, x, _, _, _ = lo.case(3, 4, 40, 32)
    m = copy.deepcopy(lstm).to(DEV)
    assert all(p.requires_grad for p in m.parameters())
    with torch.no_grad():
        a = L.bilstm(x.to(DEV), m)
    b = L.bilstm(x.to(DEV), m)
    assert seen == [(True, (1, 2, 4, 32)), (False, (3, 2, 4, 32))]
    assert torch.equal(a, b) and b.grad_fn is not None and a.grad_fn is None


# ------------------------------------------------------------------- determinism and capture
def test_two_runs_bit_equal():
    L = _L()
    lstm, x, gout, _, _ = lo.case(5, 33, 40, 96)
    a = lo.run(L.bilstm, lstm, x, gout, DEV)
    b = lo.run(L.bilstm, lstm, x, gout, DEV)
    for n, u, v in zip(lo.NAMES, a, b):
        assert torch.equal(u, v), n


def test_graph_capture_replays_bit_equal():
    L = _L()
    lstm, x, _, _, _ = lo.case(5, 33, 40, 96)
    m = copy.deepcopy(lstm).to(DEV)
    xs = x.to(DEV)
    with torch.no_grad():
        eager = L.bilstm(xs, m).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            L.bilstm(xs, m)                        # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = L.bilstm(xs, m)
        for _ in range(2):
            cap.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap, eager)


# --------------------------------------------------------------------------------- the model
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
    return base, x, gl, [25, 20, 10, 25]


def _model_run(base, cell, x, gl, lengths, dtype, device):
    from mercury_amd.models import MyLSTM
    m = MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell=cell)
    m.load_state_dict(base.state_dict())
    m = m.to(device=device, dtype=dtype).train()
    logits = m(x.to(device=device, dtype=dtype), lengths)
    logits.backward(gl.to(device=device, dtype=dtype))
    names = [n for n, _ in m.named_parameters()]
    return names, [logits.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()]


def test_model_native_vs_torch_cell():
    base, x, gl, lengths = _model_case()
    names, ref = _model_run(base, 'torch', x, gl, lengths, torch.float64, 'cpu')
    _, tb = _model_run(base, 'torch', x, gl, lengths, BF16, 'cpu')
    _, got = _model_run(base, 'native', x, gl, lengths, torch.float32, DEV)
    lo.assert_vs_bf16(got, ref, tb, 'MyLSTM native', ['logits'] + names)


def test_auto_cell_follows_the_measured_table(monkeypatch):
    from mercury_amd.ops import lstm as L
    base, x, _, lengths = _model_case()

    def logits(cell):
        from mercury_amd.models import MyLSTM
        m = MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell=cell)
        m.load_state_dict(base.state_dict())
        with torch.no_grad():
            return m.to(DEV).eval()(x.to(DEV), lengths)

    assert (4, 32) not in L.MEASURED_NATIVE
    assert torch.equal(logits('auto'), logits('torch'))
    monkeypatch.setattr(L, 'MEASURED_NATIVE', frozenset({(4, 32)}))
    assert torch.equal(logits('auto'), logits('native'))
    assert not torch.equal(logits('auto'), logits('torch'))


class _Loader:
    def __init__(self, n=3, b=4):
        g = _gen(21)
        self.batches = [(torch.arange(i * b, (i + 1) * b), torch.randn(b, 1, 40, 25, generator=g),
                         torch.randint(0, 12, (b,), generator=g)) for i in range(n)]
        self.batch_size = b

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def test_trainer_step_with_native_cell():
    from mercury_amd.config import Config
    from mercury_amd.models import MyLSTM
    from mercury_amd.trainer import Trainer
    from mercury_amd.utils import Accuracy, Average, EMAverage
    torch.manual_seed(2)
    net = MyLSTM(40, 12, hidden_dim=32, cell='native').to(DEV)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    t = Trainer(net, opt, _Loader(), _Loader(), None, DEV, Config(print_every=0, eval_every=0))
    before = t.flat.data.clone()
    ema = EMAverage()
    probs, data, label, _, _ = t.update_samples(ema)       # scoring: the no-grad native forward
    _, loss = t.train_step(probs, data, label, ema, Average(), Accuracy())
    assert torch.isfinite(loss)
    assert torch.isfinite(t.flat.data).all() and not torch.equal(t.flat.data, before)
    w = net.lstm2.weight_hh_l0_reverse
    assert w.grad is not None and float(w.grad.abs().sum()) > 0
