"""GPU tests of the persistent BiLSTM recurrence (``csrc/lstm_persist.hip``, ``recur='persistent'``).

Sequences are held to ``lstm_oracles`` exactly as the step kernels are in ``test_lstm_gpu.py``:
2.5 x the error of CPU bf16 ``nn.LSTM`` against fp64 ``nn.LSTM`` for ``out``, ``dx`` and the eight
parameter gradients, and ``out`` within 2 bf16 ulps of ``emulate`` on >= 99 % of the elements.
Every case that launches ends with ``persist_check``: a barrier wait that ran out of its budget
is a failure, not a wrong number.

Printed on an MI355X, RATIO (error / torch-bf16 error, bound 2.5) over the six sequence shapes: out
0.84-0.98, dx 0.78-0.83, parameter gradients 0.60-0.92 (0.00 for weight_hh at T = 1, where it is
exactly zero), the same with either ``proj``; EMU: every shape, with and without lengths, 1.0000 of
the elements within 2 bf16 ulps of emulate; dG through the step and the persistent backward: 1.0000
within 2 bf16 ulps.
"""
import copy
from functools import partial

import pytest
import torch

import lstm_oracles as lo
from kernel_oracles import BF16

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')

SEQ_CASES = [((1, 4, 40, 32), 'torch'), ((1, 4, 40, 32), 'native'), ((3, 4, 40, 32), 'torch'),
             ((5, 33, 40, 96), 'torch'), ((25, 4, 40, 32), 'torch'), ((4, 32, 101, 512), 'torch'),
             ((4, 32, 101, 512), 'native'), ((3, 320, 40, 64), 'torch')]


def _L():
    from mercury_amd.ops import lstm as L
    return L


def _check():
    L = _L()
    L.persist_check(L.persist_workspace(DEV))


@pytest.mark.parametrize('shape,proj', SEQ_CASES)
def test_sequence_forward_backward(shape, proj):
    L = _L()
    lstm, x, gout, ref, tb = lo.case(*shape)
    got = lo.run(partial(L.bilstm, recur='persistent', proj=proj), lstm, x, gout, DEV)
    _check()
    what = 'persistent %r proj=%s' % (shape, proj)
    lo.assert_vs_bf16(got, ref, tb, what)
    with torch.no_grad():
        emu = L.emulate(x.to(DEV), copy.deepcopy(lstm).to(DEV))
    lo.assert_close_to_emulate(got[0], emu, what)


def _fwd_bwd(fn, lstm, x, gout, *args):
    m = copy.deepcopy(lstm).to(DEV)
    xs = x.to(DEV).requires_grad_()
    out = fn(xs, m, *args)
    out.backward(gout.to(DEV))
    return [out.detach(), xs.grad] + [p.grad for p in m.parameters()]


@pytest.mark.parametrize('shape,lens', [
    ((6, 5, 40, 32), [6, 1, 0, 3, 8]),
    ((5, 33, 40, 96), [5, 1, 0] + [(7 * i) % 6 for i in range(30)])], ids=['B5', 'B33'])
def test_lengths(shape, lens):
    L = _L()
    T, B, F, H = shape
    lstm = lo.make_lstm(F, H, 3)
    x, gout = lo.make_io(T, B, F, H, 3)
    pad = torch.arange(T)[:, None] >= torch.tensor(lens).clamp(0, T)[None, :]
    x[pad], gout[pad] = NAN, NAN                 # nothing in the padding may reach a result
    per = partial(L.bilstm, recur='persistent')
    dev = _fwd_bwd(per, lstm, x, gout, torch.tensor(lens, device=DEV))
    host = _fwd_bwd(per, lstm, x, gout, lens)    # also cuts the sequence to max(len_b) steps
    _check()
    emu = _fwd_bwd(L.emulate, lstm, x, gout, lens)
    for n, u, v in zip(lo.NAMES, dev, host):
        assert torch.isfinite(u).all(), n
        assert torch.equal(u, v), n
    assert (dev[0][pad] == 0).all() and (dev[1][pad] == 0).all()
    lo.assert_close_to_emulate(dev[0], emu[0], 'persistent lengths %r' % (shape,))


def test_two_runs_and_graph_replays_bit_equal():
    # a replay that did not clear the arrival counters would let every wait through at once
    L = _L()
    lstm, x, gout, _, _ = lo.case(5, 33, 40, 96)
    m = copy.deepcopy(lstm).to(DEV)
    xs, g = x.to(DEV).requires_grad_(), gout.to(DEV)

    def step():
        xs.grad = None
        for p in m.parameters():
            p.grad = None
        out = L.bilstm(xs, m, recur='persistent')
        out.backward(g)
        return [out.detach(), xs.grad] + [p.grad for p in m.parameters()]

    eager = [t.clone() for t in step()]
    for n, u, v in zip(lo.NAMES, eager, step()):
        assert torch.equal(u, v), n
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = step()
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n, u, v in zip(lo.NAMES, cap, eager):
            assert torch.equal(u, v), n
    assert L.persist_status(L.persist_workspace(DEV)) == 0


def test_no_grad_forward_takes_the_inference_form(monkeypatch):
    L = _L()
    seen = []
    real = L.lstm_seq_fwd

    def spy(pre, whh, out, c, gates=None, **kw):
        seen.append((gates is None, tuple(c.shape)))
        return real(pre, whh, out, c, gates, **kw)

    monkeypatch.setattr(L, 'lstm_seq_fwd', spy)
    lstm, x, _, _, _ = lo.case(3, 4, 40, 32)
    m = copy.deepcopy(lstm).to(DEV)
    with torch.no_grad():
        a = L.bilstm(x.to(DEV), m, recur='persistent')
    b = L.bilstm(x.to(DEV), m, recur='persistent')
    _check()
    assert seen == [(True, (1, 2, 4, 32)), (False, (3, 2, 4, 32))]
    assert torch.equal(a, b) and b.grad_fn is not None and a.grad_fn is None


def test_saved_state_feeds_either_backward():
    # out, gates and c as lstm_seq_fwd wrote them, through lstm_step_bwd and lstm_seq_bwd: the two
    # dG differ only in the order of the K = 4H sums.  Seed 0: on the CPU, _steps_bwd_torch with
    # the K sum taken whole and taken as four round-robin chunk shares merged in order (the
    # kernel's split) gave 1.0000 of the dG elements within 2 bf16 ulps at this shape, so the
    # reference alone holds the 99 % cap.
    L = _L()
    T, B, F, H = 5, 33, 40, 96
    lstm, x, gout, _, _ = lo.case(T, B, F, H, 0)
    pk = {k: v.to(DEV) for k, v in L.pack_lstm(lstm).items()}
    pre = (x.view(T * B, F) @ pk['w_ih'].view(8 * H, F).float().cpu().t()).to(DEV) + pk['b'].view(1, -1)
    pre = pre.view(T, B, 2, 4 * H).permute(0, 2, 1, 3).contiguous()
    out = torch.empty(T, B, 2 * H, dtype=BF16, device=DEV)
    gates = torch.empty(T, 2, B, 4 * H, dtype=BF16, device=DEV)
    c = torch.empty(T, 2, B, H, device=DEV)
    ws = L.persist_workspace(DEV)
    L.lstm_seq_fwd(pre, pk['w_hh'], out, c, gates, T=T, B=B, H=H, ws=ws)
    dG = [torch.full_like(gates, NAN) for _ in range(2)]
    dc = [torch.empty(2, B, H, device=DEV) for _ in range(2)]
    L.lstm_step_bwd(gout.to(DEV), gates, c, pk['w_hhT'], dG[0], dc[0], T=T, B=B, H=H)
    L.lstm_seq_bwd(gout.to(DEV), gates, c, pk['w_hhT'], dG[1], dc[1], T=T, B=B, H=H, ws=ws)
    L.persist_check(ws)
    a, b = dG[0].double().cpu(), dG[1].double().cpu()
    frac = float(((a - b).abs() <= 2 * lo.bf16_ulp(a)).double().mean())
    print('dG step vs persistent within-2ulp %.4f' % frac)
    assert torch.isfinite(b).all() and frac >= 0.99


def _refusal(which):
    from mercury_amd.models import MyLSTM
    L = _L()
    if which in ('cell_torch', 'unknown_model'):
        return MyLSTM(40, 12, hidden_dim=32, cell='torch' if which == 'cell_torch' else 'native',
                      recur='persistent' if which == 'cell_torch' else 'resident')
    F, H, B, dev, recur = {'cpu': (40, 32, 4, 'cpu', 'persistent'), 'H48': (40, 48, 4, DEV, 'persistent'),
                           'B513': (8, 32, 513, DEV, 'persistent'), 'H1024': (8, 1024, 4, DEV, 'persistent'),
                           'unknown': (40, 32, 4, DEV, 'resident')}[which]
    lstm = torch.nn.LSTM(F, H, bidirectional=True).to(dev)
    return L.bilstm(torch.zeros(2, B, F, device=dev), lstm, recur=recur)


@pytest.mark.parametrize('which', ['cpu', 'H48', 'B513', 'H1024', 'cell_torch', 'unknown',
                                   'unknown_model'])
def test_refusals(which):
    with pytest.raises(ValueError):
        _refusal(which)


def _model(recur, cell='native'):
    from mercury_amd.models import MyLSTM
    torch.manual_seed(11)
    return MyLSTM(40, 12, hidden_dim=32, dropout=0.0, cell=cell, recur=recur).to(DEV)


def test_auto_recur_follows_the_measured_table(monkeypatch):
    L = _L()
    x = lo.rbf(torch.randn(4, 1, 40, 25, generator=torch.Generator().manual_seed(12))).to(DEV)

    def logits(recur):
        with torch.no_grad():
            return _model(recur).eval()(x)

    assert (4, 32) not in L.MEASURED_PERSISTENT
    assert torch.equal(logits('auto'), logits('step'))
    calls = []
    real = L.lstm_seq_fwd
    monkeypatch.setattr(L, 'lstm_seq_fwd', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(L, 'MEASURED_PERSISTENT', frozenset({(4, 32)}))
    assert torch.equal(logits('auto'), logits('persistent')) and len(calls) == 4
    _check()


def test_trainer_step_with_persistent_recurrence():
    from test_lstm_gpu import _Loader
    from mercury_amd.config import Config
    from mercury_amd.trainer import Trainer
    from mercury_amd.utils import Accuracy, Average, EMAverage
    torch.manual_seed(2)
    net = _model('persistent')
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    t = Trainer(net, opt, _Loader(), _Loader(), None, DEV, Config(print_every=0, eval_every=0))
    before = t.flat.data.clone()
    ema = EMAverage()
    probs, data, label, _, _ = t.update_samples(ema)       # scoring: the no-grad persistent forward
    _, loss = t.train_step(probs, data, label, ema, Average(), Accuracy())
    _check()
    assert torch.isfinite(loss)
    assert torch.isfinite(t.flat.data).all() and not torch.equal(t.flat.data, before)
    w = net.lstm2.weight_hh_l0_reverse
    assert w.grad is not None and float(w.grad.abs().sum()) > 0
