"""CPU tests of the native BiLSTM cell's front-end (``mercury_amd/ops/lstm.py``): the plain-torch
``emulate`` against fp64 ``nn.LSTM``, the packed operands, and the refusals -- no GPU needed."""
import copy

import pytest
import torch
import torch.nn as nn

import lstm_oracles as lo
from mercury_amd.models import MyLSTM
from mercury_amd.ops import lstm as L

BF16 = torch.bfloat16


@pytest.mark.parametrize('shape', [(3, 4, 40, 32), (5, 33, 40, 96)])
def test_emulate_vs_fp64(shape):
    lstm, x, gout, ref, tb = lo.case(*shape)
    got = lo.run(L.emulate, lstm, x, gout)
    lo.assert_vs_bf16(got, ref, tb, 'emulate %r' % (shape,))


def test_emulate_catches_a_swapped_gate_order():
    # the yardstick has teeth: the same run with the f and g rows of W_hh exchanged is far outside
    lstm, x, gout, ref, tb = lo.case(3, 4, 40, 32)
    bad = lo.make_lstm(40, 32, 0)
    H = 32
    with torch.no_grad():
        w = bad.weight_hh_l0.clone()
        bad.weight_hh_l0[H:2 * H], bad.weight_hh_l0[2 * H:3 * H] = w[2 * H:3 * H], w[H:2 * H]
    got = lo.run(L.emulate, bad, x, gout)
    e_out = float((got[0] - ref[0]).norm()) / float((tb[0] - ref[0]).norm())
    assert e_out > 10 * lo.FACTOR


# every sequence shape of tests/test_lstm_gpu.py: emulate against emulate with the hidden units and
# the input features relabelled (the K sums of both GEMMs taken in another order) stays inside
# the criterion the device output is held to, so that criterion separates a summation order
# from a wrong kernel at these shapes and seeds
@pytest.mark.parametrize('shape', [(1, 4, 40, 32), (3, 4, 40, 32), (5, 33, 40, 96),
                                   (25, 4, 40, 32), (4, 32, 101, 512), (161, 8, 101, 128)])
def test_emulate_criterion_holds_across_summation_orders(shape):
    T, B, F, H = shape
    lstm, x, _, _, _ = lo.case(*shape)
    g = torch.Generator().manual_seed(7)
    pu, pf = torch.randperm(H, generator=g), torch.randperm(F, generator=g)
    rows = torch.cat([pu + k * H for k in range(4)])
    perm = nn.LSTM(F, H, num_layers=1, bidirectional=True)
    with torch.no_grad():
        for sfx in ('', '_reverse'):
            getattr(perm, 'weight_ih_l0' + sfx).copy_(getattr(lstm, 'weight_ih_l0' + sfx)[rows][:, pf])
            getattr(perm, 'weight_hh_l0' + sfx).copy_(getattr(lstm, 'weight_hh_l0' + sfx)[rows][:, pu])
            getattr(perm, 'bias_ih_l0' + sfx).copy_(getattr(lstm, 'bias_ih_l0' + sfx)[rows])
            getattr(perm, 'bias_hh_l0' + sfx).copy_(getattr(lstm, 'bias_hh_l0' + sfx)[rows])
        a = L.emulate(x, lstm)
        b = L.emulate(x[:, :, pf], perm)
    inv = torch.argsort(pu)
    b = torch.cat([b[:, :, :H][:, :, inv], b[:, :, H:][:, :, inv]], dim=2)
    lo.assert_close_to_emulate(b, a, 'order %r' % (shape,))


def test_pack_lstm_round_trip():
    F, H = 40, 32
    lstm = nn.LSTM(F, H, num_layers=1, bidirectional=True)
    keys = {k: v.clone() for k, v in lstm.state_dict().items()}
    pk = L.pack_lstm(lstm)
    assert pk['w_ih'].dtype == pk['w_hh'].dtype == pk['w_hhT'].dtype == BF16
    assert pk['b'].dtype == torch.float32
    assert pk['w_ih'].shape == (2, 4 * H, F) and pk['w_hh'].shape == (2, 4 * H, H)
    assert pk['w_hhT'].shape == (2, H, 4 * H) and pk['b'].shape == (2, 4 * H)
    for d, sfx in enumerate(('', '_reverse')):
        assert torch.equal(pk['w_ih'][d], getattr(lstm, 'weight_ih_l0' + sfx).to(BF16))
        assert torch.equal(pk['w_hh'][d], getattr(lstm, 'weight_hh_l0' + sfx).to(BF16))
        assert torch.equal(pk['w_hhT'][d], pk['w_hh'][d].t())
        assert torch.equal(pk['b'][d], getattr(lstm, 'bias_ih_l0' + sfx) + getattr(lstm, 'bias_hh_l0' + sfx))
    assert pk['w_hhT'].is_contiguous()
    # the module is untouched
    assert all(torch.equal(v, lstm.state_dict()[k]) for k, v in keys.items())
    assert set(keys) == set(lstm.state_dict())


def test_gate_order_is_i_f_g_o():
    # one step from a zero state with hand-set pre-activations: only i and g open -> c = h/o = 1*1
    F, H = 32, 32
    lstm = nn.LSTM(F, H, num_layers=1, bidirectional=True)
    big = 32.0
    with torch.no_grad():
        for p in lstm.parameters():
            p.zero_()
        for sfx in ('', '_reverse'):
            b = getattr(lstm, 'bias_ih_l0' + sfx)
            b[0:H] = big          # i -> 1
            b[H:2 * H] = -big     # f -> 0
            b[2 * H:3 * H] = big  # g -> 1
            b[3 * H:] = 0.0       # o -> 0.5
    x = torch.zeros(1, 2, F)
    out = L.emulate(x, lstm)
    want = 0.5 * torch.tanh(torch.tensor(1.0))
    assert torch.allclose(out, lo.rbf(want).expand_as(out), atol=0, rtol=0)
    assert torch.allclose(lstm(x)[0], out, atol=2.0 ** -8)
    pk = L.pack_lstm(lstm)
    assert torch.equal(pk['b'][0], torch.cat([torch.full((H,), big), torch.full((H,), -big),
                                              torch.full((H,), big), torch.zeros(H)]))


@pytest.mark.parametrize('mode', ['no_grad', 'eval_no_grad', 'frozen', 'grad'])
def test_no_grad_forward_takes_the_non_saving_form(monkeypatch, mode):
    # what the step function is handed: gates None and one running c [1][2][B][H] = nothing saved
    seen = {}
    real = L._steps_fwd_torch

    def spy(pre, whh, out, c, gates, T, B, H):
        seen['gates'], seen['c'] = gates, tuple(c.shape)
        return real(pre, whh, out, c, gates, T, B, H)

    monkeypatch.setattr(L, '_steps_fwd_torch', spy)
    T, B, H = 3, 4, 32
    lstm = lo.make_lstm(40, H, 0)
    assert all(p.requires_grad for p in lstm.parameters())
    x = torch.randn(T, B, 40)
    if mode == 'grad':
        out = L.emulate(x, lstm)
        assert seen['gates'] is not None and seen['c'] == (T, 2, B, H) and out.grad_fn is not None
        return
    if mode == 'frozen':
        lstm.requires_grad_(False)
        out = L.emulate(x, lstm)
    else:
        if mode == 'eval_no_grad':
            lstm.eval()
        with torch.no_grad():
            out = L.emulate(x, lstm)
    assert seen['gates'] is None and seen['c'] == (1, 2, B, H)
    assert out.grad_fn is None


def test_backward_skips_dx_when_x_needs_no_gradient(monkeypatch):
    lstm, x, gout, _, _ = lo.case(3, 4, 40, 32)
    want = lo.run(L.emulate, lstm, x, gout)
    calls = []
    real = L._f32mm
    monkeypatch.setattr(L, '_f32mm', lambda a, b: calls.append((tuple(a.shape), tuple(b.shape))) or real(a, b))
    m = copy.deepcopy(lstm)
    assert not x.requires_grad
    L.emulate(x, m).backward(gout)           # x does not require a gradient
    assert ((12, 128), (128, 40)) not in calls          # dG . W_ih was not formed
    for n, w in zip(lo.NAMES[2:], want[2:]):
        assert torch.equal(getattr(m, n).grad.double(), w), n


def test_emulate_saves_nothing_without_grad():
    lstm = lo.make_lstm(40, 32, 0)
    x = torch.randn(3, 4, 40)
    with torch.no_grad():
        out = L.emulate(x, lstm)
    assert out.grad_fn is None and not out.requires_grad
    lstm.eval()
    out = L.emulate(x.requires_grad_(), lstm)    # eval mode alone does not stop autograd
    assert out.requires_grad


def test_native_cell_refuses_cpu_and_auto_is_torch_on_cpu():
    x = torch.randn(4, 1, 40, 25)
    with pytest.raises(ValueError):
        MyLSTM(40, 12, hidden_dim=32, cell='native')(x)
    with pytest.raises(ValueError):
        MyLSTM(40, 12, hidden_dim=32, cell='sometimes')
    torch.manual_seed(3)
    a = MyLSTM(40, 12, hidden_dim=32, cell='torch').eval()
    torch.manual_seed(3)
    b = MyLSTM(40, 12, hidden_dim=32, cell='auto').eval()
    with torch.no_grad():
        assert torch.equal(a(x, [25, 20, 10, 25]), b(x, [25, 20, 10, 25]))


def test_native_cell_refuses_unsupported_hidden_size():
    with pytest.raises(ValueError, match='multiple of 32'):
        L.bilstm(torch.randn(3, 4, 40), nn.LSTM(40, 40, bidirectional=True))


def test_same_parameter_tree():
    a = MyLSTM(40, 12, hidden_dim=32, cell='torch').state_dict()
    b = MyLSTM(40, 12, hidden_dim=32, cell='native').state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)


def _fwd_args(T, B, H):
    return dict(pre=torch.zeros(T, 2, B, 4 * H), whh=torch.zeros(2, 4 * H, H, dtype=BF16),
                out=torch.zeros(T, B, 2 * H, dtype=BF16), c=torch.zeros(2, B, H))


def test_op_wrapper_refusals():
    T, B = 2, 4
    a = _fwd_args(T, B, 40)
    with pytest.raises(ValueError, match='multiple of 32'):
        L.lstm_step_fwd(a['pre'], a['whh'], a['out'], a['c'], T=T, B=B, H=40)
    a = _fwd_args(T, B, 32)
    with pytest.raises(ValueError, match='HIP device'):       # a CPU tensor never reaches the device
        L.lstm_step_fwd(a['pre'], a['whh'], a['out'], a['c'], T=T, B=B, H=32)
    strided = torch.zeros(T, 2, B, 8 * 32)[..., ::2]
    assert strided.shape == a['pre'].shape
    with pytest.raises(ValueError, match='pre must be contiguous'):
        L.lstm_step_fwd(strided, a['whh'], a['out'], a['c'], T=T, B=B, H=32)
    off = torch.zeros(a['pre'].numel() + 1)[1:].view_as(a['pre'])       # contiguous, 4 bytes off
    assert off.is_contiguous()
    with pytest.raises(ValueError, match='pre must be 16-byte aligned'):
        L.lstm_step_fwd(off, a['whh'], a['out'], a['c'], T=T, B=B, H=32)
    with pytest.raises(ValueError, match='grid dimension'):
        L.lstm_step_fwd(a['pre'], a['whh'], a['out'], a['c'], T=T, B=65535 * 16 + 1, H=32)
    with pytest.raises(ValueError, match='steps'):
        L.lstm_step_fwd(a['pre'], a['whh'], a['out'], a['c'], T=T, B=B, H=32, s0=1, s1=3)
    with pytest.raises(ValueError, match='multiple of 32'):
        L.lstm_step_bwd(None, None, None, None, None, None, T=T, B=B, H=48)
    with pytest.raises(ValueError, match='HIP device'):
        L.lstm_step_bwd(torch.zeros(T, B, 64), torch.zeros(T, 2, B, 128, dtype=BF16),
                        torch.zeros(T, 2, B, 32), torch.zeros(2, 32, 128, dtype=BF16),
                        torch.zeros(T, 2, B, 128, dtype=BF16), torch.zeros(2, B, 32), T=T, B=B, H=32)
