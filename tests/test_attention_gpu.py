"""GPU tests of the attention pooling kernels (``csrc/attn.hip``) and of the modules on them.

The kernels are held to the fp64 oracles of ``attention_oracles`` with the elementwise criterion
of ``kernel_oracles`` (k = K = 1e-5; the magnitudes are derived in that module's docstring).  The
op-level backward is fed the oracle's own ``a``, ``s`` and ``rep`` (cast to fp32) as the saved
tensors, so its relu mask is the oracle's by construction; the module-level tests assert as a
condition that no valid score of their inputs lies within 2 K ms of the relu kink.

T is chosen from the kernels' split constants (W = WAVE_FRAMES = 8 frames per wave at these batch
sizes, BLOCK_WAVES = 4 waves per block): 1, W - 1, W + 1 (a second wave with one frame),
2 * 4 * W + 7 = 71 (three blocks per row, the last with one full and one 7-frame wave) and 161
(six blocks), so the wave merge in LDS and the cross-block merge both run.

Printed on an MI355X (largest KNEED over all cases of a kind; K is 1e-5): attn_fwd_score
1.53e-08, attn_fwd_attn 1.66e-08, attn_fwd_rep 2.3e-08, attn_bwd_dx 1.29e-07, attn_bwd_dw
3.98e-09; large scores: attn_range_attn 3.11e-10, attn_range_rep 3.94e-10, attn_range_dx
6.06e-09, attn_range_dw 1.45e-09; through autograd: attn_module_rep 1.63e-08, attn_module_attn
1.62e-08, attn_module_dx 2.97e-07, attn_module_dw 1.29e-09; bf16 input: attn_bf16_autograd_rep
2.73e-09, attn_bf16_autograd_dx 9.23e-10, attn_bf16_autograd_dw 1.54e-09.
"""
import pytest
import torch

import attention_oracles as ao
from kernel_oracles import BF16, F64, K, assert_within, record

pytestmark = pytest.mark.gpu
DEV = 'cuda'

W, BW = 8, 4
SHAPES = [(1, 1, 64), (W - 1, 33, 192), (W + 1, 2, 64), (161, 4, 1024), (2 * BW * W + 7, 2, 2048)]
DTYPES = [torch.float32, BF16]
ORDERS = ['tbd', 'btd']          # memory order of the time-major [T][B][D] the op is given


def _A():
    from mercury_amd.ops import attention as A
    return A


def _place(x, order, dtype):
    """x [T][B][D] on the device in ``dtype``: dense time-major, or the transposed view of a
    dense batch-major tensor."""
    x = x.to(device=DEV, dtype=dtype)
    if order == 'tbd':
        return x.contiguous()
    return x.transpose(0, 1).contiguous().transpose(0, 1)


def _dev_lengths(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)


def _fwd(A, x, w, lengths, train=True):
    T, B, D = x.shape
    rep = torch.full((B, D), float('nan'), device=DEV)
    attn = torch.full((B, T), float('nan'), device=DEV)
    score = torch.full((B, T), float('nan'), device=DEV) if train else None
    ws = torch.full((A.fwd_ws_floats(T, B, D),), float('nan'), device=DEV)
    A.attn_pool_fwd(x, w, lengths, rep, attn, score, ws)
    return rep, attn, score


def _bwd(A, x, w, g, rep, attn, score, lengths):
    T, B, D = x.shape
    dx = torch.full_like(x, float('nan'))             # keeps x's strides
    assert dx.stride() == x.stride()
    dw = torch.full((D,), float('nan'), device=DEV)
    ws = torch.full((A.bwd_ws_floats(T, B, D),), float('nan'), device=DEV)
    A.attn_pool_bwd(x, w, g, rep, attn, score, lengths, dx, dw, ws)
    return dx, dw


def _length_cases(T, B):
    return [('none', None), ('mixed', ao.mixed_lengths(T, B)), ('above', ao.above_lengths(T, B))]


def test_split_constants_match_the_launcher():
    from mercury_amd.ops import lib
    A = _A()
    assert (A.WAVE_FRAMES, A.BLOCK_WAVES) == (W, BW)
    for T, B in [(T, B) for T, B, _ in SHAPES] + [(161, 32), (161, 320), (100000, 1), (5, 5000)]:
        assert tuple(lib().attn_pool_split(T, B)) == A.split(T, B), (T, B)
    assert A.split(W + 1, 2) == (W, 1) and A.split(2 * BW * W + 7, 2) == (W, 3)
    assert A.split(161, 4) == (W, 6)


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('T,B,D', SHAPES)
def test_forward(T, B, D, dtype, order):
    A = _A()
    x, w, _ = ao.inputs(T, B, D, seed=T + B + D)
    wd = w.to(DEV)
    for name, lengths in _length_cases(T, B):
        ref = ao.fwd_ref(x, w, lengths)
        ld = _dev_lengths(lengths)
        # padded frames hold 1e30 for the kernel; the same input with zeros there gives the same bits
        xd = _place(ao.pad_fill(x, lengths, 1e30), order, dtype)
        rep, attn, score = _fwd(A, xd, wd, ld)
        rep0, attn0, _ = _fwd(A, _place(ao.pad_fill(x, lengths, 0.0), order, dtype), wd, ld)
        rep2, attn2, score2 = _fwd(A, xd, wd, ld)                    # a second run
        repn, attnn, _ = _fwd(A, xd, wd, ld, train=False)            # the no-grad form
        torch.cuda.synchronize()
        for a, b in ((rep0, rep), (attn0, attn), (rep2, rep), (attn2, attn), (score2, score),
                     (repn, rep), (attnn, attn)):
            assert torch.equal(a, b)
        tag = '%s %s %s %s' % ((T, B, D), str(dtype)[6:], order, name)
        v = ref['valid']
        zero = torch.zeros_like(ref['s'])
        ks = assert_within(score.cpu(), torch.where(v, ref['s'], zero), ref['ms'], K, 'score ' + tag)
        ka = assert_within(attn.cpu(), ref['a'], ref['a_mag'], K, 'attn ' + tag)
        kr = assert_within(rep.cpu(), ref['rep'], ref['rep_mag'], K, 'rep ' + tag)
        record('attn_fwd_score ' + tag, ks)
        record('attn_fwd_attn ' + tag, ka)
        record('attn_fwd_rep ' + tag, kr)


# ------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('T,B,D', SHAPES)
def test_backward(T, B, D, dtype, order):
    A = _A()
    x, w, g = ao.inputs(T, B, D, seed=T + B + D + 1)
    wd, gd = w.to(DEV), g.to(DEV)
    for name, lengths in _length_cases(T, B):
        ref = ao.fwd_ref(x, w, lengths)
        bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
        saved = [ref[k].float().to(DEV) for k in ('rep', 'a', 's')]
        ld = _dev_lengths(lengths)
        xd = _place(ao.pad_fill(x, lengths, 1e30), order, dtype)
        dx, dw = _bwd(A, xd, wd, gd, *saved, ld)
        dx2, dw2 = _bwd(A, xd, wd, gd, *saved, ld)
        torch.cuda.synchronize()
        assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
        assert dx.dtype == dtype
        pad = (~ref['valid']).t().to(DEV)
        assert bool((dx[pad] == 0).all())            # written, and exactly 0
        tag = '%s %s %s %s' % ((T, B, D), str(dtype)[6:], order, name)
        record('attn_bwd_dx ' + tag,
               assert_within(dx.cpu(), bref['dx'], bref['dx_mag'], K, 'dx ' + tag))
        record('attn_bwd_dw ' + tag,
               assert_within(dw.cpu(), bref['dw'], bref['dw_mag'], K, 'dw ' + tag))


# ------------------------------------------------------------------------ range and masks
def test_large_scores_do_not_overflow():
    # every score is above 100: exp(s) without the max subtracted is inf in fp32
    A = _A()
    T, B, D = 20, 3, 64
    gg = ao.gen(7)
    w = ao.rbf((torch.rand(D, generator=gg) + 0.5) * (torch.randint(0, 2, (D,), generator=gg) * 2 - 1))
    x = ao.rbf(3 * torch.sign(w)[None, None] + 0.05 * torch.randn(T, B, D, generator=gg))
    g = ao.rbf(torch.randn(B, D, generator=gg))
    lengths = [20, 13, 1]
    ref = ao.fwd_ref(x, w, lengths)
    assert float(ref['s'][ref['valid']].min()) > 100
    assert float(ref['a'][0].max() / ref['a'][0].min()) > 2          # not a uniform softmax
    ld = _dev_lengths(lengths)
    rep, attn, score = _fwd(A, x.to(DEV), w.to(DEV), ld)
    assert bool(torch.isfinite(rep).all())
    record('attn_range_attn', assert_within(attn.cpu(), ref['a'], ref['a_mag'], K, 'range attn'))
    record('attn_range_rep', assert_within(rep.cpu(), ref['rep'], ref['rep_mag'], K, 'range rep'))
    bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
    dx, dw = _bwd(A, x.to(DEV), w.to(DEV), g.to(DEV), rep, attn, score, ld)
    record('attn_range_dx', assert_within(dx.cpu(), bref['dx'], bref['dx_mag'], K, 'range dx'))
    record('attn_range_dw', assert_within(dw.cpu(), bref['dw'], bref['dw_mag'], K, 'range dw'))


def test_all_scores_negative_gives_uniform_attention_and_zero_ds():
    A = _A()
    T, B, D = 19, 3, 192
    x, w, g = ao.inputs(T, B, D, seed=8)
    x = -x.abs() * torch.sign(w)[None, None] - ao.rbf(0.25 * torch.sign(w))[None, None]
    lengths = [19, 4, 0]
    ref = ao.fwd_ref(x, w, lengths)
    assert float(ref['s'].max()) <= 0 and float(ref['s'][ref['valid']].max()) < 0
    ld = _dev_lengths(lengths)
    rep, attn, score = _fwd(A, x.to(DEV), w.to(DEV), ld)
    want = torch.zeros(B, T)
    want[0, :19], want[1, :4] = 1.0 / 19, 1.0 / 4
    assert_within(attn.cpu(), want.double(), want.double(), K, 'uniform attn')
    assert bool((score.cpu()[ref['valid']] < 0).all())
    dx, dw = _bwd(A, x.to(DEV), w.to(DEV), g.to(DEV), rep, attn, score, ld)
    assert bool((dw == 0).all())                                     # ds is exactly 0
    assert torch.equal(dx.cpu(), attn.cpu().t()[:, :, None] * g[None])


# ------------------------------------------------------------------------ through autograd
LAYOUTS = ['time_major', 'transposed_view', 'batch_first']


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('T,B,D', [(W + 1, 33, 192), (161, 4, 1024)])
def test_module_native_vs_fp64_autograd(T, B, D, layout):
    from mercury_amd.models.lstm import Attention
    x, w, g = ao.inputs(T, B, D, seed=T + D + 2)
    for name, lengths in (('none', None), ('mixed', ao.mixed_lengths(T, B))):
        ref = ao.fwd_ref(x, w, lengths)
        assert ao.mask_is_safe(ref), 'pick another seed: a score sits on the relu kink'
        bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
        rep64, attn64, dx64, dw64 = ao.module_ref(x, w, g, lengths)
        m = Attention(D, batch_first=layout != 'time_major', impl='native').to(DEV)
        with torch.no_grad():
            m.att_weights.copy_(w.reshape(1, D))
        if layout == 'time_major':
            leaf = x.to(DEV).requires_grad_(True)                        # [T][B][D]
            inp = leaf
        elif layout == 'transposed_view':                                # what MyLSTM passes
            leaf = x.to(DEV).requires_grad_(True)
            inp = leaf.transpose(0, 1)
        else:
            leaf = x.transpose(0, 1).contiguous().to(DEV).requires_grad_(True)   # [B][T][D]
            inp = leaf
        rep, attn = m(inp, lengths)
        assert not attn.requires_grad and rep.shape == (B, D) and attn.shape == (B, T)
        (rep * g.to(DEV)).sum().backward()
        dx = leaf.grad if layout != 'batch_first' else leaf.grad.transpose(0, 1)
        tag = '%s %s %s' % ((T, B, D), layout, name)
        record('attn_module_rep ' + tag,
               assert_within(rep.detach().cpu(), rep64, ref['rep_mag'], K, 'rep ' + tag))
        record('attn_module_attn ' + tag,
               assert_within(attn.cpu(), attn64, ref['a_mag'], K, 'attn ' + tag))
        # atol: the reference's own cancellation residue at padded frames (test_attention.py)
        record('attn_module_dx ' + tag,
               assert_within(dx.cpu(), dx64, bref['dx_mag'], K, 'dx ' + tag, atol=1e-13))
        record('attn_module_dw ' + tag,
               assert_within(m.att_weights.grad.cpu().reshape(D), dw64, bref['dw_mag'], K,
                             'dw ' + tag, atol=1e-13))


def test_bf16_input_through_autograd():
    A = _A()
    T, B, D = 2 * BW * W + 7, 2, 2048
    x, w, g = ao.inputs(T, B, D, seed=9)
    lengths = ao.mixed_lengths(T, B)
    xb = x.to(device=DEV, dtype=BF16).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    rep, attn = A.attn_pool(xb, wd, lengths)
    (rep * g.to(DEV)).sum().backward()
    with torch.no_grad():                                               # a CPU tensor of lengths
        rep2, attn2 = A.attn_pool(xb, wd, torch.tensor(lengths))
    assert xb.grad.dtype == BF16 and torch.equal(rep, rep2) and torch.equal(attn, attn2)
    ref = ao.fwd_ref(x, w, lengths)
    bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
    assert ao.mask_is_safe(ref)
    record('attn_bf16_autograd_rep',
           assert_within(rep.detach().cpu(), ref['rep'], ref['rep_mag'], K, 'bf16 autograd rep'))
    record('attn_bf16_autograd_dw',
           assert_within(wd.grad.cpu(), bref['dw'], bref['dw_mag'], K, 'bf16 autograd dw'))
    record('attn_bf16_autograd_dx',
           assert_within(xb.grad.cpu(), bref['dx'], bref['dx_mag'], K, 'bf16 autograd dx'))


def test_graph_capture_replays_bit_equal():
    A = _A()
    x, w, _ = ao.inputs(161, 4, 1024, seed=10)
    xd, wd = x.to(DEV), w.to(DEV)
    ld = _dev_lengths(ao.mixed_lengths(161, 4))
    with torch.no_grad():
        eager = [t.clone() for t in A.attn_pool(xd, wd, ld)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            A.attn_pool(xd, wd, ld)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = A.attn_pool(xd, wd, ld)
        for _ in range(2):
            for t in cap:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1])


def test_auto_follows_the_measured_table(monkeypatch):
    from mercury_amd.models.lstm import Attention
    A = _A()
    x, w, _ = ao.inputs(W + 1, 2, 64, seed=11)
    key = (2, W + 1, 64, torch.float32)
    assert key not in A.MEASURED_NATIVE
    auto, eager, native = (Attention(64, impl=i).to(DEV) for i in ('auto', 'torch', 'native'))
    calls = []
    real = A.attn_pool
    monkeypatch.setattr(A, 'attn_pool', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    with torch.no_grad():
        for m in (auto, eager, native):
            m.att_weights.copy_(w.reshape(1, 64))
        xd = x.to(DEV)
        assert torch.equal(auto(xd)[0], eager(xd)[0]) and not calls
        monkeypatch.setattr(A, 'MEASURED_NATIVE', frozenset({key}))
        assert torch.equal(auto(xd)[0], native(xd)[0]) and len(calls) == 2

# --------------------------------------------------------------------------------- the model
def _model(cell):
    from mercury_amd.models import MyLSTM
    torch.manual_seed(13)
    m = MyLSTM(20, 6, hidden_dim=32, dropout=0.0, cell=cell, attn='native').to(DEV).eval()
    # the RNN library differentiates only a forward run in training mode; a one-layer nn.LSTM
    # computes the same in both, and dropout / batch norm stay in eval mode
    m.lstm1.train()
    m.lstm2.train()
    return m


def test_model_with_native_attention():
    A = _A()
    m = _model('torch')
    outs = {}
    hooks = [getattr(m, n).register_forward_hook(lambda mod, i, o, n=n: outs.__setitem__(n, o[0]))
             for n in ('lstm1', 'lstm2')]
    x = torch.randn(5, 1, 20, 12, generator=ao.gen(14)).to(DEV)
    lengths = [12, 7, 1, 12, 3]
    logits = m(x, lengths)
    for h in hooks:
        h.remove()
    with torch.no_grad():
        a = A.attn_pool(outs['lstm1'], m.atten1.att_weights, lengths)[0]
        b = A.attn_pool(outs['lstm2'], m.atten2.att_weights, lengths)[0]
        hand = m.fc2(m.fc1(torch.cat([a, b], dim=1)))
    assert torch.equal(logits, hand)
    logits.backward(torch.randn(5, 6, generator=ao.gen(15)).to(DEV))
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for att in (m.atten1, m.atten2):
        assert float(att.att_weights.grad.abs().sum()) > 0


def test_model_native_cell_and_native_attention_compose():
    m = _model('native')
    x = torch.randn(5, 1, 20, 12, generator=ao.gen(14)).to(DEV)
    logits = m(x, [12, 7, 1, 12, 3])
    assert bool(torch.isfinite(logits).all())
    logits.backward(torch.randn(5, 6, generator=ao.gen(15)).to(DEV))
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
