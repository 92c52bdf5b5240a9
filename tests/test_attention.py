"""CPU tests of the attention pooling front-end (``mercury_amd.ops.attention``): the plain-torch
``emulate`` (the hand-written backward formulas) against fp64 autograd of the eager
``Attention.forward`` under the criterion of ``attention_oracles``, the argument checks, and the
module contract of ``Attention(impl=...)`` / ``MyLSTM(attn=...)``."""
import pytest
import torch

import attention_oracles as ao
from kernel_oracles import BF16, K, assert_within

SHAPES = [(1, 1, 64), (5, 3, 192), (40, 4, 64)]          # (T, B, D)


def _A():
    from mercury_amd.ops import attention as A
    return A


def _length_cases(T, B):
    cases = [None, ao.mixed_lengths(T, B), ao.above_lengths(T, B)]
    if B == 1:
        cases.append([0])
    return cases


# ------------------------------------------------------------------ emulate vs fp64 autograd
@pytest.mark.parametrize('as_tensor', [False, True], ids=['list', 'tensor'])
@pytest.mark.parametrize('T,B,D', SHAPES)
def test_emulate_matches_fp64_autograd_of_the_module(T, B, D, as_tensor):
    A = _A()
    x, w, g = ao.inputs(T, B, D, seed=T * 100 + B)
    for lengths in _length_cases(T, B):
        ref = ao.fwd_ref(x, w, lengths)
        assert ao.mask_is_safe(ref), 'pick another seed: a score sits on the relu kink'
        bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
        # the formulas the oracle is written from are the module's own derivative
        rep64, attn64, dx64, dw64 = ao.module_ref(x, w, g, lengths)
        for got, want in ((ref['rep'], rep64), (ref['a'], attn64), (bref['dx'], dx64),
                          (bref['dw'], dw64)):
            assert torch.allclose(got, want, rtol=1e-11, atol=1e-13)

        xe = x.clone().requires_grad_(True)
        we = w.clone().reshape(1, D).requires_grad_(True)        # the module's parameter shape
        arg = lengths if lengths is None or not as_tensor else torch.tensor(lengths)
        rep, attn = A.emulate(xe, we, arg)
        assert rep.dtype == attn.dtype == torch.float32 and not attn.requires_grad
        (rep * g).sum().backward()
        tag = '%r lengths %r' % ((T, B, D), lengths)
        assert_within(rep.detach(), rep64, ref['rep_mag'], K, 'rep ' + tag)
        assert_within(attn, attn64, ref['a_mag'], K, 'attn ' + tag)
        # autograd walks softmax -> mask -> renormalise, whose terms cancel at padded frames
        # only up to fp64 rounding (1e-17 seen where the formulas give 0): the reference's own
        # error is allowed as an absolute 1e-13, the bound it was just held to
        assert_within(xe.grad, dx64, bref['dx_mag'], K, 'dx ' + tag, atol=1e-13)
        assert_within(we.grad.reshape(D), dw64, bref['dw_mag'], K, 'dw ' + tag, atol=1e-13)
        pad = ~ref['valid'].t()
        assert bool((xe.grad[pad] == 0).all()) and bool((attn.t()[pad] == 0).all())


def test_emulate_bf16_input_and_padding_never_read():
    A = _A()
    T, B, D = 5, 3, 192
    x, w, g = ao.inputs(T, B, D, seed=3)
    lengths = ao.mixed_lengths(T, B)
    xb = x.to(BF16).requires_grad_(True)
    rep, attn = A.emulate(xb, w, lengths)
    (rep * g).sum().backward()
    assert xb.grad.dtype == BF16
    with torch.no_grad():
        rep32, attn32 = A.emulate(x, w, lengths)
        for fill in (1e30, float('inf'), float('nan')):
            repf, attnf = A.emulate(ao.pad_fill(x, lengths, fill), w, lengths)
            assert torch.equal(repf, rep32) and torch.equal(attnf, attn32)
    assert torch.equal(rep.detach(), rep32) and torch.equal(attn, attn32)
    ref = ao.fwd_ref(x, w, lengths)
    bref = ao.bwd_ref(x, w, g, ref['a'], ref['s'], lengths)
    assert_within(xb.grad, bref['dx'], bref['dx_mag'], K, 'bf16 dx')


def test_no_grad_form_saves_nothing():
    A = _A()
    x, w, _ = ao.inputs(5, 3, 64, seed=4)
    w = w.requires_grad_(True)
    with torch.no_grad():
        rep0, _ = A.emulate(x, w)
    rep1, _ = A.emulate(x, w)
    assert rep0.grad_fn is None and rep1.grad_fn is not None and torch.equal(rep0, rep1)


def test_split_follows_the_constants():
    A = _A()
    W, BW = A.WAVE_FRAMES, A.BLOCK_WAVES
    assert A.split(1, 1) == (W, 1) and A.split(W + 1, 33) == (W, 1)
    assert A.split(2 * BW * W + 1, 2) == (W, 3)
    assert A.split(161, 32) == (W, -(-161 // (W * BW)))
    share, nsb = A.split(161, 320)                 # B alone nearly fills TARGET_WAVES
    assert share == -(-161 // -(-A.TARGET_WAVES // 320)) and nsb == 2
    share, nsb = A.split(100000, 1)
    assert -(-100000 // share) <= A.MAX_SPLITS and nsb == A.MAX_SPLITS // BW


# ------------------------------------------------------------------------- argument errors
def _bufs(T, B, D):
    return (torch.zeros(B, D), torch.zeros(B, T), torch.zeros(B, T),
            torch.zeros(_A().fwd_ws_floats(T, B, D)))


def test_cpu_input_is_refused():
    A = _A()
    x, w, _ = ao.inputs(5, 3, 64, seed=1)
    with pytest.raises(ValueError, match='x must be a HIP device tensor'):
        A.attn_pool(x, w)
    with pytest.raises(ValueError, match='x must be a HIP device tensor'):
        A.attn_pool_fwd(x, w, None, *_bufs(5, 3, 64))


def test_width_must_be_a_multiple_of_64_within_the_limit():
    A = _A()
    for D in (96, 32, A.MAX_D + 64):
        with pytest.raises(ValueError, match='width %d' % D):
            A.attn_pool(torch.zeros(5, 3, D), torch.zeros(D))
    for D in (64, 192, 1024, 2048):
        A.check_width(D)


def test_layout_errors_name_the_tensor():
    A = _A()
    w = torch.zeros(64)
    strided = torch.zeros(5, 3, 128)[:, :, ::2]
    with pytest.raises(ValueError, match='x: the last dimension must be contiguous'):
        A.attn_pool(strided, w)
    offset = torch.zeros(5 * 3 * 64 + 1)[1:].view(5, 3, 64)
    with pytest.raises(ValueError, match='x: rows must be 16-byte aligned'):
        A.attn_pool(offset, w)
    rows = torch.zeros(5, 3, 66, dtype=BF16)[:, :, :64]       # 132-byte row pitch
    with pytest.raises(ValueError, match='x: rows must be 16-byte aligned'):
        A.attn_pool(rows, w)
    with pytest.raises(TypeError, match='x: expected'):
        A.attn_pool(torch.zeros(5, 3, 64, dtype=torch.float64), w)
    with pytest.raises(ValueError, match='x: expected'):
        A.attn_pool(torch.zeros(5, 64), w)


def test_operand_size_errors():
    A = _A()
    x, w, _ = ao.inputs(5, 3, 64, seed=1)
    with pytest.raises(ValueError, match='w: expected 64 elements'):
        A.emulate(x, torch.zeros(128))
    with pytest.raises(ValueError, match='lengths: expected shape'):
        A.emulate(x, w, [5, 5])
    with pytest.raises(ValueError, match='lengths: expected shape'):
        A.emulate(x, w, torch.tensor([5, 5, 5, 5]))
    with pytest.raises(TypeError, match='lengths: expected integers'):
        A.emulate(x, w, torch.tensor([5.0, 5.0, 5.0]))


def test_bad_switch_values():
    from mercury_amd.models import MyLSTM
    from mercury_amd.models.lstm import Attention
    with pytest.raises(ValueError, match='impl must be'):
        Attention(64, impl='hip')
    with pytest.raises(ValueError, match='attn must be'):
        MyLSTM(20, 5, hidden_dim=32, attn='fast')
    with pytest.raises(ValueError, match='attn must be'):
        MyLSTM(20, 5, hidden_dim=32, attn=None)


# ------------------------------------------------------------------------- module contract
def test_native_attention_refuses_cpu_and_unsupported_width():
    from mercury_amd.models.lstm import Attention
    with pytest.raises(ValueError, match='HIP device'):
        Attention(64, impl='native')(torch.zeros(5, 3, 64))
    with pytest.raises(ValueError, match='width 96'):
        Attention(96, batch_first=True, impl='native')(torch.zeros(3, 5, 96))


def test_auto_attention_stays_on_torch_on_the_cpu():
    from mercury_amd.models.lstm import Attention
    x, w, _ = ao.inputs(5, 3, 64, seed=2)
    outs = []
    for impl in ('torch', 'auto'):
        m = Attention(64, impl=impl)
        with torch.no_grad():
            m.att_weights.copy_(w.reshape(1, 64))
        outs.append(m(x, [5, 2, 0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_state_dict_is_independent_of_impl():
    from mercury_amd.models.lstm import Attention
    ref = {k: tuple(v.shape) for k, v in Attention(64).state_dict().items()}
    assert ref == {'att_weights': (1, 64)}
    for impl in ('torch', 'native', 'auto'):
        m = Attention(64, batch_first=True, impl=impl)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref
        m.load_state_dict(Attention(64).state_dict())


def test_mylstm_default_is_unchanged():
    from mercury_amd.models import MyLSTM

    def build(**kw):
        torch.manual_seed(5)
        return MyLSTM(20, 7, hidden_dim=32, **kw).eval()

    old, new = build(), build(attn='torch')
    assert old.attn == 'torch' and old.atten1.impl == old.atten2.impl == 'torch'
    assert list(old.state_dict()) == list(new.state_dict()) == list(build(attn='native').state_dict())
    x = torch.randn(4, 1, 20, 12, generator=ao.gen(6))
    with torch.no_grad():
        for lengths in (None, [12, 3, 0, 7]):
            assert torch.equal(old(x, lengths), new(x, lengths))
