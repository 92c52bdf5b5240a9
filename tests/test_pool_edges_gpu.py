"""Pooling and layout-conversion kernels (csrc/misc.hip) at their window and tie edges, against
the fp64 references of ``kernel_oracles``.

Covered here and nowhere else: the average pool, the runtime-window path (k other than 2 or
3), ties (the first maximum in scan order wins, and the backward routes the gradient to that
tap alone), input rows that no window covers (k = s, H % k != 0: exactly 0), the 9-fold overlap
of k = 3 / s = 1, the fused-BN pool at k = 2 and at a runtime window, and ``nchw_to_nhwc8``.

NaN: the max pool keeps the finite maximum of a window where torch returns NaN (its
comparisons are false for NaN).  That is left as it is and neither asserted nor exercised here.

Largest measured (|err| - 2^-8 |ref|) / mag on an MI355X, against k = 1e-5:
    average pool                                   0
    max pool backward                              0
(0: every error was under the bf16 half-ulp term; the max pool forward, its argmax bytes, the
fused-BN pool and nchw_to_nhwc8 are compared bit for bit.)
"""
import struct

import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KSP, SHAPES = ko.POOL_KSP, ko.POOL_SHAPES


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _data(shape, kind, seed):
    return ko.pool_data(shape, kind, seed, DEV)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('k,s,p', KSP)
def test_avg_pool(k, s, p, shape):
    ops = _ops()
    N, H, W, C = shape
    P, Q = ko.pool_out(H, k, s, p), ko.pool_out(W, k, s, p)
    x = _data(shape, 'random', k * 10 + s)
    y = torch.full((N, P, Q, C), float('nan'), dtype=torch.bfloat16, device=DEV)
    ops.pool2d_fwd(x, y, N, H, W, C, P, Q, k, s, p, is_max=False)
    ref, mag = ko.avgpool_ref(x, k, s, p)
    ko.record('avg_pool', ko.assert_within(y, ref, mag, what='avg pool k%d s%d p%d' % (k, s, p)))


@pytest.mark.parametrize('kind', ['random', 'ties'])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('k,s,p', KSP + [(3, 3, 0)])
def test_max_pool_argmax_and_backward(k, s, p, shape, kind):
    """Forward bit-equal, the argmax bytes equal to the first-maximum taps, the backward within
    the criterion with mag = the sum of |gradients| routed to each input (0 -> exactly 0: at
    (3, 3, 0) and H = 11 rows 9 and 10 are covered by no window)."""
    ops = _ops()
    N, H, W, C = shape
    P, Q = ko.pool_out(H, k, s, p), ko.pool_out(W, k, s, p)
    x = _data(shape, kind, k * 10 + s)
    ref, tap = ko.maxpool_ref(x, k, s, p)
    for with_arg in (False, True):
        y = torch.full((N, P, Q, C), float('nan'), dtype=torch.bfloat16, device=DEV)
        am = torch.full((N * P * Q * C,), 255, dtype=torch.uint8, device=DEV) if with_arg else None
        ops.pool2d_fwd(x, y, N, H, W, C, P, Q, k, s, p, True, am)
        assert torch.equal(y.double(), ref), 'forward (argmax=%s)' % with_arg
    assert torch.equal(am.view(N, P, Q, C), tap), 'argmax taps'
    dy = ko.pool_grad((N, P, Q, C), DEV)
    dx = torch.full((N, H, W, C), float('nan'), dtype=torch.bfloat16, device=DEV)
    ops.maxpool2d_bwd(dy, am, dx, N, H, W, C, P, Q, k, s, p)
    dref, dmag = ko.maxpool_bwd_ref(dy, tap, H, W, k, s, p)
    if (k, s, p) == (3, 3, 0) and H == 11:
        assert (dmag[:, 9:] == 0).all() and (dx[:, 9:] == 0).all()
    ko.record('maxpool_bwd', ko.assert_within(dx, dref, dmag,
                                              what='max pool bwd k%d s%d p%d' % (k, s, p)))


@pytest.mark.parametrize('k,s,p', [(2, 2, 0), (4, 2, 1)])
@pytest.mark.parametrize('act', ['relu', 'relu6'])
def test_fused_bn_pool_bit_equal_to_bn_apply_then_pool(k, s, p, act):
    """Two ghost groups, negative scales (the min branch); k = 4 takes the runtime window."""
    ops = _ops()
    N, H, W, C, G = 4, 10, 6, 24, 2
    P, Q = ko.pool_out(H, k, s, p), ko.pool_out(W, k, s, p)
    M, gr = N * H * W, (N // G) * H * W
    y, gamma, beta = ko.bn_inputs(M, C, gr, seed=k, device=DEV)
    assert (gamma < 0).any()
    stats = ko.bn_sums(y, gr)
    g = ko.gen(9)
    rm = (torch.rand(C, generator=g) * 6 - 3).to(DEV)
    rv = ((torch.rand(C, generator=g) * 1.5 + 0.5) ** 2).to(DEV)
    for bn in (dict(stats=stats, group_imgs=N // G), dict(rmean=rm, rvar=rv)):
        a = torch.empty_like(y)
        if 'stats' in bn:
            ops.bn_apply(y, stats, gamma, beta, a, M, C, group_rows=gr, act=act)
        else:
            ops.bn_apply(y, None, gamma, beta, a, M, C, act=act, running=(rm, rv))
        ref = torch.empty(N, P, Q, C, dtype=torch.bfloat16, device=DEV)
        ops.pool2d_fwd(a, ref, N, H, W, C, P, Q, k, s, p, True)
        out = torch.full_like(ref, float('nan'))
        ops.pool2d_fwd(y, out, N, H, W, C, P, Q, k, s, p, True,
                       bn=dict(bn, gamma=gamma, beta=beta, act=act, eps=1e-5))
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
        # and the two-pass result is itself the reference's: bn_apply_ref then the max
        v, mag = ko.bn_apply_ref(y, stats if 'stats' in bn else None, gamma, beta, gr, act,
                                 running=(rm, rv) if 'rmean' in bn else None)
        ko.assert_within(a, v, mag, what='bn_apply before the pool')


def _f32(bits):
    return struct.unpack('<f', struct.pack('<I', bits))[0]


@pytest.mark.parametrize('C,Cpad', [(1, 8), (3, 8), (4, 8), (10, 16)])
def test_nchw_to_nhwc8_rounds_like_torch(C, Cpad):
    """Bit-equal to permute + .to(bfloat16) (round to nearest even), zero-padded to Cpad."""
    ops = _ops()
    N, H, W = 2, 5, 7
    x = torch.randn(N, C, H, W, generator=ko.gen(C))
    special = [
        _f32(0x3F808000), _f32(0xBF808000),     # halfway, lower neighbour even: rounds down
        _f32(0x3F818000), _f32(0xBF818000),     # halfway, lower neighbour odd: rounds up
        1e-40, -1e-40,                          # fp32 subnormals
        float('inf'), float('-inf'), float('nan'),
        3.4e38, -3.4e38,                        # above bf16's largest finite value
    ]
    flat = x.view(-1)
    pos = torch.randperm(flat.numel(), generator=ko.gen(1))[:len(special)]
    flat[pos] = torch.tensor(special)
    ref = torch.zeros(N, H, W, Cpad, dtype=torch.bfloat16)
    ref[..., :C] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    y = torch.full((N, H, W, Cpad), float('nan'), dtype=torch.bfloat16, device=DEV)
    ops.nchw_to_nhwc8(x.to(DEV), y)
    y = y.cpu()
    nan = torch.isnan(ref)
    assert int(nan.sum()) == 1 and torch.equal(torch.isnan(y), nan)
    bits, rbits = y.view(torch.int16), ref.view(torch.int16)
    assert torch.equal(bits[~nan], rbits[~nan]), (y[~nan][bits[~nan] != rbits[~nan]],
                                                  ref[~nan][bits[~nan] != rbits[~nan]])
