"""Stage counts of the two-stages-in-flight loops (csrc/igemm.hip igemm_nt_body, PF == 2, and
csrc/wgrad_body.h wgrad_body, PF == 2).

Those loops run whole two-stage trips and finish the last one or two stages as straight-line
code behind the loop, so what can go wrong is how many stages run and which register set or LDS
buffer the tail reads.  The cases are therefore chosen by stages per block -- 1, 2, 3, 4, 5 and
9 stages of 64 reduction elements, and K splits that leave 5+4, 3+3+3, 2+2+2+2+1 and 1 each --
at small spatial sizes (the wgrad pixel-stage cases need 64, 128, 192 and 320 pixels and use
8 x 8 images).

Every case runs on random data, against ``F.conv2d`` on bf16-rounded inputs with ``close``
(rtol = atol = 2e-2, as tests/test_kernels_gpu.py), and on integer data drawn from {-2 .. 2},
against an fp64 reference EXACTLY: every product and partial sum is an integer below 2^24, so
fp32 accumulation is exact in any order, split-K and atomics included -- conv outputs must equal
the reference rounded to bf16 and dW the reference itself.  A dropped, doubled or mis-buffered
stage cannot pass that.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def bf(x):
    return x.to(torch.bfloat16).float()


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, 'max err %g (scale %g)' % (err, scale)


# N, H, W, C, K, R, S, stride, pad
CHANNELS = (64, 128, 192, 256, 320)                      # 1 .. 5 stages of a 1x1 reduction
FWD_1X1 = [(2, 5, 7, c, 128, 1, 1, 1, 0) for c in CHANNELS]   # M = 70: a partial second tile
BWD_1X1 = [(2, 5, 7, 64, k, 1, 1, 1, 0) for k in CHANNELS]    # the dgrad reduces over K
CONV3 = (3, 5, 7, 64, 64, 3, 3, 1, 1)                    # 9 stages both ways, M = 105
WG_PIX = [(n, 8, 8, 64, 64, 3, 3, 1, 1) for n in (1, 2, 3, 5)]   # 64 / 128 / 192 / 320 pixels
S2 = [(2, 7, 5, 64, k, r, r, 2, r // 2) for r in (3, 1) for k in (64, 128)]
FWD_TILES = [(64, 64), (64, 128)]
DGRAD_TILES = [(64, 64), (128, 64)]
WGRAD_TILES = [(64, 64), (128, 128)]
SPLITS = [2, 4, 5, 9]      # of 9 stages: 5+4; 3+3+3; 2+2+2+2+1; 1 each
KINDS = ['random', 'integer']


@functools.lru_cache(maxsize=None)
def _data(case, kind):
    """(x, w, gy, y_ref, dx_ref, dw_ref) on the device, computed once and shared (read-only).
    random: fp32 torch conv of the bf16-rounded operands; integer: fp64 on the host, exact."""
    N, H, W, C, K, R, S, st, pd = case
    g = torch.Generator(device='cpu').manual_seed(7)
    P, Q = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
    if kind == 'integer':
        x = torch.randint(-2, 3, (N, C, H, W), generator=g).double()
        w = torch.randint(-2, 3, (K, C, R, S), generator=g).double()
        gy = torch.randint(-2, 3, (N, K, P, Q), generator=g).double()
    else:
        x = bf(torch.randn(N, C, H, W, generator=g)).to(DEV)
        w = bf(torch.randn(K, C, R, S, generator=g) / math.sqrt(C * R * S)).to(DEV)
        gy = bf(torch.randn(N, K, P, Q, generator=g)).to(DEV)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=st, padding=pd)
    y.backward(gy)
    out = (x, w, gy, y.detach(), xr.grad, wr.grad)
    if kind == 'integer':
        assert max(t.abs().max().item() for t in out) < 2 ** 24
        out = tuple(t.float().to(DEV) for t in out)       # integers below 2^24: exact in fp32
    return out


def _nhwc(t):
    """NCHW reference -> the kernels' [pixels][channels] order"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _check_out(out, ref_nchw, kind):
    ref = _nhwc(ref_nchw)
    if kind == 'integer':
        assert torch.equal(out.view(ref.shape), ref.to(torch.bfloat16)), \
            '%d outputs differ from the exact result' % \
            (out.view(ref.shape) != ref.to(torch.bfloat16)).sum().item()
    else:
        close(out.view(ref.shape), ref)


def _check_dw(dw, ref_kcrs, kind):
    ref = ref_kcrs.permute(0, 2, 3, 1).reshape(-1)        # [K][R][S][C]
    if kind == 'integer':
        assert torch.equal(dw, ref), '%d weight gradients differ from the exact result' % \
            (dw != ref).sum().item()
    else:
        close(dw, ref)


def _fwd(ops, case, kind, plan):
    from mercury_amd.ops.conv import ConvSpec, slab_bytes
    x, w = _data(case, kind)[:2]
    spec = ConvSpec(*case)
    out = torch.empty(spec.M, spec.K, dtype=torch.bfloat16, device=DEV)
    slab = torch.zeros(max(1, slab_bytes(spec.M, spec.K, *plan) // 4), device=DEV)
    ops.conv_fwd(ops.to_nhwc(x), ops.pack_conv_weight(w)[0], out, spec, slab=slab, plan=plan)
    return out


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tile', FWD_TILES)
@pytest.mark.parametrize('case', FWD_1X1 + [CONV3])
def test_tail_forward_stage_counts(case, tile, kind):
    """1, 2, 3, 4, 5 and 9 stages in one block (igemm_nt_kernel<64, 64 | 128, false, 2>)"""
    ops = _ops()
    _check_out(_fwd(ops, case, kind, tile + (1,)), _data(case, kind)[3], kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tile', FWD_TILES)
@pytest.mark.parametrize('splits', SPLITS)
def test_tail_forward_split_stage_counts(splits, tile, kind):
    """the 9-stage conv split 2, 4, 5 and 9 ways: blocks of 5 and 4, of 3, of 2 and 1, of 1"""
    ops = _ops()
    _check_out(_fwd(ops, CONV3, kind, tile + (splits,)), _data(CONV3, kind)[3], kind)


def _pair(ops, case, kind, dplan, wplan, wslab=False):
    """dgrad + wgrad of a stride-1 conv through the pair launcher itself (conv_bwd_pair: no
    fallback to separate launches); skips where it has no instantiation for the tiles"""
    from mercury_amd.ops.conv import (ConvSpec, _pair_args, _wslab_ptr, slab_bytes,
                                      wgrad_slab_bytes)
    from mercury_amd.ops import stream_ptr
    x, w, gy = _data(case, kind)[:3]
    spec = ConvSpec(*case)
    Cp, Mx = spec.Cp, spec.N * spec.H * spec.W
    dy, wt, xn = ops.to_nhwc(gy), ops.pack_conv_weight(w)[1], ops.to_nhwc(x)
    dx = torch.empty(Mx, Cp, dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros(spec.K * spec.R * spec.S * spec.C, device=DEV)
    bm, bn, splits = dplan
    slab = torch.zeros(max(1, slab_bytes(Mx, Cp, bm, bn, splits) // 4), device=DEV)
    ws = torch.zeros(max(1, wgrad_slab_bytes(spec, wplan) // 4), device=DEV) if wslab else None
    args = _pair_args(dy, wt, dx, xn, dw, spec, dplan, wplan, slab,
                      wslab=_wslab_ptr(spec, wplan, ws))
    ok = ops.lib().conv_bwd_pair(*args, stream_ptr())
    if not ok:
        assert (bm, bn) != (64, 64), 'the 64 x 64 pair must launch'
        pytest.skip('no pair instantiation for tiles %s / %s' % (dplan, wplan))
    return dx, dw


def _check_pair(dx, dw, case, kind):
    ref = _data(case, kind)
    _check_out(dx, ref[4], kind)
    _check_dw(dw, ref[5], kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tile', DGRAD_TILES)
@pytest.mark.parametrize('case', BWD_1X1 + [CONV3])
def test_tail_pair_dgrad_stage_counts(case, tile, kind):
    """bwd_pair_kernel: 1, 2, 3, 4, 5 and 9 dgrad stages in one block, 64 x 64 and 128 x 64
    dgrad tiles; the 64 x 64 wgrad half runs 2 pixel stages (70 and 105 pixels)"""
    ops = _ops()
    _check_pair(*_pair(ops, case, kind, tile + (1,), (64, 64, 1)), case, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tile', DGRAD_TILES)
@pytest.mark.parametrize('splits', SPLITS)
def test_tail_pair_dgrad_split_stage_counts(splits, tile, kind):
    ops = _ops()
    _check_pair(*_pair(ops, CONV3, kind, tile + (splits,), (64, 64, 1)), CONV3, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('wtile', WGRAD_TILES)
@pytest.mark.parametrize('wsplits', [1, 2, 3])
@pytest.mark.parametrize('case', WG_PIX)
def test_tail_pair_wgrad_pixel_stage_counts(case, wsplits, wtile, kind):
    """wgrad_body<64, 64> and <128, 128>: 1, 2, 3 and 5 pixel stages, unsplit and over 2 and 3
    splits (2 stages over 3 splits: the launcher clamps to one stage each); split sums through
    fp32 atomics and through the slab hand-off"""
    ops = _ops()
    _check_pair(*_pair(ops, case, kind, (64, 64, 1), wtile + (wsplits,)), case, kind)
    if wsplits > 1:
        _check_pair(*_pair(ops, case, kind, (64, 64, 1), wtile + (wsplits,), wslab=True), case,
                    kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', S2)
def test_tail_pair_s2_class_stage_counts(case, kind):
    """bwd_pair_s2_kernel: the parity classes of a 3x3 stride-2 dgrad reduce over 1, 2, 2 and 4
    taps -- 1/2/2/4 stages at K = 64, 2/4/4/8 at K = 128; a 1x1's only class over 1 or 2"""
    from mercury_amd.ops.conv import ConvSpec, _pair_s2_args
    from mercury_amd.ops import stream_ptr
    ops = _ops()
    x, w, gy = _data(case, kind)[:3]
    spec = ConvSpec(*case)
    Cp, Mx = spec.Cp, spec.N * spec.H * spec.W
    dy, wt, xn = ops.to_nhwc(gy), ops.pack_conv_weight(w)[1], ops.to_nhwc(x)
    dx = torch.empty(Mx, Cp, dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros(spec.K * spec.R * spec.S * spec.C, device=DEV)
    args = _pair_s2_args(dy, wt, dx, xn, dw, spec, (64, 64, 1))
    ok = ops.lib().conv_bwd_pair_s2(*args, stream_ptr())
    assert ok, 'the 64 x 64 stride-2 pair must launch'
    _check_pair(dx, dw, case, kind)
