"""Epilogue of the dgrad kernels (csrc/conv_epi.h epi_rows, reached through igemm_nt_body):
the row loop runs on operands requested ahead of their use -- the old dx of an accumulating
dgrad, the BN-backward operands and the BN statistics -- and reduces the three BN-backward sums
across lanes with DPP / permlane swaps.

What can go wrong is which rows and chunk columns a prefetched register belongs to, rows >= M or
columns >= N contributing, a K-split block that did not win the tile's ticket touching dx or
the sums, and the lane a packed partial sum ends up in.  The cases are the smallest that reach
each: two full 64-row tiles, a last tile with 11 valid rows, 40 and 72 channels (a chunk column
past N in the last N tile), accumulate / shortcut BN / the three activations, 1-3 K splits of a
9-stage conv, the stride-2 parity classes and the shortcut pair, a 128 x 64 pair tile and the
128 x 128 dgrad tile (16 chunks per row: the reduction without the DPP step).

Checks: dx against torch (``close`` of tests/test_igemm_stage_tail_gpu.py: rtol = atol = 2e-2)
and, on integer data, exactly; the sums against the standalone bn_bwd reduce kernel run on the
same dx within 4 * M * 2^-24 * sum|term| per channel (the worst case of reordering an fp32 sum
of M terms), and exactly on integer data with mean 0 and rstd 2.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ACTS = {'none': 0, 'relu': 1, 'relu6': 2}


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


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@functools.lru_cache(maxsize=None)
def _data(case, kind):
    """Conv operands, the exact dx, and the BN-backward operands of dx's shape; computed once
    per (case, kind) and shared read-only.  integer: everything is a small integer, the
    statistics are zero sums with eps = 1/4 (mean 0, rstd 2), so every term and every partial
    sum is an integer below 2^24 -- exact in fp32 in any order."""
    N, H, W, C, K, R, S, st, pd = case
    g = torch.Generator(device='cpu').manual_seed(11)
    P, Q = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
    Mx = N * H * W
    if kind == 'integer':
        x = torch.randint(-2, 3, (N, C, H, W), generator=g).double()
        w = torch.randint(-2, 3, (K, C, R, S), generator=g).double()
        gy = torch.randint(-2, 3, (N, K, P, Q), generator=g).double()
        old = torch.randint(-2, 3, (Mx, C), generator=g).float()
        levels = torch.tensor([-1., 0., 1., 3., 6., 7.])     # on, at and past both relu6 bounds
        out = levels[torch.randint(0, 6, (Mx, C), generator=g)]
        y = torch.randint(-2, 3, (Mx, C), generator=g).float()
        y2 = torch.randint(-2, 3, (Mx, C), generator=g).float()
        stats = torch.zeros(2, C)
        stats2 = torch.zeros(2, C)
        eps = 0.25
    else:
        x = bf(torch.randn(N, C, H, W, generator=g))
        w = bf(torch.randn(K, C, R, S, generator=g) / math.sqrt(C * R * S))
        gy = bf(torch.randn(N, K, P, Q, generator=g))
        old = bf(torch.randn(Mx, C, generator=g))
        out = bf(torch.randn(Mx, C, generator=g) * 3 + 1.5)
        y = bf(torch.randn(Mx, C, generator=g) + 0.5)
        y2 = bf(torch.randn(Mx, C, generator=g) * 2 - 0.25)
        stats = torch.stack([y.sum(0), (y * y).sum(0)])
        stats2 = torch.stack([y2.sum(0), (y2 * y2).sum(0)])
        eps = 1e-5
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, stride=st, padding=pd).backward(gy)
    dx = _nhwc(xr.grad)
    dw = wr.grad.permute(0, 2, 3, 1).reshape(-1)             # [K][R][S][C]
    if kind == 'integer':
        assert dx.abs().max().item() < 2 ** 24
    d = dict(x=x.float(), w=w.float(), gy=gy.float(), dx=dx.float(), dw=dw.float(), old=old,
             out=out, y=y, y2=y2, stats=stats, stats2=stats2)
    d = {k: v.to(DEV) for k, v in d.items()}
    d['eps'] = eps
    return d


def _bw(d, C, Mx, two, act):
    from mercury_amd.ops import bn as bnops
    b16 = lambda t: t.to(torch.bfloat16).contiguous()
    bw = dict(out=b16(d['out']), y=b16(d['y']), stats=d['stats'].contiguous(),
              sums=torch.zeros(bnops.sums_numel(C), device=DEV), act=act, eps=d['eps'])
    if two:
        bw['y2'] = b16(d['y2'])
        bw['stats2'] = d['stats2'].contiguous()
    return bw


def _expect_dx(d, acc, kind):
    r = d['dx'].to(torch.bfloat16)
    if acc:     # the kernel rounds the conv result to bf16, adds the old bf16 dx, rounds again
        r = (r.float() + d['old']).to(torch.bfloat16)
    return r


def _check(ops, d, dx, bw, case, kind, acc, two, act):
    """dx against the reference; the fused sums against the standalone reduce of the SAME dx"""
    from mercury_amd.ops import bn as bnops, ptr, stream_ptr
    N, H, W, C = case[:4]
    Mx = N * H * W
    ref = _expect_dx(d, acc, kind)
    if kind == 'integer':
        assert torch.equal(dx.view(ref.shape), ref), '%d of %d dx values differ' % (
            (dx.view(ref.shape) != ref).sum().item(), ref.numel())
    else:
        close(dx.view(ref.shape), ref)
    if bw is None:
        return
    fused = bnops.sums_total(bw['sums'], C)
    ws = torch.zeros(bnops.sums_numel(C), device=DEV)
    ops.lib().bn_bwd(ptr(dx), ptr(bw['out']), ptr(bw['y']), ptr(bw['stats']), 0, ptr(bw.get('y2')),
                     ptr(bw.get('stats2')), 0, ptr(ws), 0, 0, 0, 0, 0, 0, 0, Mx, C, ACTS[act],
                     d['eps'], stream_ptr(), 1)
    alone = bnops.sums_total(ws, C)
    # sum |term| per channel, fp64, from the dx the kernel produced
    g = dx.view(Mx, C).double()
    o = bw['out'].double()
    hi = 6 if act == 'relu6' else math.inf
    mask = torch.ones_like(o) if act == 'none' else ((o > 0) & (o < hi)).double()
    dz = g * mask

    def xhat(y, st):
        mean = st[0].double() / Mx
        var = (st[1].double() / Mx - mean * mean).clamp_min(0)
        return (y.double() - mean) / torch.sqrt(var + d['eps'])
    terms = [dz, dz * xhat(bw['y'], bw['stats'])]
    if two:
        terms.append(dz * xhat(bw['y2'], bw['stats2']))
    for i, t in enumerate(terms):
        if kind == 'integer':
            assert torch.equal(fused[i], alone[i]), 'sum %d: %d channels differ (max %g)' % (
                i, (fused[i] != alone[i]).sum().item(), (fused[i] - alone[i]).abs().max().item())
            assert torch.equal(fused[i].double(), t.sum(0)), 'sum %d differs from the exact sum' % i
        else:
            bound = 4 * Mx * 2.0 ** -24 * t.abs().sum(0)
            err = (fused[i].double() - alone[i].double()).abs()
            assert bool((err <= bound).all()), 'sum %d: err %g over bound %g' % (
                i, err.max().item(), bound[err.argmax()].item())
    if not two:
        assert not fused[2].any(), 'the shortcut sum was written without a shortcut BN'


def _tensors(ops, d, case, acc):
    from mercury_amd.ops.conv import ConvSpec
    spec = ConvSpec(*case)
    assert spec.Cp == spec.C
    Mx = spec.N * spec.H * spec.W
    dy = ops.to_nhwc(d['gy'])
    wf, wt = ops.pack_conv_weight(d['w'])[:2]
    xn = ops.to_nhwc(d['x'])
    dx = d['old'].to(torch.bfloat16).contiguous().clone() if acc else \
        torch.full((Mx, spec.Cp), float('nan'), dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros(spec.K * spec.R * spec.S * spec.C, device=DEV)
    return spec, Mx, dy, wt, xn, dx, dw


def _pair_case(case, kind, dplan, acc=False, two=False, act='relu', with_bw=True):
    """stride 1: bwd_pair_kernel; stride 2 (N <= 32): bwd_pair_s2_kernel"""
    ops = _ops()
    d = _data(case, kind)
    spec, Mx, dy, wt, xn, dx, dw = _tensors(ops, d, case, acc)
    bw = _bw(d, spec.C, Mx, two, act) if with_bw else None
    ops.conv_bwd(dy, wt, dx, xn, dw, spec, dplan=dplan, wplan=(64, 64, 1), accumulate=acc, bw=bw)
    _check(ops, d, dx, bw, case, kind, acc, two, act)
    close(dw, d['dw'])       # the wgrad half still runs


KINDS = ['random', 'integer']
# N, H, W, C, K, R, S, stride, pad
FULL = (2, 8, 8, 64, 64, 3, 3, 1, 1)       # M = 128: two full 64-row tiles, 9 dgrad stages
EDGE = (3, 5, 5, 64, 64, 3, 3, 1, 1)       # M = 75: the last tile has 11 valid rows
C40 = (3, 5, 5, 40, 64, 3, 3, 1, 1)        # chunk columns 5..7 of the only N tile are past N
C72 = (3, 5, 5, 72, 64, 3, 3, 1, 1)        # second N tile: one valid chunk column
S2 = (2, 8, 8, 64, 64, 3, 3, 2, 1)         # stride-2 parity classes, 8 x 8 -> 4 x 4
S2_ODD = (2, 7, 5, 64, 64, 3, 3, 2, 1)     # classes of 12 / 8 / 9 / 6 pixels per image


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', [FULL, EDGE, C40, C72])
def test_pair_tile_edges(case, kind):
    _pair_case(case, kind, (64, 64, 1), acc=True, two=True, act='relu')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('act', ['none', 'relu', 'relu6'])
@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('acc', [False, True])
def test_pair_options(acc, two, act, kind):
    _pair_case(EDGE, kind, (64, 64, 1), acc=acc, two=two, act=act)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('acc', [False, True])
def test_pair_without_sums(acc, kind):
    _pair_case(EDGE, kind, (64, 64, 1), acc=acc, with_bw=False)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('splits', [1, 2, 3])
def test_pair_split_k(splits, acc, kind):
    """9 stages over 1, 2 and 3 K slices: only the last arriver of a tile runs the epilogue"""
    _pair_case(EDGE, kind, (64, 64, splits), acc=acc, two=True, act='relu6')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', [FULL, EDGE])
def test_pair_128_wide_tile(case, kind):
    _pair_case(case, kind, (128, 64, 1), acc=True, two=True, act='relu')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('case', [S2, S2_ODD])
def test_pair_stride2_classes(case, acc, kind):
    _pair_case(case, kind, None, acc=acc, two=True, act='relu')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('plan', [(64, 64, 1), (64, 64, 3), (128, 128, 1)])
def test_dgrad_alone(plan, kind):
    """igemm_nt_kernel<.., TRANS>: the two-stage 64 x 64 kernel, split and unsplit, and the
    128 x 128 tile (one-stage loop, 16 chunks per row) on 128 channels"""
    ops = _ops()
    case = EDGE if plan[1] == 64 else (3, 5, 5, 128, 64, 3, 3, 1, 1)
    d = _data(case, kind)
    spec, Mx, dy, wt, xn, dx, dw = _tensors(ops, d, case, True)
    bw = _bw(d, spec.C, Mx, True, 'relu6')
    ops.conv_dgrad(dy, wt, dx, spec, plan=plan, accumulate=True, bw=bw)
    _check(ops, d, dx, bw, case, kind, True, True, 'relu6')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', [S2, S2_ODD])
def test_dgrad_s2_alone(case, kind):
    """dgrad_s2_kernel<64, 64, 2>"""
    ops = _ops()
    d = _data(case, kind)
    spec, Mx, dy, wt, xn, dx, dw = _tensors(ops, d, case, True)
    bw = _bw(d, spec.C, Mx, False, 'relu')
    ops.conv_dgrad(dy, wt, dx, spec, plan=(64, 64, 1), accumulate=True, bw=bw)
    _check(ops, d, dx, bw, case, kind, True, False, 'relu')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('acc', [False, True])
def test_shortcut_pair(acc, kind):
    """bwd_pair_sc_kernel: a 3x3 stride-1 pair on 4 x 4 images (sums fused) and the 1x1 stride-2
    shortcut's class pair on 8 x 8 -> 4 x 4 in one launch"""
    from mercury_amd.ops.conv import conv_bwd_sc
    ops = _ops()
    ca = (3, 4, 4, 64, 64, 3, 3, 1, 1)      # M = 48: one partial tile
    cb = (3, 8, 8, 64, 64, 1, 1, 2, 0)
    da, db = _data(ca, kind), _data(cb, kind)
    sa, Ma, dya, wta, xa, dxa, dwa = _tensors(ops, da, ca, acc)
    sb, Mb, dyb, wtb, xb, dxb, dwb = _tensors(ops, db, cb, acc)
    bw = _bw(da, sa.C, Ma, True, 'relu')
    ok = conv_bwd_sc(dict(dy=dya, wt=wta, dx=dxa, x=xa, dw=dwa, spec=sa, dplan=(64, 64, 1),
                          wplan=(64, 64, 1), accumulate=acc, bw=bw),
                     dict(dy=dyb, wt=wtb, dx=dxb, x=xb, dw=dwb, spec=sb, wplan=(64, 64, 1),
                          accumulate=acc))
    assert ok, 'the 64 x 64 shortcut pair must launch'
    _check(ops, da, dxa, bw, ca, kind, acc, True, 'relu')
    _check(ops, db, dxb, None, cb, kind, acc, False, 'none')
