"""The implicit-GEMM loop's buffer-addressed gathers (csrc/igemm.hip igemm_nt_body).

Both operands are read through buffer resources sized to the tensors' exact byte ranges; padding
taps, rows past M and chunks past a split's range take an out-of-range offset and load zeros, and
a row's valid filter taps are bit masks.  The shapes are small and sit where that addressing can
go wrong; the reference and tolerances are those of tests/test_kernels_gpu.py (``close``:
rtol = atol = 2e-2 against ``F.conv2d`` on bf16-rounded inputs).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')


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
PAD_ALL = (1, 3, 3, 64, 64, 3, 3, 1, 1)       # every pixel pads on some tap; M = 9 << tile
PART_TILE = (3, 5, 7, 64, 64, 3, 3, 1, 1)     # M = 105: a partial second tile
S2_UNEVEN = (2, 7, 5, 64, 128, 3, 3, 2, 1)    # uneven parity classes; one class has one tap
S2_1X1 = (2, 7, 5, 64, 64, 1, 1, 2, 0)        # three classes get no tap
C8_5X5 = (2, 6, 6, 8, 64, 5, 5, 1, 2)         # C/8 = 1: the lanes of a stage sit in 8 taps
K7X7 = (2, 9, 9, 16, 64, 7, 7, 2, 3)          # R*S = 49 taps: more than one 32-bit word
DEEP = (2, 4, 4, 512, 512, 3, 3, 1, 1)        # 72 k-stages, split 5 and 7 ways
CASES = [PAD_ALL, PART_TILE, S2_UNEVEN, S2_1X1, C8_5X5, K7X7, DEEP]
GUARDED = [PAD_ALL, PART_TILE, S2_UNEVEN]


@functools.lru_cache(maxsize=None)
def _data(case):
    """(x, w, gy, y_ref, dx_ref, dw_ref) of a case, computed once and shared (read-only)"""
    N, H, W, C, K, R, S, st, pd = case
    g = torch.Generator(device='cpu').manual_seed(11)
    x = bf(torch.randn(N, C, H, W, generator=g)).to(DEV)
    w = bf(torch.randn(K, C, R, S, generator=g) / math.sqrt(C * R * S)).to(DEV)
    P, Q = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
    gy = bf(torch.randn(N, K, P, Q, generator=g)).to(DEV)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=st, padding=pd)
    y.backward(gy)
    return x, w, gy, y.detach(), xr.grad, wr.grad


def _guarded(t, band=4096):
    """a contiguous copy of ``t`` in the middle of a larger allocation filled with NaN"""
    big = torch.full((t.numel() + 2 * band,), NAN, dtype=t.dtype, device=t.device)
    mid = big[band:band + t.numel()].view(t.shape)
    mid.copy_(t)
    assert mid.is_contiguous() and mid.data_ptr() % 16 == 0
    return mid


def _fwd(ops, case, plan=None, guard=False):
    from mercury_amd.ops.conv import ConvSpec, fwd_plan, slab_bytes
    x, w = _data(case)[:2]
    spec = ConvSpec(*case)
    xn, wk = ops.to_nhwc(x), ops.pack_conv_weight(w)[0]
    if guard:
        xn, wk = _guarded(xn), _guarded(wk)
    plan = plan or fwd_plan(spec)
    out = torch.empty(spec.M, spec.K, dtype=torch.bfloat16, device=DEV)
    slab = torch.zeros(max(1, slab_bytes(spec.M, spec.K, *plan) // 4), device=DEV)
    ops.conv_fwd(xn, wk, out, spec, slab=slab, plan=plan)
    return out


def _dgrad(ops, case, plan=None, guard=False):
    from mercury_amd.ops.conv import ConvSpec, dgrad_plan, slab_bytes
    N, H, W = case[:3]
    w, gy = _data(case)[1:3]
    spec = ConvSpec(*case)
    gyn, wt = ops.to_nhwc(gy), ops.pack_conv_weight(w)[1]
    if guard:
        gyn, wt = _guarded(gyn), _guarded(wt)
    plan = plan or dgrad_plan(spec)
    dx = torch.empty(N * H * W, spec.Cp, dtype=torch.bfloat16, device=DEV)
    slab = torch.zeros(max(1, slab_bytes(N * H * W, spec.Cp, *plan) // 4), device=DEV)
    ops.conv_dgrad(gyn, wt, dx, spec, slab=slab, plan=plan)
    return dx


def _nchw_out(out, case):
    from mercury_amd.ops.conv import ConvSpec
    spec = ConvSpec(*case)
    return out.view(spec.N, spec.P, spec.Q, spec.K).permute(0, 3, 1, 2)


def _nchw_dx(ops, dx, case):
    N, H, W, C = case[:4]
    return ops.from_nhwc(dx.view(N, H, W, -1), C)


@pytest.mark.parametrize('case', CASES)
def test_gather_fwd(case):
    ops = _ops()
    close(_nchw_out(_fwd(ops, case), case), _data(case)[3])


@pytest.mark.parametrize('case', CASES)
def test_gather_dgrad(case):
    ops = _ops()
    close(_nchw_dx(ops, _dgrad(ops, case), case), _data(case)[4])


@pytest.mark.parametrize('splits', [5, 7])
def test_gather_split_not_dividing_stages(splits):
    """72 k-stages over 5 / 7 splits: the last split is short and the two-stage prefetch of
    every split runs past its range (those loads must be zeros, not the next split's data)"""
    ops = _ops()
    close(_nchw_out(_fwd(ops, DEEP, plan=(64, 64, splits)), DEEP), _data(DEEP)[3])
    close(_nchw_out(_fwd(ops, DEEP, plan=(128, 128, splits)), DEEP), _data(DEEP)[3])
    close(_nchw_dx(ops, _dgrad(ops, DEEP, plan=(64, 64, splits)), DEEP), _data(DEEP)[4])


@pytest.mark.parametrize('case', GUARDED)
def test_gather_reads_stay_inside_the_tensors(case):
    """Activations and weights each sit in the middle of a NaN-filled allocation: a load outside
    a tensor's byte range would put a NaN into an output that is finite otherwise.  This is the
    check of the resource ranges -- one taken too large passes every other test."""
    ops = _ops()
    for run in (_fwd, _dgrad):
        plain, guarded = run(ops, case), run(ops, case, guard=True)
        assert bool(torch.isfinite(plain.float()).all())
        assert bool(torch.isfinite(guarded.float()).all()), 'read outside the tensor'
        assert torch.equal(plain, guarded)


def _separate(ops, case, dplan, wplan):
    from mercury_amd.ops.conv import ConvSpec
    N, H, W = case[:3]
    x, w, gy = _data(case)[:3]
    spec = ConvSpec(*case)
    dx = _dgrad(ops, case, plan=dplan)
    dw = torch.zeros(spec.K * spec.R * spec.S * spec.C, device=DEV)
    ops.conv_wgrad(ops.to_nhwc(gy), ops.to_nhwc(x), dw, spec, plan=wplan)
    return dx, dw


def _check_pair(dx, dw, dx2, dw2, dplan, wplan):
    if dplan[2] == 1:
        assert torch.equal(dx, dx2)
    close(dx, dx2, 1e-2, 1e-2)
    if wplan[2] == 1:
        assert torch.equal(dw, dw2)
    close(dw, dw2, 1e-2, 1e-2)


@pytest.mark.parametrize('case', [PAD_ALL, PART_TILE, DEEP, S2_UNEVEN, S2_1X1])
@pytest.mark.parametrize('unsplit', [True, False])
def test_gather_pair_matches_separate_launches(case, unsplit):
    """dgrad + wgrad in one launch (stride 1: bwd_pair_kernel; stride 2: bwd_pair_s2_kernel) ==
    the standalone kernels: dx bit-equal on unsplit tiles, dw bit-equal where unsplit"""
    ops = _ops()
    from mercury_amd.ops.conv import ConvSpec, dgrad_plan, slab_bytes, wgrad_plan
    N, H, W = case[:3]
    x, w, gy = _data(case)[:3]
    spec = ConvSpec(*case)
    s2 = spec.stride == 2
    dplan = (64, 64, 1) if unsplit or s2 else dgrad_plan(spec)
    wplan = (64, 64, 1) if unsplit else tuple(wgrad_plan(spec)[:3])
    dx2, dw2 = _separate(ops, case, None if s2 else dplan, wplan)
    Mx = N * H * W
    dx = torch.empty(Mx, spec.Cp, dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros_like(dw2)
    slab = torch.zeros(max(1, slab_bytes(Mx, spec.Cp, *dplan) // 4), device=DEV)
    ops.conv_bwd(ops.to_nhwc(gy), ops.pack_conv_weight(w)[1], dx, ops.to_nhwc(x), dw, spec,
                 dplan=dplan, wplan=wplan, slab=slab)
    _check_pair(dx, dw, dx2, dw2, dplan, wplan)
    close(_nchw_dx(ops, dx, case), _data(case)[4])
    close(dw.view(spec.K, spec.R, spec.S, spec.C).permute(0, 3, 1, 2), _data(case)[5])


def test_gather_shortcut_pair_matches_separate_launches():
    """A block's last 3x3 conv and its 1x1 stride-2 shortcut, both pairs in one launch
    (bwd_pair_sc_kernel), against the standalone dgrad / wgrad of each"""
    ops = _ops()
    from mercury_amd.ops.conv import ConvSpec, conv_bwd_sc, slab_bytes
    sc = S2_1X1                                   # 7 x 5 -> 4 x 3, 64 -> 64
    last = (2, 4, 3, 64, 64, 3, 3, 1, 1)          # the conv whose output the shortcut joins
    dplan, wplan = (64, 64, 1), (64, 64, 1)
    want = {c: _separate(ops, c, None if c is sc else dplan, wplan) for c in (last, sc)}
    args = {}
    for c in (last, sc):
        x, w, gy = _data(c)[:3]
        spec = ConvSpec(*c)
        Mx = spec.N * spec.H * spec.W
        args[c] = dict(dy=ops.to_nhwc(gy), wt=ops.pack_conv_weight(w)[1],
                       dx=torch.empty(Mx, spec.Cp, dtype=torch.bfloat16, device=DEV),
                       x=ops.to_nhwc(x), dw=torch.zeros_like(want[c][1]), spec=spec, wplan=wplan)
    args[last].update(dplan=dplan, slab=torch.zeros(
        max(1, slab_bytes(2 * 4 * 3, 64, *dplan) // 4), device=DEV))
    assert conv_bwd_sc(args[last], args[sc]), 'shortcut pair not launched'
    for c in (last, sc):
        _check_pair(args[c]['dx'], args[c]['dw'], want[c][0], want[c][1], dplan, wplan)
        close(_nchw_dx(ops, args[c]['dx'], c), _data(c)[4])


# a geometry whose gathered tensor (2 x 4096 x 4096 x 64 bf16 = 4 GiB) or weight
# (65536 x 7*7*1024 bf16 = 6.1 GiB) does not fit a 32-bit buffer resource
BIG_A = dict(SH=4096, SW=4096, SC=64, RP=4096, RQ=4096, R=3, S=3, stride=1, pad=1, Ncols=64,
             N=2)
BIG_B = dict(SH=8, SW=8, SC=1024, RP=8, RQ=8, R=7, S=7, stride=1, pad=3, Ncols=65536, N=2)


@pytest.mark.parametrize('geo', [BIG_A, BIG_B])
def test_gather_refuses_ranges_past_32_bits(geo):
    """Every launcher validates the byte ranges before it touches memory or launches: called
    with small dummy tensors and the oversized geometry only, each must raise."""
    ops = _ops()
    C = ops.lib()
    t = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    p, fp, st = t.data_ptr(), f.data_ptr(), torch.cuda.current_stream().cuda_stream
    g = dict(geo)
    N = g.pop('N')
    M = N * g['RP'] * g['RQ']
    Kc = g['R'] * g['S'] * g['SC'] // 8
    nobw = (0, 0, 0, 0, 0, 0, 0.0, 0.0, 0)
    geom = (g['SH'], g['SW'], g['SC'], g['RP'], g['RQ'], g['R'], g['S'], g['stride'], g['pad'],
            Kc, g['Ncols'], M)
    for trans in (False, True):
        with pytest.raises(ValueError, match='32-bit'):
            C.igemm(p, p, p, g['Ncols'], 0, 0, g['Ncols'], M, 0, 0, *geom, 64, 64, 1, trans, st,
                    *nobw)
    with pytest.raises(ValueError, match='32-bit'):
        C.igemm_pro(p, p, p, g['Ncols'], 0, 0, g['Ncols'], M, 0, *geom, 64, 64, 1, st,
                    0, fp, fp, fp, fp, 0, M, 1.0, 1e-5, 0, 0, 0)
    dual = [p, p, p, g['Ncols'], 0, g['Ncols'], M, 0, *geom, 1]
    small = [p, p, p, 64, 0, 64, 64, 0, 8, 8, 64, 8, 8, 1, 1, 1, 0, 8, 64, 64, 1]
    for a, b in ((dual, small), (small, dual)):
        with pytest.raises(ValueError, match='32-bit'):
            C.igemm_dual(a, b, 64, 64, st)
    wg = (N, g['RP'], g['RQ'], g['Ncols'], g['SH'], g['SW'], g['SC'], g['Ncols'])
    with pytest.raises(ValueError, match='32-bit'):
        C.conv_bwd_pair(p, p, p, g['Ncols'], 0, 0, *geom, 64, 64, 1, *nobw, p, fp, *wg,
                        64, 64, 1, 0, st)
    # the stride-2 launchers take the dy geometry (SH, SW = dy dims) and dx dims H, W
    s2 = (g['SH'], g['SW'], 64 * (g['SC'] // 64 or 1), 3, 3, 2, 1, g['Ncols'])
    H2, W2 = 2 * g['SH'], 2 * g['SW']
    if geo is BIG_A:
        with pytest.raises(ValueError, match='32-bit'):
            C.dgrad_s2(p, p, p, g['Ncols'], 0, *s2, 64, 64, H2, W2, N, st, *nobw)
        with pytest.raises(ValueError, match='32-bit'):
            C.conv_bwd_pair_s2(p, p, p, g['Ncols'], 0, *s2, 64, 64, H2, W2, N, *nobw, p, fp,
                               g['Ncols'], g['SH'], g['SW'], s2[2], g['Ncols'], 64, 64, 1, 0, st)
