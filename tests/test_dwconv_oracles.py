"""The depthwise oracles themselves (tests/dwconv_oracles.py), on the CPU: the references against
float64 ``F.conv2d`` / ``F.batch_norm`` and their autograd, the exactness bounds of the integer
data of every case, the path each case of tests/test_dwconv_paths_gpu.py was chosen for (from the
launch-arithmetic mirror), and the argument checks of the depthwise front-ends."""
import pytest
import torch
import torch.nn.functional as F

import dwconv_oracles as do

F64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('shape', [(2, 8, 5, 7, 1), (3, 16, 6, 9, 2), (2, 8, 1, 1, 1),
                                   (1, 8, 2, 3, 2), (2, 8, 7, 4, 2)], ids=str)
def test_dw_ref_matches_conv2d_and_autograd(shape):
    N, C, H, W, s = shape
    g = torch.Generator().manual_seed(5)
    P, Q = do.out_hw(H, W, s)
    x = torch.randn(N, H, W, C, generator=g, dtype=F64)
    w = torch.randn(C, 3, 3, generator=g, dtype=F64)
    gy = torch.randn(N, P, Q, C, generator=g, dtype=F64)
    y, dx, dw = do.dw_ref(x, w, gy, s)
    xr, wr = _nchw(x).requires_grad_(True), w[:, None].clone().requires_grad_(True)
    ref = F.conv2d(xr, wr, stride=s, padding=1, groups=C)
    assert ref.shape == (N, C, P, Q)
    ref.backward(_nchw(gy))
    for got, want in ((_nchw(y), ref.detach()), (_nchw(dx), xr.grad), (dw, wr.grad[:, 0])):
        assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))
    assert do.dw_ref(x, w, None, s)[1:] == (None, None)
    assert torch.equal(do.dw_ref(x, w, None, s)[0], y)


@pytest.mark.parametrize('mode', ['batch', 'ghost', 'running'])
@pytest.mark.parametrize('act', ['none', 'relu', 'relu6'])
def test_bn_ref_prologue_matches_batch_norm(mode, act):
    N, H, W, C, gi = 6, 3, 5, 8, (2 if mode == 'ghost' else 6)
    g = torch.Generator().manual_seed(9)
    y = torch.randn(N, H, W, C, generator=g, dtype=F64) * 2 + 0.3
    y[..., 3] = 0.5                                     # a constant channel: variance 0
    gamma = torch.rand(C, generator=g, dtype=F64) + 0.5
    beta = torch.randn(C, generator=g, dtype=F64)
    fact = {'none': lambda v: v, 'relu': F.relu, 'relu6': F.relu6}[act]
    if mode == 'running':
        rmean = torch.randn(C, generator=g, dtype=F64)
        rvar = torch.rand(C, generator=g, dtype=F64) + 0.5
        a, ysc, sh = do.bn_ref(y, gamma, beta, act, rmean=rmean, rvar=rvar)
        want = fact(F.batch_norm(_nchw(y), rmean, rvar, gamma, beta, False, 0.0, do.EPS))
    else:
        yg = y.reshape(N // gi, -1, C)
        stats = torch.stack([yg.sum(1), (yg * yg).sum(1)], 1)
        a, ysc, sh = do.bn_ref(y, gamma, beta, act, stats=stats, count=gi * H * W, group_imgs=gi)
        want = torch.cat([fact(F.batch_norm(_nchw(y[i:i + gi]), None, None, gamma, beta, True,
                                            0.0, do.EPS)) for i in range(0, N, gi)])
    # the constant channel: sqrt(eps) amplifies the 1e-16 of sum y^2 / n - mean^2 (316 * 1e-16)
    assert (_nchw(a) - want).abs().max() <= 1e-11
    assert ysc.shape == sh.shape == y.shape and (ysc >= 0).all() and (sh >= 0).all()


@pytest.mark.parametrize('act', ['none', 'relu', 'relu6'])
def test_bn_bwd_ref_matches_autograd(act):
    """sum dz = d/d beta and sum dz * xhat = d/d gamma of sum(dout * act(bn(y)))."""
    M, C = 200, 8
    g = torch.Generator().manual_seed(4)
    y = torch.randn(M, C, generator=g, dtype=F64) * 1.5 + 0.3
    dout = torch.randn(M, C, generator=g, dtype=F64)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=F64) + 2.0).requires_grad_(True)
    fact = {'none': lambda v: v, 'relu': F.relu, 'relu6': F.relu6}[act]
    out = fact(F.batch_norm(y, None, None, gamma, beta, True, 0.0, do.EPS))
    (out * dout).sum().backward()
    stats = torch.stack([y.sum(0), (y * y).sum(0)])
    sdz, sxh, sabs = do.bn_bwd_ref(dout, out.detach(), y, stats, act)
    assert (sdz - beta.grad).abs().max() <= 1e-11 and (sxh - gamma.grad).abs().max() <= 1e-11
    assert (sabs >= sxh.abs() - 1e-12).all()


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_int_data_is_exact_in_bf16_and_fp32(case):
    """int_data's own assertions (every reference quantity an integer below 2^24, |y| and |dx|
    <= 256, |mean| <= 2^-5), and that the references are integers at all."""
    d = do.int_data(case)
    for k in ('y', 'dx', 'dw', 'stats', 'sdz', 'st_in'):
        assert torch.equal(d[k], d[k].round()), k
    assert d['y'].abs().max() <= 36 and d['dx'].abs().max() <= 36
    # nine products of magnitude <= 4 per output; a sum of squares of at most 36^2 per pixel
    assert d['stats'][:, 1].max() <= 36 * 36 * (d['y'].numel() // case[1])
    m = do.act_mask(d['out'], d['act'])
    assert set(m.unique().tolist()) <= {0.0, 1.0}
    if d['act'] != 'none':
        assert 0 < m.mean() < 1


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_exact_cases_reach_their_paths(case):
    N, C, H, W, s, G = case
    assert set(do.PATHS) == set(do.EXACT_CASES)
    do.assert_path(case, do.dispatch(N, C, H, W, s, groups=G, stats=True, bw=True))


def test_dispatch_details_of_the_large_cases():
    # DH = 2 and LOOP: 270 blocks before the cap; without statistics no cap and no loop
    d = do.dispatch(128, 96, 17, 18, 1, stats=False)
    assert d['fwd_blocks'] == 270 and not d['loop'] and d['straddle'] == 0
    assert do.dispatch(128, 96, 17, 18, 1, bw=False)['dg_blocks'] == 510
    # ghost groups never loop, whatever the size
    assert not do.dispatch(128, 96, 17, 18, 1, groups=4)['loop']
    # the BW cap: 628 and 576 blocks without it, and a plain grid (stride = T) without bw
    for shape, blocks in (((32, 144, 31, 33, 1), 628), ((32, 144, 32, 32, 2), 576)):
        d = do.dispatch(*shape, bw=False)
        assert d['dg_blocks'] == blocks and not d['capped'] and d['dg_stride'] == blocks * 256
        assert d['dg_trips'] == 1
        assert (256 * 256) % (shape[1] // 8) == 16
    # odd P with two rows per thread: the last row group is half empty
    assert do.dispatch(128, 16, 5, 7, 1)['per_img'] == 3 * 2 * 2
    # the wgrad without a slab never splits a row
    assert do.dispatch(2, 16, 25, 25, 1)['nblk_atomic'] == 1


def test_prologue_shapes_reach_their_paths():
    """DH = 2 with ghost groups of 32 images (straddling blocks), and the grid-stride forward
    with the prologue: 96 images loop, the 64-image shape (192 blocks) stays under the cap."""
    d = do.dispatch(128, 16, 5, 7, 1, groups=4)
    assert d['DH'] == 2 and d['straddle'] == 2
    d = do.dispatch(64, 96, 16, 16, 1)
    assert d['DH'] == 1 and d['fwd_blocks'] == 192 and not d['loop']
    d = do.dispatch(96, 96, 16, 16, 1)
    assert d['DH'] == 1 and d['loop'] and d['fwd_stride'] == 65532 and d['fwd_trips'] == 2
    assert do.dispatch(4, 40, 5, 11, 1)['DH'] == 1 and do.dispatch(6, 24, 8, 12, 2)['P'] == 4
    for N, C, H, W, s, gi in do.PRO_SHAPES:
        assert N % gi == 0 and do.out_hw(H, W, s) == (H // s, W // s)    # a 'same' conv


def test_reduce_layers_cover_the_shares_thresholds():
    L = do.RED_LAYERS
    assert len(L) == 26 > do.DW_RED_MAX and len(set(L)) == 26
    assert {c for c, _ in L} == set(do.RED_C) and {n for _, n in L} == set(do.RED_NBLK)
    assert [do.red_shares(n) for n in do.RED_NBLK] == [1, 1, 1, 4, 4, 8, 8]
    first, second = L[:24], L[24:]
    # shares come from the largest layer of a launch: 8 and 4; layers with fewer blocks than that
    assert do.red_shares(max(n for _, n in first)) == 8 and min(n for _, n in first) < 8
    assert do.red_shares(max(n for _, n in second)) == 4
    # a narrow layer next to the widest one, in both launches (the early return)
    assert (960, 127) in first and (8, 128) in first and second == [(960, 32), (8, 127)]


# --------------------------------------------------------------------------- argument checks
def _no_lib(monkeypatch):
    from mercury_amd.ops import misc

    def boom():
        raise AssertionError('the library was loaded before the check')
    monkeypatch.setattr(misc, 'lib', boom)
    return misc


@pytest.mark.parametrize('C', [12, 4, 0, 100])
def test_dwconv_rejects_channels_not_a_multiple_of_8(monkeypatch, C):
    misc = _no_lib(monkeypatch)
    t = None
    with pytest.raises(ValueError, match='multiple of 8'):
        misc.dwconv_fwd(t, t, t, 1, 4, 4, C, 4, 4, 1, 1)
    with pytest.raises(ValueError, match='multiple of 8'):
        misc.dwconv_dgrad(t, t, t, 1, 4, 4, C, 4, 4, 1, 1)
    with pytest.raises(ValueError, match='multiple of 8'):
        misc.dwconv_bwd(t, t, t, t, t, 1, 4, 4, C, 4, 4, 1, 1, t)
    with pytest.raises(ValueError, match='multiple of 8'):
        misc.dwconv_wgrad(t, t, t, 1, 4, 4, C, 4, 4, 1, 1)


def test_dwconv_rejects_bw_above_2048_channels(monkeypatch):
    misc = _no_lib(monkeypatch)
    t = None
    with pytest.raises(ValueError, match='2048'):
        misc.dwconv_dgrad(t, t, t, 1, 4, 4, 2056, 4, 4, 1, 1, bw={})
    with pytest.raises(ValueError, match='2048'):
        misc.dwconv_bwd(t, t, t, t, t, 1, 4, 4, 2056, 4, 4, 1, 1, t, bw={})


def test_no_model_reaches_a_rejected_depthwise_shape():
    """Every grouped conv of the model zoo is depthwise with a width the kernels take."""
    import torch.nn as nn
    from mercury_amd.models.mobilenetv2 import MobileNetV2
    widths = [m.in_channels for m in MobileNetV2().modules()
              if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(widths) == 17
    assert all(c % 8 == 0 and 8 <= c <= 2048 for c in widths)
