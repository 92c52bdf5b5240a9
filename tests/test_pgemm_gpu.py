"""Persistent pointwise GEMM (csrc/pgemm.hip) vs fp32 torch: the 1x1 convs of ResNet-50's
bottlenecks and MobileNetV2's expand / project layers (`pytorch_model.py:44-49`).  Covers every
tile width, odd channel counts (K, N not multiples of 32 / 64), M not a tile multiple, stride-2
row gathers, ghost-BN statistics with groups that straddle tiles, and more tiles than blocks
(the persistent step stream crossing tile boundaries).  The panel-resident narrow-input kernel
(csrc/pwconv.hip, K <= 128) runs the same checks on its stride-1 shapes."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def bf(x):
    return x.to(torch.bfloat16).float()


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, 'max err %g (scale %g)' % (err, scale)


CASES = [
    # N, H, W, C, K, stride, group_imgs, bn, grid
    (32, 16, 16, 256, 64, 1, 0, 64, 0),
    (32, 16, 16, 64, 256, 1, 0, 256, 0),
    (16, 14, 14, 512, 128, 1, 4, 128, 0),      # 784-row groups: tiles straddle group edges
    (8, 28, 28, 128, 512, 2, 0, 256, 0),       # stride-2 shortcut gather
    (20, 8, 8, 96, 24, 1, 0, 64, 0),           # MobileNetV2 project: N = 24, K = 96
    (20, 8, 8, 24, 144, 1, 5, 128, 0),         # expand: K = 24 (< one 32-deep step)
    (12, 9, 11, 40, 72, 1, 0, 64, 7),          # M = 1188 (not a tile multiple), 7 blocks
    (64, 7, 7, 2048, 512, 1, 32, 256, 5),      # deep K, few blocks: long step streams
    # pwconv-only shapes: every panel depth (32 / 64 / 96 / 128 channels), N not a 64 multiple
    (16, 14, 14, 64, 256, 1, 4, 0, 0),
    (10, 10, 10, 96, 200, 1, 2, 0, 0),         # 200-row groups: blocks straddle group edges
    (9, 7, 13, 128, 512, 1, 3, 0, 0),
    # large M: 200-row groups (every other 128-row panel straddles a group edge), 16384-row groups
    (2700, 10, 20, 32, 96, 1, 1, 0, 0),
    (128, 64, 64, 64, 128, 1, 4, 0, 0),
]


def _pw_ok(C, st, resid=False):
    return st == 1 and C <= 128 and not resid


def _kern_cases(cases, bn_at, pw_ok):
    # only the (case, kernel) pairs that apply: pgemm where a tile width is given (bn != 0),
    # pwconv on its stride-1 narrow-input shapes
    return [(c, k) for c in cases for k in ('pgemm', 'pwconv')
            if (k == 'pgemm' and c[bn_at] != 0) or (k == 'pwconv' and pw_ok(c))]


@pytest.mark.parametrize('case,kern', _kern_cases(CASES, 7, lambda c: _pw_ok(c[3], c[5])))
def test_pgemm_matches_torch(case, kern):
    from mercury_amd import ops
    from mercury_amd.ops.conv import ConvSpec
    ops.lib()
    N, H, W, C, K, st, gimgs, bn, grid = case

    def run(xn, wk, out, spec, stats=None):
        if kern.startswith('pwconv'):
            return ops.pwconv_fwd(xn, wk, out, spec, stats=stats)
        return ops.pgemm_fwd(xn, wk, out, spec, stats=stats, bn=bn, grid=grid)
    g = torch.Generator(device='cpu').manual_seed(hash(case) % 1000)
    x = bf(torch.randn(N, C, H, W, generator=g)).to(DEV)
    w = bf(torch.randn(K, C, 1, 1, generator=g) / math.sqrt(C)).to(DEV)
    spec = ConvSpec(N, H, W, C, K, 1, 1, st, 0)
    G = N // gimgs if gimgs else 1
    if gimgs:
        spec.group_rows = gimgs * spec.P * spec.Q
    xn = ops.to_nhwc(x)
    wk, _ = ops.pack_conv_weight(w)
    out = torch.full((spec.M, K), float('nan'), dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(G, 2, K, device=DEV)
    run(xn, wk, out, spec, stats=stats)
    ref = F.conv2d(x, w, stride=st)
    got = out.view(N, spec.P, spec.Q, K).permute(0, 3, 1, 2)
    assert not torch.isnan(got.float()).any()
    close(got, ref)
    rb = bf(ref)
    per = gimgs or N
    r = rb.view(G, per, K, spec.P, spec.Q)
    close(stats[:, 0], r.sum((1, 3, 4)), rtol=1e-2, atol=0.5)
    close(stats[:, 1], r.pow(2).sum((1, 3, 4)), rtol=1e-2, atol=0.5)
    # no stats: plain GEMM path, bitwise equal output
    out2 = torch.empty_like(out)
    run(xn, wk, out2, spec)
    assert torch.equal(out2, out)


PRO_CASES = [
    # N, H, W, C, K, group_imgs, bn, act, residual, eval
    (16, 14, 14, 256, 64, 4, 64, 'relu', False, False),     # R50 conv3-style input BN
    (16, 14, 14, 128, 512, 4, 128, 'relu', True, False),    # block-final BN + identity residual
    (8, 16, 16, 96, 24, 0, 64, 'none', True, False),        # MobileNetV2 linear bottleneck + res
    (8, 16, 16, 24, 144, 2, 128, 'relu6', False, False),    # expand after a project BN, K < 32
    (12, 9, 11, 40, 72, 0, 64, 'relu', False, True),        # eval: running statistics
    (32, 7, 7, 512, 2048, 8, 256, 'relu', True, False),     # wide N: 256 -> 128 tile
    (16, 14, 14, 64, 256, 4, 64, 'relu', False, False),     # R50 conv3: 64 -> 256, 4 N-tiles
    (9, 10, 10, 128, 520, 3, 64, 'relu', False, False),     # 300-row groups, N % 64 != 0
    (6, 12, 12, 96, 576, 0, 64, 'relu6', False, True),      # MobileNetV2 expand, eval
    (2700, 10, 20, 32, 96, 1, 0, 'relu6', False, False),    # large M, 200-row groups
]


@pytest.mark.parametrize('case,kern', _kern_cases(PRO_CASES, 6, lambda c: _pw_ok(c[3], 1, c[8])))
def test_pgemm_input_bn_prologue(case, kern):
    """pgemm(pro=...) == bn_apply (+ residual) pass followed by the plain conv, and == an fp32
    torch reference; the kept activation == bn_apply's output."""
    from mercury_amd import ops
    from mercury_amd.ops.conv import ConvSpec
    ops.lib()
    N, H, W, C, K, gimgs, bn, act, resid, ev = case
    g = torch.Generator(device='cpu').manual_seed(7 + C + K)
    rows = N * H * W
    y = bf(torch.randn(rows, C, generator=g) * 2 + 0.5).to(DEV)
    res = bf(torch.randn(rows, C, generator=g)).to(DEV) if resid else None
    w = bf(torch.randn(K, C, 1, 1, generator=g) / math.sqrt(C)).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
    rmean = (torch.randn(C, generator=g) * 0.2).to(DEV)
    rvar = (torch.rand(C, generator=g) + 0.5).to(DEV)
    spec = ConvSpec(N, H, W, C, K, 1, 1, 1, 0)
    G = N // gimgs if gimgs else 1
    grp = (gimgs or N) * H * W
    if gimgs:
        spec.group_rows = grp
    yg = y.view(G, grp, C)
    stats = torch.stack([yg.sum(1), yg.pow(2).sum(1)], 1).contiguous()       # [G][2][C]
    yb = y.to(torch.bfloat16)
    rb = res.to(torch.bfloat16) if resid else None
    # reference activation
    if ev:
        mean, var = rmean.view(1, 1, C), rvar.view(1, 1, C)
    else:
        mean = (stats[:, 0] / grp).view(G, 1, C)
        var = (stats[:, 1] / grp).view(G, 1, C) - mean ** 2
    a = (yg - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    if resid:
        a = a + res.view(G, grp, C)
    a = {'relu': torch.relu, 'relu6': lambda t: t.clamp(0, 6), 'none': lambda t: t}[act](a)
    a = a.reshape(rows, C)
    ref = bf(a) @ w.view(K, C).t()
    wk, _ = ops.pack_conv_weight(w)
    keep = torch.full_like(yb, float('nan'))
    coef = torch.zeros(G * 2 * C, device=DEV)
    pro = dict(gamma=gamma, beta=beta, act=act, eps=1e-5, keep=keep, coef=coef, group_rows=grp,
               count=grp, res=rb)
    if ev:
        pro.update(rmean=rmean, rvar=rvar)
    else:
        pro.update(stats=stats.reshape(-1))
    out = torch.empty(rows, K, dtype=torch.bfloat16, device=DEV)
    ostats = torch.zeros(G, 2, K, device=DEV)
    if kern.startswith('pwconv'):
        ops.pwconv_fwd(yb, wk, out, spec, stats=ostats, pro=pro)
    else:
        ops.pgemm_fwd(yb, wk, out, spec, stats=ostats, bn=bn, pro=pro)
    close(out, ref)
    # unfused: bn_apply (+ residual) pass, then the plain conv
    an = torch.empty_like(yb)
    ops.bn_apply(yb, None if ev else stats.reshape(-1), gamma, beta, an, rows, C,
                 group_rows=grp if gimgs else 0, act=act, running=(rmean, rvar) if ev else None,
                 res=rb)
    out2 = torch.empty_like(out)
    ostats2 = torch.zeros_like(ostats)
    if kern.startswith('pwconv'):
        ops.pwconv_fwd(an, wk, out2, spec, stats=ostats2)
    else:
        ops.pgemm_fwd(an, wk, out2, spec, stats=ostats2, bn=bn)
    close(out, out2, rtol=1e-2, atol=1e-2)
    close(ostats, ostats2, rtol=1e-2, atol=0.5)
    assert not torch.isnan(keep.float()).any()
    close(keep.float(), an.float(), rtol=1e-2, atol=1e-2)
    assert torch.equal(keep, an), '%d of %d elements differ' % ((keep != an).sum().item(),
                                                                keep.numel())


COEF_CASES = [
    # N, H, W, C, group_imgs, eval
    # groups of 256 rows: the smallest both launchers accept (pgemm's prologue needs groups of
    # at least one 256-row tile, pwconv's of one 128-row panel)
    (4, 8, 8, 24, 0, False),       # one group
    (8, 8, 8, 24, 4, False),       # two ghost groups
    (4, 8, 8, 40, 0, True),        # running statistics
]


@pytest.mark.parametrize('case', COEF_CASES)
def test_coef_workspace_pgemm_equals_pwconv(case):
    """The scale / shift workspace ([G][2][C]) that the pgemm path (bn = 64) and the pwconv path
    derive from the same producer statistics is the same to the bit (both reach one kernel through
    bn_coef_launch), and equals the fp32 formula to the statistics rtol of this file (v_rsq_f32 is
    not correctly rounded, so no bitwise match with torch is expected)."""
    from mercury_amd import ops
    from mercury_amd.ops.conv import ConvSpec
    ops.lib()
    N, H, W, C, gimgs, ev = case
    K = 64
    g = torch.Generator(device='cpu').manual_seed(11 + C + N)
    rows = N * H * W
    yb = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV)
    w = bf(torch.randn(K, C, 1, 1, generator=g) / math.sqrt(C)).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
    rmean = (torch.randn(C, generator=g) * 0.2).to(DEV)
    rvar = (torch.rand(C, generator=g) + 0.5).to(DEV)
    spec = ConvSpec(N, H, W, C, K, 1, 1, 1, 0)
    G = N // gimgs if gimgs else 1
    grp = (gimgs or N) * H * W
    if gimgs:
        spec.group_rows = grp
    yg = yb.float().view(G, grp, C)
    stats = torch.stack([yg.sum(1), yg.pow(2).sum(1)], 1).contiguous()       # [G][2][C]
    wk, _ = ops.pack_conv_weight(w)
    coefs = []
    for kern in ('pgemm', 'pwconv'):
        coef = torch.zeros(G * 2 * C, device=DEV)
        pro = dict(gamma=gamma, beta=beta, act='relu', eps=1e-5, coef=coef, group_rows=grp,
                   count=grp)
        if ev:
            pro.update(rmean=rmean, rvar=rvar)
        else:
            pro.update(stats=stats.reshape(-1))
        out = torch.empty(rows, K, dtype=torch.bfloat16, device=DEV)
        if kern == 'pwconv':
            ops.pwconv_fwd(yb, wk, out, spec, pro=pro)
        else:
            ops.pgemm_fwd(yb, wk, out, spec, bn=64, pro=pro)
        coefs.append(coef.view(G, 2, C))
    assert torch.equal(coefs[0], coefs[1])
    if ev:
        mean, var = rmean.view(1, C), rvar.view(1, C)
    else:
        mean = stats[:, 0] / grp
        var = (stats[:, 1] / grp - mean ** 2).clamp_min(0)
    sc = gamma / torch.sqrt(var + 1e-5)
    for coef in coefs:
        close(coef[:, 0], sc.expand(G, C), rtol=1e-2, atol=0)
        close(coef[:, 1], (beta - mean * sc).expand(G, C), rtol=1e-2, atol=0)
