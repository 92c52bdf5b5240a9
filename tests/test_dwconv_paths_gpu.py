"""Dispatch paths and tails of the depthwise 3x3 kernels (csrc/dwconv.hip), held exactly.

The shapes are chosen by path, not by size: two output rows per thread (N >= 128, stride 1)
with odd and even P, blocks that span two ghost groups, the grid-stride forward, the capped
grid-stride dgrad with its BN-backward sums (standalone and in the dgrad + wgrad pair), wgrad
rows whose last column segment is empty, one-pixel and 2 x 3 images, C = 8.  Each case asserts
the path it was chosen for through the launch-arithmetic mirror ``dwconv_oracles.dispatch``
(the table is ``dwconv_oracles.PATHS``), whose block count is checked against the library
here.

Integer data (``dwconv_oracles.int_data``): every y, dx, dw, BN sum and sum of dz is an integer
that bf16 / fp32 hold exactly, so the kernels must reproduce the float64 reference bit for bit
(``torch.equal``), whatever the order of their additions.  Outputs are pre-filled with NaN and
followed by a guard of a sentinel that must survive (a whole output row + 64 elements behind
the forward's y).

Three comparisons are not exact.  Each test prints ``RATIO <what> <case> <err / bound>``
(pytest -rP shows the lines); the largest measured on an MI355X, per case:

  sum dz * xhat (dgrad and pair, K = ``dispatch``'s dg_chain: strips per thread -- a strip
  counted as one addition although it holds up to four columns, so K is on the strict side --
  + 256 / C8 + blocks per replica + SUMS_R + 8)
    (128, 16, 5, 7, 1, 1)    0.0014      (128, 16, 5, 7, 1, 4)    0.0014
    (128, 24, 6, 9, 1, 4)    0.0017      (130, 40, 3, 5, 1, 1)    0.0042
    (128, 16, 1, 1, 1, 1)    0.0057      (1, 8, 1, 1, 1, 1)       0 (xhat == 0)
    (1, 8, 2, 3, 2, 1)       0.0032      (128, 96, 17, 18, 1, 1)  0.0015
    (2, 16, 25, 25, 1, 1)    0.0028      (2, 16, 9, 27, 1, 1)     0.0071
    (2, 16, 50, 50, 2, 1)    0.0020      (32, 144, 31, 33, 1, 1)  0.0020
    (32, 144, 32, 32, 2, 1)  0.0017
  prologue, per shape (largest over the nine statistics x activation modes): keep and conv
  against 2^-8 |ref| + the fp32 allowance -- close to 1 by nature, some element always rounds
  at nearly half a bf16 ulp -- with, in brackets, the share of the fp32 allowance needed
  beyond that half ulp; the output statistics against K * 2^-24 * sum |terms|
                               keep            conv            statistics
    (4, 40, 5, 11, 1)          0.993 (0)       0.994 (0)       0.10
    (6, 24, 8, 12, 2)          0.991 (0)       0.991 (0)       0.051
    (128, 16, 5, 7, 1)         0.993 (0)       0.996 (0)       0.077
    (64, 96, 16, 16, 1)        0.994 (0.032)   0.996 (0.038)   0.14
    (96, 96, 16, 16, 1)        0.994 (0.019)   0.996 (0.056)   0.11
"""
import functools
import os

import pytest
import torch

import dwconv_oracles as do

_ENV = [k for k in ('MERCURY_DW_DH', 'MERCURY_DW_STAT_BLOCKS') if os.environ.get(k)]
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(_ENV), reason='%s overrides the dispatch these cases are '
                                 'chosen for' % ' / '.join(_ENV))]

DEV = 'cuda'
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -77.0            # exact in bf16
NAN = float('nan')


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def guarded(n, dtype, fill, guard=64):
    """(buffer, view of its first n elements): ``fill`` in front, ``guard`` sentinels behind."""
    buf = torch.full((n + guard,), fill, dtype=dtype, device=DEV)
    buf[n:] = SENT
    return buf, buf[:n]


def intact(buf, view, what):
    assert bool((buf[view.numel():] == SENT).all()), '%s: written behind the end' % what


def same_bits(a, b):
    it = {BF16: torch.int16, F32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def ratio(err, bound):
    """max err / bound (0 / 0 = 0, x / 0 = inf, NaN = inf)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float(r.max())


def record(what, case, r):
    print('RATIO %s %s %.3g' % (what, case, r))
    return r


def bf16_criterion(what, case, out, ref, mag_term):
    """|out - ref| <= 2^-8 |ref| + mag_term, elementwise; returns err / bound, and prints that
    and the share of ``mag_term`` (the fp32 arithmetic's allowance) the output needed beyond
    the bf16 half ulp."""
    err = (out - ref).abs()
    half = do.HALF_ULP_BF16 * ref.abs()
    record(what + '-fp32-share', case, ratio((err - half).clamp(min=0.0), mag_term))
    return record(what, case, ratio(err, half + mag_term))


# --------------------------------------------------------------------------- exact cases
@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands and expected outputs of a case on the device (computed once, read-only)."""
    d = do.int_data(case)
    N, C, H, W, s, G = case

    def dev(t, dtype):
        return t.to(dtype).reshape(-1).to(DEV)
    D = dict(P=d['P'], Q=d['Q'], M=d['M'], act=d['act'],
             disp=do.dispatch(N, C, H, W, s, groups=G, stats=True, bw=True))
    do.assert_path(case, D['disp'])
    for k in ('x', 'gy', 'y', 'dx', 'yin', 'out'):
        D[k] = dev(d[k], BF16)
    for k in ('w', 'dw0', 'stats', 'st_in', 'sdz'):
        D[k] = dev(d[k], F32)
    D['dw'] = dev(d['dw'] + d['dw0'], F32)                  # a wgrad ADDS to what dw holds
    D['sxh'], D['sabs'] = d['sxh'].to(DEV), d['sabs'].to(DEV)
    return D


def _dims(case):
    N, C, H, W, s, G = case
    D = _case(case)
    return D, (N, H, W, C, D['P'], D['Q'], s, 1)


def _bw(D, C):
    sbuf, sums = guarded(_ops().sums_numel(C), F32, 0.0)
    return sbuf, sums, dict(out=D['out'], y=D['yin'], stats=D['st_in'], sums=sums, act=D['act'],
                            eps=1e-5)


def _check_sums(what, case, D, sbuf, sums):
    """sum dz exactly; sum dz * xhat within K * 2^-24 * sum |dz * xhat| (K from the mirror)."""
    C = case[1]
    tot = _ops().sums_total(sums, C)
    intact(sbuf, sums, what)
    assert torch.equal(tot[0], D['sdz']), '%s: sum dz' % what
    assert not bool(tot[2].any()), '%s: the shortcut row is not this kernel\'s' % what
    err = (tot[1].to(F64) - D['sxh']).abs()
    bound = D['disp']['dg_chain'] * do.U * D['sabs']
    r = record(what, case, ratio(err, bound))
    assert r <= 1.0, '%s: sum dz*xhat off by %.3g of its bound (K = %d)' % (
        what, r, D['disp']['dg_chain'])


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_mirror_matches_the_library(case):
    ops = _ops()
    N, C, H, W, s, G = case
    d = do.dispatch(N, C, H, W, s, groups=G)
    assert ops.dwconv_wgrad_blocks(N, d['P'], d['Q'], C) == d['nblk']
    assert ops.dwconv_wgrad_slab_floats(N, d['P'], d['Q'], C) == d['nblk'] * 9 * C
    assert do.SUMS_R * 3 * C == ops.sums_numel(C)


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_forward_exact(case):
    """y and the per-group sums of y and y^2, with and without statistics."""
    ops = _ops()
    D, dims = _dims(case)
    N, C, G = case[0], case[1], case[5]
    P, Q = D['P'], D['Q']
    for with_stats in (False, True):
        ybuf, y = guarded(N * P * Q * C, BF16, NAN, 64 + Q * C)
        sbuf, st = guarded(G * 2 * C, F32, 0.0) if with_stats else (None, None)
        ops.dwconv_fwd(D['x'], D['w'], y, *dims, stats=st,
                       group_rows=(N // G) * P * Q if G > 1 else 0)
        assert torch.equal(y, D['y']), 'y (stats %s)' % with_stats
        intact(ybuf, y, 'y')
        if with_stats:
            assert torch.equal(st, D['stats']), 'sum y / sum y^2'
            intact(sbuf, st, 'stats')


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_dgrad_exact(case):
    """dx alone, and with ``bw``: the same dx plus the BN-backward sums."""
    ops = _ops()
    D, dims = _dims(case)
    C = case[1]
    for with_bw in (False, True):
        xbuf, dx = guarded(D['M'] * C, BF16, NAN)
        sbuf, sums, bw = _bw(D, C) if with_bw else (None, None, None)
        ops.dwconv_dgrad(D['gy'], D['w'], dx, *dims, bw=bw)
        assert torch.equal(dx, D['dx']), 'dx (bw %s)' % with_bw
        intact(xbuf, dx, 'dx')
        if with_bw:
            _check_sums('dgrad', case, D, sbuf, sums)


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
def test_wgrad_exact(case):
    """dw += the weight gradient: with atomics (no slab, whole rows) and through a NaN-filled
    slab (column segments + the reduce kernel), onto a dw that already holds integers."""
    ops = _ops()
    D, dims = _dims(case)
    C = case[1]
    for with_slab in (False, True):
        wbuf, dw = guarded(C * 9, F32, NAN)
        dw.copy_(D['dw0'])
        lbuf, slab = guarded(D['disp']['nblk'] * 9 * C, F32, NAN) if with_slab else (None, None)
        ops.dwconv_wgrad(D['gy'], D['x'], dw, *dims, slab=slab)
        assert torch.equal(dw, D['dw']), 'dw (slab %s)' % with_slab
        intact(wbuf, dw, 'dw')
        if with_slab:
            intact(lbuf, slab, 'slab')
            assert not bool(torch.isnan(slab).any()), 'a block left its slab row unwritten'
            part = slab.view(-1, 9, C).to(F64).sum(0).t().reshape(-1)       # [C][9]
            assert torch.equal(part, (D['dw'] - D['dw0']).to(F64)), 'slab partials'


@pytest.mark.parametrize('case', do.EXACT_CASES, ids=str)
@pytest.mark.parametrize('mode', ['reduce', 'deferred', 'plain'])
def test_bwd_pair_exact(case, mode):
    """dgrad + slab wgrad in one launch: with ``bw`` and the reduce at once, with ``bw`` and the
    reduce deferred (dw untouched, bit for bit, until dwconv_wgrad_reduce_batch), without bw."""
    ops = _ops()
    D, dims = _dims(case)
    C = case[1]
    nblk = D['disp']['nblk']
    xbuf, dx = guarded(D['M'] * C, BF16, NAN)
    wbuf, dw = guarded(C * 9, F32, NAN)
    dw.copy_(D['dw0'])
    lbuf, slab = guarded(nblk * 9 * C, F32, NAN)
    sbuf, sums, bw = _bw(D, C) if mode != 'plain' else (None, None, None)
    ops.dwconv_bwd(D['gy'], D['x'], D['w'], dx, dw, *dims, slab, bw=bw,
                   reduce=mode != 'deferred')
    if mode == 'deferred':
        assert same_bits(dw, D['dw0']), 'dw changed before the batched reduce'
        ops.dwconv_wgrad_reduce_batch([(slab, dw, C, nblk)])
    assert torch.equal(dx, D['dx']), 'dx'
    assert torch.equal(dw, D['dw']), 'dw'
    for buf, view, what in ((xbuf, dx, 'dx'), (wbuf, dw, 'dw'), (lbuf, slab, 'slab')):
        intact(buf, view, what)
    if bw is not None:
        _check_sums('pair-' + mode, case, D, sbuf, sums)


# --------------------------------------------------------------------------- batched reduce
def _run_reduce(layers, seed):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    items, want, bufs = [], [], []
    for C, nblk in layers:
        slab = torch.randint(-3, 4, (nblk, 9, C), generator=g).to(F32).to(DEV)
        wbuf, dw = guarded(C * 9, F32, NAN)
        dw.copy_(torch.randint(-5, 6, (C * 9,), generator=g).to(F32))
        want.append(dw.to(F64) + slab.to(F64).sum(0).t().reshape(-1))      # [C][9]
        items.append((slab.reshape(-1), dw, C, nblk))
        bufs.append(wbuf)
    ops.dwconv_wgrad_reduce_batch(items)
    for i, ((_, dw, C, nblk), w, wbuf) in enumerate(zip(items, want, bufs)):
        assert torch.equal(dw.to(F64), w), 'layer %d (C %d, %d blocks)' % (i, C, nblk)
        intact(wbuf, dw, 'dw of layer %d' % i)


def test_reduce_batch_26_layers_two_launches():
    """dw[c][t] = old + the sum over the blocks, exactly, for 26 layers of mixed widths and
    block counts: two launches, 8 and 4 shares, layers with fewer blocks than shares, a C = 8
    layer beside a C = 960 one (tests/test_dwconv_oracles.py asserts that mix)."""
    _run_reduce(do.RED_LAYERS, 1)


@pytest.mark.parametrize('layer', [(40, 3), (144, 300)], ids=str)
def test_reduce_batch_one_layer(layer):
    _run_reduce([layer], 2)


def test_reduce_batch_empty_list_is_a_no_op():
    assert _ops().dwconv_wgrad_reduce_batch([]) is None
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- input prologue
@functools.lru_cache(maxsize=None)
def _pro_data(shape):
    N, C, H, W, s, _ = shape
    g = torch.Generator().manual_seed(21)
    y = (torch.randn(N, H, W, C, generator=g) * 2 + 0.3)
    y[..., 3] = 0.5                                       # a constant channel: the variance clamp
    return dict(y=y.to(BF16).to(DEV), w=(torch.randn(C, 3, 3, generator=g) * 0.3).to(DEV),
                gamma=(torch.rand(C, generator=g) + 0.5).to(DEV),
                beta=(torch.randn(C, generator=g) * 0.3).to(DEV),
                rmean=(torch.randn(C, generator=g) * 0.5 + 0.3).to(DEV),
                rvar=(torch.rand(C, generator=g) * 2.5 + 0.5).to(DEV))


@pytest.mark.parametrize('act', ['none', 'relu', 'relu6'])
@pytest.mark.parametrize('mode', ['batch', 'ghost', 'running'])
@pytest.mark.parametrize('shape', do.PRO_SHAPES, ids=str)
def test_input_prologue(shape, mode, act):
    """act(bn(y)) applied to the loaded chunks: the kept activation against the float64 BN, the
    conv against the float64 conv of that kept activation, the output statistics against the
    sums of the kernel's own output, and keep=None == keep given, bit for bit."""
    ops = _ops()
    N, C, H, W, s, gi = shape
    P, Q = H // s, W // s
    S = _pro_data(shape)
    y, w = S['y'], S['w']
    gi = gi if mode == 'ghost' else N
    G = N // gi
    disp = do.dispatch(N, C, H, W, s, groups=G)
    if shape[0] == 96 and mode != 'ghost':
        assert disp['loop'] and disp['fwd_stride'] % 256 != 0
    if shape[0] == 128:
        assert disp['DH'] == 2 and (disp['straddle'] == 2) == (mode == 'ghost')
    pro = dict(gamma=S['gamma'], beta=S['beta'], act=act, eps=1e-5)
    if mode == 'running':
        pro.update(rmean=S['rmean'], rvar=S['rvar'])
        ref = do.bn_ref(y, S['gamma'], S['beta'], act, rmean=S['rmean'], rvar=S['rvar'])
    else:
        yg = y.to(F64).view(G, gi * H * W, C)
        stats = torch.stack([yg.sum(1), (yg * yg).sum(1)], 1).to(F32)      # what the kernel gets
        pro.update(stats=stats.reshape(-1), count=gi * H * W, group_imgs=gi)
        ref = do.bn_ref(y, S['gamma'], S['beta'], act, stats=stats, count=gi * H * W,
                        group_imgs=gi)
    a_ref, ysc, sh = ref
    kbuf, keep = guarded(N * H * W * C, BF16, NAN)
    obuf, out = guarded(N * P * Q * C, BF16, NAN, 64 + Q * C)
    sbuf, st = guarded(G * 2 * C, F32, 0.0)
    group_rows = gi * P * Q if G > 1 else 0
    ops.dwconv_fwd(y.reshape(-1), w.reshape(-1), out, N, H, W, C, P, Q, s, 1, stats=st,
                   group_rows=group_rows, pro=dict(pro, keep=keep))
    for buf, view, what in ((kbuf, keep, 'keep'), (obuf, out, 'y'), (sbuf, st, 'stats')):
        intact(buf, view, what)
    # the kept activation: one bf16 rounding of the fp32 y * sc + sh
    assert not bool(torch.isnan(keep).any()), 'an input pixel was not written to keep'
    k4 = keep.view(N, H, W, C).to(F64)
    r = bf16_criterion('pro-keep', (shape, mode, act), k4, a_ref, 1e-5 * (ysc + sh))
    assert r <= 1.0, 'keep off by %.3g of its bound' % r
    # the conv of exactly that activation: nine fp32 products and additions, one bf16 rounding
    cref = do.dw_ref(k4, w, None, s)[0]
    mag = do.dw_ref(k4.abs(), w.abs(), None, s)[0]
    o4 = out.view(N, P, Q, C).to(F64)
    r = bf16_criterion('pro-conv', (shape, mode, act), o4, cref, 16 * do.U * mag)
    assert r <= 1.0, 'conv output off by %.3g of its bound' % r
    # the statistics of the bf16 output the kernel wrote
    og = o4.view(G, gi * P * Q, C)
    sref = torch.stack([og.sum(1), (og * og).sum(1)], 1)
    smag = torch.stack([og.abs().sum(1), (og * og).sum(1)], 1)
    r = record('pro-stats', (shape, mode, act),
               ratio((st.view(G, 2, C).to(F64) - sref).abs(), disp['fwd_chain'] * do.U * smag))
    assert r <= 1.0, 'output statistics off by %.3g of their bound (K = %d)' % (
        r, disp['fwd_chain'])
    # without keep (same launch otherwise): the same output bits
    obuf2, out2 = guarded(N * P * Q * C, BF16, NAN, 64 + Q * C)
    ops.dwconv_fwd(y.reshape(-1), w.reshape(-1), out2, N, H, W, C, P, Q, s, 1,
                   stats=torch.zeros_like(st), group_rows=group_rows, pro=pro)
    assert same_bits(out2, out), 'keep=None changed the output'
    intact(obuf2, out2, 'y (keep=None)')
