"""Every forward dispatch of the classifier head (csrc/head.hip), its BN-applying pool, its
backward paths and the speech-VGG head, each held to the fp64 references of ``kernel_oracles``
(not only to each other).

``head_fwd_launch`` dispatches three ways: the per-sample kernel (``logits=None``), the class-
chunk kernel (``logits`` given, classes >= 64: MobileNetV2 / CIFAR-100's 100 x 1280, whose last
chunk holds 4 classes), and pool + split-R GEMM (classes * C >= 2^20, ``pooled`` and ``logits``
given, C % 16 == 0).  A case runs on every dispatch that can reach it.

Tolerances: ``pooled`` / ``logits`` by ``assert_within`` (fp32 form, mag = sum |w h| + |b|);
with T_b sample b's largest logit tolerance, losses get 2 T_b + 1e-5 max(1, |lse|) and dlogits
scale_b (p (2 T_b + 1e-5) + 1e-7).

Largest measured |err| / mag on an MI355X, against k = 1e-5:
    pooled (per-sample, chunk, pool kernel)        1.0e-7
    pooled (head_pool_bn_kernel)                   2.2e-6
    logits: chunk 8.0e-8, wide (split-R) 7.7e-8
    head_bwd: dw 2.8e-7, db 1.3e-7, dact 2.0e-8
    MLP head: h1 8.8e-8, logits 1.5e-8, dw2 3.4e-7, db2 1.3e-7, dh1 4.0e-7, db1 1.3e-7,
              dw1 2.5e-7, dx 5.3e-9
and as a fraction of their own tolerance: losses 0.0024, gradnorm 0.0045, dlogits 0.46 (the
1e-7 floor against the fast exp of a small probability).
"""
import functools

import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


@functools.lru_cache(maxsize=None)
def _case(B, HW, C, K, wscale=1.0, tie=None):
    """Inputs and the fp64 reference of one head shape (computed once, never modified)."""
    act, w, b, label, isw = ko.head_case(B, HW, C, K, wscale, tie, DEV)
    ref = ko.head_ref(act, w, b, label, isw)
    return dict(B=B, HW=HW, C=C, K=K, act=act, w=w, b=b, label=label, isw=isw, ref=ref)


def _fwd(c, path, mode, score='loss', pooled_buf=True):
    """One head_fwd launch on ``path`` ('sample' | 'chunk' | 'wide'), every output checked."""
    ops = _ops()
    B, HW, C, K, r = c['B'], c['HW'], c['C'], c['K'], c['ref']
    wide_size = K * C >= 1 << 20
    if path == 'sample':
        pass                                # logits=None always takes the per-sample kernel
    elif path == 'chunk':
        assert K >= 64 and (not wide_size or C % 16 or not pooled_buf)
    else:
        assert wide_size and C % 16 == 0 and pooled_buf
    pooled = torch.full((B, C), NAN, device=DEV) if pooled_buf else None
    logits = None if path == 'sample' else torch.full((B, K), NAN, device=DEV)
    dlog = torch.full((B, K), NAN, device=DEV)
    losses = torch.full((B,), NAN, device=DEV)
    meters = torch.zeros(8, device=DEV)
    ops.head_fwd(c['act'], c['w'], c['b'], c['label'], B, HW, C, K, mode, pooled=pooled,
                 logits=logits, dlogits=dlog, losses=losses, isw=c['isw'], meters=meters,
                 score=score)
    tag = 'head %s %s/%s B=%d HW=%d C=%d K=%d ' % (path, mode, score, B, HW, C, K)
    if pooled is not None:
        ko.record('head_pool', ko.assert_within(pooled, r['pooled'], r['pooled_mag'],
                                                what=tag + 'pooled'))
    if logits is not None:
        ko.record('head_logits_' + path, ko.assert_within(logits, r['logits'], r['logits_mag'],
                                                          what=tag + 'logits'))
    assert torch.isfinite(losses).all(), tag + 'losses not finite'
    if score == 'gradnorm':
        ko.record('head_gradnorm/tol', ko.assert_tol(losses, r['gradnorm'], r['gradnorm_tol'],
                                                     tag + 'gradnorm'))
    else:
        ko.record('head_losses/tol', ko.assert_tol(losses, r['losses'], r['losses_tol'],
                                                   tag + 'losses'))
    m = meters.cpu().tolist()
    if mode == 'score':
        assert m == [0.0] * 8, tag + 'score mode touches no meter'
    else:
        if mode == 'train':
            want, tol = r['meter0_train']
        else:
            # isw is passed in every mode: eval must ignore it (an eval meter of loss / w fails)
            want, tol = r['meter0_eval']
            assert abs(r['meter0_train'][0] - want) > 10 * (tol + r['meter0_train'][1]) or B == 1
        assert abs(m[0] - want) <= tol, tag + 'meters[0] %r want %r tol %g' % (m[0], want, tol)
        assert m[1] == B, tag + 'meters[1]'
        assert r['correct'][0] <= m[2] <= r['correct'][1], tag + 'meters[2] %r %r' % (m[2], r['correct'])
        assert m[3:] == [0.0] * 5
    if mode == 'train':
        ko.record('head_dlogits/tol', ko.assert_tol(dlog, r['dlogits'], r['dlogits_tol'],
                                                    tag + 'dlogits'))
    else:
        assert torch.isnan(dlog).all(), tag + 'dlogits written outside train mode'
    return m


def _all_modes(c, path, pooled_buf=True):
    _fwd(c, path, 'train', pooled_buf=pooled_buf)
    _fwd(c, path, 'eval', pooled_buf=pooled_buf)
    _fwd(c, path, 'score', pooled_buf=pooled_buf)
    if pooled_buf or path == 'sample':       # gradnorm over ready logits reads pooled[]
        _fwd(c, path, 'score', 'gradnorm', pooled_buf=pooled_buf)


@pytest.mark.parametrize('B,HW,C,K,ws', ko.HEAD_SAMPLE_CASES)
def test_head_per_sample_path(B, HW, C, K, ws):
    c = _case(B, HW, C, K)
    _all_modes(c, 'sample')
    _fwd(c, 'sample', 'train', pooled_buf=False)


@pytest.mark.parametrize('B,HW,C,K,ws', ko.HEAD_CHUNK_CASES)
def test_head_chunk_path(B, HW, C, K, ws):
    """100 = 6 * 16 + 4 and 65 = 4 * 16 + 1: short last chunks; 1008 x 1048 is wide-sized but
    C % 16 != 0 sends it here.  One case passes no pooled[] (score = 'loss' only)."""
    c = _case(B, HW, C, K)
    pooled_buf = K != 65
    _all_modes(c, 'chunk', pooled_buf)
    _all_modes(c, 'sample')                  # the same reference through the other dispatch


@pytest.mark.parametrize('B,HW,C,K,ws', ko.HEAD_WIDE_CASES)
def test_head_wide_path(B, HW, C, K, ws):
    """1000 x 1056 at B = 5: four split-R slices of 320 channels, the last one 96 = 64 + 32 (it
    ends inside a 64-deep step); at B = 70 two row tiles, the second with 6 live rows."""
    c = _case(B, HW, C, K)
    _all_modes(c, 'wide')
    _fwd(c, 'chunk', 'train', pooled_buf=False)     # no pooled[]: the chunk kernel
    _fwd(c, 'sample', 'train')


def test_head_logit_range_needs_max_subtraction():
    """Every sample's logits span more than 100: exp() of an unshifted logit overflows fp32."""
    c = _case(*ko.HEAD_RANGE_CASE)
    lg = c['ref']['logits']
    assert float((lg.max(1).values - lg.min(1).values).min()) > 100 and float(lg.max()) > 89
    for path in ('sample', 'chunk'):
        _fwd(c, path, 'train')
        _fwd(c, path, 'score', 'gradnorm')


@pytest.mark.parametrize('tie', ko.HEAD_TIES)
def test_head_argmax_tie_first_maximum_wins(tie):
    """Rows 3 and 77 (another lane and chunk) or 3 and 67 (the same lane's second class) are
    identical and largest; the label is the later one, so no sample counts as correct."""
    c = _case(5, 16, 1280, 100, tie=tie)
    assert (c['ref']['argmax'] == tie[0]).all() and c['ref']['correct'] == (0, 0)
    for path in ('sample', 'chunk'):
        assert _fwd(c, path, 'eval')[2] == 0.0
        assert _fwd(c, path, 'train')[2] == 0.0


# ------------------------------------------------------------------------------ BN pool
@pytest.mark.parametrize('HW,C', ko.HEAD_POOL_BN_CASES)
def test_head_pool_bn(HW, C):
    """head_pool_bn_kernel: B = 12 in ghost groups of 4 images, every activation, with and
    without the identity residual, from ghost sums and from running statistics."""
    ops = _ops()
    B, gi, K = 12, 4, 10
    x3, gamma, beta, stats, res, rm, rv, w, b, label = ko.head_pool_bn_case(HW, C, DEV)
    for act in ('none', 'relu', 'relu6'):
        for r in (None, res):
            for running in (False, True):
                bn = dict(gamma=gamma, beta=beta, eps=1e-5, act=act, res=r)
                if running:
                    bn.update(rmean=rm, rvar=rv)
                else:
                    bn.update(stats=stats, count=gi * HW, group_imgs=gi)
                pooled = torch.full((B, C), NAN, device=DEV)
                losses = torch.full((B,), NAN, device=DEV)
                ops.head_fwd(x3, w, b, label, B, HW, C, K, 'score', pooled=pooled, losses=losses,
                             bn=bn)
                ref, mag = ko.head_pool_bn_ref(x3, r, stats, gamma, beta, gi * HW, gi, act, 1e-5,
                                               (rm, rv) if running else None)
                tag = 'head_pool_bn %s res=%s running=%s HW=%d C=%d' % (act, r is not None, running,
                                                                        HW, C)
                ko.record('head_pool_bn', ko.assert_within(pooled, ref, mag, what=tag))
                # the FC and the loss then run on that pooled[]
                hr = ko.head_ref(None, w, b, label, pooled=ref, logits_mag=mag @ w.double().abs().t()
                                 + b.double().abs())
                ko.assert_tol(losses, hr['losses'], hr['losses_tol'], tag + ' losses')


# ------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('B,HW,C,K,gemm', ko.HEAD_BWD_CASES)
def test_head_bwd_paths(B, HW, C, K, gemm):
    """The per-sample kernel (also at a wide size whose classes % 4 != 0 sends it back) and the
    three-GEMM path."""
    ops = _ops()
    assert gemm == (K * C >= 1 << 20 and K % 4 == 0 and C % 4 == 0)
    pooled, dlog, w = ko.head_bwd_case(B, C, K, DEV)
    dw = torch.full((K, C), NAN, device=DEV)
    db = torch.full((K,), NAN, device=DEV)
    dact = torch.full((B, HW, C), NAN, dtype=torch.bfloat16, device=DEV)
    assert ops.head_bwd(pooled, dlog, w, dw, db, dact, B, HW, C, K) is False
    r = ko.head_bwd_ref(pooled, dlog, w, HW)
    tag = 'head_bwd %s B=%d HW=%d C=%d K=%d ' % ('gemm' if gemm else 'sample', B, HW, C, K)
    ko.record('head_bwd_dw', ko.assert_within(dw, r['dw'], r['dw_mag'], what=tag + 'dw'))
    ko.record('head_bwd_db', ko.assert_within(db, r['db'], r['db_mag'], what=tag + 'db'))
    ko.record('head_bwd_dact', ko.assert_within(
        dact, r['dact'][:, None].expand(B, HW, C).contiguous(),
        r['dact_mag'][:, None].expand(B, HW, C).contiguous(), what=tag + 'dact'))


# ------------------------------------------------------------------------------ speech-VGG head
@pytest.mark.parametrize('splits', [1, 3, 0])
@pytest.mark.parametrize('B', ko.MLP_BATCHES)
def test_mlp_head_fwd_bwd(B, splits):
    """F = 200 (3 full 64-deep steps + 8), H1 = 72 (a second, 8-wide column tile), K = 30:
    every head_gemm_kernel instantiation of the MLP head, bf16 operands included."""
    ops = _ops()
    F, H1, K = ko.MLP_DIMS
    x, w1, b1, w2, b2, label, isw = ko.mlp_case(B, DEV)
    h1 = torch.full((B, H1), NAN, device=DEV)
    logits = torch.full((B, K), NAN, device=DEV)
    dlog = torch.full((B, K), NAN, device=DEV)
    losses = torch.full((B,), NAN, device=DEV)
    meters = torch.zeros(8, device=DEV)
    ops.mlp_head_fwd(x, w1, b1, w2, b2, h1, logits, label, B, F, H1, K, 'train', isw=isw,
                     dlogits=dlog, losses=losses, meters=meters, splits=splits)
    f = ko.mlp_fwd_ref(x, w1, b1, w2, b2)
    tag = 'mlp_head B=%d splits=%d ' % (B, splits)
    ko.record('mlp_h1', ko.assert_within(h1, f['h1'], f['h1_mag'], what=tag + 'h1'))
    ko.record('mlp_logits', ko.assert_within(logits, f['logits'], f['logits_mag'], what=tag + 'logits'))
    r = ko.head_ref(None, w2, b2, label, isw, pooled=f['h1'], logits_mag=f['logits_mag'])
    ko.assert_tol(losses, r['losses'], r['losses_tol'], tag + 'losses')
    ko.assert_tol(dlog, r['dlogits'], r['dlogits_tol'], tag + 'dlogits')
    m = meters.cpu().tolist()
    assert abs(m[0] - r['meter0_train'][0]) <= r['meter0_train'][1] and m[1] == B
    assert r['correct'][0] <= m[2] <= r['correct'][1]
    # backward from the buffers the forward left (fp32 inputs of the backward kernels)
    dh1 = torch.full((B, H1), NAN, device=DEV)
    dw1 = torch.full((H1, F), NAN, device=DEV)
    db1 = torch.full((H1,), NAN, device=DEV)
    dw2 = torch.full((K, H1), NAN, device=DEV)
    db2 = torch.full((K,), NAN, device=DEV)
    dx = torch.full((B, F), NAN, dtype=torch.bfloat16, device=DEV)
    ops.mlp_head_bwd(dlog, h1, x, w1, w2, dh1, dw1, db1, dw2, db2, dx, B, F, H1, K)
    q = ko.mlp_bwd_ref(dlog, h1, x, w1, w2)
    for name, out in (('dw2', dw2), ('db2', db2), ('dh1', dh1), ('db1', db1), ('dw1', dw1),
                      ('dx', dx)):
        ko.record('mlp_' + name, ko.assert_within(out, q[name], q[name + '_mag'], what=tag + name))
