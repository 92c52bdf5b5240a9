"""Classifier head front-end: avg-pool + FC + (IS-weighted) CE (``csrc/head.hip``)."""
from __future__ import annotations

import torch

from . import _chk, lib, ptr, stream_ptr

MODE = {'score': 0, 'train': 1, 'eval': 2}


SCORE = {'loss': 0, 'gradnorm': 1}


_ACT = {'none': 0, 'relu': 1, 'relu6': 2}


def _extras(who, mode, smooth, topk, classes, meters):
    """(smooth, topk) checked before anything touches the device: smoothing is the training
    loss's alone (a non-zero value in score or eval mode is refused, never ignored), top-k counts
    into meters[5]."""
    from ..utils.meters import check_label_smoothing, check_topk
    smooth = check_label_smoothing(smooth)
    topk = check_topk(topk, classes)
    if smooth != 0.0 and mode != 'train':
        raise ValueError('%s: label smoothing applies to train mode only (%s mode stays plain '
                         'cross-entropy)' % (who, mode))
    if topk and meters is not None and meters.numel() < 6:
        raise ValueError('%s: topk counts into meters[5]; meters has %d' % (who, meters.numel()))
    return smooth, topk


def head_fwd(act, w, b, label, B, HW, C, classes, mode, pooled=None, logits=None, dlogits=None,
             losses=None, isw=None, meters=None, score='loss', bn=None, smooth=0.0, topk=0):
    """``score``: what score mode writes into ``losses`` -- 'loss' (per-sample CE, the
    reference) or 'gradnorm' (exact per-sample gradient norm of the classifier layer).

    ``bn`` (scoring / eval): ``act`` is the last conv's raw output and the head pools
    act(bn(act) [+ res]) -- dict(gamma, beta, eps, act, res=None, and stats + count +
    group_imgs (ghost / batch statistics) or rmean + rvar (running)) -- instead of reading a
    block output that a bn_apply pass wrote.

    ``smooth`` (train mode only): ``F.cross_entropy``'s ``label_smoothing`` in [0, 1) -- dlogits
    and meters[0] are the smoothed loss's, ``losses`` stays plain CE.  ``topk`` = k >= 1 (train /
    eval): meters[5] counts the samples whose label ranks below k, the lower index winning a tie
    (k = 1 equals meters[2]).  Both are launch constants, so a captured launch replays them."""
    smooth, topk = _extras('head_fwd', mode, smooth, topk, classes, meters)
    if score == 'gradnorm' and logits is not None and pooled is None:
        raise ValueError('head_fwd: the gradnorm score over ready logits reads pooled[]')
    _chk(act, torch.bfloat16, 'act', B * HW * C)
    _chk(w, torch.float32, 'w', classes * C)
    _chk(label, torch.int32, 'label', B)
    bnargs = (0, 0, 0, 0, 0, 0, 0.0, 0.0, 1, 0)
    if bn is not None:
        if pooled is None:
            raise ValueError('head_fwd: the BN prologue writes pooled[]')
        if bn.get('res') is not None:
            _chk(bn['res'], torch.bfloat16, 'bn res', B * HW * C)
        st = bn.get('stats')
        bnargs = (ptr(bn.get('res')), ptr(st), ptr(bn.get('rmean')), ptr(bn.get('rvar')),
                  ptr(bn['gamma']), ptr(bn['beta']),
                  1.0 / float(bn['count']) if st is not None else 0.0, float(bn['eps']),
                  int(bn.get('group_imgs') or B), _ACT[bn['act']])
    lib().head_fwd(ptr(act), ptr(w), ptr(b), ptr(label), ptr(isw), ptr(pooled), ptr(logits),
                   ptr(dlogits), ptr(losses), ptr(meters), B, HW, C, classes, MODE[mode],
                   stream_ptr(), SCORE[score], *bnargs, smooth, topk)


def head_bwd(pooled, dlogits, w, dw, db, dact, B, HW, C, classes, bw=None):
    """Classifier-head backward.  ``bw`` (as conv_dgrad's): also reduce the BN-backward sums of
    the final BN whose activation the head read; returns True when it did (the per-sample
    path -- the wide GEMM path does not, and the caller then runs bn_bwd's reduce)."""
    from .conv import _bw_args
    _chk(dact, torch.bfloat16, 'dact', B * HW * C)
    return bool(lib().head_bwd(ptr(pooled), ptr(dlogits), ptr(w), ptr(dw), ptr(db), ptr(dact),
                               B, HW, C, classes, stream_ptr(), *_bw_args(bw, B * HW, C)))


def mlp_head_fwd(x, w1, b1, w2, b2, h1, logits, label, B, F, H1, classes, mode, isw=None,
                 dlogits=None, losses=None, meters=None, score='loss', splits=0, smooth=0.0,
                 topk=0):
    """Speech-VGG head (`pytorch_model.py:145-153`): h1 = x . W1^T + b1, logits = h1 . W2^T + b2,
    then log-softmax CE (loss / IS-weighted dlogits / meters / score) -- all HIP kernels.
    x: bf16 [B][F] (NHWC flatten), W1: bf16 [H1][F] in the same (H, W, C) column order.
    ``smooth`` / ``topk``: as ``head_fwd``'s."""
    smooth, topk = _extras('mlp_head_fwd', mode, smooth, topk, classes, meters)
    _chk(x, torch.bfloat16, 'x', B * F)
    _chk(w1, torch.bfloat16, 'w1', H1 * F)
    for t, n, k in ((b1, 'b1', H1), (w2, 'w2', classes * H1), (b2, 'b2', classes),
                    (h1, 'h1', B * H1), (logits, 'logits', B * classes)):
        _chk(t, torch.float32, n, k)
    _chk(label, torch.int32, 'label', B)
    if not splits:
        # split the 7680-deep fc1 reduction so ~256 blocks run (64 x 64 output tiles)
        tiles = -(-B // 64) * -(-H1 // 64)
        splits = max(1, min(-(-F // 64), 256 // max(tiles, 1)))
    lib().mlp_head_fwd(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(h1), ptr(logits),
                       ptr(label), ptr(isw), ptr(dlogits), ptr(losses), ptr(meters), B, F, H1,
                       classes, MODE[mode], SCORE[score], splits, stream_ptr(), smooth, topk)


def mlp_head_bwd(dlogits, h1, x, w1, w2, dh1, dw1, db1, dw2, db2, dx, B, F, H1, classes):
    """Gradients of the speech-VGG head: dW2, db2, dh1, db1, dW1 (engine [H1][F] layout) and the
    bf16 activation gradient dx [B][F]."""
    _chk(dx, torch.bfloat16, 'dx', B * F)
    _chk(dw1, torch.float32, 'dw1', H1 * F)
    _chk(dh1, torch.float32, 'dh1', B * H1)
    lib().mlp_head_bwd(ptr(dlogits), ptr(h1), ptr(x), ptr(w1), ptr(w2), ptr(dh1), ptr(dw1),
                       ptr(db1), ptr(dw2), ptr(db2), ptr(dx), B, F, H1, classes, stream_ptr())
