"""Native classifier head of the speech LSTM front-end (``csrc/fc_head.hip``).

``MyLSTM``'s tail -- dropout, ``fc1 = Sequential(Linear(K, N), BatchNorm1d(N), ReLU())``, dropout,
``fc2 = Linear(N, C)`` -- as two forward and two backward launches.  With ``m0 [B][K]`` and
``m1 [B][N]`` the dropout keep-masks (uint8; a kept element counts ``scale = 1 / (1 - p)``; absent
in eval mode or at ``p = 0``)::

    zd     = bf16(z * m0)                    y = zd . bf16(W1)^T + b1              fp32 [B][N]
    mean, var (biased) over the B rows in training, the running pair in eval
    rstd   = rsqrt(var + eps)
    a2     = bf16(relu(gamma * (y - mean) * rstd + beta) * m1)
    logits = a2 . bf16(W2)^T + b2                                                  fp32 [B][C]

In training the running statistics are updated as ``nn.BatchNorm1d`` does (the module's momentum,
the unbiased variance ``var * B / (B - 1)``, ``num_batches_tracked += 1``) and B = 1 is a
``ValueError``; eval writes no buffer.  Backward, given ``d = dlogits``::

    da2 = bf16(d) . bf16(W2)        dh = da2 * m1 * (a2 > 0)        xhat = (y - mean) * rstd
    dbeta = sum_b dh                dgamma = sum_b dh * xhat
    dy  = gamma * rstd * (dh - dbeta / B - xhat * dgamma / B)       (eval: gamma * rstd * dh)
    db1 = sum_b dy                  dW1 = bf16(dy)^T . zd           dz = (bf16(dy) . bf16(W1)) * m0
    dW2 = bf16(d)^T . a2            db2 = sum_b d

Every GEMM operand is bf16 (round to nearest even), every sum and all BN arithmetic fp32; the
parameters stay the modules' own fp32 tensors.  No atomics: two runs are bit-equal.  The kernels
draw no random numbers: ``fc_head`` draws the masks with torch (one launch each), which are
torch's draws but not the draws ``nn.Dropout`` would make from the same generator state.

Supported: ``N % 16 == 0``, ``K % 32 == 0``, ``1 <= C <= 1024``, ``B <= 320``, contiguous fp32
HIP tensors; anything else is a ``ValueError`` that names the tensor.  ``emulate`` is the same
arithmetic in plain torch on any device.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import lib, ptr, stream_ptr

MAX_B = 320          # csrc/kernels.h FC_HEAD_MAX_B: 20 row tiles, the largest instantiation
MAX_C = 1024

# (B, W, classes) at which bench/fc_head_bench.py measured the native head not slower than the
# torch chain, forward alone and forward + backward (profiles/r23/fc_head/fc_head_bench.jsonl:
# 23.5 against 31.3 us and 94.7 against 101.9 us); MyLSTM(head='auto') takes it exactly there.
# (320, 2048, 35) was measured and lost (112 against 53 us, 717 against 178 us), so it is absent.
MEASURED_NATIVE = frozenset({(32, 2048, 35)})


def _need(t, dtype, name, shape):
    if not torch.is_tensor(t):
        raise ValueError('%s: expected a tensor, got %s' % (name, type(t).__name__))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s: expected shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    if t.dtype != dtype:
        raise ValueError('%s: expected %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    if not t.is_cuda:
        raise ValueError('%s must be a HIP device tensor' % name)


def _geom(z, w1, w2, train):
    if not torch.is_tensor(z) or z.dim() != 2:
        raise ValueError('z: expected a [B][K] tensor')
    if not torch.is_tensor(w1) or w1.dim() != 2 or not torch.is_tensor(w2) or w2.dim() != 2:
        raise ValueError('w1 / w2: expected [N][K] and [C][N] tensors')
    B, K = z.shape
    N, C = w1.shape[0], w2.shape[0]
    if N < 16 or N % 16:
        raise ValueError('w1: N = %d is not a positive multiple of 16' % N)
    if K < 32 or K % 32:
        raise ValueError('z: K = %d is not a positive multiple of 32' % K)
    if not 1 <= C <= MAX_C:
        raise ValueError('w2: classes = %d is not in [1, %d]' % (C, MAX_C))
    if not 1 <= B <= MAX_B:
        raise ValueError('z: B = %d is not in [1, %d]' % (B, MAX_B))
    if train and B < 2:
        raise ValueError('z: batch statistics need more than 1 row (got B = 1 in training mode)')
    return B, K, N, C


def _chk_masks(m0, m1, B, K, N):
    if m0 is not None:
        _need(m0, torch.uint8, 'm0', (B, K))
    if m1 is not None:
        _need(m1, torch.uint8, 'm1', (B, N))


def fc_head_fwd(z, m0, m1, scale, w1, b1, gamma, beta, run_mean, run_var, batches, w2, b2, eps,
                momentum, train, save=True):
    """Two launches.  z fp32 [B][K]; m0 / m1 uint8 keep-masks or None; w1 [N][K], b1 / gamma /
    beta [N], w2 [C][N], b2 [C] fp32; run_mean / run_var fp32 [N] (read in eval; updated in
    place in training, None = no update), batches int64 [] or None.  ``train``: batch statistics.
    Returns ``(logits, y, mean, rstd, a2)``: y is None without ``save`` (no backward follows)."""
    B, K, N, C = _geom(z, w1, w2, train)
    _need(z, torch.float32, 'z', (B, K))
    _chk_masks(m0, m1, B, K, N)
    for t, name, shape in ((w1, 'w1', (N, K)), (b1, 'b1', (N,)), (gamma, 'gamma', (N,)),
                           (beta, 'beta', (N,)), (w2, 'w2', (C, N)), (b2, 'b2', (C,))):
        _need(t, torch.float32, name, shape)
    if (run_mean is None) != (run_var is None):
        raise ValueError('run_mean and run_var come together')
    if run_mean is None and not train:
        raise ValueError('run_mean: the eval form needs the running statistics')
    if run_mean is not None:
        _need(run_mean, torch.float32, 'run_mean', (N,))
        _need(run_var, torch.float32, 'run_var', (N,))
    if batches is not None:
        _need(batches, torch.int64, 'batches', ())
    dev = z.device
    y = torch.empty(B, N, dtype=torch.float32, device=dev) if save else None
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    rstd = torch.empty(N, dtype=torch.float32, device=dev)
    a2 = torch.empty(B, N, dtype=torch.bfloat16, device=dev)
    logits = torch.empty(B, C, dtype=torch.float32, device=dev)
    lib().fc_head_fwd(ptr(z), ptr(m0), ptr(m1), ptr(w1), ptr(b1), ptr(gamma), ptr(beta),
                      ptr(run_mean), ptr(run_var), ptr(batches) if train else 0, ptr(w2), ptr(b2),
                      ptr(y), ptr(mean), ptr(rstd), ptr(a2), ptr(logits), B, K, N, C,
                      float(scale), float(eps), float(momentum), int(bool(train)), stream_ptr())
    return logits, y, mean, rstd, a2


def fc_head_bwd(dlogits, z, m0, m1, scale, w1, w2, gamma, y, mean, rstd, a2, train):
    """Two launches, from the tensors the saving forward returned.  Returns ``(dz, dW1, db1,
    dgamma, dbeta, dW2, db2, dy)``: fp32, and the bf16 ``dy [B][N]`` the first launch leaves for
    the second (dW1 and dz are formed from it)."""
    B, K, N, C = _geom(z, w1, w2, train)
    _need(dlogits, torch.float32, 'dlogits', (B, C))
    _need(z, torch.float32, 'z', (B, K))
    _chk_masks(m0, m1, B, K, N)
    for t, name, shape in ((w1, 'w1', (N, K)), (w2, 'w2', (C, N)), (gamma, 'gamma', (N,)),
                           (y, 'y', (B, N)), (mean, 'mean', (N,)), (rstd, 'rstd', (N,))):
        _need(t, torch.float32, name, shape)
    _need(a2, torch.bfloat16, 'a2', (B, N))
    dev = z.device

    def f32(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    dy = torch.empty(B, N, dtype=torch.bfloat16, device=dev)        # workspace between the kernels
    dz, dw1, db1, dgamma, dbeta, dw2, db2 = (f32(B, K), f32(N, K), f32(N), f32(N), f32(N),
                                              f32(C, N), f32(C))
    lib().fc_head_bwd(ptr(dlogits), ptr(z), ptr(m0), ptr(m1), ptr(w1), ptr(w2), ptr(gamma), ptr(y),
                      ptr(mean), ptr(rstd), ptr(a2), ptr(dy), ptr(dz), ptr(dw1), ptr(db1),
                      ptr(dgamma), ptr(dbeta), ptr(dw2), ptr(db2), B, K, N, C, float(scale),
                      int(bool(train)), stream_ptr())
    return dz, dw1, db1, dgamma, dbeta, dw2, db2, dy


def _rbf(x):
    return x.to(torch.bfloat16).float()


def _keep(m, scale):
    return None if m is None else m.float() * scale


def _fwd_torch(z, m0, m1, scale, w1, b1, gamma, beta, run_mean, run_var, batches, w2, b2, eps,
               momentum, train):
    B = z.shape[0]
    if train and B < 2:
        raise ValueError('z: batch statistics need more than 1 row (got B = 1 in training mode)')
    k0, k1 = _keep(m0, scale), _keep(m1, scale)
    zd = _rbf(z.float() if k0 is None else z.float() * k0)
    y = zd @ _rbf(w1).t() + b1
    if train:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        if run_mean is not None:
            run_mean.mul_(1 - momentum).add_(mean * momentum)
            run_var.mul_(1 - momentum).add_(var * (momentum * B / (B - 1)))
        if batches is not None:
            batches.add_(1)
    else:
        mean, var = run_mean.clone(), run_var
    rstd = torch.rsqrt(var + eps)
    h = torch.relu((y - mean) * (gamma * rstd) + beta)
    a2 = (h if k1 is None else h * k1).to(torch.bfloat16)
    return a2.float() @ _rbf(w2).t() + b2, y, mean, rstd, a2


def _bwd_torch(dlogits, z, m0, m1, scale, w1, w2, gamma, y, mean, rstd, a2, train):
    B = z.shape[0]
    k0, k1 = _keep(m0, scale), _keep(m1, scale)
    zd = _rbf(z.float() if k0 is None else z.float() * k0)
    d, a2f = _rbf(dlogits), a2.float()
    dh = d @ _rbf(w2) * (a2f > 0)
    if k1 is not None:
        dh = dh * k1
    xh = (y - mean) * rstd
    dbeta, dgamma = dh.sum(0), (dh * xh).sum(0)
    dy = gamma * rstd * (dh - dbeta / B - xh * (dgamma / B) if train else dh)
    dyb = _rbf(dy)
    dz = dyb @ _rbf(w1)
    if k0 is not None:
        dz = dz * k0
    return dz, dyb.t() @ zd, dy.sum(0), dgamma, dbeta, d.t() @ a2f, dlogits.sum(0), dyb


class FcHeadFunction(torch.autograd.Function):
    """``logits = FcHeadFunction.apply(native, save, train, scale, eps, momentum, z, m0, m1, w1,
    b1, gamma, beta, run_mean, run_var, batches, w2, b2)``; differentiable in z and the six
    parameters.  ``native``: the HIP kernels, else the same arithmetic in plain torch.  ``save``:
    the caller's grad mode, as for ``AttnPoolFunction``."""

    @staticmethod
    def forward(ctx, native, save, train, scale, eps, momentum, z, m0, m1, w1, b1, gamma, beta,
                run_mean, run_var, batches, w2, b2):
        save = bool(save) and any(ctx.needs_input_grad)
        if native:
            logits, y, mean, rstd, a2 = fc_head_fwd(z, m0, m1, scale, w1, b1, gamma, beta,
                                                    run_mean, run_var, batches, w2, b2, eps,
                                                    momentum, train, save)
        else:
            logits, y, mean, rstd, a2 = _fwd_torch(z, m0, m1, scale, w1, b1, gamma, beta,
                                                   run_mean, run_var, batches, w2, b2, eps,
                                                   momentum, train)
        if save:
            ctx.cfg = (native, train, scale)
            ctx.save_for_backward(z, m0, m1, w1, w2, gamma, y, mean, rstd, a2)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        native, train, scale = ctx.cfg
        z, m0, m1, w1, w2, gamma, y, mean, rstd, a2 = ctx.saved_tensors
        bwd = fc_head_bwd if native else _bwd_torch
        dz, dw1, db1, dgamma, dbeta, dw2, db2, _ = bwd(g.float().contiguous(), z, m0, m1, scale,
                                                       w1, w2, gamma, y, mean, rstd, a2, train)
        return (None,) * 6 + (dz, None, None, dw1, db1, dgamma, dbeta, None, None, None, dw2, db2)


def draw_masks(B, K, N, p, device):
    """Two uint8 keep-masks, P(keep) = 1 - p: one bernoulli launch each."""
    return (torch.empty(B, K, dtype=torch.uint8, device=device).bernoulli_(1 - p),
            torch.empty(B, N, dtype=torch.uint8, device=device).bernoulli_(1 - p))


def _apply(native, z, fc1, fc2, p, training, masks):
    lin, bn = fc1[0], fc1[1]
    if not (isinstance(lin, torch.nn.Linear) and isinstance(bn, torch.nn.BatchNorm1d)
            and isinstance(fc1[2], torch.nn.ReLU) and len(fc1) == 3):
        raise ValueError('fc1: expected Sequential(Linear, BatchNorm1d, ReLU)')
    if lin.bias is None or fc2.bias is None or not bn.affine:
        raise ValueError('fc1 / fc2: the head needs both biases and an affine BatchNorm1d')
    if not 0 <= p < 1:
        raise ValueError('p: dropout probability must be in [0, 1), got %r' % (p,))
    train = bool(training) or bn.running_mean is None
    if train and bn.running_mean is not None and bn.momentum is None:
        raise ValueError('fc1: BatchNorm1d(momentum=None) (cumulative average) is not supported')
    if native:
        _geom(z, lin.weight, fc2.weight, train)
    m0 = m1 = None
    if masks is not None:
        m0, m1 = masks
    elif training and p > 0:
        m0, m1 = draw_masks(z.shape[0], lin.in_features, lin.out_features, p, z.device)
    scale = 1.0 / (1.0 - p) if m0 is not None or m1 is not None else 1.0
    run = bool(training) and bn.running_mean is not None      # nn.BatchNorm1d updates them
    return FcHeadFunction.apply(
        native, torch.is_grad_enabled(), train, scale, bn.eps, bn.momentum or 0.0, z, m0, m1,
        lin.weight, lin.bias, bn.weight, bn.bias,
        bn.running_mean if (run or not train) else None,
        bn.running_var if (run or not train) else None,
        bn.num_batches_tracked if run else None, fc2.weight, fc2.bias)


def fc_head(z, fc1, fc2, p, training, masks=None):
    """``fc2(dropout(fc1(dropout(z))))`` through the HIP kernels: ``fc1`` the
    ``Sequential(Linear, BatchNorm1d, ReLU)``, ``fc2`` the ``Linear``, ``p`` the dropout
    probability, ``training`` the modules' mode.  ``masks``: ``(m0 [B][K], m1 [B][N])`` uint8
    keep-masks; drawn with torch when ``training and p > 0`` and none are given.  Refuses
    (``ValueError``) a CPU tensor, an unsupported shape, a wrong dtype and B = 1 in training."""
    if not torch.is_tensor(z) or not z.is_cuda:
        raise ValueError('z must be a HIP device tensor')
    return _apply(True, z, fc1, fc2, p, training, masks)


def emulate(z, fc1, fc2, p, training, masks=None):
    """The arithmetic of ``fc_head`` in plain torch on any device (forward and, through autograd,
    the same hand-written backward): bf16-rounded operands, fp32 sums."""
    return _apply(False, z, fc1, fc2, p, training, masks)
