"""Native attention pooling over time front-end (``csrc/attn.hip``).

For a time-major ``x [T][B][D]``, a vector ``w [D]`` (``Attention.att_weights[0]``) and optional
``lengths [B]`` (``len_b = min(max(lengths[b], 0), T)``, T when None)::

    s[b,t]   = sum_d x[t,b,d] * w[d]
    r[b,t]   = max(s[b,t], 0)
    a[b,t]   = exp(r[b,t] - M_b) / sum_{u < len_b} exp(r[b,u] - M_b)   for t < len_b, else 0
    rep[b,d] = sum_{t < len_b} a[b,t] * x[t,b,d]

with ``M_b`` the largest valid ``r``.  A row of length 0 gives ``rep = 0`` and ``a = 0``.  This
is what ``models.lstm.Attention`` computes (softmax over all T, then mask and renormalise)
whenever the valid frames keep at least 1e-12 of the unmasked softmax mass -- below that the torch
module's ``clamp_min(1e-12)`` takes over and its result is no longer a normalised softmax.
Frames at ``t >= len_b`` are never read, so whatever they hold (inf, NaN) cannot reach a result.

Backward, given ``g = d rep``::

    da[b,t]   = g[b,:] . x[t,b,:]            c_b = g[b,:] . rep[b,:]   (= sum_t a da)
    ds[b,t]   = a[b,t] * (da[b,t] - c_b) * (s[b,t] > 0)
    dx[t,b,:] = a[b,t] * g[b,:] + ds[b,t] * w        (written as 0 for t >= len_b)
    dw[d]     = sum_{b,t} ds[b,t] * x[t,b,d]

The returned attentions are **not differentiable** here (``MyLSTM`` discards them): a caller that
differentiates through them keeps ``Attention(impl='torch')``.

``x`` is fp32 or bf16 and is addressed by its strides for t and b (the D row contiguous and
16-byte aligned): a contiguous ``[T][B][D]``, its ``transpose(0, 1)`` and the transposed view of a
contiguous ``[B][T][D]`` all run without a copy.  ``dx`` has x's dtype; everything else is fp32,
as is every accumulation.  No atomics: two runs are bit-equal.  ``emulate`` is the same
arithmetic in plain torch on any device.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _chk, lib, ptr, stream_ptr

# csrc/kernels.h: a wave walks ``share`` >= WAVE_FRAMES frames of one batch row, a block is
# BLOCK_WAVES waves and leaves one partial; T is cut into at most MAX_SPLITS shares, and only
# until B * shares reaches TARGET_WAVES
WAVE_FRAMES = 8
BLOCK_WAVES = 4
MAX_SPLITS = 32
TARGET_WAVES = 2048
MAX_D = 2048

# (B, T, D, dtype of x) at which bench/attn_bench.py measured the native path not slower than
# the eager Attention, forward alone and forward + backward (profiles/r11/attn/attn_bench.jsonl:
# 0.17-0.22 of the eager time); Attention(impl='auto') takes the native path exactly there.
# bf16 input was timed for the native op alone, so no bf16 key is listed.
MEASURED_NATIVE = frozenset({(32, 161, 1024, torch.float32), (320, 161, 1024, torch.float32)})


def split(T, B):
    """(share, nsb) as the launchers cut T: frames per wave, blocks (partials) per batch row."""
    want = min(max(-(-TARGET_WAVES // B), 1), MAX_SPLITS)
    share = max(-(-T // want), WAVE_FRAMES)
    ns = -(-T // share)
    return share, -(-ns // BLOCK_WAVES)


def check_width(D):
    """A lane holds whole 16-byte chunks of a row and the row is spread over 64 lanes."""
    if D < 64 or D % 64 != 0 or D > MAX_D:
        raise ValueError('native attention: width %d is not a multiple of 64 in [64, %d]'
                         % (D, MAX_D))


def _chk_rows(t, name, T, B, D, dtypes):
    """t [T][B][D] with any t / b strides: a device tensor of one of ``dtypes`` whose rows are
    contiguous and 16-byte aligned."""
    if t.dim() != 3 or tuple(t.shape) != (T, B, D):
        raise ValueError('%s: expected shape (%d, %d, %d), got %s' % (name, T, B, D, tuple(t.shape)))
    if t.dtype not in dtypes:
        raise TypeError('%s: expected %s, got %s' % (name, ' or '.join(map(str, dtypes)), t.dtype))
    # layout before device, so a strided or offset view is named as such on any device
    if t.stride(2) != 1:
        raise ValueError('%s: the last dimension must be contiguous' % name)
    per16 = 16 // t.element_size()
    if t.data_ptr() % 16 or t.stride(0) % per16 or t.stride(1) % per16:
        raise ValueError('%s: rows must be 16-byte aligned' % name)
    if not t.is_cuda:
        raise ValueError('%s must be a HIP device tensor' % name)


def _chk_flat(specs):
    for t, _, name, _ in specs:
        if t is not None and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16:
            raise ValueError('%s must be 16-byte aligned' % name)
    for t, dtype, name, numel in specs:
        if t is None:
            raise ValueError('%s is required' % name)
        _chk(t, dtype, name, numel)
        if t.numel() != numel:
            raise ValueError('%s: expected %d elements, got %d' % (name, numel, t.numel()))


def _geom(x):
    if x.dim() != 3:
        raise ValueError('x: expected [T][B][D], got shape %s' % (tuple(x.shape),))
    T, B, D = x.shape
    check_width(D)
    if T < 1 or B < 1:
        raise ValueError('native attention: B and T must be >= 1, got B=%d T=%d' % (B, T))
    if B > 65535:
        raise ValueError('native attention: B=%d exceeds a grid dimension' % B)
    if B * T > 2 ** 31 - 1:
        raise ValueError('native attention: B * T = %d exceeds a 32-bit index' % (B * T))
    return T, B, D


def _chk_lengths(lengths, B):
    if lengths is None:
        return
    if not lengths.is_cuda or lengths.dtype != torch.int32 or not lengths.is_contiguous():
        raise ValueError('lengths must be a contiguous int32 HIP device tensor')
    if lengths.numel() != B:
        raise ValueError('lengths: expected %d elements, got %d' % (B, lengths.numel()))


def fwd_ws_floats(T, B, D):
    return B * split(T, B)[1] * (D + 2)


def bwd_ws_floats(T, B, D):
    return B * split(T, B)[1] * D


def attn_pool_fwd(x, w, lengths, rep, attn, score, ws):
    """Two launches: x [T][B][D] fp32 / bf16 (strided in t and b); w fp32 [D]; lengths int32 [B]
    or None; rep fp32 [B][D], attn fp32 [B][T]; score fp32 [B][T] (the saved s) or None = the
    no-grad form, which does not write it; ws fp32, ``fwd_ws_floats`` elements."""
    T, B, D = _geom(x)
    _chk_rows(x, 'x', T, B, D, (torch.float32, torch.bfloat16))
    _chk_lengths(lengths, B)
    _chk_flat(((w, torch.float32, 'w', D), (rep, torch.float32, 'rep', B * D),
               (attn, torch.float32, 'attn', B * T)))
    if score is not None:
        _chk_flat(((score, torch.float32, 'score', B * T),))
    _chk(ws, torch.float32, 'ws', fwd_ws_floats(T, B, D))
    if ws is None:
        raise ValueError('ws is required')
    lib().attn_pool_fwd(ptr(x), ptr(w), ptr(lengths), ptr(rep), ptr(attn), ptr(score), ptr(ws),
                        ws.numel(), x.stride(0), x.stride(1), T, B, D,
                        int(x.dtype == torch.bfloat16), stream_ptr())


def attn_pool_bwd(x, w, g, rep, attn, score, lengths, dx, dw, ws):
    """Two launches: g fp32 [B][D]; rep / attn / score as the training forward left them; dx
    [T][B][D] in x's dtype (strided like x may be; every frame is written); dw fp32 [D]; ws
    fp32, ``bwd_ws_floats`` elements."""
    T, B, D = _geom(x)
    _chk_rows(x, 'x', T, B, D, (torch.float32, torch.bfloat16))
    _chk_rows(dx, 'dx', T, B, D, (x.dtype,))
    if not (dx.is_contiguous() or dx.transpose(0, 1).is_contiguous()):
        raise ValueError('dx must be a dense [T][B][D] or the transposed view of a dense [B][T][D]')
    _chk_lengths(lengths, B)
    _chk_flat(((w, torch.float32, 'w', D), (g, torch.float32, 'g', B * D),
               (rep, torch.float32, 'rep', B * D), (attn, torch.float32, 'attn', B * T),
               (score, torch.float32, 'score', B * T), (dw, torch.float32, 'dw', D)))
    _chk(ws, torch.float32, 'ws', bwd_ws_floats(T, B, D))
    if ws is None:
        raise ValueError('ws is required')
    lib().attn_pool_bwd(ptr(x), ptr(w), ptr(g), ptr(rep), ptr(attn), ptr(score), ptr(lengths),
                        ptr(dx), ptr(dw), ptr(ws), ws.numel(), x.stride(0), x.stride(1),
                        dx.stride(0), dx.stride(1), T, B, D,
                        int(x.dtype == torch.bfloat16), stream_ptr())


def _lengths_tensor(lengths, B, device):
    """None, or ``lengths`` (list, CPU tensor, device tensor) as an int32 tensor [B] on
    ``device``; the values are clamped where they are used, not here (no host sync)."""
    if lengths is None:
        return None
    if not torch.is_tensor(lengths):
        lengths = torch.tensor(list(lengths), dtype=torch.int32)
    if lengths.is_floating_point() or lengths.dtype == torch.bool:
        raise TypeError('lengths: expected integers, got %s' % lengths.dtype)
    if lengths.dim() != 1 or lengths.numel() != B:
        raise ValueError('lengths: expected shape (%d,), got %s' % (B, tuple(lengths.shape)))
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def _like_rows(x):
    """An uninitialised [T][B][D] in x's dtype, dense, with x's order of t and b in memory."""
    T, B, D = x.shape
    if x.stride(0) >= x.stride(1):
        return torch.empty(T, B, D, dtype=x.dtype, device=x.device)
    return torch.empty(B, T, D, dtype=x.dtype, device=x.device).transpose(0, 1)


def _valid(lengths, T, B, device):
    """[B][T] bool, t < len_b."""
    if lengths is None:
        return torch.ones(B, T, dtype=torch.bool, device=device)
    return torch.arange(T, device=device)[None, :] < lengths.clamp(0, T)[:, None]


def _fwd_torch(x, w, lengths):
    T, B, D = x.shape
    valid = _valid(lengths, T, B, x.device)                          # [B][T]
    xm = torch.where(valid.t()[:, :, None], x.float(), torch.zeros((), device=x.device))
    s = (xm * w).sum(-1).t()                                         # [B][T]
    r = torch.where(valid, s.clamp_min(0), torch.zeros_like(s))
    p = torch.where(valid, torch.exp(r - r.max(1, keepdim=True).values), torch.zeros_like(s))
    den = p.sum(1, keepdim=True)
    a = torch.where(den > 0, p / den, torch.zeros_like(p))
    rep = (xm * a.t()[:, :, None]).sum(0)
    return rep, a, torch.where(valid, s, torch.zeros_like(s))


def _bwd_torch(x, w, g, rep, a, s, lengths):
    T, B, D = x.shape
    valid = _valid(lengths, T, B, x.device)
    xm = torch.where(valid.t()[:, :, None], x.float(), torch.zeros((), device=x.device))
    da = (xm * g[None]).sum(-1).t()                                  # [B][T]
    c = (g * rep).sum(1, keepdim=True)
    ds = torch.where(valid & (s > 0), a * (da - c), torch.zeros_like(a))
    dx = a.t()[:, :, None] * g[None] + ds.t()[:, :, None] * w
    dx = torch.where(valid.t()[:, :, None], dx, torch.zeros((), device=x.device))
    dw = (ds.t()[:, :, None] * xm).sum((0, 1))
    return dx.to(x.dtype), dw


class AttnPoolFunction(torch.autograd.Function):
    """``rep, attn = AttnPoolFunction.apply(native, save, x, w, lengths)``: x [T][B][D] fp32 or
    bf16, w fp32 [D], lengths an int32 tensor [B] on x's device or None; rep fp32 [B][D], attn
    fp32 [B][T] (non-differentiable).  ``native``: the HIP kernels (device tensors only); else
    the same arithmetic in plain torch (``emulate``).  ``save``: the caller's grad mode, as for
    ``BiLSTMFunction``; without it, or when neither x nor w needs a gradient, the forward takes
    the inference form and saves no scores."""

    @staticmethod
    def forward(ctx, native, save, x, w, lengths):
        T, B, D = x.shape
        save = bool(save) and any(ctx.needs_input_grad)
        w = w.float().contiguous()
        if native:
            dev = x.device
            rep = torch.empty(B, D, dtype=torch.float32, device=dev)
            attn = torch.empty(B, T, dtype=torch.float32, device=dev)
            score = torch.empty(B, T, dtype=torch.float32, device=dev) if save else None
            ws = torch.empty(fwd_ws_floats(T, B, D), dtype=torch.float32, device=dev)
            attn_pool_fwd(x, w, lengths, rep, attn, score, ws)
        else:
            rep, attn, score = _fwd_torch(x, w, lengths)
        if save:
            ctx.native = native
            ctx.lengths = lengths
            ctx.save_for_backward(x, w, rep, attn, score)
        ctx.mark_non_differentiable(attn)
        return rep, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gattn):
        x, w, rep, attn, score = ctx.saved_tensors
        T, B, D = x.shape
        g = g.float().contiguous()
        if ctx.native:
            dx = _like_rows(x)
            dw = torch.empty(D, dtype=torch.float32, device=x.device)
            ws = torch.empty(bwd_ws_floats(T, B, D), dtype=torch.float32, device=x.device)
            attn_pool_bwd(x, w, g, rep, attn, score, ctx.lengths, dx, dw, ws)
        else:
            dx, dw = _bwd_torch(x, w, g, rep, attn, score, ctx.lengths)
        return None, None, dx, dw, None


def _apply(native, x, w, lengths):
    if x.dim() != 3:
        raise ValueError('x: expected [T][B][D], got shape %s' % (tuple(x.shape),))
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('x: expected torch.float32 or torch.bfloat16, got %s' % x.dtype)
    T, B, D = x.shape
    if w.numel() != D or w.dim() > 2:
        raise ValueError('w: expected %d elements, got shape %s' % (D, tuple(w.shape)))
    if w.device != x.device:
        raise ValueError('w must be on the device of x')
    lengths = _lengths_tensor(lengths, B, x.device)
    return AttnPoolFunction.apply(native, torch.is_grad_enabled(), x, w.reshape(D), lengths)


def attn_pool(x, w, lengths=None):
    """``(rep [B][D], attn [B][T])`` of a time-major x [T][B][D] through the HIP kernels;
    differentiable in x and w, not through attn.  ``lengths``: None, a list, a CPU tensor or a
    device tensor of B integers.  Refuses a CPU input, an unsupported width, and rows that are
    not contiguous and 16-byte aligned (``ValueError``) -- it never copies x."""
    T, B, D = _geom(x)
    _chk_rows(x, 'x', T, B, D, (torch.float32, torch.bfloat16))
    return _apply(True, x, w, lengths)


def emulate(x, w, lengths=None):
    """The arithmetic of ``attn_pool`` in plain torch on any device (forward and, through
    autograd, the same hand-written backward), fp32 throughout."""
    return _apply(False, x, w, lengths)
