"""Native bidirectional LSTM cell front-end (``csrc/lstm.hip``).

One ``nn.LSTM(bidirectional=True, num_layers=1)`` layer, time-major ``x [T][B][F]``:

* the time-batched GEMMs stay on ``torch.matmul``: ``pre = x . W_ih^T + (b_ih + b_hh)`` for all
  T and both directions before the recurrence, and ``dW_ih``, ``dW_hh``, ``db``, ``dx`` after
  the backward recurrence;
* the sequential part runs in the HIP step kernels, one launch per time step with both
  directions in it (direction 1 walks t = T-1 .. 0).

Precision: every GEMM operand is bf16 (x, W_ih, W_hh, h, dG), every accumulation fp32.  ``pre``
is kept in **fp32** (the batched GEMMs take bf16 operands and give an fp32 result: products are
exact and only the summation order differs between devices); ``h`` is rounded to
bf16 once per step (it is the next step's MFMA operand), ``c`` stays fp32, the saved gates and
the pre-activation gradients ``dG`` are bf16.  ``emulate`` is the same arithmetic in plain torch
on any device and is what the kernels are compared with.

Lengths (``bilstm(x, lstm, lengths)``): with ``len_b = clamp(lengths[b], 0, T)`` frame ``(t, b)``
is valid iff ``t < len_b`` and the layer computes what pack / ``nn.LSTM`` / unpack computes, by
per-row masking -- no reordering, no packing, no host synchronisation.  A padded frame gets
``h = +0`` and ``c = 0`` in the forward and ``dG = 0`` and ``dc = 0`` in the backward, by a select,
so nothing in the padding of ``x`` or of the upstream gradient (NaN and Inf included) reaches a
result; the reverse direction of row b then starts at ``t = len_b - 1`` from the zeros stored at
``len_b``, and the batched GEMMs need no change because ``dG``, ``out`` and the bf16 copy of ``x``
are zero at padded frames.  Lengths given on the host (list, CPU tensor) also trim the launches to
``max(len_b)`` steps; device lengths run all T steps, and waves whose rows are all padded skip
their GEMM.  Both forms give the same bits.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _chk, lib, ptr, stream_ptr
from .attention import _chk_lengths, _lengths_tensor

# (B, H) pairs at which bench/lstm_bench.py measured the native cell not slower than nn.LSTM in
# bf16, forward alone and forward + backward, on both layer widths (T = 161; F = 101 and 1024;
# profiles/r8/lstm/lstm_bench.jsonl: 0.17-0.56 of MIOpen's time); MyLSTM(cell='auto') takes the
# native cell exactly there.
MEASURED_NATIVE = frozenset({(32, 512), (320, 512)})
# The same with lengths, against bf16 nn.LSTM with pack / unpack, on both layer widths and both
# length distributions of bench/lstm_bench.py --lengths (all T; uniform in [T/2, T]);
# MyLSTM(packed=True, cell='auto') takes the native cell with lengths exactly there.  Empty: that
# comparison has no recorded run yet (the step kernels alone: profiles/r13/lstm_lengths/).
MEASURED_NATIVE_PACKED = frozenset()

_PARAMS = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0',
           'weight_ih_l0_reverse', 'weight_hh_l0_reverse', 'bias_ih_l0_reverse',
           'bias_hh_l0_reverse')


def check_hidden(H):
    """The step kernels tile H by 32-deep MFMA chunks and 16-unit output tiles."""
    if H < 32 or H % 32 != 0:
        raise ValueError('native LSTM cell: hidden size %d is not a positive multiple of 32' % H)


def _chk_all(specs):
    # contiguity and alignment first, so a strided or offset view is named as such on any device;
    # the kernels read and write 16-byte vectors at offsets that are multiples of 16 bytes
    for t, _, name, _ in specs:
        if t is not None and not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        if t is not None and t.data_ptr() % 16:
            raise ValueError('%s must be 16-byte aligned' % name)
    for t, dtype, name, numel in specs:
        _chk(t, dtype, name, numel)


def _chk_geom(T, B, H, s0, s1):
    check_hidden(H)
    if B < 1 or T < 1:
        raise ValueError('native LSTM cell: B and T must be >= 1, got B=%d T=%d' % (B, T))
    if (B + 15) // 16 > 65535:
        raise ValueError('native LSTM cell: B=%d has more 16-row tiles than a grid dimension' % B)
    if not 0 <= s0 <= s1 <= T:
        raise ValueError('native LSTM cell: steps [%d, %d) outside [0, %d]' % (s0, s1, T))


def lstm_step_fwd(pre, whh, out, c, gates=None, h0=None, c0=None, *, T, B, H, s0=0, s1=None,
                  lengths=None):
    """Forward steps ``[s0, s1)`` (default: all T), one launch each.

    pre fp32 [T][2][B][4H]; whh bf16 [2][4H][H]; out bf16 [T][B][2H] (h_t lands at column
    dir*H and is the next step's h_prev); ``gates`` bf16 [T][2][B][4H] given = training: the
    post-activation gates are saved and ``c`` is fp32 [T][2][B][H]; else ``c`` is the running
    state [2][B][H].  ``h0`` bf16 / ``c0`` fp32 [2][B][H]: the state step 0 starts from (None =
    zero, no memset).  ``lengths`` int32 [B] on the device: row b is valid at ``t <
    clamp(lengths[b], 0, T)``; a padded frame gets ``h = +0`` in ``out`` and ``c = 0`` (the running
    c or ``c[t]``), its ``pre`` is not read and its ``gates`` are left as they are.  Not with
    ``h0`` / ``c0``."""
    s1 = T if s1 is None else s1
    _chk_geom(T, B, H, s0, s1)
    _chk_lengths(lengths, B)
    if lengths is not None and (h0 is not None or c0 is not None):
        raise ValueError('lstm_step_fwd: lengths together with h0 / c0 is not supported')
    train = gates is not None
    _chk_all(((pre, torch.float32, 'pre', T * 2 * B * 4 * H),
              (whh, torch.bfloat16, 'whh', 2 * 4 * H * H),
              (out, torch.bfloat16, 'out', T * B * 2 * H),
              (c, torch.float32, 'c', (T if train else 1) * 2 * B * H),
              (gates, torch.bfloat16, 'gates', T * 2 * B * 4 * H),
              (h0, torch.bfloat16, 'h0', 2 * B * H),
              (c0, torch.float32, 'c0', 2 * B * H)))
    for t, n in ((pre, 'pre'), (whh, 'whh'), (out, 'out'), (c, 'c')):
        if t is None:
            raise ValueError('lstm_step_fwd: %s is required' % n)
    lib().lstm_step_fwd(ptr(pre), ptr(whh), ptr(out), ptr(c), ptr(gates), ptr(h0), ptr(c0),
                        ptr(lengths), T, B, H, s0, s1, int(train), stream_ptr())


def lstm_step_bwd(dout, gates, c, whhT, dG, dc, *, T, B, H, s0=0, s1=None, lengths=None):
    """Backward steps ``[s0, s1)``: step s handles t = T-1-s (direction 0) and t = s (direction 1).

    dout fp32 [T][B][2H]; gates / c as the training forward saved them; whhT bf16 [2][H][4H];
    dG bf16 [T][2][B][4H] (written per step, the next step's GEMM operand); dc fp32 [2][B][H],
    dc_next in and dc_prev out.  Step 0 has no recurrent term and reads dc as zero; the forward
    it differentiates started from a zero state (no ``h0`` / ``c0``).  ``lengths`` as the
    forward's: a padded frame gets ``dG[t] = 0`` and ``dc = 0`` and reads neither ``dout`` nor
    ``gates``, so ``dc`` ends as zero in direction 1 for every row shorter than T."""
    s1 = T if s1 is None else s1
    _chk_geom(T, B, H, s0, s1)
    _chk_lengths(lengths, B)
    _chk_all(((dout, torch.float32, 'dout', T * B * 2 * H),
              (gates, torch.bfloat16, 'gates', T * 2 * B * 4 * H),
              (c, torch.float32, 'c', T * 2 * B * H),
              (whhT, torch.bfloat16, 'whhT', 2 * H * 4 * H),
              (dG, torch.bfloat16, 'dG', T * 2 * B * 4 * H),
              (dc, torch.float32, 'dc', 2 * B * H)))
    for t, n in ((dout, 'dout'), (gates, 'gates'), (c, 'c'), (whhT, 'whhT'), (dG, 'dG'),
                 (dc, 'dc')):
        if t is None:
            raise ValueError('lstm_step_bwd: %s is required' % n)
    lib().lstm_step_bwd(ptr(dout), ptr(gates), ptr(c), ptr(whhT), ptr(dG), ptr(dc), ptr(lengths),
                        T, B, H, s0, s1, stream_ptr())


def _pack(w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r):
    whh = torch.stack([w_hh, w_hh_r]).to(torch.bfloat16)
    return {'w_ih': torch.stack([w_ih, w_ih_r]).to(torch.bfloat16),     # [2][4H][F]
            'w_hh': whh,                                                # [2][4H][H]
            'w_hhT': whh.transpose(1, 2).contiguous(),                  # [2][H][4H]
            'b': torch.stack([b_ih + b_hh, b_ih_r + b_hh_r]).float()}   # [2][4H]


def _lstm_params(lstm):
    if not isinstance(lstm, torch.nn.LSTM):
        raise TypeError('expected an nn.LSTM, got %s' % type(lstm).__name__)
    if (not lstm.bidirectional or lstm.num_layers != 1 or not lstm.bias or lstm.batch_first
            or getattr(lstm, 'proj_size', 0)):
        raise ValueError('native LSTM cell: only nn.LSTM(bidirectional=True, num_layers=1, '
                         'bias=True, batch_first=False) without projection')
    return [getattr(lstm, n) for n in _PARAMS]


def pack_lstm(lstm):
    """The operands the kernels read, from the module's own fp32 parameters: ``w_ih``
    [2][4H][F], ``w_hh`` [2][4H][H] and its transpose ``w_hhT`` [2][H][4H] in bf16 (direction
    0 = forward, 1 = reverse; rows in torch's gate order i, f, g, o) and ``b`` = b_ih + b_hh
    fp32 [2][4H].  The state dict is not touched."""
    with torch.no_grad():
        return _pack(*_lstm_params(lstm))


def _f32mm(a, b):
    """a . b for 2-D bf16 operands with fp32 accumulation and an fp32 result: on the device the
    bf16 GEMM with an fp32 output, elsewhere the operands widened to fp32 (exact products,
    fp32 sums -- the same arithmetic up to the summation order)."""
    if a.is_cuda:
        return torch.mm(a, b, out_dtype=torch.float32)
    return torch.matmul(a.float(), b.float())


def _valid(lengths, T, device):
    """[T][B][1] bool, t < len_b."""
    return (torch.arange(T, device=device)[:, None] < lengths.clamp(0, T)[None, :])[:, :, None]


def _steps_fwd_torch(pre, whh, out, c, gates, T, B, H, lengths=None):
    w = whh.float()
    cur = [None, None]
    valid = None if lengths is None else _valid(lengths, T, pre.device)
    zero = torch.zeros((), dtype=torch.float32, device=pre.device)
    for s in range(T):
        for d in (0, 1):
            t, tp = (s, s - 1) if d == 0 else (T - 1 - s, T - s)
            g = pre[t, d]
            if s:
                g = g + torch.matmul(out[tp, :, d * H:(d + 1) * H].float(), w[d].t())
            i, f, gg, o = g.split(H, dim=1)
            i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
            ct = i * gg if cur[d] is None else f * cur[d] + i * gg
            ht = o * torch.tanh(ct)
            if valid is not None:       # a padded frame stores h = +0 and c = 0 (a select)
                ct, ht = torch.where(valid[t], ct, zero), torch.where(valid[t], ht, zero)
            cur[d] = ct
            out[t, :, d * H:(d + 1) * H] = ht.to(torch.bfloat16)
            if gates is not None:
                gates[t, d] = torch.cat([i, f, gg, o], dim=1).to(torch.bfloat16)
                c[t, d] = ct


def _steps_bwd_torch(dout, gates, c, whh, dG, T, B, H, lengths=None):
    w = whh.float()
    dcn = [None, None]
    valid = None if lengths is None else _valid(lengths, T, dout.device)
    zero = torch.zeros((), dtype=torch.float32, device=dout.device)
    for s in range(T):
        for d in (0, 1):
            t = T - 1 - s if d == 0 else s
            tn, tc = (t + 1, t - 1) if d == 0 else (t - 1, t + 1)
            dh = dout[t, :, d * H:(d + 1) * H]
            if s:
                dh = dh + torch.matmul(dG[tn, d].float(), w[d])
            i, f, gg, o = gates[t, d].float().split(H, dim=1)
            th = torch.tanh(c[t, d])
            dc = dh * o * (1 - th * th)
            if dcn[d] is not None:
                dc = dcn[d] + dc
            cp = c[tc, d] if s < T - 1 else torch.zeros_like(th)
            dg = torch.cat([dc * gg * i * (1 - i), dc * cp * f * (1 - f),
                            dc * i * (1 - gg * gg), dh * th * o * (1 - o)], dim=1)
            dcp = dc * f
            if valid is not None:       # a padded frame stores dG = 0 and dc = 0 (a select)
                dg, dcp = torch.where(valid[t], dg, zero), torch.where(valid[t], dcp, zero)
            dG[t, d] = dg.to(torch.bfloat16)
            dcn[d] = dcp


class BiLSTMFunction(torch.autograd.Function):
    """``out = BiLSTMFunction.apply(native, save, x, *params)``: x [T][B][F], the eight
    parameters of an ``nn.LSTM(bidirectional=True, num_layers=1)`` in ``_PARAMS`` order; out fp32
    [T][B][2H] (bf16-valued).  ``native``: the HIP step kernels (device tensors only); else the
    same steps in plain torch (``emulate``).  ``save``: the caller's grad mode -- ``forward``
    itself always runs with grad mode off, and ``needs_input_grad`` reports ``requires_grad``
    whatever the mode, so ``_apply`` passes ``torch.is_grad_enabled()``.  Without it, or when no
    input needs a gradient, the steps take the inference form: no gates, one running c.

    Two more arguments may follow the parameters: ``lengths`` (an int32 tensor [B] on x's device,
    non-differentiable) and ``steps`` (an int, ``max(len_b)`` where the host knows it, else T).
    The native steps then run as ``T = steps`` on the time-major prefixes and ``out`` / ``dG``
    beyond them are zero-filled; the batched GEMMs stay on all T frames."""

    @staticmethod
    def forward(ctx, native, save, x, *params):
        ctx.n_extra = len(params) - 8
        params, (lengths, Te) = params[:8], (params[8:] + (None, None))[:2]
        T, B, F = x.shape
        H = params[1].shape[1]
        pk = _pack(*params)
        save = bool(save) and any(ctx.needs_input_grad)
        dev = x.device
        xb = x.to(torch.bfloat16).contiguous()
        Te = T if lengths is None or Te is None else max(0, min(int(Te), T))
        if lengths is not None:
            # exact zeros in the padding of the bf16 copy: what x holds there (NaN, Inf) cannot
            # enter dW_ih, and pre at padded frames is never read
            xb = torch.where(_valid(lengths, T, dev), xb, torch.zeros((), dtype=xb.dtype, device=dev))
        pre = _f32mm(xb.view(T * B, F), pk['w_ih'].view(8 * H, F).t()) + pk['b'].view(1, 8 * H)
        pre = pre.view(T, B, 2, 4 * H).permute(0, 2, 1, 3).contiguous()     # [T][2][B][4H]
        out = torch.empty(T, B, 2 * H, dtype=torch.bfloat16, device=dev)
        gates = torch.empty(T, 2, B, 4 * H, dtype=torch.bfloat16, device=dev) if save else None
        c = torch.empty((T if save else 1), 2, B, H, dtype=torch.float32, device=dev)
        kw = {} if lengths is None else {'lengths': lengths}
        if native:
            if Te < T:
                out[Te:].zero_()
            if Te > 0:
                lstm_step_fwd(pre, pk['w_hh'], out, c, gates, T=Te, B=B, H=H, **kw)
        else:
            _steps_fwd_torch(pre, pk['w_hh'], out, c, gates, T, B, H, **kw)
        if save:
            ctx.native = native
            ctx.lengths, ctx.steps = lengths, Te
            ctx.x_dtype = x.dtype
            ctx.need_dx = ctx.needs_input_grad[2]
            ctx.save_for_backward(xb, pk['w_ih'], pk['w_hh'], pk['w_hhT'], out, gates, c)
        return out.float()

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        xb, w_ih, w_hh, w_hhT, out, gates, c = ctx.saved_tensors
        T, B, F = xb.shape
        H = w_hh.shape[2]
        dout = dout.float().contiguous()
        dG = torch.empty(T, 2, B, 4 * H, dtype=torch.bfloat16, device=xb.device)
        kw = {} if ctx.lengths is None else {'lengths': ctx.lengths}
        if ctx.native:
            Te = ctx.steps
            if Te < T:
                dG[Te:].zero_()
            if Te > 0:
                dc = torch.empty(2, B, H, dtype=torch.float32, device=xb.device)
                lstm_step_bwd(dout, gates, c, w_hhT, dG, dc, T=Te, B=B, H=H, **kw)
        else:
            _steps_bwd_torch(dout, gates, c, w_hh, dG, T, B, H, **kw)
        # the time-batched GEMMs: bf16 operands, fp32 accumulation
        x2 = xb.view(T * B, F)
        dx = None
        grads = []
        for d in (0, 1):
            g2 = dG[:, d].reshape(T * B, 4 * H)
            if ctx.need_dx:
                part = _f32mm(g2, w_ih[d])
                dx = part if dx is None else dx + part
            dw_ih = _f32mm(g2.t(), x2)
            db = g2.float().sum(0)
            if T > 1:
                # h_prev of step t: out[t-1] (forward direction), out[t+1] (reverse)
                gs, hs = (dG[1:, d], out[:-1, :, :H]) if d == 0 else (dG[:-1, d], out[1:, :, H:])
                dw_hh = _f32mm(gs.reshape(-1, 4 * H).t(), hs.reshape(-1, H))
            else:
                dw_hh = torch.zeros(4 * H, H, dtype=torch.float32, device=xb.device)
            grads += [dw_ih, dw_hh, db, db.clone()]
        if dx is not None:
            dx = dx.view(T, B, F).to(ctx.x_dtype)
        return (None, None, dx, *grads) + (None,) * ctx.n_extra


def _host_steps(lengths, T):
    """max(len_b) where it costs nothing (a list or a CPU tensor), else None."""
    if lengths is None or (torch.is_tensor(lengths) and lengths.is_cuda):
        return None
    if torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.is_floating_point() or lengths.dtype == torch.bool:
            return None                 # _lengths_tensor refuses it
        lengths = lengths.tolist()
    return max(0, min(max((int(v) for v in lengths), default=0), T))


def _apply(native, x, lstm, lengths=None):
    params = _lstm_params(lstm)
    if x.dim() != 3 or x.shape[2] != lstm.input_size:
        raise ValueError('expected x [T][B][%d], got %s' % (lstm.input_size, tuple(x.shape)))
    if lengths is None:
        return BiLSTMFunction.apply(native, torch.is_grad_enabled(), x, *params)
    T, B = x.shape[:2]
    steps = _host_steps(lengths, T)
    lengths = _lengths_tensor(lengths, B, x.device)
    return BiLSTMFunction.apply(native, torch.is_grad_enabled(), x, *params, lengths,
                                T if steps is None else steps)


def bilstm(x, lstm, lengths=None):
    """The layer's output [T][B][2H] through the HIP step kernels; differentiable in x and the
    module's parameters.  Refuses a CPU input or an unsupported hidden size (``ValueError``).
    ``lengths``: None, a list, a CPU tensor or a device tensor of B integers (no host sync for a
    device tensor; values are clamped to [0, T]): packed-sequence semantics, ``out`` and ``dx``
    exactly 0 at ``t >= len_b``.  Lengths known on the host also cut the launches to
    ``max(len_b)`` steps; the result has the same bits either way."""
    check_hidden(lstm.hidden_size)
    if not x.is_cuda or not lstm.weight_hh_l0.is_cuda:
        raise ValueError('native LSTM cell: x and the module must be on a HIP device')
    return _apply(True, x, lstm, lengths)


def emulate(x, lstm, lengths=None):
    """The arithmetic of ``bilstm`` in plain torch on any device (forward and, through
    autograd, the same hand-written backward): bf16 operands, fp32 accumulation, h rounded to
    bf16 per step, dG rounded to bf16; with ``lengths``, the same masking rules."""
    return _apply(False, x, lstm, lengths)
