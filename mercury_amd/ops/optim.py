"""Fused flat-buffer optimizer front-end (``csrc/optim.hip``).

``FlatOptimizer`` owns fp32 ``p``/``g``/``m``/``v`` flat buffers (4-element
aligned segments), a device segment table describing which segments are conv
weights (and where their bf16 MFMA operand copies live), and a device
hyper-parameter vector ``[lr, beta1, beta2, eps, weight_decay, clip max_norm,
grad norm, clip coefficient]``.  ``step`` is one launch; ``clip`` (global-norm
gradient clipping, off by default) is the norm pass in front of it; ``set_lr``
is a 4-byte host->device copy done outside graphs (the cosine schedule changes
lr once per epoch).
"""
from __future__ import annotations


import torch

from . import lib, ptr, stream_ptr

# kernel algorithm codes (csrc/kernels.h OptArgs.algo)
ALGOS = {'adam': 0, 'sgd': 1, 'adamw': 2}

# ---------------------------------------------------------------- gradient norm
# Mirror of csrc/grad_norm_plan.h (the launch arithmetic of grad_norm_launch): 256 threads, each
# GN_U float4 loads per grid-stride trip, at most GN_CAP blocks.
GN_NT, GN_U, GN_CAP = 256, 2, 1024
GN_BLOCK_SPAN = GN_NT * GN_U * 4          # floats one block reads per trip
GN_GRID_SPAN = GN_CAP * GN_BLOCK_SPAN     # floats the capped grid reads per trip
GN_WS_FLOATS = GN_CAP                     # workspace: one fp32 partial per block
GN_EPS = 1e-6                             # torch.nn.utils.clip_grad_norm_'s epsilon


def grad_norm_plan(n):
    """Launch arithmetic of the norm pass over ``n`` floats, as the launcher computes it.

    ``n4`` whole float4s go through the grid-stride loop, the ``tail`` = n % 4 floats to block
    0's thread 0.  ``chain`` is the longest per-thread run of fp32 accumulations (one rounding
    each: 4 per float4, GN_U float4s per trip, plus the tail), ``depth`` the additions on the
    longest path from a thread's partial to the total: 6 shuffle levels + 3 wave sums in the
    block, then (fp64) 3 in-thread + 6 shuffle levels + 3 wave sums over the block partials.
    The relative error of the sum of squares is at most (chain + depth) * 2**-24 (every term is
    non-negative, so the sum is perfectly conditioned); the square root halves it and adds its
    own rounding and the fp64 -> fp32 one."""
    n = int(n)
    if n < 1:
        raise ValueError('grad_norm: n must be >= 1')
    n4, tail = n // 4, n % 4
    per_block = GN_NT * GN_U
    blocks = min(max((n4 + per_block - 1) // per_block, 1), GN_CAP)
    span = blocks * per_block
    trips = (n4 + span - 1) // span
    return dict(n=n, n4=n4, tail=tail, blocks=blocks, trips=trips,
                chain=trips * GN_U * 4 + tail, depth=(6 + 3) + (3 + 6 + 3))


def grad_norm_ranges(n):
    """Every float range [lo, hi) the launch reads, per (trip, block, u) row plus the tail --
    what the kernel's index arithmetic gives; the tests check they tile [0, n) exactly once."""
    pl = grad_norm_plan(n)
    out = []
    stride = pl['blocks'] * GN_NT * GN_U
    for b in range(pl['blocks']):
        base = b * GN_NT * GN_U
        while base < pl['n4']:
            for u in range(GN_U):
                lo = base + u * GN_NT
                hi = min(lo + GN_NT, pl['n4'])
                if hi > lo:
                    out.append((4 * lo, 4 * hi))
            base += stride
    if pl['tail']:
        out.append((4 * pl['n4'], n))
    return out


def grad_norm_edge_sizes():
    """The sizes at which the launch takes another path: a tail only (no float4), one float4
    with and without a tail, one block's span - 1 / + 0 / + 1, the capped grid's one-trip
    span + 4 (a second, ragged grid-stride trip) and an n % 4 == 3 size just past twice that
    span (a third trip and a tail).  The tests run these."""
    b, g = GN_BLOCK_SPAN, GN_GRID_SPAN
    return [1, 3, 4, 5, b - 1, b, b + 1, g + 4, 2 * g + 7]


def check_max_norm(max_norm):
    """0 / None: clipping off (returns 0.0); negative or NaN: ValueError; inf is allowed (the
    norm is computed, the coefficient is 1)."""
    if max_norm is None:
        return 0.0
    c = float(max_norm)
    if c != c or c < 0.0:
        raise ValueError('clip_grad_norm must be >= 0 (0 = off), got %r' % (max_norm,))
    return c


def grad_norm(g, max_norm, record, ws):
    """L2 norm of the contiguous fp32 device tensor ``g`` and torch's clip coefficient
    ``min(1, max_norm / (norm + 1e-6))`` into ``record[0:2]``; ``max_norm`` is a 1-element
    device tensor (read at run time: a graph replay sees its current value), ``ws`` a
    workspace of at least ``GN_WS_FLOATS`` floats.  Two launches on the current stream, no
    allocation, no sync; bit-equal from run to run."""
    from . import _chk
    _chk(g, torch.float32, 'g', 1)
    _chk(max_norm, torch.float32, 'max_norm', 1)
    _chk(record, torch.float32, 'record', 2)
    _chk(ws, torch.float32, 'ws', grad_norm_plan(g.numel())['blocks'])
    lib().grad_norm(ptr(g), g.numel(), ptr(max_norm), ptr(record), ptr(ws), ws.numel(),
                    stream_ptr())
    return record


def optimizer_spec(optimizer):
    """Map a ``torch.optim`` instance onto the fused kernel, or raise ``ValueError``.

    Only exact types are accepted (``AdamW`` subclasses ``Adam`` in torch 2.x, so an
    ``isinstance`` test would silently run it with coupled L2 decay), with one param group and
    no option the kernel does not implement.  Returns the ``FlatOptimizer`` keyword arguments."""
    groups = optimizer.param_groups
    if len(groups) != 1:
        raise ValueError('native optimizer: exactly one param group supported, got %d'
                         % len(groups))
    g = groups[0]
    t = type(optimizer)
    if g.get('maximize', False):
        raise ValueError('native optimizer: maximize=True is not supported')
    if g.get('differentiable', False):
        raise ValueError('native optimizer: differentiable=True is not supported')
    if t is torch.optim.Adam or t is torch.optim.AdamW:
        if g.get('amsgrad', False):
            raise ValueError('native optimizer: amsgrad=True is not supported')
        algo = 'adamw' if (t is torch.optim.AdamW or g.get('decoupled_weight_decay', False)) \
            else 'adam'
        lr = g['lr']
        if torch.is_tensor(lr):
            lr = float(lr)
        return dict(algo=algo, lr=lr, betas=tuple(g['betas']), eps=g['eps'],
                    weight_decay=g['weight_decay'], momentum=0.9)
    if t is torch.optim.SGD:
        if g.get('nesterov', False):
            raise ValueError('native optimizer: nesterov=True is not supported')
        if g.get('dampening', 0) != 0:
            raise ValueError('native optimizer: dampening != 0 is not supported')
        if g.get('momentum', 0) == 0:
            raise ValueError('native optimizer: SGD without momentum is not supported '
                             '(the kernel keeps a momentum buffer)')
        return dict(algo='sgd', lr=g['lr'], betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=g['weight_decay'], momentum=g['momentum'])
    raise ValueError('native optimizer: %s is not supported (Adam, AdamW, SGD with momentum)'
                     % t.__name__)


class FlatOptimizer(object):

    def __init__(self, segments, total, device, algo='adam', lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, momentum=0.9, fused=True, clip_grad_norm=0.0):
        clip = check_max_norm(clip_grad_norm)      # (before anything touches the device)
        self.device = torch.device(device)
        self.total = int(total)
        self.segments = segments
        self.p = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.g = torch.zeros_like(self.p)
        self.m = torch.zeros_like(self.p)
        if algo not in ALGOS:
            raise ValueError('FlatOptimizer algo must be one of %s, got %r' % (sorted(ALGOS), algo))
        adam = algo in ('adam', 'adamw')
        self.v = torch.zeros_like(self.p) if adam else torch.zeros(4, device=device)
        self.algo = ALGOS[algo]
        b1 = betas[0] if adam else momentum
        # [5] clip max_norm, [6] the last step's gradient norm, [7] its clip coefficient (the
        # norm pass writes [6:8], the optimizer kernels read [7] when clipping is on)
        self.hyper = torch.tensor([lr, b1, betas[1], eps, weight_decay, clip, 0, 1],
                                  dtype=torch.float32, device=device)
        self.clip_on = clip > 0.0
        self.gn_ws = torch.zeros(GN_WS_FLOATS, dtype=torch.float32, device=device) \
            if self.clip_on else None
        rows = []
        for s in segments:
            rows.append([s['off'], s['numel'], s['kind'], s.get('K', 0), s.get('R', 1),
                         s.get('S', 1), s.get('C', 1), s.get('Cpad', 1),
                         ptr(s.get('w_krsc')), ptr(s.get('w_crsk'))])
        self._seg_starts = set(int(s['off']) for s in segments)
        packed = lib().pack_opt_segs(rows)
        self.segbuf = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(device)
        self.nsegs = len(rows)
        # 64x64 transpose tiles producing the dgrad ([C][R][S][K]) weight copies
        jobs = []
        for i, s in enumerate(segments):
            if s['kind'] == 1 and s.get('w_crsk') is not None:
                for rs in range(s['R'] * s['S']):
                    for k0 in range(0, s['K'], 64):
                        for c0 in range(0, s['C'], 64):
                            jobs.append((i, rs, k0, c0))
        self.njobs = len(jobs)
        # jobs are ordered by segment, hence by flat offset: a range's jobs are a slice
        self._job_off = [segments[j[0]]['off'] for j in jobs]
        self.jobs = torch.tensor(jobs if jobs else [(0, 0, 0, 0)], dtype=torch.int32,
                                 device=device).contiguous()
        # fused full step (csrc/optim.hip optimizer_fused_kernel): 64x64 update tiles for conv
        # segments that carry a dgrad copy (their [C][R][S][K] copy is written from the update),
        # float4 elementwise ranges for everything else
        fjobs, ew = [], []
        for i, s in enumerate(segments):
            if s['kind'] == 1 and s.get('w_crsk') is not None and s['C'] % 4 == 0:
                for rs in range(s['R'] * s['S']):
                    for k0 in range(0, s['K'], 64):
                        for c0 in range(0, s['C'], 64):
                            fjobs.append((i, rs, k0, c0))
            else:
                ew.append((int(s['off']), (int(s['numel']) + 3) // 4 * 4))
        pre = [0]
        for _, n in ew:
            pre.append(pre[-1] + n // 4)
        self.fused = bool(fused)        # EngineOptions.fused_opt
        self.n_fjobs = len(fjobs)
        self.fjobs = torch.tensor(fjobs if fjobs else [(0, 0, 0, 0)], dtype=torch.int32,
                                  device=device).contiguous()
        self.ew = torch.tensor(ew if ew else [(0, 0)], dtype=torch.int64, device=device)
        self.ewp = torch.tensor(pre, dtype=torch.int64, device=device)
        self.n_ew, self.ew4 = len(ew), pre[-1]
        # dgrad copies of conv segments the tiles do not cover still go through the transpose
        fused_segs = set(j[0] for j in fjobs)
        rest = [j for j in jobs if j[0] not in fused_segs]
        self.n_rest = len(rest)
        self.rest_jobs = torch.tensor(rest if rest else [(0, 0, 0, 0)], dtype=torch.int32,
                                      device=device).contiguous()

    def _transpose(self, start=0, end=None):
        end = self.total if end is None else end
        j0 = next((i for i, o in enumerate(self._job_off) if o >= start), self.njobs)
        j1 = next((i for i, o in enumerate(self._job_off) if o >= end), self.njobs)
        if j1 > j0:
            lib().transpose_weights(ptr(self.segbuf), ptr(self.jobs) + 16 * j0, j1 - j0,
                                    stream_ptr())

    @property
    def lr(self):
        return float(self.hyper[0].item())

    def set_lr(self, lr):
        self.hyper[0].fill_(float(lr))

    def set_clip(self, max_norm):
        """New clipping threshold; a 4-byte device write, valid between graph replays (the norm
        pass reads it from device memory).  Only on an optimizer built with clipping on: the
        captured step of one built without it has no norm launch to turn on."""
        c = check_max_norm(max_norm)
        if not self.clip_on:
            raise ValueError('set_clip: this FlatOptimizer was built with clip_grad_norm off')
        if c == 0.0:
            raise ValueError('set_clip: 0 would zero every gradient; use float("inf") to '
                             'stop clipping on an optimizer built with it')
        self.hyper[5].fill_(c)

    def clip(self):
        """Launch the norm pass over g[0, total): hyper[6] = ||g||_2, hyper[7] = the clip
        coefficient the next ``step`` multiplies the gradient by.  Call it once the whole
        gradient is final (after the last all-reduce), before the first range step."""
        if not self.clip_on:
            raise ValueError('clip: this FlatOptimizer was built with clip_grad_norm off')
        lib().grad_norm(ptr(self.g), self.total, ptr(self.hyper) + 20, ptr(self.hyper) + 24,
                        ptr(self.gn_ws), self.gn_ws.numel(), stream_ptr())

    def last_grad_norm(self):
        """The gradient norm the last ``clip`` recorded (before clipping).  A host sync: for
        log cadence only."""
        return float(self.hyper[6].item())

    def step(self, step_counter, zero_grad=True, start=0, end=None):
        """``step_counter``: device int64 scalar tensor/view holding t (already incremented).
        ``start``/``end``: update only the flat range [start, end) -- both must be segment
        starts (or ``total``); two range steps equal one full step.  With clipping on, the
        gradient is multiplied by the coefficient of the last ``clip`` before weight decay."""
        end = self.total if end is None else end
        gscale = ptr(self.hyper) + 28 if self.clip_on else 0
        for b in (start, end):
            if b != self.total and b not in self._seg_starts:
                raise ValueError('optimizer range bound %d is not a segment start' % b)
        if self.fused and start == 0 and end == self.total:
            lib().optimizer_fused(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v),
                                  ptr(self.segbuf), self.nsegs, self.total, ptr(self.hyper),
                                  ptr(step_counter), self.algo, int(zero_grad), ptr(self.fjobs),
                                  self.n_fjobs, ptr(self.ew), ptr(self.ewp), self.n_ew, self.ew4,
                                  stream_ptr(), gscale)
            if self.n_rest:
                lib().transpose_weights(ptr(self.segbuf), ptr(self.rest_jobs), self.n_rest,
                                        stream_ptr())
            return
        lib().optimizer(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), ptr(self.segbuf),
                        self.nsegs, end, ptr(self.hyper), ptr(step_counter), self.algo,
                        int(zero_grad), stream_ptr(), start, gscale)
        self._transpose(start, end)

    def pack_weights(self):
        """Write the bf16 conv-weight copies from the fp32 master (after init / load)."""
        lib().pack_weights(ptr(self.p), ptr(self.segbuf), self.nsegs, self.total, stream_ptr())
        self._transpose()
