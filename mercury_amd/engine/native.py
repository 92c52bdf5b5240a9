"""The MI355X-native training engine: fused HIP kernels + HIP graphs + RCCL.

One importance-sampled step (reference `pytorch_collab.py:127-164`) runs as:

    S1 (score stream)  : pool_build -> forward(B=320, ghost BN) -> CE scores
                         -> is_sample (EMA replay, p, draws, weights)
    S0 (main stream)   : forward(B=32) -> IS-weighted CE -> backward, segmented
                         at gradient-bucket boundaries; after each segment the
                         bucket's RCCL all-reduce (AVG) is issued on the NCCL
                         stream while later segments and S1 keep computing
    S0 after join      : BN running stats (train batch, then the 10 scoring
                         groups, in reference order) -> fused Adam (+bf16
                         weight packing, gradient zeroing) -> gather the drawn
                         samples into the next training batch

Scoring uses the same (pre-update) weights as training, exactly like the
reference, so it overlaps the whole train fwd/bwd and the all-reduce instead
of serialising after them (the reference's dead overlap code,
`pytorch_collab.py:154-156`, made real without the race).  Each stream's work
is captured once into HIP graphs (``torch.cuda.CUDAGraph``) and replayed, so
a step costs a handful of host calls.  All buffers are allocated up front.
"""
from __future__ import annotations

import dataclasses
import gc
import math
import time
import weakref

import numpy as np
import torch
import torch.distributed as dist

from .. import ops
from ..data.augment import PHOTO_PARAMS, SPEC_PARAMS, SpecRecipe
from ..ops import hconv, tune
from ..ops.conv import cpad8, slab_bytes
from ..parallel.buckets import default_bucket_bytes
from . import schedule

_RELEASE = []    # (hipGraphExec_t, [hipEvent_t]) of un-closed collected engines


_HWQ_WARNED = []
LIVE = weakref.WeakSet()   # open engines of this process (close_all: test / program teardown)


def close_all():
    """Close every open engine of this process (deterministic teardown)."""
    for e in list(LIVE):
        e.close()


def _warn_hw_queues():
    """Once per process: the step's three streams need >= 16 hardware queues, set before HIP
    starts (mercury_amd/__init__.py); say so when that did not happen."""
    import warnings
    from .. import HW_QUEUES
    if HW_QUEUES['effective'] or _HWQ_WARNED:
        return
    _HWQ_WARNED.append(1)
    warnings.warn('mercury_amd: the HIP runtime started with GPU_MAX_HW_QUEUES=%s (< 16): the '
                  'scoring / train / comm streams can share hardware queues and the step runs '
                  'serially (~1.6x slower).  Import mercury_amd (or export GPU_MAX_HW_QUEUES=16) '
                  'before anything initialises the GPU.' % (HW_QUEUES['before'] or 'default 4'),
                  RuntimeWarning, stacklevel=3)


def _release_queued():
    """Destroy what collected (never closed) engines queued -- caller has synchronised."""
    while _RELEASE:
        ex, evs = _RELEASE.pop()
        if ex:
            ops.lib().graph_exec_destroy(ex)
        for e in evs:
            ops.lib().ext_event_destroy(e)


from ..trainer import Trainer
from ..utils import profiling as prof
from ..utils.meters import Accuracy, Average, EMAverage
from .lower import lower, supports  # noqa: F401

BN_EPS = 1e-5


class _Mode(object):
    """Per-batch-size buffers (activations, stats, slabs), plans and launch schedules."""

    def __init__(self, name, mp, lw, opts):
        self.name = name
        self.mp = mp                     # schedule.ModePlan (``spec`` / ``plan`` are its dicts)
        self.lw, self.opts = lw, opts
        self.N = mp.N
        self.group_imgs = mp.group_imgs  # images per BN stat group (0 = whole batch)
        self.train = mp.train
        self.spec = mp.spec
        self.plan = mp.plan
        self.buf = {}
        self.stats = {}
        self.slab = None
        self.G = mp.G
        self.head_bn = None
        self.head_reduced = False        # the head's backward reduced the last BN's sums
        self.dw_region = {}              # depthwise unit -> (slab offset, floats, wgrad blocks)
        self.dw_pending = []             # deferred depthwise wgrad reduces of this backward

    def resolve(self):
        """(Re-)resolve the launch schedules from the plans as they stand: at mode build, and
        again whenever a plan changed (ops/step_tune.py) or graphs are captured, so that a
        schedule never describes plans that are gone.  A dual forward pair whose plans both
        split K gets the shortcut's slab here (never from inside ``forward``)."""
        schedule.apply_globals(self.opts)
        self.fwd_steps = schedule.forward_schedule(self.lw, self.mp, self.opts)
        self.bwd = schedule.backward_schedule(self.lw, self.mp, self.opts) if self.train \
            else None
        for s in self.fwd_steps:
            pa, pb = self.plan.get((s.unit, 'fwd')), self.plan.get((s.unit2, 'fwd'))
            if s.op == 'dual_conv' and pa[2] > 1 and pb[2] > 1:
                # the shortcut's split-K partials and tile counters get a slab of their own
                sp = self.spec[s.unit2]
                need = (slab_bytes(sp.M, sp.K, *pb[:3]) + 3) // 4
                if (s.unit2, 'slab') not in self.buf or self.buf[s.unit2, 'slab'].numel() < need:
                    self.buf[s.unit2, 'slab'] = torch.zeros(need, dtype=torch.float32,
                                                            device=self.slab.device)


class NativeEngine(object):

    def __init__(self, net, device, batch_size=32, pool_batches=10, num_classes=None,
                 image_hw=(32, 32), optimizer='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, momentum=0.9, seed=0, alpha=0.5, ema_alpha=0.9,
                 importance=True, world_size=1, bucket_bytes=None, use_graphs=True,
                 sampler='alias', exchange_scores=False, global_table=True, score='loss',
                 global_ema=False, autotune=None, force_buckets=False, comm='auto',
                 wire_bf16=False, debug=False, check_order=False, grad_compress=None,
                 opts=None, augment=None, eval_augment=None, clip_grad_norm=0.0,
                 label_smoothing=0.0, topk=0):
        self.clip_grad_norm = ops.optim.check_max_norm(clip_grad_norm)
        from ..utils.meters import check_label_smoothing, check_topk
        # the train head's label smoothing (scoring and evaluation stay plain CE) and the k of
        # the top-k hit count of the train and eval heads (meters[5]; 0 = off)
        self.label_smoothing = check_label_smoothing(label_smoothing)
        self.topk = check_topk(topk)
        self.eval_topk = (0, 0)          # (top-k hits, count) of the last evaluate_arrays call
        ops.lib()
        _warn_hw_queues()
        from ..config import EngineOptions
        self.opts = opts if opts is not None else EngineOptions.from_env()
        if autotune is not None:
            tune.enable(autotune)
        self.net = net
        self.device = torch.device(device)
        self.lw = lower(net)
        self.B = batch_size
        self.P = batch_size * pool_batches
        self.pool_batches = pool_batches
        self.classes = self.lw.num_classes
        check_topk(self.topk, self.classes)
        self.H, self.W = image_hw
        # augmentation recipes (data/augment.py) of the pool builds and of evaluate_arrays;
        # None: RandomCrop(pad 4) + flip + CIFAR Normalize on a shard of the input size, and
        # plain Normalize for evaluation
        self.augment = self._recipe(augment)
        self.eval_augment = self._recipe(eval_augment)
        if isinstance(self.eval_augment, SpecRecipe):
            raise ValueError('eval_augment: a SpecRecipe augments training pools only')
        self.aug_params = None           # [P][8] fp32: the last pool's draws (set_shard);
        #                                  [P][12] for a SpecRecipe, [P][16] with rrc / jitter
        self.seed = seed
        self.alpha, self.ema_alpha, self.importance = alpha, ema_alpha, importance
        self.world_size = world_size
        self.use_graphs = use_graphs and not debug
        self.debug = debug
        # data-parallel gradient path.  ``force_buckets`` runs the real bucketed all-reduces
        # even at W = 1 (the one-GPU box exercises the RCCL code path; AVG over one rank is the
        # identity, so results are bit-identical to the unbucketed step)
        self.dp = world_size > 1 or (force_buckets and dist.is_initialized())
        self._avg_op = None
        self.comm = None                 # own RCCL communicator (csrc/comm.hip)
        self.s_comm = None               # ... and the stream its bucket all-reduces run on
        rp = self.opts.role_prio
        self._role_prio = (-1 if self.dp else 0) if rp == 'auto' else int(rp)
        self.wire_bf16 = wire_bf16
        if self.dp:
            nccl = dist.get_backend() == 'nccl'
            self._avg_op = dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM
            if comm == 'auto':
                comm = 'rccl' if nccl else 'pg'
            if comm in ('rccl', 'xgmi'):
                from ..parallel.rccl import RcclComm
                self.comm = RcclComm.shared()
                self.s_comm = ops.role_stream(self.device, 'comm', self._role_prio)
            elif comm != 'pg':
                raise ValueError("comm must be 'auto', 'rccl', 'xgmi' or 'pg'")
        self.comm_kind = comm if self.dp else None
        self.xgmi = None                 # direct-xGMI two-shot all-reduce (parallel/xgmi.py)
        if grad_compress not in (None, 'none', 'ternary'):
            raise ValueError("grad_compress must be None, 'none' or 'ternary'")
        if grad_compress == 'ternary' and (wire_bf16 or comm == 'xgmi'):
            raise ValueError('grad_compress=ternary is its own wire format (no bf16 / xgmi)')
        self.grad_compress = grad_compress if grad_compress != 'none' else None
        self.tern = None                 # ternary-compressed all-reduce (parallel/compress.py)
        self._pg_works = []              # ProcessGroup works issued by the last step ('pg')
        self._closed = True              # (open once __init__ has finished: see its end)
        self._tern_ctr = 0
        # DP verification hook (tests): grad_probe(stage, i, t) sees bucket i's gradient slice as
        # the backward left it ('pre', on the stream that reduces it, before the collective) and
        # the whole flat gradient the optimizer will read ('post', i = None, on the train stream
        # before the tail).  Host-issued, so it sees every step, graphs or not.
        self.grad_probe = None
        self.bucket_bytes = bucket_bytes or default_bucket_bytes(world_size)
        # the last bucket (closed when the backward ends, so fully exposed) holds only the
        # leading blocks' parameters up to this many bytes (bucket_plan)
        self.last_bucket_bytes = int(self.opts.last_bucket_mb * (1 << 20))
        # measured all-reduce cost model (alpha, beta) and the plan derived from it: under DP on
        # the engine's RCCL communicator the bucket sizes come from timing the real collective
        # at start-up, not from an assumed link bandwidth (parallel/buckets.py)
        self.comm_calib = None
        cal = self.opts.bucket_calib
        if cal not in ('auto', 'on', 'off'):
            raise ValueError("EngineOptions.bucket_calib must be 'auto', 'on' or 'off'")
        if self.comm is not None and comm == 'rccl' and grad_compress in (None, 'none') and (
                cal == 'on' or (cal == 'auto' and bucket_bytes is None and
                                (self.comm.size > 1 or self.opts.rccl_one_rank))):
            from ..parallel.buckets import calibrate_allreduce, plan_from_calibration
            self.comm_calib = calibrate_allreduce(self.comm, self.device)
            bb, lb = plan_from_calibration(self.comm_calib)
            if bucket_bytes is None:
                self.bucket_bytes = bb
            self.last_bucket_bytes = lb
            self.comm_calib.update(bucket_bytes=self.bucket_bytes, last_bucket_bytes=lb)
        self.units = []
        for blk in self.lw.blocks:
            self.units += blk.units + ([blk.shortcut] if blk.shortcut else [])
        self.unit = {u.name: u for u in self.units}
        # conv bias (speech VGG) is added in the conv epilogue; under train-mode BN its gradient
        # is exactly zero (the batch mean absorbs it), so its grad segment is never written
        self._make_params(optimizer, lr, betas, eps, weight_decay, momentum)
        self.modes = {}
        self.ctrl = torch.zeros(8, dtype=torch.int64, device=self.device)
        self.ema = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.meters = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.eval_meters = torch.zeros(8, dtype=torch.float32, device=self.device)
        # (stream priorities, a CU-masked scoring stream, a weight-gradient side stream and an
        # early optimizer split were all measured neutral or slower on MI355X and removed:
        # profiles/ab_experiments_r1c.json)
        # the scoring and comm streams each own a hardware queue (ops.role_stream): a pooled
        # stream that lands on the train stream's queue serialises the step (1.37 -> 2.1 ms)
        self.s_score = ops.role_stream(self.device, 'score', self._role_prio)
        self.graphs = None
        self._bucket_evs = []            # event-record nodes of the one-graph DP replay
        self._train_exec = 0             # ... and that graph (hipGraphExec_t)
        self.shard = None
        self.primed = False              # a scored pool / drawn batch is pending
        self.scoring = True
        self.roctx = False               # per-phase roctx ranges around the step's host calls
        # (the kernel-path switches of config.EngineOptions -- defaults = the measured-best
        # paths, each with the A/B that keeps it -- are read by engine/schedule.py)
        self._apply_globals()

        if sampler not in ('alias', 'cdf', 'groupwise'):
            raise ValueError("sampler must be 'alias', 'cdf' or 'groupwise'")
        self.sampler = sampler
        if sampler == 'groupwise' and not global_table:
            raise ValueError("sampler='groupwise' draws from the global table (global_table=True)")
        if sampler == 'groupwise' and (exchange_scores or global_ema):
            raise ValueError("sampler='groupwise' has no pool EMA to share across ranks")
        if score not in ('loss', 'gradnorm'):
            raise ValueError('score must be loss or gradnorm')
        self.score = score
        self.global_table = global_table
        self.table = None
        self.score_exchange = None
        self.global_ema = global_ema
        if self.dp and (exchange_scores or global_ema):
            from ..parallel.scores import ScoreExchange
            # on an RCCL communicator of its own when the engine has one: stream-ordered on the
            # score stream, no ProcessGroup work in flight during a step or a capture, and not
            # queued in front of the gradient buckets (RCCL runs one communicator's operations
            # in issue order across streams, and the all-gather is issued first every step)
            xc = None
            if self.comm is not None:
                from ..parallel.rccl import RcclComm
                xc = RcclComm.shared(tag='score')
            self.score_exchange = ScoreExchange(self.P, self.device, force=world_size == 1,
                                                comm=xc)
        from .timing import StepTimer
        self.timer = StepTimer(self.device)   # per-phase device timing (off until enabled)
        self.wire = None
        # race detection: device-side stream-order assertions (csrc/runtime.hip);
        # debug mode also serialises the streams, runs eagerly and syncs after every phase
        self.check_order = check_order or debug
        self.order = torch.zeros(16, dtype=torch.int32, device=self.device)
        self.debug_log = self.opts.debug_log
        if self.comm_kind == 'xgmi':
            from ..parallel.xgmi import XgmiAllReduce
            cap = max(e - s_ for s_, e in self.bucket_plan().values())
            self.xgmi = XgmiAllReduce(cap, self.device, wire_bf16=wire_bf16)
        if self.dp and self.grad_compress == 'ternary':
            from ..parallel.compress import TernaryAllReduce
            cap = max(e - s_ for s_, e in self.bucket_plan().values())
            self.tern = TernaryAllReduce(cap, self.device, comm=self.comm, seed=seed)
        # registered for close_all() only once fully built: a constructor that raised leaves
        # nothing half-initialised for a later teardown to trip over
        self._closed = False
        LIVE.add(self)

    def _apply_globals(self):
        """The few EngineOptions that live in process-wide state (the halo-conv launcher's
        persistent grid / waves / plan overrides, the stride-2 dgrad switch) are re-applied by
        every phase of THIS engine that reads them -- plan building (set_shard / mode), eager
        launches and graph capture -- so engines with different options can share a process."""
        schedule.apply_globals(self.opts)
        hconv.configure_launcher()

    # ------------------------------------------------------------------ parameters
    def _final_chw(self):
        """(C, H, W) of the last block's output (speech VGG: 512 x 3 x 5 for 1x101x161)."""
        h, w = self.H, self.W
        for blk in self.lw.blocks:
            for u in blk.units:
                h = (h + 2 * u.pad - u.R) // u.stride + 1
                w = (w + 2 * u.pad - u.R) // u.stride + 1
            if blk.pool is not None:
                k, st, pd = blk.pool
                h = (h + 2 * pd - k) // st + 1
                w = (w + 2 * pd - k) // st + 1
        return self.lw.blocks[-1].units[-1].K, h, w

    def _make_params(self, optimizer, lr, betas, eps, wd, momentum):
        segs = []
        self.w_krsc, self.w_crsk = {}, {}
        # speech VGG: fc1's master weights live in [f1][H][W][C] order (the flatten order of the
        # NHWC activation), so fc1 is a plain GEMM on the activation rows; the optimizer writes
        # its bf16 copy like a conv weight's (torch's [f1][C][H][W] at the state-dict boundary)
        self.mlp_chw = None
        self.w1p = None
        if self.lw.head_pool == 'mlp2':
            c, h, w = self._final_chw()
            f1 = self.lw.fc1.out_features
            if c * h * w != self.lw.fc1.in_features:
                raise ValueError('fc1 expects %d inputs, the features give %d x %d x %d'
                                 % (self.lw.fc1.in_features, c, h, w))
            self.mlp_chw = (c, h, w)
            self.w1p = torch.zeros(f1, h, w, c, dtype=torch.bfloat16, device=self.device)
        for u in self.units:
            if u.depthwise:
                continue
            K, C, R = u.K, u.C, u.R
            self.w_krsc[u.name] = torch.zeros(K, R, R, cpad8(C), dtype=torch.bfloat16,
                                              device=self.device)
            if u.need_dgrad:
                self.w_crsk[u.name] = torch.zeros(C, R, R, K, dtype=torch.bfloat16,
                                                  device=self.device)
        unit_by_w = {id(u.w_seg): u for u in self.units}
        for s in self.lw.segs:
            d = dict(off=s.off, numel=s.numel, kind=0)
            u = unit_by_w.get(id(s))
            if u is not None and not u.depthwise:
                d.update(kind=1, K=u.K, R=u.R, S=u.R, C=u.C, Cpad=cpad8(u.C),
                         w_krsc=self.w_krsc[u.name], w_crsk=self.w_crsk.get(u.name))
            elif self.mlp_chw is not None and s is self.lw.fc1_w:
                c, h, w = self.mlp_chw
                d.update(kind=1, K=self.lw.fc1.out_features, R=h, S=w, C=c, Cpad=c,
                         w_krsc=self.w1p, w_crsk=None)
            segs.append(d)
        self.opt = ops.FlatOptimizer(segs, self.lw.total, self.device, optimizer, lr, betas, eps,
                                     wd, momentum, fused=self.opts.fused_opt,
                                     clip_grad_norm=self.clip_grad_norm)
        self.load_from_module()

    def _pview(self, seg, grad=False):
        buf = self.opt.g if grad else self.opt.p
        return buf[seg.off:seg.off + seg.numel]

    def _krsc_shape(self, seg):
        """[K][C][R][S] torch shape of a segment stored KRSC in the master, else None."""
        if seg.kind == 'conv':
            return tuple(seg.param.shape)
        if self.mlp_chw is not None and seg is self.lw.fc1_w:
            c, h, w = self.mlp_chw
            return (self.lw.fc1.out_features, c, h, w)
        return None

    @torch.no_grad()
    def load_from_module(self):
        """Module parameters (torch layout) -> flat master (engine layout) + bf16 copies."""
        for s in self.lw.segs:
            self._from_torch_layout(s, self.opt.p, s.param.detach())
        self.opt.pack_weights()

    @torch.no_grad()
    def sync_to_module(self):
        """Flat master -> module parameters (torch layout).  BN buffers are shared already."""
        for s in self.lw.segs:
            s.param.data.copy_(self._to_torch_layout(s, self.opt.p).reshape(s.param.shape))

    def _to_torch_layout(self, seg, flat):
        v = flat[seg.off:seg.off + seg.numel]
        sh = self._krsc_shape(seg)
        if sh is not None:
            k, c, r, s = sh
            return v.view(k, r, s, c).permute(0, 3, 1, 2).reshape(seg.param.shape).contiguous()
        return v.view(seg.param.shape).clone()

    def _from_torch_layout(self, seg, flat, t):
        t = t.to(self.device, torch.float32)
        sh = self._krsc_shape(seg)
        if sh is not None:
            t = t.reshape(sh).permute(0, 2, 3, 1)
        flat[seg.off:seg.off + seg.numel].copy_(t.reshape(-1))

    # ------------------------------------------------------------------ buffers
    def mode(self, name, N=None, group_imgs=0, train=False):
        """Plan the mode (engine/schedule.py), allocate its buffers from the plan's sizes,
        resolve its launch schedules."""
        if name in self.modes:
            return self.modes[name]
        self._apply_globals()
        mp = schedule.plan_mode(self.lw, self.opts, N, self.H, self.W, group_imgs, train)
        m = _Mode(name, mp, self.lw, self.opts)
        dev = self.device
        dw_slab = 0
        nsums = 0
        bf = torch.bfloat16

        def act(M, K):
            return torch.empty(M * K, dtype=bf, device=dev)

        for bi, blk in enumerate(self.lw.blocks):
            for u in blk.units + ([blk.shortcut] if blk.shortcut else []):
                sp = m.spec[u.name]
                inner = u is not blk.units[-1] and u is not blk.shortcut
                if u.depthwise and train:
                    # per-block weight-gradient partials (summed by a reduce kernel), a region
                    # per layer so the reduces can be deferred and batched at the end of the
                    # backward; its own buffer (the split-K slab's head holds tile counters)
                    m.dw_region[u.name] = (dw_slab, ops.dwconv_wgrad_slab_floats(
                        N, sp.P, sp.Q, sp.C), ops.dwconv_wgrad_blocks(N, sp.P, sp.Q, sp.C))
                    dw_slab += m.dw_region[u.name][1]
                m.buf[u.name, 'y'] = act(sp.M, u.K)
                if inner:
                    m.buf[u.name, 'a'] = act(sp.M, u.K)
                if train:
                    m.buf[u.name, 'dy'] = act(sp.M, u.K)
                    m.buf[u.name, 'sums'] = nsums
                    nsums += ops.sums_numel(u.K)      # [SUMS_R][3][K] replicas
                    if inner:
                        m.buf[u.name, 'da'] = act(sp.M, u.K)
            K = blk.units[-1].K
            h, w = mp.hw[bi]
            geom = mp.pool.get(bi)
            rows = N * h * w if geom is None else N * geom[1] * geom[2]
            m.buf[bi, 'out'] = act(rows, K)
            if train:
                m.buf[bi, 'dout'] = act(rows, K)
            if geom is not None:
                m.buf[bi, 'pre'] = m.buf[bi, 'out']
                m.buf[bi, 'out'] = act(N * h * w, K)
                m.buf[bi, 'pool_geom'] = geom
                if train:
                    m.buf[bi, 'argmax'] = torch.empty(N * h * w * K, dtype=torch.uint8,
                                                      device=dev)
                    m.buf[bi, 'dpre'] = m.buf[bi, 'dout']
                    m.buf[bi, 'dout'] = act(N * h * w, K)
            m.buf[bi, 'hw'] = (h, w)
        m.stats_arena = torch.zeros(max(mp.nstats, 1), device=dev)
        m.sums_arena = torch.zeros(max(nsums, 1), device=dev)
        for u in self.units:
            off = mp.stats[u.name]
            m.stats[u.name] = m.stats_arena[off:off + m.G * 2 * u.K]
            if train:
                so = m.buf[u.name, 'sums']
                m.buf[u.name, 'sums'] = m.sums_arena[so:so + ops.sums_numel(u.K)]
        m.final_hw = mp.final_hw
        m.final_C = C = mp.final_C
        m.pooled = torch.zeros(N, C, device=dev)
        m.logits = torch.zeros(N, self.classes, device=dev)   # wide heads' FC output
        m.losses = torch.zeros(N, device=dev)
        if train:
            m.dlogits = torch.zeros(N, self.classes, device=dev)
        m.slab = torch.zeros(max(1, (mp.slab + 3) // 4), dtype=torch.float32, device=dev)
        m.dw_slab = torch.empty(dw_slab, dtype=torch.float32, device=dev) if dw_slab else None
        # per-stream scale / shift workspace of the pointwise GEMM's input prologue (each fused
        # conv's coefficient kernel fills it right before the conv, on the same stream)
        m.coef = torch.zeros(max(1, mp.coef), dtype=torch.float32, device=dev)
        m.input = torch.zeros(N, self.H, self.W, cpad8(self.lw.in_channels), dtype=bf, device=dev)
        m.label = torch.zeros(N, dtype=torch.int32, device=dev)
        m.index = torch.zeros(N, dtype=torch.int32, device=dev)
        m.resolve()
        self.modes[name] = m
        return m

    # ------------------------------------------------------------------ layer execution
    def _gamma(self, u, grad=False):
        return self._pview(u.g_seg, grad)

    def _beta(self, u, grad=False):
        return self._pview(u.beta_seg, grad)

    def _bn_desc(self, m, u, act, count=True, ghost=False, **extra):
        """The BN of ``u`` + activation ``act`` as the descriptor its consumers take (a conv's
        input prologue, the pool, the head, bn_apply): batch / ghost-group statistics (+ the
        rows per group ``count``; ``ghost``: + the images per group) in train and scoring
        modes, the running statistics in eval; ``extra``: the consumer's own keys."""
        d = dict(gamma=self._gamma(u), beta=self._beta(u), act=act, eps=BN_EPS, **extra)
        if m.train or m.group_imgs:
            su = m.spec[u.name]
            d['stats'] = m.stats[u.name]
            if count:
                d['count'] = su.group
            if ghost:
                d['group_imgs'] = m.group_imgs
        else:
            d.update(rmean=u.bn.running_mean, rvar=u.bn.running_var)
        return d

    def _block_in(self, m, bi, x):
        """Input of block ``bi`` in a forward that started from ``x``."""
        return x if bi == 0 else m.buf[bi - 1, 'out']

    def _pro(self, m, s, x):
        """The input prologue of conv step ``s``: the BN + activation of ``s.src_unit`` applied
        to its raw output while the conv loads it (csrc/igemm.h ProParams, pgemm / pwconv /
        dwconv prologues, the halo staging of csrc/hconv.hip MODE 1)."""
        if s.pro is None:
            return None
        u = self.unit[s.src_unit]
        if s.pro == 'halo':
            return self._bn_desc(m, u, s.act, group_imgs=m.group_imgs or m.N)
        kw = dict(keep={None: None, 'a': m.buf.get((u.name, 'a')),
                        'out': m.buf.get((s.block - 1, 'out'))}[s.keep])
        if s.pro == 'dw':
            kw.update(dw=True, group_imgs=m.group_imgs or m.N)
        elif s.pro != 'igemm':
            kw['res'] = self._block_in(m, s.block - 1, x) if s.res == 'in' else None
        if s.pro in ('pg', 'pw'):
            su = m.spec[u.name]
            kw.update({s.pro: True}, coef=m.coef, group_rows=su.group)
        return self._bn_desc(m, u, s.act, **kw)

    def _conv_fwd(self, m, name, route, x, pro=None):
        """Conv unit ``name`` on the kernel ``route`` (schedule.route)."""
        u, sp, y = self.unit[name], m.spec[name], m.buf[name, 'y']
        stats = m.stats[name] if m.train or m.group_imgs else None
        w = self.w_krsc.get(name)
        bias = self._pview(u.b_seg) if u.b_seg is not None else None
        if route == 'stem':
            ops.stem_fwd(x, w, y, sp, stats=stats, bias=bias)
        elif route == 'pwconv':
            ops.pwconv_fwd(x, w, y, sp, stats=stats, pro=pro)
        elif route == 'pgemm':
            ops.pgemm_fwd(x, w, y, sp, stats=stats, bn=m.plan[name, 'pgemm'], pro=pro)
        elif route == 'dwconv':
            ops.dwconv_fwd(x, self._pview(u.w_seg), y, sp.N, sp.H, sp.W, sp.C, sp.P, sp.Q,
                           sp.stride, sp.pad, stats=stats, group_rows=sp.group,
                           pro=pro)
        elif route == 'hconv':
            hconv.hconv_fwd(x, w, y, sp, m.plan[name, 'hconv' if pro is None else 'hconv_bn'],
                            stats=stats, slab=m.slab, bias=bias, pro=pro)
        else:
            ops.conv_fwd(x, w, y, sp, stats=stats, slab=m.slab, bias=bias, pro=pro,
                         plan=m.plan[name, 'fwd'] if pro is None else
                         schedule.pro_plan_of(m.plan, name))

    def _dual_fwd(self, m, s, x):
        """A downsampling block's first conv and its shortcut conv (both read the block input
        x) in ONE launch (ops.conv_fwd_dual); False when the launcher declines the pair."""
        stats_on = m.train or m.group_imgs
        pa, pb = m.plan[s.unit, 'fwd'], m.plan[s.unit2, 'fwd']
        d = [dict(x=x, w=self.w_krsc[n], out=m.buf[n, 'y'], spec=m.spec[n],
                  stats=m.stats[n] if stats_on else None, slab=m.slab, plan=p)
             for n, p in ((s.unit, pa), (s.unit2, pb))]
        if pa[2] > 1 and pb[2] > 1:
            d[1]['slab'] = m.buf[s.unit2, 'slab']      # (_Mode.resolve)
        return ops.conv_fwd_dual(*d)

    def _bn_apply(self, m, s, x):
        blk = self.lw.blocks[s.block]
        u, sp = self.unit[s.unit], m.spec[s.unit]
        out = m.buf[s.unit, 'a'] if s.keep == 'a' else m.buf[s.block, 'pre' if blk.pool else 'out']
        d = self._bn_desc(m, u, s.act)
        kw = {}
        if s.res == 'sc':
            r = self._bn_desc(m, self.unit[s.unit2], None)
            kw['res_bn'] = (r.get('stats'), r['gamma'], r['beta'],
                            (r['rmean'], r['rvar']) if 'rmean' in r else None)
        ops.bn_apply(m.buf[s.unit, 'y'], d.get('stats'), d['gamma'], d['beta'], out, sp.M, u.K,
                     group_rows=sp.group, act=s.act, eps=BN_EPS,
                     running=(d['rmean'], d['rvar']) if 'rmean' in d else None,
                     res={'in': x, 'sc': m.buf.get((s.unit2, 'y')), None: None}[s.res], **kw)

    def forward(self, m, x=None):
        """Forward through all blocks: walks ``m.fwd_steps`` (schedule.forward_schedule).
        Returns the final activation buffer, or the raw last conv output when the head applies
        the last block's BN (``m.head_bn``)."""
        x0 = m.input if x is None else x
        m.head_bn = None
        late_sc = None       # a shortcut conv whose dual launch was declined
        for s in m.fwd_steps:
            x = self._block_in(m, s.block, x0)
            src = x if s.src == 'in' else m.buf[{'pre': (s.block, 'pre'), 'act': (s.src_unit, 'a'),
                                                 'raw': (s.src_unit, 'y')}[s.src]]
            if s.op == 'conv':
                self._conv_fwd(m, s.unit, s.route, src, self._pro(m, s, x0))
            elif s.op == 'dual_conv':
                if not self._dual_fwd(m, s, x):
                    self._conv_fwd(m, s.unit, 'igemm', x)
                    late_sc = s.unit2
            elif s.op == 'bn_apply':
                if s.res == 'sc' and late_sc is not None:
                    self._conv_fwd(m, late_sc, 'igemm', x)
                    late_sc = None
                self._bn_apply(m, s, x)
            elif s.op == 'pool':
                N, h, w, K, P_, Q_, k, st, pd = m.buf[s.block, 'pool_geom']
                bn = self._bn_desc(m, self.unit[s.unit], s.act, count=False, ghost=True) \
                    if s.pro else None
                ops.pool2d_fwd(src, m.buf[s.block, 'out'], N, h, w, K, P_, Q_, k, st, pd,
                               True, m.buf.get((s.block, 'argmax')), bn=bn)
            else:
                # scoring / eval: the head's average pool applies the last block's BN (+
                # identity residual) + activation itself (ops.head_fwd ``bn``)
                m.head_bn = self._bn_desc(m, self.unit[s.unit], s.act, ghost=True,
                                          res=x if s.res == 'in' else None)
                return src
        return m.buf[len(self.lw.blocks) - 1, 'out']

    # ------------------------------------------------------------------ speech-VGG head
    # flatten -> fc1 -> fc2 -> log_softmax (CE on log-probs == CE on logits), all HIP kernels
    # (csrc/head.hip mlp_head_*): fc1 runs on the NHWC activation rows against the [f1][H][W][C]
    # bf16 copy the optimizer writes, its weight gradient lands in the flat buffer in that order
    def _mlp_setup(self, m):
        f1 = self.lw.fc1.out_features
        m.h1 = torch.zeros(m.N, f1, device=self.device)
        if m.train:
            m.dh1 = torch.zeros(m.N, f1, device=self.device)

    def _mlp_head(self, m, x, mode, isw=None, meters=None):
        if getattr(m, 'h1', None) is None:
            self._mlp_setup(m)
        c, h, w = self.mlp_chw
        ops.mlp_head_fwd(x, self.w1p, self._pview(self.lw.fc1_b), self._pview(self.lw.fc_w),
                         self._pview(self.lw.fc_b), m.h1, m.logits, m.label, m.N, c * h * w,
                         self.lw.fc1.out_features, self.classes, mode, isw=isw,
                         dlogits=m.dlogits if mode == 'train' else None, losses=m.losses,
                         meters=meters if mode != 'score' else None,
                         score=self.score if mode == 'score' else 'loss',
                         smooth=self.label_smoothing if mode == 'train' else 0.0,
                         topk=self.topk if mode != 'score' else 0)

    def _mlp_head_bwd(self, m, dout):
        """Grads of fc2 / fc1 into the flat buffer and d(activation) (NHWC bf16) into dout."""
        c, h, w = self.mlp_chw
        x = m.buf[len(self.lw.blocks) - 1, 'out']
        ops.mlp_head_bwd(m.dlogits, m.h1, x, self.w1p, self._pview(self.lw.fc_w), m.dh1,
                         self._pview(self.lw.fc1_w, True), self._pview(self.lw.fc1_b, True),
                         self._pview(self.lw.fc_w, True), self._pview(self.lw.fc_b, True), dout,
                         m.N, c * h * w, self.lw.fc1.out_features, self.classes)

    def head(self, m, x, mode, isw=None, meters=None):
        if self.lw.head_pool == 'mlp2':
            return self._mlp_head(m, x, mode, isw=isw, meters=meters)
        hb = getattr(m, 'head_bn', None) if mode != 'train' else None
        ops.head_fwd(x, self._pview(self.lw.fc_w), self._pview(self.lw.fc_b), m.label, m.N,
                     m.final_hw, m.final_C, self.classes, mode, pooled=m.pooled,
                     logits=m.logits,
                     dlogits=getattr(m, 'dlogits', None) if mode == 'train' else None,
                     losses=m.losses, isw=isw, meters=meters,
                     score=self.score if mode == 'score' else 'loss', bn=hb,
                     smooth=self.label_smoothing if mode == 'train' else 0.0,
                     topk=self.topk if mode != 'score' else 0)

    def flush_dw_reduces(self, m):
        """The deferred depthwise wgrad reduces of this backward, in one launch."""
        ops.dwconv_wgrad_reduce_batch(m.dw_pending)
        m.dw_pending = []

    def _wgrad(self, m, u, dy, x):
        sp = m.spec[u.name]
        gw = self._pview(u.w_seg, grad=True)
        if u.depthwise:          # (a train mode with a depthwise unit has its dw_slab region)
            off, n, _ = m.dw_region[u.name]
            ops.dwconv_wgrad(dy, x, gw, sp.N, sp.H, sp.W, sp.C, sp.P, sp.Q, sp.stride,
                             sp.pad, slab=m.dw_slab[off:off + n])
        else:
            ops.conv_wgrad(dy, x, gw, sp, plan=m.plan[u.name, 'wgrad'])

    def _conv_bwd(self, m, name, kind, dy, x, dx, accumulate=False, bw=None):
        """Weight gradient and (``dx``) data gradient of conv ``name`` by launch ``kind``
        (schedule.BwdStep).  ``bw``: the dgrad epilogue also reduces the BN-backward sums of
        the unit feeding ``dx``."""
        u, sp = self.unit[name], m.spec[name]
        if kind == 'pair':
            # dgrad + wgrad of this conv in ONE launch (they share dy and are independent)
            ops.conv_bwd(dy, self.w_crsk[name], dx, x, self._pview(u.w_seg, grad=True), sp,
                         dplan=m.plan[name, 'dgrad'], wplan=m.plan[name, 'wgrad'],
                         slab=m.slab, accumulate=accumulate, bw=bw)
        elif kind == 'dw_pair':
            assert not accumulate
            # dgrad + wgrad in one launch; the wgrad partials' reduce is deferred to one batched
            # launch (flush_dw_reduces): at the end of the backward, or (DP) before the bucket
            # all-reduce that carries this weight gradient (train_segments) -- nothing reads a
            # depthwise weight gradient before the optimizer or its bucket's all-reduce
            off, n, nblk = m.dw_region[name]
            region = m.dw_slab[off:off + n]
            gw = self._pview(u.w_seg, grad=True)
            ops.dwconv_bwd(dy, x, self._pview(u.w_seg), dx, gw, sp.N, sp.H, sp.W, sp.C, sp.P,
                           sp.Q, sp.stride, sp.pad, region, bw=bw, reduce=False)
            m.dw_pending.append((region, gw, sp.C, nblk))
        else:
            self._wgrad(m, u, dy, x)
            if dx is not None and u.depthwise:
                assert not accumulate
                ops.dwconv_dgrad(dy, self._pview(u.w_seg), dx, sp.N, sp.H, sp.W, sp.C, sp.P,
                                 sp.Q, sp.stride, sp.pad, bw=bw)
            elif dx is not None:
                ops.conv_dgrad(dy, self.w_crsk[name], dx, sp, slab=m.slab,
                               plan=m.plan[name, 'dgrad'], accumulate=accumulate, bw=bw)

    def _conv_bwd_sc(self, m, s, dy, x, dx, bw, xs, dxs):
        """``s.unit``'s dgrad + wgrad (dx, fused BN-backward sums ``bw``) and the shortcut
        ``s.unit2``'s (input ``xs``, writes ``dxs``) in one launch; two launches when the
        launcher declines the pair."""
        u, sc = self.unit[s.unit], self.unit[s.unit2]
        a = dict(dy=dy, wt=self.w_crsk[u.name], dx=dx, x=x, dw=self._pview(u.w_seg, grad=True),
                 spec=m.spec[u.name], dplan=m.plan[u.name, 'dgrad'],
                 wplan=m.plan[u.name, 'wgrad'], slab=m.slab, accumulate=False, bw=bw)
        b = dict(dy=m.buf[sc.name, 'dy'], wt=self.w_crsk[sc.name], dx=dxs, x=xs,
                 dw=self._pview(sc.w_seg, grad=True), spec=m.spec[sc.name],
                 wplan=m.plan[sc.name, 'wgrad'], accumulate=False)
        if ops.conv.conv_bwd_sc(a, b):
            return
        self._conv_bwd(m, sc.name, 'pair', m.buf[sc.name, 'dy'], xs, dxs)
        self._conv_bwd(m, u.name, 'pair', dy, x, dx, bw=bw)

    def _bw(self, m, u, out, act, unit2=None):
        """Fused-reduce descriptor for the BN of ``u`` (+ shortcut BN ``unit2``) whose activation
        output is ``out`` -- consumed by conv_dgrad(bw=...)."""
        d = dict(out=out, y=m.buf[u.name, 'y'], stats=m.stats[u.name], sums=m.buf[u.name, 'sums'],
                 act=act, eps=BN_EPS)
        if unit2 is not None:
            d.update(y2=m.buf[unit2.name, 'y'], stats2=m.stats[unit2.name])
        return d

    def _bn_bwd(self, m, u, dout, out, act, dy, unit2=None, dy2=None, dz=None, reduce=True):
        sp = m.spec[u.name]
        kw = {}
        if unit2 is not None:
            kw = dict(y2=m.buf[unit2.name, 'y'], stats2=m.stats[unit2.name],
                      gamma2=self._gamma(unit2), dy2=dy2, dgamma2=self._gamma(unit2, True),
                      dbeta2=self._beta(unit2, True))
        ops.bn_bwd(dout, out, m.buf[u.name, 'y'], m.stats[u.name], self._gamma(u),
                   m.buf[u.name, 'sums'], dy, sp.M, u.K, act=act, eps=BN_EPS, dz=dz,
                   dgamma=self._gamma(u, True), dbeta=self._beta(u, True), zero_sums=False,
                   reduce=reduce, **kw)

    def backward_block(self, m, bi):
        for _, f in self.backward_parts(m, bi):
            f()
        if bi == 0:                      # the backward is complete: deferred reduces
            self.flush_dw_reduces(m)

    def _bwd_step(self, m, s):
        """One launch of the backward schedule (schedule.BwdStep)."""
        bi, blk = s.block, self.lw.blocks[s.block]
        x = m.buf[bi - 1, 'out'] if bi > 0 else m.input
        dx = m.buf.get((bi - 1, 'dout'))
        u = self.unit[s.unit]
        final = u is blk.units[-1]
        pre = 'pre' if blk.pool else 'out'
        if s.op == 'pool_bwd':
            N, h, w, K, P_, Q_, k, st, pd = m.buf[bi, 'pool_geom']
            ops.maxpool2d_bwd(m.buf[bi, 'dout'], m.buf[bi, 'argmax'], m.buf[bi, 'dpre'], N, h, w,
                              K, P_, Q_, k, st, pd)
        elif s.op == 'bn_bwd' and final:
            sc = blk.shortcut
            reduce = s.reduce == 'pass' or (s.reduce == 'head' and not m.head_reduced)
            m.head_reduced = False
            self._bn_bwd(m, u, m.buf[bi, 'd' + pre], m.buf[bi, pre], blk.final_act,
                         m.buf[u.name, 'dy'], unit2=sc, dy2=m.buf[sc.name, 'dy'] if sc else None,
                         dz=dx if s.dx else None, reduce=reduce)
        elif s.op == 'bn_bwd':
            self._bn_bwd(m, u, m.buf[u.name, 'da'], m.buf[u.name, 'a'], u.act,
                         m.buf[u.name, 'dy'], reduce=s.reduce == 'pass')
        else:
            i = blk.units.index(u) if u is not blk.shortcut else 0
            inp = x if i == 0 else m.buf[blk.units[i - 1].name, 'a']
            bw = None
            if s.bw is not None and i > 0:
                p = blk.units[i - 1]
                bw = self._bw(m, p, m.buf[p.name, 'a'], p.act)
            elif s.bw is not None:
                pb = self.lw.blocks[bi - 1]
                bw = self._bw(m, pb.units[-1], m.buf[bi - 1, 'out'], pb.final_act,
                              unit2=pb.shortcut)
            d = {'block': dx, 'da': m.buf.get((blk.units[i - 1].name, 'da')), None: None}[s.dx]
            if s.kind == 'pair_sc':
                self._conv_bwd_sc(m, s, m.buf[u.name, 'dy'], inp, d, bw, x, dx)
            else:
                self._conv_bwd(m, u.name, s.kind, m.buf[u.name, 'dy'], inp, d,
                               accumulate=s.acc, bw=bw)

    def backward_parts(self, m, bi):
        """Block ``bi``'s backward as [(unit index, callable)] in execution order (last unit
        first): after part i, the gradients of units i..last, of the BNs of units i-1..last
        and of the shortcut are final -- so a gradient bucket may close between parts."""
        return [(i, lambda steps=steps: [self._bwd_step(m, s) for s in steps])
                for i, steps in m.bwd.parts[bi]]


    # ------------------------------------------------------------------ data
    def _recipe(self, recipe):
        """A recipe whose crop is the network's input size (filled in where it has none)."""
        if recipe is None:
            return None
        if isinstance(recipe, SpecRecipe):
            recipe.check(self.lw.in_channels, self.H, self.W)
            return recipe
        recipe = recipe.with_crop((self.H, self.W))
        if recipe.out_hw != (self.H, self.W):
            raise ValueError('augmentation recipe crops to %s but the engine was built for '
                             'image_hw=%s' % (recipe.out_hw, (self.H, self.W)))
        return recipe

    def _device_inputs(self, images, recipe=None):
        """uint8 HWC images stay uint8 [N][H][W][3] (augmented on the fly) -- with a recipe,
        [N][Hs][Ws][3] of any size its crop fits; float inputs [N][C][H][W] (e.g. spectrograms)
        are converted ONCE to NHWC bf16 [N][H][W][8] -- or, with a ``SpecRecipe``, kept planar
        as bf16 [N][C][H][W] (the same rounding, one eighth of the bytes at C = 1)."""
        x = torch.as_tensor(np.ascontiguousarray(images)) if not torch.is_tensor(images) \
            else images
        if isinstance(recipe, SpecRecipe):
            C = self.lw.in_channels
            if x.dtype == torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (C, self.H, self.W):
                raise ValueError('a SpecRecipe needs a float shard [N][%d][%d][%d], got %s %s'
                                 % (C, self.H, self.W, x.dtype, tuple(x.shape)))
            out = torch.empty(x.shape, dtype=torch.bfloat16, device=self.device)
            for s0 in range(0, x.shape[0], 4096):
                out[s0:s0 + 4096] = x[s0:s0 + 4096].to(self.device, torch.float32)
            return out
        if x.dtype == torch.uint8 and recipe is not None:
            if x.dim() != 4 or x.shape[3] != 3:
                raise ValueError('uint8 shard must be [N][Hs][Ws][3], got %s' % (tuple(x.shape),))
            recipe.check(x.shape[1], x.shape[2])
            return x.to(self.device).contiguous()
        if recipe is not None:
            raise ValueError('an augmentation recipe needs uint8 HWC images, got %s' % x.dtype)
        if x.dtype == torch.uint8:
            if x.dim() != 4 or tuple(x.shape[1:]) != (self.H, self.W, 3):
                raise ValueError('uint8 shard must be [N][%d][%d][3], got %s'
                                 % (self.H, self.W, tuple(x.shape)))
            return x.to(self.device).contiguous()
        C = self.lw.in_channels
        if x.dim() != 4 or tuple(x.shape[1:]) != (C, self.H, self.W):
            raise ValueError('float shard must be [N][%d][%d][%d], got %s'
                             % (C, self.H, self.W, tuple(x.shape)))
        out = torch.empty(x.shape[0], self.H, self.W, 8, dtype=torch.bfloat16, device=self.device)
        step = 4096
        for s0 in range(0, x.shape[0], step):
            blk = x[s0:s0 + step].to(self.device, torch.float32).contiguous()
            ops.nchw_to_nhwc8(blk, out[s0:s0 + step])
        return out

    def set_shard(self, images, labels):
        """Keep this rank's training shard resident in HBM: uint8 [Ns][H][W][3] images, or
        float [Ns][C][H][W] inputs pre-converted to NHWC bf16 (planar bf16 under a SpecRecipe)."""
        x = self._device_inputs(images, self.augment)
        if x.shape[0] < 1:
            raise ValueError('empty shard')
        if self.augment is not None and self.aug_params is None:
            n = SPEC_PARAMS if isinstance(self.augment, SpecRecipe) else \
                PHOTO_PARAMS if self.augment.photo else 8
            self.aug_params = torch.zeros(self.P, n, dtype=torch.float32, device=self.device)
        # (a shard smaller than one batch -- possible for a Dirichlet non-IID split at large
        # world size -- is cycled: every batch is the shard's epoch permutation, wrapped)
        self.shard = x
        self.shard_labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(self.device)
        self.train_mode = self.mode('train', self.B, 0, True)
        self.score_mode = self.mode('score', self.P, self.B, False)
        if self.lw.head_pool == 'mlp2':
            self._mlp_setup(self.train_mode)
            self._mlp_setup(self.score_mode)
        self.idx = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._arange_b = torch.arange(self.B, dtype=torch.int32, device=self.device)
        self.isw = torch.ones(self.B, dtype=torch.float32, device=self.device)
        if self.global_table:
            # shard-wide importance table resident in HBM: every scored pool sample's latest
            # loss, stamped with the optimizer step that scored it
            self.table = ops.ImportanceTable(self.shard.shape[0], self.device)
        if self.sampler == 'groupwise':
            if self.shard.shape[0] < self.P:
                raise ValueError("sampler='groupwise' needs a shard of at least one pool "
                                 '(%d samples)' % self.P)
            self._draw_pos = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self._gstamp = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._build_bn_table()

    def _build_bn_table(self):
        """Running-stat update table: the train batch, then (importance mode) the 10 scored
        pool batches, each a train-mode forward in the reference.  The uniform baseline
        scores nothing, so its table updates from the train batch only."""
        tables = []
        tm, sm = self.train_mode, self.score_mode
        for n_score in (sm.G, 0):
            rows = []
            for u in self.units:
                sp_t, sp_s = tm.spec[u.name], sm.spec[u.name]
                rows.append((u.bn.running_mean, u.bn.running_var, tm.stats[u.name],
                             sm.stats[u.name], u.bn.num_batches_tracked, u.K, 1, n_score,
                             float(sp_t.M), float(sp_s.group)))
            tables.append(ops.BnRunTable(rows, self.device))
        self.bn_table, self.bn_table_uniform = tables

    # ------------------------------------------------------------------ step pieces
    def score_branch(self):
        self.score_forward()
        if not self._split_score:
            self.score_sample()

    def score_forward(self):
        sm = self.score_mode
        if not self.scoring:
            # uniform-sampling baseline: the next batch is the next 32 shard samples
            # (epoch-shuffled, augmented), no pool forward, unit weights
            ops.pool_build(self.shard, self.shard_labels, self.ctrl, sm.input, sm.label,
                           sm.index, self.B, self.B, self.seed, recipe=self.augment,
                           params=self.aug_params)
            self.ctrl[0:1].add_(1)
            self.idx.copy_(self._arange_b)
            self.isw.fill_(1.0)
            return
        # groupwise (Groupwise_Sampler, `util.py:114-138`): the pool is the next CONTIGUOUS slice
        # of the shard (cursor order, wrapping), which becomes this iteration's group.
        # Deviation (parity unpinned: no reference fixture covers it): when Ns % P != 0 the
        # slice that reaches the end of the shard wraps to its head and stays a full P-sample
        # group, where the reference truncates it at len(dataset) (a short group) and resets
        # the cursor.  Group sizes stay P, so the table weights need no short-group handling.
        ops.pool_build(self.shard, self.shard_labels, self.ctrl, sm.input, sm.label, sm.index,
                       self.P, self.B, self.seed, zero=sm.stats_arena,
                       shuffle=self.sampler != 'groupwise', recipe=self.augment,
                       params=self.aug_params)
        # (the scoring convs keep their full occupancy: reserving extra LDS per scoring block
        # so train blocks fit beside them measured 1.70-2.21 ms/step vs 1.65 -- in the
        # concurrent step the GPU is throughput-bound, bench/ab_env.sh)
        x = self.forward(sm)
        self.head(sm, x, 'score')
        if self.table is not None:
            if self.sampler == 'groupwise':
                # a new group per scored slice (never 0: group 0 is the initial uniform table)
                torch.add(self.ctrl[0:1], 1, out=self._gstamp)
                self.table.scatter(sm.index, sm.losses, stamp=self._gstamp)
            else:
                self.table.scatter(sm.index, sm.losses, stamp=self.ctrl[2:3])

    def score_sample(self):
        if not self.scoring:
            return
        sm = self.score_mode
        if self.sampler == 'groupwise':
            # draw from the global HBM table over the current group (the slice just scattered,
            # stamped with this step's counter): p ~ imp + mean(imp) (`util.py:144-152`), then
            # pool slots + unbiased weights n_group * p
            self.table.draw_batch(self.B, self._gstamp, self._draw_pos, sm.index,
                                  self.shard.shape[0], self.P, self.idx, self.isw, seed=self.seed,
                                  meters=self.meters)
            self.ctrl[0:2].add_(1)       # pool and draw counters (is_sample bumps them otherwise)
            return
        gathered = self.score_exchange.gathered if self._split_score else None
        ops.is_sample(sm.losses, self.ema, self.ctrl, self.idx, self.isw, self.P, self.B, self.B,
                      self.alpha, self.ema_alpha, self.seed, self.importance, self.meters,
                      alias=self.sampler == 'alias', gathered=gathered)

    @property
    def _split_score(self):
        # global EMA: the all-gather of every rank's pool scores sits between the scoring
        # forward and the draw, so the score stream runs as two graphs around the collective
        return self.global_ema and self.score_exchange is not None and self.scoring

    def _score_stream_work(self, graphs):
        """Everything on the score stream for one step (caller sets the stream)."""
        if graphs:
            graphs['score'].replay()
        else:
            self.score_forward() if self._split_score else self.score_branch()
        if self.score_exchange is not None and self.scoring:
            # cross-worker importance-score all-gather, issued on the score stream
            # right after scoring; RCCL runs it beside the train backward
            cs = torch.cuda.current_stream(self.device)
            self.timer.mark('xchg0', cs)
            self.score_exchange.start(self.score_mode.losses)
            self.timer.mark('xchg1', cs)
        if self._split_score:
            self.score_exchange.wait()          # stream-side wait on RCCL
            if graphs:
                graphs['score_sample'].replay()
            else:
                self.score_sample()

    def gather_batch(self):
        sm, tm = self.score_mode, self.train_mode
        ops.gather(sm.input, sm.label, sm.index, self.idx, tm.input, tm.label, tm.index, self.B)

    def train_segments(self):
        """Train fwd + backward as a list of callables; bucket all-reduces go between them."""
        tm = self.train_mode
        segs = []

        def fwd_head():
            tm.dw_pending = []
            ops.lib().step_begin(ops.ptr(self.ctrl), ops.stream_ptr(), ops.ptr(tm.stats_arena),
                                 tm.stats_arena.numel(), ops.ptr(tm.sums_arena),
                                 tm.sums_arena.numel())
            x = self.forward(tm)
            self.head(tm, x, 'train', isw=self.isw, meters=self.meters)
            last = len(self.lw.blocks) - 1
            if self.lw.head_pool == 'mlp2':
                self._mlp_head_bwd(tm, tm.buf[last, 'dout'])
                return
            # the head's backward also reduces the final BN's backward sums (no bn_bwd reduce
            # pass at the top of the last block) where its per-sample path runs
            lb = self.lw.blocks[last]
            bw = None
            if tm.bwd.head_bw:
                bw = self._bw(tm, lb.units[-1], tm.buf[last, 'out'], lb.final_act,
                              unit2=lb.shortcut)
            tm.head_reduced = bool(ops.head_bwd(
                tm.pooled, tm.dlogits, self._pview(self.lw.fc_w), self._pview(self.lw.fc_w, True),
                self._pview(self.lw.fc_b, True), tm.buf[last, 'dout'], self.B, tm.final_hw,
                tm.final_C, self.classes, bw=bw))
        cuts = self.bucket_plan()
        dw = any(u.depthwise for u in self.units)
        cur = [fwd_head]
        for bi in range(len(self.lw.blocks) - 1, -1, -1):
            for i, f in self.backward_parts(tm, bi):
                cur.append(f)
                if (bi, i) in cuts:
                    if dw:
                        # the bucket's depthwise weight gradients are complete before it
                        # all-reduces (a no-op when none is pending)
                        cur.append(lambda: self.flush_dw_reduces(tm))
                    segs.append((cur, cuts[bi, i]))
                    cur = []
        if cur:
            segs.append((cur, None))
        if dw:
            segs[-1][0].append(lambda: self.flush_dw_reduces(tm))
        if self.check_order:
            # every train segment ticks o[2]; the comm stream checks it before reducing
            for fs, _ in segs:
                fs.append(lambda: self._order(tick=2, at=1))
        return segs

    def _block_starts(self):
        starts = []
        for bi, blk in enumerate(self.lw.blocks):
            us = blk.units + ([blk.shortcut] if blk.shortcut else [])
            starts.append(min(min(s.off for s in (u.w_seg, u.g_seg, u.beta_seg)) for u in us))
        return starts

    def bucket_plan(self):
        """{(block, unit index): (flat_start, flat_end)} -- a bucket closes after that unit's
        backward part (backward_parts) once it holds >= ``bucket_bytes`` of gradient, and
        always after block 0's first unit.  Parameters are laid out in forward order, so the
        backward finishes them from the end of the flat buffer; cutting inside a block (not
        only at block boundaries) lets the first all-reduce start one conv earlier.  A block
        whose shortcut parameters precede its last unit's is cut only at its boundary."""
        if not self.dp:
            return {}
        if getattr(self, '_bucket_plan', None) is not None:
            return self._bucket_plan       # static: cached once (the issue loop reads it)
        starts = self._block_starts()
        cuts = {}
        end = self.lw.total
        # the last bucket: blocks 0 .. kl - 1, the largest leading run within last_bucket_bytes
        # (a cut at block kl's start is forced; 0: no forced cut)
        kl = 0
        for k in range(1, len(starts) if self.last_bucket_bytes > 0 else 1):
            if starts[k] * 4 > self.last_bucket_bytes:
                break
            kl = k
        for bi in range(len(self.lw.blocks) - 1, -1, -1):
            blk = self.lw.blocks[bi]
            ustart = [min(s.off for s in (u.w_seg, u.g_seg, u.beta_seg)) for u in blk.units]
            inner = blk.shortcut is None or min(
                s.off for s in (blk.shortcut.w_seg, blk.shortcut.g_seg,
                                blk.shortcut.beta_seg)) >= ustart[-1]
            inner = inner and all(ustart[i] < ustart[i + 1] for i in range(len(ustart) - 1))
            for i in range(len(blk.units) - 1, -1, -1):
                if i > 0 and not inner:
                    continue
                start = starts[bi] if i == 0 else ustart[i]
                if (bi == 0 and i == 0) or (end - start) * 4 >= self.bucket_bytes or (
                        bi == kl and i == 0 and kl > 0 and end > start):
                    cuts[bi, i] = (0 if (bi == 0 and i == 0) else start, end)
                    end = start
        self._bucket_plan = cuts
        return cuts

    def tail(self):
        if self.check_order:
            # the tail consumes the scoring stream's draw and (DP) every reduced bucket: both
            # must have finished this step -- o[0] / o[1] == steps completed + 1
            self._order(slot=0, ref=3, mult=1, add=1, at=3)
            if self.dp:
                self._order(slot=1, ref=3, mult=1, add=1, at=4)
            self._order(tick=3, at=5)
        (self.bn_table if self.scoring else self.bn_table_uniform).launch(0.1)
        if self.opt.clip_on:
            # global-norm clipping: the tail runs behind every bucket's all-reduce, so this is
            # the norm of the averaged gradient and every rank computes the same coefficient
            self.opt.clip()
        self.opt.step(self.ctrl[2:3])
        self.gather_batch()

    def _order(self, slot=-1, ref=0, mult=0, add=0, ge=False, tick=-1, at=0):
        ops.lib().order_check(ops.ptr(self.order), slot, ref, mult, add, int(ge), tick, at,
                              ops.stream_ptr())

    def order_violations(self):
        """(count, first violation record) of the stream-order checks (``check_order``)."""
        o = self.order.tolist()
        return o[4], dict(slot=o[8], seen=o[9], want=o[10], at=o[11]) if o[4] else None

    # ------------------------------------------------------------------ graphs
    def _capture(self, fn, stream, keep=False):
        """Capture ``fn`` on ``stream`` in THREAD-LOCAL mode.  The default global mode forbids
        "unsafe" HIP calls on every thread of the process while a capture is open; the
        ProcessGroupNCCL watchdog thread polls its works' events every ~100 ms, and a poll that
        lands inside a global capture fails and aborts the process from that native thread (the
        round-4 driver suite abort).  Thread-local mode confines the restriction to this
        thread; build_graphs additionally quiesces the process before capturing."""
        g = torch.cuda.CUDAGraph(keep_graph=keep)
        with torch.cuda.graph(g, stream=stream, capture_error_mode='thread_local'):
            fn()
        if keep:
            g.instantiate()
        return g

    def _quiesce(self):
        """Nothing of this process may run a HIP call into an open capture: drain the device,
        the score exchange and every ProcessGroup work this engine issued, then run the
        collector NOW (finalizers of dead engines -- torch graphs, queued HIP objects -- execute
        here, not inside a capture) and release what dead engines queued."""
        torch.cuda.synchronize(self.device)
        if self.score_exchange is not None:
            self.score_exchange.wait()
        works, self._pg_works = self._pg_works, []
        if works and dist.is_initialized():      # (a destroyed group's works are moot)
            for w in works:
                w.wait()
        torch.cuda.synchronize(self.device)
        gc.collect()
        _release_queued()

    def build_graphs(self):
        self._check_open()
        self._quiesce()
        # no collector pass (and so no finalizer HIP call) while a capture is open
        gc_on = gc.isenabled()
        gc.disable()
        try:
            self._build_graphs()
        finally:
            if gc_on:
                gc.enable()

    def _build_graphs(self):
        self._apply_globals()
        for m in self.modes.values():
            m.resolve()                  # (the plans may have changed: ops/step_tune.py)
        cap = torch.cuda.Stream(self.device)
        segs = self.train_segments()
        comm_ev = (self.dp and self.s_comm is not None
                   and self.opts.comm_events and len(segs) > 1)
        if self._train_exec and not comm_ev:
            ops.lib().graph_exec_destroy(self._train_exec)
            self._train_exec = 0
        self.graphs = {
            'score': self._capture(self.score_forward if self._split_score else self.score_branch,
                                   cap),
            'train': [(self._capture(lambda fs=fs: [f() for f in fs], cap, keep=comm_ev), b)
                      for fs, b in segs],
            'tail': self._capture(self.tail, cap),
        }
        if self._split_score:
            self.graphs['score_sample'] = self._capture(self.score_sample, cap)
        if comm_ev:
            # ONE linear executable graph: the segment graphs as child nodes, an event-record
            # node after each bucket's segment; each bucket's host-issued all-reduce on the comm
            # stream waits on its node of this replay (segmented replays cost ~33 us per extra
            # segment at W = 1).  The segment graphs stay for the timed (phase-marked) path.
            L = ops.lib()
            if not self._bucket_evs:
                self._bucket_evs = [L.ext_event_create() for _, b in segs if b is not None]
            evs, k = [], 0
            for _, b in segs:
                evs.append(self._bucket_evs[k] if b is not None else 0)
                k += b is not None
            if self._train_exec:
                L.graph_exec_destroy(self._train_exec)
            self._train_exec = L.graph_chain(
                [g.raw_cuda_graph() for g, _ in self.graphs['train']], evs)
        self._graph_scoring = self.scoring
        torch.cuda.synchronize(self.device)

    def close(self):
        """Release everything this engine owns that is not plain device memory, in a fixed
        order, now: drain the device and outstanding collectives, drop the torch graphs
        (their executables and private pools), destroy the chained DP executable and its
        events, unmap / free the xGMI exchange buffers.  Idempotent; the engine cannot step
        afterwards.  The shared RCCL communicator is left to ``RcclComm.close`` (other engines
        of the process use it)."""
        if getattr(self, '_closed', True):
            return
        self._quiesce()
        if self.graphs:
            for v in self.graphs.values():
                for g in (v if isinstance(v, list) else [v]):
                    g = g[0] if isinstance(g, tuple) else g
                    g.reset()
        self.graphs = None
        L = ops.lib()
        if self._train_exec:
            L.graph_exec_destroy(self._train_exec)
            self._train_exec = 0
        for e in self._bucket_evs:
            L.ext_event_destroy(e)
        self._bucket_evs = []
        self.score_exchange = None
        torch.cuda.synchronize(self.device)
        self._closed = True
        LIVE.discard(self)
        x, self.xgmi = self.xgmi, None
        if x is not None:
            x.close()                    # collective at W > 1; raises XgmiTimeout last

    def _check_open(self):
        if self._closed:
            raise RuntimeError('NativeEngine was closed')

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        # an engine that was never closed: its chained DP executable and events are HIP objects
        # of the extension, not torch's.  No HIP call here (a collection can run at any point):
        # they are queued and released by the next _quiesce, after a device synchronisation
        try:
            if getattr(self, '_closed', True):
                return
            ex, evs = getattr(self, '_train_exec', 0), getattr(self, '_bucket_evs', ())
            if ex or evs:
                _RELEASE.append((ex, list(evs)))
        except Exception:       # interpreter shutdown
            pass

    def prime(self):
        """Score a first pool and gather the first training batch (reference `train()` entry)."""
        self._check_open()
        self._apply_globals()
        s0 = torch.cuda.current_stream(self.device)
        self.s_score.wait_stream(s0)
        with torch.cuda.stream(self.s_score):
            self._score_stream_work(None)
        s0.wait_stream(self.s_score)
        self.gather_batch()
        self.primed = True

    def step(self):
        """One importance-sampled DP step (all async; nothing syncs the host unless ``debug``).

        Streams: the scoring stream (next pool) and the train stream (this batch) start
        together; after each bucket segment of the backward the comm stream all-reduces that
        bucket (RCCL, AVG) while later segments and the scoring keep computing; the tail on the
        train stream waits for the scoring stream and the last bucket."""
        if self._closed:
            raise RuntimeError('NativeEngine was closed')
        s0 = torch.cuda.current_stream(self.device)
        graphs = self.graphs if self.use_graphs else None
        if not graphs:
            self._apply_globals()            # eager launches read the launcher globals
        if graphs and self._graph_scoring != self.scoring:
            raise RuntimeError('scoring was toggled after build_graphs(); rebuild the graphs')
        T = self.timer
        T.begin_step()
        T.mark('start', s0)
        rx = self.roctx
        debug = self.debug
        if rx:
            prof.push('score')
        if debug:
            # serialised: scoring first, on the train stream, checked before training starts
            self._score_stream_work(None)
            if self.check_order:
                self._order(tick=0, at=0)
            self._debug_sync('score')
        else:
            ev_start = torch.cuda.Event()
            ev_start.record(s0)
            self.s_score.wait_event(ev_start)
            with torch.cuda.stream(self.s_score):
                T.mark('score0', self.s_score)
                self._score_stream_work(graphs)
                if self.check_order:
                    self._order(tick=0, at=0)
                T.mark('score1', self.s_score)
        if rx:
            prof.pop()
            prof.push('train')
        works = []
        segs = graphs['train'] if graphs else self.train_segments()
        nb = 0
        if graphs and self._train_exec and not T.on and not debug:
            # one train replay; each bucket's all-reduce waits on its event node in it
            ops.lib().graph_launch(self._train_exec, s0.cuda_stream)
            for si, (_, bucket) in enumerate(segs):
                if bucket is not None:
                    works.append(self._reduce_bucket(s0, bucket, nb, si,
                                                     ev=self._bucket_evs[nb]))
                    nb += 1
            segs = []
        for si, (g, bucket) in enumerate(segs):
            if graphs:
                g.replay()
            else:
                for f in g:
                    f()
            if debug:
                self._debug_sync('train segment %d' % si)
            if bucket is not None and self.dp:
                works.append(self._reduce_bucket(s0, bucket, nb, si))
                nb += 1
        T.mark('train1', s0)
        if rx:
            prof.pop()
            prof.push('allreduce')
        if self.s_comm is not None and nb:
            if self.check_order:
                with torch.cuda.stream(self.s_comm):
                    self._order(tick=1, at=2)
            ev_c = torch.cuda.Event()
            ev_c.record(self.s_comm)
            s0.wait_event(ev_c)
        for wk in works:
            if wk is not None:
                self._finish_work(wk)
                if self.check_order and wk is works[-1]:
                    self._order(tick=1, at=2)
        # (kept until the next step / quiesce: drained before any capture)
        self._pg_works = [wk[0] for wk in works if wk is not None]
        if debug and self.dp:
            self._debug_sync('allreduce')
        if not debug:
            ev_score = torch.cuda.Event()
            ev_score.record(self.s_score)
            s0.wait_event(ev_score)
        if rx:
            prof.pop()
            prof.push('tail')
        T.mark('tail0', s0)
        if self.grad_probe is not None and self.dp:
            self.grad_probe('post', None, self.opt.g)
        if graphs:
            graphs['tail'].replay()
        else:
            self.tail()
        T.mark('end', s0)
        if debug:
            self._debug_sync('tail')
        if rx:
            prof.pop()

    def _reduce_bucket(self, s0, bucket, i, si, ev=None):
        """Issue bucket ``i``'s gradient all-reduce behind train segment ``si`` (or behind
        ``ev``, that segment's event node in the one-graph train replay)."""
        s, e = bucket
        g = self.opt.g[s:e]
        if self.tern is not None:
            self._tern_ctr += 1          # a fresh Philox stream per (step, bucket) (host path)
        if self.s_comm is None:          # torch ProcessGroup (gloo / CPU tests)
            if self.grad_probe is not None:
                self.grad_probe('pre', i, g)
            if self.tern is not None:
                self.tern.allreduce(g, self._tern_ctr)
                return None
            return [dist.all_reduce(g, op=self._avg_op, async_op=True), s, e, False]
        if ev is None:
            ev = torch.cuda.Event()
            ev.record(s0)
            self.s_comm.wait_event(ev)
        else:
            ops.lib().ext_event_wait(self.s_comm.cuda_stream, ev)
        with torch.cuda.stream(self.s_comm):
            if self.check_order:
                # the bucket's gradients are final: train segment si has ticked this step
                self._order(slot=2, ref=3, mult=self._nseg, add=si + 1, ge=True, at=6)
            self.timer.bucket(i, 0, self.s_comm)
            if self.grad_probe is not None:
                self.grad_probe('pre', i, g)
            if self.xgmi is not None:
                # direct two-shot over xGMI (all peers' exchange buffers mapped by IPC, device
                # flag barriers); consecutive buckets alternate the two exchange slots; the bf16
                # wire option lives in the exchange buffers
                self.xgmi.allreduce(g, avg=True, slot=i % 2)
                if i == len(self.bucket_plan()) - 1:
                    self.xgmi.end_step(i + 1)
            elif self.tern is not None:
                # 2-bit stochastic ternary codes + one scale per rank, all-gathered (1/16 of
                # the fp32 bytes), decoded to the same mean on every rank; Philox stream =
                # (device optimizer-step counter, bucket): fresh every replayed step
                self.tern.allreduce(g, i, dctr=self.ctrl[2:3])
            elif self.comm.size == 1 and not self.opts.rccl_one_rank:
                # one rank (forced buckets): the AVG is the identity -- the bucket plan, the
                # event waits and the comm stream run as at W > 1, RCCL's one-rank copy kernel
                # does not (EngineOptions.rccl_one_rank issues it: the tests)
                pass
            elif self.wire_bf16:
                # bf16 on the wire: half the bytes over xGMI; the sum is rounded once per hop
                if self.wire is None:
                    self.wire = torch.empty(self.lw.total, dtype=torch.bfloat16,
                                            device=self.device)
                w = self.wire[s:e]
                w.copy_(g)
                self.comm.allreduce(w, avg=True)
                g.copy_(w)
            else:
                self.comm.allreduce(g, avg=True)
            self.timer.bucket(i, 1, self.s_comm)
        return None

    @property
    def _nseg(self):
        plan = self.bucket_plan()
        return len(plan) + (0 if (0, 0) in plan else 1)

    def _debug_sync(self, what):
        """Debug mode: drain the device after every phase so a fault names its phase."""
        try:
            torch.cuda.synchronize(self.device)
        except RuntimeError as e:
            raise RuntimeError('device error after %s: %s' % (what, e)) from e
        if self.check_order:
            n, first = self.order_violations()
            if n:
                raise RuntimeError('stream-order violation after %s: %s' % (what, first))
        if self.debug_log:
            print('[mercury_amd debug] step phase done: %s' % what, flush=True)

    def _finish_work(self, wk):
        """Make the current stream wait for a bucket all-reduce (once per stream is harmless;
        the gloo SUM -> mean scaling runs once)."""
        w, s, e, done = wk
        w.wait()
        if not done and self._avg_op != dist.ReduceOp.AVG:   # gloo has no AVG
            self.opt.g[s:e].mul_(1.0 / self.world_size)
        wk[3] = True

    # ------------------------------------------------------------------ misc API
    def reset_ema(self):
        self.ema.zero_()

    def broadcast_from(self, src=0):
        """Initial replica sync (reference `pytorch_collab.py:84-87` averages parameters only;
        this broadcasts parameters AND BN running stats from ``src``).  On the engine's own
        RCCL communicator when it has one (stream-ordered, no ProcessGroup work left in flight
        for a later graph capture), else the ProcessGroup, drained before returning."""
        self._check_open()
        bufs = [self.opt.p]
        seen = set()
        for u in self.units:
            for b in (u.bn.running_mean, u.bn.running_var):
                if id(b) not in seen:
                    seen.add(id(b))
                    bufs.append(b)
        if self.comm is not None:
            for b in bufs:
                self.comm.broadcast(b, src)
        else:
            works = [dist.broadcast(b, src, async_op=True) for b in bufs]
            for w in works:
                w.wait()
            torch.cuda.synchronize(self.device)
        self.opt.pack_weights()

    @torch.no_grad()
    def evaluate_arrays(self, images, labels, batch=500, augment=None):
        """Eval-mode (running-stats BN) loss / accuracy over uint8 HWC images (or float NCHW
        inputs) on device.  ``augment`` (default: the engine's ``eval_augment``): the recipe
        applied to the images, its random crop included -- drawn from the engine's seed and the
        batch number, so a second call sees the same views; the batch order is kept."""
        recipe = self._recipe(augment) if augment is not None else self.eval_augment
        imgs = self._device_inputs(images, recipe)
        labs = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(self.device)
        n = imgs.shape[0]
        self.eval_meters.zero_()
        ctrl = torch.zeros(8, dtype=torch.int64, device=self.device)
        # with a recipe the loss is the ordered fp64 sum of the per-sample losses: the meters'
        # atomic fp32 sum depends on block arrival order, and fixed random views should give one
        # number (a forward with split-K convs still moves single losses by an ulp)
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        done = 0
        while done < n:
            b = min(batch, n - done)
            m = self.mode('eval%d' % b, b, 0, False)
            if recipe is not None:
                ops.pool_build(imgs[done:done + b], labs[done:done + b], ctrl, m.input, m.label,
                               m.index, b, b, self.seed, shuffle=False, recipe=recipe)
                ctrl[0:1].add_(1)       # (the next batch draws its own crops)
            else:
                ops.pool_build(imgs[done:done + b], labs[done:done + b], ctrl, m.input, m.label,
                               m.index, b, b, self.seed, augment=False, shuffle=False)
            x = self.forward(m)
            self.head(m, x, 'eval', meters=self.eval_meters)
            if recipe is not None:
                loss_sum += m.losses[:b].double().sum()
            done += b
        r = self.eval_meters[:6].tolist()
        self.eval_topk = (int(r[5]), int(r[1]))
        if recipe is not None:
            r[0] = loss_sum.item()
        return r[0] / max(r[1], 1), r[2] / max(r[1], 1), int(r[1])

    def global_share(self):
        """Each rank's fraction of total pool importance (needs ``exchange_scores``)."""
        if self.score_exchange is None:
            return torch.ones(1, device=self.device)
        return self.score_exchange.global_share()

    def read_meters(self):
        b = self.meters.tolist()
        if self.xgmi is not None:
            # host-synchronised already: a device barrier that gave up on a peer (its error word)
            # fails loudly here instead of turning into silent replica divergence
            self.xgmi.check()
        return {'loss_sum': b[0], 'count': b[1], 'correct': b[2], 'pool_mean': b[3], 'ema': b[4],
                'correct_k': b[5]}


# ---------------------------------------------------------------------- trainer
def _dataset_arrays(loader):
    ds = getattr(loader, 'dataset', None)
    x = getattr(ds, 'data', None)
    y = getattr(ds, 'target', None)
    if y is None:
        y = getattr(ds, 'targets', None)
    if x is None or y is None:
        raise ValueError('native engine needs a dataset with uint8 HWC .data and .target')
    return np.asarray(x), np.asarray(y)


def _image_hw(x):
    """uint8 [N][H][W][3] images or float [N][C][H][W] inputs -> (H, W)."""
    return tuple(x.shape[1:3]) if x.dtype == np.uint8 else tuple(x.shape[2:4])


def _config_recipes(cfg, presam_loader, test_loader):
    """``Config.augment`` -> (train recipe, eval recipe): 'cifar' keeps the engine's built-in
    pipeline (None, None); 'dataset' reads the loaders' ``dataset.transform``; anything else
    is an ``AugmentRecipe.parse`` spec, evaluated with its Resize, crop (``rrc`` included: there
    is no CenterCrop) and Normalize only.
    A spec starting with ``spec:`` (``SpecRecipe.parse``), or a ``transforms.SpecAugment`` as
    the train dataset's transform, gives that spectrogram recipe and no eval recipe."""
    from ..data.augment import AugmentRecipe
    from ..data.transforms import SpecAugment
    spec = getattr(cfg, 'augment', 'cifar')
    if spec == 'cifar':
        return None, None
    if spec.startswith('spec:'):
        return SpecRecipe.parse(spec), None
    if spec == 'dataset':
        tr = [getattr(getattr(ld, 'dataset', None), 'transform', None)
              for ld in (presam_loader, test_loader)]
        if isinstance(tr[0], SpecAugment):
            return tr[0].recipe, None
        return AugmentRecipe.from_transform(tr[0]), AugmentRecipe.from_transform(tr[1])
    aug = AugmentRecipe.parse(spec)
    return aug, dataclasses.replace(aug, flip=False, degrees=0.0, scale=None, cutout=0,
                                    jitter=None)


class NativeTrainer(Trainer):
    """``Trainer`` whose step runs on the native engine (same public API)."""

    def __init__(self, net, optimizer, train_loader, presam_loader, test_loader, device,
                 config=None):
        from ..config import Config
        cfg = config or Config()
        self.cfg = cfg
        self.net = net
        self.optimizer = optimizer
        self.train_loader = train_loader
        self.presam_loader = presam_loader
        self.test_loader = test_loader
        self.device = torch.device(device)
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.com_tensor = torch.ones(1)
        self.epoch, self.step, self.writer, self.scheduler = 0, 1, None, None
        self.epoch_step = 0
        self.next_batch_iter = None
        self.computed_samples = {'index': [], 'prob': []}
        self.should_compute_importance = True
        self.batch_size = getattr(train_loader, 'batch_size', None) or cfg.batch_size
        self.steps_per_epoch = len(train_loader) if train_loader is not None else 1
        self.flat = None
        self.bucketer = None
        from ..utils.logging import PhaseTimer
        self.timer = PhaseTimer(self.device)
        # the engine's fused kernel performs the optimizer step; tell the LR scheduler so it
        # does not warn that optimizer.step() was never called
        optimizer._opt_called = True
        osp = ops.optimizer_spec(optimizer)       # raises on anything the kernel cannot run
        x, y = _dataset_arrays(presam_loader)
        aug, eval_aug = _config_recipes(cfg, presam_loader, test_loader)
        image_hw = _image_hw(x)
        if aug is not None and not isinstance(aug, SpecRecipe):
            image_hw = aug.with_crop(image_hw).out_hw
        self.engine = NativeEngine(
            net, self.device, self.batch_size, cfg.presample_batches, image_hw=image_hw,
            augment=aug, eval_augment=eval_aug,
            optimizer=osp['algo'], lr=osp['lr'], betas=osp['betas'], eps=osp['eps'],
            weight_decay=osp['weight_decay'], momentum=osp['momentum'],
            seed=cfg.seed * 1000 + self.rank, alpha=cfg.alpha,
            ema_alpha=cfg.ema_alpha, importance=cfg.importance, world_size=self.world_size,
            bucket_bytes=int(cfg.bucket_mb * (1 << 20)) or None, use_graphs=cfg.use_graphs,
            sampler=cfg.sampler, exchange_scores=cfg.exchange_scores,
            score=cfg.score, global_ema=cfg.global_ema, wire_bf16=cfg.wire_bf16,
            grad_compress=cfg.grad_compress,
            comm=cfg.comm, debug=cfg.debug, check_order=cfg.check_order,
            force_buckets=cfg.force_buckets, clip_grad_norm=cfg.clip_grad_norm,
            label_smoothing=cfg.label_smoothing, topk=cfg.topk)
        self.label_smoothing, self.topk = self.engine.label_smoothing, self.engine.topk
        self.engine.set_shard(x, y)
        self.engine.roctx = cfg.roctx
        from ..utils.profiling import StepWindow
        self.profile_window = StepWindow(cfg.profile_start, cfg.profile_steps)

    def _flat_params(self):
        return self.engine.opt.p

    def average_model(self):
        if self.world_size == 1:
            return
        if self.cfg.parity:
            dist.all_reduce(self.engine.opt.p, op=dist.ReduceOp.SUM)
            self.engine.opt.p /= float(self.world_size)
            self.engine.opt.pack_weights()
        else:
            self.engine.broadcast_from(0)

    def average_gradients(self):
        pass  # bucketed inside engine.step()

    def update_samples(self, ema_loss=None, alpha=None):
        """API-compatible scoring call: returns (weights, data NCHW, label, index, pool_mean).

        The native step scores the next pool inside ``step()``, so this is a read-only view of
        the pending (already scored and drawn) batch; only before the first step does it score
        a pool (``prime``)."""
        e = self.engine
        if not e.primed:
            e.prime()
        sm = e.score_mode
        idx = e.idx.long()
        data = sm.input[idx][..., :3].permute(0, 3, 1, 2).float()
        mean = e.meters[3].clone()
        if ema_loss is not None:
            ema_loss.first_update = False
            ema_loss.value = float(e.ema[0].item())
        return e.isw.clone(), data, sm.label[idx].long(), sm.index[idx].long(), mean

    def _sync_lr(self):
        self.engine.opt.set_lr(self.optimizer.param_groups[0]['lr'])

    def train(self):
        e = self.engine
        running_train_loss = Average()
        presam_ema_loss = EMAverage(self.cfg.ema_alpha)
        runing_train_acc = Accuracy(self._report_k())
        e.reset_ema()                      # reference: fresh EMAverage per epoch (`:121`)
        e.meters[:3].zero_()
        e.meters[5:6].zero_()
        self._sync_lr()
        e.prime()
        t0 = time.perf_counter()
        pe = self.cfg.print_every
        for _ in range(max(0, self.steps_per_epoch - self.epoch_step)):
            # device-phase timing for the steps that are printed (events cost host time)
            e.timer.on = bool(pe) and self.step % pe == 0 and self.rank == 0
            if e.use_graphs and e.graphs is None:
                # the first step runs eagerly (warms every kernel), then the step is captured;
                # it is a real training step and counts like every other one
                e.step()
                e.build_graphs()
            else:
                e.step()
            self._health()
            if self.cfg.print_every and self.step % self.cfg.print_every == 0:
                self._log(t0)
                t0 = time.perf_counter()
            if self.cfg.eval_every and self.step % self.cfg.eval_every == 0 and (
                    self.rank == 0 or self.cfg.eval_all_ranks):
                self._eval_log()
            self._advance()
            if self._stop():
                break
        m = e.read_meters()
        running_train_loss.update(m['loss_sum'] / max(m['count'], 1), max(int(m['count']), 1))
        runing_train_acc.update_counts(m['correct'], int(m['count']), m['correct_k'])
        presam_ema_loss.update(m['ema'])
        return running_train_loss, runing_train_acc, presam_ema_loss

    def _log(self, t0):
        if self.rank != 0:
            return
        m = self.engine.read_meters()
        cnt = max(m['count'], 1)
        ph = self.engine.timer.collect()
        dev = ''
        if ph:
            # reference C27 fields (`pytorch_collab.py:129-178`), from device events: step, IS
            # (scoring stream), ff+bp, sync (all-reduce, and the part not hidden), opt (tail)
            dev = (', device ms: step {step:.3f} (critical path {critical:.3f}), IS {score:.3f}, '
                   'ff+bp {train:.3f}, sync {comm:.3f} (exposed {exp:.3f}), wait {wait:.3f}, '
                   'opt+tail {tail:.3f}, IS share {share:.1f}%').format(
                       exp=ph.get('comm_exposed', 0.0), share=100.0 * ph['score'] / max(
                           ph['score'] + ph['train'], 1e-9), **ph)
        clip = ''
        if self.engine.opt.clip_on:
            # the last step's norm (before clipping); read here only -- it is a host sync
            gn = self.engine.opt.last_grad_norm()
            clip = ', grad_norm: {:.6g}'.format(gn)
        k = self._report_k()
        topk = ', top{}: {:.2f}%'.format(k, 100 * m['correct_k'] / cnt) if k else ''
        print('step:{}, running train loss: {:.6f}, running train acc: {:.2f}%{}, '
              'presam_ema_loss: {:.6f}, pool_mean: {:.4f}{}, {:.3f} ms/step{}'.format(
                  self.step, m['loss_sum'] / cnt, 100 * m['correct'] / cnt, topk, m['ema'],
                  m['pool_mean'], clip,
                  (time.perf_counter() - t0) * 1e3 / self.cfg.print_every, dev),
              flush=True)
        if self.engine.check_order:
            n, first = self.engine.order_violations()
            if n:
                raise RuntimeError('stream-order violation (%d): %s' % (n, first))

    def _eval_log(self):
        train_loss, train_acc, test_loss, test_acc = self.evaluate()
        if self.writer is not None:
            self.writer.add_scalar('train/acc', train_acc.accuracy, self.step)
            self.writer.add_scalar('test/acc', test_acc.accuracy, self.step)
            self.writer.add_scalar('train/loss', train_loss.average, self.step)
            self.writer.add_scalar('test/loss', test_loss.average, self.step)
            self._write_acc_k(train_acc, test_acc)
            if self.engine.opt.clip_on:
                self.writer.add_scalar('train/grad_norm', self.engine.opt.last_grad_norm(),
                                       self.step)
        if self.rank == 0:
            self._print_eval(train_loss, train_acc, test_loss, test_acc)

    def evaluate(self, max_batches=None):
        out = []
        for loader in (self.train_loader, self.test_loader):
            lm, am = Average(), Accuracy(self._report_k())
            if loader is not None:
                x, y = _dataset_arrays(loader)
                bs = getattr(loader, 'batch_size', 32) or 32
                n = (len(x) // bs) * bs       # drop_last, as the reference loaders
                if max_batches is not None:
                    n = min(n, max_batches * bs)
                loss, acc, cnt = self.engine.evaluate_arrays(x[:n], y[:n])
                lm.update(loss, cnt)
                am.update_counts(acc * cnt, cnt, self.engine.eval_topk[0])
            out += [lm, am]
        return out[0], out[1], out[2], out[3]

    def state_dict(self):
        e = self.engine
        e.sync_to_module()
        ost = self.optimizer.state_dict()
        state = {}
        t = int(e.ctrl[2].item())
        for i, s in enumerate(e.lw.segs):
            st = {'step': torch.tensor(float(t)), 'exp_avg': e._to_torch_layout(s, e.opt.m).cpu()}
            if e.opt.algo in (0, 2):
                st['exp_avg_sq'] = e._to_torch_layout(s, e.opt.v).cpu()
            else:
                st = {'momentum_buffer': st['exp_avg']}
            state[i] = st
        ost['state'] = state
        return {'model': {k: v.detach().cpu() for k, v in self.net.state_dict().items()},
                'optimizer': ost,
                'scheduler': self.scheduler.state_dict() if self.scheduler else None,
                'step': self.step, 'epoch': self.epoch, 'epoch_step': self.epoch_step,
                'engine': self._engine_state()}

    def _engine_state(self):
        e = self.engine
        out = {'ctrl': e.ctrl.cpu(), 'ema': e.ema.cpu()}
        if e.table is not None:
            # shard importance table with the Groupwise_Sampler field names (`util.py:106-107`)
            out['importance'] = e.table.importance.cpu()
            out['group_indicator'] = e.table.group.cpu().to(torch.int64)
        return out

    def load_state_dict(self, sd):
        e = self.engine
        self.net.load_state_dict(sd['model'])
        e.load_from_module()
        st = sd['optimizer'].get('state', {})
        for i, s in enumerate(e.lw.segs):
            if i in st:
                if 'exp_avg' in st[i]:
                    e._from_torch_layout(s, e.opt.m, st[i]['exp_avg'])
                if 'exp_avg_sq' in st[i] and e.opt.algo in (0, 2):
                    e._from_torch_layout(s, e.opt.v, st[i]['exp_avg_sq'])
                if 'momentum_buffer' in st[i]:
                    e._from_torch_layout(s, e.opt.m, st[i]['momentum_buffer'])
        if sd.get('scheduler') and self.scheduler is not None:
            self.scheduler.load_state_dict(sd['scheduler'])
        self.optimizer.param_groups[0]['lr'] = sd['optimizer']['param_groups'][0]['lr']
        self.step, self.epoch = sd['step'], sd['epoch']
        self.epoch_step = int(sd.get('epoch_step', 0))
        if 'engine' in sd:
            es = sd['engine']
            if e.table is not None and 'importance' in es:
                n = es['importance'].numel()
                if n != e.table.importance.numel():
                    raise ValueError(
                        'checkpoint importance table has %d entries but this rank\'s shard has '
                        '%d: resume each rank from its own file (Config.resume = a directory of '
                        'ckpt_rank<r>.pt files, or a path with {rank})'
                        % (n, e.table.importance.numel()))
            e.ctrl.copy_(es['ctrl'].to(e.device))
            e.ema.copy_(es['ema'].to(e.device))
            if e.table is not None and 'importance' in es:
                e.table.importance.copy_(es['importance'].to(e.device))
                e.table.group.copy_(es['group_indicator'].to(e.device, torch.int32))


# ---------------------------------------------------------------------- smoke
def smoke_step(device='cuda:0', steps=2):
    """Tiny end-to-end check used by ``__graft_entry__.smoke``."""
    from ..models import ResNet18
    torch.manual_seed(0)
    net = ResNet18(10).to(device)
    eng = NativeEngine(net, device, batch_size=32, pool_batches=10, use_graphs=True)
    rng = np.random.RandomState(0)
    eng.set_shard(rng.randint(0, 256, (640, 32, 32, 3), dtype=np.uint8),
                  rng.randint(0, 10, 640))
    eng.prime()
    eng.step()
    eng.build_graphs()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    m = eng.read_meters()
    assert math.isfinite(m['loss_sum']) and m['count'] == 32 * (steps + 1), m
    return m
