"""Per-mode planning of the native engine: pure Python over ``lower(net)``, no device.

``plan_mode`` builds the conv specs, looks up every plan table and sizes the buffers of one
batch mode; ``forward_schedule`` / ``backward_schedule`` resolve, from those plans, which kernel
runs each unit and who applies (forward) or reduces (backward) each BatchNorm.  The engine
(``native.NativeEngine``) allocates from the sizes and walks the schedules: it takes no placement
decision while it launches.  Nothing here touches the extension or ``torch.cuda``, so a CPU test
can ask how many ``bn_apply`` passes a mode runs (tests/test_schedule.py).
"""
from __future__ import annotations

from collections import namedtuple

from ..ops import conv, hconv, tune
from ..ops.conv import (ConvSpec, cpad8, dgrad_plan, fwd_plan, pgemm_ok, pgemm_plain_wins,
                        pgemm_plan, pgemm_pro_wins, pro_ok, pro_plan, pwconv_ok,
                        pwconv_plain_wins, pwconv_pro_wins, slab_bytes, stem_ok, wgrad_plan)

ACTS = ('relu', 'relu6', 'none')     # activations every BN-applying consumer implements


class ModePlan(object):
    """Specs, plans and buffer sizes of one batch mode (``plan_mode``)."""

    def __init__(self, N, group_imgs, train):
        self.N = N
        self.group_imgs = group_imgs   # images per BN stat group (0 = whole batch)
        self.train = train
        self.G = 1 if not group_imgs else N // group_imgs
        self.spec = {}                 # unit name -> ConvSpec
        self.plan = {}                 # (unit name, kind) -> plan
        self.slab = 0                  # split-K slab, bytes
        self.coef = 0                  # pg / pw prologue scale + shift workspace, floats
        self.stats = {}                # unit name -> offset into the statistics arena
        self.nstats = 0
        self.pool = {}                 # block -> (N, h, w, K, P, Q, k, stride, pad)
        self.hw = {}                   # block -> output (h, w)
        self.final_hw = 0              # H * W and C of the last block's output
        self.final_C = 0


def apply_globals(opts):
    """The EngineOptions that live in process-wide Python state and that planning reads: the
    halo-conv plan switches and the stride-2 dgrad switch (the C++ launcher's share of them is
    set where launches happen: ``hconv.configure_launcher``)."""
    hconv.configure(opts)
    conv.DGRAD_S2 = opts.dgrad_s2


def plan_mode(lw, opts, N, H, W, group_imgs, train):
    """The ``ModePlan`` of batch ``N`` at input ``H`` x ``W``."""
    apply_globals(opts)
    mp = ModePlan(N, group_imgs, train)
    persist_bn = opts.persist_bn if opts.persist_bn in ('0', '1', 'row', 'stat') else (
        '1' if str(opts.persist_bn).lower() in ('true', 'on', 'yes') else '0')
    C = cpad8(lw.in_channels)
    for bi, blk in enumerate(lw.blocks):
        h, w = H, W
        main_hw = None
        for u in blk.units + ([blk.shortcut] if blk.shortcut else []):
            if u is blk.shortcut:
                main_hw = (h, w)
                h, w = H, W          # the shortcut reads the block input
            sp = ConvSpec(N, h, w, u.C, u.K, u.R, u.R, u.stride, u.pad)
            if group_imgs:
                sp.group_rows = group_imgs * sp.P * sp.Q
            mp.spec[u.name] = sp
            if not u.depthwise:
                # measured-best plans from the tuning cache (ops/tune.py) when present
                # the scoring pass runs beside the latency-bound train chain: fewer, larger
                # tiles leave the train kernels more room (measured, ResNet-18: 128-block
                # target 1.656 vs 256-block 1.667 ms/step; split-K or 512 blocks slower)
                mb = opts.score_min_blocks if group_imgs else 0
                mp.plan[u.name, 'fwd'] = p = tune.fwd_plan_for(
                    sp, fwd_plan(sp, min_blocks=mb) if mb else fwd_plan(sp))
                slab = slab_bytes(sp.M, sp.K, *p[:3])
                pp = pro_plan(sp) if opts.pro_plans else None
                if pp is not None:
                    # the plan it runs with when it takes its input's BN in the prologue
                    mp.plan[u.name, 'fwd_pro'] = pp
                    slab = max(slab, slab_bytes(sp.M, sp.K, *pp))
                if opts.pgemm and pgemm_ok(sp) and u.b_seg is None:
                    mp.plan[u.name, 'pgemm'] = pgemm_plan(sp)
                    mp.coef = max(mp.coef, mp.G * 2 * sp.Cp)
                if opts.stem and stem_ok(sp) and bi == 0 and u is blk.units[0]:
                    mp.plan[u.name, 'stem'] = True
                if opts.pwconv and pwconv_ok(sp) and u.b_seg is None:
                    mp.plan[u.name, 'pwconv'] = True
                    mp.coef = max(mp.coef, mp.G * 2 * sp.Cp)
                # stride-1 3x3 convs on the halo-tile kernel where it measured faster
                uh = opts.hconv == '1' or opts.hconv == ('train' if train else 'score')
                hp = hconv.engine_plan(sp, bias=u.b_seg is not None, train=train) if uh else None
                if hp is not None:
                    mp.plan[u.name, 'hconv'] = hp
                    slab = max(slab, slab_bytes(sp.M, sp.K, *hp[:3]))
                # scoring pass: an intra-block conv on the persistent kernel takes its
                # input's BN + activation in the halo staging (no residual there)
                hb = None
                if not train and group_imgs and persist_bn != '0' and \
                        u is not blk.units[0] and u is not blk.shortcut:
                    hb = hconv.persist_bn_plan(sp, group_imgs,
                                               row_only=persist_bn in ('row', 'stat'),
                                               stat_only=persist_bn == 'stat')
                if hb is not None:
                    mp.plan[u.name, 'hconv_bn'] = hb
                    slab = max(slab, slab_bytes(sp.M, sp.K, *hb[:3]))
                if train:
                    if u.need_dgrad and sp.K % 8 == 0:
                        dp, wp = tune.bwd_plans_for(sp, dgrad_plan(sp), wgrad_plan(sp))
                    else:
                        dp, wp = dgrad_plan(sp), wgrad_plan(sp)
                    if u.need_dgrad:
                        mp.plan[u.name, 'dgrad'] = dp
                        slab = max(slab, slab_bytes(N * h * w, sp.Cp, *dp))
                    mp.plan[u.name, 'wgrad'] = wp
                mp.slab = max(mp.slab, slab)
            mp.stats[u.name] = mp.nstats
            mp.nstats += mp.G * 2 * u.K
            if u is not blk.shortcut:
                h, w = sp.P, sp.Q
        if main_hw is not None:
            h, w = main_hw
        K = blk.units[-1].K
        if blk.pool is not None:
            k, st, pd = blk.pool
            P_ = (h + 2 * pd - k) // st + 1
            Q_ = (w + 2 * pd - k) // st + 1
            mp.pool[bi] = (N, h, w, K, P_, Q_, k, st, pd)
            h, w = P_, Q_
        mp.hw[bi] = (h, w)
        H, W, C = h, w, K
    mp.final_hw = H * W
    mp.final_C = C
    return mp


def route(plan, spec, unit, opts, pro_kind):
    """The forward kernel of ``unit``: 'stem', 'pwconv', 'pgemm', 'dwconv', 'hconv' or 'igemm',
    given the kind of input prologue it runs with (None: plain)."""
    n = unit.name
    if pro_kind == 'halo':
        return 'hconv'
    if pro_kind is None and (n, 'stem') in plan:
        return 'stem'
    if pro_kind == 'pw':
        return 'pwconv'
    if pro_kind is None and (n, 'pwconv') in plan and pwconv_plain_wins(spec) and \
            opts.pwconv_plain:
        return 'pwconv'
    if (n, 'pgemm') in plan and (pro_kind == 'pg' or
                                 pro_kind is None and pgemm_plain_wins(spec)):
        return 'pgemm'
    if unit.depthwise:
        return 'dwconv'
    if pro_kind is None and (n, 'hconv') in plan:
        return 'hconv'
    return 'igemm'


def pro_plan_of(plan, name):
    """igemm plan of a conv when it applies its input's BN in the prologue."""
    return plan.get((name, 'fwd_pro'), plan[name, 'fwd'])


Step = namedtuple('Step', 'op block unit unit2 route src src_unit pro act keep res',
                  defaults=(None,) * 8)
Step.__doc__ = """One forward launch (names and kinds only).

op        'conv', 'dual_conv' (``unit`` and the shortcut ``unit2`` in one launch; the launcher
          may decline: then the two-launch form), 'bn_apply', 'pool', or 'head_bn' (last: the
          classifier head applies the last block's BN; launches nothing itself)
route     the conv's kernel (``route``)
src       what it reads: 'in' (the block input), 'act' (the activation of ``src_unit``), 'raw'
          (the raw conv output of ``src_unit``) or 'pre' (the pool's pre-pool activation)
pro       who applies the BN + ``act`` of ``src_unit``: a conv's input prologue ('igemm', 'dw',
          'pg', 'pw', 'res', 'halo'), 'pass' (bn_apply), 'pool' or 'head'; None: nobody here
keep      where the activation is written: 'a' (intra-block), 'out' (the block output of
          ``src_unit``'s block) or None (nothing reads it)
res       the residual added before the activation: 'in' (the input of ``src_unit``'s block),
          'sc' (the BN of the shortcut ``unit2``) or None"""


def _pg_kind(mp, nxt, act, res):
    """'pw' / 'pg' when the panel conv / pointwise GEMM running ``nxt`` applies its producer's
    BN in its input prologue, else None.  Narrow-input convs whose output spans several N-tiles
    take the panel-resident kernel (pwconv.hip: each element normalised once, not per tile)."""
    if act not in ACTS:
        return None
    sn = mp.spec[nxt.name]
    if res is None and (nxt.name, 'pwconv') in mp.plan and pwconv_pro_wins(sn):
        return 'pw'
    if (nxt.name, 'pgemm') in mp.plan and sn.stride == 1 and pgemm_pro_wins(sn):
        return 'pg'
    return None


def _intra_pro(mp, opts, u, nxt):
    """Prologue kind with which ``nxt`` applies the BN of its intra-block producer ``u``, or
    None (a bn_apply pass).  Train mode keeps the activation (backward reads it)."""
    if not opts.fuse_bn_fwd or u.act not in ACTS:
        return None
    if nxt.depthwise:
        # MobileNetV2's expand BN + ReLU6 applied to each chunk the depthwise conv loads
        return 'dw' if opts.dw_pro else None
    pg = _pg_kind(mp, nxt, u.act, None)
    if pg is not None:
        return pg
    ok = pro_ok(mp.spec[nxt.name], pro_plan_of(mp.plan, nxt.name), keep=mp.train)
    return 'igemm' if ok else None


def _res_pro_ok(mp, opts, act, nxt):
    """Block-final BN (+ identity residual) + activation folded into the register-staged load
    of the next block's first (pointwise) conv on igemm, which writes the block output through
    the prologue's keep (MobileNetV2's linear-bottleneck outputs feeding the next expand conv).
    Not where that conv runs plain on another kernel (a pwconv plan only runs with its own
    prologue kind: with this prologue the conv runs on igemm)."""
    if not (opts.fuse_bn_fwd and opts.res_pro) or act not in ACTS:
        return False
    sp = mp.spec[nxt.name]
    if sp.R != 1 or route(mp.plan, sp, nxt, opts, None) not in ('igemm', 'pwconv'):
        return False
    return pro_ok(sp, pro_plan_of(mp.plan, nxt.name), keep=True)


def dual_ok(mp, opts, u, sc):
    """A downsampling block's first conv and its shortcut conv (both read the block input) in
    ONE launch: both plain igemm, no bias, equal tiles."""
    if not opts.dual_fwd or u.b_seg is not None or sc.b_seg is not None:
        return False
    if any(route(mp.plan, mp.spec[v.name], v, opts, None) != 'igemm' for v in (u, sc)):
        return False
    return tuple(mp.plan[u.name, 'fwd'][:2]) == tuple(mp.plan[sc.name, 'fwd'][:2])


def forward_schedule(lw, mp, opts):
    """The forward launches of mode ``mp`` in order, as ``Step``s."""
    steps = []
    nblk = len(lw.blocks)
    carry = None     # the previous block's final BN (+ identity residual), applied by this
    #                  block's first conv (which writes that block's output): Step fields
    for bi, blk in enumerate(lw.blocks):
        nu = len(blk.units)
        sc = blk.shortcut
        sc_done = False      # the shortcut conv already ran (with the first conv, one launch)
        cur = dict(src='in')   # how the next conv of this block reads its input
        for i, u in enumerate(blk.units):
            sp = mp.spec[u.name]
            if carry is not None:
                cur, carry = carry, None
            if i == 0 and cur.get('pro') is None and sc is not None and dual_ok(mp, opts, u, sc):
                steps.append(Step('dual_conv', bi, u.name, unit2=sc.name, route='igemm',
                                   src='in'))
                sc_done = True
            else:
                steps.append(Step('conv', bi, u.name,
                                   route=route(mp.plan, sp, u, opts, cur.get('pro')), **cur))
            if i < nu - 1:
                nxt = blk.units[i + 1]
                if (nxt.name, 'hconv_bn') in mp.plan and not nxt.depthwise and u.act in ACTS:
                    # the next conv applies this BN + act while staging its halo (scoring
                    # pass: nothing reads the intra-block activation)
                    cur = dict(src='raw', src_unit=u.name, pro='halo', act=u.act)
                    continue
                # intra-block BN + activation: inside the next conv's operand load when it
                # can take it, else its own pass
                kind = _intra_pro(mp, opts, u, nxt)
                if kind is not None:
                    cur = dict(src='raw', src_unit=u.name, pro=kind, act=u.act,
                               keep='a' if mp.train else None)
                    continue
                steps.append(Step('bn_apply', bi, u.name, src='raw', src_unit=u.name,
                                   pro='pass', act=u.act, keep='a'))
                cur = dict(src='act', src_unit=u.name)
                continue
            # the block-final BN (+ residual) + activation
            if sc is not None and not sc_done:
                steps.append(Step('conv', bi, sc.name, src='in',
                                   route=route(mp.plan, mp.spec[sc.name], sc, opts, None)))
            res = 'sc' if sc is not None else 'in' if blk.identity else None
            nb = lw.blocks[bi + 1] if bi + 1 < nblk else None
            act = blk.final_act
            last = dict(src='raw', src_unit=u.name, act=act, res=res)
            kind = None
            if nb is not None and not blk.pool and nb.units and sc is None:
                n0 = nb.units[0]
                kind = _pg_kind(mp, n0, act, res)
                if kind is None and not n0.depthwise and _res_pro_ok(mp, opts, act, n0):
                    kind = 'res'
            if kind is not None:
                # the next block's first (pointwise) conv applies this BN (+ identity
                # residual) + activation in its operand tiles and writes the block output
                carry = dict(last, pro=kind, keep='out')
            elif (nb is None and not mp.train and not blk.pool and sc is None and
                  opts.head_bn and lw.head_pool != 'mlp2' and act in ACTS and u.K % 8 == 0):
                # scoring / eval: nothing reads the last block's output but the head's
                # average pool, which applies this BN (+ identity residual) + activation
                # itself (ops.head_fwd ``bn``): no bn_apply pass
                steps.append(Step('head_bn', bi, u.name, pro='head', **last))
            elif blk.pool and not mp.train and res is None and act in ACTS:
                # scoring / eval (nothing reads the pre-pool activation): the pool applies
                # this BN + activation per tap, straight from the conv output
                steps.append(Step('pool', bi, u.name, pro='pool', **last))
            else:
                steps.append(Step('bn_apply', bi, u.name, unit2=sc.name if sc else None,
                                   pro='pass', keep='out', **last))
                if blk.pool:
                    steps.append(Step('pool', bi, u.name, src='pre'))
    return steps


def last_bn_by(steps):
    """Who applies the last block's BN: 'pass', 'pool' or 'head'."""
    return next(s.pro for s in reversed(steps) if s.pro in ('pass', 'pool', 'head'))


BwdStep = namedtuple('BwdStep', 'op block unit unit2 kind dx acc bw reduce',
                     defaults=(None, None, None, False, None, None))
BwdStep.__doc__ = """One backward launch (names and kinds only).

op        'pool_bwd', 'bn_bwd' (the BN of ``unit`` + the shortcut BN of ``unit2``) or 'conv_bwd'
kind      conv_bwd: 'pair' (dgrad + wgrad in one launch), 'pair_sc' (... and the shortcut
          ``unit2``'s; the launcher may decline: then the shortcut's own launch kind and
          'pair'), 'dw_pair' (depthwise dgrad + wgrad) or 'separate' (wgrad, then the dgrad)
dx        conv_bwd: where the data gradient goes: 'block' (the block input's gradient), 'da'
          (the previous unit's activation gradient) or None (no dgrad);
          bn_bwd: 'block' when it also adds the identity branch's gradient into it
acc       conv_bwd: the dgrad accumulates into ``dx``
bw        conv_bwd: the unit whose BN-backward sums this dgrad reduces in its epilogue
reduce    bn_bwd: who reduced its sums: 'pass' (its own reduce), 'dgrad' (the consumer's
          dgrad epilogue) or 'head' (the head's backward where its per-sample path ran,
          known at run time: else its own reduce)"""


def _bwd_kind(mp, opts, u, dx):
    """Backward launch kind of conv ``u`` (``dx``: it has a data gradient)."""
    if dx and not u.depthwise and mp.spec[u.name].K % 8 == 0:
        return 'pair'
    if dx and u.depthwise and opts.dw_pair:
        return 'dw_pair'
    return 'separate'


def _bw_unit(mp, u, dx, prod, prod_sc=None):
    """The gate of the fused BN-backward reduce: ``prod`` when the dgrad of ``u`` may reduce the
    sums of its producer BN ``prod`` (+ shortcut BN ``prod_sc``) in its epilogue, else None.
    The igemm dgrad needs unpadded input channels; the depthwise dgrad has no shortcut BN."""
    if prod is None or not dx:
        return None
    if u.depthwise:
        return prod.name if prod_sc is None else None
    sp = mp.spec[u.name]
    return prod.name if sp.Cp == sp.C else None


def _bwd_sc_ok(mp, opts, u, sc):
    """Can the shortcut ``sc``'s backward share one launch with ``u``'s (ops.conv_bwd_sc)?"""
    if not opts.dual_bwd or u.depthwise or sc.depthwise:
        return False
    su, ss = mp.spec[u.name], mp.spec[sc.name]
    if su.stride != 1 or su.K % 8 or ss.K % 8 or not conv.dgrad_s2_ok(ss) or ss.N > 32:
        return False
    return (tuple(mp.plan[u.name, 'dgrad'][:2]) == (64, 64) and
            tuple(mp.plan[u.name, 'wgrad'][:2]) in ((64, 64), (128, 128)) and
            tuple(mp.plan[sc.name, 'wgrad'][:2]) == (64, 64))


BwdSchedule = namedtuple('BwdSchedule', 'parts head_bw')


def backward_schedule(lw, mp, opts):
    """``parts[bi]``: block ``bi``'s backward as [(unit index, [BwdStep])], last unit first
    (after part i the gradients of units i..last, of the BNs of units i-1..last and of the
    shortcut are final); ``head_bw``: the head's backward is handed the last BN's sums."""
    nblk = len(lw.blocks)
    head_bw = bool(opts.head_bw and not lw.blocks[-1].pool and lw.head_pool != 'mlp2')
    parts = {}
    final = 'head' if head_bw else 'pass'      # who reduces the sums of the block's last BN
    for bi in range(nblk - 1, -1, -1):
        blk = lw.blocks[bi]
        units, sc = blk.units, blk.shortcut
        last = units[-1]
        has_dx = bi > 0 and blk.need_dx
        # the shortcut's backward runs in ONE launch with the last conv's (both start from the
        # block-final BN's backward; EngineOptions.dual_bwd)
        merge = sc is not None and has_dx and len(units) > 1 and _bwd_sc_ok(mp, opts, last, sc)
        parts[bi] = []
        for i in range(len(units) - 1, -1, -1):
            u = units[i]
            st = []
            if u is last:
                if blk.pool:
                    st.append(BwdStep('pool_bwd', bi, u.name))
                st.append(BwdStep('bn_bwd', bi, u.name, sc.name if sc else None, reduce=final,
                                  dx='block' if blk.identity and has_dx else None))
                if sc is not None and not merge:
                    st.append(BwdStep('conv_bwd', bi, sc.name, dx='block' if has_dx else None,
                                      kind=_bwd_kind(mp, opts, sc, has_dx)))
            if i > 0:
                bw = _bw_unit(mp, u, True, units[i - 1])
                pair = merge and u is last
                st.append(BwdStep('conv_bwd', bi, u.name, sc.name if pair else None,
                                  'pair_sc' if pair else _bwd_kind(mp, opts, u, True), 'da',
                                  bw=bw))
                st.append(BwdStep('bn_bwd', bi, units[i - 1].name,
                                  reduce='dgrad' if bw else 'pass'))
            else:
                dx = has_dx and u.need_dgrad
                bw = None
                if has_dx and not lw.blocks[bi - 1].pool:
                    # this dgrad is the LAST writer of the previous block's output gradient:
                    # it reduces that block's final BN (+ shortcut BN) sums in its epilogue
                    pb = lw.blocks[bi - 1]
                    bw = _bw_unit(mp, u, dx, pb.units[-1], pb.shortcut)
                st.append(BwdStep('conv_bwd', bi, u.name, None, _bwd_kind(mp, opts, u, dx),
                                  'block' if dx else None,
                                  acc=bool(blk.identity or sc is not None), bw=bw))
                final = 'dgrad' if bw else 'pass'
            parts[bi].append((i, st))
    return BwdSchedule(parts, head_bw)
