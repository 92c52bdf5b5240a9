"""Halo-tile forward convolution (csrc/hconv.hip): geometry, LDS pitch and launch.

A block's output tile is IMG whole images (IMG * P * Q rows) or TR whole output rows of one
image (TR * Q rows), so the input one 64-channel slice of the tile reads is a rectangle -- the
halo -- staged into LDS once and read by all R*R taps.  The producer's BatchNorm (+ identity
residual or shortcut BatchNorm) + activation is applied while staging (``pro``), so a ResNet
forward needs no standalone bn_apply pass between convs.

Reference: the conv/BN/ReLU stack of `pytorch_model.py:19-36,72-97`.
"""
from __future__ import annotations

import math

import torch

from . import _chk, lib, ptr, stream_ptr
from .conv import _ACT, ConvSpec, slab_bytes

HRMAX_PIX = 512                 # halo pixels per tile (csrc/hconv.hip HRMAX pieces x 32 pixels)
LDS_MAX = 160 * 1024            # one workgroup may take the whole 160 KiB of a CU
NSLOT = 3                       # weight ring slots (csrc/hconv.hip)
PSLOT = 6                       # persistent kernel's weight ring (csrc PSLOT)
PERSIST_TILES = ((256, 64), (128, 64), (64, 64))   # (BN = 128 rings exceed 160 KiB)
TILES = ((256, 64, 4), (128, 64, 2), (64, 64, 1), (256, 128, 4), (128, 128, 2), (64, 128, 1))
_WM = {(bm, bn): wm for bm, bn, wm in TILES}

# ds_read_b128 lane groups (MI355X_MICROARCH.md §LDS): one LDS cycle per group when its 16
# lanes hit 16 distinct 16-byte bank quads
_GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
           [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
_GROUPS = _GROUPS + tuple([l + 32 for l in g] for g in _GROUPS)


def supported(spec: ConvSpec):
    """3x3 convs (stride 1 or 2, pad 1) on 64-channel slices with whole 64/128-column weight
    tiles; 1x1 convs stay on igemm."""
    return (spec.R == spec.S == 3 and spec.stride in (1, 2) and spec.C % 64 == 0
            and spec.pad == 1 and spec.Cp == spec.C and spec.K % 64 == 0
            and (spec.K <= 64 or spec.K % 128 == 0))


def persist_table_bytes(spec: ConvSpec, pro):
    """LDS of the persistent kernel's BN table (BN-applying input): G x C scale / shift."""
    if pro is None:
        return 0
    G = spec.N // (pro.get('group_imgs') or spec.N) if pro.get('stats') is not None else 1
    return G * spec.C * 8


def lds_bytes(g, bm, bn, splits):
    """Dynamic LDS of one block (csrc/hconv.hip launch_one): one halo buffer per tile, two when
    a block walks several 64-channel slices (the next slice's halo is prefetched), the weight
    ring, a 4 KB DMA sink; at least the epilogue's staging area.  ``splits == 0`` is the
    persistent kernel (launch_persist): two halo buffers (each large enough to stage the
    epilogue), a 4-slot ring and the sink."""
    nch = g['C'] // 64
    hbytes = -(-g['HPIX'] // 32) * 32 * 128
    red = 16 * bn * 4 + bm * (bn + 8) * 2
    if splits == 0:
        nw = persist_waves()
        ppx = 8 * nw                           # halo pixels per DMA piece
        hbytes = -(-g['HPIX'] // ppx) * ppx * 128
        if hbytes < red:                       # a halo buffer doubles as the epilogue's staging
            return 1 << 30
        return 2 * hbytes + PSLOT * bn * 128 + nw * 1024
    per = -(-nch // max(1, min(splits, nch)))
    main = (2 if per > 1 else 1) * hbytes + NSLOT * bn * 128 + 4096
    return max(main, red)


# engine-selected settings (config.EngineOptions via ``configure``)
_CFG = dict(persist=True, plans='', waves=8, grid=0, row='score', wm8=0, swa=True, pad=True)


def configure(opts):
    """Take the halo-kernel switches of an ``EngineOptions`` (Python side only: plan building
    reads them; ``configure_launcher`` hands the C++ launcher its share)."""
    _CFG.update(persist=bool(opts.hconv_persist), plans=opts.hconv_plans or '',
                waves=8 if opts.hconv_persist_waves == 8 else 4,
                grid=int(opts.hconv_persist_grid), row=opts.hconv_row,
                wm8=int(opts.hconv_persist_wm8), swa=bool(opts.hconv_swa),
                pad=bool(opts.hconv_pad))


def configure_launcher():
    """The persistent kernel's grid and wave count of the last ``configure``, to the C++
    launcher."""
    lib().hconv_configure(_CFG['grid'], _CFG['waves'], _CFG['wm8'])


def persist_waves():
    """Waves per persistent block (the C++ launcher uses the same value: ``configure``)."""
    return _CFG['waves']


# row-step persistent kernel (csrc/hconv.hip hrow_kernel): plans (256, 64, -1), 8 waves;
# stride-1 3x3 convs, plain input
ROW_TILES = ((256, 64),)


def row_lds_bytes(g, bm, bn, splits):
    """Dynamic LDS of the row-step kernel: two halo buffers (8-pixel pieces) and a ring of
    filter rows (3 taps x bn channel rows x 64 channels): 3 slots when the weights are
    stationary (C = K = bn), else 2."""
    nw = 8
    p8 = -(-g['HPIX'] // 8)
    hb = p8 * 8 * 128
    if -(-p8 // nw) > 8 or hb < 2 * (bm // 64) * bn * 4:
        return 1 << 30
    stat = g['C'] == 64 and g['K'] == bn
    return 2 * hb + (3 if stat else 2) * 3 * bn * 128


def row_ok(spec: ConvSpec, bm, bn, stats=True, bias=None, pro=None):
    """The row-step kernel runs this conv: stride-1 3x3, plain input or the input's BN +
    activation (no residual, no kept activation), no bias, whole tiles, ghost-BN groups made of
    whole tiles."""
    if pro is not None and any(pro.get(k) is not None for k in ('res', 'y2', 'keep')):
        return False      # rejected by _pro_args too
    if bias is not None or (bm, bn) not in ROW_TILES:
        return False
    if spec.stride != 1 or spec.R != 3 or spec.M % bm or spec.K % bn:
        return False
    # the kernel's address arithmetic (csrc/hconv.hip hrow_kernel): a halo slot packs its byte
    # offset inside the tile's images into 26 bits and its halo row into the 6 above (63 =
    # padding), the tile base is an int, the buffer resource's size an unsigned
    ts = _tile_shape(spec, bm)
    if ts is None:
        return False
    img, tr = ts
    halo_rows = (tr if img == 1 else spec.P) + 2
    if halo_rows >= 63 or img * spec.H * spec.W * spec.C * 2 >= (1 << 26):
        return False
    if spec.Mx * spec.C * 2 >= (1 << 31):
        return False
    return not stats or spec.group % bm == 0


def persistent_ok(spec: ConvSpec, bm, bn, stats=True, bias=None, pro=None):
    """The persistent kernel runs this conv (else the launcher falls back to the per-tile
    kernel): plain input or the input's BN + activation (no residual, no kept activation), no
    bias, whole tiles (of whole image rows, padded to ``bm`` where none fills it), ghost-BN groups
    made of whole tiles."""
    if pro is not None and any(pro.get(k) is not None for k in ('res', 'y2', 'keep')):
        return False      # rejected by _pro_args too
    if bias is not None or (bm, bn) not in PERSIST_TILES:
        return False
    ts = _tile_shape(spec, bm, pad=True)
    if ts is None:
        return False
    vr = ts[0] * ts[1] * spec.Q
    if spec.M % vr or spec.K % bn:
        return False
    return not stats or spec.group % vr == 0


# padded tiles whose valid rows are below this fraction of BM are not offered
PAD_MIN = 0.75


def _tile_shape(spec: ConvSpec, bm, pad=False):
    """(IMG, TR) for a BM-row tile, or None.  ``pad`` (the persistent kernel): when no whole
    image / whole-row count fills BM exactly, the largest that fits (ResNet-50's 56- and 28-wide
    images: 2 x 56 or 4 x 28 = 112 rows of a 128-row tile); the kernel drops the padding rows."""
    P, Q = spec.P, spec.Q
    PQ = P * Q
    grp_imgs = spec.group_rows // PQ if spec.group_rows else spec.N
    if bm >= PQ:
        if bm % PQ and not pad:
            return None
        img = bm // PQ
        while img > 1 and (spec.N % img or grp_imgs % img):
            img -= 1               # a tile's images share one ghost-BN group
        if spec.N % img or grp_imgs % img or img * PQ < (PAD_MIN * bm if pad else bm):
            return None
        return img, P
    if bm % Q and not pad:
        return None
    tr = bm // Q
    while tr > 1 and P % tr:
        if not pad:
            return None
        tr -= 1
    if P % tr or tr * Q < (PAD_MIN * bm if pad else bm):
        return None
    return 1, tr


def _conflict_cycles(g, bm, bn):
    """LDS cycles of every A-fragment ds_read_b128 of one 64-channel slice (all taps), by the
    lane-group model: each group costs its maximum multiplicity over 16-byte bank quads."""
    wm = _WM[bm, bn]
    TM = bm // (16 * wm)
    IMG, TR, Q, SR, HWP, HALF, R = g['IMG'], g['TR'], g['Q'], g['SR'], g['HWP'], g['HALF'], g['R']
    swa = g.get('SWA', 0)
    per_img = g['HT'] * HWP
    cyc = 0
    vr = IMG * TR * Q
    for w in range(wm):
        for tm in range(TM):
            pix = []
            for l in range(16):
                row = w * (bm // wm) + tm * 16 + l
                row = row if row < vr else 0           # padding rows (the kernel's clamp)
                img, rem = divmod(row, TR * Q)
                tr, q = divmod(rem, Q)
                hc = q * SR
                col = ((hc & 1) * HALF + (hc >> 1)) if HALF else hc
                pix.append(img * per_img + tr * SR * HWP + col)
            for t in range(R * R):
                r, s = divmod(t, R)
                toff = r * HWP + ((s >> 1) + (s & 1) * HALF if HALF else s)
                for kk in range(2):
                    for grp in _GROUPS:
                        seen = {}
                        for lane in grp:
                            p = pix[lane & 15] + toff
                            c = kk * 4 + (lane >> 4)
                            sw = (p + swa * ((p % per_img) // HWP)) & 7
                            u = (p * 8 + (c ^ sw)) % 16
                            seen[u] = seen.get(u, 0) + 1
                        cyc += max(seen.values())
    return cyc


def geometry(spec: ConvSpec, bm, bn, swa=False, pad=False):
    """HconvGeom as a dict (csrc/igemm.h), or None when this tile does not fit the conv.

    The halo image stores pixel p's 64-channel slice as 8 16-byte chunks, logical chunk c at
    slot c ^ swz(p) with swz(p) = (p + SWA * halo_row(p)) & 7.  The row pitch HWP and (for the
    per-tile kernel, ``swa=True``) the row term SWA are chosen by the lane-group model so the
    A-fragment reads are bank-conflict-free: for layer4's 4x4 images the pitch-6 image with
    SWA = 0 costs 2x the ideal LDS cycles (PMC: 2.03 conflict cycles per LDS instruction in
    hconv_kernel<128,128,2>), SWA = 6 none.  The persistent / row-step kernels take SWA = 0;
    ``pad`` allows the persistent kernel's padded row tiles (``_tile_shape``)."""
    if not supported(spec) or (bm, bn) not in _WM:
        return None
    ts = _tile_shape(spec, bm, pad)
    if ts is None:
        return None
    IMG, TR = ts
    R, st = spec.R, spec.stride
    if R == 1 and st == 2:
        HS, SR = 2, 1                          # only the even input pixels are ever read
        HT, HWd = TR, spec.Q
    else:
        HS, SR = 1, st
        HT, HWd = (TR - 1) * st + R, (spec.Q - 1) * st + R
    g = dict(N=spec.N, H=spec.H, W=spec.W, C=spec.C, P=spec.P, Q=spec.Q, K=spec.K, R=R,
             stride=st, pad=spec.pad, IMG=IMG, TR=TR, HT=HT, HWd=HWd, HS=HS, SR=SR, PGRID=0)
    best = None
    halves = [0] if SR == 1 else [(HWd + 1) // 2 + d for d in range(0, 9)]
    for half in halves:
        base = max(HWd, half + HWd // 2) if half else HWd
        for hwp in range(base, base + 17):
            hp = IMG * HT * hwp
            if hp > HRMAX_PIX:
                break
            for sa in (range(8) if swa else (0,)):
                g.update(HWP=hwp, HALF=half, HPIX=hp, SWA=sa)
                c = _conflict_cycles(g, bm, bn)
                key = (c, hp, sa)
                if best is None or key < best[0]:
                    best = (key, dict(g))
    return None if best is None else best[1]


_GEO_CACHE = {}


def geometry_cached(spec: ConvSpec, bm, bn, swa=False, pad=False):
    swa = bool(swa) and _CFG['swa']
    key = (spec.N, spec.H, spec.W, spec.C, spec.K, spec.R, spec.stride, spec.pad,
           spec.group_rows, bm, bn, swa, bool(pad))
    if key not in _GEO_CACHE:
        _GEO_CACHE[key] = geometry(spec, bm, bn, swa, pad)
    return _GEO_CACHE[key]


# PGRID: the persistent kernel's grid for this launch (0: the configured default, half the CUs)
_ORDER = ('N', 'H', 'W', 'C', 'P', 'Q', 'K', 'R', 'stride', 'pad', 'IMG', 'TR', 'HT', 'HWd',
          'HWP', 'HALF', 'HS', 'SR', 'HPIX', 'SWA', 'PGRID')


def plan(spec: ConvSpec, min_blocks=256):
    """(bm, bn, splits) for hconv, or None.  Larger tiles first (fewer halo re-reads per FLOP);
    split the 64-channel slices when the grid would leave CUs idle."""
    bn = 64 if spec.K <= 64 else 128
    for bm in (256, 128, 64):
        if (bm, bn) not in _WM:
            continue
        g = geometry_cached(spec, bm, bn, swa=True)
        if g is None or lds_bytes(g, bm, bn, 1) > LDS_MAX:
            continue
        blocks = math.ceil(spec.M / bm) * math.ceil(spec.K / bn)
        if blocks >= min_blocks or bm == 64:
            break
    else:
        return None
    g = geometry_cached(spec, bm, bn, swa=True)
    if g is None:
        return None
    blocks = math.ceil(spec.M / bm) * math.ceil(spec.K / bn)
    nch = spec.C // 64
    splits = 1
    if blocks < min_blocks * 3 // 4 and nch >= 2 and blocks <= 1024:
        splits = min(nch, math.ceil(min_blocks / blocks), 8)
    if lds_bytes(g, bm, bn, splits) > LDS_MAX:
        return None
    return bm, bn, splits


# Measured winners (bench/hconv_sweep.py, graph-timed, MI355X; profiles/r2/hconv_sweep_b*.jsonl):
# stride-1 3x3 convs of the CIFAR ResNets, keyed (N, H, C, K) -> (bm, bn, splits).  On these the
# halo conv beats the generic implicit GEMM by 2-30 % (B=320 layer4 46 vs 66 us); on stride-2
# convs it does not, so those stay on igemm.
MEASURED = {
    (320, 32, 64, 64): (128, 64, 1), (320, 16, 128, 128): (128, 64, 2),
    (320, 8, 256, 256): (256, 128, 1), (320, 4, 512, 512): (128, 128, 1),
    (32, 32, 64, 64): (256, 64, 1), (32, 16, 128, 128): (64, 64, 1),
    (32, 8, 256, 256): (64, 64, 2), (32, 4, 512, 512): (64, 64, 4),
}
# shapes that stay on igemm in the engine although a halo plan exists: the train-batch layer4
# conv (1.5011 vs 1.5058 ms/step over 3 same-box rounds, profiles/r2/ab_train_l4.json)
MEASURED_IGEMM = {(32, 4, 512, 512)}


# Persistent-kernel winners (splits 0; bench/hconv_sweep.py at B=320, profiles/r2/
# hconv_sweep_b320_persistent.jsonl): layer1 38.7 vs 53.9 us (best per-tile plan), layer2 35.4
# vs 39.6, layer3 39.9 vs 40.9, the layer3 -> 4 stride-2 conv 33.6 vs igemm's 36.9 us.
MEASURED_PERSIST = {
    (320, 32, 64, 64): (256, 64, 0), (320, 16, 128, 128): (256, 64, 0),
    (320, 8, 256, 256): (128, 64, 0),
    # train batch (one or two tiles per block: the 8-wave slice pipeline, not the tile stream,
    # is what helps here): step 1.536 -> 1.521 ms same-box (profiles/r2/ab_train_persist.json)
    (32, 32, 64, 64): (256, 64, 0), (32, 16, 128, 128): (128, 64, 0),
    (32, 8, 256, 256): (64, 64, 0),
}
# (the layer3 -> 4 stride-2 scoring conv left the persistent kernel in round 5: on igemm it runs
# in one launch with its 1x1 shortcut (igemm_dual), 1.2922-1.2981 vs 1.2976-1.3026 ms/step,
# scoring solo 1.013 vs 1.027-1.031 ms, profiles/r5/ab_l4_s2/ab.json)
MEASURED_PERSIST_S2 = {}


def _plan_override(key):
    """EngineOptions.hconv_plans = "N,H,C,K=bm,bn,splits;..." (A/B runs): a plan for that
    shape, or 'none' for igemm.  Returns (found, plan)."""
    for item in filter(None, _CFG['plans'].split(';')):
        k, v = item.split('=')
        if tuple(int(t) for t in k.split(',')) == key:
            return True, (None if v == 'none' else tuple(int(t) for t in v.split(',')))
    return False, None


# Row-step kernel plans: the weight-stationary layer1 scoring conv 51.6 vs 60.4 us on the
# per-tap persistent kernel (bench/hrow_bench.py, graph-timed at the engine's 128-block grid,
# profiles/r5/hrow_bench_v3.jsonl); layer2 53.1 vs 52.1 in isolation, but with the intra-block
# BN folded into both kernels' halos the step is faster with it on the row-step kernel
# (1.307 vs 1.333 ms/step, profiles/r5/ab_persist_bn_scope.json)
MEASURED_ROW = {(320, 32, 64, 64): (256, 64, -1), (320, 16, 128, 128): (256, 64, -1)}

# Padded-row persistent plans: ResNet-50's stride-1 3x3 convs (56/28/14/7-wide images, no
# whole-row 64/128/256-pixel tile), keyed (N, H, C, K) -> (plan, input BN in the halo staging).
# The 4th plan element is the launch's grid: all 256 CUs (these run at B = 1280 / 128, not beside
# a latency-bound train chain).  bench/hconv_r50_bench.py, graph-timed (profiles/r6/
# hconv_r50.jsonl), us: scoring B = 1280 layer1 441.6 vs igemm 586 (with its input BN folded
# 518 vs 586 + a 188 us bn_apply pass), layer3 354 vs 406; train B = 128 layer1 53.8 vs 88.5,
# layer2 50.1 vs 65.5, layer3 44.4 vs 53.4, layer4 44.0 vs 68.7.  With the 16-byte epilogue
# stores (hc_perm; profiles/r6/hconv_perm/) scoring layer2 398-404 vs the engine's tuned igemm
# ~420 joined; layer4 scoring stays on igemm (363 vs 335), and the folded BN only pays at
# layer1 (layer2 568 vs 415 + 100, layer3 596 vs 354 + 42: the transform runs once per N tile)
MEASURED_PAD = {
    (1280, 56, 64, 64): ((256, 64, 0, 256), True),
    (1280, 28, 128, 128): ((256, 64, 0, 256), False),
    (1280, 14, 256, 256): ((256, 64, 0, 256), False),
    (128, 56, 64, 64): ((256, 64, 0, 256), False),
    (128, 28, 128, 128): ((256, 64, 0, 256), False),
    (128, 14, 256, 256): ((256, 64, 0, 256), False),
    (128, 7, 512, 512): ((256, 64, 0, 256), False),
}


def _pad_plan(spec: ConvSpec, bias=False):
    """(plan, bn_ok) of MEASURED_PAD for this conv when it runs there, else None."""
    if not _CFG['pad'] or bias or spec.H != spec.W or spec.stride != 1:
        return None
    e = MEASURED_PAD.get((spec.N, spec.H, spec.C, spec.K))
    if e is None:
        return None
    p = e[0]
    g = geometry_cached(spec, p[0], p[1], pad=True)
    if g is None or lds_bytes(g, p[0], p[1], 0) > LDS_MAX or not persistent_ok(spec, p[0], p[1]):
        return None
    return e


def engine_plan(spec: ConvSpec, bias=False, train=None):
    """The plan the engine runs hconv with for this conv, or None (use igemm): measured
    persistent-kernel winners (EngineOptions.hconv_persist=0 turns them off), measured per-tile
    winners, else the heuristic for stride-1 3x3 convs with >= 128 channels (where it won every
    measured shape)."""
    if not supported(spec):
        return None
    found, p = _plan_override((spec.N, spec.H, spec.C, spec.K))
    pp = None if found else _pad_plan(spec, bias)
    if pp is not None:
        return pp[0]
    if found and spec.H == spec.W:
        if p is None:
            return None
        g = geometry_cached(spec, p[0], p[1], swa=p[2] > 0)
        if g is not None and lds_bytes(g, *p) <= LDS_MAX and (p[2] != 0 or (
                not bias and persistent_ok(spec, p[0], p[1]))):
            return p
    # (the measured tables are keyed by the square CIFAR shapes)
    key = (spec.N, spec.H, spec.C, spec.K) if spec.H == spec.W else None
    row = _CFG['row']
    if key in MEASURED_ROW and not bias and (row == '1' or (row == 'score' and train is False)
                                             or (row == 'train' and train is True)):
        p = MEASURED_ROW[key]
        g = geometry_cached(spec, p[0], p[1])
        if g is not None and row_ok(spec, p[0], p[1]) and row_lds_bytes(g, *p) <= LDS_MAX:
            return p
    if _CFG['persist'] and not bias and key is not None:
        p = (MEASURED_PERSIST if spec.stride == 1 else MEASURED_PERSIST_S2).get(key)
        if p is not None and persistent_ok(spec, p[0], p[1]):
            g = geometry_cached(spec, p[0], p[1])
            if g is not None and lds_bytes(g, *p) <= LDS_MAX:
                return p
    if spec.stride != 1 or key in MEASURED_IGEMM:
        return None
    p = MEASURED.get(key)
    if p is not None:
        g = geometry_cached(spec, p[0], p[1], swa=True)
        if g is not None and lds_bytes(g, *p) <= LDS_MAX:
            return p
    if spec.C >= 128:
        return plan(spec)
    return None


def persist_bn_plan(spec: ConvSpec, group_imgs, row_only=False, stat_only=False):
    """The persistent plan with the input's BN + activation in the halo staging (no residual),
    or None: the row-step kernel where it runs this conv, else (unless ``row_only``) the per-tap
    persistent kernel.  Scoring pass only (EngineOptions.persist_bn, engine)."""
    pp = _pad_plan(spec)
    if pp is not None:
        # padded-row plan: the table says whether the fold pays
        if not pp[1]:
            return None
        g = geometry_cached(spec, pp[0][0], pp[0][1], pad=True)
        pro = dict(stats=True, group_imgs=group_imgs)
        if lds_bytes(g, pp[0][0], pp[0][1], 0) + persist_table_bytes(spec, pro) > LDS_MAX:
            return None
        return pp[0]
    p = engine_plan(spec, train=False)
    if p is not None and p[2] < 0:
        # stat_only: only where the row-step kernel keeps its weights stationary (C = K = 64,
        # one slice, one channel tile: each halo element is transformed once per tile).  With
        # several slices x channel tiles the transform runs once per (slice, channel tile) pass
        # on the slice's critical path
        if stat_only and not (spec.C == 64 and spec.K == p[1]):
            return None
        return p
    if row_only:
        return None
    if p is None or p[2] != 0:
        return None
    pro = dict(stats=True, group_imgs=group_imgs)
    g = geometry_cached(spec, p[0], p[1])
    if g is None or lds_bytes(g, *p) + persist_table_bytes(spec, pro) > LDS_MAX:
        return None
    return p


def _pro_args(pro, spec):
    """HconvPro from a dict: the input's BatchNorm + activation (mode 1) -- the producer's stats
    [G][2][C] (or rmean/rvar), gamma, beta, act, eps, count (pixels per stat group), group_imgs.
    The persistent kernels take no residual, second BN or kept activation: the per-tile
    kernel's staged modes that did measured slower than a bn_apply pass
    (profiles/r2/ab_fuse_bn_halo.json) and were removed in round 5."""
    if pro is None:
        return (0, 0, 0, 0, 0, 0, 1, 1.0, 1e-5, 0)
    bad = [k for k in ('res', 'y2', 'keep') if pro.get(k) is not None]
    if bad:
        raise ValueError('hconv: the staged prologue takes no %s' % ', '.join(bad))
    for k in ('stats', 'rmean', 'rvar', 'gamma', 'beta'):
        _chk(pro.get(k), torch.float32, 'pro.' + k)
    if pro.get('stats') is None and pro.get('rmean') is None:
        raise ValueError('pro needs stats or running statistics')
    gi = pro.get('group_imgs') or spec.N
    return (1, ptr(pro.get('stats')), ptr(pro.get('rmean')), ptr(pro.get('rvar')),
            ptr(pro['gamma']), ptr(pro['beta']), gi, 1.0 / float(pro.get('count', 1)),
            float(pro.get('eps', 1e-5)), _ACT[pro.get('act')])


def _hconv_args(x, w, out, bias, stats, spec: ConvSpec, slab, g, plan_):
    """hconv's arguments up to the stream (csrc/bindings.cpp); ``g``: the geometry dict."""
    return (ptr(x), ptr(w), ptr(out), ptr(bias), ptr(stats), spec.group,
            ptr(slab) if plan_[2] > 1 else 0, [int(g[k]) for k in _ORDER], *plan_[:3])


def hconv_fwd(x, w, out, spec: ConvSpec, plan_=None, stats=None, bias=None, slab=None, pro=None):
    """out[M][K] = conv(pro(x) NHWC, w [K][R][S][C]) with the fused BN-statistics epilogue."""
    _chk(x, torch.bfloat16, 'x', spec.Mx * spec.C)
    _chk(w, torch.bfloat16, 'w', spec.K * spec.R * spec.S * spec.C)
    _chk(out, torch.bfloat16, 'out', spec.M * spec.K)
    _chk(stats, torch.float32, 'stats')
    _chk(bias, torch.float32, 'bias', spec.K)
    p = plan_ or plan(spec)
    if p is None:
        raise ValueError('hconv does not support this conv')
    bm, bn, splits = p[:3]
    g = geometry_cached(spec, bm, bn, swa=splits > 0, pad=splits == 0)
    if g is not None and splits == 0 and len(p) > 3 and p[3]:
        g = dict(g, PGRID=int(p[3]))              # a plan's own persistent grid
    if splits < 0:
        if g is None or row_lds_bytes(g, bm, bn, splits) > LDS_MAX:
            raise ValueError('hconv: row-step tile %dx%d does not fit this conv' % (bm, bn))
        if not row_ok(spec, bm, bn, stats is not None, bias, pro):
            raise ValueError('hconv: the row-step plan does not take this conv')
    else:
        extra = persist_table_bytes(spec, pro) if splits == 0 else 0
        if g is None or lds_bytes(g, bm, bn, splits) + extra > LDS_MAX:
            raise ValueError('hconv: tile %dx%d does not fit this conv' % (bm, bn))
        if splits == 0 and not persistent_ok(spec, bm, bn, stats is not None, bias, pro):
            raise ValueError('hconv: the persistent plan does not take this conv')
        if pro is not None and splits != 0:
            raise ValueError('hconv: only the persistent plans take the input BN in staging')
        if splits > 1:
            need = slab_bytes(spec.M, spec.K, bm, bn, splits)
            if slab is None or slab.numel() * slab.element_size() < need:
                raise ValueError('hconv: split-K slab too small')
    args = _hconv_args(x, w, out, bias, stats, spec, slab, g, (bm, bn, splits))
    lib().hconv(*args, stream_ptr(), *_pro_args(pro, spec))
    return out
