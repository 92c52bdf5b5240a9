"""fp64 references, integer test data and a mirror of the launch arithmetic of the depthwise
3x3 kernels (csrc/dwconv.hip).

A helper module (no tests, no fixtures); everything here is plain torch in float64, on the CPU
unless it is handed device tensors (the prologue tests run ``bn_ref`` and ``dw_ref`` there).
Activations are NHWC ``[N][H][W][C]``, weights ``[C][3][3]``, the conv is pad 1, stride 1 or 2.

Integer data.  ``int_data`` draws x, w and gy from {-2 .. 2}.  A depthwise output is a sum of
nine products, so y and dx are integers of magnitude <= 36, exact in bf16 (asserted <= 256), and
every sum the kernels form -- dw, the per-group BN sums of y and y^2, the BN-backward sum of
dz -- is an integer below 2^24 (asserted), exact in fp32 in ANY order of additions, LDS
partials, slabs and atomics included.  Those outputs are compared with ``torch.equal``.

The one fused quantity that is not an integer is sum(dz * xhat).  Its criterion is

    |sum - ref| <= K * 2^-24 * sum |dz * xhat|,

K = the additions on the longest way to the sum (``dispatch`` counts them: strips per thread,
256 / C8 partials of the block's LDS fold, the blocks adding into one replica, the SUMS_R
replicas) + 8 for xhat itself.  The 8, in units of 2^-24 relative to a term: rstd <= 4 (1/count
rounded, its product with sum y^2, the subtraction, + eps: 4 on the variance, 2 on its inverse
root, and 2 for a 1-ulp rsqrtf), the mean 2 (1/count and the product; ``int_data`` keeps
|mean| <= 2^-5, so where y != 0 that is 2/31 of the term, and where y == 0 the subtraction
y - mean is exact), the subtraction 1, the two products 2: 8 where y == 0, 7.1 elsewhere.

``dispatch`` is a copy of dwconv_fwd_launch, dwconv_dgrad_launch, dw_qs and
dwconv_wgrad_blocks.  The GPU cases assert the path they were chosen for through it, and the
GPU file checks its ``nblk`` against the library, so a retuned dispatch fails loudly instead
of leaving a case on another path.  It describes the defaults: MERCURY_DW_DH and
MERCURY_DW_STAT_BLOCKS unset.
"""
import torch

F64 = torch.float64
DT = 256            # threads per block
DWL = 4             # outputs per strip
SUMS_R = 8          # replicas of the BN-backward sums
STAT_BLOCKS = 256   # dw_stat_blocks()
DW_RED_MAX = 24     # layers per batched-reduce launch
EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the kernels take eps as a float
U = 2.0 ** -24      # fp32 half ulp, relative
HALF_ULP_BF16 = 2.0 ** -8

# (N, C, H, W, stride, ghost groups); what each reaches is asserted in test_dwconv_oracles.py
EXACT_CASES = [
    (128, 16, 5, 7, 1, 1), (128, 16, 5, 7, 1, 4), (128, 24, 6, 9, 1, 4), (130, 40, 3, 5, 1, 1),
    (128, 16, 1, 1, 1, 1), (1, 8, 1, 1, 1, 1), (1, 8, 2, 3, 2, 1),
    (128, 96, 17, 18, 1, 1),
    (2, 16, 25, 25, 1, 1), (2, 16, 9, 27, 1, 1), (2, 16, 50, 50, 2, 1),
    (32, 144, 31, 33, 1, 1), (32, 144, 32, 32, 2, 1),
]
# (N, C, H, W, stride, group_imgs of the ghost mode); 64 images of 16 x 16 x 96 are 192 forward
# blocks, under the cap of 256: the grid-stride forward with a prologue needs the 96 of the last
PRO_SHAPES = [(4, 40, 5, 11, 1, 2), (6, 24, 8, 12, 2, 3), (128, 16, 5, 7, 1, 32),
              (64, 96, 16, 16, 1, 16), (96, 96, 16, 16, 1, 24)]
# the batched reduce: 26 layers, (C, nblk) cycling with coprime periods (all pairs distinct)
RED_C = (8, 16, 40, 144, 960)
RED_NBLK = (1, 3, 31, 32, 127, 128, 300)
RED_LAYERS = [(RED_C[i % 5], RED_NBLK[i % 7]) for i in range(26)]


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1      # (H + 2 - 3) // stride + 1


# --------------------------------------------------------------------------- references
def dw_ref(x, w, gy, stride):
    """(y, dx, dw) of the pad-1 depthwise 3x3 conv in float64, as nine shifted-slice sums.
    x [N][H][W][C], w [C][3][3], gy [N][P][Q][C] or None (then dx = dw = None)."""
    x, w = x.to(F64), w.to(F64)
    N, H, W, C = x.shape
    P, Q = out_hw(H, W, stride)
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=F64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = torch.zeros(N, P, Q, C, dtype=F64, device=x.device)
    if gy is not None:
        gy = gy.to(F64)
        dxp = torch.zeros_like(xp)
        dw = torch.zeros(C, 3, 3, dtype=F64, device=x.device)
    for r in range(3):
        for t in range(3):
            rows = slice(r, r + (P - 1) * stride + 1, stride)
            cols = slice(t, t + (Q - 1) * stride + 1, stride)
            y += xp[:, rows, cols] * w[:, r, t]
            if gy is not None:
                dw[:, r, t] = (xp[:, rows, cols] * gy).sum((0, 1, 2))
                dxp[:, rows, cols] += gy * w[:, r, t]
    if gy is None:
        return y, None, None
    return y, dxp[:, 1:H + 1, 1:W + 1].contiguous(), dw


def act_ref(v, act):
    if act == 'relu':
        return v.clamp(min=0.0)
    if act == 'relu6':
        return v.clamp(0.0, 6.0)
    assert act in (None, 'none')
    return v


def act_mask(out, act):
    if act == 'relu':
        return (out > 0).to(F64)
    if act == 'relu6':
        return ((out > 0) & (out < 6)).to(F64)
    assert act in (None, 'none')
    return torch.ones_like(out, dtype=F64)


def bn_ref(y, gamma, beta, act, stats=None, count=None, group_imgs=None, rmean=None, rvar=None,
           eps=EPS):
    """The input prologue act(bn(y)) in float64: (a, |y * sc|, |sh|), each [N][H][W][C].
    Batch or ghost statistics: ``stats`` [G][2][C] (sum, sum of squares over ``count`` values,
    groups of ``group_imgs`` images; the variance clamped at 0); running: ``rmean``, ``rvar``."""
    y = y.to(F64)
    N, C = y.shape[0], y.shape[-1]
    if stats is not None:
        st = stats.to(F64).reshape(-1, 2, C)
        mean = st[:, 0] / count
        var = (st[:, 1] / count - mean * mean).clamp(min=0.0)
        gi = group_imgs or N
        assert st.shape[0] == cdiv(N, gi)
        idx = torch.arange(N, device=y.device) // gi
        mean, var = mean[idx], var[idx]                      # [N][C]
    else:
        mean = rmean.to(F64).expand(N, C)
        var = rvar.to(F64).expand(N, C)
    sc = gamma.to(F64) / torch.sqrt(var + eps)
    sh = beta.to(F64) - mean * sc
    sc, sh = sc[:, None, None, :], sh[:, None, None, :]
    ysc = y * sc
    return act_ref(ysc + sh, act), ysc.abs(), sh.abs().expand_as(ysc)


def bn_bwd_ref(dx, out, y, stats, act, eps=EPS):
    """The BN-backward sums the dgrad fuses, in float64: dz = dx * act'(out);
    (sum dz, sum dz * xhat, sum |dz * xhat|) per channel.  dx, out, y [M][C]; stats [2][C] the
    sum and sum of squares of y (one batch group)."""
    dx, out, y, st = dx.to(F64), out.to(F64), y.to(F64), stats.to(F64)
    M = y.shape[0]
    mean = st[0] / M
    rstd = 1.0 / torch.sqrt((st[1] / M - mean * mean).clamp(min=0.0) + eps)
    dz = dx * act_mask(out, act)
    t = dz * ((y - mean) * rstd)
    return dz.sum(0), t.sum(0), t.abs().sum(0)


# --------------------------------------------------------------------------- integer data
def case_act(case):
    """The activation of the BN feeding the conv in a case's ``bw=`` runs (every act_mask arm)."""
    return {16: 'relu', 8: 'none'}.get(case[1], 'relu6')


def int_data(case, seed=0):
    """Integer operands and exact float64 references of one EXACT_CASES entry (a dict).

    x, w, gy in {-2 .. 2}; ``dw0`` in {-3 .. 3}: what dw holds before a wgrad adds to it.  For
    the ``bw=`` runs: ``yin`` (the feeding BN's input) in antisymmetric pairs, so a channel's
    sum is 0, plus (c % 5) - 2 on one pixel where the image set has >= 64 pixels: a mean that
    is not zero, differs between channels and stays under 2^-5 (module docstring); ``out``
    from {-1, 0, 1, 3, 6, 7}, on and beside both relu6 bounds, so the mask is exactly 0 or 1."""
    N, C, H, W, stride, G = case
    g = torch.Generator().manual_seed(1000 + seed)
    P, Q = out_hw(H, W, stride)

    def ri(*shape, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F64)

    x, w, gy = ri(N, H, W, C), ri(C, 3, 3), ri(N, P, Q, C)
    y, dx, dw = dw_ref(x, w, gy, stride)
    dw0 = ri(C, 3, 3, lo=-3, hi=3)
    assert N % G == 0
    yg = y.reshape(G, -1, C)
    stats = torch.stack([yg.sum(1), (yg * yg).sum(1)], 1)           # [G][2][C]
    M = N * H * W
    half = ri((M + 1) // 2, C)
    yin = torch.cat([half, -half])[:M][torch.randperm(M, generator=g)]
    if M >= 64:
        yin[0] += (torch.arange(C) % 5 - 2).to(F64)
    out = torch.tensor([-1., 0., 1., 3., 6., 7.], dtype=F64)[
        torch.randint(0, 6, (M, C), generator=g)]
    act = case_act(case)
    st_in = torch.stack([yin.sum(0), (yin * yin).sum(0)])            # [2][C]
    sdz, sxh, sabs = bn_bwd_ref(dx.reshape(M, C), out, yin, st_in, act)
    # exactness: bf16 holds the activations, fp32 every sum
    for t in (x, gy, yin, out):
        assert t.abs().max() <= 256
    assert y.abs().max() <= 256 and dx.abs().max() <= 256
    for t in (w, dw, dw0, dw + dw0, stats, st_in, sdz):
        assert t.abs().max() < 2 ** 24
    assert M == 1 or (st_in[0] / M).abs().max() <= 2.0 ** -5
    return dict(case=case, P=P, Q=Q, M=M, x=x, w=w, gy=gy, y=y, dx=dx, dw=dw, dw0=dw0,
                stats=stats, yin=yin, out=out, act=act, st_in=st_in, sdz=sdz, sxh=sxh, sabs=sabs)


# --------------------------------------------------------------------------- dispatch mirror
def dw_qs(N, P, Q, C):
    rows = N * P * (C // 8)
    QS = 1
    while rows * QS < 256 * 4 * 64 and (Q + 2 * QS - 1) // (2 * QS) >= 4:
        QS *= 2
    return QS


def red_shares(nblk):
    return 8 if nblk >= 128 else (4 if nblk >= 32 else 1)


def dispatch(N, C, H, W, stride, groups=1, stats=True, bw=False):
    """What the launchers do with a shape (defaults; no MERCURY_DW_* override).

    forward : DH, fwd_blocks, loop, fwd_stride, fwd_trips (strips per thread), straddle (blocks
              whose threads span two statistics groups: the global-atomic path), per_img
              (threads per image), fwd_chain (additions on the longest way to a statistic)
    dgrad   : dg_blocks, capped, dg_stride, dg_trips, dg_chain (K of the module docstring)
    wgrad   : QS, QL, empty (column segments without a column, per row), nblk, shares (slab
              path); nblk_atomic (no slab: QS = 1)"""
    P, Q = out_hw(H, W, stride)
    C8 = C // 8
    d = dict(P=P, Q=Q, C8=C8)
    # dwconv_fwd_launch / dw_fwd_kernel
    DH = 2 if stride == 1 and N >= 128 else 1
    per_img = cdiv(P, DH) * cdiv(Q, DWL) * C8
    total = N * per_img
    blocks = cdiv(total, DT)
    assert N % groups == 0
    ipg = N // groups                        # group_rows / (P * Q)
    loop = bool(stats) and ipg >= N and blocks > STAT_BLOCKS
    if loop:
        blocks = STAT_BLOCKS
    T = blocks * DT
    fstride = T - T % C8 if loop else T
    lim = min(total, fstride)
    straddle = 0
    if stats and not loop:
        for b in range(blocks):
            first = (b * DT // per_img) // ipg
            last = (min(lim - 1, b * DT + DT - 1) // per_img) // ipg
            straddle += first != last
    trips = cdiv(total, fstride)
    adders = cdiv(min(ipg * per_img, lim), DT) + 1          # blocks adding into one group
    chain = trips + cdiv(DT, C8) * (3 if straddle else 1) + adders + 1    # + 1: f * f rounds
    d.update(DH=DH, per_img=per_img, fwd_blocks=blocks, loop=loop, fwd_stride=fstride,
             fwd_trips=trips, straddle=straddle, fwd_chain=chain)
    # dwconv_dgrad_launch / dw_dgrad_body
    dtotal = N * H * cdiv(W, DWL) * C8
    dblocks = cdiv(dtotal, DT)
    capped = bool(bw) and dblocks > STAT_BLOCKS
    if capped:
        dblocks = STAT_BLOCKS
    T = dblocks * DT
    dstride = T - T % C8 if bw else T
    dtrips = cdiv(dtotal, dstride)
    d.update(dg_blocks=dblocks, capped=capped, dg_stride=dstride, dg_trips=dtrips,
             dg_chain=dtrips + cdiv(DT, C8) + cdiv(dblocks, SUMS_R) + SUMS_R + 8)
    # dw_qs / dwconv_wgrad_blocks / dw_wgrad_body
    QS = dw_qs(N, P, Q, C)
    QL = cdiv(Q, QS)
    nblk = cdiv(N * P * C8 * QS, DT)
    d.update(QS=QS, QL=QL, empty=sum(seg * QL >= Q for seg in range(QS)), nblk=nblk,
             shares=red_shares(nblk), nblk_atomic=cdiv(N * P * C8, DT))
    return d


# the path every case was chosen for: what dispatch(..., stats=True, bw=True) must say of it
PATHS = {
    (128, 16, 5, 7, 1, 1): dict(DH=2, P=5, fwd_blocks=6, straddle=0, loop=False),
    (128, 16, 5, 7, 1, 4): dict(DH=2, P=5, fwd_blocks=6, straddle=2, loop=False),
    (128, 24, 6, 9, 1, 4): dict(DH=2, P=6, Q=9, straddle=3),
    (130, 40, 3, 5, 1, 1): dict(DH=2, per_img=20, dg_stride=4095, dg_blocks=16),
    (128, 16, 1, 1, 1, 1): dict(DH=2, P=1, Q=1),
    (1, 8, 1, 1, 1, 1): dict(DH=1, P=1, Q=1, C8=1),
    (1, 8, 2, 3, 2, 1): dict(DH=1, P=1, Q=2, C8=1),
    (128, 96, 17, 18, 1, 1): dict(DH=2, loop=True, fwd_blocks=256, fwd_stride=65532, fwd_trips=2,
                                  QS=4, QL=5, nblk=408, shares=8, empty=0),
    (2, 16, 25, 25, 1, 1): dict(QS=8, QL=4, empty=1),
    (2, 16, 9, 27, 1, 1): dict(QS=8, QL=4, empty=1),
    (2, 16, 50, 50, 2, 1): dict(QS=8, QL=4, empty=1, P=25, Q=25),
    (32, 144, 31, 33, 1, 1): dict(capped=True, dg_blocks=256, dg_stride=65520, dg_trips=3),
    (32, 144, 32, 32, 2, 1): dict(capped=True, dg_blocks=256, dg_stride=65520, dg_trips=3),
}


def assert_path(case, d):
    for k, v in PATHS[case].items():
        assert d[k] == v, 'case %s no longer reaches its path: %s is %s, not %s' % (case, k, d[k], v)
