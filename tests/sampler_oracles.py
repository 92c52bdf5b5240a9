"""Plain CPU references for the two samplers (``csrc/importance.hip`` is_sample_kernel and the
importance table of ``csrc/table.hip``): no GPU, numpy and ``fractions`` only.

Every draw of either sampler is a pure function of ``philox4x32(counter, d, stream word; seed,
k1)`` (``csrc/common.h``), so a test that replays the generator knows the uniforms behind draw
``d`` and can say which sample that draw had to be.

* ``philox4x32``            the ten rounds as ``common.h`` writes them (Random123's Philox4x32-10)
* ``u01`` / ``table_u``     the fp32 uniform of the pool sampler, the fp64 uniform of the table
* ``pool_draw_uniforms``    per draw: (bin, second uniform) on the alias path, the CDF uniform else
* ``table_draw_uniforms``   per draw: the table's fp64 uniform in [0, 1)
* ``alias_closed_form``     the alias table the kernel's comment states, in exact arithmetic
* ``alias_fp32_emulation``  the same build in fp32 with the kernel's scan order
* ``cdf_fp32_emulation``    the inverse-CDF path's fp32 CDF with the kernel's scan order
* ``recover_alias_table``   model-free: what (bin, u, idx) alone say about the table that drew them
"""
import bisect
from fractions import Fraction

import numpy as np

U32 = np.uint64(0xffffffff)
IS_T = 1024                       # threads of is_sample_kernel
ALIAS_WORD, CDF_WORD, TABLE_WORD = 0xa11a, 0xd1a5, 0x7ab1e5
POOL_K1, TABLE_K1 = 0x3C6EF372, 0x1B873593
F32 = np.float32
ULP = 2.0 ** -24                  # fp32 unit roundoff


def philox4x32(ctr4, k0, k1):
    """Philox4x32-10.  ``ctr4``: four counter words (ints or arrays, broadcast together);
    returns four uint64 arrays holding 32-bit words."""
    x, y, z, w = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & U32 for c in ctr4])
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * x, m1 * z              # 32 x 32 bits: fits uint64
        x, y, z, w = (p1 >> s32) ^ y ^ k0, p1 & U32, (p0 >> s32) ^ w ^ k1, p0 & U32
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return x, y, z, w


def u01(x):
    """``(x >> 8) * 2**-24`` in fp32 (exact: 24 bits times a power of two)."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def _ctr(counter, n, word):
    counter = int(counter) & 0xffffffffffffffff
    return (counter & 0xffffffff, counter >> 32, np.arange(n, dtype=np.uint64), word)


def pool_draw_uniforms(dc, seed, B, alias, P=None):
    """Draws 0..B-1 of is_sample at draw counter ``dc``.  Alias path: ``(bin, u_y)`` with
    ``bin = min(int(fp32(u01(r.x)) * fp32(P)), P - 1)`` (``P`` required) and the fp32 uniform
    that is compared with the bucket's kept share.  Inverse-CDF path: the fp32 uniform."""
    r = philox4x32(_ctr(dc, B, ALIAS_WORD if alias else CDF_WORD), seed, POOL_K1)
    if not alias:
        return u01(r[0])
    b = np.minimum((u01(r[0]) * F32(P)).astype(np.int64), P - 1)
    return b, u01(r[1])


def table_u(rx, ry, total):
    """table_draw_kernel's uniform, formed as the kernel forms it (every step one fp64
    operation; ``ry * 2**32`` is exact, so a fused multiply-add gives the same bits)."""
    u01d = (rx.astype(np.float64) + ry.astype(np.float64) * 4294967296.0) * (2.0 ** -64)
    return np.minimum(u01d * total, total * (1.0 - 1e-12))


def table_draw_uniforms(counter, seed, ndraw):
    """``(r.x, r.y)`` of every table draw at the snapshot ``counter`` (feed to ``table_u``)."""
    r = philox4x32(_ctr(counter, ndraw, TABLE_WORD), seed, TABLE_K1)
    return r[0], r[1]


# ---- alias table ---------------------------------------------------------------------------
def alias_closed_form(v):
    """``(q, alias)`` of the closed form in is_sample_kernel's comment, in exact arithmetic when
    ``v`` holds ints / Fractions / dyadic floats (floats are converted exactly)."""
    v = [x if isinstance(x, (int, Fraction)) else Fraction(float(x)) for x in v]
    P = len(v)
    tot = sum(v)
    s = [x * P / tot for x in v]
    lights = [i for i in range(P) if s[i] < 1]
    heavies = [i for i in range(P) if s[i] >= 1]
    q, alias = list(s), list(range(P))
    if not heavies:
        return [Fraction(1)] * P, alias
    D, acc = [], Fraction(0)                 # exclusive deficit prefix per light
    for i in lights:
        D.append(acc)
        acc += 1 - s[i]
    dtot = acc
    S, acc = [Fraction(0)], Fraction(0)      # S[k] exclusive excess prefix, S[nh] the total
    for i in heavies:
        acc += s[i] - 1
        S.append(acc)
    nh = len(heavies)
    for j, i in enumerate(lights):           # smallest k with D_i <= S_{k+1}
        alias[i] = heavies[min(bisect.bisect_left(S, D[j], 1) - 1, nh - 1)]
    for k, i in enumerate(heavies):          # first light prefix above S_{k+1}
        j = bisect.bisect_right(D, S[k + 1])
        dn = D[j] if j < len(D) else dtot
        q[i] = Fraction(1) if k == nh - 1 else min(Fraction(1), max(Fraction(0),
                                                                     1 - (dn - S[k + 1])))
        alias[i] = heavies[k + 1] if k + 1 < nh else i
    return q, alias


def implied_distribution(q, alias):
    """The draw probabilities an alias table stands for: ``(q_i + sum_{alias_j == i} (1 - q_j))
    / P``, in the arithmetic of ``q``."""
    P = len(q)
    out = list(q)
    for j in range(P):
        if alias[j] != j:
            out[alias[j]] = out[alias[j]] + (1 - q[j])
    return [x / P for x in out]


def _block_scan_f32(local):
    """is_block_scan over IS_T per-thread values: a 64-lane Hillis-Steele scan per wave, the 16
    wave totals scanned the same way, added back.  fp32 (or integer) in the kernel's order."""
    v = np.array(local).reshape(IS_T // 64, 64)
    for o in (1, 2, 4, 8, 16, 32):
        t = v.copy()
        t[:, o:] = v[:, o:] + v[:, :-o]
        v = t
    wt = v[:, 63].copy()
    for o in (1, 2, 4, 8):
        t = wt.copy()
        t[o:] = wt[o:] + wt[:-o]
        wt = t
    v[1:] = v[1:] + wt[:-1, None]
    return v.reshape(-1)


def _segments(P):
    seg = (P + IS_T - 1) // IS_T
    s0 = np.minimum(P, np.arange(IS_T) * seg)
    return seg, s0, np.minimum(P, s0 + seg)


def _serial_prefix(vals, P):
    """(exclusive prefix per item, block total) of fp32 ``vals`` as the kernel forms it:
    per-thread serial segment sums, block scan, then a serial walk from the thread's offset."""
    seg, s0, s1 = _segments(P)
    local = np.zeros(IS_T, F32)
    for k in range(seg):
        i = s0 + k
        m = i < s1
        local[m] = local[m] + vals[i[m]]
    scan = _block_scan_f32(local)
    run = np.concatenate([[F32(0)], scan[:-1]]).astype(F32)
    excl = np.zeros(P, F32)
    for k in range(seg):
        i = s0 + k
        m = i < s1
        excl[i[m]] = run[m]
        run[m] = run[m] + vals[i[m]]
    return excl, scan[-1]


def cdf_fp32_emulation(p):
    """``(cdf, total)`` of fp32 weights ``p`` as the inverse-CDF path of is_sample forms them."""
    p = np.asarray(p, F32)
    excl, total = _serial_prefix(p, len(p))
    return (excl + p).astype(F32), total


def alias_fp32_emulation(p):
    """``(q, alias, total)`` of fp32 weights ``p`` (already ``l + alpha * ema``) as the alias
    path of is_sample builds them: fp32 throughout, the block scans in the kernel's order."""
    p = np.asarray(p, F32)
    P = len(p)
    _, total = _serial_prefix(p, P)
    v = p * (F32(P) / total)
    light = v < 1
    one = F32(1)
    deficit = np.where(light, one - v, F32(0)).astype(F32)
    excess = np.where(light, F32(0), v - one).astype(F32)
    dex, dtot = _serial_prefix(deficit, P)
    eex, etot = _serial_prefix(excess, P)
    L, H = np.nonzero(light)[0], np.nonzero(~light)[0]
    Ld, Hs = dex[L], np.concatenate([eex[H], [etot]]).astype(F32)
    nl, nh = len(L), len(H)
    q, alias = v.copy(), np.arange(P)
    if nh == 0:
        return np.ones(P, F32), alias, total
    # light: smallest k in [0, nh-1] with D <= Hs[k+1]
    alias[L] = H[np.minimum(np.searchsorted(Hs[1:], Ld, side='left'), nh - 1)]
    # heavy: first light prefix > Hs[k+1]
    lo = np.searchsorted(Ld, Hs[1:], side='right')
    dn = np.full(nh, dtot, F32)
    if nl:
        dn = np.where(lo < nl, Ld[np.minimum(lo, nl - 1)], dtot).astype(F32)
    r = np.minimum(one, np.maximum(F32(0), one - (dn - Hs[1:]))).astype(F32)
    r[nh - 1] = one
    q[H] = r
    alias[H] = np.concatenate([H[1:], H[-1:]])
    return q, alias, total


def recover_alias_table(bins, uy, idx, P):
    """What the draws alone say about the alias table.  Returns ``(alias, qlo, qhi, unique)``:
    per bucket the one index drawn when the draw left its bin (-1 if it never did), the largest
    second uniform that stayed (kept share > qlo, 0 if none stayed), the smallest that moved
    (kept share <= qhi, 1 if none moved), and whether the moved draws all went to one index."""
    moved = idx != bins
    qlo, qhi = np.zeros(P), np.ones(P)
    np.maximum.at(qlo, bins[~moved], uy[~moved].astype(np.float64))
    np.minimum.at(qhi, bins[moved], uy[moved].astype(np.float64))
    amin, amax = np.full(P, np.iinfo(np.int64).max), np.full(P, -1)
    np.minimum.at(amin, bins[moved], idx[moved])
    np.maximum.at(amax, bins[moved], idx[moved])
    return amax, qlo, qhi, bool(np.all((amax < 0) | (amin == amax)))


def implied_bracket(alias, qlo, qhi):
    """Rigorous ``[lo_i, hi_i]`` for ``P * p_i`` from a recovered table, and the mass ``U`` of
    the buckets whose alias is unknown (never moved): their ``1 - q_j <= 1 - qlo_j`` may belong
    to any item, so it is upward slack on every ``hi_i`` through its sum only."""
    P = len(alias)
    lo, hi = qlo.copy(), qhi.copy()
    known = alias >= 0
    np.add.at(lo, alias[known], 1.0 - qhi[known])
    np.add.at(hi, alias[known], 1.0 - qlo[known])
    return lo, hi, float(np.sum(1.0 - qlo[~known]))


# ---- the weight vectors of the exact GPU cases ----------------------------------------------
# Dyadic losses with mean exactly 1 (P / total = 1; a one-item pool has P / total = 1 / loss, a
# power of two), every partial sum a multiple of 0.25 below 2**13: all of the kernel's fp32
# arithmetic is exact on them, so the table is alias_closed_form bit for bit.
def exact_losses(kind, P):
    if kind == 'uniform':                    # the importance=False case draws from ones
        return np.ones(P, F32)
    if P == 1:
        return np.array([{'alternating': 0.5, 'blocks': 0.25, 'one_heavy': 2.0}[kind]], F32)
    if kind == 'alternating':                # nl == nh; a tie: lights 0 and 2 both go to heavy 1
        return np.tile(np.array([0.5, 1.5], F32), P // 2)
    if kind == 'blocks':                     # three lights (deficit 0.25 each) per heavy
        return np.tile(np.array([0.75, 0.75, 0.75, 1.75], F32), P // 4)
    if kind == 'one_heavy':                  # one heavy in the middle tops up every other item
        v = np.full(P, 0.5, F32)
        v[P // 3] = (P + 1) / 2.0
        return v
    raise KeyError(kind)


EXACT_KINDS = ('alternating', 'blocks', 'one_heavy')
EXACT_SHAPES = ((1, 1), (32, 32), (320, 32), (1024, 1), (1056, 32), (4064, 32))   # (P, group)


def skewed_losses(P, seed=0):
    """``rand**3 * 3`` (many light, few heavy bins), fp32, from numpy's generator."""
    return (np.random.default_rng(seed).random(P) ** 3 * 3).astype(F32)


def pool_eps(P):
    """Relative bound of the is_sample checks on random data: all terms are positive, a prefix
    carries at most seg + 6 + 4 fp32 additions, and u01 * total one more rounding."""
    seg = (P + IS_T - 1) // IS_T
    return 2 * (seg + 12) * ULP


def ema_replay(losses, group, ema_alpha=0.9):
    """The EMA is_sample leaves in ``ema[0]`` from a zeroed state: replayed over the cumulative
    means of the pool's groups (the kernel's arithmetic, up to its fp32 group sums)."""
    cs, ema = 0.0, None
    a = F32(ema_alpha)
    for gi in range(len(losses) // group):
        cs += float(np.sum(losses[gi * group:(gi + 1) * group], dtype=np.float64))
        m = F32(cs / ((gi + 1) * group))
        ema = m if ema is None else F32(a * ema + (F32(1) - a) * m)
    return ema


# ---- the checks, shared by the CPU evidence and the GPU tests --------------------------------
def cdf_draw_violation(idx, u, p64, eps):
    """Inverse-CDF draws against the fp64 CDF of ``p64``: draw d with fp32 uniform ``u[d]`` must
    satisfy ``cdf[k-1] - eps*total <= u*total < cdf[k] + eps*total`` for ``k = idx[d]``.  Returns
    (worst distance below, worst distance above, fraction outside the fp64 interval), distances
    in units of ``eps * total`` (<= 0: inside the fp64 interval itself)."""
    cdf = np.cumsum(p64)
    total = cdf[-1]
    u64 = u.astype(np.float64) * total
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    below, above = (lo - u64) / (eps * total), (u64 - cdf[idx]) / (eps * total)
    outside = np.mean((below > 0) | (above >= 0))
    return float(below.max()), float(above.max()), float(outside)


def alias_tol(p64, P):
    """Bound of the alias checks on P * p: the deficit and the excess prefix each carry the
    scan's roundings relative to the total deficit (at least to one bucket)."""
    x = P * p64 / p64.sum()
    return pool_eps(P) * max(1.0, float(np.sum(np.maximum(0.0, 1.0 - x))))


def alias_draw_violation(bins, uy, idx, p64):
    """Alias-path draws against ``p64``, model-free (recover_alias_table, implied_bracket).
    Returns (unique, worst violation of ``lo_i - tol <= P p_i <= hi_i + U + tol`` in units of
    tol, U, number of buckets whose alias never showed, mean bracket width)."""
    P = len(p64)
    alias, qlo, qhi, unique = recover_alias_table(bins, uy, idx, P)
    lo, hi, U = implied_bracket(alias, qlo, qhi)
    x = P * p64 / p64.sum()
    tol = alias_tol(p64, P)
    worst = float(np.max(np.maximum(lo - x, x - (hi + U)))) / tol
    return unique, worst, U, int(np.sum(alias < 0)), float(np.mean(hi - lo))


def ulps32(a, b):
    """Distance of fp32 arrays ``a`` and ``b`` in units in the last place (finite, same sign)."""
    ia = np.asarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def weight_violation(w, idx, p64, eps):
    """``w[d]`` against ``P * p64[idx[d]] / total`` with the bound ``eps`` relative plus 2 ulp;
    returns the worst error in units of that bound."""
    ref = len(p64) * p64[idx] / p64.sum()
    bound = eps * ref + 2 * np.spacing(ref.astype(F32)).astype(np.float64)
    return float(np.max(np.abs(w.astype(np.float64) - ref) / bound))


# ---- importance table ------------------------------------------------------------------------
TSEG = 2048


def table_C(N):
    """Constant of the table's draw bound ``eps = C * 2**-24 * total`` (all terms are >= 0, so
    every fp32 addition costs at most one unit roundoff of the running sum):

    * a segment's masked sum: 8 serial adds per thread + 6 butterfly steps + 4 wave totals = 18;
    * the group sum over segments: ``per`` serial adds + 6 + 16 = per + 22, and the division
      that forms the mean: the mean is within 18 + per + 23 of the fp64 mean, and so is every
      entry of the fp64 prefix (sums plus count times mean) and the total that scales the
      uniform: twice (41 + per);
    * inside the drawn segment: the fp32 remainder (1), each weight ``imp + mean`` (1), 32 serial
      adds per lane in 8 chunks (40), the 6-step wave scan, ``incl - ls`` (1) and the owner's
      walk of 32 more adds with their weights (33): 82."""
    per = ((N + TSEG - 1) // TSEG + 1023) // 1024
    return 2 * (41 + per) + 82


def table_reference(imp, grp, stamp):
    """``(members, cdf, mean, total)`` in fp64: the group's members in index order and the CDF
    of ``imp_i + mean`` over them."""
    members = np.nonzero(grp == stamp)[0]
    v = imp[members].astype(np.float64)
    mean = v.sum() / len(members) if len(members) else 0.0
    cdf = np.cumsum(v + mean)
    return members, cdf, mean, (cdf[-1] if len(members) else 0.0)


def table_draw_violation(picks, members, cdf, total, counter, seed, C):
    """Every pick must be a member q with ``cdf[q-1] - eps <= u < cdf[q] + eps``.  Returns (all
    picks are members, worst distance outside the fp64 interval in units of eps)."""
    picks = np.asarray(picks, np.int64)
    k = np.searchsorted(members, picks)
    k = np.minimum(k, len(members) - 1)
    if not np.array_equal(members[k], picks):
        return False, float('inf')
    rx, ry = table_draw_uniforms(counter, seed, len(picks))
    u = table_u(rx, ry, total)
    eps = C * ULP * total
    lo = np.where(k > 0, cdf[np.maximum(k - 1, 0)], 0.0)
    return True, float(max(((lo - u) / eps).max(), ((u - cdf[k]) / eps).max()))
