"""fp64 references and one elementwise criterion for the BN, pooling and head kernels.

A helper module (no tests, no fixtures).  Every reference runs in float64 torch on the device
of its inputs and returns, next to each value, ``mag``: the sum of the absolute values of the
terms that are added to form it.  ``assert_within`` holds a kernel output to

    |out - ref| <= 2^-8 * |ref| + k * mag        (bf16 output)
    |out - ref| <=                k * mag        (fp32 output)

``2^-8 |ref|`` is bf16's half-ulp bound (8 significand bits); it also covers a fp32 value that
falls on the other side of a rounding boundary.  ``k = 1e-5`` (about 170 fp32 epsilons) covers
rsqrt at 1 ulp, the variance cancellation ``E[x^2] / var <= ~10`` of the input recipe below, FMA
contraction and a fp32 chain a few hundred terms deep accumulated in another order.  Where a
value is formed from an earlier fp32 reduction (mean(dz) inside dy, h1 inside the MLP logits),
``mag`` carries that reduction's sum of |terms|, not the absolute value of its result: the
earlier sum's error is relative to the former.  A reference may also state an absolute
allowance that does not scale with k (``atol``; bn_bwd_ref's ``sums_atol``).

Input recipe (``bn_inputs``): everything is rounded to bf16 before the kernel and the
reference see it; per-(group, channel) means uniform in [-3, 3] and standard deviations in
[0.5, 2], so every ghost group has its own statistics; gamma of magnitude [0.5, 1.5] with a
quarter of the channels negative; the sums handed to a kernel are computed in fp64 and cast to
fp32.
"""
import math

import torch

K = 1e-5
HALF_ULP_BF16 = 2.0 ** -8
F64 = torch.float64
BF16 = torch.bfloat16


def rbf(x):
    """x rounded to bf16, in x's dtype."""
    return x.to(BF16).to(x.dtype)


# --------------------------------------------------------------------------- criterion
def needed_k(out, ref, mag, atol=None):
    """max over elements of (|out - ref| - 2^-8 |ref| [bf16 only] - atol) / mag: the k the
    output needs (inf where an element with mag == 0 is off, nan-safe)."""
    err = (out.to(F64) - ref).abs()
    if out.dtype == BF16:
        err = err - HALF_ULP_BF16 * ref.abs()
    if atol is not None:
        err = err - atol
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    need = torch.where(err <= 0, torch.zeros_like(err), err / mag)   # x / 0 -> inf
    return float(need.max()) if need.numel() else 0.0


def record(kernel, k):
    """Print the k a kernel output needed (pytest -s / -rP shows it; the margin under K is
    recorded in the GPU modules' docstrings from these lines)."""
    print('KNEED %s %.3g' % (kernel, k))
    return k


def assert_within(out, ref, mag, k=K, what='', decode=None, atol=None):
    """Elementwise criterion of the module docstring; returns the k the output needed.
    ``atol``: an absolute allowance, independent of k, added where a reference states one
    (bn_bwd_ref's ``sums_atol``).

    ``decode``: dict(C=, group_rows=, rpi=) -- on failure the worst element's flat index is
    printed as row, channel, ghost group and row-within-group % rpi (the rows one thread of
    the BN kernels visits are congruent mod rpi)."""
    assert out.shape == ref.shape == mag.shape, (what, out.shape, ref.shape, mag.shape)
    assert ref.dtype == F64 and mag.dtype == F64, what
    assert out.dtype in (BF16, torch.float32), (what, out.dtype)
    err = (out.to(F64) - ref).abs()
    tol = k * mag
    if out.dtype == BF16:
        tol = tol + HALF_ULP_BF16 * ref.abs()
    if atol is not None:
        tol = tol + atol
    bad = ~(err <= tol)                     # a NaN fails
    nbad = int(bad.sum())
    if nbad:
        over = torch.where(bad, torch.nan_to_num(err - tol, nan=math.inf), torch.zeros_like(err))
        idx = int(over.flatten().argmax())
        msg = '%s: %d of %d elements fail; worst at flat index %d' % (what, nbad, err.numel(), idx)
        if decode:
            C = decode['C']
            row, ch = idx // C, idx % C
            msg += ' = row %d channel %d' % (row, ch)
            gr = decode.get('group_rows')
            if gr:
                msg += ' group %d' % (row // gr)
                row = row % gr
            if decode.get('rpi'):
                msg += ' row %% rpi %d (rpi %d)' % (row % decode['rpi'], decode['rpi'])
        msg += ': out %r ref %r |err| %.3e tol %.3e mag %.3e' % (
            float(out.flatten()[idx]), float(ref.flatten()[idx]), float(err.flatten()[idx]),
            float(tol.flatten()[idx]), float(mag.flatten()[idx]))
        raise AssertionError(msg)
    return needed_k(out, ref, mag, atol)


# --------------------------------------------------------------------------- BN launch geometry
NT = 256


def bn_grid(chunks, C8, per_thread, cap):
    """csrc/bn.hip grid_for."""
    blocks = max(1, -(-chunks // (NT * per_thread)))
    blocks = min(blocks, cap)
    return max(blocks, -(-C8 // NT))


def bn_rpi(blocks, C):
    """rows between two visits of one thread: stride / C8 with stride = T - T % C8."""
    T, C8 = blocks * NT, C // 8
    return (T - T % C8) // C8


def bn_apply_rpi(M, C, group_rows):
    G = -(-M // group_rows)
    return bn_rpi(bn_grid(group_rows * (C // 8), C // 8, 4, -(-2048 // G)), C)


def bn_bwd_rpi(M, C, cap):
    """cap 256: the reduce kernel, 2048: the apply kernel."""
    return bn_rpi(bn_grid(M * (C // 8), C // 8, 4, cap), C)


# --------------------------------------------------------------------------- input recipe
def gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def bn_params(C, g):
    """gamma (|.| in [0.5, 1.5], a quarter of the channels negative) and beta, bf16 values."""
    gamma = torch.rand(C, generator=g, dtype=F64) + 0.5
    gamma[1::4] = -gamma[1::4]
    beta = torch.randn(C, generator=g, dtype=F64) * 0.5
    return rbf(gamma).float(), rbf(beta).float()


def bn_inputs(M, C, group_rows=0, seed=0, device='cpu'):
    """y bf16 [M][C] with per-(group, channel) mean / std, gamma, beta (fp32, bf16 values)."""
    g = gen(seed)
    group_rows = group_rows or M
    G = -(-M // group_rows)
    mean = torch.rand(G, C, generator=g) * 6 - 3
    std = torch.rand(G, C, generator=g) * 1.5 + 0.5
    grp = torch.arange(M) // group_rows
    z = torch.randn(M, C, generator=g)
    for gi in range(G):
        # a group of a few rows is standardised, so that its SAMPLE variance is the recipe's
        # (a chance sample variance near 0 would put E[x^2] / var far above the ~10 that k covers)
        r0, r1 = gi * group_rows, min(M, (gi + 1) * group_rows)
        if 2 <= r1 - r0 < 32:
            zz = z[r0:r1]
            z[r0:r1] = (zz - zz.mean(0)) / zz.std(0, unbiased=False)
    y = (z * std[grp] + mean[grp]).to(BF16)
    gamma, beta = bn_params(C, g)
    return y.to(device), gamma.to(device), beta.to(device)


def bn_sums(y, group_rows=0):
    """[G][2][C] fp32: per-group sum and sum of squares of y [M][C], computed in fp64."""
    M, C = y.shape
    group_rows = group_rows or M
    G = -(-M // group_rows)
    st = torch.empty(G, 2, C, dtype=F64, device=y.device)
    for gi in range(G):
        v = y[gi * group_rows:(gi + 1) * group_rows].to(F64)
        st[gi, 0], st[gi, 1] = v.sum(0), (v * v).sum(0)
    return st.float()


# --------------------------------------------------------------------------- BN forward
def act_ref(v, act):
    if act == 'relu':
        return v.clamp(min=0)
    if act == 'relu6':
        return v.clamp(min=0, max=6)
    return v


def bn_scale_shift(stats, counts, gamma, beta, eps, running=None):
    """fp64 per-(group, channel) scale / shift: [G][C] each ([1][C] from running statistics)."""
    if running is not None:
        mean, var = running[0].to(F64)[None], running[1].to(F64)[None]
    else:
        st = stats.to(F64).reshape(-1, 2, gamma.numel())
        cnt = counts.to(F64)[:, None]
        mean = st[:, 0] / cnt
        var = (st[:, 1] / cnt - mean * mean).clamp(min=0)
    sc = gamma.to(F64)[None] / torch.sqrt(var + eps)
    return sc, beta.to(F64)[None] - mean * sc


def group_counts(M, group_rows, device):
    G = -(-M // group_rows)
    return torch.tensor([min(M, (g + 1) * group_rows) - g * group_rows for g in range(G)],
                        dtype=F64, device=device)


def bn_apply_ref(y, stats, gamma, beta, group_rows=0, act='relu', eps=1e-5, running=None,
                 res=None, res_bn=None):
    """(ref, mag) of out = act(y*sc + sh [+ res | + res*sc2 + sh2]); a short last group is
    normalised with its own row count.  ``res_bn`` as ops.bn_apply's."""
    M, C = y.shape
    group_rows = group_rows or M
    cnt = group_counts(M, group_rows, y.device)
    grp = torch.arange(M, device=y.device) // group_rows
    if running is not None:
        grp = torch.zeros_like(grp)
    sc, sh = bn_scale_shift(stats, cnt, gamma, beta, eps, running)
    t = y.to(F64) * sc[grp]
    v, mag = t + sh[grp], t.abs() + sh[grp].abs()
    if res is not None and res_bn is None:
        v, mag = v + res.to(F64), mag + res.to(F64).abs()
    elif res is not None:
        run2 = res_bn[3] if len(res_bn) > 3 else None
        sc2, sh2 = bn_scale_shift(res_bn[0], cnt, res_bn[1], res_bn[2], eps, run2)
        t2 = res.to(F64) * sc2[grp]
        v, mag = v + t2 + sh2[grp], mag + t2.abs() + sh2[grp].abs()
    return act_ref(v, act), mag


# --------------------------------------------------------------------------- BN backward
def act_mask_ref(out, act):
    o = out.to(F64)
    if act == 'relu':
        return (o > 0).to(F64)
    if act == 'relu6':
        return ((o > 0) & (o < 6)).to(F64)
    return torch.ones_like(o)


def bn_bwd_ref(dout, out, y, stats, gamma, act='relu', eps=1e-5, y2=None, stats2=None,
               gamma2=None, totals=None, totals_mag=None):
    """One stat group.  The activation mask comes from the bf16 ``out`` the kernel reads.
    Returns a dict: dy, dy2, dz and sums [3][C] (sum dz, sum dz*xhat, sum dz*xhat2), each with
    its ``*_mag``, the sum of the |terms| the kernel adds: ``sums_mag`` is sum |dz| and
    sum |dz xhat|; ``dy_mag`` is |gamma rstd| (|dz| + sum |dz| / M + |xhat| sum |dz xhat| / M).
    ``sums_atol`` [3][C] is an absolute allowance for the xhat sums alone (see ``norm``).
    ``totals`` / ``totals_mag`` ([3][C] fp64): dy is formed from these sums instead (an apply
    pass over given replicas, whose fold is a sum of SUMS_R terms of magnitude totals_mag)."""
    M, C = y.shape
    dz = dout.to(F64) * act_mask_ref(out, act)

    def norm(yy, st):
        st = st.to(F64).reshape(2, C)
        mean = st[0] / M
        rstd = 1 / torch.sqrt((st[1] / M - mean * mean).clamp(min=0) + eps)
        # xhat = (y - mean) * rstd subtracts the fp32 mean = sum * (1 / M), which carries two
        # roundings (2 * 2^-24 |mean|); where y is close to the mean that error is not relative
        # to |xhat|, so a sum of dz * xhat is allowed 2^-23 |mean| rstd sum |dz| on top of
        # k sum |dz xhat|.  (Found at M = 5, C = 2048, relu: a channel whose only unmasked row
        # had xhat = 2e-3.  Relative to sum |dz xhat| alone the kernel needed k = 2.0e-5 there,
        # and so did the CPU fp32 emulation on the same inputs, 2e-6 ... 6e-5 over 20 other
        # seeds.  The allowance is the analytic bound of those two roundings, 1x, not a fit.)
        xh = (yy.to(F64) - mean) * rstd
        return xh, rstd, 2.0 ** -23 * mean.abs() * rstd

    r = {'dz': dz, 'dz_mag': dz.abs()}
    zero = torch.zeros(C, dtype=F64, device=y.device)
    sums, mags, atols = [dz.sum(0)], [dz.abs().sum(0)], [zero]
    for tag, yy, st, gm in (('', y, stats, gamma), ('2', y2, stats2, gamma2)):
        if yy is None:
            sums.append(zero)
            mags.append(zero)
            atols.append(zero)
            continue
        xh, rstd, slack = norm(yy, st)
        sx = (dz * xh).sum(0)
        sums.append(sx)
        mags.append((dz * xh).abs().sum(0))
        atols.append(slack * mags[0])
        i = len(sums) - 1
        # mean(dz) and mean(dz xhat) are themselves fp32 sums of M terms, whose error is relative
        # to their sum of |terms|, not to a result that may cancel: with |mean(dz)| and
        # |mean(dz xhat)| in their place the CPU fp32 emulation needs k = 1.5e-5 at
        # (22051, 96, relu6, with shortcut), with the sums of |terms| 1.4e-7 (1x, no factor)
        s0, a0, ax = sums[0], mags[0], mags[i]
        if totals is not None:
            s0, a0, sx, ax = totals[0], totals_mag[0], totals[i], totals_mag[i]
        k1 = gm.to(F64) * rstd
        r['dy' + tag] = k1 * (dz - s0 / M - xh * sx / M)
        r['dy' + tag + '_mag'] = k1.abs() * (dz.abs() + a0 / M + xh.abs() * ax / M)
    r['sums'], r['sums_mag'], r['sums_atol'] = torch.stack(sums), torch.stack(mags), torch.stack(atols)
    return r


# --------------------------------------------------------------------------- running statistics
def bn_running_ref(rm, rv, stats_train, n_train, cnt_train, stats_score, n_score, cnt_score,
                   momentum=0.1):
    """Sequential momentum folds, train groups first, then score groups; unbiased variance with
    the max(cnt - 1, 1) guard.  Returns fp64 (rmean, rvar)."""
    rm, rv = rm.to(F64).clone(), rv.to(F64).clone()
    C = rm.numel()
    for st, n, cnt in ((stats_train, n_train, cnt_train), (stats_score, n_score, cnt_score)):
        for g in range(n):
            s = st.to(F64).reshape(-1, 2, C)[g]
            mean = s[0] / cnt
            var = (s[1] / cnt - mean * mean).clamp(min=0) * (cnt / max(cnt - 1.0, 1.0))
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var
    return rm, rv


# --------------------------------------------------------------------------- pooling
def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def _taps(x, k, s, p, fill):
    """x [N][H][W][C] fp64 -> list over taps t = r*k + c of ([N][P][Q][C] values, in-image mask
    [P][Q])."""
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, s, p), pool_out(W, k, s, p)
    xp = torch.full((N, H + 2 * p + k, W + 2 * p + k, C), fill, dtype=F64, device=x.device)
    xp[:, p:p + H, p:p + W] = x
    inside = torch.zeros(H + 2 * p + k, W + 2 * p + k, dtype=torch.bool, device=x.device)
    inside[p:p + H, p:p + W] = True
    out = []
    for t in range(k * k):
        r, c = t // k, t % k
        sl = (slice(r, r + (P - 1) * s + 1, s), slice(c, c + (Q - 1) * s + 1, s))
        out.append((xp[:, sl[0], sl[1]], inside[sl[0], sl[1]]))
    return out


def maxpool_ref(x, k, s, p):
    """(max [N][P][Q][C] fp64, tap uint8): the tap r*k + c of the FIRST maximum in scan order
    (a later equal value does not replace it); out-of-image taps are skipped."""
    best = arg = None
    for t, (v, _) in enumerate(_taps(x.to(F64), k, s, p, -math.inf)):
        if best is None:
            best, arg = v.clone(), torch.zeros(v.shape, dtype=torch.uint8, device=x.device)
            continue
        win = v > best
        best = torch.where(win, v, best)
        arg = torch.where(win, torch.full_like(arg, t), arg)
    return best, arg


def maxpool_bwd_ref(dy, arg, H, W, k, s, p):
    """(dx, mag) [N][H][W][C]: every input sums the gradients of the windows whose recorded
    tap it is; mag sums their absolute values (0 where no window points: exactly 0 expected)."""
    N, P, Q, C = dy.shape
    g = dy.to(F64)
    dx = torch.zeros(N, H + 2 * p + k, W + 2 * p + k, C, dtype=F64, device=dy.device)
    mag = torch.zeros_like(dx)
    for t in range(k * k):
        r, c = t // k, t % k
        m = (arg == t).to(F64)
        sl = (slice(None), slice(r, r + (P - 1) * s + 1, s), slice(c, c + (Q - 1) * s + 1, s))
        dx[sl] += g * m
        mag[sl] += g.abs() * m
    return dx[:, p:p + H, p:p + W].contiguous(), mag[:, p:p + H, p:p + W].contiguous()


def avgpool_ref(x, k, s, p):
    """(mean, mag): in-image taps summed and divided by k*k (F.avg_pool2d's default,
    count_include_pad=True)."""
    taps = _taps(x.to(F64), k, s, p, 0.0)
    v = sum(t for t, _ in taps) / (k * k)
    mag = sum(t.abs() for t, _ in taps) / (k * k)
    return v, mag


# --------------------------------------------------------------------------- classifier head
def head_ref(act, w, b, label, isw=None, pooled=None, logits_mag=None):
    """Pool, FC, log-sum-exp loss, IS-weighted dlogits, meters, gradnorm score -- fp64.

    ``act`` [B][HW][C] (or ``pooled`` [B][C] given; ``logits_mag`` replaces sum |w h| + |b| where
    pooled is itself an fp32 reduction of the kernel's).  Returns a dict with value / ``*_mag`` or
    ``*_tol`` entries as the tolerances of the head tests define them:
      T_b = max_k K * logits_mag[b][k];  losses: 2 T_b + 1e-5 max(1, |lse|);
      dlogits: scale_b (p (2 T_b + 1e-5) + 1e-7)."""
    r = {}
    if pooled is None:
        a = act.to(F64)
        pooled, r['pooled_mag'] = a.mean(1), a.abs().mean(1)
    else:
        pooled = pooled.to(F64)
    B = pooled.shape[0]
    w64, b64 = w.to(F64), b.to(F64)
    logits = pooled @ w64.t() + b64
    r['pooled'], r['logits'] = pooled, logits
    r['logits_mag'] = pooled.abs() @ w64.abs().t() + b64.abs() if logits_mag is None else logits_mag
    lab = label.long()
    lse = torch.logsumexp(logits, 1)
    loss = lse - logits.gather(1, lab[:, None])[:, 0]
    T = K * r['logits_mag'].max(1).values
    r['T'], r['lse'], r['losses'] = T, lse, loss
    r['losses_tol'] = 2 * T + 1e-5 * lse.abs().clamp(min=1)
    wi = isw.to(F64) if isw is not None else torch.ones(B, dtype=F64, device=pooled.device)
    scale = 1 / (B * wi)
    p = torch.exp(logits - lse[:, None])
    d = p.clone()
    d[torch.arange(B), lab] -= 1
    r['scale'], r['p'] = scale, p
    r['dlogits'] = d * scale[:, None]
    d_tol = p * (2 * T[:, None] + 1e-5) + 1e-7
    r['dlogits_tol'] = scale[:, None] * d_tol
    # argmax: the first maximum wins.  A sample whose two largest logits differ by less than
    # both their tolerances (and are not equal) may go either way in fp32
    am = torch.argmax((logits == logits.max(1, keepdim=True).values).to(torch.int8), 1)
    top2 = logits.topk(2, 1).values if logits.shape[1] > 1 else None
    gap = top2[:, 0] - top2[:, 1] if top2 is not None else torch.ones_like(lse)
    unsure = (gap > 0) & (gap <= 2 * T)
    hit = am == lab
    r['argmax'] = am
    r['correct'] = (int((hit & ~unsure).sum()), int((hit | unsure).sum()))     # [lo, hi]
    for m, terms in (('train', loss / wi), ('eval', loss)):
        tol = (r['losses_tol'] / (wi if m == 'train' else 1)).sum() + K * terms.abs().sum()
        r['meter0_' + m] = (float(terms.sum()), float(tol))
    # gradnorm = |softmax - onehot| * sqrt(|h|^2 + 1): the error of |d| is at most |d_tol|
    h2 = (pooled * pooled).sum(1) + 1
    gn = torch.sqrt((d * d).sum(1) * h2)
    r['gradnorm'] = gn
    r['gradnorm_tol'] = torch.sqrt((d_tol * d_tol).sum(1) * h2) + 1e-5 * gn
    return r


def assert_tol(out, ref, tol, what):
    """|out - ref| <= tol elementwise (the head's loss / dlogits tolerances); returns the
    largest |err| / tol."""
    err = (out.to(F64) - ref).abs()
    bad = ~(err <= tol)
    if int(bad.sum()):
        idx = int(torch.where(bad, torch.nan_to_num(err / tol, nan=math.inf),
                              torch.zeros_like(err)).flatten().argmax())
        raise AssertionError('%s: %d of %d fail; worst at %d: out %r ref %r tol %.3e' % (
            what, int(bad.sum()), err.numel(), idx, float(out.flatten()[idx]),
            float(ref.flatten()[idx]), float(tol.flatten()[idx])))
    return float((err / tol).max())


def head_pool_bn_ref(x, res, stats, gamma, beta, count, group_imgs, act, eps, running=None):
    """(pooled, mag) [B][C]: mean over HW of act(bn(x) [+ res]); x [B][HW][C]; mag is the mean
    of |terms|."""
    B, HW, C = x.shape
    cnt = torch.full((-(-B // group_imgs),), float(count), dtype=F64, device=x.device)
    sc, sh = bn_scale_shift(stats, cnt, gamma, beta, eps, running)
    grp = torch.arange(B, device=x.device) // group_imgs
    if running is not None:
        grp = torch.zeros_like(grp)
    t = x.to(F64) * sc[grp][:, None]
    v, mag = t + sh[grp][:, None], t.abs() + sh[grp][:, None].abs()
    if res is not None:
        v, mag = v + res.to(F64), mag + res.to(F64).abs()
    return act_ref(v, act).mean(1), mag.mean(1)


def head_bwd_ref(pooled, dlogits, w, HW):
    """dact row [B][C] (broadcast over HW by the kernel, bf16), dw, db with their mags."""
    p, d, w64 = pooled.to(F64), dlogits.to(F64), w.to(F64)
    return {'dact': d @ w64 / HW, 'dact_mag': d.abs() @ w64.abs() / HW,
            'dw': d.t() @ p, 'dw_mag': d.abs().t() @ p.abs(),
            'db': d.sum(0), 'db_mag': d.abs().sum(0)}


# --------------------------------------------------------------------------- speech-VGG head
def mlp_fwd_ref(x, w1, b1, w2, b2):
    """h1 = x W1^T + b1, logits = h1 W2^T + b2.  The kernel forms logits from ITS fp32 h1, so
    logits_mag carries h1's sum of |terms|."""
    x, w1, b1, w2, b2 = (t.to(F64) for t in (x, w1, b1, w2, b2))
    h1, h1_mag = x @ w1.t() + b1, x.abs() @ w1.abs().t() + b1.abs()
    return {'h1': h1, 'h1_mag': h1_mag, 'logits': h1 @ w2.t() + b2,
            'logits_mag': h1_mag @ w2.abs().t() + b2.abs()}


def mlp_bwd_ref(dlogits, h1, x, w1, w2):
    """All gradients of the two-layer head from given dlogits / h1 (fp32 inputs of the kernel).
    db1, dW1 and dx are formed from the kernel's fp32 dh1: their mags carry dh1's |terms|."""
    d, h1, x, w1, w2 = (t.to(F64) for t in (dlogits, h1, x, w1, w2))
    dh1, dh1_mag = d @ w2, d.abs() @ w2.abs()
    return {'dw2': d.t() @ h1, 'dw2_mag': d.abs().t() @ h1.abs(),
            'db2': d.sum(0), 'db2_mag': d.abs().sum(0),
            'dh1': dh1, 'dh1_mag': dh1_mag,
            'db1': dh1.sum(0), 'db1_mag': dh1_mag.sum(0),
            'dw1': dh1.t() @ x, 'dw1_mag': dh1_mag.t() @ x.abs(),
            'dx': dh1 @ w1, 'dx_mag': dh1_mag @ w1.abs()}


# --------------------------------------------------------------------------- shared cases
# The GPU tests and the CPU emulation checks (test_kernel_oracles.py) build their inputs here:
# the same shapes and the same seeds, so a GPU failure can be compared with the fp32 emulation
# on the very inputs that failed.
ACTS = ['none', 'relu', 'relu6']
RES = ['none', 'identity', 'bn']


def running_pair(C, seed, device='cpu'):
    """(rmean, rvar) of the recipe: means in [-3, 3], standard deviations in [0.5, 2]."""
    g = gen(seed)
    return ((torch.rand(C, generator=g) * 6 - 3).to(device),
            ((torch.rand(C, generator=g) * 1.5 + 0.5) ** 2).to(device))


def bn_apply_case(M, C, group_rows, res, seed, running=False, device='cpu'):
    """(y, stats | None, gamma, beta, kwargs): the kwargs go to ops.bn_apply and to bn_apply_ref."""
    y, gamma, beta = bn_inputs(M, C, group_rows, seed, device)
    stats = bn_sums(y, group_rows)
    kw = {}
    if running:
        kw['running'] = running_pair(C, seed + 7, device)
    if res == 'identity':
        kw['res'] = (torch.randn(M, C, generator=gen(seed + 1)) * 2).to(BF16).to(device)
    elif res == 'bn':
        y2, g2, b2 = bn_inputs(M, C, group_rows, seed + 2, device)
        kw['res'] = y2
        kw['res_bn'] = (bn_sums(y2, group_rows), g2, b2)
        if running:
            kw['res_bn'] = (None, g2, b2, running_pair(C, seed + 9, device))
    return y, (None if running else stats), gamma, beta, kw


# (M, C, group_rows, act, res, running, seed)
BN_APPLY_FORMS = [(M, C, 0, act, res, False, M + C) for M, C in ((37, 24), (1027, 96))
                  for res in RES for act in ACTS]
BN_APPLY_CHANNELS = [(M, C, 0, 'relu', 'identity', False, C)
                     for C, M in ((8, 45), (24, 19), (40, 19), (144, 19), (320, 19), (960, 11),
                                  (1280, 11), (4096, 2))]
BN_APPLY_SHORT_GROUP = [(1300, 24, 500, 'relu', 'identity', False, 3),
                        (1300, 40, 500, 'none', 'bn', False, 4)]
BN_APPLY_RUNNING = [c for res in RES for c in ((37, 40, 0, 'relu6', res, True, 11),
                                               (1027, 96, 0, 'relu', res, True, 12))]
BN_APPLY_STREAMING = [(37, 24, 0, 'relu', 'identity', False, 31), (1027, 96, 0, 'none', 'bn', False, 31)]
# G = 64 caps the grid at 32 blocks per group: T = 8192, stride = 8184, rpi = 682; a trip covers
# 4 * 682 = 2728 rows, so a 3000-row group gets a 272-row second trip; the last group has 1700
BN_APPLY_MULTI_TRIP = (64 * 3000 - 1300, 96, 3000, 'relu6', 'bn', False, 21)


def bn_bwd_case(M, C, act, two, sparse, seed, device='cpu'):
    """(dout, out, y, stats [2][C], gamma, kwargs for ops.bn_bwd / bn_bwd_ref)."""
    y, gamma, beta = bn_inputs(M, C, 0, seed, device)
    stats = bn_sums(y)
    kw, fkw = {}, {}
    if two:
        y2, g2, b2 = bn_inputs(M, C, 0, seed + 2, device)
        st2 = bn_sums(y2)
        kw = dict(y2=y2, stats2=st2[0], gamma2=g2)
        fkw = dict(res=y2, res_bn=(st2, g2, b2))
    # the block output whose activation mask both sides read: the fp64 forward, rounded
    out = bn_apply_ref(y, stats, gamma, beta, 0, act, **fkw)[0].to(BF16)
    g = gen(seed + 5)
    dout = torch.randn(M, C, generator=g)
    if sparse:
        # zero except the last 5 rows and 5 random rows: a dropped or doubled tail row changes
        # a channel's sum by the order of its value
        keep = torch.zeros(M, dtype=torch.bool)
        keep[M - 5:] = True
        keep[torch.randperm(M - 5, generator=g)[:5]] = True
        dout = dout * keep[:, None]
    return dout.to(BF16).to(device), out, y, stats[0], gamma, kw


# (M, C, act, two, sparse, seed)
BN_BWD_SMALL = [(M, C, act, two, False, M) for M, C in ((37, 24), (1027, 96)) for act in ACTS
                for two in (False, True)]
BN_BWD_LARGE = [(M, C, act, two, sparse, M) for M, C in ((22051, 96), (13109, 320))
                for act in ACTS for two in (False, True) for sparse in (False, True)]
BN_BWD_LIMIT = (5, 2048, 'relu', True, False, 8)
BN_BWD_NO_OPTIONAL = (1027, 96, 'relu', False, False, 5)
BN_BWD_APPLY_ONLY = (1027, 96, 'relu6', True, False, 6)


def replica_parts(sums, R):
    """A known total spread unevenly (signs mixed, one replica empty) over R replicas:
    (parts [R][3][C] fp32, totals, totals_mag fp64)."""
    wts = torch.tensor(([3.5, -2.75, 0.0, 0.25] + [0.125] * R)[:R], dtype=F64, device=sums.device)
    wts[-1] += 1 - wts.sum()
    parts = (sums[None] * wts[:, None, None]).float().contiguous()
    return parts, parts.double().sum(0), parts.double().abs().sum(0)


# C, n_train, n_score, initial nbt (None: null pointer), cnt_train, cnt_score
RUNNING_LAYERS = [(24, 1, 10, 5, 128.0, 64.0), (320, 0, 17, None, 128.0, 48.0),
                  (264, 1, 0, 7, 1.0, 64.0)]


def bn_running_case(li, device='cpu'):
    """(rm0, rv0, stats_train, stats_score) of layer ``li`` of RUNNING_LAYERS."""
    C, ntr, nsc, _, ctr, csc = RUNNING_LAYERS[li]
    g = gen(100 + li)

    def group_sums(n, cnt):
        if n == 0:
            return torch.full((1, 2, C), float('nan'), device=device)    # never read
        return bn_sums(bn_inputs(n * int(cnt), C, int(cnt), 200 + li, device)[0], int(cnt)).contiguous()

    rm0 = torch.randn(C, generator=g).to(device)
    rv0 = (torch.rand(C, generator=g) + 0.5).to(device)
    return rm0, rv0, group_sums(ntr, ctr), group_sums(nsc, csc)


POOL_KSP = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (4, 4, 0), (5, 3, 2)]
POOL_SHAPES = [(3, 11, 7, 8), (2, 12, 12, 24)]


def pool_data(shape, kind, seed, device='cpu'):
    g = gen(seed)
    if kind == 'ties':       # five values: most windows hold their maximum more than once
        x = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, shape, generator=g)]
    else:
        x = torch.randn(shape, generator=g) * 2
    return x.to(BF16).to(device)


def pool_grad(shape, device='cpu'):
    return (torch.randn(shape, generator=gen(5)) * 2).to(BF16).to(device)


def head_case(B, HW, C, K, wscale=1.0, tie=None, device='cpu'):
    """(act bf16 [B][HW][C], w, b, label int32, isw).  ``tie`` = (j1, j2): two identical rows whose
    logit is every sample's largest, every label naming the second."""
    g = gen(B * 1000 + HW * 100 + C + K)
    act = (torch.rand(B, HW, C, generator=g) * 2 - 0.5).to(BF16)
    w = torch.randn(K, C, generator=g) * 0.05 * wscale
    b = torch.randn(K, generator=g) * 0.1
    label = torch.randint(0, K, (B,), generator=g).int()
    isw = torch.rand(B, generator=g) + 0.5
    if tie:
        w[tie[0]] = w[tie[1]] = 0.2
        b[tie[0]] = b[tie[1]] = 0.5
        label[:] = tie[1]
    return tuple(t.to(device) for t in (act, w, b, label, isw))


# (B, HW, C, K, wscale)
HEAD_SAMPLE_CASES = [(B, HW, C, K, 1.0) for K, C in ((10, 512), (100, 1280)) for HW in (1, 16)
                     for B in (1, 5)]
HEAD_CHUNK_CASES = [(5, 16, 1280, 100, 1.0), (5, 16, 328, 65, 1.0), (5, 4, 1048, 1008, 1.0)]
HEAD_WIDE_CASES = [(5, 16, 1056, 1000, 1.0), (70, 49, 1056, 1000, 1.0)]
HEAD_RANGE_CASE = (5, 16, 1280, 100, 60.0)
HEAD_TIES = [(3, 77), (3, 67)]


def head_pool_bn_case(HW, C, device='cpu'):
    """B = 12 in ghost groups of 4 images, K = 10: (x [B][HW][C], gamma, beta, stats, res, rm, rv,
    w, b, label)."""
    B, gi, K = 12, 4, 10
    x, gamma, beta = bn_inputs(B * HW, C, gi * HW, seed=HW + C, device=device)
    stats = bn_sums(x, gi * HW)
    g = gen(HW)
    res = (torch.randn(B, HW, C, generator=g) * 2).to(BF16).to(device)
    rm = (torch.rand(C, generator=g) * 6 - 3).to(device)
    rv = ((torch.rand(C, generator=g) * 1.5 + 0.5) ** 2).to(device)
    w = (torch.randn(K, C, generator=g) * 0.05).to(device)
    b = (torch.randn(K, generator=g) * 0.1).to(device)
    label = torch.randint(0, K, (B,), generator=g).int().to(device)
    return x.view(B, HW, C), gamma, beta, stats, res, rm, rv, w, b, label


HEAD_POOL_BN_CASES = [(HW, C) for C in (24, 512) for HW in (1, 16, 49)]
# (B, HW, C, K, takes the GEMM path)
HEAD_BWD_CASES = [(5, 1, 328, 10, False), (70, 16, 1280, 100, False), (5, 4, 1056, 1001, False),
                  (70, 49, 1056, 1000, True)]


def head_bwd_case(B, C, K, device='cpu'):
    g = gen(B + K)
    pooled = (torch.rand(B, C, generator=g) * 2 - 0.5).to(device)
    dlog = (torch.randn(B, K, generator=g) / B).to(device)
    w = (torch.randn(K, C, generator=g) * 0.05).to(device)
    return pooled, dlog, w


MLP_DIMS = (200, 72, 30)          # F, H1, K
MLP_BATCHES = [5, 70]


def mlp_case(B, device='cpu'):
    """(x bf16 [B][F], w1 bf16 [H1][F], b1, w2, b2, label, isw)."""
    F, H1, K = MLP_DIMS
    g = gen(B)
    x = torch.randn(B, F, generator=g).to(BF16)
    w1 = (torch.randn(H1, F, generator=g) * 0.1).to(BF16)
    b1 = torch.randn(H1, generator=g) * 0.1
    w2 = torch.randn(K, H1, generator=g) * 0.2
    b2 = torch.randn(K, generator=g) * 0.1
    label = torch.randint(0, K, (B,), generator=g).int()
    isw = torch.rand(B, generator=g) + 0.5
    return tuple(t.to(device) for t in (x, w1, b1, w2, b2, label, isw))
