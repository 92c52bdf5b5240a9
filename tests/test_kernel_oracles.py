"""CPU evidence for the criterion of ``kernel_oracles`` (no GPU needed).

For every operation a plain fp32 torch emulation of the kernel's arithmetic order (fp32
scale / shift, sums taken in per-thread chunks, then one bf16 rounding) must pass
``assert_within`` against the fp64 reference with at most k / 2 -- the criterion can be met --
and a list of deliberately wrong emulations must each fail it -- the GPU tests built on it
would notice a subtly wrong kernel.
"""
import pytest
import torch

import kernel_oracles as ko

F32, BF16 = torch.float32, torch.bfloat16
HALF_K = ko.K / 2


def passes(out, ref, mag, what):
    need = ko.assert_within(out, ref, mag, what=what)
    assert need <= HALF_K, '%s: a correct fp32 evaluation needs k = %g > k / 2' % (what, need)


def rejects(out, ref, mag, what):
    with pytest.raises(AssertionError, match='elements fail'):
        ko.assert_within(out, ref, mag, what=what)


def act32(v, act):
    if act == 'relu':
        return v.clamp(min=0)
    if act == 'relu6':
        return v.clamp(min=0, max=6)
    return v


# ------------------------------------------------------------------------------ criterion
def test_criterion_reports_and_decodes_the_worst_element():
    ref = torch.arange(1, 49, dtype=torch.float64).reshape(6, 8)
    out = ref.to(BF16)
    assert ko.assert_within(out, ref, ref.abs()) == 0.0
    out[4, 3] = float(out[4, 3]) * 1.02
    with pytest.raises(AssertionError) as e:
        ko.assert_within(out, ref, ref.abs(), what='probe',
                         decode=dict(C=8, group_rows=3, rpi=2))
    msg = str(e.value)
    assert 'probe: 1 of 48 elements fail' in msg and 'row 4 channel 3 group 1' in msg
    assert 'row % rpi 1 (rpi 2)' in msg
    # fp32 outputs get no 2^-8 |ref| term; a NaN fails; mag == 0 demands exactly ref
    f = ref.float()
    assert ko.assert_within(f, ref, ref.abs()) == 0.0
    with pytest.raises(AssertionError):
        ko.assert_within((ref * (1 + 3e-5)).float(), ref, ref.abs())
    f[0, 0] = float('nan')
    with pytest.raises(AssertionError):
        ko.assert_within(f, ref, ref.abs())
    z = torch.zeros(4, dtype=torch.float64)
    assert ko.assert_within(z.float(), z, z) == 0.0
    with pytest.raises(AssertionError):
        ko.assert_within(z.float() + 1e-30, z, z)


def test_recipe_gives_every_group_its_own_statistics():
    y, gamma, beta = ko.bn_inputs(1300, 24, 500, seed=3)
    assert y.dtype == BF16 and (gamma < 0).sum() == 6 and gamma.abs().min() >= 0.5
    assert torch.equal(gamma, ko.rbf(gamma)) and torch.equal(beta, ko.rbf(beta))
    st = ko.bn_sums(y, 500).double()
    mean = st[:, 0] / torch.tensor([500.0, 500.0, 300.0])[:, None]
    assert (mean[0] - mean[1]).abs().median() > 0.5 and (mean[1] - mean[2]).abs().median() > 0.5
    assert ko.bn_apply_rpi(64 * 3000 - 1300, 96, 3000) == 682
    assert ko.bn_bwd_rpi(22051, 96, 256) == 5461


# ------------------------------------------------------------------------------ BN apply
def scale_shift32(s, ss, inv, gamma, beta, eps=1e-5, running=None, var_as_std=False):
    if running is not None:
        mean, var = running[0].float(), running[1].float()
    else:
        mean = s * inv
        var = (ss * inv - mean * mean).clamp(min=0)
    sc = gamma / (var + eps) if var_as_std else gamma * torch.rsqrt(var + eps)
    return sc, beta - mean * sc


def emu_bn_apply(y, stats, gamma, beta, group_rows, act, running=None, res=None, res_bn=None,
                 bug=None):
    M, C = y.shape
    gr = group_rows or M
    G = -(-M // gr)
    grp = torch.arange(M) // gr
    cnt = ko.group_counts(M, gr, 'cpu').float()
    if bug == 'group_rows_divisor':
        cnt = torch.full_like(cnt, float(gr))
    inv = (1.0 / cnt)[:, None]

    def ss(st, g, b, run):
        if run is not None:
            sc, sh = scale_shift32(None, None, None, g, b, running=run,
                                   var_as_std=bug == 'var_as_std')
            return sc[None].expand(G, C), sh[None].expand(G, C)
        st = st.reshape(G, 2, C)
        if bug == 'neighbour_group':
            st = st.roll(1, 0)
        return scale_shift32(st[:, 0], st[:, 1], inv, g, b)

    sc, sh = ss(stats, gamma, beta, running)
    v = y.float() * sc[grp] + sh[grp]
    if res is not None and res_bn is None:
        v = v + res.float()
    elif res is not None:
        g2 = gamma if bug == 'shortcut_main_gamma' else res_bn[1]
        sc2, sh2 = ss(res_bn[0], g2, res_bn[2], res_bn[3] if len(res_bn) > 3 else None)
        v = v + (res.float() * sc2[grp] + sh2[grp])
    out = act32(v, 'relu' if (bug == 'relu6_no_cap' and act == 'relu6') else act).to(BF16)
    if bug == 'stale_tail_row':
        out[M - 1] = out[M - 9]       # the tail row's registers still hold the previous trip
    return out


APPLY_CASES = (ko.BN_APPLY_FORMS + ko.BN_APPLY_CHANNELS + ko.BN_APPLY_SHORT_GROUP
               + ko.BN_APPLY_RUNNING + ko.BN_APPLY_STREAMING + [ko.BN_APPLY_MULTI_TRIP])


@pytest.mark.parametrize('M,C,gr,act,res,running,seed', APPLY_CASES)
def test_bn_apply_fp32_emulation_meets_the_criterion(M, C, gr, act, res, running, seed):
    """Every bn_apply case of the GPU module, on the same inputs."""
    y, stats, gamma, beta, kw = ko.bn_apply_case(M, C, gr, res, seed, running)
    ref, mag = ko.bn_apply_ref(y, stats, gamma, beta, gr, act, **kw)
    passes(emu_bn_apply(y, stats, gamma, beta, gr, act, **kw), ref, mag, 'bn_apply emulation')


@pytest.mark.parametrize('bug,M,C,gr,act,res,running', [
    ('neighbour_group', 1300, 24, 500, 'relu', 'identity', False),
    ('group_rows_divisor', 1300, 24, 500, 'relu', 'identity', False),
    ('stale_tail_row', 1027, 96, 0, 'none', 'none', False),
    ('relu6_no_cap', 1027, 96, 0, 'relu6', 'identity', False),
    ('shortcut_main_gamma', 1027, 96, 0, 'relu', 'bn', False),
    ('var_as_std', 1027, 96, 0, 'relu', 'none', True),
    ('var_as_std', 37, 40, 0, 'relu6', 'bn', True),
])
def test_bn_apply_wrong_variants_are_rejected(bug, M, C, gr, act, res, running):
    y, stats, gamma, beta, kw = ko.bn_apply_case(M, C, gr, res, M + C, running)
    ref, mag = ko.bn_apply_ref(y, stats, gamma, beta, gr, act, **kw)
    passes(emu_bn_apply(y, stats, gamma, beta, gr, act, **kw), ref, mag, 'bn_apply emulation')
    rejects(emu_bn_apply(y, stats, gamma, beta, gr, act, bug=bug, **kw), ref, mag, bug)


# ------------------------------------------------------------------------------ BN backward
def mask32(out, act, no_upper=False):
    o = out.float()
    if act == 'relu' or (act == 'relu6' and no_upper):
        return (o > 0).float()
    if act == 'relu6':
        return ((o > 0) & (o < 6)).float()
    return torch.ones_like(o)


def chunked_sum(t, rpi):
    """Per-thread partials over the rows congruent mod rpi, then their fp32 total."""
    M, C = t.shape
    part = torch.zeros(min(rpi, M), C).index_add_(0, torch.arange(M) % rpi, t)
    return part.sum(0)


def emu_bn_bwd(dout, out, y, stats, gamma, act, y2=None, stats2=None, gamma2=None, bug=None,
               parts=None):
    M, C = y.shape
    inv = torch.tensor(1.0) / M
    dz = dout.float() * mask32(out, act, bug == 'relu6_mask_no_upper')
    rpi = ko.bn_bwd_rpi(M, C, 256)
    rows = torch.ones(M)
    if bug == 'drop_tail_row':
        rows[M - 1] = 0
    if bug == 'double_tail_row':
        rows[M - 1] = 2

    def norm(yy, st):
        mean = st[0] * inv
        rstd = torch.rsqrt((st[1] * inv - mean * mean).clamp(min=0) + 1e-5)
        return (yy.float() - mean) * rstd, rstd

    r = {'dz': dz.to(BF16)}
    sdz = chunked_sum(dz * rows[:, None], rpi)
    sums = [sdz]
    for i, (tag, yy, st, gm) in enumerate((('', y, stats, gamma), ('2', y2, stats2, gamma2))):
        if yy is None:
            sums.append(torch.zeros(C))
            continue
        xh, rstd = norm(yy, st)
        sx = chunked_sum(dz * xh * rows[:, None], rpi)
        sums.append(sx)
        if parts is not None:            # the apply pass over given replicas
            tot = parts[0].clone() if bug == 'replica0_only' else parts.sum(0)
            sdz, sx = tot[0], tot[1 + i]
        r['dy' + tag] = ((gm * rstd) * (dz - sdz * inv - xh * (sx * inv))).to(BF16)
    r['sums'] = torch.stack(sums)
    return r


def check_bwd(e, r, two, check):
    n = 3 if two else 2
    need = ko.assert_within(e['sums'][:n], r['sums'][:n], r['sums_mag'][:n], what='bn_bwd sums',
                            atol=r['sums_atol'][:n])
    assert need <= HALF_K, 'bn_bwd sums: a correct fp32 evaluation needs k = %g' % need
    check(e['dy'], r['dy'], r['dy_mag'], 'bn_bwd dy')
    check(e['dz'], r['dz'], r['dz_mag'], 'bn_bwd dz')
    if two:
        check(e['dy2'], r['dy2'], r['dy2_mag'], 'bn_bwd dy2')


@pytest.mark.parametrize('M,C,act,two,sparse,seed', ko.BN_BWD_SMALL + ko.BN_BWD_LARGE
                         + [ko.BN_BWD_LIMIT, ko.BN_BWD_NO_OPTIONAL])
def test_bn_bwd_fp32_emulation_meets_the_criterion(M, C, act, two, sparse, seed):
    """Every bn_bwd case of the GPU module, on the same inputs."""
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(M, C, act, two, sparse, seed)
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, act, **kw)
    check_bwd(emu_bn_bwd(dout, out, y, stats, gamma, act, **kw), r, two, passes)


@pytest.mark.parametrize('bug,act,sparse,which', [
    ('drop_tail_row', 'none', True, 'sums'), ('double_tail_row', 'none', True, 'sums'),
    ('drop_tail_row', 'relu', True, 'dy'), ('relu6_mask_no_upper', 'relu6', False, 'dz'),
    ('relu6_mask_no_upper', 'relu6', False, 'sums')])
def test_bn_bwd_wrong_variants_are_rejected(bug, act, sparse, which):
    M, C = 22051, 96
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(M, C, act, True, sparse, M)
    if act == 'relu6':
        assert int((out.float() >= 6).sum()) >= 100
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, act, **kw)
    e = emu_bn_bwd(dout, out, y, stats, gamma, act, bug=bug, **kw)
    with pytest.raises(AssertionError, match='elements fail'):
        ko.assert_within(e[which], r[which], r[which + '_mag'], what=bug,
                         atol=r['sums_atol'] if which == 'sums' else None)


def test_bn_bwd_replica_fold():
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(*ko.BN_BWD_APPLY_ONLY)
    r0 = ko.bn_bwd_ref(dout, out, y, stats, gamma, 'relu6', **kw)
    parts, tot, tmag = ko.replica_parts(r0['sums'], 8)
    assert float(tot[0].abs().sum()) > 0 and (parts[2] == 0).all()
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, 'relu6', totals=tot, totals_mag=tmag, **kw)
    e = emu_bn_bwd(dout, out, y, stats, gamma, 'relu6', parts=parts, **kw)
    passes(e['dy'], r['dy'], r['dy_mag'], 'apply-only dy')
    passes(e['dy2'], r['dy2'], r['dy2_mag'], 'apply-only dy2')
    e = emu_bn_bwd(dout, out, y, stats, gamma, 'relu6', parts=parts, bug='replica0_only', **kw)
    rejects(e['dy'], r['dy'], r['dy_mag'], 'replica 0 only')


# ------------------------------------------------------------------------------ running statistics
def emu_running(rm, rv, passes_, momentum=0.1, biased=False):
    rm, rv = rm.clone(), rv.clone()
    m = torch.tensor(momentum)
    for st, n, cnt in passes_:
        cnt = torch.tensor(float(cnt))
        for g in range(n):
            mean = st[g, 0] / cnt
            var = (st[g, 1] / cnt - mean * mean).clamp(min=0)
            if not biased:
                var = var * (cnt / torch.clamp(cnt - 1, min=1))
            rm = (1 - m) * rm + m * mean
            rv = (1 - m) * rv + m * var
    return rm, rv


@pytest.mark.parametrize('li', range(len(ko.RUNNING_LAYERS)))
def test_running_statistics_recurrence(li):
    C, ntr, nsc, _, ctr, csc = ko.RUNNING_LAYERS[li]
    rm0, rv0, st_tr, st_sc = ko.bn_running_case(li)
    rm, rv = ko.bn_running_ref(rm0, rv0, st_tr, ntr, float(ctr), st_sc, nsc, float(csc))
    tol = 1e-5 * (rm.abs() + rv.abs() + 1)
    a, b = emu_running(rm0, rv0, [(st_tr, ntr, ctr), (st_sc, nsc, csc)])
    assert ko.assert_tol(a, rm, tol, 'rmean') <= 0.5 and ko.assert_tol(b, rv, tol, 'rvar') <= 0.5
    if ntr and nsc:
        a, b = emu_running(rm0, rv0, [(st_sc, nsc, csc), (st_tr, ntr, ctr)])
        with pytest.raises(AssertionError):
            ko.assert_tol(a, rm, tol, 'score groups folded first')
    if ctr > 1 or nsc:
        a, b = emu_running(rm0, rv0, [(st_tr, ntr, ctr), (st_sc, nsc, csc)], biased=True)
        with pytest.raises(AssertionError):
            ko.assert_tol(b, rv, tol, 'biased variance')


# ------------------------------------------------------------------------------ pooling
pool_data = ko.pool_data


def emu_maxpool(x, k, s, p, last_wins=False):
    best = arg = None
    for t, (v, inside) in enumerate(ko._taps(x.double(), k, s, p, float('-inf'))):
        v = v.float()
        if best is None:
            best, arg = torch.full_like(v, -3.4e38), torch.zeros(v.shape, dtype=torch.uint8)
        win = ((v >= best) if last_wins else (v > best)) & inside[None, :, :, None]
        best, arg = torch.where(win, v, best), torch.where(win, torch.full_like(arg, t), arg)
    return best.to(BF16), arg


def emu_maxpool_bwd(dy, arg, H, W, k, s, p):
    return ko.maxpool_bwd_ref(dy.float(), arg, H, W, k, s, p)[0].float().to(BF16)


@pytest.mark.parametrize('kind', ['random', 'ties'])
@pytest.mark.parametrize('shape', ko.POOL_SHAPES)
@pytest.mark.parametrize('k,s,p', ko.POOL_KSP + [(3, 3, 0)])
def test_max_pool_first_maximum_and_backward(k, s, p, shape, kind):
    N, H, W, C = shape
    x = pool_data(shape, kind, k * 10 + s)
    ref, tap = ko.maxpool_ref(x, k, s, p)
    import torch.nn.functional as Fn
    tref = Fn.max_pool2d(x.float().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    assert torch.equal(ref.float(), tref)
    y, arg = emu_maxpool(x, k, s, p)
    assert torch.equal(y.double(), ref) and torch.equal(arg, tap)
    P, Q = ref.shape[1:3]
    dy = ko.pool_grad((N, P, Q, C))
    dref, dmag = ko.maxpool_bwd_ref(dy, tap, H, W, k, s, p)
    # the reference routes like autograd where no window holds a tie
    if kind == 'random':
        xx = x.float().permute(0, 3, 1, 2).requires_grad_(True)
        Fn.max_pool2d(xx, k, s, p).backward(dy.float().permute(0, 3, 1, 2))
        cnt = sum((v == ref).double() * m[None, :, :, None] for v, m in ko._taps(x.double(), k, s, p, float('-inf')))
        if float(cnt.max()) == 1:
            assert torch.allclose(xx.grad.permute(0, 2, 3, 1).double(), dref, atol=1e-6)
    passes(emu_maxpool_bwd(dy, arg, H, W, k, s, p), dref, dmag, 'max pool backward')
    if (k, s, p) == (3, 3, 0) and H == 11:
        assert (dmag[:, 9:] == 0).all() and (dmag[:, :, 6:] == 0).all()
    if kind == 'ties':
        y2, arg2 = emu_maxpool(x, k, s, p, last_wins=True)
        assert torch.equal(y2, y) and not torch.equal(arg2, tap)
        rejects(emu_maxpool_bwd(dy, arg2, H, W, k, s, p), dref, dmag, 'the last maximum wins a tie')


@pytest.mark.parametrize('shape', ko.POOL_SHAPES)
@pytest.mark.parametrize('k,s,p', ko.POOL_KSP)
def test_avg_pool_divides_by_the_window(k, s, p, shape):
    x = pool_data(shape, 'random', k * 10 + s)
    ref, mag = ko.avgpool_ref(x, k, s, p)
    import torch.nn.functional as Fn
    tref = Fn.avg_pool2d(x.double().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    assert torch.allclose(ref, tref, atol=1e-12)
    taps = ko._taps(x.double(), k, s, p, 0.0)
    acc = torch.zeros_like(taps[0][0], dtype=F32)
    n_in = torch.zeros(taps[0][1].shape)
    for v, inside in taps:
        acc = acc + v.float()
        n_in = n_in + inside.float()
    passes((acc / float(k * k)).to(BF16), ref, mag, 'avg pool emulation')
    if p:
        rejects((acc / n_in[None, :, :, None]).to(BF16), ref, mag, 'divides by the in-image taps')


# ------------------------------------------------------------------------------ classifier head
def lane_dot(h, w, b):
    """logits[b][k] as the kernels form them: 64 lane partials over c = lane, lane + 64, ...,
    then their total."""
    B, C = h.shape
    pad = (-C) % 64
    hp = torch.nn.functional.pad(h, (0, pad)).view(B, 1, -1, 64)
    wp = torch.nn.functional.pad(w, (0, pad)).view(1, w.shape[0], -1, 64)
    return (hp * wp).sum(2).sum(2) + b


def emu_head(act, w, b, label, isw, mode, bug=None):
    B, HW, C = act.shape
    K = w.shape[0]
    s = torch.zeros(B, C)
    for hw in range(HW):
        s = s + act[:, hw].float()
    pooled = s * (torch.tensor(1.0) / HW)
    logits = lane_dot(pooled, w, b)
    if bug == 'chunk_tail_unwritten':
        logits[:, K - K % 16:] = 0.0          # the buffer's previous contents
    mx = logits.max(1, keepdim=True).values
    lse = mx[:, 0] + torch.log(torch.exp(logits - mx).sum(1))
    lab = label.long()
    loss = lse - logits.gather(1, lab[:, None])[:, 0]
    wi = torch.ones(B) if (mode == 'eval' and bug != 'eval_weighted') else isw
    scale = 1.0 / isw if bug == 'no_1_over_B' else 1.0 / (B * isw)
    d = torch.exp(logits - lse[:, None])
    d[torch.arange(B), lab] -= 1
    if bug == 'last_argmax':
        am = K - 1 - torch.argmax((logits == mx).flip(1).to(torch.int8), 1)
    else:
        am = torch.argmax((logits == mx).to(torch.int8), 1)
    terms = loss * wi if bug == 'loss_times_w' else loss / wi
    g = torch.sqrt((d * d).sum(1) * ((pooled * pooled).sum(1) + 1))
    return dict(pooled=pooled, logits=logits, losses=loss, dlogits=d * scale[:, None],
                meters=(float(terms.sum()), float(B), float((am == lab).sum())), gradnorm=g)


head_case = ko.head_case


def check_head(e, r, mode):
    passes(e['pooled'], r['pooled'], r['pooled_mag'], 'head pooled')
    passes(e['logits'], r['logits'], r['logits_mag'], 'head logits')
    assert ko.assert_tol(e['losses'], r['losses'], r['losses_tol'], 'head losses') <= 0.5
    assert ko.assert_tol(e['gradnorm'], r['gradnorm'], r['gradnorm_tol'], 'head gradnorm') <= 0.5
    if mode == 'train':
        assert ko.assert_tol(e['dlogits'], r['dlogits'], r['dlogits_tol'], 'head dlogits') <= 0.5
    want, tol = r['meter0_' + mode]
    assert abs(e['meters'][0] - want) <= tol / 2
    assert e['meters'][1] == r['pooled'].shape[0]
    assert r['correct'][0] <= e['meters'][2] <= r['correct'][1]


@pytest.mark.parametrize('B,HW,C,K,wscale', ko.HEAD_SAMPLE_CASES + ko.HEAD_CHUNK_CASES[1:]
                         + ko.HEAD_WIDE_CASES + [ko.HEAD_RANGE_CASE])
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_head_fp32_emulation_meets_the_tolerances(B, HW, C, K, wscale, mode):
    act, w, b, label, isw = head_case(B, HW, C, K, wscale)
    r = ko.head_ref(act, w, b, label, isw)
    check_head(emu_head(act, w, b, label, isw, mode), r, mode)


def test_head_wrong_variants_are_rejected():
    B, HW, C, K = 5, 16, 1280, 100
    act, w, b, label, isw = head_case(B, HW, C, K)
    r = ko.head_ref(act, w, b, label, isw)
    want, tol = r['meter0_train']
    e = emu_head(act, w, b, label, isw, 'train', bug='loss_times_w')
    assert abs(e['meters'][0] - want) > tol
    e = emu_head(act, w, b, label, isw, 'train', bug='no_1_over_B')
    with pytest.raises(AssertionError):
        ko.assert_tol(e['dlogits'], r['dlogits'], r['dlogits_tol'], 'no 1/B')
    e = emu_head(act, w, b, label, isw, 'train', bug='chunk_tail_unwritten')
    rejects(e['logits'], r['logits'], r['logits_mag'], 'last 4 classes unwritten')
    with pytest.raises(AssertionError):
        ko.assert_tol(e['losses'], r['losses'], r['losses_tol'], 'last 4 classes unwritten')
    want, tol = r['meter0_eval']
    assert abs(emu_head(act, w, b, label, isw, 'eval')['meters'][0] - want) <= tol / 2
    assert abs(emu_head(act, w, b, label, isw, 'eval', bug='eval_weighted')['meters'][0] - want) > tol
    # an argmax tie: rows 3 and 77 identical and largest, every label 77
    act, w, b, label, isw = head_case(B, HW, C, K, tie=(3, 77))
    r = ko.head_ref(act, w, b, label, isw)
    assert (r['argmax'] == 3).all() and r['correct'] == (0, 0)
    assert emu_head(act, w, b, label, isw, 'eval')['meters'][2] == 0
    assert emu_head(act, w, b, label, isw, 'eval', bug='last_argmax')['meters'][2] == B
    # without the max subtraction a wide logit range overflows
    act, w, b, label, isw = head_case(*ko.HEAD_RANGE_CASE)
    r = ko.head_ref(act, w, b, label, isw)
    lg = r['logits']
    assert float((lg.max(1).values - lg.min(1).values).min()) > 100 and float(lg.max()) > 89
    naive = torch.log(torch.exp(lg.float()).sum(1)) - lg.float().gather(1, label.long()[:, None])[:, 0]
    assert not torch.isfinite(naive).all()


@pytest.mark.parametrize('HW,C', ko.HEAD_POOL_BN_CASES)
def test_head_pool_bn_emulation(HW, C):
    B, gi = 12, 4
    x3, gamma, beta, stats, res, rm, rv, w, b, label = ko.head_pool_bn_case(HW, C)
    inv = torch.tensor(1.0 / (gi * HW))
    for act in ('none', 'relu', 'relu6'):
        for r in (None, res):
            for running in (False, True):
                ref, mag = ko.head_pool_bn_ref(x3, r, stats, gamma, beta, gi * HW, gi, act, 1e-5,
                                               (rm, rv) if running else None)
                if running:
                    sc, sh = scale_shift32(None, None, None, gamma, beta, running=(rm, rv))
                    sc, sh = sc[None].expand(3, C), sh[None].expand(3, C)
                else:
                    sc, sh = scale_shift32(stats[:, 0], stats[:, 1], inv, gamma, beta)
                for bug in (False, True):
                    if bug and running:
                        continue
                    grp = torch.arange(B) % (B // gi) if bug else torch.arange(B) // gi
                    v = x3.float() * sc[grp][:, None] + sh[grp][:, None]
                    v = act32(v if r is None else v + r.float(), act)
                    out = v.sum(1) * torch.tensor(1.0 / HW)
                    (rejects if bug else passes)(out, ref, mag, 'head_pool_bn group index')


@pytest.mark.parametrize('B,HW,C,K,gemm', ko.HEAD_BWD_CASES)
def test_head_bwd_emulation(B, HW, C, K, gemm):
    pooled, dlog, w = ko.head_bwd_case(B, C, K)
    r = ko.head_bwd_ref(pooled, dlog, w, HW)
    passes(((dlog @ w) / HW).to(BF16), r['dact'], r['dact_mag'], 'head_bwd dact')
    passes(dlog.t() @ pooled, r['dw'], r['dw_mag'], 'head_bwd dw')
    passes(dlog.sum(0), r['db'], r['db_mag'], 'head_bwd db')
    if HW > 1:
        rejects((dlog @ w).to(BF16), r['dact'], r['dact_mag'], 'head_bwd without 1 / HW')


@pytest.mark.parametrize('B', ko.MLP_BATCHES)
def test_mlp_head_emulation(B):
    F, H1, K = ko.MLP_DIMS
    x, w1, b1, w2, b2, label, isw = ko.mlp_case(B)
    g = ko.gen(B + 1)
    f = ko.mlp_fwd_ref(x, w1, b1, w2, b2)
    # split-R: two slices added in turn, slice 0 carrying the bias
    sl = [slice(0, 128), slice(128, 200)]
    h1 = sum((x.float()[:, s] @ w1.float()[:, s].t()) + (b1 if i == 0 else 0) for i, s in enumerate(sl))
    logits = h1 @ w2.t() + b2
    passes(h1, f['h1'], f['h1_mag'], 'mlp h1')
    passes(logits, f['logits'], f['logits_mag'], 'mlp logits')
    bad = sum((x.float()[:, s] @ w1.float()[:, s].t()) + b1 for s in sl)
    rejects(bad, f['h1'], f['h1_mag'], 'every split-R slice adds the bias')
    dlog = torch.randn(B, K, generator=g) / B
    q = ko.mlp_bwd_ref(dlog, h1, x, w1, w2)
    dh1 = dlog @ w2
    emu = dict(dw2=dlog.t() @ h1, db2=dlog.sum(0), dh1=dh1, db1=dh1.sum(0),
               dw1=dh1.t() @ x.float(), dx=(dh1 @ w1.float()).to(BF16))
    for name, out in emu.items():
        passes(out, q[name], q[name + '_mag'], 'mlp ' + name)
    rejects((dh1.t() @ x.float()) * 1.001, q['dw1'], q['dw1_mag'], 'dw1 off by 1e-3')


# ------------------------------------------------------------------------------ front-end
def test_head_fwd_refuses_gradnorm_over_ready_logits_without_pooled():
    """With logits given the loss kernel reads pooled[] for the gradnorm score: a null pointer.
    Refused as the first statement: CPU tensors never reach the device checks."""
    from mercury_amd.ops.head import head_fwd
    B, HW, C, K = 2, 1, 64, 64
    with pytest.raises(ValueError, match='gradnorm score over ready logits reads pooled'):
        head_fwd(torch.zeros(B, HW, C, dtype=BF16), torch.zeros(K, C), torch.zeros(K),
                 torch.zeros(B, dtype=torch.int32), B, HW, C, K, 'score', pooled=None,
                 logits=torch.zeros(B, K), losses=torch.zeros(B), score='gradnorm')


def test_streaming_stores_restores_the_default(monkeypatch):
    from mercury_amd.ops import bn

    class Lib:
        calls = []

        def bn_configure(self, n):
            self.calls.append(n)

    fake = Lib()
    monkeypatch.setattr(bn, 'lib', lambda: fake)
    assert bn.NT_MIN_BYTES == 256 << 20
    with bn.streaming_stores(0):
        assert fake.calls == [0]
    with pytest.raises(KeyError):
        with bn.streaming_stores(1 << 62):
            raise KeyError('x')
    assert fake.calls == [0, bn.NT_MIN_BYTES, 1 << 62, bn.NT_MIN_BYTES]
