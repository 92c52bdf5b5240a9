"""fp64 references for the classifier head's label smoothing and top-k count.

A helper module (no tests, no fixtures) on top of ``kernel_oracles.head_ref``, whose constants
(``T_b`` = sample b's largest logit tolerance, ``ko.K = 1e-5``) every tolerance here is made of.

Label smoothing s (``F.cross_entropy(z, y, label_smoothing=s)``), lse = logsumexp(z), K classes:

    loss_s = (1 - s) (lse - z[y]) + s (lse - mean_k z[k])
    dz[k]  = softmax(z)[k] - (1 - s) [k == y] - s / K

Tolerances (``smooth_ref``):
    loss_s    2 T_b + 1e-5 max(1, |lse|) + s * 1e-5 * mean_k |z|   (the new term: the fp32 mean
              of K logits, whose relative error is what ko.K covers)
    dlogits   scale_b (p (2 T_b + 1e-5) + 2e-7)   (head_ref's bound has 1e-7 as its absolute
              term; the second 1e-7 is the one extra fp32 rounding of a target of magnitude <= 1)
    meters[0] sum_b tol_b / w_b + ko.K * sum_b |loss_s / w_b|, as head_ref forms meter0_train

Top-k (``rank_ref``, ``topk_bounds``): rank = #{k : z[k] > z[y]} + #{k < y : z[k] == z[y]} (the
lower index wins a tie, so rank 0 is "argmax == y"); a hit iff z[y] is not NaN and rank < k.  In
fp32 a logit may sit T_b off, so a sample is a sure hit when fewer than k other logits satisfy
z + T >= z[y] - T, a sure miss when at least k satisfy z - T > z[y] + T, and ambiguous
otherwise; the bounds are [sure hits, sure hits + ambiguous].

Labels are chosen, not random (``rank_labels``): sample b gets the class whose fp64 rank is
b mod (k + 2), so hits and misses on both sides of the boundary occur and the expected count is
neither 0 nor B.  (With ``head_case``'s random labels most shapes have no top-5 hit at all, and
a kernel that never wrote the meter would pass.)  The cases below contain no ambiguous sample
under these labels -- tests/test_head_smooth.py asserts it -- so [lo, hi] is one number.
"""
import functools

import torch

import kernel_oracles as ko

F64 = ko.F64
SMOOTH = [0.1, 0.5]
TOPK = [1, 2, 5]

# (path, (B, HW, C, K)) -- path: the dispatch the case runs on ('sample': logits=None)
CASES = [('sample', (1, 16, 512, 10)), ('sample', (9, 16, 512, 10)), ('sample', (9, 1, 1280, 100)),
         ('chunk', ko.HEAD_CHUNK_CASES[1][:4]), ('wide', ko.HEAD_WIDE_CASES[0][:4]),
         ('mlp', (5,))]
assert CASES[3][1] == (5, 16, 328, 65) and CASES[4][1] == (5, 16, 1056, 1000)


def rank_ref(logits, label):
    """Rank of every sample's label by the rule above ([B] int64) and the NaN-label mask."""
    z = logits
    y = label.long()
    zy = z.gather(1, y[:, None])
    before = torch.arange(z.shape[1], device=z.device)[None, :] < y[:, None]
    rank = ((z > zy) | ((z == zy) & before)).sum(1)
    return rank, zy[:, 0] != zy[:, 0]


def rank_labels(logits, k):
    """Label of sample b: the class whose rank among b's fp64 logits is b mod (k + 2)."""
    B, K = logits.shape
    # (stable: the lower index comes first among equal logits)
    order = torch.sort(logits, dim=1, descending=True, stable=True).indices
    want = (torch.arange(B, device=logits.device) % (k + 2)) % K
    return order.gather(1, want[:, None])[:, 0].int()


def topk_bounds(logits, label, T, k):
    """(lo, hi, ambiguous [B] bool): the top-k hit count's bounds when every logit may be T_b
    off."""
    z = logits
    y = label.long()
    zy = z.gather(1, y[:, None])
    other = torch.arange(z.shape[1], device=z.device)[None, :] != y[:, None]
    t = T[:, None]
    maybe_above = (other & (z + t >= zy - t)).sum(1)
    sure_above = (other & (z - t > zy + t)).sum(1)
    sure_hit, sure_miss = maybe_above < k, sure_above >= k
    amb = ~(sure_hit | sure_miss)
    return int(sure_hit.sum()), int((sure_hit | amb).sum()), amb


def smooth_ref(r, label, s):
    """From ``r = ko.head_ref(...)`` (computed with the same labels and isw): the smoothed
    per-sample loss, dlogits and the train meter, each with its tolerance."""
    logits, lse, p, scale, T = r['logits'], r['lse'], r['p'], r['scale'], r['T']
    B, K = logits.shape
    loss_s = (1 - s) * r['losses'] + s * (lse - logits.mean(1))
    loss_tol = r['losses_tol'] + s * 1e-5 * logits.abs().mean(1)
    d = p - s / K
    d[torch.arange(B), label.long()] -= 1 - s
    wi = 1 / (B * scale)
    terms = loss_s / wi
    return {'loss': loss_s, 'loss_tol': loss_tol,
            'dlogits': d * scale[:, None],
            'dlogits_tol': scale[:, None] * (p * (2 * T[:, None] + 1e-5) + 2e-7),
            'meter0': (float(terms.sum()), float((loss_tol / wi).sum() + ko.K * terms.abs().sum()))}


def ref_from_logits(logits, label, isw):
    """``ko.head_ref`` on given fp32 logits (``logits_mag`` = |logits|)."""
    K = logits.shape[1]
    z = logits.to(F64)
    eye = torch.eye(K, dtype=F64, device=z.device)
    return ko.head_ref(None, eye, torch.zeros(K, dtype=F64, device=z.device), label, isw,
                       pooled=z, logits_mag=z.abs())


@functools.lru_cache(maxsize=None)
def case(ci, k, device='cpu'):
    """Case ``CASES[ci]`` with labels chosen for top-``k``: the kernel inputs, ``ref`` (head_ref
    under those labels), ``rank`` and ``topk`` = (lo, hi, ambiguous).  Computed once, shared."""
    path, shape = CASES[ci]
    c = {'path': path, 'k': k}
    if path == 'mlp':
        x, w1, b1, w2, b2, label, isw = ko.mlp_case(shape[0], device)
        f = ko.mlp_fwd_ref(x, w1, b1, w2, b2)
        F_, H1, K = ko.MLP_DIMS
        c.update(B=shape[0], F=F_, H1=H1, K=K, x=x, w1=w1, b1=b1, w2=w2, b2=b2, isw=isw)
        logits = f['logits']
        c['label'] = label = rank_labels(logits, k)
        c['ref'] = ko.head_ref(None, w2, b2, label, isw, pooled=f['h1'], logits_mag=f['logits_mag'])
    else:
        B, HW, C, K = shape
        act, w, b, label, isw = ko.head_case(B, HW, C, K, device=device)
        c.update(B=B, HW=HW, C=C, K=K, act=act, w=w, b=b, isw=isw)
        logits = ko.head_ref(act, w, b, label, isw)['logits']
        c['label'] = label = rank_labels(logits, k)
        c['ref'] = ko.head_ref(act, w, b, label, isw)
    c['rank'] = rank_ref(logits, label)[0]
    c['topk'] = topk_bounds(logits, label, c['ref']['T'], k)
    return c
