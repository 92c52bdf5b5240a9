"""Draw-by-draw tests of the global importance table (``csrc/table.hip``: table_partial_kernel,
table_prep_kernel, table_draw_kernel, table_weights_kernel).

Every draw is ``philox4x32(counter snapshot, d, 0x7ab1e5; seed, 0x1B873593)``;
``sampler_oracles`` replays it and forms the kernel's fp64 uniform, so each of a case's 20 000
draws is checked on its own: the pick q must be a member of the group and must satisfy

    cdf64[q-1] - eps <= u < cdf64[q] + eps,      eps = C * 2**-24 * total,

with the fp64 CDF of ``imp_i + mean64`` over the members in index order.  C (``table_C``): all
terms are >= 0, so every fp32 addition costs at most 2**-24 of the running sum.  A segment's
masked sum carries 8 + 6 + 4 = 18 additions, the group sum ``per`` + 22 more and the mean one
division, so the mean, every entry of the fp64 prefix and the total that scales the uniform are
within 41 + per each; inside the drawn segment the fp32 remainder (1), the weights (1), 32 adds
in 8 chunks (40), the wave scan (6), ``incl - ls`` (1) and the owner's walk (33) give 82:
C = 2 * (41 + per) + 82 = 166 (168 above 1024 segments).  Groups have at most about 2000
members, so the smallest weight (the mean: total / 2n) is 25 eps or more and a pick that is off
by one member fails.  ``group_stats()``: the count is exact, mean and total within the same C.

Observed on the MI355X: the worst draw of any case lies 0.0077 eps outside its fp64 interval
(edge_2049; 0.0029 above 1024 segments), the mean is within 0.013 and the total within 0.0099 of
their bounds (chunk_2149), the count is exact; ``draw_batch`` weights are within 1 ulp (bound 4).
The bound is a worst case over some 170 roundings; what matters is that it stays 25 times below
the smallest member's weight.  The slowest test took 0.10 s, the parent's slowest chi-square
test of the table 0.24 s.

One boundary rule is beyond any draw test: ``prefix[mid] <= u`` against ``<`` in the segment
search differs only where the 53-bit product ``u01 * total`` equals a segment prefix bit for
bit (at most nseg * 2**-53 per draw), so that mutant passes here as it passes everywhere.

Pinned, as the kernels behave today:

* a group whose members' importance is all exactly zero draws -1, like an empty group (its total
  weight ``sum + count * mean`` is zero);
* ``scatter`` drops the indices -1 and N and leaves entries 0 and N-1 untouched by them.
"""
import numpy as np
import pytest
import torch

import sampler_oracles as so

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = np.float32
STAMP, OTHER = 3, 7
NDRAW = 20_000
SEED = 5
TSEG = so.TSEG


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _table(N, members, seed=0, zeros=True):
    """A table whose ``members`` carry STAMP and ``rand * 4`` (some exact zeros); every other
    entry carries another stamp and an importance hundreds of times larger."""
    rng = np.random.default_rng(seed)
    members = np.unique(np.asarray(members, np.int64))
    imp = (rng.random(N) * 1000 + 500).astype(F32)
    grp = np.full(N, OTHER, np.int32)
    v = (rng.random(len(members)) * 4).astype(F32)
    if zeros and len(members) > 4:
        v[rng.choice(len(members), max(1, len(members) // 16), replace=False)] = 0
    imp[members] = v
    grp[members] = STAMP
    t = _ops().ImportanceTable(N, DEV)
    t.importance.copy_(torch.from_numpy(imp))
    t.group.copy_(torch.from_numpy(grp))
    return t, imp, grp


def _check(t, imp, grp, name, counter=0, ndraw=NDRAW, preset=True, **kw):
    """One ``sample`` call at the given counter (``preset=False``: the table's own counter has
    to stand there already): every draw and the scalars."""
    if preset:
        t.counter.fill_(counter)
    out = t.sample(ndraw, STAMP, seed=SEED, **kw)
    members, cdf, mean, total = so.table_reference(imp, grp, STAMP)
    C = so.table_C(len(imp))
    ok, worst = so.table_draw_violation(out.cpu().numpy(), members, cdf, total, counter, SEED, C)
    assert ok, 'drew a non-member'
    gm, gc, gt = t.group_stats()
    sm, st = abs(gm - mean) / (C * so.ULP * mean), abs(gt - total) / (C * so.ULP * total)
    print('\n%s: worst draw %.4f of eps (C = %d), mean %.4f, total %.4f' % (name, worst, C, sm, st))
    assert worst < 1
    assert gc == len(members) and sm <= 1 and st <= 1
    assert int(t.counter.item()) == counter + 1
    return out


def _spread(rng, lo, hi, n):
    return lo + rng.choice(hi - lo, min(n, hi - lo), replace=False)


def _cases():
    rng = np.random.default_rng(1)
    c = {}
    for N in (1, 7, 13):                                   # below 8: only the scalar tails run
        c['small_%d' % N] = (N, np.arange(N))
    for N in (2047, 2048, 2049):                           # segment edges, members at both ends
        c['edge_%d' % N] = (N, np.concatenate([[0, N - 1], _spread(rng, 0, N, 300)]))
    for N in (2048 + 98, 2048 + 101):                      # e + 4 <= N against the scalar path
        c['chunk_%d' % N] = (N, np.concatenate([[N - 3, N - 2, N - 1], _spread(rng, 0, N, 300)]))
    c['tail_5003'] = (5003, np.arange(4990, 5003))
    N = 10 * TSEG                                          # zero-weight segments around the group
    c['last_segment'] = (N, _spread(rng, 9 * TSEG, N, 400))
    c['first_segment'] = (N, _spread(rng, 0, TSEG, 400))
    c['segments_2_and_7'] = (N, np.concatenate([_spread(rng, 2 * TSEG, 3 * TSEG, 300),
                                                _spread(rng, 7 * TSEG, 8 * TSEG, 300)]))
    c['single_member'] = (5003, np.array([2500]))
    return c


CASES = _cases()


@pytest.mark.parametrize('name', list(CASES))
def test_every_draw_is_the_cdf_pick(name):
    N, members = CASES[name]
    t, imp, grp = _table(N, members)
    out = _check(t, imp, grp, name)
    if name == 'single_member':
        assert bool((out == 2500).all())
    if name.startswith('chunk') or name.startswith('edge') or name == 'tail_5003':
        assert int(out.max()) == N - 1, 'the last entry is a member and 20 000 draws reach it'


@pytest.fixture(scope='module')
def big():
    """More than 1024 segments (per = 2 in table_prep_kernel): about 1500 members over the first,
    a middle and the last segments, one of them at N-1."""
    rng = np.random.default_rng(2)
    N = TSEG * 1030 + 5
    members = np.concatenate([_spread(rng, 0, TSEG, 500), _spread(rng, 515 * TSEG, 516 * TSEG, 500),
                              _spread(rng, 1029 * TSEG, N - 1, 500), [N - 1]])
    return _table(N, members)


def test_more_than_1024_segments(big):
    t, imp, grp = big
    assert so.table_C(len(imp)) == 168
    out = _check(t, imp, grp, 'segments_1031')
    assert int(out.max()) >= 1029 * TSEG and int(out.min()) < TSEG


def test_stamp_source_and_output_form(big):
    """The stamp as a device scalar and as a host int draw the same; ``out`` and ``out32`` given
    together agree."""
    t, imp, grp = big
    host = _check(t, imp, grp, 'host_stamp', counter=11)
    t.counter.fill_(11)
    dev = t.sample(NDRAW, 99, seed=SEED, group_dev=torch.tensor([STAMP], dtype=torch.int64,
                                                                  device=DEV))
    assert torch.equal(host, dev)
    o64 = torch.full((NDRAW,), -5, dtype=torch.int64, device=DEV)
    o32 = torch.full((NDRAW,), -5, dtype=torch.int32, device=DEV)
    _check(t, imp, grp, 'both_outputs', counter=11, out=o64, out32=o32)
    assert torch.equal(o64, host) and torch.equal(o32.long(), host)


def test_counter_snapshot_is_the_generator_counter():
    """A second call draws the replica's draws for counter + 1; the high word counts."""
    N, members = CASES['edge_2049']
    t, imp, grp = _table(N, members)
    a = _check(t, imp, grp, 'counter_0', counter=0)
    b = _check(t, imp, grp, 'counter_1', counter=1, preset=False)   # advanced on its own
    assert not torch.equal(a, b)
    hi = _check(t, imp, grp, 'counter_hi', counter=2 ** 32 + 3)
    lo = _check(t, imp, grp, 'counter_lo', counter=3)
    assert not torch.equal(hi, lo)


def test_pinned_zero_group_and_scatter_bounds():
    N = 5003
    t, imp, grp = _table(N, np.arange(100, 140), zeros=False)
    t.importance[100:140] = 0
    assert bool((t.sample(64, STAMP, seed=SEED) == -1).all())       # all-zero group: like empty
    assert bool((t.sample(64, 99, seed=SEED) == -1).all())          # empty group
    assert t.group_stats() == (0.0, 0, 0.0)
    before_i, before_g = t.importance.clone(), t.group.clone()
    index = torch.tensor([-1, N, 17], dtype=torch.int32, device=DEV)
    t.scatter(index, torch.tensor([9.0, 8.0, 7.0], device=DEV), group_index=55)
    before_i[17], before_g[17] = 7.0, 55
    assert torch.equal(t.importance, before_i) and torch.equal(t.group, before_g)


# ---- draw_batch / table_weights_kernel ------------------------------------------------------
def _batch(members, Ns=1000, P=320, start=900, nd=NDRAW, stamp=STAMP):
    t, imp, grp = _table(Ns, members)
    pool_index = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    pool_index[0] = start
    pos = torch.full((nd,), -9, dtype=torch.int32, device=DEV)
    idx = torch.full((nd,), -9, dtype=torch.int32, device=DEV)
    isw = torch.full((nd,), float('nan'), device=DEV)
    meters = torch.full((8,), -1.0, device=DEV)
    st = torch.tensor([stamp], dtype=torch.int64, device=DEV)
    t.draw_batch(nd, st, pos, pool_index, Ns, P, idx, isw, seed=SEED, meters=meters)
    return t, imp, grp, pos.cpu().numpy().astype(np.int64), idx.cpu().numpy(), \
        isw.cpu().numpy(), meters.cpu().numpy()


def test_draw_batch_wrapping_slice():
    """The slice wraps the shard: positions 900..999, 0..219 are slots 0..319."""
    members = np.concatenate([np.arange(900, 1000), np.arange(0, 220)])
    t, imp, grp, pos, idx, isw, meters = _batch(members)
    mem, cdf, mean, total = so.table_reference(imp, grp, STAMP)
    ok, worst = so.table_draw_violation(pos, mem, cdf, total, 0, SEED, so.table_C(1000))
    assert ok and worst < 1
    assert np.array_equal(idx, (pos - 900) % 1000) and idx.min() == 0 and idx.max() == 319
    assert set(np.unique(pos)) == set(members.tolist())
    ref = len(mem) * (imp[pos].astype(np.float64) + mean) / total
    ulps = so.ulps32(isw, ref.astype(F32))
    print('\nweights: worst %d ulp' % ulps.max())
    assert ulps.max() <= 4
    gm = t.group_stats()[0]
    assert meters[3] == F32(gm) and abs(gm - mean) <= so.table_C(1000) * so.ULP * mean
    assert np.all(meters[[0, 1, 2, 4, 5, 6, 7]] == -1)


def test_draw_batch_clamps_a_slot_beyond_the_pool():
    """Members behind the slice (positions 220..299 are slots 320..399) land on slot P - 1."""
    members = np.concatenate([np.arange(900, 1000), np.arange(0, 300)])
    t, imp, grp, pos, idx, isw, meters = _batch(members)
    slot = (pos - 900) % 1000
    assert slot.max() > 319
    assert np.array_equal(idx, np.minimum(slot, 319))


def test_draw_batch_empty_group():
    t, imp, grp, pos, idx, isw, meters = _batch(np.arange(900, 1000), stamp=99)
    assert np.all(pos == -1) and np.all(idx == 0) and np.all(isw == F32(1))
    assert meters[3] == 0
