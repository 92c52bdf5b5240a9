"""Tail, group and dispatch-path tests of the streaming BN kernels (csrc/bn.hip) against the
fp64 references and the elementwise criterion of ``kernel_oracles``.

Shapes are chosen for the paths the friendly shapes never take: channel counts whose C/8 does
not divide the grid (``stride = T - T % C8``), more than one trip of the U = 4 unrolled loops
with a partial last trip, a short last ghost group, every act x residual instantiation, the
streaming-store variant, the 2048-channel limit, and a multi-layer running-statistics table.

Largest measured (|err| - 2^-8 |ref|) / mag on an MI355X, against k = 1e-5:
    bn_apply (all forms, multi-trip included)      1.8e-7
    bn_bwd dy / dy2                                3.9e-7
    bn_bwd dz                                      0 (exact)
    bn_bwd sums, dgamma, dbeta (atomics)           1.1e-6 (beyond the xhat sums' sums_atol)
(0: every error was under the bf16 half-ulp term.)
"""
import functools

import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _run_apply(M, C, group_rows, act, res, running, seed, what=None):
    ops = _ops()
    y, stats, gamma, beta, kw = ko.bn_apply_case(M, C, group_rows, res, seed, running, DEV)
    out = torch.full((M, C), float('nan'), dtype=torch.bfloat16, device=DEV)
    ops.bn_apply(y, stats, gamma, beta, out, M, C, group_rows=group_rows, act=act, **kw)
    ref, mag = ko.bn_apply_ref(y, stats, gamma, beta, group_rows, act, **kw)
    gr = group_rows or M
    k = ko.assert_within(out, ref, mag, what=what or 'bn_apply %s/%s M=%d C=%d' % (act, res, M, C),
                         decode=dict(C=C, group_rows=gr, rpi=ko.bn_apply_rpi(M, C, gr)))
    ko.record('bn_apply', k)
    return out, (y, stats, gamma, beta, kw)


@pytest.mark.parametrize('case', ko.BN_APPLY_FORMS, ids=str)
def test_bn_apply_every_act_and_residual_form(case):
    _run_apply(*case)


@pytest.mark.parametrize('case', ko.BN_APPLY_CHANNELS, ids=str)
def test_bn_apply_channel_counts(case):
    """MobileNetV2's channel counts (T % C8 != 0) and C = 4096 at M = 2, where one block would
    not hold a full period of C8 chunks and grid_for's ``need`` raises the grid to two."""
    M, C = case[:2]
    if C == 4096:
        assert -(-M * (C // 8) // 1024) == 1 and ko.bn_grid(M * (C // 8), C // 8, 4, 2048) == 2
    _run_apply(*case)


@pytest.mark.parametrize('case', ko.BN_APPLY_SHORT_GROUP, ids=str)
def test_bn_apply_short_last_ghost_group(case):
    """G = 3, group_rows = 500, M = 1300: the last group has 300 rows and its own 1 / 300."""
    _run_apply(*case)


@pytest.mark.parametrize('case', ko.BN_APPLY_RUNNING, ids=str)
def test_bn_apply_running_statistics(case):
    """Eval form: (rmean, rvar) and, for a BN'd shortcut, its own (rmean2, rvar2)."""
    _run_apply(*case)


@functools.lru_cache(maxsize=None)
def _multi_trip():
    """The smallest shape with more than one trip (ko.BN_APPLY_MULTI_TRIP): re-load, clamped
    tail loads and the break of a partial trip.  fp64 reference on the device."""
    M, C, gr = ko.BN_APPLY_MULTI_TRIP[:3]
    assert ko.bn_apply_rpi(M, C, gr) == 682 and -(-M // gr) == 64 and M - 63 * gr == 1700
    return _run_apply(*ko.BN_APPLY_MULTI_TRIP, what='bn_apply multi-trip')


def test_bn_apply_multi_trip():
    _multi_trip()


@pytest.mark.parametrize('case', ko.BN_APPLY_STREAMING + [ko.BN_APPLY_MULTI_TRIP], ids=str)
def test_bn_apply_streaming_stores_bit_equal(case):
    """The nontemporal-store instantiations write the same bits as the ordinary ones."""
    ops = _ops()
    M, C, gr, act = case[:4]
    base, (y, stats, gamma, beta, kw) = _multi_trip() if case == ko.BN_APPLY_MULTI_TRIP \
        else _run_apply(*case)
    out = torch.full((M, C), float('nan'), dtype=torch.bfloat16, device=DEV)
    with ops.streaming_stores(0):
        ops.bn_apply(y, stats, gamma, beta, out, M, C, group_rows=gr, act=act, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), base.view(torch.int16))


# ------------------------------------------------------------------------------ bn_bwd
def _run_bwd(M, C, act, two, sparse, seed):
    ops = _ops()
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(M, C, act, two, sparse, seed, DEV)
    nan = float('nan')
    sums = torch.full((ops.sums_numel(C),), nan, device=DEV)      # bn_bwd zeroes it
    dy, dy2, dz = (torch.full((M, C), nan, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    dg, db, dg2, db2 = (torch.full((C,), nan, device=DEV) for _ in range(4))
    ops.bn_bwd(dout, out, y, stats, gamma, sums, dy, M, C, act=act, dz=dz, dgamma=dg, dbeta=db,
               dy2=dy2 if two else None, dgamma2=dg2 if two else None,
               dbeta2=db2 if two else None, **kw)
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, act, **kw)
    tag = 'bn_bwd %s two=%d sparse=%d M=%d C=%d ' % (act, two, sparse, M, C)
    dec_r = dict(C=C, rpi=ko.bn_bwd_rpi(M, C, 256))
    dec_a = dict(C=C, rpi=ko.bn_bwd_rpi(M, C, 2048))
    n = 3 if two else 2
    tot = ops.sums_total(sums, C)
    at = r['sums_atol']
    ko.record('bn_bwd_sums', ko.assert_within(tot[:n], r['sums'][:n], r['sums_mag'][:n],
                                              what=tag + 'sums', decode=dec_r, atol=at[:n]))
    ko.record('bn_bwd_sums', ko.assert_within(dg, r['sums'][1], r['sums_mag'][1], what=tag + 'dgamma',
                                              atol=at[1]))
    ko.record('bn_bwd_sums', ko.assert_within(db, r['sums'][0], r['sums_mag'][0], what=tag + 'dbeta'))
    ko.record('bn_bwd_dy', ko.assert_within(dy, r['dy'], r['dy_mag'], what=tag + 'dy', decode=dec_a))
    ko.record('bn_bwd_dz', ko.assert_within(dz, r['dz'], r['dz_mag'], what=tag + 'dz', decode=dec_a))
    if two:
        ko.assert_within(dg2, r['sums'][2], r['sums_mag'][2], what=tag + 'dgamma2', atol=at[2])
        ko.assert_within(db2, r['sums'][0], r['sums_mag'][0], what=tag + 'dbeta2')
        ko.record('bn_bwd_dy', ko.assert_within(dy2, r['dy2'], r['dy2_mag'], what=tag + 'dy2',
                                                decode=dec_a))
    else:
        assert torch.isnan(dy2.float()).all() and torch.isnan(dg2).all()


@pytest.mark.parametrize('case', ko.BN_BWD_SMALL, ids=str)
def test_bn_bwd_small(case):
    _run_bwd(*case)


@pytest.mark.parametrize('case', ko.BN_BWD_LARGE, ids=str)
def test_bn_bwd_large(case):
    """(22051, 96): the reduce kernel hits its 256-block cap (rpi = 5461) and gets a 207-row
    second trip; (13109, 320): the apply kernel runs several rows per thread."""
    M, C = case[:2]
    if C == 96:
        assert ko.bn_bwd_rpi(M, C, 256) == 5461 and M - 4 * 5461 == 207
    else:
        assert M > ko.bn_bwd_rpi(M, C, 2048)
    _run_bwd(*case)


def test_bn_bwd_without_optional_outputs():
    """dz = None and null parameter-gradient pointers: dy alone is written."""
    ops = _ops()
    M, C = ko.BN_BWD_NO_OPTIONAL[:2]
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(*ko.BN_BWD_NO_OPTIONAL, DEV)
    sums = torch.zeros(ops.sums_numel(C), device=DEV)
    dy = torch.full((M, C), float('nan'), dtype=torch.bfloat16, device=DEV)
    ops.bn_bwd(dout, out, y, stats, gamma, sums, dy, M, C, act='relu')
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, 'relu')
    ko.assert_within(dy, r['dy'], r['dy_mag'], what='bn_bwd dy only',
                     decode=dict(C=C, rpi=ko.bn_bwd_rpi(M, C, 2048)))


def test_bn_bwd_apply_only_folds_uneven_replicas():
    """reduce=False: the apply pass alone, over a known total spread unevenly (signs mixed, one
    replica empty) over the SUMS_R replicas."""
    ops = _ops()
    M, C = ko.BN_BWD_APPLY_ONLY[:2]
    dout, out, y, stats, gamma, kw = ko.bn_bwd_case(*ko.BN_BWD_APPLY_ONLY, DEV)
    r0 = ko.bn_bwd_ref(dout, out, y, stats, gamma, 'relu6', **kw)
    parts, totals, totals_mag = ko.replica_parts(r0['sums'], ops.sums_numel(C) // (3 * C))
    r = ko.bn_bwd_ref(dout, out, y, stats, gamma, 'relu6', totals=totals, totals_mag=totals_mag,
                      **kw)
    dy, dy2 = (torch.full((M, C), float('nan'), dtype=torch.bfloat16, device=DEV) for _ in range(2))
    dg, db, dg2, db2 = (torch.full((C,), float('nan'), device=DEV) for _ in range(4))
    sums = parts.view(-1).clone()
    ops.bn_bwd(dout, out, y, stats, gamma, sums, dy, M, C, act='relu6', dy2=dy2, dgamma=dg,
               dbeta=db, dgamma2=dg2, dbeta2=db2, reduce=False, **kw)
    assert torch.equal(sums, parts.view(-1))          # the apply pass only reads them
    dec = dict(C=C, rpi=ko.bn_bwd_rpi(M, C, 2048))
    ko.assert_within(dy, r['dy'], r['dy_mag'], what='apply-only dy', decode=dec)
    ko.assert_within(dy2, r['dy2'], r['dy2_mag'], what='apply-only dy2', decode=dec)
    for o, i in ((db, 0), (dg, 1), (dg2, 2), (db2, 0)):
        ko.assert_within(o, totals[i], totals_mag[i], what='apply-only parameter gradient %d' % i)


def test_bn_bwd_channel_limit():
    """C = 2048 fills the kernels' [3][2048] LDS arrays.  C = 2056 is refused by a default call
    before anything is launched: neither the sums workspace (which a default call zeroes first)
    nor dy is touched."""
    ops = _ops()
    _run_bwd(*ko.BN_BWD_LIMIT)
    M, C = 5, 2056
    z = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    dy = torch.full((M, C), 7.0, dtype=torch.bfloat16, device=DEV)
    sums = torch.full((ops.sums_numel(C),), 3.0, device=DEV)
    st, gm = torch.ones(2, C, device=DEV), torch.ones(C, device=DEV)
    with pytest.raises(ValueError, match='at most 2048'):
        ops.bn_bwd(z, z, z, st, gm, sums, dy, M, C, act='relu')
    torch.cuda.synchronize()
    assert (dy == 7).all() and (sums == 3).all()
    # the launcher's own refusal stands behind the front-end's
    with pytest.raises(RuntimeError, match='at most 2048'):
        ops.lib().bn_bwd(ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(st), ops.ptr(gm), 0, 0, 0,
                         ops.ptr(sums), ops.ptr(dy), 0, 0, 0, 0, 0, 0, M, C, 1, 1e-5,
                         ops.stream_ptr(), 3)
    torch.cuda.synchronize()
    assert (dy == 7).all() and (sums == 3).all()


# ------------------------------------------------------------------------------ bn_running
def test_bn_running_multi_layer_table():
    """Three layers of different C in one launch (maxC = 320 sizes the grid: the second block
    of the C = 24 layer does nothing, of the C = 264 layer 8 channels), n_score off the
    8-wide load batches, n_train = 0, nbt = null, cnt = 1."""
    ops = _ops()
    layers = ko.RUNNING_LAYERS
    GUARD = 64
    rows, keep = [], []
    for li, (C, ntr, nsc, nbt0, ctr, csc) in enumerate(layers):
        rm0, rv0, st_tr, st_sc = ko.bn_running_case(li, DEV)
        buf = torch.full((2, C + GUARD), -77.0, device=DEV)      # guard past each layer's C
        buf[0, :C], buf[1, :C] = rm0, rv0
        nbt = None if nbt0 is None else torch.tensor([nbt0], dtype=torch.int64, device=DEV)
        rows.append((buf[0], buf[1], st_tr, st_sc, nbt, C, ntr, nsc, ctr, csc))
        keep.append((buf, rm0, rv0, st_tr, st_sc, nbt))
    ops.BnRunTable(rows, DEV).launch(0.1)
    torch.cuda.synchronize()
    for (C, ntr, nsc, nbt0, ctr, csc), (buf, rm0, rv0, st_tr, st_sc, nbt) in zip(layers, keep):
        rm, rv = ko.bn_running_ref(rm0, rv0, st_tr, ntr, ctr, st_sc, nsc, csc, 0.1)
        tol = 1e-5 * (rm.abs() + rv.abs() + 1)
        ko.assert_tol(buf[0, :C], rm, tol, 'running mean C=%d' % C)
        ko.assert_tol(buf[1, :C], rv, tol, 'running var C=%d' % C)
        assert (buf[:, C:] == -77.0).all(), 'wrote past C=%d' % C
        if nbt is not None:
            assert int(nbt.item()) == nbt0 + ntr + nsc
