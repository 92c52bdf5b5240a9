"""The positional lists the conv front-end hands to the extension, checked on the CPU.

``ConvSpec``'s geometry helpers are compared with literals worked out by hand from the field
comments of ``ConvGeom`` / ``WgradGeom`` (csrc/igemm.h); every argument builder of
``ops/conv.py`` and ``ops/hconv.py`` is compared, position by position, with the parameter
names of its binding's lambda in csrc/bindings.cpp (the name lists below are those parameter
lists, in order).  No extension is loaded: ``data_ptr()`` of CPU tensors stands in for device
addresses, and where a wrapper is driven, ``lib`` is a recording stub.
"""
import pytest
import torch

from mercury_amd.ops import conv as cv
from mercury_amd.ops import hconv as hc
from mercury_amd.ops.conv import ConvSpec

ST = 'STREAM'

CONV_GEOM = 'SH SW SC RP RQ R Sk stride pad Kc Ncols M'
BW = 'bw_out bw_y bw_stats bw_y2 bw_stats2 bw_sums bw_inv_count bw_eps bw_act'
IGEMM = ('src wt out ldo bias stats stats_ld group_rows accumulate slab ' + CONV_GEOM +
         ' bm bn splits trans st ' + BW).split()
IGEMM_PRO = ('src wt out ldo bias stats stats_ld group_rows slab ' + CONV_GEOM + ' bm bn splits '
             'st p_stats p_rmean p_rvar p_gamma p_beta p_keep p_group_rows p_inv_count p_eps '
             'p_act p_keep_tap p_res').split()
DUAL = ('src wt out ldo stats stats_ld group_rows slab ' + CONV_GEOM + ' splits').split()
S2_HEAD = 'dy wt dx ldo accumulate SH SW SC R Sk stride pad Ncols bm bn H W N'
DGRAD_S2 = (S2_HEAD + ' st ' + BW).split()
WGRAD = 'dy x dw N H W C Pp Q K R Sk stride pad Creal bm bn splits slab st'.split()
PAIR = ('dy wt dx ldo accumulate slab ' + CONV_GEOM + ' bm bn splits ' + BW +
        ' x dw N H W C Pp Q K Creal wbm wbn wsplits wslab st').split()
PAIR_S2 = (S2_HEAD + ' ' + BW + ' x dw C Pp Q K Creal wbm wbn wsplits wslab st').split()
PGEMM = ('a b out stats M N K ldo stats_ld group_rows a_bytes b_bytes out_bytes H W Pp Q stride '
         'bn grid st p_mode p_stats p_rmean p_rvar p_gamma p_beta p_inv_count p_eps p_act '
         'p_group_rows p_G p_coef p_res p_keep p_res_bytes p_keep_bytes p_coef_bytes').split()
HCONV = ('src wt out bias stats group_rows slab geo bm bn splits st mode p_stats p_rmean p_rvar '
         'p_gamma p_beta p_group_imgs p_inv_count p_eps p_act').split()


def test_binding_arities():
    """the parameter counts of the lambdas in csrc/bindings.cpp"""
    assert [len(n) for n in (IGEMM, IGEMM_PRO, DUAL, DGRAD_S2, WGRAD, PAIR, PAIR_S2, PGEMM,
                             HCONV)] == [36, 37, 21, 28, 20, 45, 39, 38, 22]


# ---------------------------------------------------------------- geometry literals
# (spec, fwd_geom, dgrad_geom, s2_geom, wgrad_geom), by hand: P = (H + 2 pad - R) // stride + 1,
# Q likewise from W and S; Kc = R * S * (source channels) / 8; M = N P Q; the dgrad reads dy
# (P x Q x K) and writes N H W rows of Cp columns
GEOMS = [
    (ConvSpec(2, 8, 8, 16, 32, 3, 3, 1, 1),
     (8, 8, 16, 8, 8, 3, 3, 1, 1, 18, 32, 128), (8, 8, 32, 8, 8, 3, 3, 1, 1, 36, 16, 128),
     ((8, 8, 32, 3, 3, 1, 1, 16), (8, 8, 2)), (2, 8, 8, 16, 8, 8, 32, 3, 3, 1, 1, 16)),
    # 3x3 stride 2: P = Q = 4, M = 32
    (ConvSpec(2, 8, 8, 16, 64, 3, 3, 2, 1),
     (8, 8, 16, 4, 4, 3, 3, 2, 1, 18, 64, 32), (4, 4, 64, 8, 8, 3, 3, 2, 1, 72, 16, 128),
     ((4, 4, 64, 3, 3, 2, 1, 16), (8, 8, 2)), (2, 8, 8, 16, 4, 4, 64, 3, 3, 2, 1, 16)),
    # 1x1 stride 2 pad 0: P = Q = 8
    (ConvSpec(4, 16, 16, 64, 128, 1, 1, 2, 0),
     (16, 16, 64, 8, 8, 1, 1, 2, 0, 8, 128, 256), (8, 8, 128, 16, 16, 1, 1, 2, 0, 16, 64, 1024),
     ((8, 8, 128, 1, 1, 2, 0, 64), (16, 16, 4)), (4, 16, 16, 64, 8, 8, 128, 1, 1, 2, 0, 64)),
    # stem: C = 3 padded to 8 in memory; the wgrad keeps the real 3
    (ConvSpec(2, 32, 32, 3, 64, 3, 3, 1, 1),
     (32, 32, 8, 32, 32, 3, 3, 1, 1, 9, 64, 2048), (32, 32, 64, 32, 32, 3, 3, 1, 1, 72, 8, 2048),
     ((32, 32, 64, 3, 3, 1, 1, 8), (32, 32, 2)), (2, 32, 32, 8, 32, 32, 64, 3, 3, 1, 1, 3)),
    # H != W, stride 2: P = (12 + 2 - 3) // 2 + 1 = 6, Q = (20 + 2 - 3) // 2 + 1 = 10
    (ConvSpec(3, 12, 20, 24, 40, 3, 3, 2, 1),
     (12, 20, 24, 6, 10, 3, 3, 2, 1, 27, 40, 180), (6, 10, 40, 12, 20, 3, 3, 2, 1, 45, 24, 720),
     ((6, 10, 40, 3, 3, 2, 1, 24), (12, 20, 3)), (3, 12, 20, 24, 6, 10, 40, 3, 3, 2, 1, 24)),
    # R != S (1 x 3), no padding: P = 9, Q = 7 - 3 + 1 = 5
    (ConvSpec(1, 9, 7, 8, 16, 1, 3, 1, 0),
     (9, 7, 8, 9, 5, 1, 3, 1, 0, 3, 16, 45), (9, 5, 16, 9, 7, 1, 3, 1, 0, 6, 8, 63),
     ((9, 5, 16, 1, 3, 1, 0, 8), (9, 7, 1)), (1, 9, 7, 8, 9, 5, 16, 1, 3, 1, 0, 8)),
]


@pytest.mark.parametrize('spec,fwd,dgrad,s2,wgrad', GEOMS)
def test_geometry_literals(spec, fwd, dgrad, s2, wgrad):
    assert spec.fwd_geom() == fwd
    assert spec.dgrad_geom() == dgrad
    assert spec.s2_geom() == s2
    assert spec.wgrad_geom() == wgrad
    assert spec.Mx == spec.N * spec.H * spec.W == dgrad[-1]


def test_stem_and_stride2_fields():
    s = ConvSpec(2, 32, 32, 3, 64, 3, 3, 1, 1)
    assert s.Cp == 8 and s.wgrad_geom()[-1] == 3
    s = ConvSpec(2, 8, 8, 16, 64, 3, 3, 2, 1)
    assert (s.P, s.Q, s.M) == (4, 4, 32)


def test_group():
    s = ConvSpec(4, 8, 8, 16, 32, 3, 3, 1, 1)
    assert s.M == 256 and s.group == 256               # 0: the whole batch
    s.group_rows = 64
    assert s.group == 64
    s.group_rows = 256
    assert s.group == 256


# ---------------------------------------------------------------- builder positions
SPEC = ConvSpec(3, 12, 20, 24, 40, 3, 3, 2, 1, group_rows=60)    # the H != W case above
FWD_GEOM = dict(SH=12, SW=20, SC=24, RP=6, RQ=10, R=3, Sk=3, stride=2, pad=1, Kc=27, Ncols=40,
                M=180)
DGRAD_GEOM = dict(SH=6, SW=10, SC=40, RP=12, RQ=20, R=3, Sk=3, stride=2, pad=1, Kc=45, Ncols=24,
                  M=720)
NO_BW = dict(bw_out=0, bw_y=0, bw_stats=0, bw_y2=0, bw_stats2=0, bw_sums=0, bw_inv_count=0.0,
             bw_eps=0.0, bw_act=0)


class Tensors(object):
    """CPU tensors of distinct sizes, all alive at once: every data_ptr() is distinct."""

    def __init__(self):
        self._n = 8
        self._all = []

    def __call__(self, dtype=torch.bfloat16):
        self._n += 8
        t = torch.empty(self._n, dtype=dtype)
        self._all.append(t)
        assert len({u.data_ptr() for u in self._all}) == len(self._all)
        return t


def named(names, values):
    values = list(values)
    assert len(values) == len(names)
    return dict(zip(names, values))


def p(t):
    return t.data_ptr()


def test_igemm_forward_positions():
    T = Tensors()
    x, w, out = T(), T(), T()
    slab, bias, stats = T(torch.float32), T(torch.float32), T(torch.float32)
    a = cv._igemm_args(x, w, out, SPEC, (5, 7, 11), slab, bias, stats, accumulate=True)
    assert named(IGEMM, a + (ST,) + cv._NO_BW) == dict(
        src=p(x), wt=p(w), out=p(out), ldo=40, bias=p(bias), stats=p(stats), stats_ld=40,
        group_rows=60, accumulate=1, slab=p(slab), bm=5, bn=7, splits=11, trans=False, st=ST,
        **FWD_GEOM, **NO_BW)
    a = cv._igemm_args(x, w, out, SPEC, (5, 7, 1), slab)
    got = named(IGEMM, a + (ST,) + cv._NO_BW)
    assert (got['slab'], got['bias'], got['stats'], got['accumulate']) == (0, 0, 0, 0)


def test_igemm_dgrad_positions():
    T = Tensors()
    dy, wt, dx, slab = T(), T(), T(), T(torch.float32)
    bw = tuple(range(101, 110))
    a = cv._igemm_args(dy, wt, dx, SPEC, (5, 7, 11), slab, accumulate=True, trans=True)
    assert named(IGEMM, a + (ST,) + bw) == dict(
        src=p(dy), wt=p(wt), out=p(dx), ldo=24, bias=0, stats=0, stats_ld=24, group_rows=720,
        accumulate=1, slab=p(slab), bm=5, bn=7, splits=11, trans=True, st=ST, **DGRAD_GEOM,
        **named(BW.split(), bw))


def test_igemm_pro_positions():
    T = Tensors()
    x, w, out = T(), T(), T()
    slab, bias, stats = T(torch.float32), T(torch.float32), T(torch.float32)
    pro = tuple(range(201, 213))
    a = cv._igemm_pro_args(x, w, out, SPEC, (5, 7, 11), slab, bias, stats)
    assert named(IGEMM_PRO, a + (ST,) + pro) == dict(
        src=p(x), wt=p(w), out=p(out), ldo=40, bias=p(bias), stats=p(stats), stats_ld=40,
        group_rows=60, slab=p(slab), bm=5, bn=7, splits=11, st=ST, **FWD_GEOM,
        **named(IGEMM_PRO[25:], pro))
    assert named(IGEMM_PRO, cv._igemm_pro_args(x, w, out, SPEC, (5, 7, 1), slab) + (ST,) + pro
                 )['slab'] == 0


def test_dual_positions():
    T = Tensors()
    x, w, out, stats, slab = T(), T(), T(), T(torch.float32), T(torch.float32)
    a = cv._dual_args(x, w, out, SPEC, stats, slab, (5, 7, 11))
    assert isinstance(a, list)                      # the binding takes std::vector<int64_t>
    assert named(DUAL, a) == dict(src=p(x), wt=p(w), out=p(out), ldo=40, stats=p(stats),
                                  stats_ld=40, group_rows=60, slab=p(slab), splits=11, **FWD_GEOM)
    assert named(DUAL, cv._dual_args(x, w, out, SPEC, None, slab, (5, 7, 1)))['slab'] == 0


S2_GEOM = dict(SH=6, SW=10, SC=40, R=3, Sk=3, stride=2, pad=1, Ncols=24, H=12, W=20, N=3)


def test_dgrad_s2_positions():
    T = Tensors()
    dy, wt, dx = T(), T(), T()
    bw = tuple(range(101, 110))
    a = cv._dgrad_s2_args(dy, wt, dx, SPEC, (5, 7), accumulate=True)
    assert named(DGRAD_S2, a + (ST,) + bw) == dict(
        dy=p(dy), wt=p(wt), dx=p(dx), ldo=24, accumulate=1, bm=5, bn=7, st=ST, **S2_GEOM,
        **named(BW.split(), bw))


def test_wgrad_positions():
    T = Tensors()
    dy, x, dw = T(), T(), T(torch.float32)
    a = cv._wgrad_args(dy, x, dw, SPEC, (13, 17, 19), 777)
    assert named(WGRAD, a + (ST,)) == dict(
        dy=p(dy), x=p(x), dw=p(dw), N=3, H=12, W=20, C=24, Pp=6, Q=10, K=40, R=3, Sk=3, stride=2,
        pad=1, Creal=24, bm=13, bn=17, splits=19, slab=777, st=ST)
    stem = ConvSpec(2, 32, 32, 3, 64, 3, 3, 1, 1)
    got = named(WGRAD, cv._wgrad_args(dy, x, dw, stem, (13, 17, 19)) + (ST,))
    assert (got['C'], got['Creal'], got['slab']) == (8, 3, 0)


def _pair_case():
    T = Tensors()
    return T(), T(), T(), T(), T(torch.float32), T(torch.float32)


def test_pair_positions():
    dy, wt, dx, x, dw, slab = _pair_case()
    bw = tuple(range(101, 110))
    # a channel-padded shape too, so that C and Creal differ
    for spec, geom, wg in (
            (SPEC, DGRAD_GEOM, dict(N=3, H=12, W=20, C=24, Pp=6, Q=10, K=40, Creal=24)),
            (ConvSpec(2, 9, 7, 3, 16, 3, 3, 1, 1),
             dict(SH=9, SW=7, SC=16, RP=9, RQ=7, R=3, Sk=3, stride=1, pad=1, Kc=18, Ncols=8,
                  M=126), dict(N=2, H=9, W=7, C=8, Pp=9, Q=7, K=16, Creal=3))):
        a = cv._pair_args(dy, wt, dx, x, dw, spec, (5, 7, 11), (13, 17, 19), slab, True, bw, 777)
        assert len(a) == 44                             # conv_bwd_pair_sc's first tuple
        assert named(PAIR, a + (ST,)) == dict(
            dy=p(dy), wt=p(wt), dx=p(dx), ldo=spec.Cp, accumulate=1, slab=p(slab), bm=5, bn=7,
            splits=11, x=p(x), dw=p(dw), wbm=13, wbn=17, wsplits=19, wslab=777, st=ST, **geom,
            **wg, **named(BW.split(), bw))
    got = named(PAIR, cv._pair_args(dy, wt, dx, x, dw, SPEC, (5, 7, 1), (13, 17, 19), slab)
                + (ST,))
    assert (got['slab'], got['accumulate'], got['wslab']) == (0, 0, 0)
    assert {k: got[k] for k in NO_BW} == NO_BW


def test_pair_s2_positions():
    dy, wt, dx, x, dw, _ = _pair_case()
    bw = tuple(range(101, 110))
    a = cv._pair_s2_args(dy, wt, dx, x, dw, SPEC, (13, 17, 19), True, bw, 777)
    assert len(a) == 38                                 # conv_bwd_pair_sc's second tuple
    assert named(PAIR_S2, a + (ST,)) == dict(
        dy=p(dy), wt=p(wt), dx=p(dx), ldo=24, accumulate=1, bm=64, bn=64, x=p(x), dw=p(dw), C=24,
        Pp=6, Q=10, K=40, Creal=24, wbm=13, wbn=17, wsplits=19, wslab=777, st=ST, **S2_GEOM,
        **named(BW.split(), bw))
    stem = ConvSpec(2, 32, 32, 3, 64, 3, 3, 2, 1)
    got = named(PAIR_S2, cv._pair_s2_args(dy, wt, dx, x, dw, stem, (64, 64, 1)) + (ST,))
    assert (got['C'], got['Creal'], got['Pp'], got['Q'], got['K']) == (8, 3, 16, 16, 64)
    assert {k: got[k] for k in NO_BW} == NO_BW and got['wslab'] == 0


def test_pgemm_positions():
    T = Tensors()
    x, w, out, stats = T(), T(), T(), T(torch.float32)
    spec = ConvSpec(5, 6, 10, 24, 40, 1, 1, 2, 0, group_rows=30)    # P = 3, Q = 5, M = 75
    pro = tuple(range(301, 318))
    a = cv._pgemm_args(x, w, out, stats, spec, 2, 128, 96)
    assert named(PGEMM, a + (ST,) + pro) == dict(
        a=p(x), b=p(w), out=p(out), stats=p(stats), M=75, N=40, K=24, ldo=40, stats_ld=40,
        group_rows=30, a_bytes=x.numel() * 2, b_bytes=w.numel() * 2, out_bytes=out.numel() * 2,
        H=6, W=10, Pp=3, Q=5, stride=2, bn=128, grid=96, st=ST, **named(PGEMM[21:], pro))
    assert len(cv._PG_NO_PRO) == len(PGEMM[21:])
    # the panel-resident kernel's call: stride 1, bn = 0, grid 0
    got = named(PGEMM, cv._pgemm_args(x, w, out, None, spec, 1, 0, 0) + (ST,) + pro)
    assert (got['stats'], got['stride'], got['bn'], got['grid']) == (0, 1, 0, 0)


def test_hconv_positions():
    T = Tensors()
    x, w, out, bias, stats, slab = T(), T(), T(), T(torch.float32), T(torch.float32), \
        T(torch.float32)
    spec = ConvSpec(4, 8, 8, 64, 64, 3, 3, 1, 1, group_rows=128)
    g = hc.geometry(spec, 64, 64)
    assert g is not None
    geo = [g[k] for k in hc._ORDER]
    assert len(geo) == 21 and geo[:10] == [4, 8, 8, 64, 8, 8, 64, 3, 1, 1]   # N H W C P Q K R s p
    pro = hc._pro_args(None, spec)
    a = hc._hconv_args(x, w, out, bias, stats, spec, slab, g, (64, 64, 2))
    assert named(HCONV, a + (ST,) + pro) == dict(
        src=p(x), wt=p(w), out=p(out), bias=p(bias), stats=p(stats), group_rows=128,
        slab=p(slab), geo=geo, bm=64, bn=64, splits=2, st=ST, **named(HCONV[12:], pro))
    for splits in (1, 0, -1):                       # unsplit, persistent, row-step: no slab
        assert named(HCONV, hc._hconv_args(x, w, out, None, None, spec, slab, g, (64, 64, splits))
                     + (ST,) + pro)['slab'] == 0


# ---------------------------------------------------------------- wrappers on a recording stub
class Recorder(object):
    SUMS_R = 1

    def __init__(self, ret=1):
        self.calls, self.ret = [], ret

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return self.ret
        return f


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    for mod in (cv, hc):
        monkeypatch.setattr(mod, 'lib', lambda: r)
        monkeypatch.setattr(mod, 'stream_ptr', lambda: ST)
        monkeypatch.setattr(mod, '_chk', lambda *a, **k: None)
    monkeypatch.setattr(cv, 'DGRAD_S2', True)
    return r


def test_wrappers_hand_over_the_builders_lists(rec):
    T = Tensors()
    x, w, out, slab, stats = T(), T(), T(), torch.empty(1 << 18), T(torch.float32)
    spec = ConvSpec(3, 12, 20, 24, 40, 3, 3, 1, 1)
    cv.conv_fwd(x, w, out, spec, stats=stats, slab=slab, plan=(64, 64, 3))
    dy, wt, dx, dw = T(), T(), T(), T(torch.float32)
    cv.conv_dgrad(dy, wt, dx, spec, slab=slab, plan=(64, 64, 3), accumulate=True)
    cv.conv_wgrad(dy, x, dw, spec, plan=(64, 64, 2))
    cv.conv_bwd(dy, wt, dx, x, dw, spec, dplan=(64, 64, 3), wplan=(64, 64, 2), slab=slab)
    s2 = ConvSpec(3, 12, 20, 24, 64, 3, 3, 2, 1)
    cv.conv_bwd(dy, wt, dx, x, dw, s2, wplan=(64, 64, 2))
    cv.conv_dgrad(dy, wt, dx, s2, plan=(128, 64, 1))
    assert rec.calls == [
        ('igemm', cv._igemm_args(x, w, out, spec, (64, 64, 3), slab, None, stats) + (ST,)
         + cv._NO_BW),
        ('igemm', cv._igemm_args(dy, wt, dx, spec, (64, 64, 3), slab, accumulate=True, trans=True)
         + (ST,) + cv._NO_BW),
        ('wgrad', cv._wgrad_args(dy, x, dw, spec, (64, 64, 2)) + (ST,)),
        ('conv_bwd_pair', cv._pair_args(dy, wt, dx, x, dw, spec, (64, 64, 3), (64, 64, 2), slab)
         + (ST,)),
        ('conv_bwd_pair_s2', cv._pair_s2_args(dy, wt, dx, x, dw, s2, (64, 64, 2)) + (ST,)),
        ('dgrad_s2', cv._dgrad_s2_args(dy, wt, dx, s2, (128, 64)) + (ST,) + cv._NO_BW),
    ]


def _sc_dicts():
    T = Tensors()
    sa = ConvSpec(4, 8, 8, 64, 64, 3, 3, 1, 1)
    sb = ConvSpec(4, 16, 16, 32, 64, 1, 1, 2, 0)
    a = dict(dy=T(), wt=T(), dx=T(), x=T(), dw=T(torch.float32), spec=sa, dplan=(64, 64, 3),
             wplan=(64, 64, 5), slab=torch.empty(1 << 18), accumulate=True)
    b = dict(dy=T(), wt=T(), dx=T(), x=T(), dw=T(torch.float32), spec=sb, wplan=(64, 64, 7),
             accumulate=True)
    return a, b


def test_conv_bwd_sc_hands_over_the_pair_tuples(rec):
    a, b = _sc_dicts()
    sa, sb = a['spec'], b['spec']
    bf = torch.bfloat16
    a['bw'] = dict(out=torch.empty(11, dtype=bf), y=torch.empty(13, dtype=bf),
                   stats=torch.empty(17), sums=torch.empty(19), act='relu', eps=1e-3)
    assert cv.conv_bwd_sc(a, b) is True
    (name, (ta, tb, st)), = rec.calls
    assert name == 'conv_bwd_pair_sc' and st == ST
    assert ta == cv._pair_args(a['dy'], a['wt'], a['dx'], a['x'], a['dw'], sa, (64, 64, 3),
                               (64, 64, 5), a['slab'], True, cv._bw_args(a['bw'], sa.Mx, sa.Cp))
    assert tb == cv._pair_s2_args(b['dy'], b['wt'], b['dx'], b['x'], b['dw'], sb, (64, 64, 7),
                                  True)
    assert isinstance(ta, tuple) and isinstance(tb, tuple) and (len(ta), len(tb)) == (44, 38)
    got = named(PAIR, ta + (ST,))
    assert (got['bw_out'], got['bw_act'], got['bw_inv_count'], got['wslab']) == (
        a['bw']['out'].data_ptr(), 1, 1.0 / 256, 0)
    rec.ret = 0
    assert cv.conv_bwd_sc(a, b) is False


def test_conv_bwd_sc_declines_without_a_call(rec):
    a, b = _sc_dicts()
    a['spec'] = ConvSpec(4, 16, 16, 64, 64, 3, 3, 2, 1)           # last conv not stride 1
    assert cv.conv_bwd_sc(a, b) is False
    a, b = _sc_dicts()
    b['wplan'] = (128, 128, 1)                                     # shortcut tiles not 64 x 64
    assert cv.conv_bwd_sc(a, b) is False
    b['wplan'] = (64, 128, 1)
    assert cv.conv_bwd_sc(a, b) is False
    a, b = _sc_dicts()
    b['spec'] = ConvSpec(33, 16, 16, 32, 64, 1, 1, 2, 0)           # shortcut batch > 32
    assert cv.conv_bwd_sc(a, b) is False
    assert rec.calls == []
