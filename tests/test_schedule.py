"""The engine's per-mode launch schedules (engine/schedule.py), resolved on the CPU.

The expected counts below were read off recordings of what commit 46f3bdb (the engine before
it had a schedule) launched on an MI355X: every ``ops`` entry point wrapped, one eager pass per
mode of each ``bench.py`` preset at its own batch size (scoring: 10 x batch in ghost groups of
one batch; train: batch; eval: 2 x batch).  They pin where each BatchNorm is applied and which
kernel runs each conv; a change that moves one has to change this table.
"""
import collections

import pytest

from mercury_amd.config import EngineOptions
from mercury_amd.engine import schedule as S
from mercury_amd.engine.lower import lower
from mercury_amd.models import build_model
from mercury_amd.ops import tune

PRESETS = {     # bench.py --config: (model, classes, (H, W), batch)
    'resnet18-cifar10': ('resnet18', 10, (32, 32), 32),
    'mobilenetv2-cifar100': ('mobilenetv2', 100, (32, 32), 32),
    'resnet50-imagenet': ('resnet50_imagenet', 1000, (224, 224), 128),
    'vgg11-speech': ('vgg11', 30, (101, 161), 32),
}
OFF = dict(persist_bn='0', head_bn=False, dual_fwd=False, dual_bwd=False)

# recorded on 46f3bdb.  Forward: bn_apply passes, convs per kernel (one launch each; a dual
# pair is one launch, counted under 'dual'), convs that apply a BN in their input prologue,
# who applies the last block's BN.
FWD = {
    ('resnet18-cifar10', 'score'): dict(bn_apply=12, dual=3, pro=4, last='head',
                                        conv=dict(stem=1, hconv=13)),
    ('resnet18-cifar10', 'train'): dict(bn_apply=17, dual=3, pro=0, last='pass',
                                        conv=dict(stem=1, hconv=10, igemm=3)),
    ('resnet18-cifar10', 'eval'): dict(bn_apply=16, dual=3, pro=0, last='head',
                                       conv=dict(stem=1, hconv=9, igemm=4)),
    ('resnet18-cifar10/off', 'score'): dict(bn_apply=17, dual=0, pro=0, last='pass',
                                            conv=dict(stem=1, hconv=13, igemm=6)),
    ('resnet18-cifar10/off', 'train'): dict(bn_apply=17, dual=0, pro=0, last='pass',
                                            conv=dict(stem=1, hconv=10, igemm=9)),
    ('resnet18-cifar10/off', 'eval'): dict(bn_apply=17, dual=0, pro=0, last='pass',
                                           conv=dict(stem=1, hconv=9, igemm=10)),
    ('mobilenetv2-cifar100', 'score'): dict(bn_apply=12, dual=0, pro=40, last='head',
                                            conv=dict(stem=1, igemm=29, dwconv=17, pgemm=4,
                                                      pwconv=6)),
    ('mobilenetv2-cifar100', 'train'): dict(bn_apply=10, dual=1, pro=43, last='pass',
                                            conv=dict(stem=1, igemm=37, dwconv=17)),
    ('mobilenetv2-cifar100', 'eval'): dict(bn_apply=10, dual=1, pro=42, last='head',
                                           conv=dict(stem=1, igemm=33, dwconv=17, pgemm=1,
                                                     pwconv=3)),
    ('resnet50-imagenet', 'score'): dict(bn_apply=33, dual=0, pro=14, last='head', pool_bn=1,
                                         conv=dict(stem=1, igemm=14, hconv=11, pgemm=19,
                                                   pwconv=8)),
    ('resnet50-imagenet', 'train'): dict(bn_apply=32, dual=0, pro=17, last='pass', pool_bn=0,
                                         conv=dict(stem=1, igemm=25, hconv=13, pgemm=6,
                                                   pwconv=8)),
    ('resnet50-imagenet', 'eval'): dict(bn_apply=35, dual=1, pro=12, last='head', pool_bn=1,
                                        conv=dict(stem=1, igemm=36, pgemm=6, pwconv=8)),
    ('vgg11-speech', 'score'): dict(bn_apply=3, dual=0, pro=0, last='pool', pool_bn=5,
                                    conv=dict(stem=1, igemm=7)),
    ('vgg11-speech', 'train'): dict(bn_apply=8, dual=0, pro=0, last='pass', pool_bn=0,
                                    conv=dict(stem=1, igemm=7)),
    ('vgg11-speech', 'eval'): dict(bn_apply=3, dual=0, pro=0, last='pool', pool_bn=5,
                                   conv=dict(stem=1, igemm=7)),
}
# Backward (train mode): bn_bwd passes with / without their own reduce and what head_bwd
# returned (True: it reduced the last BN's sums, so that bn_bwd ran without its reduce; None:
# no head_bwd, the speech MLP head); dgrad + wgrad pairs, of them with the shortcut's in the
# same launch (conv_bwd_sc returned True); depthwise pairs; convs with separate launches;
# dgrads that reduce BN sums.
BWD = {
    'resnet18-cifar10': dict(reduce=0, no_reduce=17, head=True, pair=13, pair_sc=3, dw_pair=0,
                             separate=1, bw=16),
    'resnet18-cifar10/off': dict(reduce=0, no_reduce=17, head=True, pair=19, pair_sc=0,
                                 dw_pair=0, separate=1, bw=16),
    'mobilenetv2-cifar100': dict(reduce=0, no_reduce=53, head=True, pair=39, pair_sc=0,
                                 dw_pair=17, separate=1, bw=52),
    'resnet50-imagenet': dict(reduce=2, no_reduce=47, head=False, pair=52, pair_sc=0, dw_pair=0,
                              separate=1, bw=47),
    'vgg11-speech': dict(reduce=5, no_reduce=3, head=None, pair=7, pair_sc=0, dw_pair=0,
                         separate=1, bw=3),
}

_LW = {}


def _lowered(preset):
    if preset not in _LW:
        model, ncls, _, _ = PRESETS[preset]
        _LW[preset] = lower(build_model(model, ncls))
    return _LW[preset]


def _units(lw):
    return {u.name: u for b in lw.blocks for u in b.units + ([b.shortcut] if b.shortcut else [])}


def _resolve(preset, mode, **opt):
    name, _, var = preset.partition('/')
    _, _, (H, W), B = PRESETS[name]
    opts = EngineOptions(**dict(OFF if var == 'off' else {}, **opt))
    N, group, train = dict(score=(10 * B, B, False), train=(B, 0, True),
                           eval=(2 * B, 0, False))[mode]
    lw = _lowered(name)
    mp = S.plan_mode(lw, opts, N, H, W, group, train)
    return lw, opts, mp, S.forward_schedule(lw, mp, opts)


@pytest.fixture(autouse=True)
def _tuner_off(monkeypatch):
    # the recordings ran with the plan tuner at its default (off: cached or heuristic plans)
    monkeypatch.setattr(tune, '_ENABLED', False)


@pytest.mark.parametrize('preset,mode', sorted(FWD))
def test_forward_schedule_matches_recorded_launches(preset, mode):
    lw, opts, mp, steps = _resolve(preset, mode)
    want = FWD[preset, mode]
    ops_ = collections.Counter(s.op for s in steps)
    assert ops_['bn_apply'] == want['bn_apply']
    assert ops_['dual_conv'] == want['dual']
    routes = collections.Counter(s.route for s in steps if s.op == 'conv')
    assert dict(routes) == want['conv']
    assert sum(s.op == 'conv' and s.pro is not None for s in steps) == want['pro']
    assert S.last_bn_by(steps) == want['last']
    assert ops_['head_bn'] == (want['last'] == 'head')
    assert sum(s.op == 'pool' and s.pro == 'pool' for s in steps) == want.get('pool_bn', 0)
    # every unit runs exactly once, every BN is applied exactly once
    by_name = _units(lw)
    units = list(by_name)
    ran = [n for s in steps if s.op in ('conv', 'dual_conv') for n in (s.unit, s.unit2) if n]
    assert sorted(ran) == sorted(units)
    applied = [s.src_unit for s in steps if s.pro is not None]
    shortcuts = [s.unit2 for s in steps if s.op == 'bn_apply' and s.res == 'sc']
    assert sorted(applied + shortcuts) == sorted(units)
    # route() agrees with the schedule for every unit
    for s in steps:
        if s.op == 'conv':
            assert S.route(mp.plan, mp.spec[s.unit], by_name[s.unit], opts, s.pro) == s.route
        elif s.op == 'dual_conv':
            for n in (s.unit, s.unit2):
                assert S.route(mp.plan, mp.spec[n], by_name[n], opts, None) == 'igemm'


@pytest.mark.parametrize('preset', sorted(BWD))
def test_backward_schedule_matches_recorded_launches(preset):
    lw, opts, mp, _ = _resolve(preset, 'train')
    want = BWD[preset]
    bwd = S.backward_schedule(lw, mp, opts)
    assert sorted(bwd.parts) == list(range(len(lw.blocks)))
    steps = [s for bi in bwd.parts for _, st in bwd.parts[bi] for s in st]
    red = collections.Counter(s.reduce for s in steps if s.op == 'bn_bwd')
    assert red['head'] == (want['head'] is not None) == bwd.head_bw
    assert red['pass'] + (red['head'] if want['head'] is False else 0) == want['reduce']
    assert red['dgrad'] + (red['head'] if want['head'] else 0) == want['no_reduce']
    kinds = collections.Counter(s.kind for s in steps if s.op == 'conv_bwd')
    assert kinds['pair'] == want['pair']
    assert kinds['pair_sc'] == want['pair_sc']
    assert kinds['dw_pair'] == want['dw_pair']
    assert kinds['separate'] == want['separate']
    assert sum(s.bw is not None for s in steps) == want['bw']
    # every BN's sums are reduced by exactly one party; a dgrad reduces only a real producer's
    assert red['dgrad'] == want['bw']
    for bi, parts in bwd.parts.items():
        assert [i for i, _ in parts] == list(range(len(lw.blocks[bi].units) - 1, -1, -1))


def _diff(a, b):
    return [(x, y) for x, y in zip(a, b) if x != y], len(a) - len(b)


def test_option_flips_change_only_their_steps():
    base = _resolve('resnet18-cifar10', 'score')[3]
    # head_bn off: the head's step becomes a bn_apply pass writing the block output
    st = _resolve('resnet18-cifar10', 'score', head_bn=False)[3]
    assert st[:-1] == base[:-1] and base[-1].op == 'head_bn'
    assert st[-1] == base[-1]._replace(op='bn_apply', pro='pass', keep='out')
    # persist_bn off: each halo-staged BN becomes a pass + a plain conv on the activation
    st = _resolve('resnet18-cifar10', 'score', persist_bn='0')[3]
    halo = [s for s in base if s.pro == 'halo']
    assert len(halo) == 4 and len(st) == len(base) + 4
    assert not any(s.pro == 'halo' for s in st)
    passes = [s for s in st if s not in base and s.op == 'bn_apply']
    assert [s.unit for s in passes] == [s.src_unit for s in halo]
    assert [s for s in st if s not in base and s.op == 'conv'] == [
        s._replace(src='act', pro=None, act=None, route=s.route) for s in halo]
    assert [s for s in st if s in base] == [s for s in base if s.pro != 'halo']
    # dual_fwd off: each pair becomes the first conv in place and the shortcut conv before the
    # block-final pass
    st = _resolve('resnet18-cifar10', 'score', dual_fwd=False)[3]
    duals = [s for s in base if s.op == 'dual_conv']
    assert len(duals) == 3 and len(st) == len(base) + 3
    assert [s for s in st if s in base] == [s for s in base if s.op != 'dual_conv']
    new = [s for s in st if s not in base]
    assert new[0::2] == [s._replace(op='conv', unit2=None) for s in duals]
    assert [(s.op, s.unit, s.route, s.src) for s in new[1::2]] == [
        ('conv', d.unit2, 'igemm', 'in') for d in duals]
    for d, sc in zip(duals, new[1::2]):
        assert st[st.index(sc) + 1] == next(s for s in base if s.op == 'bn_apply' and
                                            s.unit2 == d.unit2)
    # the train schedules do not depend on the scoring-only switches
    assert _resolve('resnet18-cifar10', 'train', head_bn=False, persist_bn='0')[3] == \
        _resolve('resnet18-cifar10', 'train')[3]


def test_planning_needs_no_device(monkeypatch):
    """plan_mode and the schedules never reach the extension."""
    from mercury_amd import ops

    def boom():
        raise AssertionError('planning called ops.lib()')
    monkeypatch.setattr(ops, 'lib', boom)
    monkeypatch.setattr(ops.hconv, 'lib', boom)
    monkeypatch.setattr(ops.conv, 'lib', boom)
    lw, opts, mp, steps = _resolve('mobilenetv2-cifar100', 'train')
    assert steps and S.backward_schedule(lw, mp, opts).parts


def test_plan_change_re_resolves_the_schedule():
    """The step tuner rewrites plans of a live mode (ops/step_tune._set): the mode re-resolves
    its schedules with them, so a dual pair whose tiles no longer match is scheduled as two
    convs at once, and one whose plans both split K has the shortcut's slab before any forward."""
    import torch
    from mercury_amd.engine.native import _Mode
    from mercury_amd.ops import step_tune
    from mercury_amd.ops.conv import slab_bytes
    lw, opts, mp, steps = _resolve('resnet18-cifar10', 'train')
    m = _Mode('train', mp, lw, opts)
    m.slab = torch.zeros(1)
    m.resolve()
    assert m.fwd_steps == steps and m.bwd == S.backward_schedule(lw, mp, opts)
    d = next(s for s in steps if s.op == 'dual_conv')
    sp, old = mp.spec[d.unit2], mp.plan[d.unit2, 'fwd']
    other = (128 if old[0] == 64 else 64, old[1], 1, 0)
    step_tune._set('fwd', [(m, d.unit2, sp)], other)
    assert [s.op for s in m.fwd_steps if s.unit == d.unit][0] == 'conv'
    assert len(m.fwd_steps) == len(steps) + 1
    step_tune._set('fwd', [(m, d.unit2, sp)], old)
    assert m.fwd_steps == steps
    for n in (d.unit, d.unit2):
        step_tune._set('fwd', [(m, n, mp.spec[n])], (old[0], old[1], 2, 0))
    assert d in m.fwd_steps
    assert m.buf[d.unit2, 'slab'].numel() * 4 >= slab_bytes(sp.M, sp.K, old[0], old[1], 2)
    # the backward pair-with-shortcut launch depends on the dgrad / wgrad tiles
    b = next(s for ps in m.bwd.parts.values() for _, st in ps for s in st if s.kind == 'pair_sc')
    dp, wp = mp.plan[b.unit, 'dgrad'], mp.plan[b.unit, 'wgrad']
    step_tune._set('bwd', [(m, b.unit, mp.spec[b.unit])], ((128, 64, 1), wp))
    assert not any(s.unit == b.unit and s.kind == 'pair_sc'
                   for ps in m.bwd.parts.values() for _, st in ps for s in st)
    step_tune._set('bwd', [(m, b.unit, mp.spec[b.unit])], (dp, wp))
    assert m.bwd == S.backward_schedule(lw, mp, opts)
