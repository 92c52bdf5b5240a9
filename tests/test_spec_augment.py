"""SpecRecipe on the CPU: the spec string, the range checks, the reference's arithmetic against
hand-written expectations, the ``SpecAugment`` transform's draws and ``Config.augment``."""
import pytest
import torch

from mercury_amd.data.augment import SPEC_PARAMS, SpecRecipe
from mercury_amd.data.transforms import SpecAugment

SPEC = 'spec:shift=8,fmask=2x10,tmask=2x20,gain=0.8:1.2,fill=0'
FULL = SpecRecipe(shift=8, fmask=(2, 10), tmask=(2, 20), gain=(0.8, 1.2), fill=0.0)


def test_parse_round_trips():
    r = SpecRecipe.parse(SPEC)
    assert r == FULL
    assert SpecRecipe.parse(r.spec()) == r and r.spec().startswith('spec:')
    assert SpecRecipe.parse(SPEC[5:]) == r                      # the prefix is optional here
    for q in (SpecRecipe(), SpecRecipe(shift=3), SpecRecipe(fmask=(1, 4), fill=-1.5),
              SpecRecipe(tmask=(2, 6), gain=(0.5, 2.0))):
        assert SpecRecipe.parse(q.spec()) == q
    assert SpecRecipe.parse('spec:') == SpecRecipe()
    assert SpecRecipe.parse('gain=none,shift=2') == SpecRecipe(shift=2)
    with pytest.raises(ValueError, match='colour'):
        SpecRecipe.parse('spec:colour=1')
    with pytest.raises(ValueError, match='name=value'):
        SpecRecipe.parse('spec:shift')
    with pytest.raises(ValueError, match='fmask'):
        SpecRecipe.parse('spec:fmask=3')
    with pytest.raises(ValueError, match='gain'):
        SpecRecipe.parse('spec:gain=1')


def test_identity():
    assert SpecRecipe().identity
    assert SpecRecipe(fmask=(0, 5), tmask=(2, 0), fill=3.0).identity     # no mask can be drawn
    for r in (SpecRecipe(shift=1), SpecRecipe(fmask=(1, 1)), SpecRecipe(tmask=(1, 1)),
              SpecRecipe(gain=(1.0, 1.0))):
        assert not r.identity


def test_range_checks():
    for kw, field in ((dict(shift=-1), 'shift'), (dict(fmask=(3, 1)), 'fmask'),
                      (dict(fmask=(-1, 1)), 'fmask'), (dict(fmask=(1, -1)), 'fmask'),
                      (dict(tmask=(3, 1)), 'tmask'), (dict(tmask=(1, -2)), 'tmask'),
                      (dict(tmask=(1,)), 'tmask'),
                      (dict(gain=(2.0, 1.0)), 'gain'), (dict(gain=(0.0, float('inf'))), 'gain'),
                      (dict(gain=(float('nan'), 1.0)), 'gain'), (dict(gain=(1.0,)), 'gain'),
                      (dict(fill=float('nan')), 'fill'), (dict(fill=float('inf')), 'fill')):
        with pytest.raises(ValueError, match=field):
            SpecRecipe(**kw)
    r = SpecRecipe(shift=4, fmask=(2, 3), tmask=(1, 5))
    r.check(1, 3, 5)                                   # shift = W-1, Fmax = H, Tmax = W: all fit
    r.check(8, 101, 161)
    for (C, H, W), field in (((0, 3, 5), 'C'), ((9, 3, 5), 'C'), ((1, 3, 4), 'shift'),
                             ((1, 2, 5), 'fmask'), ((1, 0, 5), 'empty')):
        with pytest.raises(ValueError, match=field):
            r.check(C, H, W)
    with pytest.raises(ValueError, match='tmask'):
        SpecRecipe(tmask=(1, 6)).check(1, 3, 5)


X = (torch.arange(15, dtype=torch.float32) + 1).view(1, 3, 5)       # rows 1..5, 6..10, 11..15


def _ref(r, shift=0, gain=1.0, fa=(0, 0), fb=(0, 0), ta=(0, 0), tb=(0, 0), x=X):
    p = [shift, gain, fa[0], fa[1], fb[0], fb[1], ta[0], ta[1], tb[0], tb[1], 0, 0]
    y = r.reference(x, p)
    assert y.shape == (x.shape[1], x.shape[2], 8) and y.dtype == torch.bfloat16
    assert torch.equal(y[..., x.shape[0]:].view(torch.int16),
                       torch.zeros_like(y[..., x.shape[0]:]).view(torch.int16))    # +0 exactly
    return y[..., 0].float().tolist()


def test_reference_shift():
    r = SpecRecipe(shift=4, fill=-2.0)
    F = -2.0
    assert _ref(r) == [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]]
    assert _ref(r, shift=1) == [[F, 1, 2, 3, 4], [F, 6, 7, 8, 9], [F, 11, 12, 13, 14]]
    assert _ref(r, shift=-1) == [[2, 3, 4, 5, F], [7, 8, 9, 10, F], [12, 13, 14, 15, F]]
    assert _ref(r, shift=4) == [[F, F, F, F, 1], [F, F, F, F, 6], [F, F, F, F, 11]]
    assert _ref(r, shift=-4) == [[5, F, F, F, F], [10, F, F, F, F], [15, F, F, F, F]]


def test_reference_masks():
    r = SpecRecipe(shift=1, fmask=(2, 3), tmask=(2, 5), fill=0.5)
    F = 0.5
    full = [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]]
    # width 0: nothing masked, wherever it starts
    assert _ref(r, fa=(2, 0), ta=(5, 0)) == full
    # a mask touching each edge
    assert _ref(r, fa=(0, 1)) == [[F] * 5, full[1], full[2]]
    assert _ref(r, fa=(2, 1)) == [full[0], full[1], [F] * 5]
    assert _ref(r, ta=(0, 2)) == [[F, F] + row[2:] for row in full]
    assert _ref(r, ta=(3, 2)) == [row[:3] + [F, F] for row in full]
    # two overlapping masks: the union
    assert _ref(r, fa=(0, 2), fb=(1, 2)) == [[F] * 5] * 3
    assert _ref(r, ta=(1, 2), tb=(2, 2)) == [[row[0], F, F, F, row[4]] for row in full]
    # masks are in OUTPUT coordinates: the band stays at t = 3..4 under a shift
    assert _ref(r, shift=1, ta=(3, 2)) == [[F, 1, 2, F, F], [F, 6, 7, F, F], [F, 11, 12, F, F]]
    # a frequency and a time band together
    assert _ref(r, fb=(1, 1), tb=(0, 1)) == [[F, 2, 3, 4, 5], [F] * 5, [F, 12, 13, 14, 15]]


def test_reference_gain_and_rounding():
    r = SpecRecipe(gain=(0.5, 2.0), fill=0.1)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 5, generator=g)
    xb = x.bfloat16()
    one = r.reference(x, [0, 1.0] + [0] * 10)
    # a gain of exactly 1: the shard's own rounding and nothing else, bit for bit
    assert torch.equal(one[..., :2].view(torch.int16), xb.permute(1, 2, 0).contiguous().view(torch.int16))
    # one fp32 multiply of the bf16 value, rounded to nearest even
    gain = 1.2999999523162842
    got = r.reference(x, [0, gain] + [0] * 10)
    want = (xb.float() * torch.tensor(gain, dtype=torch.float32)).bfloat16()
    assert torch.equal(got[..., :2].view(torch.int16), want.permute(1, 2, 0).contiguous().view(torch.int16))
    # fill is rounded to bf16 once and is not multiplied by the gain
    y = r.reference(x, [0, 2.0, 0, 3] + [0] * 8)
    assert bool((y[..., :2] == torch.tensor(0.1).bfloat16()).all()) and bool((y[..., 2:] == 0).all())
    with pytest.raises(ValueError, match='params'):
        r.reference(x, [0, 1.0])
    with pytest.raises(ValueError, match=r'\[C\]\[H\]\[W\]'):
        r.reference(x[0], [0, 1.0] + [0] * 10)


def test_spec_augment_draws():
    r = SpecRecipe(shift=3, fmask=(2, 2), tmask=(1, 6), gain=(0.5, 2.0), fill=-1.5)
    H, W = 4, 9
    x = torch.randn(2, H, W, generator=torch.Generator().manual_seed(1))

    def run(seed, n):
        t = SpecAugment(r, generator=torch.Generator().manual_seed(seed))
        out = []
        for _ in range(n):
            y = t(x)
            assert y.shape == x.shape and y.dtype == x.dtype
            out.append((list(t.last), y))
        return out

    runs = run(5, 2000)
    seen_shift, seen_fw, seen_tw = set(), set(), set()
    for p, y in runs:
        assert len(p) == SPEC_PARAMS and p[10] == p[11] == 0
        assert p[0] == int(p[0]) and -3 <= p[0] <= 3
        assert 0.5 <= p[1] < 2.0
        for k, size, mx in ((2, H, 2), (4, H, 2), (6, W, 6)):
            assert p[k] == int(p[k]) and p[k + 1] == int(p[k + 1])
            assert 0 <= p[k + 1] <= mx and 0 <= p[k] and p[k] + p[k + 1] <= size
        assert p[8] == p[9] == 0                     # one time mask only
        seen_shift.add(p[0]), seen_fw.update((p[3], p[5])), seen_tw.add(p[7])
    assert seen_shift == set(range(-3, 4)) and seen_fw == {0, 1, 2} and seen_tw == set(range(7))
    # the transform is the reference on its own draws, in the input's dtype and layout
    p, y = runs[7]
    assert torch.equal(y, r.reference(x, p, dtype=torch.float32)[..., :2].permute(2, 0, 1))
    # deterministic under a seeded generator
    again = run(5, 20)
    for (p0, y0), (p1, y1) in zip(runs, again):
        assert p0 == p1 and torch.equal(y0, y1)
    assert [p for p, _ in run(6, 20)] != [p for p, _ in again]
    # an identity recipe passes the input through
    assert torch.equal(SpecAugment('spec:')(x), x)
    with pytest.raises(ValueError, match='SpecRecipe'):
        SpecAugment(3)


class _Set(object):
    def __init__(self, transform):
        self.transform = transform


class _Loader(object):
    def __init__(self, transform):
        self.dataset = _Set(transform)


def test_config_recipes():
    from mercury_amd.config import Config
    from mercury_amd.engine.native import _config_recipes
    aug, ev = _config_recipes(Config(augment=SPEC), None, None)
    assert aug == FULL and ev is None
    r = SpecRecipe(shift=4, tmask=(1, 8))
    aug, ev = _config_recipes(Config(augment='dataset'), _Loader(SpecAugment(r)), _Loader(None))
    assert aug == r and ev is None
    assert _config_recipes(Config(), _Loader(SpecAugment(r)), _Loader(None)) == (None, None)
    with pytest.raises(ValueError, match='unknown key'):
        _config_recipes(Config(augment='spec:crop=32'), None, None)
