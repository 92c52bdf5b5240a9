"""AugmentRecipe on the CPU: reading a Compose, the spec string, the geometry, and the
recipe's unrounded arithmetic against the staged torch pipeline the CPU transforms run."""
import math

import pytest
import torch
import torch.nn.functional as F

from mercury_amd.data import transforms as T
from mercury_amd.data.augment import AugmentRecipe

SPEC = 'resize=35,crop=32,flip=1,degrees=10,scale=0.9:1.1,cutout=0,norm=none'
FULL = AugmentRecipe(resize=35, crop=(32, 32), pad=0, flip=True, degrees=10.0, scale=(0.9, 1.1))


def test_from_transform_reads_the_loaders_pipelines():
    r = AugmentRecipe.from_transform(T.affine_train_transform())
    assert r == FULL
    assert (r.resize, r.crop, r.pad, r.flip, r.degrees, r.scale, r.mean, r.std, r.cutout) == \
        (35, (32, 32), 0, True, 10.0, (0.9, 1.1), None, None, 0)
    t = AugmentRecipe.from_transform(T.affine_test_transform())
    assert t == AugmentRecipe(resize=33, crop=(32, 32))
    assert not t.flip and not t.affine and t.mean is None
    c = AugmentRecipe.from_transform(T.cifar_train_transform())
    assert c == AugmentRecipe.cifar()
    assert c.is_legacy(32, 32) and not c.is_legacy(40, 40) and not FULL.is_legacy(32, 32)
    assert AugmentRecipe.from_transform(None) == AugmentRecipe.cifar()
    e = AugmentRecipe.from_transform(T.cifar_test_transform())       # no RandomCrop
    assert e.crop is None and e.with_crop((32, 32)).is_legacy(32, 32)
    k = AugmentRecipe.from_transform(T.Compose([
        T.RandomCrop(24, padding=2), T.ToTensor(), T.Normalize(T.CIFAR_MEAN, T.CIFAR_STD),
        T.Cutout(8)]))
    assert (k.crop, k.pad, k.cutout, k.mean) == ((24, 24), 2, 8, tuple(T.CIFAR_MEAN))


def test_from_transform_refuses_what_it_cannot_run():
    with pytest.raises(ValueError, match='lambda'):
        AugmentRecipe.from_transform(T.Compose([T.RandomCrop(32), lambda x: x, T.ToTensor()]))
    with pytest.raises(ValueError, match='RandomHorizontalFlip'):
        AugmentRecipe.from_transform(T.Compose([T.RandomHorizontalFlip(0.3), T.ToTensor()]))
    with pytest.raises(ValueError, match='RandomCrop'):       # crop after flip: another order
        AugmentRecipe.from_transform(T.Compose([T.RandomHorizontalFlip(), T.RandomCrop(32),
                                                T.ToTensor()]))
    with pytest.raises(ValueError, match='ToNumpy'):
        AugmentRecipe.from_transform(T.Compose([T.ToNumpy(), T.ToTensor()]))
    with pytest.raises(ValueError, match='ToTensor'):
        AugmentRecipe.from_transform(T.Compose([T.RandomCrop(32)]))


def test_parse_round_trips():
    r = AugmentRecipe.parse(SPEC)
    assert r == FULL
    assert AugmentRecipe.parse(r.spec()) == r
    c = AugmentRecipe.parse('crop=32,pad=4,flip=1,norm=cifar')
    assert c == AugmentRecipe.cifar()
    assert AugmentRecipe.parse(c.spec()) == c
    n = AugmentRecipe.parse('resize=27,crop=24x20,pad=2,cutout=8,norm=0.5:0.4:0.3/0.2:0.25:0.5')
    assert (n.crop, n.mean, n.std) == ((24, 20), (0.5, 0.4, 0.3), (0.2, 0.25, 0.5))
    assert AugmentRecipe.parse(n.spec()) == n
    with pytest.raises(ValueError, match='colour'):
        AugmentRecipe.parse('crop=32,colour=1')


def test_geometry_and_check():
    r = AugmentRecipe(resize=27, crop=(24, 24), pad=2)
    assert r.resized_hw(24, 32) == (27, 36)
    assert r.resized_hw(32, 24) == (36, 27)
    assert AugmentRecipe(crop=(8, 8)).resized_hw(24, 32) == (24, 32)
    assert r.out_hw == (24, 24)
    r.check(24, 32)
    with pytest.raises(ValueError):
        AugmentRecipe(crop=(32, 32), pad=2).check(24, 40)       # Hr + 2*pad = 28 < 32
    with pytest.raises(ValueError):
        AugmentRecipe(resize=20, crop=(32, 32), pad=4).check(32, 64)   # Hr + 2*pad = 28 < 32
    AugmentRecipe(resize=24, crop=(32, 32), pad=4).check(32, 64)       # exactly one position


def _staged(img, recipe, params):
    """The CPU transforms' arithmetic with the draws fixed: interpolate -> round to uint8 ->
    pad / crop -> flip -> affine_grid + grid_sample -> round to uint8 -> /255."""
    dy, dx, flip, angle, scale = params[:5]
    t = img.permute(2, 0, 1).double()[None]
    if recipe.resize:
        t = F.interpolate(t, size=recipe.resized_hw(*img.shape[:2]), mode='bilinear',
                          align_corners=False).clamp(0, 255).round()
    p = recipe.pad
    t = F.pad(t, (p, p, p, p))
    H, W = recipe.crop
    t = t[..., dy:dy + H, dx:dx + W]
    if flip:
        t = t.flip(-1)
    if recipe.affine:
        a = math.radians(angle)
        c, s = math.cos(a) / scale, math.sin(a) / scale
        theta = torch.tensor([[c, -s, 0.0], [s, c, 0.0]], dtype=torch.float64)[None]
        grid = F.affine_grid(theta, list(t.shape), align_corners=False)
        t = F.grid_sample(t, grid, mode='bilinear', padding_mode='zeros',
                          align_corners=False).clamp(0, 255).round()
    return (t[0] / 255).permute(1, 2, 0)


@pytest.mark.parametrize('hw,recipe,params', [
    ((32, 32), FULL, (2, 3, 1, 7.5, 1.07, 0, 0)),
    ((32, 32), FULL, (0, 0, 0, -10.0, 0.9, 0, 0)),
    ((32, 32), FULL, (3, 1, 1, 0.0, 1.0, 0, 0)),
    ((24, 32), AugmentRecipe(resize=27, crop=(24, 24), pad=2, flip=True, degrees=10.0,
                             scale=(0.9, 1.1)), (7, 16, 1, -4.25, 0.93, 0, 0)),
    ((24, 32), AugmentRecipe(resize=27, crop=(24, 24), pad=2, flip=True), (0, 0, 0, 0.0, 1.0, 0, 0)),
])
def test_reference_within_one_level_of_the_rounded_pipeline(hw, recipe, params):
    """The recipe keeps values float between the stages, the CPU transforms round to uint8
    after Resize and after RandomAffine: at most 0.5 level each, so within one level."""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    img = torch.randint(0, 256, hw + (3,), dtype=torch.uint8, generator=g)
    ref = recipe.reference(img, params)
    assert ref.shape == recipe.crop + (3,) and ref.dtype == torch.float64
    err = (ref - _staged(img, recipe, params)).abs().max().item()
    print('max |unrounded - rounded| = %.4f levels' % (err * 255))
    assert err <= 1 / 255
    if not recipe.affine:      # one rounding only
        assert err <= 0.5 / 255 + 1e-12


def test_reference_normalize_cutout_and_plain_crop():
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (12, 12, 3), dtype=torch.uint8, generator=g)
    r = AugmentRecipe(crop=(8, 8), pad=1, flip=True, cutout=4, mean=T.CIFAR_MEAN, std=T.CIFAR_STD)
    out = r.reference(img, (2, 5, 1, 0.0, 1.0, 1, 7))
    view = F.pad(img.permute(2, 0, 1), (1, 1, 1, 1))[:, 2:10, 5:13].flip(-1).permute(1, 2, 0)
    want = (view.double() / 255 - torch.tensor(T.CIFAR_MEAN, dtype=torch.float64)) \
        / torch.tensor(T.CIFAR_STD, dtype=torch.float64)
    want[0:3, 5:8] = 0            # Cutout(4) at (1, 7): rows clip(-1..3), columns clip(5..9)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
