"""Self-contained image transforms (torchvision is not installed).

Semantics follow the transforms the reference composes in
`cifar10/data_loader.py:78-111` and `exp_dataset.py:22-29,63-67`.  Inputs are
HWC uint8 ``numpy`` arrays (what ``CIFAR10_truncated.data`` holds) or CHW float
tensors after ``ToTensor``.  The randomness uses numpy's global RNG (like
torchvision uses torch's) so seeded runs are reproducible.

On the GPU hot path none of these objects run.  ``mercury_amd.ops.pool_build``
builds a whole presample pool in one HIP kernel from the HBM-resident uint8 shard:
by default RandomCrop(pad 4) + flip + CIFAR Normalize, or, given an
``AugmentRecipe`` (``data/augment.py``), the pipeline that recipe describes --
Resize, RandomCrop, RandomHorizontalFlip, RandomAffine, Normalize, Cutout, and the
photographic pair RandomResizedCrop and ColorJitter (``pool_recipe_kernel``), whose
classes here run the recipe's own reference arithmetic.
``AugmentRecipe.from_transform`` reads a ``Compose`` of the classes below into a
recipe (``Config.augment = 'dataset'``), so the native engine applies what the
dataset's transform says; the kernel keeps values in float between the stages,
where ``Resize`` and ``RandomAffine`` here round to uint8 (at most one level apart).
``SpecAugment`` is the float-spectrogram counterpart: it carries a ``SpecRecipe`` that the
pool build runs from a planar bf16 shard (``pool_spec_kernel``).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

CIFAR_MEAN = [0.49139968, 0.48215827, 0.44653124]
CIFAR_STD = [0.24703233, 0.24348505, 0.26158768]
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]


class Compose(object):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToPILImage(object):
    """Identity on HWC uint8 arrays (kept so reference pipelines read the same)."""

    def __call__(self, x):
        return np.asarray(x)


class ToNumpy(object):
    """PIL image / array -> ndarray (`util.py:73-91`)."""

    def __call__(self, pic):
        return np.array(pic)

    def __repr__(self):
        return self.__class__.__name__ + '()'


def _as_hwc(x):
    if torch.is_tensor(x):
        return x
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[:, :, None]
    return x


class RandomCrop(object):
    def __init__(self, size, padding=0):
        self.size = size
        self.padding = padding

    def __call__(self, x):
        x = _as_hwc(x)
        if torch.is_tensor(x):  # CHW tensor
            p = self.padding
            if p:
                x = F.pad(x, (p, p, p, p))
            h, w = x.shape[-2:]
            i = np.random.randint(0, h - self.size + 1)
            j = np.random.randint(0, w - self.size + 1)
            return x[..., i:i + self.size, j:j + self.size]
        p = self.padding
        if p:
            x = np.pad(x, ((p, p), (p, p), (0, 0)))
        h, w = x.shape[:2]
        i = np.random.randint(0, h - self.size + 1)
        j = np.random.randint(0, w - self.size + 1)
        return x[i:i + self.size, j:j + self.size]


class RandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, x):
        if np.random.rand() < self.p:
            if torch.is_tensor(x):
                return x.flip(-1)
            return _as_hwc(x)[:, ::-1]
        return x


class ToTensor(object):
    def __call__(self, x):
        if torch.is_tensor(x):
            return x
        x = np.ascontiguousarray(_as_hwc(x))
        t = torch.from_numpy(x).permute(2, 0, 1).contiguous()
        return t.float().div_(255.0) if t.dtype == torch.uint8 else t.float()


class Normalize(object):
    def __init__(self, mean, std):
        # (the constructor's own numbers: AugmentRecipe.from_transform reads these)
        self.mean_values = tuple(float(m) for m in mean)
        self.std_values = tuple(float(s) for s in std)
        self.mean = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)

    def __call__(self, t):
        return (t - self.mean) / self.std


class Resize(object):
    """Resize the shorter side to ``size`` (bilinear) like torchvision."""

    def __init__(self, size):
        self.size = size

    def __call__(self, x):
        t = x if torch.is_tensor(x) else torch.from_numpy(
            np.ascontiguousarray(_as_hwc(x))).permute(2, 0, 1).float()
        h, w = t.shape[-2:]
        if h <= w:
            nh, nw = self.size, int(self.size * w / h)
        else:
            nh, nw = int(self.size * h / w), self.size
        out = F.interpolate(t[None], size=(nh, nw), mode='bilinear', align_corners=False)[0]
        if torch.is_tensor(x):
            return out
        return out.clamp(0, 255).round().byte().permute(1, 2, 0).numpy()


class RandomAffine(object):
    """Rotation + isotropic scale about the centre (the subset used by `exp_dataset.py:27`)."""

    def __init__(self, degrees, scale=None):
        self.degrees = (-degrees, degrees) if np.isscalar(degrees) else degrees
        self.scale = scale

    def __call__(self, x):
        is_np = not torch.is_tensor(x)
        t = torch.from_numpy(np.ascontiguousarray(_as_hwc(x))).permute(2, 0, 1).float() \
            if is_np else x.float()
        ang = math.radians(np.random.uniform(*self.degrees))
        sc = np.random.uniform(*self.scale) if self.scale else 1.0
        c, s = math.cos(ang) / sc, math.sin(ang) / sc
        theta = torch.tensor([[c, -s, 0.0], [s, c, 0.0]], dtype=torch.float32)[None]
        grid = F.affine_grid(theta, [1] + list(t.shape), align_corners=False)
        out = F.grid_sample(t[None], grid, align_corners=False)[0]
        if is_np:
            return out.clamp(0, 255).round().byte().permute(1, 2, 0).numpy()
        return out


class Cutout(object):
    """Zero a random square (`cifar10/data_loader.py:57-75`)."""

    def __init__(self, length):
        self.length = length

    def __call__(self, img):
        h, w = img.size(1), img.size(2)
        mask = np.ones((h, w), np.float32)
        y = np.random.randint(h)
        x = np.random.randint(w)
        y1, y2 = np.clip(y - self.length // 2, 0, h), np.clip(y + self.length // 2, 0, h)
        x1, x2 = np.clip(x - self.length // 2, 0, w), np.clip(x + self.length // 2, 0, w)
        mask[y1:y2, x1:x2] = 0.
        return img * torch.from_numpy(mask).expand_as(img)


def _to_u8(ref):
    """``AugmentRecipe.reference`` output without Normalize ([0, 1]) -> HWC uint8 array."""
    return (ref * 255).clamp(0, 255).round().byte().numpy()


class RandomResizedCrop(object):
    """A random box of the image (area fraction in ``scale``, aspect log-uniform in ``ratio``,
    torchvision's ``get_params`` with its fallback) resized to ``size``, bilinear, no
    antialiasing, on an HWC uint8 array.  The draws come from numpy's global RNG; the arithmetic
    is ``AugmentRecipe.reference`` (``data/augment.py``) in fp64, rounded to uint8, so this and
    the native engine's pool build agree on what the transform means.  ``last``: the last
    call's draws in the recipe's 16-value params layout."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        from .augment import AugmentRecipe
        self.size = size
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.recipe = AugmentRecipe(crop=size, rrc=self.scale + self.ratio)
        self.last = None

    def get_params(self, Hs, Ws):
        """``(top, left, h, w, attempt)``; attempt 10 is the fallback box."""
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for attempt in range(10):
            target = Hs * Ws * np.random.uniform(*self.scale)
            aspect = math.exp(np.random.uniform(lo, hi))
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= Ws and 0 < h <= Hs:
                return (np.random.randint(0, Hs - h + 1), np.random.randint(0, Ws - w + 1), h, w,
                        attempt)
        return self.recipe.fallback_box(Hs, Ws) + (10,)

    def __call__(self, x):
        x = np.ascontiguousarray(_as_hwc(x))
        top, left, h, w, attempt = self.get_params(x.shape[0], x.shape[1])
        self.last = [float(top), float(left), 0.0, 0.0, 1.0, 0.0, 0.0, float(attempt), float(h),
                     float(w), 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
        return _to_u8(self.recipe.reference(x, self.last))

    def __repr__(self):
        return 'RandomResizedCrop(size=%r, scale=%r, ratio=%r)' % (self.size, self.scale,
                                                                   self.ratio)


class ColorJitter(object):
    """Brightness, contrast, saturation and hue in a random order (torchvision's tensor-path
    arithmetic) on an HWC uint8 array; each argument is a strength ``x``: the factor is drawn
    from ``[max(0, 1 - x), 1 + x]``, the hue shift from ``[-hue, hue]``, the order is one of 24
    (``AugmentRecipe.jitter_order``).  Draws from numpy's global RNG, arithmetic of
    ``AugmentRecipe.reference`` in fp64, rounded to uint8; ``last`` as in RandomResizedCrop."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        from .augment import AugmentRecipe
        self.brightness, self.contrast = float(brightness), float(contrast)
        self.saturation, self.hue = float(saturation), float(hue)
        # (validates the strengths; all four zero is the identity)
        self.recipe = AugmentRecipe(jitter=(self.brightness, self.contrast, self.saturation,
                                            self.hue))
        self.last = None

    def __call__(self, x):
        x = np.ascontiguousarray(_as_hwc(x))
        f = [np.random.uniform(max(0.0, 1.0 - s), 1.0 + s)
             for s in (self.brightness, self.contrast, self.saturation)]
        f.append(np.random.uniform(-self.hue, self.hue))
        code = int(np.random.randint(24))
        self.last = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] + \
            [float(v) for v in f] + [float(code), 0.0]
        if self.recipe.jitter is None:
            return x
        return _to_u8(self.recipe.with_crop(x.shape[:2]).reference(x, self.last))

    def __repr__(self):
        return 'ColorJitter(brightness=%r, contrast=%r, saturation=%r, hue=%r)' % (
            self.brightness, self.contrast, self.saturation, self.hue)


class SpecAugment(object):
    """A ``SpecRecipe`` (``data/augment.py``: time shift, gain, frequency and time masks) on one
    float [C][F][T] tensor: the draws come from torch's RNG (``generator``, default the global
    one) in the recipe's ranges, the arithmetic is ``SpecRecipe.reference`` in the input's dtype.
    The eager ``Trainer`` and ``MyLSTM`` run it as the dataset's transform on any device;
    ``Config(augment='dataset')`` hands its recipe to the native engine's pool build instead."""

    def __init__(self, recipe, generator=None):
        from .augment import SpecRecipe
        self.recipe = SpecRecipe.parse(recipe) if isinstance(recipe, str) else recipe
        if not isinstance(self.recipe, SpecRecipe):
            raise ValueError('SpecAugment: expected a SpecRecipe or its spec string, got %r'
                             % (recipe,))
        self.generator = generator
        self.last = None                 # the last call's draws (SpecRecipe's params layout)

    def __call__(self, x):
        x = torch.as_tensor(x)
        C, F_, T_ = x.shape
        self.last = self.recipe.draw(F_, T_, self.generator)
        y = self.recipe.reference(x, self.last, dtype=x.dtype)
        return y[:, :, :C].permute(2, 0, 1).contiguous()

    def __repr__(self):
        return 'SpecAugment(%r)' % self.recipe.spec()


def cifar_train_transform():
    return Compose([ToPILImage(), RandomCrop(32, padding=4), RandomHorizontalFlip(),
                    ToTensor(), Normalize(CIFAR_MEAN, CIFAR_STD)])


def cifar_test_transform():
    return Compose([ToPILImage(), ToTensor(), Normalize(CIFAR_MEAN, CIFAR_STD)])


def imagenet_train_transform(size=224):
    """The usual ImageNet training pipeline: RandomResizedCrop, flip, ImageNet Normalize."""
    return Compose([ToPILImage(), RandomResizedCrop(size), RandomHorizontalFlip(), ToTensor(),
                    Normalize(IMAGENET_MEAN, IMAGENET_STD)])


def affine_train_transform():
    """The IID loaders' train pipeline (`exp_dataset.py:23-29`); no Normalize."""
    return Compose([Resize(35), RandomCrop(32), RandomHorizontalFlip(),
                    RandomAffine(degrees=10, scale=(0.9, 1.1)), ToTensor()])


def affine_test_transform():
    """... and their test pipeline (`exp_dataset.py:63-67`)."""
    return Compose([Resize(33), RandomCrop(32), ToTensor()])


def _data_transforms_cifar10():
    return cifar_train_transform(), cifar_test_transform()
