"""Augmentation recipes for the native engine's pool build.

An ``AugmentRecipe`` is the data form of one ``transforms.Compose``:

    [Resize] -> RandomCrop(pad) -> [RandomHorizontalFlip] -> [RandomAffine] -> ToTensor
             -> [Normalize] -> [Cutout]

``ops.pool_build(..., recipe=r)`` runs it on the GPU for a whole presample pool
(``pool_augment_kernel``, ``csrc/importance.hip``); ``r.reference`` is the same
arithmetic for one image on the CPU, with the random draws passed in, and is what the
GPU tests compare against.  Per output pixel (i, j) of the H x W crop:

1. affine (only with ``degrees`` or ``scale``): ``xn = (2j+1)/W - 1``, ``yn = (2i+1)/H - 1``,
   ``c, s = cos(a)/scale, sin(a)/scale``, ``gx = c*xn - s*yn``, ``gy = s*xn + c*yn``,
   ``fx = ((gx+1)*W - 1)/2`` (``fy`` likewise), bilinear over the four taps at
   ``floor(fx), floor(fy)``; a tap outside the crop contributes 0 (``affine_grid`` +
   ``grid_sample``, ``align_corners=False``).  Without it the one tap is (i, j).
2. tap (y, x) of the crop: ``xc = W-1-x`` if flipped, ``ys = y + dy - pad``,
   ``xs = xc + dx - pad``; 0 outside the resized image.
3. the resized image at (ys, xs): torch's bilinear, ``align_corners=False``:
   ``fy = max((ys+0.5)*Hs/Hr - 0.5, 0)``, rows ``floor(fy)`` and ``min(floor(fy)+1, Hs-1)``.
4. ``(v/255 - mean)/std``, then 0 inside the cutout square.

Values stay float between the stages.  The CPU transforms round to uint8 after ``Resize``
and after ``RandomAffine``; the unrounded result is within one uint8 level of theirs.

``SpecRecipe`` (below) is the recipe of float spectrogram inputs: time shift, gain, frequency
and time masks, run by ``pool_spec_kernel`` from a planar bf16 shard and exact to the bit.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import transforms as T
from .transforms import CIFAR_MEAN, CIFAR_STD


def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, float)) else (int(v[0]), int(v[1]))


@dataclass(frozen=True)
class AugmentRecipe:
    crop: Optional[Tuple[int, int]] = None   # output (h, w); None: the source size (no crop)
    resize: int = 0                          # 0: off, else the shorter side's new length
    pad: int = 0
    flip: bool = False
    degrees: float = 0.0
    scale: Optional[Tuple[float, float]] = None
    cutout: int = 0
    mean: Optional[Tuple[float, ...]] = None  # None: no Normalize (mean 0, std 1)
    std: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        s = object.__setattr__
        if self.crop is not None:
            s(self, 'crop', _pair(self.crop))
        s(self, 'resize', int(self.resize))
        s(self, 'pad', int(self.pad))
        s(self, 'flip', bool(self.flip))
        s(self, 'degrees', float(self.degrees))
        s(self, 'cutout', int(self.cutout))
        if self.scale is not None:
            s(self, 'scale', (float(self.scale[0]), float(self.scale[1])))
        if (self.mean is None) != (self.std is None):
            raise ValueError('AugmentRecipe: mean and std come together')
        if self.mean is not None:
            s(self, 'mean', tuple(float(m) for m in self.mean))
            s(self, 'std', tuple(float(v) for v in self.std))
            if len(self.mean) != 3 or len(self.std) != 3:
                raise ValueError('AugmentRecipe: mean and std have three channels')
        if self.resize < 0 or self.pad < 0 or self.cutout < 0 or self.degrees < 0:
            raise ValueError('AugmentRecipe: resize, pad, cutout and degrees are >= 0')
        if self.scale is not None and not 0 < self.scale[0] <= self.scale[1]:
            raise ValueError('AugmentRecipe: scale is (lo, hi) with 0 < lo <= hi')

    # ---------------------------------------------------------------- constructors
    @classmethod
    def cifar(cls, hw=(32, 32)):
        """The pipeline the engine runs when it is given no recipe."""
        return cls(crop=hw, pad=4, flip=True, mean=CIFAR_MEAN, std=CIFAR_STD)

    @classmethod
    def from_transform(cls, t):
        """Read a ``transforms.Compose`` of this package's classes, in the order of the module
        docstring; ``ValueError`` names the transform that does not fit."""
        if t is None:
            return cls.cifar()
        if not isinstance(t, T.Compose):
            raise ValueError('AugmentRecipe.from_transform: expected a transforms.Compose, got %r'
                             % (t,))
        order = [T.ToPILImage, T.Resize, T.RandomCrop, T.RandomHorizontalFlip, T.RandomAffine,
                 T.ToTensor, T.Normalize, T.Cutout]
        kw, pos, seen_tensor = {}, 0, False
        for tr in t.transforms:
            k = next((i for i in range(pos, len(order)) if type(tr) is order[i]), None)
            if k is None:
                raise ValueError(
                    'AugmentRecipe.from_transform: %r is not supported here (accepted, in this '
                    'order: %s)' % (tr, ', '.join(c.__name__ for c in order)))
            pos = k + 1
            if isinstance(tr, T.Resize):
                kw['resize'] = tr.size
            elif isinstance(tr, T.RandomCrop):
                kw['crop'], kw['pad'] = _pair(tr.size), tr.padding
            elif isinstance(tr, T.RandomHorizontalFlip):
                if tr.p != 0.5:
                    raise ValueError('AugmentRecipe.from_transform: %r with p=%r (only p=0.5 is '
                                     'supported)' % (tr, tr.p))
                kw['flip'] = True
            elif isinstance(tr, T.RandomAffine):
                lo, hi = tr.degrees
                if lo != -hi or hi < 0:
                    raise ValueError('AugmentRecipe.from_transform: %r with degrees=%r (only a '
                                     'symmetric range is supported)' % (tr, tr.degrees))
                kw['degrees'], kw['scale'] = hi, tr.scale
            elif isinstance(tr, T.ToTensor):
                seen_tensor = True
            elif isinstance(tr, T.Normalize):
                kw['mean'], kw['std'] = tr.mean_values, tr.std_values
            elif isinstance(tr, T.Cutout):
                kw['cutout'] = tr.length
        if not seen_tensor:
            raise ValueError('AugmentRecipe.from_transform: the Compose has no ToTensor')
        return cls(**kw)

    @classmethod
    def parse(cls, spec):
        """``resize=35,crop=32,flip=1,degrees=10,scale=0.9:1.1,cutout=0,norm=none``; ``crop`` is
        ``32`` or ``24x32``, ``norm`` is ``cifar``, ``none`` or ``m0:m1:m2/s0:s1:s2``."""
        kw = {}
        for item in spec.split(','):
            if '=' not in item:
                raise ValueError('AugmentRecipe.parse: %r is not name=value' % item)
            k, v = (s.strip() for s in item.split('=', 1))
            if k in ('resize', 'pad', 'cutout'):
                kw[k] = int(v)
            elif k == 'crop':
                kw[k] = _pair([int(x) for x in v.split('x')] if 'x' in v else int(v))
            elif k == 'flip':
                kw[k] = v.lower() in ('1', 'true', 'yes', 'y')
            elif k == 'degrees':
                kw[k] = float(v)
            elif k == 'scale':
                kw[k] = None if v in ('', 'none') else tuple(float(x) for x in v.split(':'))
                if kw[k] is not None and len(kw[k]) != 2:
                    raise ValueError('AugmentRecipe.parse: scale is lo:hi')
            elif k == 'norm':
                if v == 'cifar':
                    kw['mean'], kw['std'] = CIFAR_MEAN, CIFAR_STD
                elif v != 'none':
                    m, _, s = v.partition('/')
                    kw['mean'] = [float(x) for x in m.split(':')]
                    kw['std'] = [float(x) for x in s.split(':')] if s else []
            else:
                raise ValueError('AugmentRecipe.parse: unknown key %r' % k)
        return cls(**kw)

    def spec(self):
        """The ``parse`` form of this recipe."""
        out = ['resize=%d' % self.resize]
        if self.crop is not None:
            out.append('crop=%dx%d' % self.crop)
        out += ['pad=%d' % self.pad, 'flip=%d' % self.flip, 'degrees=%r' % self.degrees]
        if self.scale is not None:
            out.append('scale=%r:%r' % self.scale)
        out.append('cutout=%d' % self.cutout)
        if self.mean is None:
            out.append('norm=none')
        else:
            out.append('norm=%s/%s' % (':'.join(repr(m) for m in self.mean),
                                       ':'.join(repr(s) for s in self.std)))
        return ','.join(out)

    # ---------------------------------------------------------------- geometry
    @property
    def out_hw(self):
        return self.crop

    @property
    def affine(self):
        return self.degrees != 0 or self.scale is not None

    def with_crop(self, hw):
        """This recipe with ``crop`` filled in where the Compose had no RandomCrop."""
        return self if self.crop is not None else dataclasses.replace(self, crop=_pair(hw))

    def resized_hw(self, Hs, Ws):
        """``transforms.Resize``'s output size (the shorter side becomes ``resize``)."""
        if not self.resize:
            return Hs, Ws
        if Hs <= Ws:
            return self.resize, int(self.resize * Ws / Hs)
        return int(self.resize * Hs / Ws), self.resize

    def check(self, Hs, Ws):
        """Raise unless both crop ranges are non-empty on an Hs x Ws source."""
        if self.crop is None:
            raise ValueError('AugmentRecipe: crop is unset (with_crop)')
        Hr, Wr = self.resized_hw(Hs, Ws)
        H, W = self.crop
        if min(H, W, Hr, Wr) < 1 or Hr + 2 * self.pad < H or Wr + 2 * self.pad < W:
            raise ValueError('AugmentRecipe: crop %dx%d does not fit the %dx%d image (source '
                             '%dx%d, resize %d) with padding %d'
                             % (H, W, Hr, Wr, Hs, Ws, self.resize, self.pad))

    def is_legacy(self, Hs, Ws):
        """Crop-with-pad and flip on a shard of the output size: ``pool_build_kernel``'s case."""
        return (not self.resize and not self.affine and not self.cutout
                and self.crop == (Hs, Ws))

    def norm(self):
        return (self.mean or (0.0, 0.0, 0.0)), (self.std or (1.0, 1.0, 1.0))

    # ---------------------------------------------------------------- CPU reference
    def reference(self, img_u8, params, dtype=torch.float64):
        """The recipe on one HWC uint8 image with explicit draws ``params = (dy, dx, flip,
        angle_deg, scale, cut_y, cut_x)`` -> [H][W][3] ``dtype`` (module docstring)."""
        src = torch.as_tensor(img_u8)
        if src.dim() != 3 or src.shape[2] != 3:
            raise ValueError('reference: image must be [H][W][3]')
        src = src.to(dtype)
        Hs, Ws = src.shape[:2]
        self.check(Hs, Ws)
        Hr, Wr = self.resized_hw(Hs, Ws)
        H, W = self.crop
        pad = self.pad
        dy, dx, flip = int(params[0]), int(params[1]), bool(int(params[2]))
        angle, scale = float(params[3]), float(params[4])
        cut_y, cut_x = int(params[5]), int(params[6])

        def resized(ys, xs):            # long tensors inside [0, Hr) x [0, Wr)
            if not self.resize:
                return src[ys, xs]
            fy = ((ys.to(dtype) + 0.5) * (Hs / Hr) - 0.5).clamp(min=0)
            fx = ((xs.to(dtype) + 0.5) * (Ws / Wr) - 0.5).clamp(min=0)
            y0 = fy.floor().long().clamp(max=Hs - 1)
            x0 = fx.floor().long().clamp(max=Ws - 1)
            y1, x1 = (y0 + 1).clamp(max=Hs - 1), (x0 + 1).clamp(max=Ws - 1)
            ly, lx = (fy - y0).unsqueeze(-1), (fx - x0).unsqueeze(-1)
            top = src[y0, x0] * (1 - lx) + src[y0, x1] * lx
            bot = src[y1, x0] * (1 - lx) + src[y1, x1] * lx
            return top * (1 - ly) + bot * ly

        def tap(y, x):                  # long tensors, any value
            xc = W - 1 - x if flip else x
            ys, xs = y + dy - pad, xc + dx - pad
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W) & \
                (ys >= 0) & (ys < Hr) & (xs >= 0) & (xs < Wr)
            v = resized(ys.clamp(0, Hr - 1), xs.clamp(0, Wr - 1))
            return v * ok.unsqueeze(-1).to(dtype)

        i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
        if self.affine:
            xn = (2 * j + 1).to(dtype) / W - 1
            yn = (2 * i + 1).to(dtype) / H - 1
            c, s = math.cos(math.radians(angle)) / scale, math.sin(math.radians(angle)) / scale
            fx = ((c * xn - s * yn + 1) * W - 1) / 2
            fy = ((s * xn + c * yn + 1) * H - 1) / 2
            x0f, y0f = fx.floor(), fy.floor()
            lx, ly = (fx - x0f).unsqueeze(-1), (fy - y0f).unsqueeze(-1)
            x0, y0 = x0f.long(), y0f.long()
            v = (tap(y0, x0) * (1 - lx) + tap(y0, x0 + 1) * lx) * (1 - ly) + \
                (tap(y0 + 1, x0) * (1 - lx) + tap(y0 + 1, x0 + 1) * lx) * ly
        else:
            v = tap(i, j)
        mean, std = self.norm()
        out = (v / 255 - torch.tensor(mean, dtype=dtype)) / torch.tensor(std, dtype=dtype)
        if self.cutout:
            h = self.cutout // 2
            y1, y2 = min(max(cut_y - h, 0), H), min(max(cut_y + h, 0), H)
            x1, x2 = min(max(cut_x - h, 0), W), min(max(cut_x + h, 0), W)
            out[y1:y2, x1:x2] = 0
        return out


# ---------------------------------------------------------------------- spectrograms
SPEC_PARAMS = 12     # shift, gain, f0a, fwa, f0b, fwb, t0a, twa, t0b, twb, 0, 0


def _mask(v, name):
    if len(v) != 2:
        raise ValueError('SpecRecipe: %s is (n, max)' % name)
    n, m = int(v[0]), int(v[1])
    if not 0 <= n <= 2 or m < 0:
        raise ValueError('SpecRecipe: %s is (n, max) with 0 <= n <= 2 and max >= 0, got %r'
                         % (name, (n, m)))
    return n, m


@dataclass(frozen=True)
class SpecRecipe:
    """Time shift, gain and SpecAugment-style masks for float inputs ``x[c][f][t]`` (``f < H``
    frequency rows, ``t < W`` frames), run by ``pool_spec_kernel`` (``csrc/importance.hip``) on a
    planar bf16 shard [Ns][C][H][W] for a whole pool: ``ops.pool_build(..., recipe=r)``.

    Output pixel ``y[f][t][c]`` of the NHWC8 pool, given the slot's draws:

    1. ``fill`` if ``f`` lies in a frequency band ``[f0, f0+fw)`` or ``t`` in a time band
       ``[t0, t0+tw)`` -- bands are in OUTPUT coordinates, applied after the shift;
    2. else ``ts = t - shift``; ``fill`` if ``ts < 0`` or ``ts >= W``;
    3. else ``bf16(float(x[c][f][ts]) * gain)``, one fp32 multiply rounded to nearest even.
       With ``gain=None`` the factor is exactly 1.0, so values pass through bit for bit.

    Channels ``C..7`` are +0; ``fill`` is rounded to bf16 once.  Draws, per pool slot (Philox on
    the image kernels' counter ``(gb, t)``, stream words 0x5bec0..0x5bec2 of its own):
    ``shift = r % (2*shift_max + 1) - shift_max``; each mask ``w = r % (max + 1)``,
    ``start = r' % (size - w + 1)``, masks beyond ``n`` have width 0;
    ``gain = lo + (hi - lo) * u01(r)``; with ``augment=False`` every draw is the identity."""
    shift: int = 0                                  # maximum time shift in frames
    fmask: Tuple[int, int] = (0, 0)                 # (n, Fmax): frequency masks
    tmask: Tuple[int, int] = (0, 0)                 # (n, Tmax): time masks
    gain: Optional[Tuple[float, float]] = None      # (lo, hi) multiplicative gain
    fill: float = 0.0

    def __post_init__(self):
        s = object.__setattr__
        s(self, 'shift', int(self.shift))
        s(self, 'fmask', _mask(self.fmask, 'fmask'))
        s(self, 'tmask', _mask(self.tmask, 'tmask'))
        s(self, 'fill', float(self.fill))
        if self.shift < 0:
            raise ValueError('SpecRecipe: shift is >= 0, got %d' % self.shift)
        if self.gain is not None:
            if len(self.gain) != 2:
                raise ValueError('SpecRecipe: gain is (lo, hi)')
            s(self, 'gain', (float(self.gain[0]), float(self.gain[1])))
            if not all(math.isfinite(g) for g in self.gain) or self.gain[0] > self.gain[1]:
                raise ValueError('SpecRecipe: gain is (lo, hi), finite, lo <= hi, got %r'
                                 % (self.gain,))
        if not math.isfinite(self.fill):
            raise ValueError('SpecRecipe: fill is finite, got %r' % self.fill)

    @classmethod
    def parse(cls, spec):
        """``spec:shift=8,fmask=2x10,tmask=2x20,gain=0.8:1.2,fill=0`` (the ``spec:`` prefix is
        optional here; ``Config.augment`` needs it to tell the two recipe kinds apart)."""
        spec = spec.strip()
        if spec.startswith('spec:'):
            spec = spec[5:]
        kw = {}
        for item in (spec.split(',') if spec else []):
            if '=' not in item:
                raise ValueError('SpecRecipe.parse: %r is not name=value' % item)
            k, v = (s.strip() for s in item.split('=', 1))
            if k == 'shift':
                kw[k] = int(v)
            elif k in ('fmask', 'tmask'):
                nm = v.split('x')
                if len(nm) != 2:
                    raise ValueError('SpecRecipe.parse: %s is NxMAX, got %r' % (k, v))
                kw[k] = (int(nm[0]), int(nm[1]))
            elif k == 'gain':
                if v in ('', 'none'):
                    kw[k] = None
                else:
                    g = v.split(':')
                    if len(g) != 2:
                        raise ValueError('SpecRecipe.parse: gain is lo:hi, got %r' % v)
                    kw[k] = (float(g[0]), float(g[1]))
            elif k == 'fill':
                kw[k] = float(v)
            else:
                raise ValueError('SpecRecipe.parse: unknown key %r' % k)
        return cls(**kw)

    def spec(self):
        """The ``parse`` form of this recipe, with the ``spec:`` prefix."""
        out = ['shift=%d' % self.shift, 'fmask=%dx%d' % self.fmask, 'tmask=%dx%d' % self.tmask]
        if self.gain is not None:
            out.append('gain=%r:%r' % self.gain)
        out.append('fill=%r' % self.fill)
        return 'spec:' + ','.join(out)

    @property
    def identity(self):
        """Nothing on: every draw is the identity whatever the random words."""
        return (self.shift == 0 and 0 in self.fmask and 0 in self.tmask and self.gain is None)

    def check(self, C, H, W):
        """Raise unless the recipe fits a [C][H][W] sample; names the field that does not."""
        if not 1 <= C <= 8:
            raise ValueError('SpecRecipe: C must be 1..8, got %d' % C)
        if H < 1 or W < 1:
            raise ValueError('SpecRecipe: empty sample %dx%d' % (H, W))
        if self.shift > W - 1:
            raise ValueError('SpecRecipe: shift %d exceeds W-1 = %d' % (self.shift, W - 1))
        if self.fmask[1] > H:
            raise ValueError('SpecRecipe: fmask width %d exceeds H = %d' % (self.fmask[1], H))
        if self.tmask[1] > W:
            raise ValueError('SpecRecipe: tmask width %d exceeds W = %d' % (self.tmask[1], W))

    def draw(self, H, W, generator=None):
        """One slot's draws from torch's RNG, in the kernel's ranges and ``params`` layout."""
        def ri(n):
            return int(torch.randint(0, n, (1,), generator=generator).item())
        p = [0.0] * SPEC_PARAMS
        p[0] = float(ri(2 * self.shift + 1) - self.shift)
        p[1] = 1.0
        if self.gain is not None:
            lo, hi = self.gain
            p[1] = lo + (hi - lo) * float(torch.rand(1, generator=generator).item())
        for base, (n, mx), size in ((2, self.fmask, H), (6, self.tmask, W)):
            for k in range(n):
                w = ri(mx + 1)
                p[base + 2 * k], p[base + 2 * k + 1] = float(ri(size - w + 1)), float(w)
        return p

    # ---------------------------------------------------------------- CPU reference
    def reference(self, x, params, dtype=torch.bfloat16):
        """The recipe on one [C][H][W] sample with explicit draws ``params`` (``SPEC_PARAMS``
        values, the kernel's layout) -> [H][W][8] ``dtype``, the pool's layout (class
        docstring).  ``x`` is rounded to ``dtype`` first, as the shard is."""
        x = torch.as_tensor(x)
        if x.dim() != 3:
            raise ValueError('reference: sample must be [C][H][W]')
        C, H, W = x.shape
        self.check(C, H, W)
        p = [float(v) for v in params]
        if len(p) != SPEC_PARAMS:
            raise ValueError('reference: params has %d values' % SPEC_PARAMS)
        shift = int(p[0])
        gain = torch.tensor(p[1], dtype=torch.float32)
        x = x.to(dtype).to(torch.float32)
        fill = torch.tensor(self.fill, dtype=torch.float32).to(dtype)
        f = torch.arange(H).view(H, 1)
        t = torch.arange(W).view(1, W)
        masked = torch.zeros(H, W, dtype=torch.bool)
        for k in (2, 4):
            masked |= (f >= int(p[k])) & (f < int(p[k]) + int(p[k + 1]))
        for k in (6, 8):
            masked |= (t >= int(p[k])) & (t < int(p[k]) + int(p[k + 1]))
        ts = t - shift
        live = ~masked & (ts >= 0) & (ts < W)
        v = (x[:, :, ts.clamp(0, W - 1).view(W)] * gain).to(dtype)       # [C][H][W]
        v = torch.where(live.unsqueeze(0), v, fill)
        out = torch.zeros(H, W, 8, dtype=dtype)
        out[:, :, :C] = v.permute(1, 2, 0)
        return out
