"""Augmentation recipes for the native engine's pool build.

An ``AugmentRecipe`` is the data form of one ``transforms.Compose``:

    [Resize] -> RandomCrop(pad) -> [RandomHorizontalFlip] -> [RandomAffine] -> ToTensor
             -> [Normalize] -> [Cutout]

``ops.pool_build(..., recipe=r)`` runs it on the GPU for a whole presample pool
(``pool_recipe_kernel``, ``csrc/pool_recipe.hip``); ``r.reference`` is the same
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

Photographic recipes add two optional fields (the same kernel, with a box or colour draw; params
are then ``PHOTO_PARAMS`` = 16 values per slot):

    RandomResizedCrop | the geometry above -> [flip] -> [ColorJitter] -> /255 -> [Normalize]
                      -> [Cutout]

* ``rrc = (scale_lo, scale_hi, ratio_lo, ratio_hi)``: ``RandomResizedCrop`` to ``crop``, in the
  place of Resize, RandomCrop, padding and RandomAffine.  The box is torchvision's
  ``get_params``: up to 10 attempts of ``target = Hs*Ws * U(scale)``, ``aspect = exp(U(log
  ratio))``, ``w = round(sqrt(target*aspect))``, ``h = round(sqrt(target/aspect))``, the first
  with ``0 < w <= Ws`` and ``0 < h <= Hs`` wins, ``top = r % (Hs-h+1)``, ``left = r' % (Ws-w+1)``;
  else the whole image clipped to the ratio range, centred (``fallback_box``).  The box is
  resized bilinearly with ``align_corners=False`` and NO antialiasing: ``fy = max((i+0.5)*h/H -
  0.5, 0)``, rows ``y0 = min(floor(fy), h-1)`` and ``min(y0+1, h-1)`` relative to the box (indices
  clamp at the box edge, the crop comes first), columns likewise from ``W-1-j`` when flipped; the
  taps are read at ``top + y``, ``left + x``.
* ``jitter = (brightness, contrast, saturation, hue)``: ``ColorJitter`` (torchvision's tensor
  path) on the [0, 1] values after ``/255``, with either geometry; the padding of the old
  geometry is black pixels of the image and takes part.  ``grey(v) = 0.299 r + 0.587 g + 0.114
  b``; brightness ``clamp(v*fb, 0, 1)``; contrast ``clamp(fc*v + (1-fc)*m, 0, 1)`` with ``m`` the
  mean of ``grey`` over the H x W image as it stands when contrast runs; saturation ``clamp(fs*v
  + (1-fs)*grey(v), 0, 1)``; hue RGB -> HSV, ``h <- (h + fh) mod 1``, HSV -> RGB.  ``fb, fc, fs ~
  U[max(0, 1-x), 1+x]``, ``fh ~ U[-hue, hue]``.  The four run in a per-slot order, one of 24
  (``jitter_order``); a strength of 0 skips that operation in place.

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
    rrc: Optional[Tuple[float, float, float, float]] = None     # scale lo, hi; ratio lo, hi
    jitter: Optional[Tuple[float, float, float, float]] = None  # brightness, contrast,
    #                                                             saturation, hue strengths

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
        if self.rrc is not None:
            if len(self.rrc) != 4:
                raise ValueError('AugmentRecipe: rrc is (scale_lo, scale_hi, ratio_lo, ratio_hi)')
            s(self, 'rrc', tuple(float(v) for v in self.rrc))
            clash = [n for n, on in (('resize', self.resize), ('pad', self.pad),
                                     ('degrees', self.degrees), ('scale', self.scale is not None))
                     if on]
            if clash:
                raise ValueError('AugmentRecipe: rrc replaces Resize, RandomCrop and RandomAffine; '
                                 'it cannot be combined with %s' % ', '.join(clash))
            slo, shi, rlo, rhi = self.rrc
            if not all(math.isfinite(v) for v in self.rrc) or not (0 < slo <= shi and
                                                                   0 < rlo <= rhi):
                raise ValueError('AugmentRecipe: rrc needs 0 < scale_lo <= scale_hi and '
                                 '0 < ratio_lo <= ratio_hi, got %r' % (self.rrc,))
        if self.jitter is not None:
            if len(self.jitter) != 4:
                raise ValueError('AugmentRecipe: jitter is (brightness, contrast, saturation, hue)')
            s(self, 'jitter', tuple(float(v) for v in self.jitter))
            if not all(math.isfinite(v) and v >= 0 for v in self.jitter):
                raise ValueError('AugmentRecipe: jitter strengths are >= 0, got %r'
                                 % (self.jitter,))
            if self.jitter[3] > 0.5:
                raise ValueError('AugmentRecipe: jitter hue lies in [0, 0.5], got %r'
                                 % self.jitter[3])
            if not any(self.jitter):
                s(self, 'jitter', None)

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
        order = [T.ToPILImage, T.Resize, T.RandomCrop, T.RandomResizedCrop,
                 T.RandomHorizontalFlip, T.RandomAffine, T.ColorJitter, T.ToTensor, T.Normalize,
                 T.Cutout]
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
            elif isinstance(tr, T.RandomResizedCrop):
                if 'crop' in kw:
                    raise ValueError('AugmentRecipe.from_transform: %r after a RandomCrop '
                                     '(RandomResizedCrop stands in the place of Resize and '
                                     'RandomCrop)' % (tr,))
                kw['crop'], kw['rrc'] = _pair(tr.size), tuple(tr.scale) + tuple(tr.ratio)
            elif isinstance(tr, T.ColorJitter):
                kw['jitter'] = (tr.brightness, tr.contrast, tr.saturation, tr.hue)
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
        ``32`` or ``24x32``, ``norm`` is ``cifar``, ``none`` or ``m0:m1:m2/s0:s1:s2``.  The
        photographic keys: ``rrc=0.08:1.0/0.75:1.3333`` (scale lo:hi / ratio lo:hi) and
        ``jitter=0.4:0.4:0.4:0.1`` (brightness:contrast:saturation:hue); ``none`` unsets either."""
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
            elif k == 'rrc':
                if v in ('', 'none'):
                    kw[k] = None
                    continue
                sc, sep, ra = v.partition('/')
                try:
                    kw[k] = tuple(float(x) for x in sc.split(':') + ra.split(':'))
                except ValueError:
                    kw[k] = ()
                if not sep or len(sc.split(':')) != 2 or len(kw[k]) != 4:
                    raise ValueError('AugmentRecipe.parse: rrc is scale_lo:scale_hi/ratio_lo:'
                                     'ratio_hi, got %r' % v)
            elif k == 'jitter':
                if v in ('', 'none'):
                    kw[k] = None
                    continue
                try:
                    kw[k] = tuple(float(x) for x in v.split(':'))
                except ValueError:
                    kw[k] = ()
                if len(kw[k]) != 4:
                    raise ValueError('AugmentRecipe.parse: jitter is brightness:contrast:'
                                     'saturation:hue, got %r' % v)
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
        if self.rrc is not None:
            out.append('rrc=%r:%r/%r:%r' % self.rrc)
        if self.jitter is not None:
            out.append('jitter=%r:%r:%r:%r' % self.jitter)
        return ','.join(out)

    # ---------------------------------------------------------------- geometry
    @property
    def out_hw(self):
        return self.crop

    @property
    def affine(self):
        return self.degrees != 0 or self.scale is not None

    @property
    def photo(self):
        """``rrc`` or ``jitter`` is set: the 16-float params row, ``PHOTO_PARAMS`` draws."""
        return self.rrc is not None or self.jitter is not None

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
        if self.rrc is not None:         # any box of any source resizes to the crop
            if min(H, W, Hs, Ws) < 1:
                raise ValueError('AugmentRecipe: empty crop %dx%d or source %dx%d'
                                 % (H, W, Hs, Ws))
            return
        if min(H, W, Hr, Wr) < 1 or Hr + 2 * self.pad < H or Wr + 2 * self.pad < W:
            raise ValueError('AugmentRecipe: crop %dx%d does not fit the %dx%d image (source '
                             '%dx%d, resize %d) with padding %d'
                             % (H, W, Hr, Wr, Hs, Ws, self.resize, self.pad))

    def is_legacy(self, Hs, Ws):
        """Crop-with-pad and flip on a shard of the output size: ``pool_build_kernel``'s case."""
        return (not self.resize and not self.affine and not self.cutout and not self.photo
                and self.crop == (Hs, Ws))

    def norm(self):
        return (self.mean or (0.0, 0.0, 0.0)), (self.std or (1.0, 1.0, 1.0))

    def fallback_box(self, Hs, Ws):
        """``(top, left, h, w)`` when all ten attempts fail, and with ``augment=False``: the
        whole image clipped to the ratio range, centred (torchvision's fallback)."""
        _, _, rlo, rhi = self.rrc
        h, w = Hs, Ws
        if Ws / Hs < rlo:
            h = min(max(int(round(Ws / rlo)), 1), Hs)
        elif Ws / Hs > rhi:
            w = min(max(int(round(Hs * rhi)), 1), Ws)
        return (Hs - h) // 2, (Ws - w) // 2, h, w

    @staticmethod
    def jitter_order(code):
        """The order of (0 brightness, 1 contrast, 2 saturation, 3 hue) that order code 0..23
        stands for, its Lehmer code: from [0, 1, 2, 3] take element ``code // 6``, then element
        ``code % 6 // 2`` of the rest, then element ``code % 2``, then what is left."""
        code = int(code)
        if not 0 <= code < 24:
            raise ValueError('jitter_order: code is 0..23, got %r' % code)
        rest = [0, 1, 2, 3]
        return [rest.pop(code // 6), rest.pop(code % 6 // 2), rest.pop(code % 2), rest[0]]

    def _jitter(self, x, params, info=None):
        """ColorJitter on [H][W][3] values in [0, 1] with the factors and the order code of
        ``params[10:15]`` (module docstring); the grey mean is this image's own."""
        f = [float(v) for v in params[10:14]]
        wts = torch.tensor([0.299, 0.587, 0.114], dtype=x.dtype)
        for op in self.jitter_order(params[14]):
            if not self.jitter[op]:
                continue
            if op == 0:
                x = (x * f[0]).clamp(0, 1)
            elif op == 1:
                m = (x * wts).sum(-1).mean()
                if info is not None:
                    info['grey_mean'] = float(m)
                x = (f[1] * x + (1 - f[1]) * m).clamp(0, 1)
            elif op == 2:
                x = (f[2] * x + (1 - f[2]) * (x * wts).sum(-1, keepdim=True)).clamp(0, 1)
            else:
                x = _adjust_hue(x, f[3])
        return x

    # ---------------------------------------------------------------- CPU reference
    def reference(self, img_u8, params, dtype=torch.float64, info=None):
        """The recipe on one HWC uint8 image with explicit draws ``params = (dy, dx, flip,
        angle_deg, scale, cut_y, cut_x)`` -> [H][W][3] ``dtype`` (module docstring).  A recipe
        with ``rrc`` or ``jitter`` takes the ``PHOTO_PARAMS`` form: ``[0..7]`` as above (``rrc``:
        top, left, flip, 0, 1, cut_y, cut_x, attempt), ``[8], [9]`` the box h, w, ``[10..13]``
        fb, fc, fs, fh, ``[14]`` the order code; ``[15]`` (the kernel's grey mean) is never read: the
        contrast step takes the mean of its own pixels, and leaves it in ``info['grey_mean']``
        when ``info`` is a dict."""
        src = torch.as_tensor(img_u8)
        if src.dim() != 3 or src.shape[2] != 3:
            raise ValueError('reference: image must be [H][W][3]')
        src = src.to(dtype)
        Hs, Ws = src.shape[:2]
        self.check(Hs, Ws)
        Hr, Wr = self.resized_hw(Hs, Ws)
        H, W = self.crop
        pad = self.pad
        if self.photo and len(params) != PHOTO_PARAMS:
            raise ValueError('reference: a recipe with rrc or jitter takes %d params, got %d'
                             % (PHOTO_PARAMS, len(params)))
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

        def box(i, j):                  # RandomResizedCrop: the resized box at (i, j)
            top, left, bh, bw = dy, dx, int(params[8]), int(params[9])
            if not (1 <= bh and 1 <= bw and 0 <= top and 0 <= left
                    and top + bh <= Hs and left + bw <= Ws):
                raise ValueError('reference: box %r leaves the %dx%d image'
                                 % ((top, left, bh, bw), Hs, Ws))
            jx = W - 1 - j if flip else j
            fy = ((i.to(dtype) + 0.5) * (bh / H) - 0.5).clamp(min=0)
            fx = ((jx.to(dtype) + 0.5) * (bw / W) - 0.5).clamp(min=0)
            y0 = fy.floor().long().clamp(max=bh - 1)
            x0 = fx.floor().long().clamp(max=bw - 1)
            y1, x1 = (y0 + 1).clamp(max=bh - 1), (x0 + 1).clamp(max=bw - 1)
            ly, lx = (fy - y0).unsqueeze(-1), (fx - x0).unsqueeze(-1)
            up = src[top + y0, left + x0] * (1 - lx) + src[top + y0, left + x1] * lx
            lo = src[top + y1, left + x0] * (1 - lx) + src[top + y1, left + x1] * lx
            return up * (1 - ly) + lo * ly

        i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
        if self.rrc is not None:
            v = box(i, j)
        elif self.affine:
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
        v = v / 255
        if self.jitter is not None:
            v = self._jitter(v, params, info)
        out = (v - torch.tensor(mean, dtype=dtype)) / torch.tensor(std, dtype=dtype)
        if self.cutout:
            h = self.cutout // 2
            y1, y2 = min(max(cut_y - h, 0), H), min(max(cut_y + h, 0), H)
            x1, x2 = min(max(cut_x - h, 0), W), min(max(cut_x + h, 0), W)
            out[y1:y2, x1:x2] = 0
        return out


def _adjust_hue(x, fh):
    """torchvision's ``adjust_hue`` on [..][3] RGB in [0, 1]: RGB -> HSV, ``h <- (h + fh) mod
    1``, HSV -> RGB (``_rgb2hsv`` / ``_hsv2rgb`` of its tensor path)."""
    r, g, b = x.unbind(-1)
    maxc, minc = x.max(-1).values, x.min(-1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    isr, isg = maxc == r, maxc == g
    h = torch.where(isr, bc - gc, torch.where(isg, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h / 6.0 + 1.0
    h = h - h.floor()
    h = h + fh
    h = h - h.floor()
    h6 = h * 6.0
    i = h6.floor()
    f = h6 - i
    i = i.long() % 6
    p = (maxc * (1.0 - s)).clamp(0, 1)
    q = (maxc * (1.0 - f * s)).clamp(0, 1)
    t = (maxc * (1.0 - s * (1.0 - f))).clamp(0, 1)
    pick = i.unsqueeze(-1)
    out = [torch.stack(a, -1).gather(-1, pick).squeeze(-1)
           for a in ((maxc, q, p, p, t, maxc), (t, maxc, maxc, q, p, p), (p, p, t, maxc, maxc, q))]
    return torch.stack(out, -1)


# ---------------------------------------------------------------------- spectrograms
SPEC_PARAMS = 12     # shift, gain, f0a, fwa, f0b, fwb, t0a, twa, t0b, twb, 0, 0
PHOTO_PARAMS = 16    # AugmentRecipe with rrc or jitter: dy|top, dx|left, flip, angle_deg, scale,
#                      cut_y, cut_x, attempt, box h, box w, fb, fc, fs, fh, order code, grey mean


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
