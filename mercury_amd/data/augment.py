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
``WaveRecipe`` is the recipe of raw waveforms: shift, gain and background noise on the clip, then
the log-spectrogram, run by ``pool_wave_kernel`` (fp32 MFMA DFT) from an int16 / float32 shard.
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


# ---------------------------------------------------------------------- waveforms
WAVE_PARAMS = 16     # shift, gain, noise_on, clip, off, vol, f0a, fwa, f0b, fwb, t0a, twa, t0b,
#                      twb, rq - 65536 (speed), 1 + rir (reverb on; else 0)
SPEED_NT, SPEED_PH, SPEED_BETA = 32, 64, 8.0    # taps, phases, Kaiser beta of the resampler
CMVN_VAR_FLOOR = 1e-5     # added to the biased variance of ``cmvn=2`` (csrc/kernels.h has its twin)
REVERB_K_MAX = 4096       # taps of a room impulse response (csrc/kernels.h has its twin)


def reverb_convolve(x, h):
    """``y[i] = sum_{k <= min(K - 1, i)} h[k] x[i - k]`` for ``0 <= i < L``: the clip ``x[L]``
    under the causal response ``h[K]``, the tail beyond L dropped.  fp64, a plain sum per
    output (a Toeplitz product, in blocks of rows)."""
    x, h = x.double(), h.double()
    L, K = x.shape[0], h.shape[0]
    rows = torch.cat([torch.zeros(K - 1, dtype=torch.float64), x]).unfold(0, K, 1)   # [L][K]
    hf = h.flip(0)
    step = max(1, (1 << 22) // K)
    return torch.cat([rows[i:i + step] @ hf for i in range(0, L, step)])


def speed_resample(xs, js, rq, table):
    """``xs[L]`` (fp64) read at the clip positions ``js`` (int64) through ``WaveRecipe``'s
    polyphase resampler at the 16.16 rate ``rq``: the kernel's positions bit for bit, ``table``
    its fp32 values (``speed_table``), the arithmetic in fp64."""
    L, NT = xs.shape[0], SPEED_NT
    c = L >> 1
    pos = (c << 16) + (js.long() - c) * int(rq)
    i0, frac = pos >> 16, pos & 0xffff
    p, mu = frac >> 10, (frac & 1023).double() / 1024
    h = table.double()
    w = h[p] + mu.view(-1, 1) * (h[p + 1] - h[p])                       # [n][NT]
    idx = i0.view(-1, 1) + torch.arange(NT) - (NT // 2 - 1)
    src = torch.where((idx >= 0) & (idx < L), xs[idx.clamp(0, L - 1)],
                      torch.zeros((), dtype=torch.float64))
    return (w * src).sum(1)


def _fpair(v, name, what='(lo, hi)'):
    if v is None:
        return None
    if len(v) != 2:
        raise ValueError('WaveRecipe: %s is %s' % (name, what))
    v = (float(v[0]), float(v[1]))
    if not all(math.isfinite(g) for g in v):
        raise ValueError('WaveRecipe: %s must be finite, got %r' % (name, v))
    return v


@dataclass(frozen=True)
class WaveRecipe:
    """Waveform augmentation and the log-spectrogram front end for raw clips ``x[0..L)``, run by
    ``pool_wave_kernel`` (``csrc/pool_wave.hip``) on an int16 or float32 shard [Ns][L] for a whole
    pool: ``ops.pool_build(..., recipe=r, noise=bank)``.  int16 PCM is read as ``x / 32768``,
    float32 as is (finite values only); the noise bank ``[Nn][Ln]``, ``Ln >= L``, has the
    shard's dtype.

    One pool slot, given its draws:

    1. ``xa[j] = gain * x[j - s]`` where ``0 <= j - s < L``, else 0; with noise on, then
       ``xa[j] = fma(vol, noise[clip][off + j], xa[j])`` -- fp32, one multiply and one FUSED
       multiply-add in the kernel (``reference`` does both in fp64, where the two agree);
    2. centre padding of ``xa`` by ``n_fft / 2`` on each side, reflected
       (``torch.stft(center=True, pad_mode='reflect')``), which needs ``L > n_fft / 2``;
    3. ``X[t][k] = sum_n w[n] xp[t*hop + n] exp(-2 pi i k n / W)``, ``w`` the periodic Hann
       window, ``t < T = 1 + L // hop`` frames, ``k < F = W/2 + 1`` bins;
    4. ``y[k][t] = a ln(re^2 + im^2 + eps) + b`` with ``a = 1/std``, ``b = -mean/std`` of ``norm``
       (1 and 0 without);
    5. ``fill`` (output units) where ``k`` lies in a frequency band or ``t`` in a time band,
       ``SpecRecipe``'s width and start formulas on (F, T);
    6. one rounding to bf16, channel 0 of the NHWC8 pixel (row k, column t); channels 1..7 +0.

    With ``mel = M > 0`` (``pool_wave_mel_kernel``, ``csrc/pool_mel.hip``) step 4 becomes
    ``mel[t][m] = sum_k (re^2 + im^2)[t][k] fb[k][m]``, ``lm = ln(mel + eps)``, ``y[m][t] = a lm +
    b``; ``fb`` is torchaudio's default bank (HTK scale ``mel(f) = 2595 log10(1 + f/700)``, no
    area normalisation): M + 2 points equally spaced in mel from ``mel(fmin)`` to ``mel(fmax)``
    map back to ``f_0..f_{M+1}`` Hz, the bins lie at ``g_k = k (sr/2) / (F-1)``, and ``fb[k][m] =
    max(0, min((g_k - f_m)/(f_{m+1} - f_m), (f_{m+2} - g_k)/(f_{m+2} - f_{m+1})))``.  A filter
    with no bin under it gives ``a ln(eps) + b``.  With ``dct = C > 0`` as well, ``c[t][j] = sum_m
    lm[t][m] D[m][j]``, ``D[m][j] = sqrt(2/M) cos(pi (m + 0.5) j / M)`` with column 0 scaled by
    ``sqrt(1/2)`` (orthonormal DCT-II), and ``y[j][t] = a c + b``.  The output has R = C, else
    M, else F rows; masks are drawn on (R, T), and a frequency mask with ``dct`` is refused.
    ``lifter = L >= 1`` (needs ``dct``) scales column j of D by ``1 + (L/2) sin(pi j / L)``, HTK's
    sinusoidal lifter.

    With ``delta = 1 | 2`` (needs ``mel``) and half-window ``dwin = N`` (1..4), let ``v[r][t]`` be
    the feature before the affine (``c`` or ``lm``).  ``d1[r][t] = sum_{n=1..N} n (v[r][clamp(t +
    n)] - v[r][clamp(t - n)]) / (2 sum_{n=1..N} n^2)``, ``clamp(u) = min(max(u, 0), T - 1)``
    (replicate padding, torchaudio's ``compute_deltas``); ``d2`` is the same operator on ``d1``.
    The output has ``(1 + delta) R`` rows: ``y[r] = a v[r] + b``, ``y[R + r] = a d1[r]``, ``y[2R +
    r] = a d2[r]`` (no ``b``).  Masks come last, drawn on (R, T) as without ``delta``: a time
    band fills every row, a frequency band of row f rows f, R + f and 2R + f; the differences
    are taken from the unmasked features.

    Draws, per pool slot (Philox on the image kernels' counter ``(gb, t)``, stream words
    0x5bec8..0x5becb of its own): ``s = r % (2*shift + 1) - shift``; ``gain = fma(hi - lo,
    u01(r), lo)``, one rounding; noise on iff ``u01(r) < p``, then ``clip = r % Nn``, ``off = r % (Ln - L + 1)``,
    ``vol = vol_max * u01(r)``; masks as ``SpecRecipe``.  ``augment=False`` draws the identity
    (no shift, gain 1, no noise, no masks), so evaluation still gets its spectrogram.

    ``speed = (LO, HI)``, ``0.5 <= LO <= HI <= 2`` (speed perturbation; off by default): the clip
    is resampled about its centre by a drawn rate, tempo and pitch together, and keeps its
    length -- what leaves the clip is lost, what enters from outside is zero.  The rate is the
    16.16 integer ``rq = rq_lo + r.x % (rq_hi - rq_lo + 1)``, ``rq_lo = round(LO * 65536)``,
    ``rq_hi = round(HI * 65536)``, ``r`` one more Philox word (stream 0x5becc); ``augment=False``
    gives 65536, and ``params[14] = rq - 65536``.  Step 1 becomes ``xa[j] = gain * xs(j - s)``
    (still 0 unless ``0 <= j - s < L``) with, for ``js = j - s`` and ``c = L >> 1``::

        pos = (c << 16) + (js - c) * rq            i0 = pos >> 16     frac = pos & 0xffff
        p = frac >> 10      mu = (frac & 1023) / 1024
        w_k = fma(mu, h[p + 1][k] - h[p][k], h[p][k])
        xs = sum_{k < 32} w_k x[i0 + k - 15]       (x = 0 outside [0, L), fmaf in ascending k)

    ``h = speed_table()``: 64 phases (and the wrap row) of a 32-tap Kaiser (beta 8) windowed
    sinc with cutoff ``0.45 / max(1, HI)`` cycles per source sample.  The noise bank is not
    resampled.  A slot with ``rq = 65536`` takes ``x[js]`` itself, unfiltered.

    ``cmvn = 1 | 2`` (needs ``mel``; off by default): cepstral mean (and variance) normalisation
    per utterance, over the clip's T frames, of the feature ``v`` above: ``mu_r = mean_t
    v[r][t]``, ``var_r = mean_t (v[r][t] - mu_r)^2`` (the biased variance, as Kaldi's
    ``apply-cmvn`` takes it), ``z = v - mu_r`` for ``cmvn=1`` and ``z = (v - mu_r) / sqrt(var_r +
    CMVN_VAR_FLOOR)`` for ``cmvn=2``.  Then ``y[r] = a z + b``, and the delta rows are the
    difference operator on ``z`` (no ``b``).  The statistics come from the unmasked fp32 features
    (``pool_cmvn_kernel``, ``csrc/pool_cmvn.hip``); masks still come last.  T = 1 gives ``z = 0``.

    ``preemph = C``, ``0 <= C < 1`` (off by default): Kaldi's per-frame pre-emphasis of each
    frame ``f[0..W)`` of the padded signal before the window, ``s[0] = f[0] - C f[0]``, ``s[n] =
    f[n] - C f[n-1]``.  It is linear in the frame, so it lives in ``table()`` alone.

    ``reverb = p``, ``0 < p <= 1`` (room-impulse reverberation; off by default), with a bank
    ``rir [Nr][K]``, float32, ``1 <= K <= 4096``: one more Philox word (stream 0x5becd) turns it
    on iff ``u01(r.x) < p`` and picks the response ``h = rir[r.y % Nr]``; ``params[15] = 1 + rir``
    when on, else 0, and ``augment=False`` draws it off.  Step 0, before everything else:
    ``xr[i] = sum_{k <= min(K - 1, i)} h[k] x[i - k]`` for ``0 <= i < L`` in fp32 (an int16 clip
    as ``x / 32768`` first); the tail beyond L is lost.  Speed, shift, gain, the noise mix and
    all later steps then run on ``xr`` in place of ``x``: a reverberant recording that is then
    perturbed, so under ``speed`` the room is resampled with the speech.  Rows are used as
    given: causal, ``h[0]`` the first tap, no normalisation, no peak alignment, finite values;
    shorter responses are zero-padded by the user.  A slot that drew it off uses the clip itself
    (``pool_reverb_kernel``, ``csrc/pool_reverb.hip``)."""
    n_fft: int = 200
    hop: int = 100
    shift: int = 0                                  # maximum shift in samples
    gain: Optional[Tuple[float, float]] = None      # (lo, hi)
    noise: Optional[Tuple[float, float]] = None     # (p, vol_max)
    eps: float = 1e-6
    norm: Optional[Tuple[float, float]] = None      # (mean, std) of the log power
    fmask: Tuple[int, int] = (0, 0)
    tmask: Tuple[int, int] = (0, 0)
    fill: float = 0.0
    mel: int = 0                                    # mel bands (0: the linear bins)
    sr: int = 16000                                 # sample rate, Hz (mel only)
    fmin: float = 0.0
    fmax: Optional[float] = None                    # None: sr / 2
    dct: int = 0                                    # cepstral coefficients kept (0: log-mel)
    delta: int = 0                                  # order of the time differences appended
    dwin: int = 2                                   # their half-window N, frames
    lifter: int = 0                                 # HTK sinusoidal lifter L (0: off)
    speed: Optional[Tuple[float, float]] = None     # (lo, hi) resampling rate (None: off)
    cmvn: int = 0                                   # 1: mean, 2: mean and variance, per clip
    preemph: float = 0.0                            # pre-emphasis coefficient C (0: off)
    reverb: float = 0.0                             # probability of a room response (0: off)

    def __post_init__(self):
        s = object.__setattr__
        for k in ('n_fft', 'hop', 'shift', 'mel', 'sr', 'dct', 'delta', 'dwin', 'lifter', 'cmvn'):
            s(self, k, int(getattr(self, k)))
        s(self, 'preemph', float(self.preemph))
        s(self, 'reverb', float(self.reverb))
        s(self, 'fmin', float(self.fmin))
        s(self, 'fmax', None if self.fmax is None else float(self.fmax))
        s(self, 'fmask', _mask(self.fmask, 'fmask'))
        s(self, 'tmask', _mask(self.tmask, 'tmask'))
        s(self, 'fill', float(self.fill))
        s(self, 'eps', float(self.eps))
        s(self, 'gain', _fpair(self.gain, 'gain'))
        s(self, 'noise', _fpair(self.noise, 'noise', '(p, vol_max)'))
        s(self, 'norm', _fpair(self.norm, 'norm', '(mean, std)'))
        s(self, 'speed', _fpair(self.speed, 'speed'))
        if self.n_fft % 2 or not 16 <= self.n_fft <= 512:
            raise ValueError('WaveRecipe: n_fft is even, 16..512, got %d' % self.n_fft)
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError('WaveRecipe: hop is 1..n_fft, got %d' % self.hop)
        if self.shift < 0:
            raise ValueError('WaveRecipe: shift is >= 0, got %d' % self.shift)
        if self.gain is not None and self.gain[0] > self.gain[1]:
            raise ValueError('WaveRecipe: gain is (lo, hi), lo <= hi, got %r' % (self.gain,))
        if self.noise is not None and not (0 <= self.noise[0] <= 1 and self.noise[1] >= 0):
            raise ValueError('WaveRecipe: noise is (p, vol_max), 0 <= p <= 1, vol_max >= 0, '
                             'got %r' % (self.noise,))
        if not (self.eps > 0 and math.isfinite(self.eps)):
            raise ValueError('WaveRecipe: eps is > 0, got %r' % self.eps)
        if self.norm is not None and not self.norm[1] > 0:
            raise ValueError('WaveRecipe: norm is (mean, std), std > 0, got %r' % (self.norm,))
        if not math.isfinite(self.fill):
            raise ValueError('WaveRecipe: fill is finite, got %r' % self.fill)
        if self.mel and not 8 <= self.mel <= 128:
            raise ValueError('WaveRecipe: mel is 0 or 8..128, got %d' % self.mel)
        if self.sr < 1:
            raise ValueError('WaveRecipe: sr is positive, got %d' % self.sr)
        top = self.sr / 2 if self.fmax is None else self.fmax
        if not 0 <= self.fmin < top:
            raise ValueError('WaveRecipe: fmin is 0 <= fmin < fmax, got %r (fmax %r)'
                             % (self.fmin, top))
        if not top <= self.sr / 2:
            raise ValueError('WaveRecipe: fmax is at most sr/2 = %r, got %r' % (self.sr / 2, top))
        if not 0 <= self.dct <= self.mel:
            raise ValueError('WaveRecipe: dct is 0..mel (and needs mel > 0), got dct = %d, '
                             'mel = %d' % (self.dct, self.mel))
        if self.dct and self.fmask[0] > 0:
            raise ValueError('WaveRecipe: fmask with dct (bands of cepstral coefficients) is '
                             'refused, got fmask = %r' % (self.fmask,))
        if not 0 <= self.delta <= 2:
            raise ValueError('WaveRecipe: delta is 0, 1 or 2, got %d' % self.delta)
        if self.delta and not self.mel:
            raise ValueError('WaveRecipe: delta needs mel > 0 (no delta rows on the linear bins)')
        if not 1 <= self.dwin <= 4:
            raise ValueError('WaveRecipe: dwin is 1..4, got %d' % self.dwin)
        if self.lifter < 0 or (self.lifter and not self.dct):
            raise ValueError('WaveRecipe: lifter is >= 0 and needs dct > 0, got lifter = %d, '
                             'dct = %d' % (self.lifter, self.dct))
        if self.speed is not None and not 0.5 <= self.speed[0] <= self.speed[1] <= 2.0:
            raise ValueError('WaveRecipe: speed is (lo, hi), 0.5 <= lo <= hi <= 2, got %r'
                             % (self.speed,))
        if not 0 <= self.cmvn <= 2:
            raise ValueError('WaveRecipe: cmvn is 0, 1 or 2, got %d' % self.cmvn)
        if self.cmvn and not self.mel:
            raise ValueError('WaveRecipe: cmvn needs mel > 0 (no CMVN on the linear bins)')
        if not 0 <= self.preemph < 1:
            raise ValueError('WaveRecipe: preemph is 0 <= C < 1, got %r' % self.preemph)
        if not 0 <= self.reverb <= 1:
            raise ValueError('WaveRecipe: reverb is a probability 0 < p <= 1 (0: off), got %r'
                             % self.reverb)

    @classmethod
    def parse(cls, spec):
        """``wave:nfft=200,hop=100,shift=1600,gain=0.8:1.2,noise=0.8x0.1,eps=1e-6,norm=-5:4,
        fmask=2x10,tmask=2x20,fill=0,mel=80,sr=16000,fmin=0,fmax=8000,dct=13,delta=2,dwin=2,
        lifter=22,speed=0.9:1.1,cmvn=2,preemph=0.97,reverb=0.5`` (the ``wave:`` prefix is optional here)."""
        spec = spec.strip()
        if spec.startswith('wave:'):
            spec = spec[5:]
        kw = {}
        for item in (spec.split(',') if spec else []):
            if '=' not in item:
                raise ValueError('WaveRecipe.parse: %r is not name=value' % item)
            k, v = (s.strip() for s in item.split('=', 1))
            if k in ('nfft', 'hop', 'shift', 'mel', 'sr', 'dct', 'delta', 'dwin', 'lifter',
                     'cmvn'):
                kw['n_fft' if k == 'nfft' else k] = int(v)
            elif k in ('fmask', 'tmask', 'noise'):
                nm = v.split('x')
                if k == 'noise' and v in ('', 'none'):
                    kw[k] = None
                elif len(nm) != 2:
                    raise ValueError('WaveRecipe.parse: %s is AxB, got %r' % (k, v))
                else:
                    kw[k] = (float(nm[0]), float(nm[1])) if k == 'noise' else \
                        (int(nm[0]), int(nm[1]))
            elif k in ('gain', 'norm', 'speed'):
                g = v.split(':')
                if v in ('', 'none'):
                    kw[k] = None
                elif len(g) != 2:
                    raise ValueError('WaveRecipe.parse: %s is A:B, got %r' % (k, v))
                else:
                    kw[k] = (float(g[0]), float(g[1]))
            elif k in ('fill', 'eps', 'fmin', 'preemph', 'reverb'):
                kw[k] = float(v)
            elif k == 'fmax':
                kw[k] = None if v in ('', 'none') else float(v)
            else:
                raise ValueError('WaveRecipe.parse: unknown key %r' % k)
        return cls(**kw)

    def spec(self):
        """The ``parse`` form of this recipe, with the ``wave:`` prefix."""
        out = ['nfft=%d' % self.n_fft, 'hop=%d' % self.hop, 'shift=%d' % self.shift]
        if self.gain is not None:
            out.append('gain=%r:%r' % self.gain)
        if self.noise is not None:
            out.append('noise=%rx%r' % self.noise)
        out.append('eps=%r' % self.eps)
        if self.norm is not None:
            out.append('norm=%r:%r' % self.norm)
        out += ['fmask=%dx%d' % self.fmask, 'tmask=%dx%d' % self.tmask, 'fill=%r' % self.fill]
        if self.mel:
            out += ['mel=%d' % self.mel, 'sr=%d' % self.sr, 'fmin=%r' % self.fmin]
            if self.fmax is not None:
                out.append('fmax=%r' % self.fmax)
            out.append('dct=%d' % self.dct)
        if self.delta:
            out.append('delta=%d' % self.delta)
        if self.delta or self.dwin != 2:
            out.append('dwin=%d' % self.dwin)
        if self.lifter:
            out.append('lifter=%d' % self.lifter)
        if self.speed is not None:
            out.append('speed=%r:%r' % self.speed)
        if self.cmvn:
            out.append('cmvn=%d' % self.cmvn)
        if self.preemph:
            out.append('preemph=%r' % self.preemph)
        if self.reverb:
            out.append('reverb=%r' % self.reverb)
        return 'wave:' + ','.join(out)

    @property
    def identity(self):
        """No augmentation on: every draw is the identity whatever the random words."""
        return (self.shift == 0 and self.gain is None and self.noise is None
                and 0 in self.fmask and 0 in self.tmask
                and self.speed_rq() in (None, (65536, 65536)) and not self.reverb)

    def out_hw(self, L):
        """(R, T): rows and frames of an L-sample clip, the network's input size.  R is ``dct``
        if set, else ``mel`` if set, else the F = n_fft/2 + 1 bins; with ``delta`` the output has
        ``(1 + delta) * R`` rows."""
        return (1 + self.delta) * self.feat_rows, 1 + L // self.hop

    @property
    def feat_rows(self):
        """R: the rows of one feature block, on which the frequency masks are drawn."""
        return self.dct or self.mel or self.n_fft // 2 + 1

    def affine(self):
        """(a, b) of ``y = a ln(power + eps) + b``."""
        return (1.0, 0.0) if self.norm is None else (1.0 / self.norm[1],
                                                     -self.norm[0] / self.norm[1])

    def check(self, L, noise_shape=None, rir_shape=None):
        """Raise unless the recipe fits L-sample clips, a noise bank of shape (Nn, Ln) and an
        RIR bank of shape (Nr, K) (``None``: no bank); names the field that does not."""
        if self.reverb and rir_shape is None:
            raise ValueError('WaveRecipe: reverb=%r needs an RIR bank [Nr][K]' % self.reverb)
        if rir_shape is not None:
            if not self.reverb:
                raise ValueError('WaveRecipe: an RIR bank needs reverb=p')
            if len(rir_shape) != 2 or rir_shape[0] < 1 or not 1 <= rir_shape[1] <= REVERB_K_MAX:
                raise ValueError('WaveRecipe: RIR bank must be [Nr >= 1][1 <= K <= %d], got %s'
                                 % (REVERB_K_MAX, tuple(rir_shape)))
        if L <= self.n_fft // 2:
            raise ValueError('WaveRecipe: n_fft %d needs clips longer than n_fft/2, got L = %d'
                             % (self.n_fft, L))
        F, T = self.feat_rows, self.out_hw(L)[1]
        if self.fmask[1] > F:
            raise ValueError('WaveRecipe: fmask width %d exceeds the %d rows'
                             % (self.fmask[1], F))
        if self.tmask[1] > T:
            raise ValueError('WaveRecipe: tmask width %d exceeds T = %d' % (self.tmask[1], T))
        if self.noise is not None and noise_shape is None:
            raise ValueError('WaveRecipe: noise=%r needs a noise bank [Nn][Ln]' % (self.noise,))
        if noise_shape is not None and (len(noise_shape) != 2 or noise_shape[0] < 1
                                        or noise_shape[1] < L):
            raise ValueError('WaveRecipe: noise bank must be [Nn >= 1][Ln >= L = %d], got %s'
                             % (L, tuple(noise_shape)))

    def draw(self, L, noise_shape=None, generator=None, rir_shape=None):
        """One slot's draws from torch's RNG, in the kernel's ranges and ``params`` layout."""
        self.check(L, noise_shape, rir_shape)

        def ri(n):
            return int(torch.randint(0, n, (1,), generator=generator).item())

        def ru():
            return float(torch.rand(1, generator=generator).item())
        p = [0.0] * WAVE_PARAMS
        p[0] = float(ri(2 * self.shift + 1) - self.shift)
        p[1] = 1.0
        if self.gain is not None:
            p[1] = self.gain[0] + (self.gain[1] - self.gain[0]) * ru()
        if self.noise is not None and ru() < self.noise[0]:
            p[2:6] = [1.0, float(ri(noise_shape[0])), float(ri(noise_shape[1] - L + 1)),
                      self.noise[1] * ru()]
        F, T = self.feat_rows, self.out_hw(L)[1]
        for base, (n, mx), size in ((6, self.fmask, F), (10, self.tmask, T)):
            for k in range(n):
                w = ri(mx + 1)
                p[base + 2 * k], p[base + 2 * k + 1] = float(ri(size - w + 1)), float(w)
        if self.speed is not None:
            lo, hi = self.speed_rq()
            p[14] = float(lo + ri(hi - lo + 1) - 65536)
        if self.reverb and ru() < self.reverb:
            p[15] = float(1 + ri(rir_shape[0]))
        return p

    def identity_params(self):
        p = [0.0] * WAVE_PARAMS
        p[1] = 1.0
        return p

    def table(self, ksteps=None):
        """The window-folded DFT table of the kernel, fp64 -> fp32 [4*ksteps][2*F16]: columns
        ``[0, F)`` hold ``w[n] cos(2 pi k n / W)``, columns ``[F16, F16 + F)`` hold
        ``-w[n] sin(2 pi k n / W)``; rows ``>= W`` and the padding columns are zero.  With
        ``preemph = C`` row ``n <= W - 2`` is ``w[n] E[n] - C w[n+1] E[n+1]`` (``E`` the cos / -sin
        pair), row ``W - 1`` stays and row 0 loses ``C w[0] E[0]`` as well: the DFT of the
        pre-emphasised frame as one product with the frame itself, folded in fp64."""
        W, F = self.n_fft, self.n_fft // 2 + 1
        F16 = (F + 15) // 16 * 16
        rows = 4 * ksteps if ksteps else W
        n = torch.arange(W, dtype=torch.float64).view(W, 1)
        k = torch.arange(F, dtype=torch.float64).view(1, F)
        w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / W)
        ang = 2 * math.pi * ((n * k) % W) / W
        tab = torch.zeros(rows, 2 * F16, dtype=torch.float64)
        tab[:W, :F] = w * torch.cos(ang)
        tab[:W, F16:F16 + F] = -w * torch.sin(ang)
        if self.preemph:
            first = tab[0].clone()
            tab[:W - 1] -= self.preemph * tab[1:W].clone()
            tab[0] -= self.preemph * first
        return tab.to(torch.float32)

    def speed_rq(self):
        """``(rq_lo, rq_hi)``, the 16.16 bounds of the drawn rate, or None with ``speed`` off."""
        if self.speed is None:
            return None
        return int(round(self.speed[0] * 65536)), int(round(self.speed[1] * 65536))

    def speed_table(self):
        """The resampler's filter, fp64 -> fp32 ``h[PH + 1][NT]``: ``h[p][k] = 2 fc sinc(2 fc u)
        I0(beta sqrt(1 - (u / (NT/2))^2)) / I0(beta)``, ``u = k - (NT/2 - 1) - p / PH``, zero for
        ``|u| > NT/2``, ``fc = 0.45 / max(1, HI)``.  Row ``PH`` is row 0 one tap on, so the phase
        interpolation never wraps.  Not renormalised (DC gain 1.00002 to 1.00004)."""
        if self.speed is None:
            raise ValueError('speed_table: the recipe has no speed')
        NT, PH = SPEED_NT, SPEED_PH
        fc = 0.45 / max(1.0, self.speed[1])
        k = torch.arange(NT, dtype=torch.float64).view(1, NT)
        p = torch.arange(PH + 1, dtype=torch.float64).view(PH + 1, 1)
        u = k - (NT // 2 - 1) - p / PH
        r = (1.0 - (u / (NT // 2)) ** 2).clamp(min=0.0).sqrt()
        i0b = torch.special.i0(torch.tensor(SPEED_BETA, dtype=torch.float64))
        h = 2 * fc * torch.sinc(2 * fc * u) * torch.special.i0(SPEED_BETA * r) / i0b
        return torch.where(u.abs() > NT // 2, torch.zeros_like(h), h).to(torch.float32)

    def _mel_fb(self):
        """fp64 [F][M]: the triangular HTK filter bank of the class docstring."""
        F, M = self.n_fft // 2 + 1, self.mel

        def to_mel(f):
            return 2595.0 * math.log10(1.0 + f / 700.0)
        top = self.sr / 2 if self.fmax is None else self.fmax
        pts = torch.linspace(to_mel(self.fmin), to_mel(top), M + 2, dtype=torch.float64)
        f = 700.0 * (10.0 ** (pts / 2595.0) - 1.0)                       # [M + 2] Hz
        g = torch.arange(F, dtype=torch.float64).view(F, 1) * (self.sr / 2) / (F - 1)
        up = (g - f[:M]) / (f[1:M + 1] - f[:M])
        down = (f[2:] - g) / (f[2:] - f[1:M + 1])
        return torch.minimum(up, down).clamp_(min=0.0)

    def _dct_mat(self):
        """fp64 [M][dct]: the first ``dct`` columns of the orthonormal DCT-II, column j scaled by
        the lifter ``1 + (L/2) sin(pi j / L)`` when ``lifter = L`` is set."""
        M = self.mel
        m = torch.arange(M, dtype=torch.float64).view(M, 1)
        j = torch.arange(self.dct, dtype=torch.float64).view(1, self.dct)
        D = math.sqrt(2.0 / M) * torch.cos(math.pi * (m + 0.5) * j / M)
        D[:, 0] *= math.sqrt(0.5)
        if self.lifter:
            D = D * (1.0 + 0.5 * self.lifter * torch.sin(math.pi * j / self.lifter))
        return D

    def _deltas(self, v):
        """fp64 [R][T] -> the time difference of the class docstring along T (replicate ends)."""
        N, T = self.dwin, v.shape[1]
        t = torch.arange(T)
        d = torch.zeros_like(v)
        for n in range(1, N + 1):
            d += n * (v[:, (t + n).clamp(max=T - 1)] - v[:, (t - n).clamp(min=0)])
        return d / (2.0 * sum(n * n for n in range(1, N + 1)))

    def mel_table(self):
        """The kernel's filter bank, fp64 -> fp32 [F16][M16], zero padding rows and columns."""
        if not self.mel:
            raise ValueError('mel_table: the recipe has mel = 0')
        F = self.n_fft // 2 + 1
        tab = torch.zeros((F + 15) // 16 * 16, (self.mel + 15) // 16 * 16, dtype=torch.float64)
        tab[:F, :self.mel] = self._mel_fb()
        return tab.to(torch.float32)

    def dct_table(self):
        """The kernel's DCT, fp64 -> fp32 [M16][C16]; rows ``>= mel`` are zero (the padded mel
        columns hold ``ln(eps)``, not 0) and so are the padding columns."""
        if not self.dct:
            raise ValueError('dct_table: the recipe has dct = 0')
        tab = torch.zeros((self.mel + 15) // 16 * 16, (self.dct + 15) // 16 * 16,
                          dtype=torch.float64)
        tab[:self.mel, :self.dct] = self._dct_mat()
        return tab.to(torch.float32)

    def mel_ksteps(self):
        """Per tile of 16 mel bands, the first and last step of 4 bins in which ``mel_table``
        holds a nonzero: a flat list (first, last, first, last, ...), the kernel's K ranges.  A
        tile of empty filters gets (0, -1)."""
        tab = self.mel_table()
        out = []
        for m0 in range(0, tab.shape[1], 16):
            rows = torch.nonzero(tab[:, m0:m0 + 16].abs().sum(1))
            out += [int(rows.min()) // 4, int(rows.max()) // 4] if len(rows) else [0, -1]
        return out

    # ---------------------------------------------------------------- CPU reference
    def reference(self, x, noise, params, dtype=torch.bfloat16, rir=None):
        """The recipe on one clip ``x[L]`` (int16 or float) with explicit draws ``params``
        (``WAVE_PARAMS`` values, the kernel's layout), the noise bank ``noise`` ([Nn][Ln] or
        None) and the RIR bank ``rir`` ([Nr][K] or None) -> [R][T][8] ``dtype``, the pool's layout
        (``out_hw``).  fp64 from step 0 on, then one rounding to ``dtype``."""
        def f64(t):
            t = torch.as_tensor(t)
            return t.double() / 32768 if t.dtype == torch.int16 else t.double()
        x = torch.as_tensor(x)
        if x.dim() != 1:
            raise ValueError('reference: the clip must be [L]')
        L, W, hop = x.shape[0], self.n_fft, self.hop
        self.check(L, None if noise is None else tuple(noise.shape),
                   None if rir is None else tuple(rir.shape))
        p = [float(v) for v in params]
        if len(p) != WAVE_PARAMS:
            raise ValueError('reference: params has %d values' % WAVE_PARAMS)
        s = int(p[0])
        j = torch.arange(L)
        xs = f64(x)
        if p[15]:         # step 0: the clip under response 1 + rir, the tail beyond L dropped
            if rir is None:
                raise ValueError('reference: params has reverb on but there is no RIR bank')
            xs = reverb_convolve(xs, torch.as_tensor(rir)[int(p[15]) - 1])
        if p[14]:         # the clip at rate rq; rq = 65536 is x[js] itself, as in the kernel
            if self.speed is None:
                raise ValueError('reference: params has a rate but the recipe has no speed')
            xs = speed_resample(xs, j, 65536 + int(p[14]), self.speed_table())
        xa = p[1] * torch.where((j - s >= 0) & (j - s < L), xs[(j - s).clamp(0, L - 1)],
                                torch.zeros((), dtype=torch.float64))
        if int(p[2]):
            if noise is None:
                raise ValueError('reference: params has noise on but there is no bank')
            clip, off = int(p[3]), int(p[4])
            xa = xa + p[5] * f64(noise[clip, off:off + L])
        h = W // 2
        xp = torch.cat([xa[1:h + 1].flip(0), xa, xa[L - h - 1:L - 1].flip(0)])
        F, T = self.feat_rows, self.out_hw(L)[1]   # (rows of one feature block)
        n = torch.arange(W, dtype=torch.float64).view(W, 1)
        k = torch.arange(W // 2 + 1, dtype=torch.float64).view(1, W // 2 + 1)
        w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / W)
        ang = 2 * math.pi * ((n * k) % W) / W
        frames = xp.unfold(0, W, hop)[:T]                               # [T][W]
        if self.preemph:
            frames = frames - self.preemph * torch.cat([frames[:, :1], frames[:, :-1]], 1)
        re, im = frames @ (w * torch.cos(ang)), frames @ (-w * torch.sin(ang))
        a, b = self.affine()
        if self.mel:
            y = torch.log((re * re + im * im) @ self._mel_fb() + self.eps)     # [T][M]
            if self.dct:
                y = y @ self._dct_mat()
            if self.cmvn:                           # per row over the clip's frames
                y = y - y.mean(0, keepdim=True)
                if self.cmvn == 2:
                    y = y / (y * y).mean(0, keepdim=True).add(CMVN_VAR_FLOOR).sqrt()
            d, y = y.t(), (a * y + b).t()                               # [R][T]
            for _ in range(self.delta):             # differences of the unmasked feature: no b
                d = self._deltas(d)
                y = torch.cat([y, a * d])
        else:
            y = (a * torch.log(re * re + im * im + self.eps) + b).t()   # [F][T]
        f = torch.arange(F).view(F, 1)
        t = torch.arange(T).view(1, T)
        masked = torch.zeros(F, T, dtype=torch.bool)
        for q in (6, 8):
            masked |= (f >= int(p[q])) & (f < int(p[q]) + int(p[q + 1]))
        for q in (10, 12):
            masked |= (t >= int(p[q])) & (t < int(p[q]) + int(p[q + 1]))
        masked = masked.repeat(1 + self.delta, 1)   # a band of row f covers rows f, R + f, 2R + f
        y = torch.where(masked, torch.tensor(self.fill, dtype=torch.float64), y)
        out = torch.zeros(y.shape[0], T, 8, dtype=dtype)
        out[:, :, 0] = y.to(dtype)
        return out
