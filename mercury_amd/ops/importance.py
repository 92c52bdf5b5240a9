"""Importance-sampling kernels front-end (``csrc/importance.hip``, ``csrc/pool_recipe.hip``)."""
from __future__ import annotations

import torch

from . import _chk, lib, ptr, stream_ptr
from ..data.augment import PHOTO_PARAMS, SPEC_PARAMS, SpecRecipe
from ..data.transforms import CIFAR_MEAN, CIFAR_STD


def pool_build(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed, pad=4,
               flip=True, augment=True, mean=CIFAR_MEAN, std=CIFAR_STD, shuffle=True, zero=None,
               recipe=None, params=None, force_augment_kernel=False):
    """Build a P-sample presample pool on device from either the uint8 image shard
    [Ns][H][W][3] (crop/flip/normalise on the fly) or a pre-converted bf16 shard
    [Ns][H][W][8] (non-image inputs: plain gather, no augmentation).  ``zero``: an fp32
    buffer the same launch zeroes (the scoring pass's BN-statistics arena).

    ``recipe`` (``data.augment.AugmentRecipe``) replaces pad / flip / mean / std by its own
    pipeline on a uint8 shard [Ns][Hs][Ws][3] of any size the recipe's crop fits; the pool is
    [P][h][w][8] for its crop (h, w).  A crop-and-flip recipe on a shard of the output size
    runs the kernel above; ``force_augment_kernel`` sends it through ``pool_recipe_kernel``
    like every other recipe (same bits).  ``params``: an fp32 [P][8] buffer that receives each
    slot's draws (dy, dx, flip, angle_deg, scale, cut_y, cut_x, 0).  A recipe with ``rrc`` or
    ``jitter`` (RandomResizedCrop, ColorJitter) dumps fp32 [P][16]
    (``data.augment.PHOTO_PARAMS``).

    A ``data.augment.SpecRecipe`` (time shift, gain, frequency / time masks) takes a PLANAR bf16
    shard [Ns][C][H][W], C <= 8, and a 4-d pool [P][H][W][8] (``pool_spec_kernel``); ``params``
    is then fp32 [P][12] (shift, gain, f0a, fwa, f0b, fwb, t0a, twa, t0b, twb, 0, 0).  With
    ``augment=False``, or ``SpecRecipe()``, the pool has the bits of the plain gather from the
    same samples' NHWC8 shard."""
    _chk(labels, torch.int64, 'labels')
    if isinstance(recipe, SpecRecipe):
        if force_augment_kernel:
            raise ValueError('force_augment_kernel belongs to an AugmentRecipe')
        return _pool_spec(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed,
                          augment, shuffle, zero, recipe, params)
    prebuilt = shard.dtype == torch.bfloat16
    if recipe is not None:
        if prebuilt:
            raise ValueError('an augmentation recipe needs the uint8 image shard, not a '
                             'pre-converted bf16 one')
        _chk(shard, torch.uint8, 'shard')
        if shard.dim() != 4 or shard.shape[-1] != 3:
            raise ValueError('uint8 shard must be [Ns][Hs][Ws][3]')
        Ns, Hs, Ws, _ = shard.shape
        recipe = recipe.with_crop((Hs, Ws))
        recipe.check(Hs, Ws)
        pad, flip = recipe.pad, recipe.flip
        mean, std = recipe.norm()
        if recipe.photo and force_augment_kernel:
            raise ValueError('force_augment_kernel: a recipe with rrc or jitter has a kernel '
                             'of its own')
        if (recipe.photo or params is not None or force_augment_kernel
                or not recipe.is_legacy(Hs, Ws)):
            return _pool_recipe(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed,
                                augment, shuffle, zero, recipe, params)
    elif params is not None or force_augment_kernel:
        raise ValueError('params / force_augment_kernel need a recipe')
    if not prebuilt:
        _chk(shard, torch.uint8, 'shard')
    elif shard.shape[-1] != 8:
        raise ValueError('pre-converted shard must be NHWC bf16 with 8 channels (a planar '
                         '[Ns][C][H][W] shard needs a SpecRecipe), got %s' % (tuple(shard.shape),))
    Ns, H, W, _ = shard.shape
    _chk(pool, torch.bfloat16, 'pool', P * H * W * 8)
    lib().pool_build(ptr(shard), ptr(labels), ptr(ctrl), ptr(pool), ptr(pool_label),
                     ptr(pool_index), Ns, H, W, P, batch, pad, int(flip), int(augment), int(shuffle),
                     int(seed) & 0xffffffff, list(mean), [1.0 / s for s in std], stream_ptr(),
                     int(prebuilt), ptr(zero), zero.numel() if zero is not None else 0)


def _pool_recipe(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed, augment,
                 shuffle, zero, recipe, params):
    """An ``AugmentRecipe`` through ``pool_recipe_kernel`` (``csrc/pool_recipe.hip``); ``params``
    is fp32 [P][16] with ``rrc`` or ``jitter``, else [P][8] (``AugmentRecipe.reference``'s
    layouts)."""
    Ns, Hs, Ws, _ = shard.shape
    H, W = recipe.out_hw
    Hr, Wr = recipe.resized_hw(Hs, Ws)
    lo, hi = recipe.scale or (1.0, 1.0)
    mean, std = recipe.norm()
    _chk(pool, torch.bfloat16, 'pool', P * H * W * 8)
    if params is not None:
        _chk(params, torch.float32, 'params', P * (PHOTO_PARAMS if recipe.photo else 8))
    lib().pool_recipe(shard=ptr(shard), labels=ptr(labels), ctrl=ptr(ctrl), pool=ptr(pool),
                      pool_label=ptr(pool_label), pool_index=ptr(pool_index), params=ptr(params),
                      params_floats=params.numel() if params is not None else 0, zero=ptr(zero),
                      nzero=zero.numel() if zero is not None else 0, stream=stream_ptr(), Ns=Ns,
                      Hs=Hs, Ws=Ws, H=H, W=W, P=P, batch=batch, augment=int(augment),
                      shuffle=int(shuffle), seed=int(seed) & 0xffffffff, flip=int(recipe.flip),
                      mean=list(mean), inv_std=[1.0 / s for s in std], cutout=recipe.cutout,
                      rrc=list(recipe.rrc or ()), jitter=list(recipe.jitter or (0.0,) * 4),
                      pad=recipe.pad, resize=recipe.resize, Hr=Hr, Wr=Wr, degrees=recipe.degrees,
                      scale_lo=lo, scale_hi=hi, affine=int(recipe.affine))


def _pool_spec(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed, augment,
               shuffle, zero, recipe, params, chunks=0):
    if shard.dtype == torch.uint8:
        raise ValueError('shard is uint8: a SpecRecipe needs the planar bf16 shard '
                         '[Ns][C][H][W] (uint8 image shards take an AugmentRecipe)')
    _chk(shard, torch.bfloat16, 'shard')
    if pool.dim() != 4 or pool.shape[3] != 8:
        raise ValueError('pool must be [P][H][W][8] for a SpecRecipe, got %s'
                         % (tuple(pool.shape),))
    H, W = int(pool.shape[1]), int(pool.shape[2])
    if shard.dim() != 4 or tuple(shard.shape[2:]) != (H, W) or not 1 <= shard.shape[1] <= 8:
        raise ValueError('shard is %s: a SpecRecipe needs the planar bf16 shard [Ns][C][%d][%d] '
                         'with C <= 8, not an NHWC8 pre-converted one'
                         % (tuple(shard.shape), H, W))
    Ns, C = int(shard.shape[0]), int(shard.shape[1])
    recipe.check(C, H, W)
    _chk(pool, torch.bfloat16, 'pool', P * H * W * 8)
    if params is not None:
        _chk(params, torch.float32, 'params', P * SPEC_PARAMS)
    lo, hi = recipe.gain or (1.0, 1.0)
    lib().pool_spec(ptr(shard), ptr(labels), ptr(ctrl), ptr(pool), ptr(pool_label),
                    ptr(pool_index), Ns, C, H, W, P, batch, int(augment), int(shuffle),
                    int(seed) & 0xffffffff, stream_ptr(), ptr(zero),
                    zero.numel() if zero is not None else 0, recipe.shift, recipe.fmask[0],
                    recipe.fmask[1], recipe.tmask[0], recipe.tmask[1], lo, hi, recipe.fill,
                    ptr(params), chunks)


def is_sample(losses, ema, ctrl, idx, w, P, B, group, alpha=0.5, ema_alpha=0.9, seed=0,
              importance=True, meters=None, alias=True, gathered=None):
    """EMA replay + probabilities + B draws with replacement.  ``alias=True``: Walker alias
    table built in LDS and O(1) draws; ``alias=False``: inverse-CDF (prefix scan + search).
    ``gathered`` ([W][P] every rank's scores): the EMA is replayed over the global pool means
    (shared normaliser across ranks) while the draw still uses this rank's ``losses``."""
    _chk(losses, torch.float32, 'losses', P)
    _chk(idx, torch.int32, 'idx', B)
    lib().is_sample(ptr(losses), ptr(ema), ptr(ctrl), ptr(idx), ptr(w), ptr(meters), P, B, group,
                    int(importance), alpha, ema_alpha, int(seed) & 0xffffffff, stream_ptr(),
                    int(alias), ptr(gathered), gathered.shape[0] if gathered is not None else 1)


def gather(pool, pool_label, pool_index, idx, batch, batch_label, batch_index, B):
    per_img = pool[0].numel() * 2 // 16
    lib().gather(ptr(pool), ptr(pool_label), ptr(pool_index), ptr(idx), ptr(batch),
                 ptr(batch_label), ptr(batch_index), B, per_img, stream_ptr())
