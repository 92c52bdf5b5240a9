"""Importance-sampling kernels front-end (``csrc/importance.hip``, ``csrc/pool_recipe.hip``)."""
from __future__ import annotations

import torch

from . import _chk, lib, ptr, stream_ptr
from ..data.augment import PHOTO_PARAMS, SPEC_PARAMS, WAVE_PARAMS, SpecRecipe, WaveRecipe
from ..data.transforms import CIFAR_MEAN, CIFAR_STD


def pool_build(shard, labels, ctrl, pool, pool_label, pool_index, P, batch, seed, pad=4,
               flip=True, augment=True, mean=CIFAR_MEAN, std=CIFAR_STD, shuffle=True, zero=None,
               recipe=None, params=None, force_augment_kernel=False, noise=None, rir=None):
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
    same samples' NHWC8 shard.

    A ``data.augment.WaveRecipe`` (shift, gain, background noise on the waveform, then the
    log-spectrogram) takes an int16 or float32 shard of raw clips [Ns][L], an optional ``noise``
    bank [Nn][Ln] of the same dtype and a pool [P][n_fft/2+1][1+L//hop][8]
    (``pool_wave_kernel``); ``params`` is then fp32 [P][16] (``data.augment.WAVE_PARAMS``).
    With ``mel`` (and ``dct``) set the pool is [P][R][1+L//hop][8], R = ``recipe.out_hw(L)[0]``
    log-mel bands or cepstral coefficients (``pool_wave_mel_kernel``, ``csrc/pool_mel.hip``),
    followed by their first and second time differences when ``delta`` is set.
    ``augment=False`` draws the identity and still transforms.  The first build for an
    ``(n_fft, device)`` makes the DFT table (an allocation and a copy), the first for a mel
    recipe its filter-bank and DCT tables, the first for a ``speed`` recipe the resampler's
    filter table, the first for a ``cmvn`` recipe and pool shape its fp32 feature workspace (the
    recipe then runs two launches: ``pool_wave_mel_kernel`` into the workspace, ``pool_cmvn_kernel``
    from it into the pool): inside a graph capture only after such a call or ``pool_wave_table`` /
    ``pool_mel_tables`` / ``pool_speed_table`` / ``pool_cmvn_workspace``
    (``NativeEngine.set_shard`` makes them).  ``preemph`` only changes the DFT table.
    A ``reverb`` recipe takes its float32 bank ``rir`` [Nr][K], K <= 4096, and with ``augment``
    on runs ``pool_reverb_kernel`` (``csrc/pool_reverb.hip``) in front: each slot's clip,
    convolved with a drawn response or copied, goes into the fp32 workspace
    ``pool_reverb_workspace(P, L, device)`` and the launches above read it in place of the shard.
    That workspace, and for an int16 shard the noise bank's fp32 copy (``pool_noise_f32``), are
    made by the first such build (outside a capture)."""
    _chk(labels, torch.int64, 'labels')
    if isinstance(recipe, WaveRecipe):
        if force_augment_kernel:
            raise ValueError('force_augment_kernel belongs to an AugmentRecipe')
        return _pool_wave(shard, noise, labels, ctrl, pool, pool_label, pool_index, P, batch,
                          seed, augment, shuffle, zero, recipe, params, rir=rir)
    if noise is not None or rir is not None:
        raise ValueError('noise / rir: a noise or RIR bank belongs to a WaveRecipe')
    if shard.dim() == 2:
        raise ValueError('shard is [Ns][L] raw clips: that needs a WaveRecipe')
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


_WAVE_TABLES = {}    # (n_fft, preemph, device) -> the DFT table, built once (never inside a capture)


def pool_wave_table(recipe, device):
    """``WaveRecipe.table`` padded to the kernel's K steps, resident on ``device``."""
    key = (recipe.n_fft, recipe.preemph, str(device))
    if key not in _WAVE_TABLES:
        _WAVE_TABLES[key] = recipe.table(lib().pool_wave_ksteps(recipe.n_fft)).to(device)
    return _WAVE_TABLES[key]


_MEL_TABLES = {}     # (n_fft, mel, sr, fmin, fmax, dct, lifter, device) -> (mel table, dct table
#                      | None, K ranges), built once (never inside a capture)


def pool_mel_tables(recipe, device):
    """``(mel_table, dct_table or None, mel_ksteps)`` of a mel recipe, the tables resident on
    ``device``."""
    key = (recipe.n_fft, recipe.mel, recipe.sr, recipe.fmin, recipe.fmax, recipe.dct,
           recipe.lifter, str(device))
    if key not in _MEL_TABLES:
        _MEL_TABLES[key] = (recipe.mel_table().to(device),
                            recipe.dct_table().to(device) if recipe.dct else None,
                            recipe.mel_ksteps())
    return _MEL_TABLES[key]


_SPEED_TABLES = {}   # (speed hi, device) -> the resampler's filter table (never inside a capture)


def pool_speed_table(recipe, device):
    """``WaveRecipe.speed_table`` resident on ``device``."""
    key = (recipe.speed[1], str(device))
    if key not in _SPEED_TABLES:
        _SPEED_TABLES[key] = recipe.speed_table().contiguous().to(device)
    return _SPEED_TABLES[key]


_CMVN_FEAT = {}      # (P, R, Tp, device) -> the fp32 feature workspace of a cmvn recipe


def pool_cmvn_workspace(recipe, P, L, device):
    """The fp32 workspace ``[P][R][Tp]``, ``Tp = T`` rounded up to 4, through which a ``cmvn``
    recipe's two launches hand the raw features, one per shape and device (never allocated
    inside a capture: ``NativeEngine.set_shard`` makes it).  Pool builds of one shape share it,
    which is safe on one stream, where the launches are ordered."""
    R, T = recipe.feat_rows, recipe.out_hw(L)[1]
    key = (P, R, (T + 3) // 4 * 4, str(device))
    if key not in _CMVN_FEAT:
        _CMVN_FEAT[key] = torch.empty(key[:3], dtype=torch.float32, device=device)
    return _CMVN_FEAT[key]


_REVERB_WS = {}      # (P, L, device) -> the fp32 workspace of a reverb recipe's pre-pass
_NOISE_F32 = {}      # (data_ptr, shape, device) -> (the int16 noise bank, its fp32 copy / 32768)


def pool_reverb_workspace(P, L, device):
    """The fp32 workspace ``[P][L]``, indexed by pool slot, into which a ``reverb`` recipe's
    pre-pass writes each slot's (convolved) clip, one per shape and device (never allocated
    inside a capture: ``NativeEngine.set_shard`` makes it).  Pool builds of one shape share it,
    which is safe on one stream, where the launches are ordered."""
    device = torch.device(device)
    if device.index is None:             # 'cuda' and 'cuda:0' name one workspace
        device = torch.device(device.type, torch.cuda.current_device())
    key = (P, L, str(device))
    if key not in _REVERB_WS:
        _REVERB_WS[key] = torch.empty(P, L, dtype=torch.float32, device=device)
    return _REVERB_WS[key]


def pool_noise_f32(noise):
    """An int16 noise bank as float32 ``x / 32768`` (exact): what the wave kernels mix from when
    they read a reverb pre-pass's fp32 workspace.  Made once per bank, which the cache keeps
    alive; a bank changed in place needs a new tensor."""
    key = (noise.data_ptr(), tuple(noise.shape), str(noise.device))
    if key not in _NOISE_F32:
        _NOISE_F32[key] = (noise, noise.to(torch.float32) / 32768)
    return _NOISE_F32[key][1]


def _pool_wave(shard, noise, labels, ctrl, pool, pool_label, pool_index, P, batch, seed, augment,
               shuffle, zero, recipe, params, chunks=0, rir=None, rev_chunks=0):
    if shard.dtype not in (torch.int16, torch.float32) or shard.dim() != 2:
        raise ValueError('a WaveRecipe needs an int16 or float32 shard [Ns][L], got %s %s'
                         % (shard.dtype, tuple(shard.shape)))
    _chk(shard, shard.dtype, 'shard')
    Ns, L = int(shard.shape[0]), int(shard.shape[1])
    recipe.check(L, None if noise is None else tuple(noise.shape),
                 None if rir is None else tuple(rir.shape))
    if noise is not None:
        if noise.dtype != shard.dtype:
            raise ValueError('noise bank is %s but the shard is %s' % (noise.dtype, shard.dtype))
        _chk(noise, shard.dtype, 'noise')
    F, T = recipe.out_hw(L)
    if pool.dim() != 4 or tuple(pool.shape[1:]) != (F, T, 8):
        raise ValueError('pool must be [P][%d][%d][8] for this WaveRecipe, got %s'
                         % (F, T, tuple(pool.shape)))
    _chk(pool, torch.bfloat16, 'pool', P * F * T * 8)
    if params is not None:
        _chk(params, torch.float32, 'params', P * WAVE_PARAMS)
    tab = pool_wave_table(recipe, shard.device)
    mel = {}
    if recipe.mel:
        mtab, dtab, krange = pool_mel_tables(recipe, shard.device)
        mel = dict(mel=recipe.mel, dct=recipe.dct, mel_tab=ptr(mtab), mel_floats=mtab.numel(),
                   dct_tab=ptr(dtab), dct_floats=dtab.numel() if dtab is not None else 0,
                   krange=krange, delta=recipe.delta, dwin=recipe.dwin)
    if recipe.speed is not None:
        stab = pool_speed_table(recipe, shard.device)
        mel.update(speed_tab=ptr(stab), speed_floats=stab.numel(),
                   **dict(zip(('rq_lo', 'rq_hi'), recipe.speed_rq())))
    if recipe.cmvn:
        feat = pool_cmvn_workspace(recipe, P, L, shard.device)
        mel.update(cmvn=recipe.cmvn, feat=ptr(feat), feat_floats=feat.numel())
    if recipe.reverb:
        if rir.dtype != torch.float32:
            raise ValueError('RIR bank is %s: it is always float32' % rir.dtype)
        _chk(rir, torch.float32, 'rir')
        rev = pool_reverb_workspace(P, L, shard.device)
        mel.update(reverb_p=recipe.reverb, rir=ptr(rir), rir_floats=rir.numel(),
                   Nr=rir.shape[0], rir_k=rir.shape[1], rev=ptr(rev), rev_floats=rev.numel(),
                   rev_chunks=rev_chunks)
        if noise is not None and noise.dtype == torch.int16:
            mel.update(noise_f32=ptr(pool_noise_f32(noise)))
    glo, ghi = recipe.gain or (1.0, 1.0)
    p, vol = recipe.noise or (0.0, 0.0)
    a, b = recipe.affine()
    lib().pool_wave(shard=ptr(shard), noise=ptr(noise), tab=ptr(tab), tab_floats=tab.numel(),
                    labels=ptr(labels), ctrl=ptr(ctrl), pool=ptr(pool), pool_label=ptr(pool_label),
                    pool_index=ptr(pool_index), params=ptr(params), zero=ptr(zero),
                    nzero=zero.numel() if zero is not None else 0, stream=stream_ptr(),
                    f32=int(shard.dtype == torch.float32), Ns=Ns, L=L,
                    Nn=noise.shape[0] if noise is not None else 0,
                    Ln=noise.shape[1] if noise is not None else 0, n_fft=recipe.n_fft,
                    hop=recipe.hop, P=P, batch=batch, augment=int(augment), shuffle=int(shuffle),
                    seed=int(seed) & 0xffffffff, shift=recipe.shift, gain_lo=glo, gain_hi=ghi,
                    noise_p=p, vol_max=vol, eps=recipe.eps, log_a=a, log_b=b,
                    fmask_n=recipe.fmask[0], fmask_max=recipe.fmask[1], tmask_n=recipe.tmask[0],
                    tmask_max=recipe.tmask[1], fill=recipe.fill, chunks=chunks,
                    **mel)


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
