"""Cost of the image recipes (csrc/pool_recipe.hip pool_recipe_kernel).

    python bench/photo_augment_bench.py pool [--out FILE] [--runs R]
    python bench/photo_augment_bench.py step [--out FILE] [--steps K] [--warmup W] [--runs R]

``pool``: ``bench/gtime.py`` time of one pool build at P = 320, 32x32 from a 40x40 shard, and at
P = 1280, 224x224 from a 256x256 shard (batch 32 and 128): the crop + flip recipe as the
yardstick against rrc + flip, rrc + flip + jitter without contrast (one sweep) and rrc + flip +
full jitter (two sweeps); at P = 320 also Resize(33) + RandomCrop(32) and the whole
``load_cifar10`` recipe (resize, crop, flip, affine) from a 32x32 shard.  Every call advances
the pool counter, so successive builds read other samples.  The variants are interleaved,
``--runs`` times.

``step``: the resnet50-imagenet preset built as ``bench.py`` builds it, ms/step with
``augment=None`` and with rrc + flip + full jitter + ImageNet Normalize, interleaved, ``--runs``
times.  One JSON line per measurement, appended to ``--out`` and printed.
"""
from __future__ import annotations

import os
if int(os.environ.get('GPU_MAX_HW_QUEUES') or 0) < 16:   # before torch loads HIP
    os.environ['GPU_MAX_HW_QUEUES'] = '16'

import argparse
import json
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bench'))

RRC = (0.08, 1.0, 3.0 / 4.0, 4.0 / 3.0)
NO_CONTRAST, FULL = (0.4, 0.0, 0.4, 0.1), (0.4, 0.4, 0.4, 0.1)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SHAPES = [(320, 32, 32, 40, 4096), (1280, 128, 224, 256, 2560)]   # P, batch, out, source, Ns


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(line + '\n')


def bench_pool(args):
    import torch
    from gtime import gtime
    from mercury_amd import ops
    from mercury_amd.data.augment import AugmentRecipe
    ops.lib()
    dev = 'cuda'
    for P, B, hw, src, Ns in SHAPES:
        g = torch.Generator(device=dev).manual_seed(8)
        shard = torch.randint(0, 256, (Ns, src, src, 3), dtype=torch.uint8, device=dev,
                              generator=g)
        labels = torch.randint(0, 1000, (Ns,), device=dev)
        ctrl = torch.zeros(4, dtype=torch.int64, device=dev)
        pool = torch.zeros(P, hw, hw, 8, dtype=torch.bfloat16, device=dev)
        pl = torch.zeros(P, dtype=torch.int32, device=dev)
        pi = torch.zeros(P, dtype=torch.int32, device=dev)
        kw = dict(crop=(hw, hw), flip=True, mean=MEAN, std=STD)
        recipes = [('crop + flip', AugmentRecipe(**kw), shard),
                   ('rrc + flip', AugmentRecipe(rrc=RRC, **kw), shard),
                   ('rrc + flip + jitter without contrast',
                    AugmentRecipe(rrc=RRC, jitter=NO_CONTRAST, **kw), shard),
                   ('rrc + flip + full jitter', AugmentRecipe(rrc=RRC, jitter=FULL, **kw), shard)]
        if hw == 32:                    # the IID loaders' test and train pipelines, 32x32 source
            small = shard[:, :32, :32].contiguous()
            recipes += [('resize 33 + crop', AugmentRecipe(resize=33, crop=(32, 32)), small),
                        ('resize 35 + crop + flip + affine',
                         AugmentRecipe(resize=35, crop=(32, 32), flip=True, degrees=10.0,
                                       scale=(0.9, 1.1)), small)]

        def build(recipe, src_shard):
            def fn():
                ops.pool_build(src_shard, labels, ctrl, pool, pl, pi, P, B, 7, recipe=recipe,
                               force_augment_kernel=not recipe.photo)
                ctrl[0:1].add_(1)
            return fn

        def tick():                     # what every variant pays beside its kernel
            ctrl[0:1].add_(1)

        variants = [('counter increment alone', tick, src)] + [
            ('pool_recipe_kernel ' + n, build(r, s), s.shape[1]) for n, r, s in recipes]
        for run in range(args.runs):
            for label, fn, source in variants:
                ctrl.zero_()
                us = gtime(fn, reps=16)
                emit({'bench': 'photo_pool', 'run': run, 'P': P, 'batch': B, 'out': hw,
                      'source': source, 'Ns': Ns, 'variant': label, 'us': round(us, 3),
                      'write_MB': round(0 if fn is tick else 16 * P * hw * hw / 1e6, 2)}, args.out)


def bench_step(args):
    import numpy as np
    import torch
    from bench import PRESETS, preset_data
    from mercury_amd.data.augment import AugmentRecipe
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    pre = PRESETS['resnet50-imagenet']
    hw, x, y = preset_data(pre)

    def one(recipe):
        torch.manual_seed(1234)
        net = build_model(pre['model'], pre['classes']).to('cuda')
        eng = NativeEngine(net, 'cuda', pre['batch'], 10, optimizer='adam', lr=0.001, seed=7,
                           importance=True, world_size=1, use_graphs=True, image_hw=hw,
                           augment=recipe)
        eng.set_shard(x, y)
        eng.prime()
        eng.step()
        eng.build_graphs()
        for _ in range(args.warmup):
            eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        m = eng.read_meters()
        eng.close()
        return ms, m['loss_sum'] / max(m['count'], 1)

    full = AugmentRecipe(crop=hw, rrc=RRC, flip=True, jitter=FULL, mean=MEAN, std=STD)
    res = {'none': [], 'full': []}
    for r in range(args.runs):
        for name, recipe in (('none', None), ('full', full)):
            ms, loss = one(recipe)
            res[name].append(ms)
            emit({'bench': 'photo_step', 'run': r, 'augment': name, 'steps': args.steps,
                  'warmup': args.warmup, 'ms_per_step': round(ms, 4),
                  'train_loss': round(loss, 4)}, args.out)
    off, on = float(np.median(res['none'])), float(np.median(res['full']))
    emit({'bench': 'photo_step_summary', 'median_ms_none': round(off, 4),
          'median_ms_full': round(on, 4), 'cost_us': round((on - off) * 1e3, 2),
          'none_max_minus_min_us': round((max(res['none']) - min(res['none'])) * 1e3, 2),
          'full_max_minus_min_us': round((max(res['full']) - min(res['full'])) * 1e3, 2)},
         args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('pool', 'step'))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    args = ap.parse_args()
    (bench_pool if args.mode == 'pool' else bench_step)(args)


if __name__ == '__main__':
    main()
