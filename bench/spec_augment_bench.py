"""Cost of the spectrogram recipes (csrc/importance.hip pool_spec_kernel).

    python bench/spec_augment_bench.py pool [--out FILE] [--runs R] [--ns N]
    python bench/spec_augment_bench.py step [--out FILE] [--steps K] [--warmup W] [--runs R]

``pool``: ``bench/gtime.py`` time of one pool build of 1x101x161 spectrograms at P = 320 and
P = 32 (batch 32), from a shard of ``--ns`` samples (default: the vgg11-speech preset's 20000):
``pool_take_kernel`` on the NHWC8 shard (the path without a recipe) against ``pool_spec_kernel``
on the planar shard, as the identity and as the full recipe, with the launcher's own grid and
with fixed numbers of blocks per slot.  Every call advances the pool counter, so successive
builds read other samples.  The variants are interleaved, ``--runs`` times.

``step``: the vgg11-speech preset built as ``bench.py`` builds it, ms/step with ``augment=None``
and with the full recipe, interleaved, ``--runs`` times; also the shard's bytes in HBM.
One JSON line per measurement, appended to ``--out`` and printed.
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

FULL = 'spec:shift=3,fmask=2x2,tmask=2x6,gain=0.5:2,fill=-1.5'
H, W = 101, 161


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
    from mercury_amd.data.augment import SpecRecipe
    from mercury_amd.ops.importance import _pool_spec
    ops.lib()
    dev = 'cuda'
    Ns, B = args.ns, 32
    planar = torch.empty(Ns, 1, H, W, dtype=torch.bfloat16, device=dev)
    nhwc8 = torch.empty(Ns, H, W, 8, dtype=torch.bfloat16, device=dev)
    g = torch.Generator(device=dev).manual_seed(8)
    for s0 in range(0, Ns, 2048):
        blk = torch.randn(min(2048, Ns - s0), 1, H, W, device=dev, generator=g)
        planar[s0:s0 + 2048] = blk
        ops.nchw_to_nhwc8(blk, nhwc8[s0:s0 + 2048])
    labels = torch.randint(0, 30, (Ns,), device=dev)
    recipes = {'identity': SpecRecipe(), 'full': SpecRecipe.parse(FULL)}
    for P in (320, 32):
        ctrl = torch.zeros(4, dtype=torch.int64, device=dev)
        pool = torch.zeros(P, H, W, 8, dtype=torch.bfloat16, device=dev)
        pl = torch.zeros(P, dtype=torch.int32, device=dev)
        pi = torch.zeros(P, dtype=torch.int32, device=dev)

        def take():
            ops.pool_build(nhwc8, labels, ctrl, pool, pl, pi, P, B, 7)
            ctrl[0:1].add_(1)

        def spec(recipe, chunks):
            def fn():
                _pool_spec(planar, labels, ctrl, pool, pl, pi, P, B, 7, True, True, None, recipe,
                           None, chunks=chunks)
                ctrl[0:1].add_(1)
            return fn

        def tick():                     # what every variant pays beside its kernel
            ctrl[0:1].add_(1)

        variants = [('pool_take_kernel (NHWC8 shard)', 'take', 0, take),
                    ('counter increment alone', 'tick', 0, tick)]
        for name, r in recipes.items():
            for chunks in (0, 1, 2, 4, 8, 16, 64):
                variants.append(('pool_spec_kernel %s' % name, name, chunks, spec(r, chunks)))
        # identity == the plain gather, at the sizes timed
        ctrl.zero_()
        take()
        want = pool.clone()
        ctrl.zero_()
        variants[2][3]()
        torch.cuda.synchronize()
        same = bool(torch.equal(want.view(torch.int16), pool.view(torch.int16)))
        px = P * H * W
        for run in range(args.runs):
            for label, kind, chunks, fn in variants:
                ctrl.zero_()
                us = gtime(fn, reps=16)
                rd = {'take': 16 * px, 'tick': 0}.get(kind, 2 * px)
                emit({'bench': 'spec_pool', 'run': run, 'P': P, 'Ns': Ns, 'variant': label,
                      'chunks': chunks, 'us': round(us, 3), 'read_MB': round(rd / 1e6, 2),
                      'write_MB': round(0 if kind == 'tick' else 16 * px / 1e6, 2),
                      'identity_equals_take': same}, args.out)
    emit({'bench': 'spec_shard_bytes', 'Ns': Ns,
          'nhwc8_bytes': nhwc8.numel() * nhwc8.element_size(),
          'planar_bytes': planar.numel() * planar.element_size()}, args.out)


def bench_step(args):
    import numpy as np
    import torch
    from bench import PRESETS, preset_data
    from mercury_amd.data.augment import SpecRecipe
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    pre = PRESETS['vgg11-speech']
    hw, x, y = preset_data(pre)

    def one(recipe):
        torch.manual_seed(1234)
        net = build_model(pre['model'], pre['classes']).to('cuda')
        eng = NativeEngine(net, 'cuda', pre['batch'], 10, optimizer='adam', lr=0.001, seed=7,
                           importance=True, world_size=1, use_graphs=True, image_hw=hw,
                           augment=recipe)
        eng.set_shard(x, y)
        shard_bytes = eng.shard.numel() * eng.shard.element_size()
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
        return ms, m['loss_sum'] / max(m['count'], 1), shard_bytes

    full = SpecRecipe.parse(FULL)
    res = {'none': [], 'full': []}
    for r in range(args.runs):
        for name, recipe in (('none', None), ('full', full)):
            ms, loss, nbytes = one(recipe)
            res[name].append(ms)
            emit({'bench': 'spec_step', 'run': r, 'augment': name, 'steps': args.steps,
                  'warmup': args.warmup, 'ms_per_step': round(ms, 4),
                  'train_loss': round(loss, 4), 'shard_bytes': nbytes}, args.out)
    off, on = float(np.median(res['none'])), float(np.median(res['full']))
    emit({'bench': 'spec_step_summary', 'median_ms_none': round(off, 4),
          'median_ms_full': round(on, 4), 'cost_us': round((on - off) * 1e3, 2),
          'none_max_minus_min_us': round((max(res['none']) - min(res['none'])) * 1e3, 2),
          'full_max_minus_min_us': round((max(res['full']) - min(res['full'])) * 1e3, 2)},
         args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('pool', 'step'))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--ns', type=int, default=20000)
    args = ap.parse_args()
    (bench_pool if args.mode == 'pool' else bench_step)(args)


if __name__ == '__main__':
    main()
