"""Cost of global-norm gradient clipping (csrc/optim.hip grad_norm_launch).

    python bench/clip_bench.py norm  [--out FILE]     # the norm pass alone, graph-replay time
    python bench/clip_bench.py step  [--out FILE] [--steps K] [--warmup W] [--runs R]

``norm``: ``bench/gtime.py`` time of the two norm launches over a flat fp32 gradient of
ResNet-18's and ResNet-50's size (the engine's padded flat length), as bytes per second, next
to a plain read-only pass of torch (``g.sum()``) over the same buffer.  Every call reads another
of four copies (180 MB / 400 MB in all), so no call finds its buffer in L2; ResNet-18's set
still fits the 256 MB Infinity Cache, as the gradient that backward just wrote does in the step.

``step``: the ResNet-18 preset built as ``bench.py`` builds it (Adam, lr 1e-3, importance
sampling, graphs), ms/step with ``clip_grad_norm`` off and on, interleaved, ``--runs`` times.
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


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(line + '\n')


def flat_sizes():
    """Padded flat parameter counts of the two models, as the engine lays them out."""
    from mercury_amd.engine.lower import lower
    from mercury_amd.models import build_model
    return {'resnet18': lower(build_model('resnet18', 10)).total,
            'resnet50_imagenet': lower(build_model('resnet50_imagenet', 1000)).total}


def bench_norm(args):
    import torch
    from gtime import gtime
    from mercury_amd import ops
    from mercury_amd.ops import optim as O
    ops.lib()
    dev = 'cuda'
    mx = torch.tensor([1.0], device=dev)
    rec = torch.zeros(2, device=dev)
    ws = torch.zeros(O.GN_WS_FLOATS, device=dev)
    for name, n in flat_sizes().items():
        bufs = [torch.randn(n, device=dev) for _ in range(4)]
        state = {'i': 0}

        def norm():
            state['i'] = (state['i'] + 1) % len(bufs)
            ops.grad_norm(bufs[state['i']], mx, rec, ws)

        acc = torch.zeros((), device=dev)

        def read_only():
            state['i'] = (state['i'] + 1) % len(bufs)
            torch.sum(bufs[state['i']], dim=0, out=acc)

        us = gtime(norm, reps=16)
        us_sum = gtime(read_only, reps=16)
        norm()                         # the record of the buffer the reference is taken from
        torch.cuda.synchronize()
        ref = float(torch.linalg.vector_norm(bufs[state['i']].double()))
        pl = O.grad_norm_plan(n)
        emit({'bench': 'grad_norm', 'model': name, 'n': n, 'bytes': 4 * n,
              'blocks': pl['blocks'], 'trips': pl['trips'], 'launches': 2,
              'us': round(us, 3), 'TBps': round(4 * n / us / 1e6, 3),
              'torch_sum_us': round(us_sum, 3), 'torch_sum_TBps': round(4 * n / us_sum / 1e6, 3),
              'norm': float(rec[0]), 'norm_fp64': ref}, args.out)


def bench_step(args):
    import numpy as np
    import torch
    from bench import PRESETS, preset_data
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    pre = PRESETS['resnet18-cifar10']
    hw, x, y = preset_data(pre)

    def one(clip):
        torch.manual_seed(1234)
        net = build_model(pre['model'], pre['classes']).to('cuda')
        eng = NativeEngine(net, 'cuda', pre['batch'], 10, optimizer='adam', lr=0.001, seed=7,
                           importance=True, world_size=1, use_graphs=True, image_hw=hw,
                           clip_grad_norm=clip)
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
        gn = eng.opt.last_grad_norm() if clip else None
        eng.close()
        return ms, m['loss_sum'] / max(m['count'], 1), gn

    res = {0.0: [], args.clip: []}
    for r in range(args.runs):
        for clip in (0.0, args.clip):
            ms, loss, gn = one(clip)
            res[clip].append(ms)
            emit({'bench': 'clip_step', 'run': r, 'clip_grad_norm': clip, 'steps': args.steps,
                  'warmup': args.warmup, 'ms_per_step': round(ms, 4),
                  'train_loss': round(loss, 4), 'last_grad_norm': gn}, args.out)
    off, on = float(np.median(res[0.0])), float(np.median(res[args.clip]))
    emit({'bench': 'clip_step_summary', 'median_ms_off': round(off, 4),
          'median_ms_on': round(on, 4), 'cost_us': round((on - off) * 1e3, 2),
          'cost_pct': round(100.0 * (on - off) / off, 3)}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('norm', 'step'))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--clip', type=float, default=1.0)
    args = ap.parse_args()
    (bench_norm if args.mode == 'norm' else bench_step)(args)


if __name__ == '__main__':
    main()
