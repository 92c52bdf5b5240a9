"""Native attention pooling (csrc/attn.hip through ops.attention) against the eager Attention.

The module as MyLSTM uses it (batch_first=True on the transposed view of a time-major layer
output), T = 161, D = 1024, at B = 32 and B = 320: forward alone (no_grad) and forward +
backward, fp32 input for both paths and bf16 input for the native op, graph-timed with
bench/gtime.py, the paths interleaved, ROUNDS times each, the median reported.  The launches
alone (preallocated buffers) are timed too, for the bytes/s of each native kernel pair: the
forward reads x once, the backward reads x once and writes dx once.  With --model, one MyLSTM
step (cell='native') is timed with attn='torch' against attn='native'.

    python bench/attn_bench.py [--out profiles/r11/attn/attn_bench.jsonl] [--quick] [--model]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T, D = 161, 1024
BATCHES = (32, 320)
ROUNDS = 3


def _etime(fn, iters=5):
    """Event-timed eager calls (microseconds, median): only where a path cannot be captured."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


def _time(fn, how, reps=4):
    from gtime import gtime
    if how[0] == 'graph':
        try:
            return gtime(fn, reps=reps, iters=5)
        except Exception as e:      # e.g. a library call that is not capturable
            import torch
            torch.cuda.synchronize()
            how[0] = 'eager events (capture failed: %s)' % type(e).__name__
    return _etime(fn)


def _interleaved(fns, rounds, reps=4):
    """{name: (median us, all us, how)} of the callables, timed in turn ``rounds`` times."""
    how = {n: ['graph'] for n in fns}
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(_time(fn, how[n], reps))
    return {n: (statistics.median(v), [round(u, 1) for u in v], how[n][0]) for n, v in ts.items()}


def _module_runners(B, train):
    import torch
    from mercury_amd.models.lstm import Attention
    torch.manual_seed(0)
    x = torch.randn(T, B, D, device='cuda')
    g = torch.randn(B, D, device='cuda')
    mods = {i: Attention(D, batch_first=True, impl=i).cuda() for i in ('torch', 'native')}
    mods['native'].load_state_dict(mods['torch'].state_dict())

    def run(m, xin):
        if not train:
            with torch.no_grad():
                m(xin.transpose(0, 1))
            return
        m.att_weights.grad = None
        xin = xin.detach().requires_grad_()
        m(xin.transpose(0, 1))[0].backward(g)

    xb = x.to(torch.bfloat16)
    return {'torch_fp32': lambda: run(mods['torch'], x), 'native_fp32': lambda: run(mods['native'], x),
            'native_bf16': lambda: run(mods['native'], xb)}


def _kernel_runners(B, dtype):
    import torch
    from mercury_amd.ops import attention as A
    torch.manual_seed(0)
    x = torch.randn(T, B, D, device='cuda').to(dtype)
    w = (torch.rand(D, device='cuda') * 2 - 1) / D ** 0.5
    g = torch.randn(B, D, device='cuda')
    rep, attn, score = (torch.empty(B, n, device='cuda') for n in (D, T, T))
    ws = torch.empty(A.fwd_ws_floats(T, B, D), device='cuda')
    dx, dw = torch.empty_like(x), torch.empty(D, device='cuda')
    A.attn_pool_fwd(x, w, None, rep, attn, score, ws)
    return {'fwd': lambda: A.attn_pool_fwd(x, w, None, rep, attn, None, ws),
            'fwd_train': lambda: A.attn_pool_fwd(x, w, None, rep, attn, score, ws),
            'bwd': lambda: A.attn_pool_bwd(x, w, g, rep, attn, score, None, dx, dw, ws)}, x.numel() * x.element_size()


def _model_runners(B, train):
    import torch
    from mercury_amd.models import MyLSTM
    torch.manual_seed(0)
    x = torch.randn(B, 1, 101, T, device='cuda')
    g = torch.randn(B, 35, device='cuda')
    base = MyLSTM(101, 35, hidden_dim=D // 2, dropout=0.0, cell='native').cuda()
    fns = {}
    for impl in ('torch', 'native'):
        m = MyLSTM(101, 35, hidden_dim=D // 2, dropout=0.0, cell='native', attn=impl).cuda()
        m.load_state_dict(base.state_dict())

        def run(m=m):
            if not train:
                with torch.no_grad():
                    m(x)
                return
            for p in m.parameters():
                p.grad = None
            m(x).backward(g)

        fns['attn_' + impl] = run
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11', 'attn', 'attn_bench.jsonl'))
    ap.add_argument('--quick', action='store_true', help='B=32 only, one round')
    ap.add_argument('--model', action='store_true', help='the MyLSTM rows instead of the op rows')
    args = ap.parse_args()
    import torch
    batches = BATCHES[:1] if args.quick else BATCHES
    rounds = 1 if args.quick else ROUNDS
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(fh, rec):
        rec['device'] = dev
        line = json.dumps(rec)
        print(line, flush=True)
        fh.write(line + '\n')
        fh.flush()

    with open(args.out, 'a') as fh:
        if args.model:
            # forward + backward at the training batch, the no-grad scoring forward at B = 320
            for B, train in ((32, True),) if args.quick else ((32, True), (320, False)):
                r = _interleaved(_model_runners(B, train), rounds, reps=1)
                emit(fh, {'what': 'mylstm', 'T': T, 'B': B, 'H': D // 2, 'cell': 'native',
                          'mode': 'fwd_bwd' if train else 'fwd',
                          'attn_torch_us': round(r['attn_torch'][0], 1),
                          'attn_native_us': round(r['attn_native'][0], 1),
                          'attn_torch_all_us': r['attn_torch'][1],
                          'attn_native_all_us': r['attn_native'][1],
                          'timing': [r['attn_torch'][2], r['attn_native'][2]]})
                torch.cuda.empty_cache()
            return
        for B in batches:
            for train in (False, True):
                r = _interleaved(_module_runners(B, train), rounds)
                rec = {'what': 'module', 'T': T, 'B': B, 'D': D, 'mode': 'fwd_bwd' if train else 'fwd'}
                for n, (med, every, how) in r.items():
                    rec[n + '_us'] = round(med, 1)
                    rec[n + '_all_us'] = every
                    rec[n + '_timing'] = how
                rec['native_over_torch'] = round(rec['native_fp32_us'] / rec['torch_fp32_us'], 3)
                emit(fh, rec)
                torch.cuda.empty_cache()
            for dtype in (torch.float32, torch.bfloat16):
                fns, xbytes = _kernel_runners(B, dtype)
                r = _interleaved(fns, rounds, reps=8)
                rec = {'what': 'launches', 'T': T, 'B': B, 'D': D, 'x': str(dtype)[6:],
                       'x_bytes': xbytes}
                for n, (med, every, how) in r.items():
                    rec[n + '_us'] = round(med, 1)
                    rec[n + '_all_us'] = every
                    # TB/s of the bytes the pair of launches must move: x once forward, x + dx backward
                    rec[n + '_TBps'] = round((2 if n == 'bwd' else 1) * xbytes / med * 1e-6, 3)
                emit(fh, rec)
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
