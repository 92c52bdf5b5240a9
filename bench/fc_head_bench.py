"""Native MyLSTM head (csrc/fc_head.hip through ops.fc_head) against the torch chain of this tree.

The head alone -- dropout, Linear(W, W) + BatchNorm1d(W) + ReLU, dropout, Linear(W, classes) --
at W = 2048, classes = 35, B = 32 and B = 320: the eval forward (no_grad, what scoring runs) and
the training forward + backward (dropout 0.2), graph-timed with bench/gtime.py, the two paths
interleaved, ROUNDS runs each; median and range are reported, and whether the shape qualifies for
``ops.fc_head.MEASURED_NATIVE`` (native's median below torch's fastest run in both columns).
With --model, one MyLSTM(cell='native', attn='native', proj='native') forward + backward at
B = 32 is timed with head='torch' against head='native': the head's share of a step.

    python bench/fc_head_bench.py [--out profiles/r23/fc_head/fc_head_bench.jsonl] [--quick] [--model]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attn_bench import _interleaved  # noqa: E402

W, CLASSES, P = 2048, 35, 0.2
BATCHES = (32, 320)
ROUNDS = 3


def _head_runners(B, train):
    import torch
    import torch.nn as nn
    from mercury_amd.ops import fc_head as FH
    torch.manual_seed(0)
    z = torch.randn(B, W, device='cuda')
    g = torch.randn(B, CLASSES, device='cuda')
    fc1 = nn.Sequential(nn.Linear(W, W), nn.BatchNorm1d(W), nn.ReLU()).cuda().train(train)
    fc2 = nn.Linear(W, CLASSES).cuda()
    drop = nn.Dropout(P).train(train)
    params = list(fc1.parameters()) + list(fc2.parameters())

    def run(head):
        if not train:
            with torch.no_grad():
                head(z)
            return
        for p in params:
            p.grad = None
        head(z.detach().requires_grad_()).backward(g)

    return {'torch': lambda: run(lambda x: fc2(drop(fc1(drop(x))))),
            'native': lambda: run(lambda x: FH.fc_head(x, fc1, fc2, P, train))}


def _model_runners(B):
    import torch
    from mercury_amd.models import MyLSTM
    torch.manual_seed(0)
    x = torch.randn(B, 1, 101, 161, device='cuda')
    g = torch.randn(B, CLASSES, device='cuda')
    kw = dict(hidden_dim=W // 4, dropout=P, cell='native', attn='native', proj='native')
    base = MyLSTM(101, CLASSES, **kw).cuda()
    fns = {}
    for head in ('torch', 'native'):
        m = MyLSTM(101, CLASSES, head=head, **kw).cuda()
        m.load_state_dict(base.state_dict())

        def run(m=m):
            for p in m.parameters():
                p.grad = None
            m(x).backward(g)

        fns[head] = run
    return fns


def _columns(rec, r):
    for n, (med, every, how) in r.items():
        rec[n + '_us'] = round(med, 1)
        rec[n + '_all_us'] = every
        rec[n + '_timing'] = how
    rec['native_over_torch'] = round(rec['native_us'] / rec['torch_us'], 3)
    rec['native_median_below_torch_min'] = rec['native_us'] < min(rec['torch_all_us'])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23', 'fc_head',
                                                  'fc_head_bench.jsonl'))
    ap.add_argument('--quick', action='store_true', help='B=32 only, one round')
    ap.add_argument('--model', action='store_true', help='the MyLSTM rows instead of the head rows')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fc_head_bench: no HIP device; nothing is measured without one')
    batches = BATCHES[:1] if args.quick else BATCHES
    rounds = 1 if args.quick else ROUNDS
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        def emit(rec):
            rec['device'] = dev
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + '\n')
            fh.flush()

        if args.model:
            emit(_columns({'what': 'mylstm', 'B': 32, 'T': 161, 'H': W // 4, 'mode': 'fwd_bwd',
                           'cell': 'native', 'attn': 'native', 'proj': 'native'},
                          _interleaved(_model_runners(32), rounds, reps=1)))
            return
        for B in batches:
            ok = True
            for train in (False, True):
                rec = _columns({'what': 'head', 'B': B, 'W': W, 'classes': CLASSES,
                                'mode': 'fwd_bwd' if train else 'fwd'},
                               _interleaved(_head_runners(B, train), rounds, reps=8))
                ok = ok and rec['native_median_below_torch_min']
                emit(rec)
                torch.cuda.empty_cache()
            emit({'what': 'measured_native', 'key': [B, W, CLASSES], 'qualifies': ok})


if __name__ == '__main__':
    main()
