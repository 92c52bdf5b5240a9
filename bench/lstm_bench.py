"""Native BiLSTM cell (csrc/lstm.hip through ops.lstm.bilstm) against nn.LSTM in bf16 (MIOpen).

One bidirectional layer, forward alone (no_grad) and forward + backward, graph-timed with
bench/gtime.py (the recurrence is T short launches: event-timing eager calls would measure the
host).  The two cells are timed interleaved, ROUNDS times each, and the median is reported.
Shapes: MyLSTM's layer 1 on the speech input (T=161, F=101, H=512) at B=32 and B=320, and its
layer 2 (F=1024).  One JSON line per (shape, mode); ops.lstm.MEASURED_NATIVE lists the (B, H)
at which ``native_us <= torch_us`` for forward + backward on every layer measured.

``--lengths full`` / ``uniform`` (all rows of length T; lengths uniform in [T/2, T], ``--seed``)
compares ``bilstm(x, lstm, lengths)`` with what a user would otherwise run: bf16 ``nn.LSTM``
between ``pack_padded_sequence(enforce_sorted=False)`` and ``pad_packed_sequence(total_length=T)``.
The native cell is timed as host-side lengths run it (the launches cut to max(len_b) steps;
``BiLSTMFunction`` is called with the device tensor and the step count, since a list's
host-to-device copy cannot be captured) and with a device tensor (all T steps, no host sync).
Both cells are also event-timed eagerly (``*_eager_us``, the native one through
``bilstm(x, lstm, list)``): where pack / unpack cannot be captured, that pair is the like-for-like one.
ops.lstm.MEASURED_NATIVE_PACKED lists the (B, H) at which native is not slower in both modes, on
both layers and both distributions.

    python bench/lstm_bench.py [--out profiles/r8/lstm/lstm_bench.jsonl] [--quick]
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

SHAPES = [('layer1_b32', 161, 32, 101, 512), ('layer1_b320', 161, 320, 101, 512),
          ('layer2_b32', 161, 32, 1024, 512), ('layer2_b320', 161, 320, 1024, 512)]
ROUNDS = 3


def _lens(kind, T, B, seed):
    import torch
    if kind == 'none':
        return None
    if kind == 'full':
        return [T] * B
    g = torch.Generator().manual_seed(seed)
    return [int(v) for v in torch.randint(T // 2, T + 1, (B,), generator=g)]


def _runners(T, B, F, H, train, lens=None):
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    from mercury_amd.ops import lstm as L
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(F, H, num_layers=1, bidirectional=True).cuda()
    ref = torch.nn.LSTM(F, H, num_layers=1, bidirectional=True).cuda().to(torch.bfloat16)
    x = torch.randn(T, B, F, device='cuda')
    gout = torch.randn(T, B, 2 * H, device='cuda')
    xb, gb = x.to(torch.bfloat16), gout.to(torch.bfloat16)

    def run(f, m, xin, g):
        if not train:
            with torch.no_grad():
                f(xin, m)
            return
        for p in m.parameters():
            p.grad = None
        xin = xin.detach().requires_grad_()
        f(xin, m).backward(g)

    if lens is None:
        return ((lambda: run(L.bilstm, lstm, x, gout)),
                (lambda: run(lambda a, m: m(a)[0], ref, xb, gb)), None)
    cpu = torch.tensor(lens, dtype=torch.int64)
    dev = cpu.to('cuda', torch.int32)

    def packed(a, m):
        pk = pack_padded_sequence(a, cpu, enforce_sorted=False)
        return pad_packed_sequence(m(pk)[0], total_length=T)[0]

    def trimmed(a, m):
        # what bilstm(a, m, lens) runs, without the list's host-to-device copy (not capturable)
        return L.BiLSTMFunction.apply(True, torch.is_grad_enabled(), a, *L._lstm_params(m), dev,
                                      min(max(lens), T))

    native = lambda: run(trimmed, lstm, x, gout)
    native.eager = lambda: run(lambda a, m: L.bilstm(a, m, lens), lstm, x, gout)
    return (native, (lambda: run(packed, ref, xb, gb)),
            (lambda: run(lambda a, m: L.bilstm(a, m, dev), lstm, x, gout)))


def _etime(fn, iters=5):
    """Event-timed eager calls (microseconds, median): only where a cell cannot be captured."""
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


def _time(fn, how):
    from gtime import gtime
    if how[0] == 'graph':
        try:
            return gtime(fn, reps=2, iters=5)
        except Exception as e:      # e.g. a library call that is not capturable
            import torch
            torch.cuda.synchronize()
            how[0] = 'eager events (capture failed: %s)' % type(e).__name__
    return _etime(fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r8', 'lstm', 'lstm_bench.jsonl'))
    ap.add_argument('--quick', action='store_true', help='B=32 layer 1 only, one round')
    ap.add_argument('--only', default='', help='comma-separated shape names')
    ap.add_argument('--lengths', choices=('none', 'full', 'uniform'), default='none')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    import torch
    shapes = SHAPES[:1] if args.quick else SHAPES
    if args.only:
        shapes = [s for s in SHAPES if s[0] in args.only.split(',')]
    rounds = 1 if args.quick else ROUNDS
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        for name, T, B, F, H in shapes:
            for train in (False, True):
                lens = _lens(args.lengths, T, B, args.seed)
                native, torch_ref, native_dev = _runners(T, B, F, H, train, lens)
                tn, tt, td, en, et = [], [], [], [], []
                hn, ht, hd = ['graph'], ['graph'], ['graph']
                for _ in range(rounds):
                    tn.append(_time(native, hn))
                    tt.append(_time(torch_ref, ht))
                    if native_dev is not None:
                        td.append(_time(native_dev, hd))
                        en.append(_etime(native.eager))
                        et.append(_etime(torch_ref))
                rec = {'shape': name, 'T': T, 'B': B, 'F': F, 'H': H,
                       'mode': 'fwd_bwd' if train else 'fwd', 'native_timing': hn[0],
                       'torch_timing': ht[0],
                       'native_us': round(statistics.median(tn), 1),
                       'torch_bf16_us': round(statistics.median(tt), 1),
                       'native_all_us': [round(v, 1) for v in tn],
                       'torch_all_us': [round(v, 1) for v in tt],
                       'device': torch.cuda.get_device_name(0)}
                rec['native_over_torch'] = round(rec['native_us'] / rec['torch_bf16_us'], 3)
                if lens is not None:
                    rec.update({'lengths': args.lengths, 'seed': args.seed, 'max_len': max(lens),
                                'mean_len': round(sum(lens) / len(lens), 1),
                                'native_device_lengths_us': round(statistics.median(td), 1),
                                'native_device_lengths_timing': hd[0],
                                'native_eager_us': round(statistics.median(en), 1),
                                'torch_eager_us': round(statistics.median(et), 1)})
                    rec['native_over_torch_eager'] = round(rec['native_eager_us'] / rec['torch_eager_us'], 3)
                line = json.dumps(rec)
                print(line, flush=True)
                fh.write(line + '\n')
                fh.flush()
                del native, torch_ref, native_dev
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
