"""Device time per step of the BiLSTM step kernels alone (csrc/lstm.hip), graph-timed.

All T = 161 steps of a layer (H = 512) are captured and replayed; the time is divided by T, so
it includes the dependent launch boundary every step pays.  Run on the shipped build, or on an
A/B build that sets the kernels' build-time knobs, to reproduce the tiles-per-wave and
backward-grouping figures quoted in csrc/lstm.hip and the README:

    MERCURY_VARIANT_FLAGS="-DLSTM_TILES_PER_WAVE=2 -DLSTM_BWD_U=4" \\
        python bench/build_variant.py HEAD /tmp/v.so
    MERCURY_EXT_PATH=/tmp/v.so python bench/lstm_step_probe.py --label tiles2_u4

``--gemm`` also times the forms of the time-batched pre GEMM x . W_ih^T (bf16 operands with an
fp32 result, fp32 operands, bf16 result) and the [T][B][2][4H] -> [T][2][B][4H] copy.
``--lengths full`` / ``uniform`` times the kernels with a device lengths tensor: all rows of
length T, or lengths uniform in [T/2, T] (``--seed``); ``uniform`` also times the launches cut
to max(len_b) steps, as host-side lengths run them (still divided by T).  A build with
``-DLSTM_NO_WAVE_SKIP`` keeps all-padded waves in the K loop, for what the skip buys.
One JSON line per run, appended to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='shipped')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r8', 'lstm', 'step_probe.jsonl'))
    ap.add_argument('--gemm', action='store_true')
    ap.add_argument('--lengths', choices=('none', 'full', 'uniform'), default='none')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    import torch
    from gtime import gtime
    from mercury_amd.ops import lstm as L
    T, H = 161, 512
    bf = torch.bfloat16
    res = {'label': args.label, 'T': T, 'H': H, 'unit': 'us per step (graph replay of T steps / T)',
           'lengths': args.lengths}
    for B in (32, 320):
        kw, Te = {}, T
        if args.lengths != 'none':
            g = torch.Generator().manual_seed(args.seed)
            lens = (torch.full((B,), T) if args.lengths == 'full'
                    else torch.randint(T // 2, T + 1, (B,), generator=g))
            kw = {'lengths': lens.to('cuda', torch.int32)}
            Te = int(lens.max())
            res['max_len_B%d' % B], res['mean_len_B%d' % B] = Te, round(float(lens.float().mean()), 1)
        pre = torch.randn(T, 2, B, 4 * H, device='cuda')
        whh = (torch.randn(2, 4 * H, H, device='cuda') / H ** 0.5).to(bf)
        whhT = whh.transpose(1, 2).contiguous()
        out = torch.empty(T, B, 2 * H, dtype=bf, device='cuda')
        c = torch.empty(T, 2, B, H, device='cuda')
        c1 = torch.empty(1, 2, B, H, device='cuda')
        gates = torch.empty(T, 2, B, 4 * H, dtype=bf, device='cuda')
        dout = torch.randn(T, B, 2 * H, device='cuda')
        dG = torch.empty_like(gates)
        dc = torch.empty(2, B, H, device='cuda')
        runs = {'fwd_train': lambda: L.lstm_step_fwd(pre, whh, out, c, gates, T=T, B=B, H=H, **kw),
                'fwd_infer': lambda: L.lstm_step_fwd(pre, whh, out, c1, None, T=T, B=B, H=H, **kw),
                'bwd': lambda: L.lstm_step_bwd(dout, gates, c, whhT, dG, dc, T=T, B=B, H=H, **kw)}
        if Te < T:
            runs.update({
                'fwd_train_trim': lambda: L.lstm_step_fwd(pre, whh, out, c, gates, T=Te, B=B, H=H, **kw),
                'fwd_infer_trim': lambda: L.lstm_step_fwd(pre, whh, out, c1, None, T=Te, B=B, H=H, **kw),
                'bwd_trim': lambda: L.lstm_step_bwd(dout, gates, c, whhT, dG, dc, T=Te, B=B, H=H, **kw)})
        for k, fn in runs.items():
            res['%s_B%d' % (k, B)] = round(gtime(fn, reps=2, iters=5) / T, 2)
        if args.gemm:
            for F in (101, 1024):
                xb = torch.randn(T * B, F, device='cuda').to(bf)
                w = torch.randn(8 * H, F, device='cuda').to(bf)
                xf, wf = xb.float(), w.float()
                tag = 'B%d_F%d_us' % (B, F)
                res['mm_bf16_f32out_' + tag] = round(gtime(
                    lambda: torch.mm(xb, w.t(), out_dtype=torch.float32), reps=2, iters=5), 1)
                res['mm_fp32_' + tag] = round(gtime(lambda: torch.matmul(xf, wf.t()), reps=2, iters=5), 1)
                res['mm_bf16_' + tag] = round(gtime(lambda: torch.mm(xb, w.t()), reps=2, iters=5), 1)
            o32 = torch.empty(T * B, 8 * H, device='cuda')
            res['permute_copy_B%d_us' % B] = round(gtime(
                lambda: o32.view(T, B, 2, 4 * H).permute(0, 2, 1, 3).contiguous(), reps=2, iters=5), 1)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
