"""Per-block phase stamps of the pair launches' dgrad half (a -DMERCURY_STAMPS build).

    MERCURY_VARIANT_FLAGS=-DMERCURY_STAMPS python bench/build_variant.py HEAD OUT.so [files...]
    MERCURY_EXT_PATH=OUT.so python bench/stamp_dgrad_epi.py

Runs conv_bwd (dgrad + wgrad pair, fused BN-backward sums, default plans) on the four ResNet-18
CIFAR train-batch layer shapes, accumulating and not, and prints the median over the dgrad
blocks that ran the epilogue of, in s_memtime ticks:

    loop    entry -> main loop done            (stamps 0 -> 2)
    finish  main loop done -> epilogue done    (2 -> 3)
    f8      ... -> ticket, slab reads, LDS sums zeroed, first barrier   (2 -> 8)
    f9      accumulators staged into LDS       (8 -> 9)
    f10     second barrier                     (9 -> 10)
    rows    row loop, reduction, atomics       (10 -> 3)

A K-split block that did not win its tile's ticket never reaches stamp 3 and is left out.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import ops                                   # noqa: E402
from mercury_amd.ops import bn as bnops                       # noqa: E402
from mercury_amd.ops.conv import ConvSpec, dgrad_plan         # noqa: E402

DEV = 'cuda'
NB = 8192
CASES = [('layer1 64->64 32x32', (32, 32, 32, 64, 64, 3, 3, 1, 1)),
         ('layer2 128->128 16x16', (32, 16, 16, 128, 128, 3, 3, 1, 1)),
         ('layer3 256->256 8x8', (32, 8, 8, 256, 256, 3, 3, 1, 1)),
         ('layer4 512->512 4x4', (32, 4, 4, 512, 512, 3, 3, 1, 1))]


def stamps():
    v = ops.lib().igemm_stamps(NB)
    if not v:
        sys.exit('not a MERCURY_STAMPS build')
    return torch.tensor(v, dtype=torch.int64).view(NB, 12)


def main():
    ops.lib()
    print('%-24s %3s %-14s %6s | %7s %7s %7s %7s %7s %7s' % (
        'case', 'acc', 'dgrad plan', 'blocks', 'loop', 'finish', 'f8', 'f9', 'f10', 'rows'))
    for name, case in CASES:
        spec = ConvSpec(*case)
        Mx, C = spec.N * spec.H * spec.W, spec.Cp
        g = torch.Generator(device='cpu').manual_seed(3)
        rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(DEV)
        dy, wt, x = rnd(spec.M, spec.K), rnd(C * 9 * spec.K), rnd(Mx, C)
        out, y = rnd(Mx, C), rnd(Mx, C)
        stats = torch.stack([y.float().sum(0), (y.float() ** 2).sum(0)]).contiguous()
        for acc in (False, True):
            dx = rnd(Mx, C)
            dw = torch.zeros(spec.K * 9 * spec.C, device=DEV)
            bw = dict(out=out, y=y, stats=stats, act='relu',
                      sums=torch.zeros(bnops.sums_numel(C), device=DEV))
            before = None
            for it in range(6):
                if it == 5:
                    torch.cuda.synchronize()
                    before = stamps()
                dw.zero_()
                ops.conv_bwd(dy, wt, dx, x, dw, spec, accumulate=acc, bw=bw)
            torch.cuda.synchronize()
            s = stamps()
            ran = ((s[:, [2, 3, 8, 9, 10]] != before[:, [2, 3, 8, 9, 10]]).all(1) &
                   (s[:, 3] > s[:, 2]) & (s[:, 2] > s[:, 0]))
            r = s[ran]
            if not len(r):
                print('%-24s %3d no stamped blocks' % (name, acc))
                continue
            med = lambda a, b: statistics.median((r[:, a] - r[:, b]).tolist())
            print('%-24s %3d %-14s %6d | %7.0f %7.0f %7.0f %7.0f %7.0f %7.0f' % (
                name, acc, str(dgrad_plan(spec)), len(r), med(2, 0), med(3, 2), med(8, 2),
                med(9, 8), med(10, 9), med(3, 10)))


if __name__ == '__main__':
    main()
