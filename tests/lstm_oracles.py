"""References shared by test_lstm.py and test_lstm_gpu.py (a helper module: no tests).

Three runs of one bidirectional layer on the same bf16-rounded weights, inputs and upstream
gradient: ``ref64`` (fp64 ``nn.LSTM`` on the CPU, the oracle), ``torch_bf16`` (``nn.LSTM`` cast
to bf16 on the CPU: deterministic, independent of MIOpen; its distance to the oracle is the
yardstick) and ``run`` (``emulate`` or the native cell).  Each returns ``[out, dx, 8 parameter
gradients]`` as fp64 CPU tensors.  ``assert_vs_bf16`` holds a result to

    ||got - ref|| <= 2.5 * ||torch_bf16 - ref||      (the factor tests/test_native_gpu.py uses)

for every one of the ten tensors.
"""
import copy
import functools

import torch
import torch.nn as nn

from mercury_amd.ops.lstm import _PARAMS

FACTOR = 2.5
NAMES = ('out', 'dx') + _PARAMS


def rbf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def make_lstm(F, H, seed):
    torch.manual_seed(seed)
    m = nn.LSTM(F, H, num_layers=1, bidirectional=True)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(rbf(p))
    return m


def make_io(T, B, F, H, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return rbf(torch.randn(T, B, F, generator=g)), rbf(torch.randn(T, B, 2 * H, generator=g))


def _collect(m, x, out):
    return [t.detach().double().cpu() for t in [out, x.grad] + [getattr(m, n).grad for n in _PARAMS]]


def ref64(lstm, x, gout):
    m = copy.deepcopy(lstm).double()
    x = x.double().requires_grad_()
    out = m(x)[0]
    out.backward(gout.double())
    return _collect(m, x, out)


def torch_bf16(lstm, x, gout):
    m = copy.deepcopy(lstm).to(torch.bfloat16)
    x = x.to(torch.bfloat16).requires_grad_()
    out = m(x)[0]
    out.backward(gout.to(torch.bfloat16))
    return _collect(m, x, out)


def run(fn, lstm, x, gout, device='cpu'):
    m = copy.deepcopy(lstm).to(device)
    x = x.detach().clone().to(device).requires_grad_()     # never the cached input itself
    out = fn(x, m)
    out.backward(gout.to(device))
    return _collect(m, x, out)


@functools.lru_cache(maxsize=None)
def case(T, B, F, H, seed=0):
    """(lstm, x, gout, ref64 results, torch_bf16 results) of one shape, computed once."""
    lstm = make_lstm(F, H, seed)
    x, gout = make_io(T, B, F, H, seed)
    return lstm, x, gout, ref64(lstm, x, gout), torch_bf16(lstm, x, gout)


def assert_vs_bf16(got, ref, tb, what='', names=NAMES):
    ratios = {}
    for n, g, r, t in zip(names, got, ref, tb):
        eg, et = float((g - r).norm()), float((t - r).norm())
        ratios[n] = eg / et if et > 0 else (0.0 if eg == 0 else float('inf'))
    print('RATIO %s %s' % (what, ' '.join('%s=%.2f' % kv for kv in ratios.items())))
    bad = {n: v for n, v in ratios.items() if not v <= FACTOR}
    assert not bad, '%s: error above %.1fx torch-bf16: %r' % (what, FACTOR, bad)
    return ratios


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (8 significand bits)."""
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 8)


def assert_close_to_emulate(out, emu, what=''):
    """out within 2 bf16 ulps of emulate for >= 99 % of the elements, and no element further
    than 2^-5 |emu| + 1e-3 (a rounding-boundary flip of one h propagates through the
    recurrence; the 1 % cap is a condition, not a tolerance)."""
    out, emu = out.double().cpu(), emu.double().cpu()
    d = (out - emu).abs()
    frac = float((d <= 2 * bf16_ulp(emu)).double().mean())
    worst = float((d - (2.0 ** -5 * emu.abs() + 1e-3)).max())
    print('EMU %s within-2ulp %.4f worst-over-cap %.3g' % (what, frac, worst))
    assert frac >= 0.99, '%s: only %.4f of the elements within 2 bf16 ulps' % (what, frac)
    assert worst <= 0, '%s: an element is %.3g past 2^-5 |ref| + 1e-3' % (what, worst)
