"""Inputs and whole-head references shared by test_fc_head.py and test_fc_head_gpu.py (a helper
module: no tests).  ``chain`` runs the torch modules themselves in a dtype (fp64: the oracle;
bf16 on the CPU: the yardstick of ``lstm_oracles.assert_vs_bf16``) with explicit keep-masks and
returns ``NAMES`` as fp64 CPU tensors; ``run`` does the same through ``fc_head`` / ``emulate``."""
import copy
import functools

import torch
import torch.nn as nn

from kernel_oracles import gen, rbf

NAMES = ('logits', 'dz', 'dW1', 'db1', 'dgamma', 'dbeta', 'dW2', 'db2')
P = 0.5


@functools.lru_cache(maxsize=None)
def case(B, K, N, C):
    """(fc1, fc2, z, dlogits, (m0, m1)): bf16-valued parameters and inputs, gamma of magnitude
    [0.5, 1.5] with a quarter negative, running statistics away from their initial (0, 1)."""
    g = gen(B + K + N + C)
    torch.manual_seed(B + K + N + C)
    fc1, fc2 = nn.Sequential(nn.Linear(K, N), nn.BatchNorm1d(N), nn.ReLU()), nn.Linear(N, C)
    with torch.no_grad():
        fc1[1].weight.copy_(torch.rand(N, generator=g) + 0.5)
        fc1[1].weight[1::4] *= -1
        fc1[1].bias.copy_(torch.randn(N, generator=g) * 0.5)
        fc1[1].running_mean.copy_(torch.randn(N, generator=g) * 0.1)
        fc1[1].running_var.copy_(torch.rand(N, generator=g) * 0.5 + 0.1)
        for p in list(fc1.parameters()) + list(fc2.parameters()):
            p.copy_(rbf(p))
    z, d = rbf(torch.randn(B, K, generator=g)), rbf(torch.randn(B, C, generator=g))
    masks = tuple((torch.rand(B, W, generator=g) >= P).to(torch.uint8) for W in (K, N))
    return fc1, fc2, z, d, masks


def _collect(out, z, f1, f2):
    ts = (out, z.grad, f1[0].weight.grad, f1[0].bias.grad, f1[1].weight.grad, f1[1].bias.grad,
          f2.weight.grad, f2.bias.grad)
    return [t.detach().double().cpu() for t in ts]


def chain(fc1, fc2, z, d, masks, training, dtype):
    f1, f2 = copy.deepcopy(fc1).to(dtype).train(training), copy.deepcopy(fc2).to(dtype)
    z = z.to(dtype).requires_grad_()
    k0, k1 = (m.to(dtype) / (1 - P) for m in masks) if masks else (1, 1)
    out = f2(f1(z * k0) * k1)
    out.backward(d.to(dtype))
    return _collect(out, z, f1, f2)


def run(fn, fc1, fc2, z, d, masks, training, device='cpu'):
    f1, f2 = copy.deepcopy(fc1).to(device).train(training), copy.deepcopy(fc2).to(device)
    z = z.clone().to(device).requires_grad_()
    out = fn(z, f1, f2, P if masks else 0.0, training, masks and tuple(m.to(device) for m in masks))
    out.backward(d.to(device))
    return _collect(out, z, f1, f2)
