"""Reference-semantics oracles from recorded fixtures.

The tests that compare against the reference implementation read what it computed on
fixed inputs from ``tests/golden/*.npz``.  The inputs are built here, by the same code for
the recorder (``oracle/record_golden.py``, which needs a reference tree) and for the tests
(which do not): seeded generators, and model weights stored in the fixture wherever they are
small enough.  The model interchange tests run in float64, so a recorded output holds to
their tolerance on any host.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def golden(name):
    """The fixture ``tests/golden/<name>.npz`` (plain arrays, no pickles)."""
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


class TinyNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3, padding=1)
        self.bn = nn.BatchNorm2d(4)
        self.fc = nn.Linear(4, 10)

    def forward(self, x):
        return self.fc(F.relu(self.bn(self.conv(x))).mean((2, 3)))


class FakeLoader:
    def __init__(self, n=20, b=32, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.batches = [(torch.arange(i * b, (i + 1) * b), torch.randn(b, 3, 8, 8, generator=g),
                         torch.randint(0, 10, (b,), generator=g)) for i in range(n)]
        self.batch_size = b

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class SliceDS:
    def __init__(self, n=100, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(n, 3, 8, 8, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.x)

    def get_slice(self, s, e):
        return self.x[s:e], self.y[s:e]


def state_to_arrays(net, prefix='sd.'):
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def load_state_arrays(net, fixture, prefix='sd.'):
    """Load the weights a fixture holds under ``prefix`` (they are the recorder's)."""
    net.load_state_dict({k[len(prefix):]: torch.from_numpy(fixture[k])
                         for k in fixture.files if k.startswith(prefix)})
    return net


def top_k_draw(p, k, replacement=True, generator=None):
    """Deterministic stand-in for ``torch.multinomial``: the k most probable indices."""
    return torch.argsort(p, descending=True)[:k].repeat(1)


METER_UPDATES = [(1.0, 32), (0.5, 16), (2.0, 8)]
GROUPWISE_SCHEDULE = [(0, 30), (0, 30), (1, 50), (2, 40), (2, 40)]


def meter_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(64, 10, generator=g), torch.randint(0, 10, (64,), generator=g)


def interchange_input(name):
    """Seeded float64 input of the state-dict interchange tests."""
    g = torch.Generator().manual_seed(1)
    shape = (2, 1, 101, 161) if name == 'VGG11' else (2, 3, 32, 32)
    return torch.randn(*shape, generator=g, dtype=torch.float64)
