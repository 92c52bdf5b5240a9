"""Global-norm gradient clipping, CPU side: the config field, the argument checks, the eager
trainer's clipped step against ``torch.nn.utils.clip_grad_norm_`` and the Python mirror of the
norm launch's arithmetic (``mercury_amd.ops.optim.grad_norm_plan`` / ``grad_norm_ranges``)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mercury_amd.config import Config
from mercury_amd.importance import pool as ispool
from mercury_amd.ops import optim as O
from mercury_amd.trainer import Trainer
from mercury_amd.utils import Accuracy, Average, EMAverage


def gpu_sizes():
    """The sizes the GPU tests run (tests/test_grad_clip_gpu.py), from the mirror."""
    return O.grad_norm_edge_sizes()


def test_config_round_trip():
    assert Config().clip_grad_norm == 0.0
    c = Config.from_args(['--clip-grad-norm', '0.25'])
    assert c.clip_grad_norm == 0.25 and isinstance(c.clip_grad_norm, float)
    assert Config.from_args([]).clip_grad_norm == 0.0
    assert Config(clip_grad_norm=2.0).to_dict()['clip_grad_norm'] == 2.0


@pytest.mark.parametrize('bad', [-1.0, -1e-9, float('nan'), float('-inf')])
def test_flat_optimizer_refuses_bad_max_norm_before_the_library_loads(bad, monkeypatch):
    from mercury_amd import ops

    def no_lib():
        raise AssertionError('the extension must not be touched before the argument check')
    monkeypatch.setattr(ops, 'lib', no_lib)
    monkeypatch.setattr(O, 'lib', no_lib)
    with pytest.raises(ValueError, match='clip_grad_norm'):
        ops.FlatOptimizer([dict(off=0, numel=4, kind=0)], 4, 'cpu', clip_grad_norm=bad)
    with pytest.raises(ValueError, match='clip_grad_norm'):
        Trainer(nn.Linear(4, 2), None, None, None, None, 'cpu', Config(clip_grad_norm=bad))


def test_check_max_norm_values():
    assert O.check_max_norm(None) == 0.0 and O.check_max_norm(0) == 0.0
    assert O.check_max_norm(1.5) == 1.5 and O.check_max_norm(float('inf')) == math.inf


# ---------------------------------------------------------------- eager trainer
class _Loader:
    def __init__(self, shape, classes, n=3, b=8, seed=5):
        g = torch.Generator().manual_seed(seed)
        self.batches = [(torch.arange(i * b, (i + 1) * b), torch.randn(b, *shape, generator=g),
                         torch.randint(0, classes, (b,), generator=g)) for i in range(n)]
        self.batch_size = b

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _linear():
    return nn.Linear(16, 5), (16,), 5


def _lstm():
    from mercury_amd.models import MyLSTM
    return MyLSTM(8, 6, hidden_dim=32, dropout=0.0, cell='torch'), (1, 8, 12), 6


_OPTS = {'sgd': lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-3),
         'adam': lambda ps: torch.optim.Adam(ps, lr=1e-2)}


def _ordered(t):
    """fp32 bit patterns as integers that are monotone in the value: |difference| = ulps."""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7fffffff), i)


def _step_pair(make, opt, c):
    """One Trainer.train_step with clip_grad_norm=c, and the manual reference: the same forward
    and backward on a copy, clip_grad_norm_ (c > 0), the same optimizer step.  Returns
    (trainer parameters, reference parameters, reference gradient norm, trainer)."""
    torch.manual_seed(3)
    net, shape, classes = make()
    ref = copy.deepcopy(net)
    loader = _Loader(shape, classes)
    t = Trainer(net, _OPTS[opt](net.parameters()), loader, loader, None, 'cpu',
                Config(print_every=0, eval_every=0, clip_grad_norm=c))
    ema = EMAverage()
    torch.manual_seed(4)
    probs, data, label, _, _ = t.update_samples(ema)
    t.train_step(probs, data, label, ema, Average(), Accuracy())
    ropt = _OPTS[opt](ref.parameters())
    losses = F.cross_entropy(ref(data).float(), label, reduction='none')
    ispool.weighted_loss(losses, probs).backward()
    params = [p for p in ref.parameters() if p.requires_grad]
    if c:
        norm = float(torch.nn.utils.clip_grad_norm_(params, c))
    else:
        norm = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in params])))
    ropt.step()
    return t.flat.data.detach(), torch.cat([p.detach().reshape(-1) for p in params]), norm, t


@pytest.mark.parametrize('make,opt', [(_linear, 'sgd'), (_linear, 'adam'), (_lstm, 'sgd')])
def test_eager_trainer_clipped_step_matches_clip_grad_norm(make, opt):
    c = 0.05
    got, want, norm, t = _step_pair(make, opt, c)
    assert norm > c, 'the case must clip: reference norm %g <= c' % norm
    ulps = (_ordered(got) - _ordered(want)).abs().max().item()
    print('clipped step: reference norm %.6g, max |ulp| %d' % (norm, ulps))
    assert ulps <= 1
    assert abs(float(t._grad_norm) - norm) <= 1e-6 * norm
    # and clipping did something: the unclipped step differs
    unclipped, _, _, _ = _step_pair(make, opt, 0.0)
    assert not torch.equal(unclipped, got)


@pytest.mark.parametrize('make,opt', [(_linear, 'sgd'), (_lstm, 'sgd')])
def test_eager_trainer_inactive_clip_is_bit_equal_to_unclipped(make, opt):
    got, want, norm, _ = _step_pair(make, opt, 1e3)
    assert norm < 1e3
    unclipped, _, _, t0 = _step_pair(make, opt, 0.0)
    assert t0._grad_norm is None
    assert torch.equal(got, unclipped)
    assert (_ordered(got) - _ordered(want)).abs().max().item() <= 1


# ---------------------------------------------------------------- launch mirror
@pytest.mark.parametrize('n', gpu_sizes() + [2, 7, O.GN_BLOCK_SPAN // 2 + 1, 3 * O.GN_GRID_SPAN])
def test_mirror_covers_the_range_exactly_once(n):
    pl = O.grad_norm_plan(n)
    assert pl['n4'] * 4 + pl['tail'] == n and 0 <= pl['tail'] < 4
    assert 1 <= pl['blocks'] <= O.GN_CAP
    # the grid is no larger than the work, and the trips cover it
    assert (pl['blocks'] - 1) * O.GN_BLOCK_SPAN < max(pl['n4'] * 4, 1)
    assert pl['trips'] * pl['blocks'] * O.GN_BLOCK_SPAN >= pl['n4'] * 4
    assert (pl['trips'] - 1) * pl['blocks'] * O.GN_BLOCK_SPAN < max(pl['n4'] * 4, 1)
    cover = np.zeros(n + 1, dtype=np.int64)
    rows = O.grad_norm_ranges(n)
    for lo, hi in rows:
        assert 0 <= lo < hi <= n
        cover[lo] += 1
        cover[hi] -= 1
    assert (np.cumsum(cover)[:n] == 1).all()
    # the longest chain: every thread does GN_U float4s per trip
    assert pl['chain'] == pl['trips'] * O.GN_U * 4 + pl['tail']


def test_mirror_sizes_take_every_path():
    b, g = O.GN_BLOCK_SPAN, O.GN_GRID_SPAN
    plans = {n: O.grad_norm_plan(n) for n in gpu_sizes()}
    assert plans[1]['n4'] == 0 and plans[1]['trips'] == 0 and plans[1]['blocks'] == 1
    assert plans[b - 1]['blocks'] == 1 and plans[b]['blocks'] == 1 and plans[b + 1]['blocks'] == 1
    assert plans[b + 1]['tail'] == 1 and plans[b - 1]['tail'] == 3
    assert O.grad_norm_plan(b + 4)['blocks'] == 2
    assert plans[g + 4]['blocks'] == O.GN_CAP and plans[g + 4]['trips'] == 2
    big = plans[2 * g + 7]
    assert big['n'] % 4 == 3 and big['trips'] == 3 and big['blocks'] == O.GN_CAP
    with pytest.raises(ValueError):
        O.grad_norm_plan(0)
