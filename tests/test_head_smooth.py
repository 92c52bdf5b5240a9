"""Label smoothing and top-k accuracy, CPU side: the oracle of ``head_smooth_oracles`` against
``F.cross_entropy(label_smoothing=s)`` (forward and autograd, fp64), the zero-ambiguity
condition its top-k cases rest on, ``Accuracy(topk=k)``'s rank rule, the config fields and one
eager ``Trainer.train_step``."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import head_smooth_oracles as hs
import kernel_oracles as ko

F64 = torch.float64


@pytest.mark.parametrize('ci', range(len(hs.CASES)))
@pytest.mark.parametrize('s', hs.SMOOTH + [0.0])
def test_oracle_equals_torch_cross_entropy(ci, s):
    c = hs.case(ci, 2)
    r, label = c['ref'], c['label'].long()
    o = hs.smooth_ref(r, label, s)
    z = r['logits'].clone().requires_grad_(True)
    want = F.cross_entropy(z, label, reduction='none', label_smoothing=s)
    assert float((o['loss'] - want.detach()).abs().max()) <= 1e-12
    # the IS-weighted mean: sum_b loss_b / (B w_b)
    (want * r['scale']).sum().backward()
    assert float((o['dlogits'] - z.grad).abs().max()) <= 1e-12
    assert abs(o['meter0'][0] - float((want.detach() * r['scale']).sum()) * c['B']) <= 1e-9
    if s == 0.0:
        assert float((o['dlogits'] - r['dlogits']).abs().max()) <= 1e-15
        assert float((o['loss'] - r['losses']).abs().max()) == 0.0


def _no_ambiguity(logits, T, k, tag):
    label = hs.rank_labels(logits, k)
    lo, hi, amb = hs.topk_bounds(logits, label, T, k)
    assert not bool(amb.any()) and lo == hi, (tag, k, lo, hi)
    rank = hs.rank_ref(logits, label)[0]
    B = logits.shape[0]
    assert rank.tolist() == [(b % (k + 2)) % logits.shape[1] for b in range(B)], (tag, k)
    assert lo == int((rank < k).sum())
    return lo


@pytest.mark.parametrize('ci', range(len(hs.CASES)))
def test_rank_chosen_labels_leave_no_ambiguous_sample(ci):
    """Every case the GPU tests run, for every k: no sample within 2 T of the boundary, so the
    expected top-k count is one number; and (B > 1) it is neither 0 nor B."""
    for k in hs.TOPK:
        c = hs.case(ci, k)
        if k > c['K']:
            continue
        lo = _no_ambiguity(c['ref']['logits'], c['ref']['T'], k, hs.CASES[ci])
        assert c['topk'][:2] == (lo, lo)
        if c['B'] > k:
            assert 0 < lo < c['B'], (hs.CASES[ci], k, lo)


@pytest.mark.parametrize('shape', [(5, 16, 512, 10), (5, 1, 1280, 100)] +
                         [s[:4] for s in ko.HEAD_CHUNK_CASES + ko.HEAD_WIDE_CASES])
def test_no_ambiguity_on_the_head_test_shapes(shape):
    """The same condition on the shapes of tests/test_head_paths_gpu.py."""
    act, w, b, label, isw = ko.head_case(*shape)
    r = ko.head_ref(act, w, b, label, isw)
    for k in hs.TOPK:
        _no_ambiguity(r['logits'], r['T'], k, shape)


# ------------------------------------------------------------------------------ Accuracy
def test_accuracy_topk_follows_the_rank_rule_on_a_tie():
    from mercury_amd.utils.meters import Accuracy, topk_hits
    z = torch.tensor([[0.5, 2.0, -1.0, 2.0, 0.0]])
    second, first = torch.tensor([3]), torch.tensor([1])
    for k, hit2, hit1 in ((1, 0, 1), (2, 1, 1), (5, 1, 1)):
        a = Accuracy(topk=k)
        a.update(z, second)
        assert float(a.correct_k) == hit2 and a.accuracy_k == hit2, k
        a = Accuracy(topk=k)
        a.update(z, first)
        assert float(a.correct_k) == hit1, k
    # top-1 by the rank rule is the argmax rule: the first maximum wins
    assert int(z.argmax(1)) == 1 and not bool(topk_hits(z, second, 1)) and bool(topk_hits(z, first, 1))
    # a label whose logit is the third largest
    y = torch.tensor([0])
    assert not bool(topk_hits(z, y, 2)) and bool(topk_hits(z, y, 3))


def test_accuracy_topk_nan_label_logit_is_no_hit():
    from mercury_amd.utils.meters import Accuracy
    nan = float('nan')
    z = torch.tensor([[nan, 1.0, 0.0], [2.0, nan, 0.0], [0.0, 1.0, 2.0]])
    y = torch.tensor([0, 0, 2])
    a = Accuracy(topk=3)
    a.update(z, y)
    # sample 0: its own logit is NaN -> no hit although nothing compares above it; sample 1:
    # another class's NaN is not above the label; sample 2: a plain hit
    assert float(a.correct_k) == 2.0 and a.count == 3
    assert abs(a.accuracy_k - 2 / 3) < 1e-12


def test_accuracy_default_is_unchanged():
    from mercury_amd.utils.meters import Accuracy
    a = Accuracy()
    a.update(torch.tensor([[0.0, 1.0], [1.0, 0.0]]), torch.tensor([1, 1]))
    assert str(a) == '50.00%' and a.accuracy == 0.5 and a.topk == 0 and a.accuracy_k == 0.0
    a.update_counts(2, 2)
    assert str(a) == '75.00%'
    b = Accuracy(topk=5)
    b.update_counts(1, 4, 3)
    assert str(b) == '25.00%' and b.accuracy_k == 0.75
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            Accuracy(topk=bad)


# ------------------------------------------------------------------------------ config
def test_config_fields_round_trip_and_defaults():
    from mercury_amd.config import Config
    d = Config()
    assert d.label_smoothing == 0.0 and d.topk == 0
    c = Config.from_args(['--label-smoothing', '0.1', '--topk', '5'])
    assert c.label_smoothing == 0.1 and c.topk == 5
    assert c == Config(label_smoothing=0.1, topk=5)
    assert Config.from_args([]) == d


class _Loader:
    batch_size = 8

    def __init__(self, seed=5):
        g = torch.Generator().manual_seed(seed)
        self.batches = [(torch.arange(i * 8, (i + 1) * 8), torch.randn(8, 16, generator=g),
                         torch.randint(0, 5, (8,), generator=g)) for i in range(3)]

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _trainer(net, **cfg):
    from mercury_amd.config import Config
    from mercury_amd.trainer import Trainer
    return Trainer(net, torch.optim.SGD(net.parameters(), lr=0.1), _Loader(), _Loader(),
                   _Loader(9), 'cpu', Config(print_every=0, eval_every=0, num_classes=5, **cfg))


@pytest.mark.parametrize('bad', [dict(label_smoothing=1.0), dict(label_smoothing=-0.1),
                                 dict(label_smoothing=float('nan')), dict(topk=-1),
                                 dict(topk=6)])
def test_trainer_refuses_bad_values(bad):
    with pytest.raises(ValueError):
        _trainer(nn.Linear(16, 5), **bad)


def test_eager_train_step_smooths_the_training_loss_only():
    from mercury_amd.utils import Accuracy, Average, EMAverage
    s = 0.1
    torch.manual_seed(3)
    net0 = nn.Linear(16, 5)
    net1, ref = copy.deepcopy(net0), copy.deepcopy(net0)
    t0, t1 = _trainer(net0), _trainer(net1, label_smoothing=s, topk=2)
    # scoring and evaluation: the same bits with smoothing on or off
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(8, 16, generator=g), torch.randint(0, 5, (8,), generator=g)
    assert torch.equal(t0._score(net0(x), y), t1._score(net1(x), y))
    e0, e1 = t0.evaluate(), t1.evaluate()
    for a, b in zip(e0, e1):
        va, vb = (a.average, b.average) if hasattr(a, 'average') else (a.accuracy, b.accuracy)
        assert va == vb
    assert e1[1].topk == 2 and e1[1].accuracy_k >= e1[1].accuracy and e0[1].topk == 0
    ema0, ema1 = EMAverage(), EMAverage()
    torch.manual_seed(11)
    b0 = t0.update_samples(ema0)
    torch.manual_seed(11)
    b1 = t1.update_samples(ema1)
    for a, b in zip(b0, b1):
        assert torch.equal(a, b)                 # the same draw: scores are not smoothed
    probs, data, label = b1[0], b1[1], b1[2]
    acc = Accuracy(2)
    _, loss = t1.train_step(probs, data, label, ema1, Average(), acc)
    # by hand: mean_b ((1 - s) (lse - z[y]) + s (lse - mean_k z)) / w_b
    z = ref(data).float()
    lse = torch.logsumexp(z, 1)
    ls = (1 - s) * (lse - z.gather(1, label[:, None])[:, 0]) + s * (lse - z.mean(1))
    want = (ls / probs).mean()
    want.backward()
    loss, want = loss.detach(), want.detach()
    assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    gwant = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
    assert float((t1.flat.grad - gwant).abs().max()) <= 1e-6 * float(gwant.abs().max()) + 1e-7
    # and it is not the plain loss's gradient
    _, loss0 = t0.train_step(b0[0], b0[1], b0[2], ema0, Average(), Accuracy())
    assert abs(float(loss0.detach()) - float(want)) > 1e-3
    assert acc.count == 8 and float(acc.correct_k) >= float(acc.correct)
