"""Metric meters.

Host meters keep the reference field names and string formats
(`util.py:183-238`: ``Average``, ``EMAverage``, ``Accuracy``).  The reference
syncs the device on every ``update`` (``.item()`` in ``Accuracy.update``,
``util.py:228``); here ``Accuracy`` and ``Average`` accept device tensors and
keep them on device until someone reads ``.accuracy`` / ``.average`` -- the
hot loop never forces a device->host sync.  The native engine's graph-captured
form is its fixed ``meters`` buffer (engine/native.py): kernels accumulate into
it and it is read back only at log cadence (``read_meters``).
"""
from __future__ import annotations

import torch


def _to_float(v):
    if torch.is_tensor(v):
        return float(v.detach().float().item())
    return float(v)


class Average(object):
    """Weighted running mean (`util.py:183-199`)."""

    def __init__(self):
        self.sum = 0
        self.count = 0

    def update(self, value, number):
        # value may be a device scalar: accumulate lazily, no sync here.
        if torch.is_tensor(value):
            value = value.detach()
        self.sum = self.sum + value * number
        self.count += number

    @property
    def average(self):
        return _to_float(self.sum) / self.count

    def __str__(self):
        return '{:.6f}'.format(self.average)


class EMAverage(object):
    """Exponential moving average, first update sets the value (`util.py:200-214`)."""

    def __init__(self, alpha=0.9):
        self.first_update = True
        self.value = 0
        self.alpha = alpha

    def update(self, value):
        if self.first_update:
            self.value = value
            self.first_update = False
        else:
            self.value = self.alpha * self.value + (1 - self.alpha) * value

    def state_dict(self):
        v = self.value
        return {'first_update': self.first_update,
                'value': _to_float(v) if torch.is_tensor(v) or isinstance(v, float) else v,
                'alpha': self.alpha}

    def load_state_dict(self, sd):
        self.first_update = sd['first_update']
        self.value = sd['value']
        self.alpha = sd['alpha']

    def __str__(self):
        return '{:.6f}'.format(_to_float(self.value))


def check_topk(topk, classes=None):
    """``topk`` as an int: 0 (off) or k >= 1, at most ``classes`` where that is known."""
    k = int(topk)
    if k != topk or k < 0:
        raise ValueError('topk must be an integer >= 0 (0 = off), got %r' % (topk,))
    if classes is not None and k > classes:
        raise ValueError('topk = %d exceeds the %d classes' % (k, classes))
    return k


def check_label_smoothing(s):
    """``label_smoothing`` as a float in [0, 1) (F.cross_entropy's meaning); NaN is refused."""
    s = float(s)
    if not 0.0 <= s < 1.0:
        raise ValueError('label_smoothing must be in [0, 1), got %r' % (s,))
    return s


def topk_hits(output, label, k):
    """Per-sample top-k hit by the rank of the label's logit, the classifier-head kernel's rule:
    rank = #{j : z[j] > z[y]} + #{j < y : z[j] == z[y]} (the lower index wins a tie, so rank 0
    is "argmax == y"); a hit iff z[y] is not NaN and rank < k.  ``torch.topk`` leaves ties
    unspecified and is not used."""
    z = output.detach()
    y = label.detach().long()
    zy = z.gather(1, y[:, None])
    below = torch.arange(z.size(1), device=z.device)[None, :] < y[:, None]
    rank = ((z > zy) | ((z == zy) & below)).sum(1)
    return (zy[:, 0] == zy[:, 0]) & (rank < k)


class Accuracy(object):
    """Top-1 accuracy (`util.py:216-238`), device-resident correct count.  ``topk`` = k >= 1 also
    counts top-k hits (``topk_hits``), read as ``accuracy_k``."""

    def __init__(self, topk=0):
        self.correct = 0
        self.count = 0
        self.topk = check_topk(topk)
        self.correct_k = 0

    def update(self, output, label):
        predictions = output.detach().argmax(dim=1)
        correct = predictions.eq(label.detach()).sum()  # stays on device
        self.correct = self.correct + correct
        self.count += output.size(0)
        if self.topk:
            self.correct_k = self.correct_k + topk_hits(output, label, self.topk).sum()

    def update_counts(self, correct, count, correct_k=None):
        self.correct = self.correct + correct
        self.count += count
        if correct_k is not None:
            self.correct_k = self.correct_k + correct_k

    @property
    def accuracy(self):
        return _to_float(self.correct) / max(self.count, 1)

    @property
    def accuracy_k(self):
        return _to_float(self.correct_k) / max(self.count, 1)

    def __str__(self):
        return '{:.2f}%'.format(self.accuracy * 100)
