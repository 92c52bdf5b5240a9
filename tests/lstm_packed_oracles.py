"""Packed-sequence references for test_lstm_packed.py (a helper module: no tests).

The runs of ``lstm_oracles`` with ``lengths``: ``ref64`` (fp64 ``nn.LSTM`` on the CPU through
``pack_padded_sequence(enforce_sorted=False)`` / ``pad_packed_sequence(total_length=T)``, the
oracle) and ``torch_bf16`` (the same in bf16 on the CPU, the yardstick).  Each returns ``[out, dx,
8 parameter gradients]`` as fp64 CPU tensors, the ten tensors of ``lstm_oracles.ref64``.  The
inputs carry ``PAD_X`` in ``x`` and ``PAD_G`` in the upstream gradient at every padded frame, so a
recurrence that walks through the padding is far outside the criterion.
"""
import copy
import functools

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_oracles as lo

PAD_X = 7.0
PAD_G = 3.0


def padded(T, lens):
    """[T][B] bool: t >= len_b (len_b clamped to [0, T])."""
    lens = torch.as_tensor(lens).clamp(0, T)
    return torch.arange(T)[:, None] >= lens[None, :]


def seeded_lens(T, B, seed=0):
    """randint(1, T+1) with lens[0] = T and lens[1] = 1: the longest and the shortest row."""
    g = torch.Generator().manual_seed(seed + 77)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0], lens[1] = T, 1
    return [int(v) for v in lens]


def make_io(T, B, F, H, lens, seed=0, pad_x=PAD_X, pad_g=PAD_G):
    x, gout = lo.make_io(T, B, F, H, seed)
    pad = padded(T, lens)
    x, gout = x.clone(), gout.clone()
    x[pad] = pad_x
    gout[pad] = pad_g
    return x, gout


def _packed(m, x, lens):
    T = x.shape[0]
    pk = pack_padded_sequence(x, torch.as_tensor(lens, dtype=torch.int64), enforce_sorted=False)
    return pad_packed_sequence(m(pk)[0], total_length=T)[0]


def ref64(lstm, x, gout, lens):
    m = copy.deepcopy(lstm).double()
    x = x.double().requires_grad_()
    out = _packed(m, x, lens)
    out.backward(gout.double())
    return lo._collect(m, x, out)


def torch_bf16(lstm, x, gout, lens):
    m = copy.deepcopy(lstm).to(torch.bfloat16)
    x = x.to(torch.bfloat16).requires_grad_()
    out = _packed(m, x, lens)
    out.backward(gout.to(torch.bfloat16))
    return lo._collect(m, x, out)


def run(fn, lstm, x, gout, lens):
    """``fn(lstm, x, lens)`` -> out on a private copy of the module, then its ten tensors."""
    m = copy.deepcopy(lstm)
    x = x.detach().clone().requires_grad_()
    out = fn(m, x, lens)
    out.backward(gout)
    return lo._collect(m, x, out)


@functools.lru_cache(maxsize=None)
def case(T, B, F, H, lens, seed=0):
    """(lstm, x, gout, ref64 results, torch_bf16 results) of one shape, computed once; ``lens``
    a tuple.  The references see a finite upstream gradient (PAD_G) at padded frames: pack/unpack
    drops it, so they are also the references of a run whose padded gradient is NaN."""
    lstm = lo.make_lstm(F, H, seed)
    x, gout = make_io(T, B, F, H, lens, seed)
    lens = list(lens)
    return lstm, x, gout, ref64(lstm, x, gout, lens), torch_bf16(lstm, x, gout, lens)
