"""BiLSTM + attention-pooling speech model (`pytorch_model.py:156-242`).

The reference version cannot run (F9): it calls ``pad_packed_sequence`` on a
plain tensor, builds its mask with a hard-coded ``.cuda()`` and feeds the
packed output of layer 1 into layer 2.  This is the repaired model: same
parameter tree (``lstm1``, ``atten1``, ``lstm2``, ``atten2``, ``fc1``, ``fc2``),
optional per-sample ``lengths`` (defaults to full length), a device-agnostic
mask, and layer 2 consuming layer 1's padded output.

``cell`` picks how the two bidirectional layers run: ``'torch'`` (default) is ``nn.LSTM`` on
PyTorch-ROCm (MIOpen RNN); ``'native'`` runs the recurrence in the HIP step kernels of
``csrc/lstm.hip`` (``mercury_amd.ops.lstm``: bf16 operands, fp32 accumulation) and refuses a CPU
input or a hidden size the kernels do not tile; ``'auto'`` takes the native cell only at the
(batch, hidden) sizes where it was measured not slower (``ops.lstm.MEASURED_NATIVE``).  The
parameters are the ``nn.LSTM`` modules' own in every case.

``attn`` picks how the two attention poolings run, in the same three values (``Attention``'s
``impl``): the eager torch chain (default), the HIP kernels of ``csrc/attn.hip``, or those only at
the shapes where they were measured not slower (``ops.attention.MEASURED_NATIVE``).

``packed`` decides whether the two recurrent layers honour ``lengths``.  ``packed=True`` is the
reference's intended model, a packed-sequence model: each layer computes what
``pad_packed_sequence(lstm(pack_padded_sequence(x, lengths, enforce_sorted=False)),
total_length=T)`` computes -- the reverse direction of row b starts at ``t = len_b - 1`` from a
zero state, the layer output is exactly 0 at ``t >= len_b``, and padded frames reach no
gradient.  ``cell='torch'`` does it with pack / ``nn.LSTM`` / unpack.  ``cell='native'`` does it
in the step kernels of ``csrc/lstm.hip``, which take device lengths and mask per row
(``ops.lstm.bilstm(x, lstm, lengths)``: no packing, no host synchronisation); on an input that is
not on a HIP device it is a ``NotImplementedError`` (never a silent walk through the padding,
never a silent switch to torch).  ``cell='auto'`` with lengths takes the native cell only on the
GPU at the (batch, hidden) sizes in ``ops.lstm.MEASURED_NATIVE_PACKED`` and torch elsewhere.  ``packed=False``
(default) is the historical behaviour: ``lengths`` reaches only the two attention poolings and
both recurrences run over the padding.  With ``lengths=None`` the two are the same.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F


_IMPLS = ('torch', 'native', 'auto')


class Attention(nn.Module):
    """Attention pooling over time: ``(representations [B][D], attentions [B][T])``.

    ``impl='torch'`` (default) is the eager chain below.  ``'native'`` runs the HIP kernels of
    ``csrc/attn.hip`` (``mercury_amd.ops.attention.attn_pool``): it refuses a CPU input or an
    unsupported width, and its returned attentions are not differentiable (a caller that
    differentiates through them keeps ``'torch'``).  ``'auto'`` takes the native path only on the
    GPU at the shapes in ``ops.attention.MEASURED_NATIVE``.  The parameter is ``att_weights``
    [1][hidden] in every case."""

    def __init__(self, hidden_size, batch_first=False, impl='torch'):
        super().__init__()
        if impl not in _IMPLS:
            raise ValueError("impl must be 'torch', 'native' or 'auto', got %r" % (impl,))
        self.hidden_size = hidden_size
        self.batch_first = batch_first
        self.impl = impl
        self.att_weights = nn.Parameter(torch.empty(1, hidden_size))
        stdv = 1.0 / math.sqrt(hidden_size)
        nn.init.uniform_(self.att_weights, -stdv, stdv)

    def _native(self, inputs):
        if self.impl == 'torch':
            return None
        from ..ops import attention as native
        if self.impl == 'auto':
            if not inputs.is_cuda or inputs.dim() != 3:
                return None
            B, T = inputs.shape[:2] if self.batch_first else inputs.shape[1::-1]
            if (B, T, inputs.shape[2], inputs.dtype) not in native.MEASURED_NATIVE:
                return None
        return native

    def forward(self, inputs, lengths=None):
        native = self._native(inputs)
        if native is not None:
            x = inputs.transpose(0, 1) if self.batch_first else inputs      # time-major view
            return native.attn_pool(x, self.att_weights, lengths)
        if not self.batch_first:
            inputs = inputs.transpose(0, 1)
        batch_size, max_len = inputs.shape[:2]
        weights = torch.matmul(inputs, self.att_weights.t()).squeeze(-1)   # [B, T]
        attentions = torch.softmax(F.relu(weights), dim=-1)
        if lengths is not None:
            lengths = torch.as_tensor(lengths, device=inputs.device)
            mask = (torch.arange(max_len, device=inputs.device)[None, :] < lengths[:, None])
            attentions = attentions * mask.to(attentions.dtype)
            attentions = attentions / attentions.sum(-1, keepdim=True).clamp_min(1e-12)
        representations = (inputs * attentions.unsqueeze(-1)).sum(1)
        return representations, attentions


class MyLSTM(nn.Module):
    def __init__(self, feature_dim, num_classes, hidden_dim=512, lstm_layer=2, dropout=0.2,
                 cell='torch', attn='torch', packed=False):
        super().__init__()
        if cell not in ('torch', 'native', 'auto'):
            raise ValueError("cell must be 'torch', 'native' or 'auto', got %r" % (cell,))
        if attn not in _IMPLS:
            raise ValueError("attn must be 'torch', 'native' or 'auto', got %r" % (attn,))
        if not isinstance(packed, bool):
            raise TypeError('packed must be a bool, got %s' % type(packed).__name__)
        self.cell = cell
        self.attn = attn
        self.packed = packed
        self.dropout = nn.Dropout(p=dropout)
        self.lstm1 = nn.LSTM(feature_dim, hidden_dim, num_layers=1, bidirectional=True)
        self.atten1 = Attention(hidden_dim * 2, batch_first=True, impl=attn)
        self.lstm2 = nn.LSTM(hidden_dim * 2, hidden_dim, num_layers=1, bidirectional=True)
        self.atten2 = Attention(hidden_dim * 2, batch_first=True, impl=attn)
        width = hidden_dim * lstm_layer * 2
        self.fc1 = nn.Sequential(nn.Linear(width, width), nn.BatchNorm1d(width), nn.ReLU())
        self.fc2 = nn.Linear(width, num_classes)

    @staticmethod
    def _torch_layer(lstm, x, lengths):
        if lengths is None:
            return lstm(x)[0]
        T = x.shape[0]
        # pack_padded_sequence wants CPU lengths in [1, T]; a row of length 0 is not packable
        cpu = torch.as_tensor(lengths).detach().to('cpu', torch.int64).clamp(max=T)
        packed = nn.utils.rnn.pack_padded_sequence(x, cpu, enforce_sorted=False)
        return nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], total_length=T)[0]

    def _layer(self, lstm, x, lengths=None):
        if not self.packed:
            lengths = None
        if self.cell == 'torch':
            return self._torch_layer(lstm, x, lengths)
        from ..ops import lstm as native
        if lengths is not None:
            if self.cell == 'auto':
                if not (x.is_cuda and
                        (x.shape[1], lstm.hidden_size) in native.MEASURED_NATIVE_PACKED):
                    return self._torch_layer(lstm, x, lengths)
            elif not x.is_cuda:
                raise NotImplementedError("MyLSTM(packed=True, cell='native'): the native LSTM "
                                          "cell takes lengths only on a HIP device; use "
                                          "cell='torch' or 'auto'")
            return native.bilstm(x, lstm, lengths)
        if self.cell == 'auto' and not (
                x.is_cuda and (x.shape[1], lstm.hidden_size) in native.MEASURED_NATIVE):
            return lstm(x)[0]
        return native.bilstm(x, lstm)

    def forward(self, x, lengths=None):
        # x: [B, 1, F, T] spectrogram (or [B, F, T]) -> time-major [T, B, F]
        if x.dim() == 4:
            x = x.squeeze(1)
        x = x.permute(2, 0, 1)
        out1 = self._layer(self.lstm1, x, lengths)
        a, _ = self.atten1(out1.transpose(0, 1), lengths)
        out2 = self._layer(self.lstm2, out1, lengths)
        b, _ = self.atten2(out2.transpose(0, 1), lengths)
        z = torch.cat([a, b], dim=1)
        z = self.fc1(self.dropout(z))
        return self.fc2(self.dropout(z))
