"""(bi)LSTM classifier of fMRI ICA time courses.

The input is [B, S, num_comps, window_size]: S windows of the ICA component
time courses of a subject. Each window goes through a linear encoder + ReLU,
the sequence of S encodings through a (bi)LSTM, attention pooling over the S
steps (a learned score, softmax over time, weighted sum) and a linear head.
On GPU the encoder and the head run the MFMA GEMM (ops.linear) and the LSTM
the persistent recurrence kernels (ops.OpsLSTM); the pooling is a few tiny
torch ops.
"""
import torch
import torch.nn as nn

from .mlp import _OpsLinear


class ICALstm(nn.Module):
    def __init__(self, num_comps=53, window_size=20, input_size=256,
                 hidden_size=128, num_layers=1, bidirectional=True,
                 num_class=2):
        super().__init__()
        from ..ops import OpsLSTM
        self.encoder = _OpsLinear(num_comps * window_size, input_size)
        self.lstm = OpsLSTM(input_size, hidden_size, num_layers=num_layers,
                            bidirectional=bidirectional, batch_first=True)
        width = hidden_size * (2 if bidirectional else 1)
        self.score = nn.Linear(width, 1)
        self.head = _OpsLinear(width, num_class)

    def forward(self, x):
        from .. import ops
        B, S = x.shape[:2]
        enc = ops.linear(x.reshape(B * S, -1), self.encoder.weight,
                         self.encoder.bias, relu=True)
        y, _ = self.lstm(enc.view(B, S, -1))
        attn = torch.softmax(self.score(y), dim=1)   # [B, S, 1]
        return self.head((attn * y).sum(1))
