"""Transformer-encoder classifier of fMRI ICA time courses, the sibling of
ICALstm.

The input is [B, S, num_comps, window_size]: S windows of the ICA component
time courses of a subject, plus optional `lengths` [B], the number of valid
windows per subject. Each window goes through a linear encoder + ReLU and
gets a learned positional embedding; `num_layers` pre-norm blocks follow
(LayerNorm, self-attention, residual; LayerNorm, two-layer MLP, residual),
then a final LayerNorm, the mean over the valid windows and a linear head.
Windows beyond `lengths` are masked as keys and left out of the mean, so
their content does not reach the logits.

On GPU the encoder, the MLPs, the attention projections and the head run
the MFMA GEMM (ops.linear) and the attention the fused kernels
(ops.OpsMultiheadAttention). LayerNorm, the residual adds, the embedding add
and the masked mean stay on the library.
"""
import torch
import torch.nn as nn

from .mlp import _OpsLinear


class _Block(nn.Module):
    def __init__(self, embed_dim, num_heads, mlp_ratio):
        super().__init__()
        from ..ops import OpsMultiheadAttention
        self.norm1 = nn.LayerNorm(embed_dim)
        self.attn = OpsMultiheadAttention(embed_dim, num_heads,
                                          batch_first=True)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.fc1 = _OpsLinear(embed_dim, embed_dim * mlp_ratio)
        self.fc2 = _OpsLinear(embed_dim * mlp_ratio, embed_dim)

    def forward(self, x, pad):
        from .. import ops
        B, S, E = x.shape
        y = self.norm1(x)
        x = x + self.attn(y, y, y, key_padding_mask=pad,
                          need_weights=False)[0]
        y = self.norm2(x).reshape(B * S, E)
        y = ops.linear(y, self.fc1.weight, self.fc1.bias, relu=True)
        return x + self.fc2(y).view(B, S, E)


class ICATransformer(nn.Module):
    def __init__(self, num_comps=53, window_size=20, embed_dim=256,
                 num_heads=4, num_layers=2, mlp_ratio=2, num_class=2,
                 max_windows=512):
        super().__init__()
        self.encoder = _OpsLinear(num_comps * window_size, embed_dim)
        self.pos = nn.Parameter(torch.zeros(max_windows, embed_dim))
        nn.init.normal_(self.pos, std=0.02)
        self.blocks = nn.ModuleList(
            _Block(embed_dim, num_heads, mlp_ratio)
            for _ in range(num_layers))
        self.norm = nn.LayerNorm(embed_dim)
        self.head = _OpsLinear(embed_dim, num_class)

    def forward(self, x, lengths=None):
        from .. import ops
        B, S = x.shape[:2]
        if S > self.pos.shape[0]:
            raise ValueError(f'{S} windows, but max_windows = '
                             f'{self.pos.shape[0]}')
        pad = None
        if lengths is not None:
            lengths = torch.as_tensor(lengths, device=x.device)
            if lengths.shape != (B,):   # entries >= 1; not checked (no sync)
                raise ValueError(f'lengths must be [{B}]')
            pad = torch.arange(S, device=x.device)[None] >= lengths[:, None]
        enc = ops.linear(x.reshape(B * S, -1), self.encoder.weight,
                         self.encoder.bias, relu=True)
        h = enc.view(B, S, -1) + self.pos[:S]
        for block in self.blocks:
            h = block(h, pad)
        h = self.norm(h)
        if pad is None:
            pooled = h.mean(1)
        else:
            keep = (~pad).to(h.dtype)[:, :, None]
            pooled = (h * keep).sum(1) / keep.sum(1)
        return self.head(pooled)
