"""Multi-head attention on the fused kernels of csrc/attention.hip.

attention(): one launch gives O and the fp32 log-sum-exp per query row
(attn_fwd); backward is attn_delta, attn_bwd_dkv and attn_bwd_dq. No
[Tq, Tk] tensor exists in either direction and no kernel uses atomics, so
outputs and gradients are bit-identical between calls.
OpsMultiheadAttention: nn.MultiheadAttention whose projections run the MFMA
GEMM (ops.linear) and whose attention reads the packed projection output in
place through strides."""
import math

import torch
import torch.nn as nn

ATTENTION_MAX_HEAD_DIM = 128
_MAX_BLOCKS = 2 ** 31 - 1


class _Attention(torch.autograd.Function):
    """Saves q, k, v, O, lse (fp32 [B, heads, Tq], base 2) and the mask."""

    @staticmethod
    def forward(ctx, q, k, v, mask, causal, scale):
        from . import require_native
        C = require_native()
        o, lse = C.attn_fwd(q, k, v, mask, causal, scale)
        ctx.save_for_backward(q, k, v, o, lse, mask)
        ctx.causal, ctx.scale = causal, scale
        return o.transpose(1, 2)

    @staticmethod
    def backward(ctx, dout):
        from . import require_native
        C = require_native()
        q, k, v, o, lse, mask = ctx.saved_tensors
        dout = dout.to(q.dtype)
        if dout.shape[-1] > 1 and dout.stride(-1) != 1:
            dout = dout.contiguous()
        delta = C.attn_delta(o, dout)
        dq = dk = dv = None
        if ctx.needs_input_grad[0]:
            dq = C.attn_bwd_dq(q, k, v, dout, mask, lse, delta, ctx.causal,
                               ctx.scale).transpose(1, 2)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dk, dv = (g.transpose(1, 2) for g in C.attn_bwd_dkv(
                q, k, v, dout, mask, lse, delta, ctx.causal, ctx.scale))
        return dq, dk, dv, None, None, None


def _attention_cpu(q, k, v, mask, causal, scale):
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float('-inf'))
    if causal:
        T = q.shape[2]
        above = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(above, float('-inf'))
    dead = (s == float('-inf')).all(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    return p @ v


def attention(q, k, v, key_padding_mask=None, causal=False, scale=None):
    """softmax(scale * q k^T + mask) v per (batch, head).

    q is [B, heads, Tq, Dh], k and v [B, heads, Tk, Dh], fp32 or bf16, with
    any batch, head and row strides (a non-unit last stride is made
    contiguous); 1 <= Dh <= 128. `key_padding_mask` is bool [B, Tk], True =
    the key is ignored; `causal` (Tq == Tk) lets row i see keys <= i; `scale`
    defaults to Dh ** -0.5. Returns [B, heads, Tq, Dh] in q's dtype, a view
    of a contiguous [B, Tq, heads, Dh] buffer; gradients go to q, k, v.

    A query row whose keys are all masked gives exactly 0 and contributes
    exactly 0 to every gradient, on both devices (torch gives NaN there).
    On the GPU the MFMA operands are bf16 (fp32 inputs are rounded while
    staging); scores, softmax statistics and accumulators are fp32. On the
    CPU this is the plain torch chain in the input dtype."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError('q, k, v must be [B, heads, T, Dh]')
    B, H, Tq, Dh = q.shape
    Tk = k.shape[2]
    if (k.shape != (B, H, Tk, Dh) or v.shape != k.shape
            or min(B, H, Tq, Tk, Dh) < 1):
        raise ValueError(f'mismatched shapes: q {tuple(q.shape)}, k '
                         f'{tuple(k.shape)}, v {tuple(v.shape)}')
    if Dh > ATTENTION_MAX_HEAD_DIM:
        raise ValueError(f'ops.attention serves head_dim <= '
                         f'{ATTENTION_MAX_HEAD_DIM}, got {Dh}')
    if causal and Tq != Tk:
        raise ValueError(f'causal attention needs Tq == Tk, got {Tq} and {Tk}')
    if key_padding_mask is not None and (
            key_padding_mask.dtype != torch.bool
            or key_padding_mask.shape != (B, Tk)):
        raise ValueError(f'key_padding_mask must be bool [{B}, {Tk}]')
    if B * H * ((max(Tq, Tk) + 15) // 16) > _MAX_BLOCKS:
        raise ValueError(f'ops.attention: B * heads * ceil(T / 16) exceeds '
                         f'the launch limit of {_MAX_BLOCKS} blocks')
    scale = float(Dh ** -0.5 if scale is None else scale)
    if not q.is_cuda:
        return _attention_cpu(q, k, v, key_padding_mask, causal, scale)
    from . import require_native
    require_native()
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'ops.attention: fp32 or bf16 only, got {q.dtype}')

    def unit(t):
        t = t.to(q.dtype)
        return t if Dh == 1 or t.stride(-1) == 1 else t.contiguous()
    mask = None
    if key_padding_mask is not None:
        mask = key_padding_mask.detach().contiguous()
    return _Attention.apply(unit(q), unit(k), unit(v), mask, bool(causal),
                            scale)


class OpsMultiheadAttention(nn.MultiheadAttention):
    """nn.MultiheadAttention (same constructor, parameter names and state
    dict) whose GPU forward and backward run ops.linear and ops.attention.

    Native on the GPU: batched [B, T, E] (batch_first) or [T, B, E] inputs
    with `key is value` (self-attention when also `query is key`: one
    in-projection GEMM over the packed weight; otherwise one for q and one
    for k / v), kdim == vdim == embed_dim, need_weights=False, attn_mask
    None, key_padding_mask None or bool [B, Tk], no bias_k / add_zero_attn,
    dropout == 0 or eval mode, head_dim <= 128. Returns (out, None). A query
    whose keys are all masked gives out-projection bias only (the library
    gives NaN). The library (nn.MultiheadAttention.forward) serves everything
    else on the GPU -- need_weights=True, an attn_mask, is_causal, attention
    dropout in training, unbatched inputs, separate k / v inputs or widths,
    float masks -- and everything on the CPU."""

    def _native(self, query, key, value, key_padding_mask, need_weights,
                attn_mask, is_causal):
        return (query.is_cuda and query.dim() == 3 and key is value
                and key.dim() == 3 and self._qkv_same_embed_dim
                and not need_weights and attn_mask is None and not is_causal
                and self.bias_k is None and not self.add_zero_attn
                and (self.dropout == 0 or not self.training)
                and self.head_dim <= ATTENTION_MAX_HEAD_DIM
                and (key_padding_mask is None
                     or key_padding_mask.dtype == torch.bool))

    def forward(self, query, key, value, key_padding_mask=None,
                need_weights=True, attn_mask=None, average_attn_weights=True,
                is_causal=False):
        if not self._native(query, key, value, key_padding_mask, need_weights,
                            attn_mask, is_causal):
            return super().forward(
                query, key, value, key_padding_mask=key_padding_mask,
                need_weights=need_weights, attn_mask=attn_mask,
                average_attn_weights=average_attn_weights,
                is_causal=is_causal)
        from . import linear, require_native
        require_native()
        E, H, Dh = self.embed_dim, self.num_heads, self.head_dim
        w, bias = self.in_proj_weight, self.in_proj_bias
        # [B, T, n, heads, Dh] axes of a projected [L, N, n * E] tensor
        perm = (0, 3, 1, 4, 2) if self.batch_first else (1, 3, 0, 4, 2)

        def project(x, lo, hi):
            """x [L, N, E] -> (hi - lo) / E tensors [B, heads, T, Dh], views
            of one GEMM output"""
            L, N = x.shape[:2]
            b = None if bias is None else bias[lo:hi]
            y = linear(x.reshape(L * N, E), w[lo:hi], b)
            y = y.view(L, N, (hi - lo) // E, H, Dh).permute(*perm)
            return y.unbind(-1)

        if query is key:
            q, k, v = project(query, 0, 3 * E)
        else:
            (q,), (k, v) = project(query, 0, E), project(key, E, 3 * E)
        o = attention(q, k, v, key_padding_mask)       # [B, heads, Tq, Dh]
        B, _, Tq, _ = o.shape
        o = o.transpose(1, 2).reshape(B * Tq, E)       # the buffer itself
        out = linear(o, self.out_proj.weight, self.out_proj.bias)
        out = out.view(B, Tq, E)
        return (out if self.batch_first else out.transpose(0, 1)), None
