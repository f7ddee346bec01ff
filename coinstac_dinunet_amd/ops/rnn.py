"""LSTM on the persistent recurrence kernels of csrc/lstm.hip.

Per layer: one MFMA GEMM gives the gate pre-activations of every step and
both directions (linear_fwd), one launch runs the whole recurrence
(lstm_rec_fwd), and in backward one launch runs the reverse-time loop
(lstm_rec_bwd) before the time-parallel weight, bias and input gradients
(linear_wgrad, colsum, linear_dgrad)."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import PackedSequence

LSTM_MAX_HIDDEN = 256


def _gate_inner(w, H):
    """Rows (gate, unit) of a [4H, ...] tensor -> rows (unit, gate): the
    kernels read the four gates of a unit as one 16-byte vector."""
    return w.reshape(4, H, -1).transpose(0, 1).reshape(4 * H, -1)


def _gate_outer(g, H):
    """Inverse of _gate_inner: rows (unit, gate) -> torch's (gate, unit)."""
    return g.reshape(H, 4, -1).transpose(0, 1).reshape(4 * H, -1)


class _LSTMLayer(torch.autograd.Function):
    """One layer, one or two directions. x [T, B, I]; h0 / c0 [D, B, H] fp32
    or None; weights = (w_ih, w_hh[, b_ih, b_hh]) per direction. Returns fp32
    y [T, B, D*H], h_T and c_T [D, B, H]."""

    @staticmethod
    def forward(ctx, x, h0, c0, has_bias, *weights):
        from . import require_native
        C = require_native()
        per = 4 if has_bias else 2
        D = len(weights) // per
        T, B, I = x.shape
        H = weights[1].shape[1]
        xf = x.reshape(T * B, I).float()
        w_ih = torch.cat([_gate_inner(weights[d * per].float(), H)
                          for d in range(D)])
        if has_bias:
            bias = torch.cat([_gate_inner(weights[d * per + 2].float()
                                          + weights[d * per + 3].float(), H)
                              for d in range(D)]).reshape(-1)
        else:
            bias = torch.empty(0, device=x.device)
        xp = C.linear_fwd(xf, w_ih, bias, False).view(T, B, D * 4 * H)
        wpack = torch.stack([C.lstm_pack_weights(weights[d * per + 1].detach())
                             for d in range(D)])
        need_grad = any(ctx.needs_input_grad)
        y, hT, cT, gates, cells = C.lstm_rec_fwd(xp, wpack, h0, c0, H,
                                                 need_grad)
        if need_grad:
            ctx.save_for_backward(xf, w_ih, wpack, gates, cells, y, h0, c0)
            ctx.has_bias = has_bias
            ctx.dtypes = (x.dtype,) + tuple(w.dtype for w in weights)
        return y, hT, cT

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        from . import require_native
        C = require_native()
        xf, w_ih, wpack, gates, cells, y, h0, c0 = ctx.saved_tensors
        T, B, D, H, _ = gates.shape
        I = xf.shape[1]

        def grad(g, like):
            return (torch.zeros_like(like) if g is None
                    else g.float().contiguous())
        hT_like = cells.new_empty(D, B, H)
        dG, dh0, dc0 = C.lstm_rec_bwd(
            grad(dy, y), grad(dhT, hT_like), grad(dcT, hT_like), gates, cells,
            c0, wpack)
        dG = dG.view(T * B, D * 4 * H)
        x_dtype, w_dtypes = ctx.dtypes[0], ctx.dtypes[1:]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = C.linear_dgrad(dG, w_ih).view(T, B, I).to(x_dtype)
        dw_ih = C.linear_wgrad(dG, xf)
        db = C.colsum(dG) if ctx.has_bias else None
        grads = []
        for d in range(D):
            yd = y[:, :, d * H:(d + 1) * H]
            first = (h0[d] if h0 is not None else y.new_zeros(B, H))[None]
            # h before step t of the direction's walk
            hprev = (torch.cat([first, yd[:-1]]) if d == 0
                     else torch.cat([yd[1:], first]))
            sl = slice(d * 4 * H, (d + 1) * 4 * H)
            dw_hh = C.linear_wgrad(dG[:, sl].contiguous(),
                                   hprev.reshape(T * B, H))
            grads += [_gate_outer(dw_ih[sl], H), _gate_outer(dw_hh, H)]
            if ctx.has_bias:
                grads += [_gate_outer(db[sl], H).reshape(-1)] * 2
        grads = [g.to(dt) for g, dt in zip(grads, w_dtypes)]
        return (dx, dh0 if h0 is not None else None,
                dc0 if c0 is not None else None, None, *grads)


def lstm(x, weights, hx=None, num_layers=1, bidirectional=False,
         batch_first=False, dropout=0.0, training=False):
    """Multi-layer (bi)LSTM with the semantics of nn.LSTM (proj_size = 0).

    x is [T, B, I] ([B, T, I] with `batch_first`), fp32 or bf16; `weights`
    is the flat list nn.LSTM keeps: w_ih, w_hh (and b_ih, b_hh) per layer
    and direction; hx = (h0, c0), each [layers * D, B, H], or None.
    1 <= H <= 256. Returns (y, (h_n, c_n)) in x's dtype. The state
    between steps is fp32 (c) and bf16 (h as the MFMA operand), the gate
    pre-activations are fp32. Layers are looped here, with F.dropout between
    them. Two calls give bit-identical y. GPU only."""
    D = 2 if bidirectional else 1
    has_bias = len(weights) == num_layers * D * 4
    per = 4 if has_bias else 2
    if len(weights) != num_layers * D * per:
        raise ValueError(f'expected {num_layers * D * 2} or '
                         f'{num_layers * D * 4} weights, got {len(weights)}')
    H = weights[1].shape[1]
    if not 1 <= H <= LSTM_MAX_HIDDEN:
        raise ValueError(f'ops.lstm serves 1 <= hidden_size <= '
                         f'{LSTM_MAX_HIDDEN}, got {H}')
    if x.dim() != 3:
        raise ValueError(f'x must be [T, B, I], got {tuple(x.shape)}')
    out = x.transpose(0, 1) if batch_first else x
    h0 = c0 = None
    if hx is not None:
        h0, c0 = (s.float().reshape(num_layers, D, s.shape[-2], H)
                  for s in hx)
    hs, cs = [], []
    for layer in range(num_layers):
        w = weights[layer * D * per:(layer + 1) * D * per]
        out, hT, cT = _LSTMLayer.apply(
            out, None if h0 is None else h0[layer].contiguous(),
            None if c0 is None else c0[layer].contiguous(), has_bias, *w)
        hs.append(hT)
        cs.append(cT)
        if dropout and training and layer + 1 < num_layers:
            out = F.dropout(out, dropout, True)
    out = out.to(x.dtype)
    if batch_first:
        out = out.transpose(0, 1)
    return out, (torch.cat(hs).to(x.dtype), torch.cat(cs).to(x.dtype))


class OpsLSTM(nn.LSTM):
    """nn.LSTM (same constructor, parameter names and state dict) whose GPU
    forward and backward run the persistent recurrence kernels (lstm.hip).

    Native on the GPU: a dense [T, B, I], batch_first [B, T, I] or unbatched
    [T, I] input, fp32 or bf16, 1 <= hidden_size <= 256, any number of
    layers, one or two directions, hx given or not. The library
    (nn.LSTM.forward) serves, on the GPU: a PackedSequence input,
    proj_size > 0, and hidden_size > 256. On the CPU everything is
    nn.LSTM.forward."""

    def forward(self, input, hx=None):
        if (isinstance(input, PackedSequence) or not input.is_cuda
                or self.proj_size > 0 or self.hidden_size > LSTM_MAX_HIDDEN):
            return super().forward(input, hx)
        from . import require_native
        require_native()
        batched = input.dim() == 3
        if not batched:
            input = input.unsqueeze(0 if self.batch_first else 1)
            if hx is not None:
                hx = tuple(s.unsqueeze(1) for s in hx)
        weights = [getattr(self, n) for n in self._flat_weights_names]
        y, (h, c) = lstm(input, weights, hx, self.num_layers,
                         self.bidirectional, self.batch_first, self.dropout,
                         self.training)
        if not batched:
            y = y.squeeze(0 if self.batch_first else 1)
            h, c = h.squeeze(1), c.squeeze(1)
        return y, (h, c)
