"""fp64 restatement of the autoregressive read-out (csrc/ar_combine.h, functional.ar_combine) and of MultiARLSTM (TEST INFRASTRUCTURE, a
plain helper).

The read-out of transformer/MFT/models.py:376-399, K = ar_order:

    teacher-forced (:381-386)   p[b,t] = in_part[b,t] + sum_{i<K} w[b,t,i] target[b,t-i]     target[b,s<0] = 0; tap 0 = the current target
    free-running   (:388-397)   p[b,t] = in_part[b,t] + sum_{k<K} w[b,t,k] p[b,t-K+k]        p[b,s<0] = p_init; tap K-1 = the newest p
    out = p * mask              (:399)

in numpy, forward and the hand-written backward.  The reference detaches the fed-back predictions (:392), so with g = dout * mask
d in_part = g and d w[b,t,k] = g[b,t] * (the value tap k read) in both branches (tests/test_arlstm_cpu.py pins this to torch autograd on
the reference's formula and to the reference's fixtures).
"""
import numpy as np
import torch

from lstm_stack_ref import _fc, local_attention, torch_stack


def history(src, K, teacher, pad):
    """(B,T,K): the value tap k of step t reads — src = target (teacher: step t-k, zeros before 0) or p (step t-K+k, pad before 0)"""
    src = np.asarray(src, dtype=np.float64)
    B, T = src.shape
    hist = np.full((B, T, K), 0.0 if teacher else float(pad))
    for k in range(K):
        back = k if teacher else K - k
        if back < T:
            hist[:, back:, k] = src[:, :T - back]
    return hist


def forward(in_part, w, mask, target=None, p_init=0.0):
    """in_part (B,T), w (B,T,K), mask (B,T), target (B,T) or None -> p (B,T) unmasked, out (B,T)"""
    c, w, mask = (np.asarray(a, dtype=np.float64) for a in (in_part, w, mask))
    B, T, K = w.shape
    if target is not None:
        p = c + (w * history(target, K, True, 0.0)).sum(axis=2)
    else:
        full = np.full((B, T + K), float(p_init))                # column K + t holds p[:, t]
        for t in range(T):
            full[:, K + t] = c[:, t] + (w[:, t, :] * full[:, t:t + K]).sum(axis=1)
        p = full[:, K:]
    return p, p * mask


def backward(dout, mask, hist_src, K, teacher, p_init=0.0):
    """dout (B,T) on out; hist_src = the target (teacher) or the forward's p -> d in_part (B,T), d w (B,T,K)"""
    g = np.asarray(dout, dtype=np.float64) * np.asarray(mask, dtype=np.float64)
    return g, g[:, :, None] * history(hist_src, K, teacher, p_init)


class _ArFn(torch.autograd.Function):
    """the numpy read-out as a torch node, so that the fp64 torch restatement of the model below can differentiate through it"""

    @staticmethod
    def forward(ctx, in_part, w, mask, target, p_init):
        tgt = None if target is None else target.detach().numpy()
        p, out = forward(in_part.detach().numpy(), w.detach().numpy(), mask.numpy(), tgt, p_init)
        ctx.saved = (mask.numpy(), p if tgt is None else tgt, w.shape[2], tgt is not None, p_init)
        return torch.from_numpy(out.copy())

    @staticmethod
    def backward(ctx, dout):
        din, dw = backward(dout.numpy(), *ctx.saved)
        return torch.from_numpy(np.ascontiguousarray(din)), torch.from_numpy(np.ascontiguousarray(dw)), None, None, None


def torch_ar(in_part, w, mask, target=None, p_init=0.0):
    """(B,T), (B,T,K), (B,T), (B,T) or None -> out (B,T)"""
    return _ArFn.apply(in_part, w, mask, target, float(p_init))


def arlstm(p, x, mask, L=1, target=None, tgt_init=0.0, flip_taps=False):
    """MultiARLSTM (transformer/MFT/models.py:310-400) with an L-layer nn.LSTM, eval mode; p: name -> fp64 tensor, x (B,T,D), mask and
    target (B,T,1).  flip_taps is the WRONG reading with the tap order of the other branch, kept so that a test can show that the fixtures
    tell the two apart."""
    embed = torch.relu(_fc(p, "embed.1", x))
    z = _fc(p, "attn.2", torch.relu(_fc(p, "attn.0", embed)))
    B, T, _ = embed.shape
    H = p["lstm.weight_hh_l0"].shape[1]
    # the front of lstm_stack_ref.lstm_baseline: a plain stacked LSTM is the stacked recurrence with no feedback columns and zero states
    P = [torch.cat([torch.zeros(4 * H, H, dtype=x.dtype), p["lstm.weight_hh_l0"]], dim=1)]
    bias = []
    for l in range(1, L):
        P.append(torch.cat([p["lstm.weight_ih_l%d" % l], p["lstm.weight_hh_l%d" % l]], dim=1))
        bias.append(p["lstm.bias_ih_l%d" % l] + p["lstm.bias_hh_l%d" % l])
    gx0 = embed.permute(1, 0, 2) @ p["lstm.weight_ih_l0"].t() + p["lstm.bias_ih_l0"] + p["lstm.bias_hh_l0"]
    zeros = torch.zeros(L, B, H, dtype=x.dtype)
    bias_t = torch.stack(bias) if bias else torch.zeros(0, 4 * H, dtype=x.dtype)
    h_top = torch_stack(gx0, torch.stack(P), bias_t, zeros, zeros)
    m = mask.reshape(B, T).to(x.dtype)
    ctx = local_attention(z, h_top, m)                                                   # (B,T,H)
    in_part = _fc(p, "decoder.2", torch.relu(_fc(p, "decoder.0", ctx))).reshape(B, T)
    w = _fc(p, "autoreg", ctx)
    if flip_taps:
        w = w.flip(2)
    tgt = None if target is None else target.reshape(B, T).to(x.dtype)
    return torch_ar(in_part, w, m, tgt, tgt_init).unsqueeze(-1)
