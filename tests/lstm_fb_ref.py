"""fp64 restatement of the LSTM scan with the read-out MLP in its recurrence (csrc/scan_fb.h) and of MultiEDLSTM (TEST INFRASTRUCTURE, a
plain helper).

The decoder loop of transformer/MFT/models.py:290-305 with nn.LSTM(1 + H, H), gate order i, f, g, o:

    p_{-1} = p_init,  h_{-1} = h0,  c_{-1} = c0
    gates_t = gxc_t + p_{t-1} w_p + h_{t-1} W_hh^T              gxc = ctx W_ih[:, 1:]^T + b_ih + b_hh,  w_p = W_ih[:, 0]
    (h_t, c_t) = cell(gates_t, c_{t-1})
    u_t = ReLU(W1 h_t + b1),  p_t = w2 . u_t + b2

in numpy, forward and the hand-derived backward, so that nothing of torch's LSTM is in it (tests/test_lstm_fb_cpu.py pins it to torch
autograd and to the reference's fixtures).
"""
import numpy as np
import torch

from lstm_stack_ref import _fc, _sig, local_attention, torch_stack  # noqa: F401


def forward(gxc, w_p, W_hh, W1, b1, w2, b2, h0=None, c0=None, p_init=0.0):
    """gxc (T,B,4H), w_p (4H), W_hh (4H,H), W1 (E,H), b1 (E), w2 (E), b2 scalar, h0 / c0 (B,H) or None
    -> p_all (T,B), h_all, c_all (T,B,H), acts (T,B,4H), u_all (T,B,E)"""
    gxc, w_p, W_hh, W1, b1, w2 = (np.asarray(a, dtype=np.float64) for a in (gxc, w_p, W_hh, W1, b1, w2))
    w_p, w2, b2 = w_p.reshape(-1), w2.reshape(-1), float(np.asarray(b2, dtype=np.float64).reshape(-1)[0])
    T, B, H4 = gxc.shape
    H, E = H4 // 4, W1.shape[0]
    h = np.zeros((B, H)) if h0 is None else np.array(h0, dtype=np.float64)
    c = np.zeros((B, H)) if c0 is None else np.array(c0, dtype=np.float64)
    p = np.full((B,), float(p_init))
    p_all, h_all, c_all = np.zeros((T, B)), np.zeros((T, B, H)), np.zeros((T, B, H))
    acts, u_all = np.zeros((T, B, 4 * H)), np.zeros((T, B, E))
    for t in range(T):
        g = gxc[t] + p[:, None] * w_p[None, :] + h @ W_hh.T
        i, f, gg, og = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
        c = f * c + i * gg
        h = og * np.tanh(c)
        u = np.maximum(h @ W1.T + b1, 0.0)
        p = u @ w2 + b2
        p_all[t], h_all[t], c_all[t], acts[t], u_all[t] = p, h, c, np.concatenate([i, f, gg, og], axis=1), u
    return p_all, h_all, c_all, acts, u_all


def backward(dp_ext, w_p, W_hh, W1, w2, h0, c0, p_init, p_all, h_all, c_all, acts, u_all):
    """dp_ext (T,B) on p_all -> dict(dgxc, dw_p, dW_hh, dW1, db1, dw2, db2, dh0, dc0, du, dp)"""
    w_p, W_hh, W1, w2 = (np.asarray(a, dtype=np.float64) for a in (w_p, W_hh, W1, w2))
    w_p, w2 = w_p.reshape(-1), w2.reshape(-1)
    T, B, H = h_all.shape
    h0 = np.zeros((B, H)) if h0 is None else np.asarray(h0, dtype=np.float64)
    c0 = np.zeros((B, H)) if c0 is None else np.asarray(c0, dtype=np.float64)
    dG, du, dp = np.zeros((T, B, 4 * H)), np.zeros_like(u_all), np.zeros((T, B))
    dg_next, dc = np.zeros((B, 4 * H)), np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        dp[t] = np.asarray(dp_ext[t], dtype=np.float64) + dg_next @ w_p
        du[t] = dp[t][:, None] * w2[None, :] * (u_all[t] > 0)
        dh = du[t] @ W1 + dg_next @ W_hh
        a = acts[t]
        i, f, gg, og = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
        cp = c_all[t - 1] if t > 0 else c0
        th = np.tanh(c_all[t])
        dct = dc + dh * og * (1 - th * th)
        dg_next = np.concatenate([dct * gg * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - gg * gg), dh * th * og * (1 - og)], axis=1)
        dc = dct * f
        dG[t] = dg_next
    hprev = np.concatenate([h0[None], h_all[:-1]], axis=0).reshape(T * B, H)
    pprev = np.concatenate([np.full((1, B), float(p_init)), p_all[:-1]], axis=0).reshape(T * B)
    G2 = dG.reshape(T * B, 4 * H)
    return dict(dgxc=dG, dw_p=G2.T @ pprev, dW_hh=G2.T @ hprev, dW1=du.reshape(T * B, -1).T @ h_all.reshape(T * B, H), db1=du.sum(axis=(0, 1)),
                dw2=dp.reshape(-1) @ u_all.reshape(T * B, -1), db2=np.array([dp.sum()]), dh0=dg_next @ W_hh, dc0=dc, du=du, dp=dp)


class _FbFn(torch.autograd.Function):
    """the numpy recurrence as a torch node, so that the fp64 torch restatement of the model below can differentiate through it"""

    @staticmethod
    def forward(ctx, gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0, p_init):
        n = [t.detach().numpy() for t in (gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0)]
        outs = forward(*n, p_init=p_init)
        ctx.n, ctx.saved, ctx.p_init = n, outs, p_init
        return torch.from_numpy(outs[0].copy())

    @staticmethod
    def backward(ctx, dp_all):
        _, w_p, W_hh, W1, _, w2, _, h0, c0 = ctx.n
        g = backward(dp_all.numpy(), w_p, W_hh, W1, w2, h0, c0, ctx.p_init, *ctx.saved)
        shapes = [a.shape for a in ctx.n]
        keys = ("dgxc", "dw_p", "dW_hh", "dW1", "db1", "dw2", "db2", "dh0", "dc0")
        return tuple(torch.from_numpy(np.ascontiguousarray(g[k]).reshape(s)) for k, s in zip(keys, shapes)) + (None,)


def torch_fb(gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0, p_init):
    return _FbFn.apply(gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0, float(p_init))


def edlstm(p, x, mask, tgt_init=0.0):
    """MultiEDLSTM (transformer/MFT/models.py:222-308) with one-layer LSTMs, eval mode; p: name -> fp64 tensor, x (B,T,D), mask (B,T,1)."""
    embed = torch.relu(_fc(p, "embed.1", x))
    z = _fc(p, "attn.2", torch.relu(_fc(p, "attn.0", embed)))
    B, T, _ = embed.shape
    H = p["encoder.weight_hh_l0"].shape[1]
    # the encoder: a plain LSTM from enc_h0 / enc_c0; pack_padded_sequence is not needed (causal; local_attention zeroes padded steps)
    gx = embed.permute(1, 0, 2) @ p["encoder.weight_ih_l0"].t() + p["encoder.bias_ih_l0"] + p["encoder.bias_hh_l0"]
    h_enc = _plain_lstm(gx, p["encoder.weight_hh_l0"], p["enc_h0"][0].expand(B, H), p["enc_c0"][0].expand(B, H))
    ctx = local_attention(z, h_enc, mask.reshape(B, T).to(x.dtype))                      # (B,T,H)
    Wi = p["decoder.weight_ih_l0"]
    gxc = ctx.permute(1, 0, 2) @ Wi[:, 1:].t() + p["decoder.bias_ih_l0"] + p["decoder.bias_hh_l0"]
    pt = torch_fb(gxc, Wi[:, 0], p["decoder.weight_hh_l0"], p["out.0.weight"], p["out.0.bias"], p["out.2.weight"][0], p["out.2.bias"],
                  p["dec_h0"][0].expand(B, H), p["dec_c0"][0].expand(B, H), tgt_init)
    return pt.t().unsqueeze(-1) * mask.to(x.dtype)


def _plain_lstm(gx, W_hh, h0, c0):
    """h_all (T,B,H) of an LSTM scan in torch ops (differentiable by autograd)"""
    T, B, H4 = gx.shape
    H = H4 // 4
    h, c, out = h0, c0, []
    for t in range(T):
        g = gx[t] + h @ W_hh.t()
        i, f, gg, og = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = og * torch.tanh(c)
        out.append(h)
    return torch.stack(out)
