"""The reference of the LSTM baselines with the softmax over the taps (TEST INFRASTRUCTURE, a plain helper module beside
tests/decoder_stream_ref.py): models._LocalAttnLSTM with ``attend_over_taps`` on, as a batch over all T and one window per call, in fp64
with the ``rounding`` switch of tests/bf16_ref.py.

``batch`` is the composition ``_LocalAttnLSTM._front`` / ``.forward`` run in eval mode, from bf16_ref.linear / linear_pair / lstm_scan and
``local_attention_taps``.  ``LstmStep`` carries, per layer, (h, c) and the ring of the last L masked outputs of the top layer, written
exactly as csrc/lstm_step.h writes it: step p writes slot p % L with m_p * h_top and reads the slots (p - i) % L for
1 <= i <= min(p, L - 1).  Every affine map and every cell of a step is the same bf16_ref call at T = 1 that ``batch`` makes over all T,
so one function serves the step and the batch path (tests/test_lstm_stream_cpu.py holds the two together).

Parameters: a dict of fp64 tensors under MultiLSTM's own names: "embed.1.weight", "embed.1.bias", "attn.0.*", "attn.2.*",
"lstm.weight_ih_l0", ..., "decoder.0.*", "decoder.2.*".
"""
import torch

import bf16_ref as R


def local_attention_taps(z, h, valid):
    """functional.local_attention(z, h, valid, over="taps") in the tensors' dtype: z (B,T,L), h (T,B,H), valid (B,T) -> ctx (B,T,H).
    a = exp(z - max) / sum over the L taps of each row; ctx[b,t] = sum_{i<L, t-i>=0} a[b,t,i] valid[b,t-i] h[t-i,b], taps in index order."""
    B, T, L = z.shape
    e = torch.exp(z - z.max(dim=2, keepdim=True).values)
    s = e[:, :, 0]
    for i in range(1, L):
        s = s + e[:, :, i]
    a = e / s.unsqueeze(-1)
    hv = h.transpose(0, 1) * valid.reshape(B, T, 1)                                                   # (B,T,H), zero at masked steps
    ctx = a[:, :, 0:1] * hv
    for i in range(1, min(L, T)):                                                                     # differentiable: no in-place writes
        ctx = ctx + torch.cat([hv.new_zeros(B, i, hv.shape[2]), a[:, i:, i:i + 1] * hv[:, :T - i]], dim=1)
    return ctx


def n_layers_of(p):
    return sum(1 for k in p if k.startswith("lstm.weight_ih_l"))


def _lstm(p, l):
    return [p["lstm.%s_l%d" % (n, l)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _readout(p, ctx, rounding):
    hid = R.linear(ctx, p["decoder.0.weight"], p["decoder.0.bias"], act=1, rounding=rounding)
    return R.linear(hid, p["decoder.2.weight"], p["decoder.2.bias"], rounding=rounding)


def batch(p, x, mask, rounding=True):
    """x (B,T,in), mask (B,T) -> (B,T,1): the taps-mode model over all T"""
    B, T, _ = x.shape
    embed = R.linear(x, p["embed.1.weight"], p["embed.1.bias"], act=1, rounding=rounding)
    Wi, Wh, bi, bh = _lstm(p, 0)
    hid, gx = R.linear_pair(embed.transpose(0, 1), p["attn.0.weight"], p["attn.0.bias"], Wi, bi + bh, act1=1, rounding=rounding)
    z = R.linear(hid, p["attn.2.weight"], p["attn.2.bias"], rounding=rounding).transpose(0, 1)      # (B,T,L)
    h_all, _ = R.lstm_scan(gx, Wh, rounding=rounding)
    for l in range(1, n_layers_of(p)):
        Wi, Wh, bi, bh = _lstm(p, l)
        h_all, _ = R.lstm_scan(R.linear(h_all, Wi, bi + bh, rounding=rounding), Wh, rounding=rounding)
    ctx = local_attention_taps(z, h_all, mask)
    return _readout(p, ctx, rounding) * mask.reshape(B, T, 1)


class LstmStep:
    """step(x_t (B, in), mask_t (B) or None) -> y_t (B, 1), window by window from position 0"""

    def __init__(self, p, batch, rounding=True):
        self.p, self.B, self.rounding = p, int(batch), rounding
        self.NL, self.L = n_layers_of(p), p["attn.2.weight"].shape[0]
        self.t = 0
        self.h = self.c = None
        self.ring = [None] * self.L                            # any contents: a slot is written before it is read

    def step(self, x, mask_t=None):
        p, B, rd, L, t = self.p, self.B, self.rounding, self.L, self.t
        m = x.new_ones(B) if mask_t is None else mask_t.reshape(B).to(x.dtype)
        embed = R.linear(x, p["embed.1.weight"], p["embed.1.bias"], act=1, rounding=rd)
        Wi, Wh, bi, bh = _lstm(p, 0)
        hid, gx = R.linear_pair(embed.reshape(1, B, -1), p["attn.0.weight"], p["attn.0.bias"], Wi, bi + bh, act1=1, rounding=rd)
        z = R.linear(hid[0], p["attn.2.weight"], p["attn.2.bias"], rounding=rd)                     # (B,L)
        h, c = [], []
        for l in range(self.NL):
            if l:
                Wi, Wh, bi, bh = _lstm(p, l)
                gx = R.linear(h[l - 1].reshape(1, B, -1), Wi, bi + bh, rounding=rd)
            first = t == 0                                                                           # zero states, nothing carried is read
            h_all, c_all = R.lstm_scan(gx, Wh, None if first else self.h[l], None if first else self.c[l], rounding=rd)
            h.append(h_all[0])
            c.append(c_all[0])
        self.h, self.c = h, c
        e = torch.exp(z - z.max(dim=1, keepdim=True).values)
        s = e[:, 0]
        for i in range(1, L):
            s = s + e[:, i]
        a = e / s.unsqueeze(-1)
        mine = h[-1] * m.unsqueeze(-1)
        ctx = a[:, 0:1] * mine
        for i in range(1, min(t, L - 1) + 1):
            ctx = ctx + a[:, i:i + 1] * self.ring[(t - i) % L]
        self.ring[t % L] = mine
        self.t += 1
        return _readout(p, ctx, rd) * m.unsqueeze(-1)


def stepped(p, x, mask=None, rounding=True):
    """x (B,T,in), mask (B,T) or None -> (B,T,1): every window through LstmStep, in order"""
    B, T, _ = x.shape
    s = LstmStep(p, B, rounding)
    return torch.stack([s.step(x[:, t], None if mask is None else mask[:, t]) for t in range(T)], dim=1)


def params(in_dim, E, H, n_layers, L, seed=11, tag="lstm_stream"):
    """fp64 parameters of an LSTM baseline under MultiLSTM's names"""
    import recipe as G
    p = {}

    def draw(name, shape, k):
        p[name] = (G.gen_normal("%s:%s" % (tag, name), shape, seed) * k).double()

    draw("embed.1.weight", (E, in_dim), 1.0 / in_dim ** 0.5)
    draw("embed.1.bias", (E,), 0.1)
    draw("attn.0.weight", (E, E), 1.0 / E ** 0.5)
    draw("attn.0.bias", (E,), 0.1)
    draw("attn.2.weight", (L, E), 2.0 / E ** 0.5)
    draw("attn.2.bias", (L,), 0.3)
    for l in range(n_layers):
        k = E if l == 0 else H
        draw("lstm.weight_ih_l%d" % l, (4 * H, k), 1.0 / k ** 0.5)
        draw("lstm.weight_hh_l%d" % l, (4 * H, H), 1.0 / H ** 0.5)
        draw("lstm.bias_ih_l%d" % l, (4 * H,), 0.1)
        draw("lstm.bias_hh_l%d" % l, (4 * H,), 0.1)
    draw("decoder.0.weight", (E, H), 1.0 / H ** 0.5)
    draw("decoder.0.bias", (E,), 0.1)
    draw("decoder.2.weight", (1, E), 1.0 / E ** 0.5)
    draw("decoder.2.bias", (1,), 0.1)
    return p
