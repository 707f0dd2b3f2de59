"""The reference of the two LSTM baselines whose read-out feeds its own prediction back, free-running, with the softmax over the taps
(TEST INFRASTRUCTURE, a plain helper module beside tests/lstm_stream_ref.py): models.MultiEDLSTM and models.MultiARLSTM with
``attend_over_taps`` on, as a batch over all T and one window per call, in fp64 with the ``rounding`` switch of tests/bf16_ref.py.
Composed from existing pieces only.

The front (embed, attention MLP, LSTM cells, local attention over the taps) is lstm_stream_ref.LstmStep's, with optional initial rows
for a one-layer LSTM: at position 0 the rows go to bf16_ref.lstm_scan as h0 / c0, so the recurrent product runs and the cell keeps its
forget term, as csrc/lstm_step.h's fb tail does.

The ``fb`` tail (MultiEDLSTM): bf16_ref.linear for gxc, then bf16_ref.lstm_fb_scan at T = 1 from the carried (hd, cd); the carried
UNMASKED q goes in through its ``mutate={"p": ...}`` hook.  The ``ar`` tail (MultiARLSTM): bf16_ref.linear_pair + linear for in_part and
w, then the chain acc = in_part; acc += w[k] * hist_k for k = 0 .. K - 1 with hist_k = p_{t-K+k}, or tgt_init before step 0
(ar_combine.h's free-running order); the UNMASKED acc is fed back.

Parameters: a dict of fp64 tensors under the models' own names ("encoder.weight_ih_l0", "enc_h0" (1,1,H), "decoder.weight_ih_l0"
(4H, 1 + H), "out.0.weight", ... for MultiEDLSTM; lstm_stream_ref's names plus "autoreg.weight" (K, H), "autoreg.bias" for MultiARLSTM).
"""
import torch

import bf16_ref as R
import lstm_stream_ref as LS
import recipe as G

TGT_INIT = 0.25


# ------------------------------------------------------------------------------------------------ the front
def _layers(p, prefix):
    n = sum(1 for k in p if k.startswith(prefix + ".weight_ih_l"))
    return [[p["%s.%s_l%d" % (prefix, name, l)] for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for l in range(n)]


def _softmax_taps(z):
    L = z.shape[-1]
    e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
    s = e[..., 0]
    for i in range(1, L):
        s = s + e[..., i]
    return e / s.unsqueeze(-1)


def front_batch(p, prefix, x, mask, rounding, rows=None):
    """x (B,T,in), mask (B,T) -> ctx (B,T,H); rows: (h0, c0), each (B,H), of a one-layer LSTM, or None"""
    layers = _layers(p, prefix)
    embed = R.linear(x, p["embed.1.weight"], p["embed.1.bias"], act=1, rounding=rounding)
    Wi, Wh, bi, bh = layers[0]
    hid, gx = R.linear_pair(embed.transpose(0, 1), p["attn.0.weight"], p["attn.0.bias"], Wi, bi + bh, act1=1, rounding=rounding)
    z = R.linear(hid, p["attn.2.weight"], p["attn.2.bias"], rounding=rounding).transpose(0, 1)
    h0, c0 = rows if rows is not None else (None, None)
    h_all, _ = R.lstm_scan(gx, Wh, h0, c0, rounding=rounding)
    for Wi, Wh, bi, bh in layers[1:]:
        h_all, _ = R.lstm_scan(R.linear(h_all, Wi, bi + bh, rounding=rounding), Wh, rounding=rounding)
    return LS.local_attention_taps(z, h_all, mask)


class _Front:
    """one window of the front: step(x_t (B,in), m (B)) -> ctx (B,H); lstm_stream_ref.LstmStep's stages up to the context"""

    def __init__(self, p, prefix, batch, rounding, rows=None):
        self.p, self.layers, self.B, self.rounding, self.rows = p, _layers(p, prefix), int(batch), rounding, rows
        self.L = p["attn.2.weight"].shape[0]
        self.t, self.h, self.c = 0, None, None
        self.ring = [None] * self.L

    def step(self, x, m):
        p, B, rd, L, t = self.p, self.B, self.rounding, self.L, self.t
        embed = R.linear(x, p["embed.1.weight"], p["embed.1.bias"], act=1, rounding=rd)
        Wi, Wh, bi, bh = self.layers[0]
        hid, gx = R.linear_pair(embed.reshape(1, B, -1), p["attn.0.weight"], p["attn.0.bias"], Wi, bi + bh, act1=1, rounding=rd)
        z = R.linear(hid[0], p["attn.2.weight"], p["attn.2.bias"], rounding=rd)
        h, c = [], []
        for l, (Wi, Wh, bi, bh) in enumerate(self.layers):
            if l:
                gx = R.linear(h[l - 1].reshape(1, B, -1), Wi, bi + bh, rounding=rd)
            if t == 0:
                h0, c0 = self.rows if (self.rows is not None and l == 0) else (None, None)
            else:
                h0, c0 = self.h[l], self.c[l]
            h_all, c_all = R.lstm_scan(gx, Wh, h0, c0, rounding=rd)
            h.append(h_all[0])
            c.append(c_all[0])
        self.h, self.c = h, c
        a = _softmax_taps(z)
        mine = h[-1] * m.unsqueeze(-1)
        ctx = a[:, 0:1] * mine
        for i in range(1, min(t, L - 1) + 1):
            ctx = ctx + a[:, i:i + 1] * self.ring[(t - i) % L]
        self.ring[t % L] = mine
        self.t += 1
        return ctx


def _mask_of(x, mask_t, B):
    return x.new_ones(B) if mask_t is None else mask_t.reshape(B).to(x.dtype)


# ------------------------------------------------------------------------------------------------ MultiEDLSTM
def _ed_rows(p, B):
    H = p["encoder.weight_hh_l0"].shape[1]
    return [p[k].reshape(1, H).expand(B, H) for k in ("enc_h0", "enc_c0", "dec_h0", "dec_c0")]


def _ed_tail(p):
    Wi = p["decoder.weight_ih_l0"]
    return (Wi[:, 0], Wi[:, 1:], p["decoder.bias_ih_l0"] + p["decoder.bias_hh_l0"], p["decoder.weight_hh_l0"],
            p["out.0.weight"], p["out.0.bias"], p["out.2.weight"][0], p["out.2.bias"])


def ed_batch(p, x, mask, tgt_init=TGT_INIT, rounding=True):
    """x (B,T,in), mask (B,T) -> (B,T,1): MultiEDLSTM.forward in eval mode, taps mode, composed as the model composes its kernels"""
    B, T, _ = x.shape
    eh, ec, dh, dc = _ed_rows(p, B)
    ctx = front_batch(p, "encoder", x, mask, rounding, (eh, ec))
    w_p, W_c, bias, Whh, W1, b1, w2, b2 = _ed_tail(p)
    gxc = R.linear(ctx.transpose(0, 1), W_c, bias, rounding=rounding)
    q, _, _, _ = R.lstm_fb_scan(gxc, w_p, Whh, W1, b1, w2, b2, dh, dc, p_init=tgt_init, rounding=rounding)
    return (q.transpose(0, 1) * mask).unsqueeze(-1)


class EdStep:
    """step(x_t (B, in), mask_t (B) or None) -> y_t (B, 1), window by window from position 0"""

    def __init__(self, p, batch, tgt_init=TGT_INIT, rounding=True):
        self.p, self.B, self.rounding, self.tgt_init = p, int(batch), rounding, float(tgt_init)
        eh, ec, self.hd, self.cd = _ed_rows(p, self.B)
        self.front = _Front(p, "encoder", batch, rounding, (eh, ec))
        self.q = None

    def step(self, x, mask_t=None):
        B, rd = self.B, self.rounding
        m = _mask_of(x, mask_t, B)
        ctx = self.front.step(x, m)
        w_p, W_c, bias, Whh, W1, b1, w2, b2 = _ed_tail(self.p)
        gxc = R.linear(ctx.reshape(1, B, -1), W_c, bias, rounding=rd)
        q_prev = x.new_full((B,), self.tgt_init) if self.q is None else self.q
        q, h, c, _ = R.lstm_fb_scan(gxc, w_p, Whh, W1, b1, w2, b2, self.hd, self.cd, rounding=rd, mutate={"p": lambda _t, _p: q_prev})
        self.q, self.hd, self.cd = q[0], h[0], c[0]                        # the UNMASKED prediction is fed back
        return (q[0] * m).unsqueeze(-1)


# ------------------------------------------------------------------------------------------------ MultiARLSTM
def _ar_chain(in_part, w, hist):
    """acc = in_part; acc += w[..., k] * hist[k], k in index order"""
    acc = in_part
    for k in range(w.shape[-1]):
        acc = acc + w[..., k] * hist[k]
    return acc


def ar_parts(p, ctx, rounding=True):
    """ctx (..., H) -> in_part (...), w (..., K)"""
    hid, w = R.linear_pair(ctx, p["decoder.0.weight"], p["decoder.0.bias"], p["autoreg.weight"], p["autoreg.bias"], act1=1, rounding=rounding)
    return R.linear(hid, p["decoder.2.weight"], p["decoder.2.bias"], rounding=rounding).squeeze(-1), w


def ar_weights(p, x, mask, rounding=True):
    """the autoregressive coefficients w (B,T,K) of the batch model"""
    return ar_parts(p, front_batch(p, "lstm", x, mask, rounding), rounding)[1]


def ar_batch(p, x, mask, tgt_init=TGT_INIT, rounding=True):
    """x (B,T,in), mask (B,T) -> (B,T,1): MultiARLSTM.forward(target=None) in eval mode, taps mode"""
    B, T, _ = x.shape
    in_part, w = ar_parts(p, front_batch(p, "lstm", x, mask, rounding), rounding)
    K = w.shape[-1]
    preds = [x.new_full((B,), float(tgt_init))] * K
    for t in range(T):
        preds.append(_ar_chain(in_part[:, t], w[:, t], preds[t:t + K]))
    return (torch.stack(preds[K:], dim=1) * mask).unsqueeze(-1)


class ArStep:
    """step(x_t (B, in), mask_t (B) or None) -> y_t (B, 1); the history as csrc/lstm_step.h keeps it: a ring of K + 1 slots, step t
    writes slot t % (K + 1) and reads the slots (t - K + k) % (K + 1)"""

    def __init__(self, p, batch, tgt_init=TGT_INIT, rounding=True):
        self.p, self.B, self.rounding, self.tgt_init = p, int(batch), rounding, float(tgt_init)
        self.front = _Front(p, "lstm", batch, rounding)
        self.K = p["autoreg.weight"].shape[0]
        self.ring = [None] * (self.K + 1)

    def step(self, x, mask_t=None):
        B, K, t = self.B, self.K, self.front.t
        m = _mask_of(x, mask_t, B)
        in_part, w = ar_parts(self.p, self.front.step(x, m), self.rounding)
        init = x.new_full((B,), self.tgt_init)
        hist = [self.ring[(t - K + k) % (K + 1)] if t - K + k >= 0 else init for k in range(K)]
        assert all((t - K + k) % (K + 1) != t % (K + 1) for k in range(K))
        acc = _ar_chain(in_part, w, hist)
        self.ring[t % (K + 1)] = acc                                       # the UNMASKED prediction is fed back
        return (acc * m).unsqueeze(-1)


def stepped(make, x, mask=None):
    """make() -> an EdStep / ArStep; x (B,T,in), mask (B,T) or None -> (B,T,1): every window in order"""
    s = make()
    return torch.stack([s.step(x[:, t], None if mask is None else mask[:, t]) for t in range(x.shape[1])], dim=1)


# ------------------------------------------------------------------------------------------------ parameters and inputs
def _draw(p, tag, seed, name, shape, k):
    p[name] = (G.gen_normal("%s:%s" % (tag, name), shape, seed) * k).double()


def ed_params(in_dim, E, H, L, seed=11, tag="lstm_feedback_stream"):
    """fp64 parameters of a one-layer MultiEDLSTM under its own names; lstm_stream_ref.params' scales for what the models share"""
    base = LS.params(in_dim, E, H, 1, L, seed=seed, tag=tag)
    p = {}
    for k, v in base.items():
        p[k.replace("lstm.", "encoder.").replace("decoder.0.", "out.0.").replace("decoder.2.", "out.2.")] = v
    for name in ("enc_h0", "enc_c0", "dec_h0", "dec_c0"):
        _draw(p, tag, seed, name, (1, 1, H), 0.3)
    _draw(p, tag, seed, "decoder.weight_ih_l0", (4 * H, 1 + H), 1.0 / (1 + H) ** 0.5)
    _draw(p, tag, seed, "decoder.weight_hh_l0", (4 * H, H), 1.0 / H ** 0.5)
    _draw(p, tag, seed, "decoder.bias_ih_l0", (4 * H,), 0.1)
    _draw(p, tag, seed, "decoder.bias_hh_l0", (4 * H,), 0.1)
    return p


def ar_params(in_dim, E, H, n_layers, L, K, seed=11, tag="lstm_feedback_stream"):
    """fp64 parameters of a MultiARLSTM: lstm_stream_ref.params and autoreg, scaled so that sum_k |w[k]| stays below 1 (the recurrence on
    the predictions contracts: tests/test_lstm_feedback_stream_cpu.py asserts it)"""
    p = LS.params(in_dim, E, H, n_layers, L, seed=seed, tag=tag)
    _draw(p, tag, seed, "autoreg.weight", (K, H), 0.5 / (K * H ** 0.5))
    _draw(p, tag, seed, "autoreg.bias", (K,), 0.3 / K)
    return p


# The shapes of tests/test_gpu_lstm_feedback_stream.py; tests/test_lstm_feedback_stream_cpu.py holds the reference on the same ones.
# ED: (in, E, H, layers, taps, B, steps); AR: (in, E, H, layers, taps, B, steps, K)
ED_CASES = [(8, 8, 4, 1, 1, 1, 1),                # position 0 only: the prepared rows and tgt_init alone
            (12, 12, 20, 1, 3, 3, 7),             # k padded to 8, the ring of taps wraps; the mask has a hole
            (300, 128, 128, 1, 3, 3, 12),         # the batch path's limit
            (64, 128, 512, 1, 7, 2, 4),           # the default h_dim; reference only (the batch path does not take it)
            (16, 8, 8, 1, 3, 33, 4)]              # 33 workgroups
AR_CASES = [(8, 8, 4, 1, 1, 1, 1, 1),
            (12, 12, 20, 1, 3, 3, 7, 3),          # the history ring wraps
            (40, 64, 32, 4, 16, 2, 20, 16),       # K + 1 = 17 slots wrap once; taps and history both reach before step 0
            (300, 128, 256, 1, 7, 3, 12, 1),
            (64, 128, 512, 1, 7, 2, 4, 1),        # the default h_dim
            (16, 8, 8, 2, 3, 33, 4, 2)]
ED_IDS = ["ed_in%d_E%d_H%d_N%d_L%d_B%d_T%d" % c for c in ED_CASES]
AR_IDS = ["ar_in%d_E%d_H%d_N%d_L%d_B%d_T%d_K%d" % c for c in AR_CASES]
ED_HOLE = ED_CASES[1]


def ed_case(c, tag="lstm_feedback_stream"):
    """(parameters, x (B,T,in), mask (B,T)) of an ED case, fp64"""
    I, E, H, _, L, B, T = c
    return (ed_params(I, E, H, L, tag=tag),) + inputs(I, B, T, hole=c == ED_HOLE, tag=tag)


def ar_case(c, tag="lstm_feedback_stream"):
    I, E, H, NL, L, B, T, K = c
    return (ar_params(I, E, H, NL, L, K, tag=tag),) + inputs(I, B, T, tag=tag)


def inputs(in_dim, B, T, hole=False, tag="lstm_feedback_stream"):
    """x (B,T,in) and a prefix mask (B,T) (hole: ones with blanked windows in the middle of two recordings), fp64"""
    x = G.gen_normal("%s:x:%d:%d:%d" % (tag, in_dim, B, T), (B, T, in_dim), 7).double()
    mask = G.prefix_mask([max(1, T - (2 * b) % T) for b in range(B)], T).double().reshape(B, T)
    if hole:
        mask = torch.ones(B, T, dtype=torch.float64)
        mask[0, T // 2] = 0.0
        mask[B - 1, 1] = 0.0
    return x, mask
