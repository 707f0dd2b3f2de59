"""fp64 restatement of the stacked LSTM scan (csrc/scan_stack.h) and of the models that use it (TEST INFRASTRUCTURE, a plain helper).

The decoder recurrence of transformer/SFT/multiTransformer.py:463-483 with nn.LSTM(2d, d, L), gate order i, f, g, o, H = d:

    o_{-1} = 0 (NOT dec_h0[L-1]),  h^l_{-1} = h0[l],  c^l_{-1} = c0[l]
    g^0_t = gx0_t + [o_{t-1} ; h^0_{t-1}] P_0^T                       gx0 = enc W_ih_l0[:, d:]^T + b_ih_l0 + b_hh_l0
    g^l_t = bias_{l-1} + [h^{l-1}_t ; h^l_{t-1}] P_l^T                l = 1 .. L-1
    (h^l_t, c^l_t) = cell(g^l_t, c^l_{t-1}),  o_t = h^{L-1}_t

in numpy, forward and the hand-derived backward, so that nothing of torch's LSTM is in it.  With the x_a columns of P_0 zero and zero
initial states it is a plain stacked LSTM (nn.LSTM(E, H, L) on a whole sequence): pack_plain.  bf16=True rounds the operands of every
recurrent product (the state rows, the gate gradients and P) to bf16 as the kernels do; the sums stay fp64.  That mode is NOT faithful
for the gradients batched after the scan: backward() forms dP and dbias from the unrounded dG and the unrounded state rows, while the
device rounds both operands (dP_l = bf16(dG_l)^T bf16([x_a ; x_b]), dbias_{l-1} = colsum(bf16(dG_l))).  Against bf16_ref.lstm_stack_scan
at (T, B, H, L) = (13, 3, 40, 3) its dP differs by 2e-3 rel-L2 (1e-2 per row) and its dbias by 1e-3, while its forward, dgx0, dh0 and
dc0 agree to 1e-16 (tests/test_bf16_ref.py test_lstm_stack_ref_bf16_mode_leaves_the_batched_gradients_unrounded).  The bf16-faithful
tier (tests/test_gpu_bf16_stack_fb.py) uses bf16_ref.lstm_stack_scan, never this mode.
o_init="h0_top" is the WRONG reading o_{-1} = dec_h0[L-1], kept so that a test can show the fixtures tell the two apart.
"""
import numpy as np
import torch


def _bf16(a):
    """round-to-nearest-even to bf16, returned as float64"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def pack_decoder(params, L, prefix="decoder."):
    """(Wx, bias0, P, bias) from nn.LSTM(2d, d, L)'s parameters (a mapping name -> array)."""
    g = lambda n: np.asarray(params[prefix + n], dtype=np.float64)       # noqa: E731
    d = g("weight_hh_l0").shape[1]
    Wi0 = g("weight_ih_l0")
    P = [np.concatenate([Wi0[:, :d], g("weight_hh_l0")], axis=1)]
    bias = []
    for l in range(1, L):
        P.append(np.concatenate([g("weight_ih_l%d" % l), g("weight_hh_l%d" % l)], axis=1))
        bias.append(g("bias_ih_l%d" % l) + g("bias_hh_l%d" % l))
    return Wi0[:, d:], g("bias_ih_l0") + g("bias_hh_l0"), np.stack(P), np.stack(bias)


def forward(gx0, P, bias, h0=None, c0=None, o_init="zeros", bf16=False):
    """gx0 (T,B,4H), P (L,4H,2H), bias (L-1,4H), h0 / c0 (L,B,H) or None -> h_all, c_all (L,T,B,H), acts (L,T,B,4H)"""
    gx0, P, bias = (np.asarray(a, dtype=np.float64) for a in (gx0, P, bias))
    T, B, H4 = gx0.shape
    H, L = H4 // 4, P.shape[0]
    h = np.zeros((L, B, H)) if h0 is None else np.array(h0, dtype=np.float64)
    c = np.zeros((L, B, H)) if c0 is None else np.array(c0, dtype=np.float64)
    rnd = _bf16 if bf16 else (lambda a: a)
    Pr = rnd(P)
    o = h[L - 1].copy() if o_init == "h0_top" else np.zeros((B, H))
    h_all, c_all, acts = np.zeros((L, T, B, H)), np.zeros((L, T, B, H)), np.zeros((L, T, B, 4 * H))
    for t in range(T):
        for l in range(L):
            xa = o if l == 0 else h[l - 1]
            g = (gx0[t] if l == 0 else bias[l - 1]) + np.concatenate([rnd(xa), rnd(h[l])], axis=1) @ Pr[l].T
            i, f, gg, og = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
            c[l] = f * c[l] + i * gg
            h[l] = og * np.tanh(c[l])
            h_all[l, t], c_all[l, t], acts[l, t] = h[l], c[l], np.concatenate([i, f, gg, og], axis=1)
        o = h[L - 1]
    return h_all, c_all, acts


def backward(dh_top, P, h0, c0, h_all, c_all, acts, o_init="zeros", bf16=False):
    """dh_top (T,B,H) on h_all[L-1] -> dict(dgx0, dP, dbias, dh0, dc0, dG)"""
    P = np.asarray(P, dtype=np.float64)
    L, T, B, H = h_all.shape
    h0 = np.zeros((L, B, H)) if h0 is None else np.asarray(h0, dtype=np.float64)
    c0 = np.zeros((L, B, H)) if c0 is None else np.asarray(c0, dtype=np.float64)
    rnd = _bf16 if bf16 else (lambda a: a)
    Pr = rnd(P)
    dG = np.zeros((L, T, B, 4 * H))
    dxb, dc, dxa0 = np.zeros((L, B, H)), np.zeros((L, B, H)), np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        dxa_up = None
        for l in range(L - 1, -1, -1):
            dh = dxb[l] + (np.asarray(dh_top[t], dtype=np.float64) + dxa0 if l == L - 1 else dxa_up)
            a = acts[l, t]
            i, f, gg, og = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
            cp = c_all[l, t - 1] if t > 0 else c0[l]
            th = np.tanh(c_all[l, t])
            dct = dc[l] + dh * og * (1 - th * th)
            dg = np.concatenate([dct * gg * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - gg * gg), dh * th * og * (1 - og)], axis=1)
            dc[l] = dct * f
            dG[l, t] = dg
            dx = rnd(dg) @ Pr[l]                                         # (B, 2H) = [dx_a ; dx_b]
            dxb[l] = dx[:, H:]
            if l == 0:
                dxa0 = dx[:, :H]
            else:
                dxa_up = dx[:, :H]
    dh0 = dxb.copy()
    if o_init == "h0_top":
        dh0[L - 1] += dxa0
    # weight gradients: dP_l = sum_t dG_l[t]^T [x_a ; x_b][t] with the unrounded operands (batched fp32-input GEMMs on the device)
    dP = np.zeros_like(P)
    for l in range(L):
        hprev = np.concatenate([h0[l][None], h_all[l, :-1]], axis=0)
        if l == 0:
            o_first = h0[L - 1] if o_init == "h0_top" else np.zeros((B, H))
            xa = np.concatenate([o_first[None], h_all[L - 1, :-1]], axis=0)
        else:
            xa = h_all[l - 1]
        X = np.concatenate([xa, hprev], axis=2).reshape(T * B, 2 * H)
        dP[l] = dG[l].reshape(T * B, 4 * H).T @ X
    return dict(dgx0=dG[0], dP=dP, dbias=dG[1:].sum(axis=(1, 2)), dh0=dh0, dc0=dc.copy(), dG=dG)


class _StackFn(torch.autograd.Function):
    """the numpy recurrence as a torch node, so that the fp64 torch restatements of the models below can differentiate through it"""

    @staticmethod
    def forward(ctx, gx0, P, bias, h0, c0, o_init):
        n = [t.detach().numpy() for t in (gx0, P, bias, h0, c0)]
        h_all, c_all, acts = forward(*n, o_init=o_init)
        ctx.n, ctx.saved, ctx.o_init = n, (h_all, c_all, acts), o_init
        return torch.from_numpy(h_all[-1].copy())

    @staticmethod
    def backward(ctx, dh_top):
        _, P, _, h0, c0 = ctx.n
        g = backward(dh_top.numpy(), P, h0, c0, *ctx.saved, o_init=ctx.o_init)
        return tuple(torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("dgx0", "dP", "dbias", "dh0", "dc0")) + (None,)


def torch_stack(gx0, P, bias, h0, c0, o_init="zeros"):
    return _StackFn.apply(gx0, P, bias, h0, c0, o_init)


# ------------------------------------------------------------------------------------------------ the models, fp64 torch around the node
def _fc(p, name, x):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def decoder_model(p, x, mask, h, L, relu_embed, o_init="zeros"):
    """NLPTransformer (relu_embed: embed.1 + ReLU, transformer/SFT/multiTransformer.py:457-484) or UniTransformer (embed,
    transformer/MFT/multiTransformer.py:348-376) with an L-layer decoder, eval mode; p: name -> fp64 tensor."""
    from oracle.encoder_ref import encoder_stack
    e = torch.relu(_fc(p, "embed.1", x)) if relu_embed else _fc(p, "embed", x)
    enc = encoder_stack(p, "encoder.", e, mask, h)
    B, T, d = enc.shape
    Wi0 = p["decoder.weight_ih_l0"]
    P = [torch.cat([Wi0[:, :d], p["decoder.weight_hh_l0"]], dim=1)]
    bias = []
    for l in range(1, L):
        P.append(torch.cat([p["decoder.weight_ih_l%d" % l], p["decoder.weight_hh_l%d" % l]], dim=1))
        bias.append(p["decoder.bias_ih_l%d" % l] + p["decoder.bias_hh_l%d" % l])
    gx0 = enc.permute(1, 0, 2) @ Wi0[:, d:].t() + p["decoder.bias_ih_l0"] + p["decoder.bias_hh_l0"]
    h_top = torch_stack(gx0, torch.stack(P), torch.stack(bias), p["dec_h0"].expand(L, B, d), p["dec_c0"].expand(L, B, d), o_init)
    out = _fc(p, "out.2", torch.relu(_fc(p, "out.0", h_top)))                           # (T,B,1)
    return out.permute(1, 0, 2) * mask.to(x.dtype)


def local_attention(z, h, valid):
    """z (B,T,A) logits, h (T,B,H), valid (B,T): softmax over TIME, pad_packed zeros, convolve (transformer/SFT/models.py:10-25,195-216)"""
    B, T, A = z.shape
    a = torch.softmax(z, dim=1)
    hb = h.permute(1, 0, 2) * valid.unsqueeze(-1)
    out = torch.zeros(B, T, h.shape[2], dtype=z.dtype)
    for i in range(A):
        if i < T:
            out[:, i:, :] = out[:, i:, :] + a[:, i:, i:i + 1] * hb[:, :T - i, :]
    return out


def lstm_baseline(p, x, mask, L, last="decoder.2"):
    """MultiLSTM (transformer/SFT/models.py:144-225; last = decoder.3 for B1's copy, transformer/B1-LSTM/models.py:135-216) with an
    L-layer nn.LSTM, eval mode: a plain stacked LSTM is the recurrence above with no feedback columns and zero initial states."""
    embed = torch.relu(_fc(p, "embed.1", x))
    z = _fc(p, "attn.2", torch.relu(_fc(p, "attn.0", embed)))
    B, T, _ = embed.shape
    H = p["lstm.weight_hh_l0"].shape[1]
    P = [torch.cat([torch.zeros(4 * H, H, dtype=x.dtype), p["lstm.weight_hh_l0"]], dim=1)]
    bias = []
    for l in range(1, L):
        P.append(torch.cat([p["lstm.weight_ih_l%d" % l], p["lstm.weight_hh_l%d" % l]], dim=1))
        bias.append(p["lstm.bias_ih_l%d" % l] + p["lstm.bias_hh_l%d" % l])
    gx0 = embed.permute(1, 0, 2) @ p["lstm.weight_ih_l0"].t() + p["lstm.bias_ih_l0"] + p["lstm.bias_hh_l0"]
    zeros = torch.zeros(L, B, H, dtype=x.dtype)
    h_top = torch_stack(gx0, torch.stack(P), torch.stack(bias), zeros, zeros)
    ctx = local_attention(z, h_top, mask.reshape(B, T).to(x.dtype))
    return _fc(p, last, torch.relu(_fc(p, "decoder.0", ctx))) * mask.to(x.dtype)
