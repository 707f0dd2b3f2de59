"""Deterministic inputs in value regimes the unit-scale recipe never reaches (TEST INFRASTRUCTURE, a plain helper module, no GPU).

tests/test_value_regimes_cpu.py asserts on the references alone that every regime is reached at every shape used on the GPU and holds
the yardsticks of the widened bounds; tests/test_gpu_value_regimes.py runs the kernels on the same bits.

Attention (``attention(regime, ...)``): q, k, v, g of shape (B, T, d), h heads; u is the first feature of every head.  Every shift is
scaled by sqrt(d_k) / 4, so that d_k = 16 and 64 see comparable scores in the log2 domain S' = q . k log2(e) / sqrt(d_k):
  peaked   q * 12: the softmax is nearly one-hot in a good share of rows;
  cold     q + c u, k - c u: every visible score of every valid row is far below zero (the stored L < -140);
  hot      q + c u, k + c u: far above (L > 140);
  rising   q + 30 u, k_j . u = floor(j / 32) 2: the running maximum moves at every key tile;
  falling  q + 30 u, k_j . u = -floor(j / 32) 2: the first tile dominates, later tiles underflow to P = 0;
  step     q + 30 u, k_j + s u for j >= j0: keys from j0 on beat every earlier key of every valid query by more than 2^140.  With
           key_lengths = j0 they are the masked keys of the boundary tile; causally, the masked keys of the diagonal tile for the
           queries 32 floor(j0 / 32) <= t < j0.
LayerNorm (``layer_norm_input``): offset (x + 1000), tiny (1e-5 x), sub_eps (1e-7 x: a spread below eps = 1e-6), huge (1e4 x),
one_constant_row (row 1 all zero: sigma = 0).
Scans: ``long_memory`` opens the forget (retain) gates by +6 and lets the upstream gradient enter at the LAST step only, so the whole
backward carry is what the earlier steps' gradients consist of; ``overflow`` sets a fixed stride of pre-activations to +-200.
"""
import math

import numpy as np
import torch

import recipe as R

SEED = 29
COLD_C = 40.0                  # cold / hot shift
STEP_S = 28.0                  # step height (test_value_regimes_cpu.py holds the margin it gives)
Q_SHIFT = 30.0                 # rising / falling / step
FORGET_SHIFT = 6.0
SAT = 200.0                    # |pre-activation| of the overflow regime
ATTN_REGIMES = ("peaked", "cold", "hot", "rising", "falling", "step")
LN_REGIMES = ("offset", "tiny", "sub_eps", "huge", "one_constant_row")
LN_DECADE = {"offset": (0.5, 2.0), "tiny": (0.5e-5, 2e-5), "sub_eps": (0.5e-7, 2e-7), "huge": (0.5e4, 2e4)}


# ------------------------------------------------------------------------------------------------ attention
def attention(regime, B, T, d, h, j0=None):
    """-> q, k, v, g (B, T, d) fp32 of the regime; the same bits for every selection (plain, keyed, causal) and mode."""
    assert regime in ATTN_REGIMES and (regime == "step") == (j0 is not None)
    tag = "vr:attn:%d:%d:%d" % (T, d, h)
    q, k, v, g = (R.gen_normal(tag + n, (B, T, d), SEED) for n in "qkvg")
    dk = d // h
    a = math.sqrt(dk) / 4.0
    u = torch.zeros(d)
    u[::dk] = 1.0                                               # the first feature of every head
    j = torch.arange(T, dtype=torch.float32).reshape(1, T, 1)
    if regime == "peaked":
        q = q * 12.0
    elif regime == "cold":
        q, k = q + COLD_C * a * u, k - COLD_C * a * u
    elif regime == "hot":
        q, k = q + COLD_C * a * u, k + COLD_C * a * u
    elif regime in ("rising", "falling"):
        sign = 1.0 if regime == "rising" else -1.0
        # (k's own u component is replaced, not shifted: times Q' ~ 11 its unit noise would be as large as half a tile's step)
        q, k = q + Q_SHIFT * a * u, k * (1.0 - u) + sign * torch.floor(j / 32.0) * 2.0 * a * u
    else:
        q, k = q + Q_SHIFT * a * u, k + (j >= j0).float() * STEP_S * a * u
    return q.contiguous(), k.contiguous(), v, g


def attn_lengths(T):
    """[T, 2T/3]: the second sequence has blanked query rows"""
    return [T, max(1, (2 * T) // 3)]


def split_heads(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def log2_scores(q, k, h):
    """S' (B, h, T, T) fp64 from the bf16 operands Q' = bf16(q log2(e) / sqrt(d_k)) and bf16(k), as the kernels form them"""
    dk = q.shape[-1] // h
    Qp = (split_heads(q.double(), h) * (1.4426950408889634 / math.sqrt(dk))).to(torch.bfloat16).double()
    return Qp @ split_heads(k.double(), h).to(torch.bfloat16).double().transpose(-2, -1)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layer_norm_input(regime, M, d, tag="ln"):
    """-> x (M, d), gain a (d), bias b (d), upstream gradient g (M, d), fp32"""
    assert regime in LN_REGIMES
    t = "vr:%s:%d:%d" % (tag, M, d)
    x = R.gen_normal(t + "x", (M, d), SEED)
    a = 1.0 + 0.1 * R.gen_normal(t + "a", (d,), SEED)
    b = 0.1 * R.gen_normal(t + "b", (d,), SEED)
    g = R.gen_normal(t + "g", (M, d), SEED)
    if regime == "offset":
        x = x + 1000.0
    elif regime == "one_constant_row":
        x = x.clone()
        x[1] = 0.0
    else:
        x = x * {"tiny": 1e-5, "sub_eps": 1e-7, "huge": 1e4}[regime]
    return x, a, b, g


def layer_norm_fp64(x, a, b, eps=1e-6, inside=False):
    """The reference's LayerNorm (unbiased std, eps added to the std) spelled out; inside=True: the sqrt(var + eps) form it is NOT."""
    d = x.shape[-1]
    c = x - x.sum(dim=-1, keepdim=True) / d
    var = (c * c).sum(dim=-1, keepdim=True) / (d - 1)
    return a * c / (torch.sqrt(var + eps) if inside else torch.sqrt(var) + eps) + b


# ------------------------------------------------------------------------------------------------ scans
def last_step_only(g):
    """the upstream gradient of long_memory: zero except at the last step"""
    out = torch.zeros_like(g)
    out[-1] = g[-1]
    return out


def saturate(pre, stride=7):
    """overflow: entries 0, stride, 2 stride, .. of the flattened tensor +SAT, entries 3, 3 + stride, .. -SAT -> (tensor, +mask, -mask)"""
    flat = pre.clone().reshape(-1)
    idx = torch.arange(flat.numel())
    hi, lo = idx % stride == 0, idx % stride == 3
    flat[hi], flat[lo] = SAT, -SAT
    return flat.reshape(pre.shape), hi.reshape(pre.shape), lo.reshape(pre.shape)


def lstm(regime, T, B, H):
    """-> gx (T, B, 4H), W (4H, H), h0, c0 (B, H), gh, gc (T, B, H), and for overflow the +-SAT masks of gx (else None, None)"""
    tag = "vr:lstm:%d:%d:%d" % (T, B, H)
    gx = R.gen_normal(tag + "gx", (T, B, 4 * H), SEED)
    W = R.gen_normal(tag + "w", (4 * H, H), SEED) / np.sqrt(H)
    h0, c0 = (0.5 * R.gen_normal(tag + n, (B, H), SEED) for n in ("h0", "c0"))
    gh, gc = (R.gen_normal(tag + n, (T, B, H), SEED) for n in ("gh", "gc"))
    if regime == "long_memory":
        gx = gx.clone()
        gx[:, :, H:2 * H] += FORGET_SHIFT
        return gx, W, h0, c0, last_step_only(gh), last_step_only(gc), None, None
    assert regime == "overflow"
    gx, hi, lo = saturate(gx)
    return gx, W, h0, c0, gh, gc, hi, lo


def mfn(regime, T, B):
    """-> apre (T, B, 128), chat (T, B, 128), Wm (128, 128), W2 (2, 128, 64), b2 (2, 128), g (T, B, 128), +-SAT masks of apre"""
    tag = "vr:mfn:%d:%d" % (T, B)
    apre = R.gen_normal(tag + "a", (T, B, 128), SEED)
    chat = torch.tanh(R.gen_normal(tag + "c", (T, B, 128), SEED))
    Wm = R.gen_normal(tag + "wm", (128, 128), SEED) / np.sqrt(128)
    W2 = R.gen_normal(tag + "w2", (2, 128, 64), SEED) / 8
    b2 = 0.1 * R.gen_normal(tag + "b2", (2, 128), SEED)
    g = R.gen_normal(tag + "g", (T, B, 128), SEED)
    if regime == "long_memory":
        b2 = b2.clone()
        b2[0] += FORGET_SHIFT                                   # the retain gate
        return apre, chat, Wm, W2, b2, last_step_only(g), None, None
    assert regime == "overflow"
    apre, hi, lo = saturate(apre)
    return apre, chat, Wm, W2, b2, g, hi, lo


AR_SHAPE = (3, 130, 3)                                          # B, T, K: the free-running walk crosses its 64-step chunk twice


def ar_inputs():
    B, T, K = AR_SHAPE
    g = lambda n, shape: R.gen_normal("vr:ar:" + n, shape, SEED)      # noqa: E731
    w = g("w", (B, T, K))
    w = w / w.abs().sum(dim=2, keepdim=True) * 0.9                      # the slowest contraction test_gpu_arlstm allows
    return dict(c=g("c", (B, T, 1)), w=w, mask=torch.ones(B, T, 1), tgt=torch.zeros(B, T, 1), g=last_step_only(g("g", (B, T, 1)).transpose(0, 1)).transpose(0, 1))


def stack_case(T):
    from test_gpu_bf16_stack_fb import _sc
    return _sc(T, 3, 40, 2)                                     # STACK_CASES[0]'s shape


def fb_case(T):
    from test_gpu_bf16_stack_fb import _fc
    return _fc(T, 3, 40, 24)                                    # FB_CASES[0]'s shape


def stack_inputs(regime, T):
    """test_gpu_bf16_stack_fb.stack_inputs' scaling; long_memory: +6 on the forget quarter of gx0 (layer 0) and of every bias (layers
    >= 1), gate order i, f, g, o; the upstream gradient at the last step only"""
    c = stack_case(T)
    g = lambda n, shape: R.gen_normal("vr:stack:%d:%s" % (T, n), shape, SEED).double()      # noqa: E731
    B, H, L = c["B"], c["H"], c["L"]
    inp = dict(gx0=g("gx0", (T, B, 4 * H)), P=g("P", (L, 4 * H, 2 * H)) / np.sqrt(2 * H), bias=0.1 * g("bias", (L - 1, 4 * H)),
               h0=0.5 * g("h0", (L, B, H)), c0=0.5 * g("c0", (L, B, H)))
    w = g("w", (T, B, H))
    if regime == "long_memory":
        inp["gx0"][:, :, H:2 * H] += FORGET_SHIFT
        inp["bias"][:, H:2 * H] += FORGET_SHIFT
        return inp, last_step_only(w), None
    inp["gx0"], hi, lo = saturate(inp["gx0"])
    return inp, w, hi | lo


def fb_inputs(regime, T):
    c = fb_case(T)
    g = lambda n, shape: R.gen_normal("vr:fb:%d:%s" % (T, n), shape, SEED).double()      # noqa: E731
    B, H, Ew = c["B"], c["H"], c["E"]
    inp = dict(gxc=g("gxc", (T, B, 4 * H)), w_p=g("w_p", (4 * H,)) / np.sqrt(1 + H), W_hh=g("W_hh", (4 * H, H)) / np.sqrt(H),
               W1=g("W1", (Ew, H)) / np.sqrt(H), b1=0.1 * g("b1", (Ew,)), w2=g("w2", (Ew,)) / np.sqrt(Ew), b2=0.1 * g("b2", (1,)),
               h0=0.5 * g("h0", (B, H)), c0=0.5 * g("c0", (B, H)))
    w = g("w", (T, B))
    if regime == "long_memory":
        inp["gxc"][:, :, H:2 * H] += FORGET_SHIFT
        return inp, last_step_only(w), None
    inp["gxc"], hi, lo = saturate(inp["gxc"])
    return inp, w, hi | lo


def per_step(got, ref):
    """max_t ||got[t] - ref[t]|| / rms_t ||ref[t]|| of (T, ...) tensors: a carry dropped at step t is a 100 % error of every earlier
    step, however small those steps' share of the whole tensor is."""
    g = np.asarray(got, dtype=np.float64).reshape(len(got), -1)
    r = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    diff = np.linalg.norm(g - r, axis=1)
    return float(diff.max() / max(np.sqrt(np.mean(np.sum(r * r, axis=1))), 1e-300))


# one case per dispatch family, each at the smallest shape the bf16-faithful tier already has for it (test_gpu_bf16_scans.py)
LSTM_FAMILIES = (("u1", 3, 48), ("u2", 257, 48), ("gen", 513, 64), ("cl4", 2, 256), ("s256", 33, 256))      # (family, B, H)
MFN_FAMILIES = (("sw1", 3), ("sw2", 257), ("gen", 513))                                                      # (family, B)
LONG_T = (70, 130)
OVERFLOW_T = 9


# ------------------------------------------------------------------------------------------------ attention cases and references
ATTN_H, ATTN_B = 2, 2
ATTN_T, ATTN_DK = (33, 70, 290), (16, 64)
KEYED_STEPS = ((33, 32), (70, 40), (290, 270))                 # (T, j0): key_lengths = j0
CAUSAL_STEPS = ((70, 40), (290, 270))


def sdpa_cases():
    """every (selection, regime, T, d_k, j0) of the stand-alone attention; each runs in eval mode and at p = 0.1"""
    out = []
    for dk in ATTN_DK:
        for T in ATTN_T:
            out += [("plain", r, T, dk, None) for r in ("peaked", "cold", "hot", "rising", "falling")]
            out.append(("keyed", "cold", T, dk, None))
        out += [("keyed", "step", T, dk, j0) for T, j0 in KEYED_STEPS]
        for T, j0 in CAUSAL_STEPS:
            out += [("causal", "step", T, dk, j0), ("causal", "cold", T, dk, None), ("causal", "rising", T, dk, None)]
    return out


def probs_cases():
    """the materialised probabilities at T = 70: (selection, regime, T, d_k, j0)"""
    out = []
    for dk in ATTN_DK:
        for sel in ("plain", "keyed", "causal"):
            out += [(sel, "step", 70, dk, 40), (sel, "cold", 70, dk, None), (sel, "peaked", 70, dk, None)]
    return out


def case_id(case):
    sel, regime, T, dk, j0 = case
    return "%s_%s%s_T%d_dk%d" % (sel, regime, "" if j0 is None else str(j0), T, dk)


def key_lengths_of(case):
    """the key lengths of a keyed case: j0 for step (the hot keys are the masked ones), the query lengths otherwise"""
    sel, regime, T, dk, j0 = case
    return [j0] * ATTN_B if regime == "step" else attn_lengths(T)


def sdpa_inputs(case):
    """-> q, k, v, g, the query-row mask (B, T, 1), key lengths (keyed) or None.  Keyed: no upstream gradient on rows >= the key length
    (the truncated reference has no such rows)."""
    sel, regime, T, dk, j0 = case
    q, k, v, g = attention(regime, ATTN_B, T, ATTN_H * dk, ATTN_H, j0)
    kl = None
    if sel == "keyed":
        kl = key_lengths_of(case)
        g = g * R.prefix_mask(kl, T)
    return q, k, v, g, R.prefix_mask(attn_lengths(T), T), kl


def sdpa_reference(case, drop=None, dtype=torch.float64, fused_attn_bwd=True):
    """y, dq, dk, dv of the case from the references as they stand: bf16_ref.sdpa (plain), bf16_ref.sdpa of every sequence cut to its
    key length (keyed; rows >= the length are zero here), causal_ref.sdpa.  drop: (B, h, T, T) multipliers or None.  dtype float32:
    the same evaluation in fp32, the yardstick of the widened bounds."""
    import bf16_ref as E
    import causal_ref as C
    sel, regime, T, dk, j0 = case
    q, k, v, g, mask, kl = sdpa_inputs(case)
    h, B, d = ATTN_H, ATTN_B, ATTN_H * dk
    drop = None if drop is None else drop.to(dtype)
    if sel != "keyed":
        lt = [t.to(dtype).requires_grad_() for t in (q, k, v)]
        if sel == "plain":
            ctx, _ = E.sdpa(*(split_heads(t, h) for t in lt), mask.to(dtype).unsqueeze(1), drop, fused_attn_bwd=fused_attn_bwd)
        else:
            ctx, _ = C.sdpa(*(split_heads(t, h) for t in lt), mask.to(dtype).unsqueeze(1), drop)
        y = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
        y.backward(g.to(dtype))
        return {"y": y.detach().numpy(), "dq": lt[0].grad.numpy(), "dk": lt[1].grad.numpy(), "dv": lt[2].grad.numpy()}
    ref = {n: torch.zeros(B, T, d, dtype=dtype) for n in ("y", "dq", "dk", "dv")}
    for b, n in enumerate(kl):
        lt = [t[b:b + 1, :n].to(dtype).requires_grad_() for t in (q, k, v)]
        ctx, _ = E.sdpa(*(split_heads(t, h) for t in lt), mask[b:b + 1, :n].to(dtype).unsqueeze(1),
                        None if drop is None else drop[b:b + 1, :, :n, :n], fused_attn_bwd=False)
        y = ctx.permute(0, 2, 1, 3).reshape(1, n, d)
        y.backward(g[b:b + 1, :n].to(dtype))
        ref["y"][b, :n] = y.detach()[0]
        for name, t in zip(("dq", "dk", "dv"), lt):
            ref[name][b, :n] = t.grad[0]
    return {n: t.numpy() for n, t in ref.items()}


def zero_scale(ref, n):
    """dq and dk are analytically zero where one key takes a row's whole probability (rising at T = 33: the one-key tail tile beats the
    first tile by 2^21 at d_k = 16, 2^43 at d_k = 64).  Below 1e-4 of dv's norm the fp32 noise of the products (2^-24 of dv's scale per
    term) alone is beyond a 2e-3 bound on the tensor's own norm: such a tensor is measured on dv's scale, as the T = 1 rows of test_sdpa
    are -> the tensor to hand to gpu_harness.check as scale_ref, or None"""
    small = n in ("dq", "dk") and np.linalg.norm(ref[n]) < 1e-4 * np.linalg.norm(ref["dv"])
    return ref["dv"] if small else None


def sdpa_measures(got, ref, n):
    """(rel-L2, per-row maximum) as gpu_harness.check computes them, zero_scale included"""
    from gpu_harness import measures
    s = zero_scale(ref, n)
    if s is None:
        return measures(got[n], ref[n])
    d = np.asarray(got[n], dtype=np.float64) - ref[n]
    return float(np.linalg.norm(d) / np.linalg.norm(s)), float(np.abs(d).max() / np.sqrt(np.mean(s * s)))


def visible(case):
    """(B, 1, T, T) bool: the keys each query attends"""
    sel, regime, T, dk, j0 = case
    vis = torch.ones(ATTN_B, 1, T, T, dtype=torch.bool)
    if sel == "keyed":
        for b, n in enumerate(key_lengths_of(case)):
            vis[b, :, :, n:] = False
    elif sel == "causal":
        vis = vis & ~(torch.arange(T).reshape(1, T) > torch.arange(T).reshape(T, 1))
    return vis


def probs_reference(case):
    """fp64 softmax over the visible keys of the bf16 operands (a blanked query row: Q' = 0, uniform) -> (B, h, T, T), exact zeros
    elsewhere"""
    sel, regime, T, dk, j0 = case
    q, k, v, g, mask, kl = sdpa_inputs(case)
    S = log2_scores(q * mask, k, ATTN_H).masked_fill(~visible(case), float("-inf"))
    return torch.softmax(S * 0.6931471805599453, dim=-1)
