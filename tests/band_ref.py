"""The bf16-faithful fp64 reference of BAND attention (TEST INFRASTRUCTURE, a plain helper module beside tests/bf16_ref.py and
tests/causal_ref.py, whose pieces it imports).

Query t of a sequence sees keys max(0, t - span + 1) .. t.  Same ``rounding`` switch as bf16_ref: ``rounding=False`` is the exact
function, softmax over scores with -inf outside the band.

Sites, read from csrc/attn.h (the *_band_kernel entries):
  * forward (attn_fwd_body, MODE = ATTN_BAND): the wave of query tile qt sweeps key tiles qt, qt-1, .. band_lo_tile(qt) =
    max(0, floor((32 qt - span + 1) / 32)) — DOWNWARDS from the diagonal.  The partial tiles are masked (-inf) BEFORE their maximum is
    taken.  The running maximum is set to the tile maximum at the first tile, the diagonal one, where every row sees its own key, and
    moves afterwards when some query of the 32-query tile exceeds it by more than RESCALE_THR; a row without a visible key in a later
    tile has tile maximum -inf, never moves the reference and contributes P = 0.  Query rows >= T of the last tile exist as Q' = 0,
    see what row T-1 sees (the kernel clamps the query index) and take part in the wave's rescale decision;
  * backward (attn_bwd_dkv_body / attn_bwd_dq_body): causal_ref._CausalCore's with P = 0 outside the band (a select: L of a query is
    the normaliser of its visible keys, so 2^(S' - L) of an invisible key can be inf).  Always the two-kernel form.
"""
import math

import torch

import bf16_ref as E
import causal_ref as C
import oracle


def check_span(span):
    if isinstance(span, bool) or not isinstance(span, int) or span < 1:
        raise ValueError("span must be an int >= 1, got %r" % (span,))
    return span


def outside_band(T, span, Tq=None):
    """(Tq, T) bool: key index > query index or <= query index - span; a query row >= T counts as row T-1"""
    q = torch.arange(T if Tq is None else Tq).clamp(max=T - 1).reshape(-1, 1)
    k = torch.arange(T).reshape(1, T)
    return (k > q) | (k <= q - check_span(span))


def band_lo_tile(qt, span):
    return max(0, (32 * qt - span + 1) // 32)


def _forward_value(Qp, K, V, prob_drop, ones_rowsum, span):
    """causal_ref._forward_value with the band sweep: (B, h, T, d_k) bf16-valued fp64 operands -> (ctx before its final rounding, L)."""
    with torch.no_grad():
        B, h, T, dk = Qp.shape
        nt = -(-T // 32)
        Tp = nt * 32
        sp = min(span, T)
        Qpad = torch.zeros(B, h, Tp, dk, dtype=Qp.dtype)
        Qpad[:, :, :T] = Qp                                    # query rows >= T exist in the last tile, as Q' = 0
        S = (Qpad @ K.transpose(-2, -1)).masked_fill(outside_band(T, sp, Tp), float("-inf"))
        keep = None
        if prob_drop is not None:
            keep = torch.zeros(B, h, Tp, T, dtype=Qp.dtype)
            keep[:, :, :T] = (prob_drop != 0).to(Qp.dtype).expand(B, h, T, T)
        P, Pb = torch.zeros_like(S), torch.zeros_like(S)
        mfin = torch.empty(B, h, Tp, dtype=Qp.dtype)
        for qt in range(nt):
            rows = slice(32 * qt, 32 * qt + 32)
            Sq = S[:, :, rows]
            tiles = list(range(qt, band_lo_tile(qt, sp) - 1, -1))          # downwards from the diagonal
            ms, m = {}, None
            for kt in tiles:
                tmax = Sq[..., 32 * kt: min(T, 32 * kt + 32)].amax(dim=-1)
                if kt == qt:
                    m = tmax                                   # finite: every row sees its own key (row >= T: key T-1)
                else:
                    rel = tmax - m                             # -inf for a row without a visible key in this tile
                    move = (rel > E.RESCALE_THR).any(dim=-1, keepdim=True)
                    m = torch.where(move, m + rel.clamp(min=0.0), m)
                ms[kt] = m
            mfin[:, :, rows] = m
            for kt in tiles:
                c0, c1 = 32 * kt, min(T, 32 * kt + 32)
                p = torch.exp2(Sq[..., c0:c1] - ms[kt].unsqueeze(-1))      # 0 outside the band
                pk = p if keep is None else p * keep[:, :, rows, c0:c1]
                alpha = torch.exp2(ms[kt] - m).unsqueeze(-1)
                P[:, :, rows, c0:c1] = p * alpha
                Pb[:, :, rows, c0:c1] = E.bf16(pk) * alpha
        P, Pb = P[:, :, :T], Pb[:, :, :T]
        l = (Pb if ones_rowsum else P).sum(dim=-1, keepdim=True)
        L = mfin[:, :, :T].unsqueeze(-1) + torch.log2(l)
        if prob_drop is None:
            return (Pb @ V) / l, L
        return (Pb @ V) * (float(prob_drop.max()) / l), L


class _BandCore(torch.autograd.Function):
    """causal_ref._CausalCore for band attention: the recomputed P is zero outside the band."""
    @staticmethod
    def forward(ctx, Qp, K, V, prob_drop, ones_rowsum, span):
        val, L = _forward_value(Qp, K, V, prob_drop, ones_rowsum, span)
        out = E.bf16(val)
        ctx.save_for_backward(Qp, K, V, out, L)
        ctx.prob_drop, ctx.span = prob_drop, span
        return out

    @staticmethod
    def backward(ctx, dout):
        Qp, K, V, out, L = ctx.saved_tensors
        T = Qp.shape[-2]
        dO = E.bf16(dout)
        P = torch.exp2((Qp @ K.transpose(-2, -1)).masked_fill(outside_band(T, ctx.span), float("-inf")) - L)
        dP = dO @ V.transpose(-2, -1)
        delta = (dO * out).sum(dim=-1, keepdim=True)
        md = ctx.prob_drop
        dS = P * ((dP if md is None else dP * md) - delta)
        Pdr, dSr = E.bf16(P if md is None else P * md), E.bf16(dS)
        return E.LN2 * (dSr @ K), E.LN2 * (dSr.transpose(-2, -1) @ Qp), Pdr.transpose(-2, -1) @ dO, None, None, None


def _attention(q_lin, k_lin, v_lin, row_keep, prob_drop, rounding, span):
    """causal_ref._attention with a band.  prob_drop: (B, h, T, T) multipliers; entries outside the band are never read."""
    span = check_span(span)
    rf, rb = E._sites(rounding)
    dk, T = q_lin.shape[-1], q_lin.shape[-2]
    Qs = rb(q_lin) * (E.LOG2E / math.sqrt(dk))
    if row_keep is not None:
        Qs = Qs * row_keep
    Qp, K, V = rf(Qs), rf(rb(k_lin)), rf(rb(v_lin))
    if rounding:
        return _BandCore.apply(Qp, K, V, prob_drop, -(-dk // 16) * 16 == 16 and prob_drop is None, span)
    P = torch.softmax(((Qp @ K.transpose(-2, -1)) * E.LN2).masked_fill(outside_band(T, span), float("-inf")), dim=-1)
    if prob_drop is not None:
        P = P * prob_drop
    return P @ V


def sdpa(q, k, v, span, row_mask=None, prob_drop=None, rounding=True):
    """bf16_ref.sdpa's arguments (q, k, v: (B, h, T, d_k); row_mask (B, 1, T, 1)) and the span -> (ctx, None)."""
    keep = None if row_mask is None else (row_mask != 0).to(q.dtype)
    return _attention(q, k, v, keep, prob_drop, rounding, span), None


def encoder_layer(p, prefix, x, mask, h, span, drops=None, rounding=True):
    """causal_ref.encoder_layer with band self-attention; every other line is that function's."""
    rf, rb = E._sites(rounding)
    dr = drops or {}
    B, T, d = x.shape
    dk = d // h
    row_keep = None if mask is None else (mask.unsqueeze(1) != 0).to(x.dtype)

    def split(z):
        return z.reshape(B, T, h, dk).permute(0, 2, 1, 3)

    n0 = rf(oracle.layer_norm(x, p[prefix + "sublayer.0.norm.a_2"], p[prefix + "sublayer.0.norm.b_2"]))
    a = prefix + "self_attn.linears."
    q, k, v = (split(E._affine(p, a + str(i), n0, rf)) for i in range(3))
    ctx = _attention(q, k, v, row_keep, dr.get("attn"), rounding, span)
    merged = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    o = E._affine(p, a + "3", merged, rf)
    o = rb(o * dr["sub0"] if "sub0" in dr else o)
    x = x + o
    n1 = rf(oracle.layer_norm(x, p[prefix + "sublayer.1.norm.a_2"], p[prefix + "sublayer.1.norm.b_2"]))
    f = prefix + "feed_forward."
    hid = torch.relu(rb(E._affine(p, f + "w_1", n1, rf)))
    if "ffn" in dr:
        hid = hid * dr["ffn"]
    y = E._affine(p, f + "w_2", rf(hid), rf)
    y = rb(y * dr["sub1"] if "sub1" in dr else y)
    return x + y


def encoder_stack(p, prefix, x, mask, h, span, drops=None, rounding=True):
    """bf16_ref.encoder_stack's arguments and the span; every layer's self-attention has that span."""
    for i in range(oracle.count_layers(p, prefix)):
        x = encoder_layer(p, "%slayers.%d." % (prefix, i), x, mask, h, span, None if drops is None else drops[i], rounding)
    return oracle.layer_norm(x, p[prefix + "norm.a_2"], p[prefix + "norm.b_2"])
