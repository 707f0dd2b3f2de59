"""The bf16-faithful fp64 reference of CAUSAL attention (TEST INFRASTRUCTURE, a plain helper module beside tests/bf16_ref.py).

Query t of a sequence sees keys 0 .. t.  Built from bf16_ref's pieces (bf16, round_fwd / round_bwd, RESCALE_THR, the affine map and
LayerNorm of encoder_layer) with the same ``rounding`` switch: ``rounding=False`` is the exact function, softmax over scores with -inf
above the diagonal.

Sites, read from csrc/attn.h (the *_causal_kernel entries):
  * forward (attn_fwd_body, MODE = ATTN_CAUSAL): the wave of query tile qt sweeps key tiles 0 .. qt in order; the diagonal tile is
    masked (key > query, key >= T: -inf) BEFORE its maximum is taken; the running maximum moves at the first tile and when some query of
    the 32-query tile exceeds it by more than RESCALE_THR.  Scores of -inf above the diagonal give all of that: a tile behind the
    diagonal has maximum -inf, never moves the reference and contributes P = 0.  Query rows >= T of the last tile exist as Q' = 0 and
    take part in the wave's rescale decision, with the keys <= their own index that are < T;
  * backward (attn_bwd_dkv_body / attn_bwd_dq_body): as bf16_ref._AttnCore with P = 0 above the diagonal (a select: L of a query
    is the normaliser of its visible keys, so 2^(S' - L) of a later key can be inf).  Always the two-kernel form: no folded drop scale.
"""
import math

import torch

import bf16_ref as E
import oracle


def above_diagonal(T, Tq=None):
    """(Tq, T) bool: key index > query index"""
    return torch.arange(T).reshape(1, T) > torch.arange(T if Tq is None else Tq).reshape(-1, 1)


def _forward_value(Qp, K, V, prob_drop, ones_rowsum):
    """bf16_ref._attn_forward_value with the causal sweep: (B, h, T, d_k) bf16-valued fp64 operands -> (ctx before its final rounding, L)."""
    with torch.no_grad():
        B, h, T, dk = Qp.shape
        nt = -(-T // 32)
        Tp = nt * 32
        Qpad = torch.zeros(B, h, Tp, dk, dtype=Qp.dtype)
        Qpad[:, :, :T] = Qp                                    # query rows >= T exist in the last tile, as Q' = 0
        S = (Qpad @ K.transpose(-2, -1)).masked_fill(above_diagonal(T, Tp), float("-inf"))
        St = S.reshape(B, h, nt, 32, T)
        ms = []
        for kt in range(nt):                                   # query tiles qt < kt see -inf only: no move, and their m stays final
            tmax = St[..., 32 * kt: min(T, 32 * kt + 32)].amax(dim=-1)
            if kt == 0:
                m = tmax                                       # finite: key 0 is visible to every query
            else:
                rel = tmax - m
                move = (rel > E.RESCALE_THR).any(dim=-1, keepdim=True)
                m = torch.where(move, m + rel.clamp(min=0.0), m)
            ms.append(m)
        keep = None
        if prob_drop is not None:
            keep = torch.zeros(B, h, Tp, T, dtype=Qp.dtype)
            keep[:, :, :T] = (prob_drop != 0).to(Qp.dtype).expand(B, h, T, T)
            keep = keep.reshape(B, h, nt, 32, T)
        P, Pb = torch.empty_like(St), torch.empty_like(St)
        for kt in range(nt):
            c0, c1 = 32 * kt, min(T, 32 * kt + 32)
            p = torch.exp2(St[..., c0:c1] - ms[kt].unsqueeze(-1))          # 0 above the diagonal
            pk = p if keep is None else p * keep[..., c0:c1]
            alpha = torch.exp2(ms[kt] - ms[-1]).unsqueeze(-1)
            P[..., c0:c1] = p * alpha
            Pb[..., c0:c1] = E.bf16(pk) * alpha
        P = P.reshape(B, h, Tp, T)[:, :, :T]
        Pb = Pb.reshape(B, h, Tp, T)[:, :, :T]
        l = (Pb if ones_rowsum else P).sum(dim=-1, keepdim=True)
        L = ms[-1].reshape(B, h, Tp)[:, :, :T].unsqueeze(-1) + torch.log2(l)
        if prob_drop is None:
            return (Pb @ V) / l, L
        return (Pb @ V) * (float(prob_drop.max()) / l), L


class _CausalCore(torch.autograd.Function):
    """bf16_ref._AttnCore for causal attention: the recomputed P is zero above the diagonal."""
    @staticmethod
    def forward(ctx, Qp, K, V, prob_drop, ones_rowsum):
        val, L = _forward_value(Qp, K, V, prob_drop, ones_rowsum)
        out = E.bf16(val)
        ctx.save_for_backward(Qp, K, V, out, L)
        ctx.prob_drop = prob_drop
        return out

    @staticmethod
    def backward(ctx, dout):
        Qp, K, V, out, L = ctx.saved_tensors
        T = Qp.shape[-2]
        dO = E.bf16(dout)
        P = torch.exp2((Qp @ K.transpose(-2, -1)).masked_fill(above_diagonal(T), float("-inf")) - L)
        dP = dO @ V.transpose(-2, -1)
        delta = (dO * out).sum(dim=-1, keepdim=True)
        md = ctx.prob_drop
        dS = P * ((dP if md is None else dP * md) - delta)
        Pdr, dSr = E.bf16(P if md is None else P * md), E.bf16(dS)
        return E.LN2 * (dSr @ K), E.LN2 * (dSr.transpose(-2, -1) @ Qp), Pdr.transpose(-2, -1) @ dO, None, None


def _attention(q_lin, k_lin, v_lin, row_keep, prob_drop, rounding):
    """bf16_ref._attention, causal.  prob_drop: (B, h, T, T) multipliers; entries above the diagonal are never read."""
    rf, rb = E._sites(rounding)
    dk, T = q_lin.shape[-1], q_lin.shape[-2]
    Qs = rb(q_lin) * (E.LOG2E / math.sqrt(dk))
    if row_keep is not None:
        Qs = Qs * row_keep
    Qp, K, V = rf(Qs), rf(rb(k_lin)), rf(rb(v_lin))
    if rounding:
        return _CausalCore.apply(Qp, K, V, prob_drop, -(-dk // 16) * 16 == 16 and prob_drop is None)
    P = torch.softmax(((Qp @ K.transpose(-2, -1)) * E.LN2).masked_fill(above_diagonal(T), float("-inf")), dim=-1)
    if prob_drop is not None:
        P = P * prob_drop
    return P @ V


def sdpa(q, k, v, row_mask=None, prob_drop=None, rounding=True):
    """bf16_ref.sdpa's arguments (q, k, v: (B, h, T, d_k); row_mask (B, 1, T, 1)) -> (ctx, None), causal."""
    keep = None if row_mask is None else (row_mask != 0).to(q.dtype)
    return _attention(q, k, v, keep, prob_drop, rounding), None


def encoder_layer(p, prefix, x, mask, h, drops=None, rounding=True):
    """bf16_ref.encoder_layer with causal self-attention; every other line is that function's."""
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
    ctx = _attention(q, k, v, row_keep, dr.get("attn"), rounding)
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


def encoder_stack(p, prefix, x, mask, h, drops=None, rounding=True):
    """bf16_ref.encoder_stack's arguments; every layer's self-attention is causal."""
    for i in range(oracle.count_layers(p, prefix)):
        x = encoder_layer(p, "%slayers.%d." % (prefix, i), x, mask, h, None if drops is None else drops[i], rounding)
    return oracle.layer_norm(x, p[prefix + "norm.a_2"], p[prefix + "norm.b_2"])
