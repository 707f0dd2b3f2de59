"""A bf16-faithful fp64 reference of the hot kernels (TEST INFRASTRUCTURE, a plain helper module).

The plain references (``oracle.scaled_dot_attention``, ``oracle.encoder_stack`` and the fp64 affine map of the linear tests) carry no
bf16, so a test against them has to absorb the whole error of the bf16 design.  The functions here take the same arguments plus
``rounding``: with ``rounding=True`` they round to bf16 at every point where the kernels form a bf16 operand, with everything else in
fp64 on the CPU; gradients come from torch autograd.  What is left between a kernel and this reference is fp32-vs-fp64 accumulation
order, the hardware exp2 / log2 / reciprocal, and a few sites noted below that are not emulated.  With ``rounding=False`` every
function is the plain reference again (tests/test_bf16_ref.py holds them to 1e-12).

Two primitives place the roundings:
  * ``round_fwd(t)``: bf16 round-to-nearest-even in the forward, straight-through in the backward;
  * ``round_bwd(t)``: identity in the forward, rounds the incoming gradient to bf16 in the backward.

Sites, read from the kernel sources (csrc/):
  * weights: every prepared weight is bf16 (pad_cast_kernel);
  * affine map (api.hip linear_*): A = bf16(drop_in(x)) (rowgemm staging; misc_kernels.h cast_rows_kernel), y = rowscale * drop_out(act(A W^T + b))
    in fp32; the backward operand g = bf16(dy * rowscale * act' * 1/(1-p_out)) (grad_prep_kernel) -> dx = (g W) * drop_in' in fp32,
    dW = g^T A, db = colsum(g);
  * encoder layer: xn1 = bf16(LN1(x)), Q' = bf16((xn1 Wq^T + bq) log2(e)/sqrt(d_k)) with blanked query rows Q' = 0, K = bf16(.),
    V = bf16(.) (rowgemm.h EPI_FRAG); ctx = bf16(.) (attn.h); x1 = x + drop(ctx Wo^T + bo) in fp32; xn2 = bf16(LN2(x1));
    hid = bf16(drop(ReLU(xn2 W1^T + b1))) (EPI_PLAIN, KEEP_A2); x2 = x1 + drop(hid W2^T + b2); LayerNorm statistics, the residual
    stream and the final LayerNorm in fp32;
  * backward of a layer: the MFMA operands dx2 (into W2), dh (into W1), dx1 (into Wo), dO (= dctx, rowgemm.h EPI_FRAG with delta)
    and dQKV are bf16; dQKV is formed by the attention kernels as bf16(dQ / sqrt(d_k)), bf16(ln2 dK'), bf16(dV);
  * attention forward (attn_fwd_kernel): scores in the log2 domain, P = 2^(S' - m) relative to a LAZILY rescaled running maximum m
    (MMT_RESCALE_THR: m moves only at the first key tile and when some query of the 32-query tile exceeds it by more than 8), P rounded
    to bf16 (dropped entries zeroed) before P V, the normaliser l summing the fp32 P — except at d_k <= 16 in eval mode, where it sums
    the bf16 P through the ones-row of the MFMA; ctx = bf16(O * (1/(1-p)) / l).  This is emulated tile by tile (``_attn_forward_value``);
  * attention backward (attn.h dkv / dq kernels, attn_bwd_pair.h): P is recomputed from the stored L = m + log2 l, delta = rowsum(dO . ctx)
    from the bf16 dO and the bf16 ctx (not sum_j P_j dP_j: the difference is coherent along a row, ~1e-2 of a dQ row), the recomputed P
    (with the drop multiplier) is bf16 in dV = P^T dO, dS = P (dP - delta) is bf16 in dK and dQ (``_AttnCore``, an explicit backward).

  * the one-kernel backward in train mode (attn_bwd_pair.h) rounds P m / c and dS / c, c = 1/(1-p), and scales the sums by c: a
    different rounding of the same operands, but dQ = sum_j dS_j K_j cancels (sum_j dS_j = 0), so it moves dQ by ~3.5e-3 rel-L2.

  * LSTM scan forward (scan_units.h:56,123, scan256.h:61,122, scan_cluster.h:89,140, scan.h:70,127): the MFMA operands bf16(h_{t-1})
    (h0 included) and bf16(W_rec); gx, the gate pre-activations and activations, c and the stored h are fp32.  Backward
    (scan_units.h:247, scan256.h:218, scan_cluster.h:244, scan.h:214): the recurrent product dh_{t-1} = bf16(dG_t) W_rec; dgx = dG in
    fp32; dW_rec = bf16(dG)^T bf16(h_prev) (functional._wgrad).  One line places all of it (``lstm_scan``):
        pre_t = gx_t + round_bwd(round_fwd(h_{t-1}) @ round_fwd(W_rec)^T);
  * MFN memory scan forward (mfn_scan.h, mfn_mem_scan_fwd_kernel :36-121, and the _sw twins): u = drop(ReLU(apre + bf16(mem) bf16(Wm)^T)), z_g = bf16(u_g) bf16(W2_g)^T
    + b2_g, mem = sigmoid(z_1) mem + sigmoid(z_2) chat; mem and everything written stays fp32.  Backward: du = bf16(dz) W2, dmem
    from bf16(dapre) Wm; dapre, dchat and dz are fp32; dWm, dW2 and db2 go through _wgrad, which rounds its operand, so
    db2 = colsum(bf16(dz)) (``mfn_mem_scan``: the bias sits inside round_bwd).
  * stacked LSTM scan forward (scan_stack.h lstm_stack_fwd_kernel): the MFMA operands (:138-140) are the bf16 state tiles [x_a ; x_b]
    and bf16(P_l) (lstm_stack_prep_kernel :38); every layer's h tile is bf16, h0 included (:82, :153); the zeros tile (:58, :115)
    stands for o_{-1}; gx0, the biases of layers >= 1 (:75, :146-149), the gates, c and the stored h_all / c_all / acts (:160-163) are
    fp32.  Backward (lstm_stack_bwd_kernel): [dx_a ; dx_b] = bf16(dG^l_t) bf16(P_l) (:251 the gradient tile, :45 the fragments,
    :278-279 the two halves), dgx0 = dG^0 in fp32 (:258-259), dh0 = the carried x_b half in fp32 (:298).  Batched after the scan
    (functional.py _LstmStackScanFn.backward :641-642, through _wgrad): dP_l = bf16(dG_l)^T bf16([x_a ; x_b]) with the operand rows
    taken from the fp32 h_all / h0 (their bf16 is the LDS tile's), dbias_{l-1} = colsum(bf16(dG_l)).  One line per layer-step
    (``lstm_stack_scan``): pre^0_t = gx0_t + round_bwd(round_fwd([o_{t-1} ; h^0_{t-1}]) @ round_fwd(P_0)^T),
    pre^l_t = round_bwd(round_fwd([h^{l-1}_t ; h^l_{t-1}]) @ round_fwd(P_l)^T + bias_{l-1});
  * feedback LSTM scan forward (scan_fb.h lstm_fb_scan_fwd_kernel): gates_t = gxc_t + p_{t-1} w_p + bf16(h_{t-1}) bf16(W_hh)^T with the
    p w_p term in fp32 (:182-183; the h tile :100, :187; the fragments lstm_fb_prep_kernel :32, :41); the read-out product reads the
    SAME h tile as the next step's gate product (:172-176, the last step :213-218); u_t = ReLU(. + b1) stored unrounded (:141-143),
    p_t = b2 + the wave partial sums of w2 . u in fp32 (:142, :147-155).  Backward (lstm_fb_scan_bwd_kernel): dp_t = g_t + dG_{t+1} . w_p
    from the fp32 dG (:310-312, :343), du_t = dp_t w2 [u_t > 0] stored fp32 and fed to the MFMA as bf16 (:321-323),
    dh_t = bf16(dG_{t+1}) bf16(W_hh) + bf16(du_t) bf16(W1) (:300, :332, the tile :340), dgxc = dG in fp32 (:351).  Batched after the
    scan (functional.py _LstmFbScanFn.backward, through _wgrad): [dW_hh | dw_p] = bf16(dG)^T bf16([h_prev | p_prev]) (:744),
    dW1 = bf16(du)^T bf16(h), db1 = colsum(bf16(du)) (:749), dw2 = bf16(dp)^T bf16(u), db2 = sum(bf16(dp)) (:752).  ``lstm_fb_scan``:
    the two terms whose two gradients are rounded differently are explicit Functions (``_FbGates``: p w_p + the recurrent product;
    ``_FbReadout``: w2 . u + b2), the read-out layer is round_bwd(round_fwd(h) @ round_fwd(W1)^T + b1).

  * window encoder forward (convpool.h): weights bf16 (convpool_prep_kernel, :43), the raw rows bf16 while staging (:103-107); the sums
    S[n, p, f] = bf16(x)[n, p] . bf16(w)[f, :, 0] + bf16(x)[n, p+1] . bf16(w)[f, :, 1] in fp32; the pool takes the FIRST maximum (:169
    inside a lane, :173 across the two lane halves, :175 across row tiles: strictly greater replaces) over positions < W - 1 (:168);
    the bias is added after the pool, in fp32 (:188).  Backward (convpool_bwd_kernel): dW[f, d, j] = sum_n bf16(dy[n, f])
    bf16(x[n, arg + j, d]) (:312 the one-hot A operand, :264-272 the transposed rows), db[f] = sum_n dy[n, f] from the UNROUNDED dy
    (:299).  ``conv_maxpool`` places it in one line: out = round_bwd(gather(S, arg)) + b;
  * tanh / sigmoid epilogues of the affine map (rowgemm.h:387-392): on the fp32 sum + bias, output fp32.  The backward takes act' from
    the SAVED fp32 OUTPUT (misc_kernels.h grad_prep_kernel, act 2 and 3: 1 - y^2, y (1 - y)), multiplies in fp32 and rounds once:
    g = bf16(dy * rowscale * act'(y)), the same place as the ReLU's, so ``linear`` keeps its one round_bwd in front of the activation;
  * Highway (functional._HighwayFn, glue.h:97-125): proj = linear(x, act 0 or 1), gate = linear(x, act 3), both fp32;
    out = drop * (x + gate * (proj - x)) in fp32 from the UNROUNDED x (:105); backward g = drop * dout, dx = g (1 - gate), dproj = g gate,
    dgate = g (proj - x) in fp32 (:122); dproj and dgate become bf16 operands inside the two affine backwards (grad_prep_kernel),
    dx sums the three fp32 paths (copy2d).  ``linear_pair`` is two affine maps of one input, dx their fp32 sum.

Not emulated: the fp32 hardware exp2 / log2 / reciprocal (the scans' sigmoid_f / tanh_f, scan_common.h:12-13; tanh_f(x) = 2 sigmoid(2x) - 1 loses
relative accuracy near 0, about 6e-8 absolute, so every measure of the scans is per row, never per element; the affine map's tanh and
sigmoid epilogues are the same two formulas), and the kernels' fp32
accumulation order.  The latter cannot be: fp32 noise (~1e-7) tips a
few bf16 roundings to the other neighbour, a whole bf16 ulp of that element, and a tipped hidden pre-activation near 0 flips a ReLU mask.
``jitter`` reproduces the effect on the reference itself (tests/test_bf16_ref.py test_fp32_noise_tips_bf16_roundings): at d = 256 it
moves the stack's output by ~7e-4, dx by ~6e-3 and the FFN gradients by ~3e-2, the size of what remains between kernels and reference.
"""
import math

import torch

import oracle

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
RESCALE_THR = 8.0           # attn.h MMT_RESCALE_THR


_JITTER = None      # (generator, relative size): see jitter()
_JITTER_INPUTS = True
_JITTER_COMPUTED_ONLY = False


def bf16(t):
    """bf16 round-to-nearest-even of an fp64 tensor, back in fp64 (no autograd)."""
    if _JITTER is not None:
        g, eps = _JITTER
        noisy = t * (1 + eps * torch.randn(t.shape, generator=g, dtype=t.dtype))
        t = torch.where(t.to(torch.float32).to(t.dtype) == t, t, noisy) if _JITTER_COMPUTED_ONLY else noisy
    return t.to(torch.bfloat16).to(t.dtype)


class jitter:
    """Within this context every value is perturbed by a relative `eps` (normal) just before it is rounded to bf16: what a different
    fp32 accumulation order does to the kernels' values.  Two runs of the reference, with and without, measure how far apart two
    equally correct implementations land when fp32 noise tips bf16 roundings (tests/test_bf16_ref.py).
    inputs=False: ``linear`` rounds its x and W unperturbed, as for a stand-alone affine map or Highway, whose x and W are given fp32
    data with the same bf16 value in every implementation; only computed values (the backward's operands) are perturbed.
    computed_only=True: in every function, an element that is exactly an fp32 number is rounded unperturbed.  Given data (fp32 weights,
    inputs, their copies and concatenations, exact zeros) has the same bf16 value in every implementation; a value computed in fp64 is
    an fp32 number only by a 2^-29 chance.  For compositions whose pieces round weights and inputs at many sites (the MFN gate)."""
    def __init__(self, eps, seed=0, inputs=True, computed_only=False):
        self.eps, self.seed, self.inputs, self.computed_only = eps, seed, inputs, computed_only

    def __enter__(self):
        global _JITTER, _JITTER_INPUTS, _JITTER_COMPUTED_ONLY
        _JITTER, _JITTER_INPUTS = (torch.Generator().manual_seed(self.seed), self.eps), self.inputs
        _JITTER_COMPUTED_ONLY = self.computed_only

    def __exit__(self, *a):
        global _JITTER, _JITTER_INPUTS, _JITTER_COMPUTED_ONLY
        _JITTER, _JITTER_INPUTS, _JITTER_COMPUTED_ONLY = None, True, False


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


def round_fwd(t):
    return _RoundFwd.apply(t)


def round_bwd(t):
    return _RoundBwd.apply(t)


def _sites(rounding):
    ident = (lambda t: t)
    return (round_fwd, round_bwd) if rounding else (ident, ident)


# ------------------------------------------------------------------------------------------------ affine map
def linear(x, W, b=None, act=0, rowscale=None, in_drop=None, out_drop=None, rounding=True, mutate=None):
    """y = rowscale * out_drop * act(in_drop * x W^T + b), act 0 (none), 1 (ReLU), 2 (tanh) or 3 (sigmoid); in_drop / out_drop are
    dropout multipliers shaped like x / y.  The plain form is the one of test_linear and test_linear_fused_dropout_replay.
    mutate (tests only): {"act": f(pre) -> y in place of the activation}."""
    rf, rb = _sites(rounding)
    xa = x * in_drop if in_drop is not None else x
    if rounding and not _JITTER_INPUTS:
        rf = _RoundInput.apply
    y = rf(xa) @ rf(W).t()
    if b is not None:
        y = y + b
    y = rb(y)                                                   # g = bf16(dy * rowscale * act'): one rounding, in front of the activation
    if mutate and "act" in mutate:
        y = mutate["act"](y)
    elif act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.tanh(y)
    elif act == 3:
        y = torch.sigmoid(y)
    elif act != 0:
        raise NotImplementedError("bf16_ref.linear: act %d" % act)
    if out_drop is not None:
        y = y * out_drop
    if rowscale is not None:
        y = y * rowscale.reshape(-1, *([1] * (y.dim() - 1)))
    return y


# ------------------------------------------------------------------------------------------------ attention core
def _attn_forward_value(Qp, K, V, prob_drop, ones_rowsum):
    """The forward value of attn_fwd_kernel from the bf16 operands Q' (log2 domain), K, V: (B, h, T, d_k) fp64 -> ctx before its final
    rounding.  Query tiles of 32 rows share one rescale decision (one wave); key tiles of 32 are swept in order."""
    with torch.no_grad():
        B, h, T, dk = Qp.shape
        nt = -(-T // 32)
        Tp = nt * 32
        Qpad = torch.zeros(B, h, Tp, dk, dtype=Qp.dtype)
        Qpad[:, :, :T] = Qp                                    # query rows >= T exist in the last tile, as Q' = 0
        S = Qpad @ K.transpose(-2, -1)                         # (B, h, Tp, T), log2 domain
        St = S.reshape(B, h, nt, 32, T)
        ms = []
        for kt in range(nt):
            tile = St[..., 32 * kt: min(T, 32 * kt + 32)]
            tmax = tile.amax(dim=-1)                           # (B, h, nt, 32)
            if kt == 0:
                m = tmax
            else:
                rel = tmax - m
                move = (rel > RESCALE_THR).any(dim=-1, keepdim=True)      # __any over the wave's 32 queries
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
            p = torch.exp2(St[..., c0:c1] - ms[kt].unsqueeze(-1))          # what the tile rounds, relative to the maximum of its time
            pk = p if keep is None else p * keep[..., c0:c1]
            alpha = torch.exp2(ms[kt] - ms[-1]).unsqueeze(-1)              # the later rescales of o and l (fp32, after the rounding)
            P[..., c0:c1] = p * alpha
            Pb[..., c0:c1] = bf16(pk) * alpha
        P = P.reshape(B, h, Tp, T)[:, :, :T]
        Pb = Pb.reshape(B, h, Tp, T)[:, :, :T]
        l = (Pb if ones_rowsum else P).sum(dim=-1, keepdim=True)
        L = ms[-1].reshape(B, h, Tp)[:, :, :T].unsqueeze(-1) + torch.log2(l)        # the row constant the backward recomputes P from
        if prob_drop is None:
            return (Pb @ V) / l, L
        scale = float(prob_drop.max())
        return (Pb @ V) * (scale / l), L


class _AttnCore(torch.autograd.Function):
    """ctx = attention(Q', K, V) on the bf16 operands: the forward kernel's value (rounded), the backward kernels' gradients.
    Backward (attn.h attn_bwd_dkv_kernel / attn_bwd_dq_kernel): dO = bf16(dctx); P = 2^(S' - L) recomputed; dP = dO V^T;
    delta = rowsum(dO . ctx) from the bf16 ctx; dS = P (dP m - delta) with m the drop multiplier; dV = bf16(P m)^T dO;
    dK' = ln2 bf16(dS)^T Q'; dQ' = ln2 bf16(dS) K."""
    @staticmethod
    def forward(ctx, Qp, K, V, prob_drop, ones_rowsum, fold_drop):
        val, L = _attn_forward_value(Qp, K, V, prob_drop, ones_rowsum)
        out = bf16(val)
        ctx.save_for_backward(Qp, K, V, out, L)
        ctx.prob_drop, ctx.fold_drop = prob_drop, fold_drop
        return out

    @staticmethod
    def backward(ctx, dout):
        Qp, K, V, out, L = ctx.saved_tensors
        dO = bf16(dout)
        P = torch.exp2(Qp @ K.transpose(-2, -1) - L)
        dP = dO @ V.transpose(-2, -1)
        delta = (dO * out).sum(dim=-1, keepdim=True)
        md = ctx.prob_drop
        dS = P * ((dP if md is None else dP * md) - delta)
        Pd = P if md is None else P * md
        if ctx.fold_drop:           # attn_bwd_pair.h in train mode rounds P m / c and dS / c (c = 1/(1-p)), and scales the sums by c
            c = float(md.max())
            Pdr, dSr = bf16(Pd / c) * c, bf16(dS / c) * c
        else:
            Pdr, dSr = bf16(Pd), bf16(dS)
        dV = Pdr.transpose(-2, -1) @ dO
        return LN2 * (dSr @ K), LN2 * (dSr.transpose(-2, -1) @ Qp), dV, None, None, None


def one_kernel_bwd(dk, T):
    """Whether the attention backward runs as ONE kernel (attn_bwd_pair.h attn_bwd_fused_ok: d_k <= 16, 9..16 key tiles)."""
    return -(-dk // 16) * 16 == 16 and 8 < -(-T // 32) <= 16


def _attention(q_lin, k_lin, v_lin, row_keep, prob_drop, rounding, fused_attn_bwd=True):
    """q_lin, k_lin, v_lin: (B, h, T, d_k) as their producers form them (before Q's softmax scale); row_keep (B, 1, T, 1) or None.
    -> ctx (B, h, T, d_k).  With rounding=False this is oracle.scaled_dot_attention (a blanked row as Q' = 0 soft-maxes to the same
    uniform row as the reference's -1e9 and passes no gradient to q)."""
    rf, rb = _sites(rounding)
    dk = q_lin.shape[-1]
    Qs = rb(q_lin) * (LOG2E / math.sqrt(dk))
    if row_keep is not None:
        Qs = Qs * row_keep
    Qp, K, V = rf(Qs), rf(rb(k_lin)), rf(rb(v_lin))
    if rounding:
        fold = prob_drop is not None and fused_attn_bwd and one_kernel_bwd(dk, Qp.shape[-2])
        return _AttnCore.apply(Qp, K, V, prob_drop, -(-dk // 16) * 16 == 16 and prob_drop is None, fold)
    P = torch.softmax((Qp @ K.transpose(-2, -1)) * LN2, dim=-1)
    if prob_drop is not None:
        P = P * prob_drop
    return P @ V


def sdpa(q, k, v, row_mask=None, prob_drop=None, rounding=True, fused_attn_bwd=True):
    """Same arguments as oracle.scaled_dot_attention (q, k, v: (B, h, T, d_k); row_mask (B, 1, T, 1)) -> (ctx, None).
    Emulates the stand-alone attention (mmt_sdpa_*): Q' = bf16(q log2(e)/sqrt(d_k)), K, V, dq, dk, dv all bf16.
    fused_attn_bwd=False: the two-kernel backward (MMT_NO_FUSED_ATTN_BWD=1) where the one-kernel backward would run."""
    keep = None if row_mask is None else (row_mask != 0).to(q.dtype)
    return _attention(q, k, v, keep, prob_drop, rounding, fused_attn_bwd), None


# ------------------------------------------------------------------------------------------------ encoder stack
def _affine(p, name, x, rf):
    return x @ rf(p[name + ".weight"]).transpose(0, 1) + p[name + ".bias"]


def encoder_layer(p, prefix, x, mask, h, drops=None, rounding=True, fused_attn_bwd=True):
    rf, rb = _sites(rounding)
    dr = drops or {}
    B, T, d = x.shape
    dk = d // h
    row_keep = None if mask is None else (mask.unsqueeze(1) != 0).to(x.dtype)

    def split(z):
        return z.reshape(B, T, h, dk).permute(0, 2, 1, 3)

    n0 = rf(oracle.layer_norm(x, p[prefix + "sublayer.0.norm.a_2"], p[prefix + "sublayer.0.norm.b_2"]))
    a = prefix + "self_attn.linears."
    q, k, v = (split(_affine(p, a + str(i), n0, rf)) for i in range(3))
    ctx = _attention(q, k, v, row_keep, dr.get("attn"), rounding, fused_attn_bwd)
    merged = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    o = _affine(p, a + "3", merged, rf)
    o = rb(o * dr["sub0"] if "sub0" in dr else o)               # dx1 (into Wo) is a bf16 operand
    x = x + o
    n1 = rf(oracle.layer_norm(x, p[prefix + "sublayer.1.norm.a_2"], p[prefix + "sublayer.1.norm.b_2"]))
    f = prefix + "feed_forward."
    hid = torch.relu(rb(_affine(p, f + "w_1", n1, rf)))         # dh (into W1) is a bf16 operand
    if "ffn" in dr:
        hid = hid * dr["ffn"]
    y = _affine(p, f + "w_2", rf(hid), rf)
    y = rb(y * dr["sub1"] if "sub1" in dr else y)               # dx2 (into W2) is a bf16 operand
    return x + y


def encoder_stack(p, prefix, x, mask, h, drops=None, rounding=True, fused_attn_bwd=True):
    """Same arguments as oracle.encoder_stack."""
    for i in range(oracle.count_layers(p, prefix)):
        x = encoder_layer(p, "%slayers.%d." % (prefix, i), x, mask, h, None if drops is None else drops[i], rounding, fused_attn_bwd)
    return oracle.layer_norm(x, p[prefix + "norm.a_2"], p[prefix + "norm.b_2"])


def encoder_param_shapes(d, d_ff, n):
    """{state_dict name: shape} of an n-layer encoder, in the order of Encoder.flat_parameters() (the fused stack's flat buffer)."""
    s = {}
    for i in range(n):
        L = "layers.%d." % i
        for j in range(4):
            s[L + "self_attn.linears.%d.weight" % j] = (d, d)
            s[L + "self_attn.linears.%d.bias" % j] = (d,)
        s[L + "feed_forward.w_1.weight"], s[L + "feed_forward.w_1.bias"] = (d_ff, d), (d_ff,)
        s[L + "feed_forward.w_2.weight"], s[L + "feed_forward.w_2.bias"] = (d, d_ff), (d,)
        for j in range(2):
            s[L + "sublayer.%d.norm.a_2" % j] = (d,)
            s[L + "sublayer.%d.norm.b_2" % j] = (d,)
    s["norm.a_2"], s["norm.b_2"] = (d,), (d,)
    return s


# ------------------------------------------------------------------------------------------------ scans
def lstm_scan(gx, W, h0=None, c0=None, rounding=True, mutate=None):
    """Same arguments as functional.lstm_scan: gx (T, B, 4H) = x W_ih^T + b_ih + b_hh, W (4H, H), h0 / c0 (B, H) or None (zeros), gate
    order i, f, g, o -> (h_all, c_all), each (T, B, H).  With rounding=False it is the oracle.lstm_cell loop.
    mutate (tests only): {"h": f(t, h_{t-1}) -> what step t multiplies, "c": f(t, c_{t-1}) -> what step t carries}."""
    rf, rb = _sites(rounding)
    m = mutate or {}
    T, B, H4 = gx.shape
    H = H4 // 4
    h = h0 if h0 is not None else gx.new_zeros(B, H)
    c = c0 if c0 is not None else gx.new_zeros(B, H)
    Wr = rf(W).t()
    hs, cs = [], []
    for t in range(T):
        hin = m["h"](t, h) if "h" in m else h
        cin = m["c"](t, c) if "c" in m else c
        pre = gx[t] + rb(rf(hin) @ Wr)
        i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
        g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        c = f * cin + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), torch.stack(cs)


def mfn_mem_scan(apre, chat, Wm, W2, b2, drop=None, rounding=True, mutate=None):
    """Same arguments as functional.mfn_mem_scan, the dropout given as its multiplier: apre (T, B, 2HG) = the batched part of both gamma
    fc1 layers, chat (T, B, MD), Wm (2HG, MD), W2 (2, MD, HG), b2 (2, MD), drop (T, B, 2HG) or None -> mem_all (T, B, MD).  With
    rounding=False it is the plain memory recurrence (test_gpu_models._oracle_mem_scan).
    mutate (tests only): {"u": f(t, relu(pre), drop_t) -> u, "z": f(t, g, product, b2_g) -> z_g}."""
    rf, rb = _sites(rounding)
    m = mutate or {}
    T, B, U = apre.shape
    HG = W2.shape[-1]
    mem = apre.new_zeros(B, chat.shape[-1])
    Wmr, W2r = rf(Wm).t(), [rf(W2[g]).t() for g in range(2)]
    out = []
    for t in range(T):
        r = torch.relu(apre[t] + rb(rf(mem) @ Wmr))
        dt = None if drop is None else drop[t]
        if "u" in m:
            u = m["u"](t, r, dt)
        else:
            u = r if dt is None else r * dt
        ur = rf(u)
        z = []
        for g in range(2):
            prod = ur[:, g * HG:(g + 1) * HG] @ W2r[g]
            z.append(m["z"](t, g, prod, b2[g]) if "z" in m else rb(prod + b2[g]))
        mem = torch.sigmoid(z[0]) * mem + torch.sigmoid(z[1]) * chat[t]
        out.append(mem)
    return torch.stack(out)


def _cell(pre, c, H):
    i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
    g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], dim=1)


def lstm_stack_scan(gx0, P, bias, h0=None, c0=None, rounding=True, mutate=None):
    """Same arguments as functional.lstm_stack_scan: gx0 (T, B, 4H), P (L, 4H, 2H) = [x_a columns | x_b columns], bias (L-1, 4H), h0 / c0
    (L, B, H) or None (zeros); o_{-1} = 0 -> (h_top (T, B, H), h_all, c_all (L, T, B, H)).  With rounding=False it is
    lstm_stack_ref.forward / backward.
    mutate (tests only): {"xa": f(t, l, x_a) and "xb": f(t, l, x_b) -> what layer-step (t, l) multiplies, "c": f(t, l, c) -> what it
    carries, "bias": f(l, bias_{l-1}) -> the bias of layer l >= 1, "pre": f(t, l, product, bias_{l-1}) -> the gate pre-activations of a
    layer >= 1 (in place of round_bwd(product + bias))}."""
    rf, rb = _sites(rounding)
    m = mutate or {}
    T, B, H4 = gx0.shape
    H, L = H4 // 4, P.shape[0]
    h = [h0[l] if h0 is not None else gx0.new_zeros(B, H) for l in range(L)]
    c = [c0[l] if c0 is not None else gx0.new_zeros(B, H) for l in range(L)]
    Pr = [rf(P[l]).t() for l in range(L)]
    bs = [None] + [m["bias"](l, bias[l - 1]) if "bias" in m else bias[l - 1] for l in range(1, L)]
    o = gx0.new_zeros(B, H)                                     # the zeros tile
    hs, cs = [[] for _ in range(L)], [[] for _ in range(L)]
    for t in range(T):
        for l in range(L):
            xa, xb = (o if l == 0 else h[l - 1]), h[l]
            if "xa" in m:
                xa = m["xa"](t, l, xa)
            if "xb" in m:
                xb = m["xb"](t, l, xb)
            cin = m["c"](t, l, c[l]) if "c" in m else c[l]
            prod = rf(torch.cat([xa, xb], dim=1)) @ Pr[l]
            if l == 0:
                pre = gx0[t] + rb(prod)
            else:
                pre = m["pre"](t, l, prod, bs[l]) if "pre" in m else rb(prod + bs[l])
            h[l], c[l], _ = _cell(pre, cin, H)
            hs[l].append(h[l])
            cs[l].append(c[l])
        o = h[L - 1]
    h_all = torch.stack([torch.stack(x) for x in hs])
    return h_all[L - 1], h_all, torch.stack([torch.stack(x) for x in cs])


class _FbGates(torch.autograd.Function):
    """p w_p + hr Wr^T on the rounded hr = bf16(h_{t-1}), Wr = bf16(W_hh).  Backward: ONE rounding of dG serves dh = bf16(dG) Wr,
    dW_hh = bf16(dG)^T hr and dw_p = bf16(dG)^T bf16(p) (functional._wgrad on [h_prev | p_prev]); dp = dG . w_p from the fp32 dG."""
    @staticmethod
    def forward(ctx, p, w_p, hr, Wr):
        ctx.save_for_backward(p, w_p, hr, Wr)
        return p.unsqueeze(1) * w_p.unsqueeze(0) + hr @ Wr.t()

    @staticmethod
    def backward(ctx, g):
        p, w_p, hr, Wr = ctx.saved_tensors
        gb = bf16(g)
        return g @ w_p, gb.t() @ bf16(p), gb @ Wr, gb.t() @ hr


class _FbReadout(torch.autograd.Function):
    """p = u . w2 + b2.  Backward: du = dp w2 from the fp32 dp; dw2 = bf16(dp)^T bf16(u), db2 = sum(bf16(dp)) (functional._wgrad)."""
    @staticmethod
    def forward(ctx, u, w2, b2):
        ctx.save_for_backward(u, w2)
        return u @ w2 + b2

    @staticmethod
    def backward(ctx, g):
        u, w2 = ctx.saved_tensors
        gb = bf16(g)
        return g.unsqueeze(1) * w2.unsqueeze(0), gb @ bf16(u), gb.sum().reshape(1)


def fb_readout(u, w2, b2, rounding=True):
    """p (B,) = u . w2 + b2 of lstm_fb_scan, with the kernels' backward roundings"""
    return _FbReadout.apply(u, w2, b2) if rounding else u @ w2 + b2


def lstm_fb_scan(gxc, w_p, W_hh, W1, b1, w2, b2, h0=None, c0=None, p_init=0.0, rounding=True, mutate=None, saved=None):
    """Same arguments as functional.lstm_fb_scan: gxc (T, B, 4H), w_p (4H), W_hh (4H, H), W1 (E, H), b1 (E), w2 (E), b2 (1), h0 / c0
    (B, H) or None (zeros), p_init a float -> (p_all (T, B), h_all, c_all (T, B, H), u_all (T, B, E)).  With rounding=False it is
    lstm_fb_ref.forward / backward.  The gate product of step t + 1 and the read-out of step t read ONE bf16 h tile.
    mutate (tests only): {"h": f(t, h_{t-1}) -> what step t's gate product multiplies, "p": f(t, p_{t-1}) -> what it feeds back,
    "c": f(t, c_{t-1}) -> what it carries, "u": f(t, u_t) -> what the read-out sums, "mask": f(t, [z_t > 0]) -> the read-out ReLU's
    mask in the BACKWARD (a 0 / 1 tensor), "readout": f(t, u, w2, b2) -> p_t}.
    saved (tests only): a dict that receives "acts" (T, B, 4H: the gate activations the forward kernel saves) and "grads", a function
    to call after backward() -> {"dG" (T, B, 4H), "du" (T, B, E), "dp" (T, B)}: the unrounded tensors the backward kernel stores."""
    rf, rb = _sites(rounding)
    m = mutate or {}
    T, B, H4 = gxc.shape
    H = H4 // 4
    w_p, w2, b2 = w_p.reshape(-1), w2.reshape(-1), b2.reshape(-1)
    h = h0 if h0 is not None else gxc.new_zeros(B, H)
    c = c0 if c0 is not None else gxc.new_zeros(B, H)
    p = gxc.new_full((B,), float(p_init))
    Wr, W1r = rf(W_hh), rf(W1).t()
    hr = rf(h)
    ps, hs, cs, us, acts, keep = [], [], [], [], [], {"dG": [], "du": [], "dp": []}
    for t in range(T):
        hin = rf(m["h"](t, h)) if "h" in m else hr
        pin = m["p"](t, p) if "p" in m else p
        cin = m["c"](t, c) if "c" in m else c
        if rounding:
            pre = gxc[t] + _FbGates.apply(pin, w_p, hin, Wr)
        else:
            pre = gxc[t] + pin.unsqueeze(1) * w_p.unsqueeze(0) + hin @ Wr.t()
        h, c, a = _cell(pre, cin, H)
        hr = rf(h)
        z = rb(hr @ W1r + b1)
        u = torch.relu(z)
        if "mask" in m:
            zb = z * m["mask"](t, (z > 0).to(z.dtype).detach())
            u = zb + (u - zb).detach()
        useen = m["u"](t, u) if "u" in m else u
        p = m["readout"](t, useen, w2, b2) if "readout" in m else fb_readout(useen, w2, b2, rounding)
        if saved is not None:
            for k, v in (("dG", pre), ("du", z), ("dp", p)):
                v.retain_grad()
                keep[k].append(v)
        ps.append(p)
        hs.append(h)
        cs.append(c)
        us.append(u)
        acts.append(a)
    if saved is not None:
        saved["acts"] = torch.stack(acts).detach()
        saved["grads"] = lambda: {k: torch.stack([x.grad for x in v]) for k, v in keep.items()}
    return torch.stack(ps), torch.stack(hs), torch.stack(cs), torch.stack(us)


# ------------------------------------------------------------------------------------------------ window encoder
def conv_plan(N, W, D, F):
    """What mmt_convpool_forward / _backward launch for (N, W, D, F): a mirror of carve_conv at K = 2, ktap = false, and of the forward's
    channel dispatch (csrc/api.hip).  nsplit window splits of `wins` windows (the last one `last` windows), npairs window pairs in the fullest split,
    nrt row tiles per window, one_rt the backward instance, fwd the forward launches as (CT, channel blocks, c_first)."""
    up = lambda a, m: -(-a // m) * m  # noqa: E731
    FPAD, DPB = up(F, 256), up(D, 128)
    blocks = (DPB // 128) * (FPAD // 256)
    ns = max(1, min(-(-512 // blocks), (N + 1) // 2))
    wins = up(-(-N // ns), 2)
    nsplit = -(-N // wins)
    last = N - (nsplit - 1) * wins
    nmain, rem = F // 256, F % 256
    fwd = [(4, nmain, 0)] if nmain else []
    if rem > 128:
        fwd.append((4, 1, nmain * 256))
    elif rem > 64:
        fwd.append((2, 1, nmain * 256))
    elif rem > 0:
        fwd.append((1, 1, nmain * 256))
    return {"nsplit": nsplit, "wins": wins, "last": last, "npairs": (min(wins, N) + 1) // 2, "nrt": -(-(W - 1) // 32), "one_rt": W <= 33,
            "fwd": fwd, "fwd_wgs": -(-N // 8)}


class _MapBwd(torch.autograd.Function):
    """identity in the forward, fn(gradient) in the backward"""
    @staticmethod
    def forward(ctx, t, fn):
        ctx.fn = fn
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


def _exact_bf16(t):
    """bf16 of an INPUT (no jitter: the rounding of given fp32 data is the same in every implementation)"""
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return _exact_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


def conv_sums(x, w, rounding=True):
    """S (N, W-1, F) without the bias, and per (n, p, f) the sum of |terms| (for the fp32 dot-product bound), no autograd"""
    with torch.no_grad():
        xr, wr = (_exact_bf16(x), _exact_bf16(w)) if rounding else (x, w)
        S = xr[:, :-1] @ wr[:, :, 0].t() + xr[:, 1:] @ wr[:, :, 1].t()
        A = xr[:, :-1].abs() @ wr[:, :, 0].abs().t() + xr[:, 1:].abs() @ wr[:, :, 1].abs().t()
    return S, A


def conv_maxpool(x, w, b, arg=None, rounding=True, mutate=None):
    """Same arguments as functional.conv_maxpool (x (N, W, D), w (F, D, 2), b (F,)) -> (out (N, F), arg (N, F), S (N, W-1, F) without
    the bias).  arg given: the pool gathers at those positions, so autograd yields the exact gradient for that choice (the kernel's own).
    With rounding=False: oracle.cnn_maxpool.  Under ``jitter`` the operands are NOT perturbed (x and w are inputs: their bf16 values are
    the same in every implementation); the sums are, by eps * sqrt(2D) * sqrt(sum of the squared terms) (normal): the random-walk size
    of an fp32 accumulation of 2D terms, 3-4x what an fp32 matmul in another order shows against fp64 on the CPU.
    mutate (tests only): {"tap": f(j, rows (N, W-1, D), w_j (F, D)) -> the tap's product, "S": f(S, xr, wr) -> S (may add positions),
    "pool": f(S) -> arg, "gathered": f(pooled sums) -> the same, "b": f(b) -> b, "round_dy": f(dy) -> the backward's dy operand}."""
    m = mutate or {}
    rin = _RoundInput.apply if rounding else (lambda t: t)
    xr, wr = rin(x), rin(w)
    S = 0
    for j in range(2):
        rows, wj = xr[:, j:j + x.shape[1] - 1], wr[:, :, j]
        S = S + (m["tap"](j, rows, wj) if "tap" in m else rows @ wj.t())
    if "S" in m:
        S = m["S"](S, xr, wr)
    if _JITTER is not None:
        g, eps = _JITTER
        with torch.no_grad():
            sq = (xr[:, :-1] ** 2) @ (wr[:, :, 0] ** 2).t() + (xr[:, 1:] ** 2) @ (wr[:, :, 1] ** 2).t()
            noise = eps * math.sqrt(2 * x.shape[2]) * sq.sqrt() * torch.randn(sq.shape, generator=g, dtype=sq.dtype)
        S = S + noise
    if arg is None:
        arg = m["pool"](S.detach()) if "pool" in m else S.detach().argmax(dim=1)      # argmax: the first position of the maximum
    pooled = S.gather(1, arg.long().unsqueeze(1)).squeeze(1)
    if "gathered" in m:
        pooled = m["gathered"](pooled)
    if rounding:
        pooled = _MapBwd.apply(pooled, m["round_dy"]) if "round_dy" in m else round_bwd(pooled)      # dW from bf16(dy), db from dy
    out = pooled + (m["b"](b) if "b" in m else b)
    return out, arg, S.detach()


def highway(x, Wp, bp, Wg, bg, drop=None, proj_act=0, rounding=True, mutate=None):
    """Same arguments as functional.highway, the dropout given as its multiplier (shaped like x): drop * (x + gate * (proj - x)),
    proj = act(x Wp^T + bp) (proj_act 0, or 1: the B1 variant's ReLU), gate = sigmoid(x Wg^T + bg).  With rounding=False: oracle.highway.
    mutate (tests only): {"combine": f(x, proj, gate) -> the combine before the dropout, "gate_act": f(pre) -> gate}."""
    m = mutate or {}
    proj = linear(x, Wp, bp, act=proj_act, rounding=rounding)
    gate = linear(x, Wg, bg, act=3, rounding=rounding, mutate={"act": m["gate_act"]} if "gate_act" in m else None)
    y = m["combine"](x, proj, gate) if "combine" in m else x + gate * (proj - x)
    return y if drop is None else y * drop


def linear_pair(x, W1, b1, W2, b2, act1=0, act2=0, rounding=True):
    """Same arguments as functional.linear_pair: two affine maps of one input; autograd sums the two fp32 gradients into x."""
    return linear(x, W1, b1, act=act1, rounding=rounding), linear(x, W2, b2, act=act2, rounding=rounding)


def window_encoder(p, mod, x, drop=None, arg=None, proj_act=0, rounding=True):
    """Same arguments as oracle.window_encoder (p: {state_dict name: tensor}, x (B, T, W, D), drop (B*T, F) or None) -> ((B, T, F), arg):
    conv + pool, Highway, dropout multiplier, as models._FrontEnd._encode chains them for one modality.  The Highway's fp32 dx is the
    conv's dy."""
    B, T, W, D = x.shape
    e, arg, _ = conv_maxpool(x.reshape(B * T, W, D), p["cnn_%s.conv1d.weight" % mod], p["cnn_%s.conv1d.bias" % mod], arg, rounding)
    h = "highway_%s." % mod
    y = highway(e, p[h + "linear_projection.weight"], p[h + "linear_projection.bias"], p[h + "linear_gate.weight"],
                p[h + "linear_gate.bias"], drop, proj_act, rounding)
    return y.reshape(B, T, -1), arg
