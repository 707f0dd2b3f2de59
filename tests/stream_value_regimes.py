"""Deterministic inputs that put the STREAM kernels and the band's lower edge into the value regimes of tests/value_regimes.py (TEST
INFRASTRUCTURE, a plain helper module, no GPU).

tests/test_stream_value_regimes_cpu.py asserts on the references alone that every regime is reached at every shape used on the GPU and
holds the yardsticks of the widened bounds; tests/test_gpu_stream_value_regimes.py runs the kernels on the same bits.

Part A, encoder streams (csrc/encoder_step.h, encoder_extend.h, step_ring.h, step_prefill.h).  A stream takes x and parameters, not
q / k / v, so a regime is built into layer 0 of the recipe's stack (seed 17); u is the first feature of every head, a = sqrt(d_k) / 4:
  peaked     W_q and b_q x 12;
  cold, hot  b_q[u] += COLD_C a, b_k[u] -+= COLD_C a (in every layer: the shifts do not depend on the input);
  positional regimes: feature 0 of x is a position channel, x[b, j, 0] = c_j exactly.  Row u of W_k is zero except column 0 (= w),
             b_k[u] = 0, b_q[u] += Q_SHIFT a, so K_j . u = w bf16(LN1(x_j))[0].  The other d - 1 features are unit normal draws that
             are centred and scaled to unit mean square PER ROW: LayerNorm's mean and deviation of a row then depend on c_j alone, and
             bf16(LN1(x_j))[0] is one monotone function of c_j for every window and sequence (with raw draws the row mean alone moves
             it by +-0.16 at d = 40, more than two neighbouring positions of a ramp differ).
    newest     c_j rises with j: every row's maximum is key t, the one kept in LDS; older keys underflow to P = 0;
    oldest     c_j falls with j: the maximum is the oldest visible key, in a ring the row that the next step evicts;
    step_up    c_j = POS_C for j >= J0: an extend tile that holds J0 has hot keys above the diagonal of its rows before J0;
    step_down  c_j = POS_C for j < J0 (20 at span 33, where T = 70 has no query behind 40 + 32): in a ring of span s the queries
               t >= J0 + s - 1 see none of them;
    flat       c_j = 0 with the parameters of one of the above: what the bit-for-bit facts compare with.
  w is chosen per case (pos_w) so that test_stream_value_regimes_cpu.py's assertions hold on the reference's own layer-0 scores: the
  recipe's W_q, W_k carry a gain of 3, so the other d_k - 1 features move a score by +-4.3 (sigma), and two neighbouring keys of a ramp
  must differ by more than the worst such pair.

Part C, the recurrent step kernels (csrc/lstm_step.h with its feedback tails, decoder_step.h, mfn_step.h): the regimes go into the
parameters that the families' own stream tests draw (lstm_stream_ref.params, decoder_stream_ref.params, lstm_feedback_stream_ref's
ed_params / ar_params, the recipe's parameters of an MFN):
  overflow     +-SAT on the summed gate bias of every LSTM layer or cell at value_regimes.saturate's stride (MFN: on the biases of
               gamma1_fc2 / gamma2_fc2), T = 9;
  long_memory  forget-gate bias + FORGET_SHIFT (MFN: also gamma1_fc2's bias, which retains the memory), T = 130, a hole in one mask;
  peaked       attn.2.weight x 60 (MFN: att1_fc2.weight x 60), T = 9: the steps whose taps reach before position 0 included.

Part B, the band's lower edge in the batch attention (csrc/attn.h, *_band_kernel): value_regimes.attention()'s inputs plus
  step_down  q + Q_SHIFT a u, k_j + STEP_S a u for j < j0: keys OLDER than the band beat every visible key of the late queries.
"""
import math

import torch

import band_ref as Bn
import bf16_ref as E
import prefill_ref as PF
import recipe as R
import ring_stream_ref as RS
import stream_ref as S
import value_regimes as V

SEED = V.SEED
PEAK = 12.0                    # peaked: layer 0's W_q and b_q
POS_C = 2.5                    # the position channel's range: LayerNorm compresses it by a few percent below 3
J0 = 40
ENC_B = 2
ENC_SHAPES = ((40, 4), (128, 8), (256, 4))                      # d_k = 10 padded, 16, 64
SPANS = (5, 16, 33)
GROUPS = {70: [7, 16, 30, 17], 130: [5, 64, 61]}               # tests/test_gpu_stream_extend.py's groupings
POSITIONAL = ("newest", "oldest", "step_up", "step_down")
PREFILL = 10                                                    # prefill(10), extend [16, 30], then steps
PREFILL_GROUPS = [16, 30]
SUBNORMAL = -133.0                                              # log2 of the smallest bf16 subnormal


# ------------------------------------------------------------------------------------------------ part A: cases
def enc_cases():
    """(kind, regime, d, h, N, T, span): kind "plain" (span None) or "ring"; each case is stepped and extended"""
    out = []
    for d, h in ENC_SHAPES:
        out += [("plain", r, d, h, 1, 70, None) for r in ("peaked", "cold", "hot", "newest", "oldest", "step_up")]
        for span in SPANS:
            out += [("ring", r, d, h, 1, 70, span) for r in ("cold", "hot", "newest", "oldest", "step_down")]
        out += [("ring", "peaked", d, h, 1, 70, 16), ("ring", "step_up", d, h, 1, 70, 16)]
    out += [("plain", r, 128, 8, 1, 130, None) for r in ("newest", "oldest")]      # key counts cross 64 and 128
    out += [("ring", r, 128, 8, 1, 130, 33) for r in ("newest", "oldest")]
    out.append(("plain", "cold", 128, 8, 2, 70, None))                                # the shifts in both layers
    return out


def enc_id(case):
    kind, regime, d, h, n, T, span = case
    return "%s_%s_d%d_n%d_T%d%s" % (kind, regime, d, n, T, "" if span is None else "_s%d" % span)


PREFILL_CASES = [("plain", "cold", 128, 8, 1, 70, None), ("plain", "step_up", 128, 8, 1, 70, None)]
# one slots run per kernel body (step, ring step, extend, ring extend), each asserted equal in bits to the host form
SLOT_CASES = [("plain", "step_up", 128, 8, 1, 70, None), ("ring", "step_down", 128, 8, 1, 70, 16)]


def j0_of(case):
    """J0, but 20 for step_down in a ring of span 33: at T = 70 no query lies behind 40 + 33 - 1"""
    return 20 if (case[1], case[6]) == ("step_down", 33) else J0


def has_flat(case):
    return case[1] in ("step_up", "step_down")


def pos_w(case):
    """column 0 of W_k's row u.  One position of a ramp moves bf16(LN1(x))[0] by ~4.5 / T and a score by 10.8 w times that; the worst
    pair of neighbouring keys differs by ~27 through the other features, and half of a ring's span must fall below 2^-133."""
    kind, regime, d, h, n, T, span = case
    if regime in ("step_up", "step_down"):
        return 16.0
    if span == 5:
        return 256.0
    return 96.0 if T == 70 else 192.0


def enc_lengths(T):
    return V.attn_lengths(T)


def enc_mask(T):
    return R.prefix_mask(enc_lengths(T), T)


def enc_params(case):
    """the recipe's parameters (seed 17) with the regime built into layer 0 (cold / hot: into every layer) -> fp32 OrderedDict"""
    kind, regime, d, h, n, T, span = case
    p = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    dk = d // h
    a = math.sqrt(dk) / 4.0
    u = torch.arange(0, d, dk)
    for i in range(n if regime in ("cold", "hot") else 1):
        L = "layers.%d.self_attn.linears." % i
        Wq, bq, Wk, bk = L + "0.weight", L + "0.bias", L + "1.weight", L + "1.bias"
        for name in (Wq, bq, Wk, bk):
            p[name] = p[name].clone()
        if regime == "peaked":
            p[Wq] *= PEAK
            p[bq] *= PEAK
        elif regime in ("cold", "hot"):
            p[bq][u] += V.COLD_C * a
            p[bk][u] += (-1.0 if regime == "cold" else 1.0) * V.COLD_C * a
        else:
            assert regime in POSITIONAL
            p[Wk][u] = 0.0
            p[Wk][u, 0] = pos_w(case)
            p[bk][u] = 0.0
            p[bq][u] += V.Q_SHIFT * a
    return p


def pos_profile(regime, T, j0=J0):
    j = torch.arange(T, dtype=torch.float32)
    if regime == "newest":
        return -POS_C + 2.0 * POS_C * j / (T - 1)
    if regime == "oldest":
        return POS_C - 2.0 * POS_C * j / (T - 1)
    if regime == "step_up":
        return POS_C * (j >= j0).float()
    if regime == "step_down":
        return POS_C * (j < j0).float()
    assert regime == "flat"
    return torch.zeros(T)


def enc_x(case, flat=False):
    """x (B, T, d) fp32; the same draws for every regime of a (d, T); flat: the positional case's input with c_j = 0"""
    kind, regime, d, h, n, T, span = case
    x = R.gen_normal("svr:enc:%d:%d:x" % (d, T), (ENC_B, T, d), SEED)
    if regime not in POSITIONAL:
        assert not flat
        return x
    o = x[..., 1:]
    o = o - o.mean(dim=-1, keepdim=True)
    o = o / o.pow(2).mean(dim=-1, keepdim=True).sqrt()
    c = pos_profile("flat" if flat else regime, T, j0_of(case)).reshape(1, T, 1).expand(ENC_B, T, 1)
    return torch.cat([c, o], dim=-1).contiguous()


# ------------------------------------------------------------------------------------------------ part A: references
class _Rec:
    """records Q' and K of every layer and step as the stream reference forms them (stream_ref.EncoderStream._attend's own lines)"""

    def reset(self):
        super().reset()
        self.rec = [[] for _ in range(self.n)]

    def _attend(self, layer, q, k, v, keep):
        rf = E.bf16 if self.rounding else (lambda z: z)
        Qs = q * (E.LOG2E / math.sqrt(q.shape[1] // self.h))
        if keep is not None:
            Qs = Qs * keep.reshape(-1, 1)
        self.rec[layer].append((rf(Qs), rf(k)))
        return super()._attend(layer, q, k, v, keep)


class _PlainRec(_Rec, S.EncoderStream):
    pass


class _RingRec(_Rec, RS.EncoderStream):
    pass


def _walk(case, flat, dtype):
    kind, regime, d, h, n, T, span = case
    p = {k: v.to(dtype) for k, v in enc_params(case).items()}
    x, mask = enc_x(case, flat).to(dtype), enc_mask(T).to(dtype)
    s = _PlainRec(p, "", h) if span is None else _RingRec(p, "", h, span)
    y = torch.stack([s.step(x[:, t], mask[:, t].reshape(-1)) for t in range(T)], dim=1)
    return y, s


def enc_reference(case, flat=False, dtype=torch.float64):
    """stream_ref.encoder_stack / ring_stream_ref.encoder_stack of the case -> (B, T, d) float64 numpy"""
    return _walk(case, flat, dtype)[0].double().numpy()


def enc_scores(case):
    """-> y (B, T, d) and, per layer, the reference's own log2 scores S' (B, h, T, T) = Q'_t . K_j of EVERY pair, visible or not"""
    kind, regime, d, h, n, T, span = case
    y, s = _walk(case, False, torch.float64)
    out = []
    for layer in range(s.n):
        Qp = V.split_heads(torch.stack([q for q, _ in s.rec[layer]], dim=1), h)
        K = V.split_heads(torch.stack([k for _, k in s.rec[layer]], dim=1), h)
        out.append(Qp @ K.transpose(-2, -1))
    return y.numpy(), out


def enc_visible(case):
    """(T, T) bool: the keys query t attends"""
    kind, regime, d, h, n, T, span = case
    return ~Bn.outside_band(T, T if span is None else span)


def valid_rows(T):
    """(B, T) bool: query rows that are not blanked"""
    return enc_mask(T).reshape(ENC_B, T) != 0


def prefill_reference(case, dtype=torch.float64):
    """prefill_ref.encoder_rows: rows < PREFILL from the batch reference, the later ones stepped from its cache"""
    kind, regime, d, h, n, T, span = case
    p = {k: v.to(dtype) for k, v in enc_params(case).items()}
    with torch.no_grad():
        return PF.encoder_rows(p, "", h, enc_x(case).to(dtype), enc_mask(T).to(dtype), [PREFILL] * ENC_B, PREFILL, span).double().numpy()


def enc_family(case):
    """the key of a case's yardstick: (kind, regime family, d)"""
    fam = {"cold": "cold_hot", "hot": "cold_hot", "newest": "ramp", "oldest": "ramp", "step_up": "step", "step_down": "step",
           "peaked": "peaked"}[case[1]]
    return (case[0], fam, case[2])


# ------------------------------------------------------------------------------------------------ part B: the band's lower edge
BAND_H, BAND_B = V.ATTN_H, V.ATTN_B
BAND_DK = V.ATTN_DK
BAND_STEPS = ((70, 5, 40), (70, 33, 20), (290, 40, 200), (290, 64, 200))      # (T, span, j0)
BAND_SWEEPS = ((290, 100), (290, 200))
BAND_SMALL = ((70, 33), (290, 40))
P_TRAIN = 0.1


def band_cases():
    """(regime, T, span, d_k, j0); each runs in eval mode and at p = 0.1"""
    out = []
    for dk in BAND_DK:
        out += [("step_down", T, span, dk, j0) for T, span, j0 in BAND_STEPS]
        out += [(r, T, span, dk, None) for T, span in BAND_SWEEPS for r in ("falling", "rising")]
        out += [("peaked", T, span, dk, None) for T, span in BAND_SMALL]
    out += [("cold", T, span, 64, None) for T, span in BAND_SMALL]             # d_k = 16: tests/test_gpu_band.py has it
    return out


def band_probs_cases():
    return [(r, 70, 33, dk, 20 if r == "step_down" else None) for dk in BAND_DK for r in ("step_down", "cold", "peaked")]


def band_id(case):
    regime, T, span, dk, j0 = case
    return "%s%s_T%d_s%d_dk%d" % (regime, "" if j0 is None else str(j0), T, span, dk)


def band_family(case):
    return ({"step_down": "step", "falling": "sweep", "rising": "sweep", "peaked": "peaked", "cold": "cold"}[case[0]], case[3])


def band_inputs(case):
    """-> q, k, v, g (B, T, d) fp32 and the query-row mask (B, T, 1)"""
    regime, T, span, dk, j0 = case
    d = BAND_H * dk
    if regime == "step_down":
        q, k, v, g = V.attention("step", BAND_B, T, d, BAND_H, j0)              # the draws; its own step is taken back out
        a = math.sqrt(dk) / 4.0
        u = torch.zeros(d)
        u[::dk] = 1.0
        j = torch.arange(T, dtype=torch.float32).reshape(1, T, 1)
        k = R.gen_normal("vr:attn:%d:%d:%dk" % (T, d, BAND_H), (BAND_B, T, d), V.SEED) + (j < j0).float() * V.STEP_S * a * u
        k = k.contiguous()
    else:
        q, k, v, g = V.attention(regime, BAND_B, T, d, BAND_H)
    return q, k, v, g, R.prefix_mask(V.attn_lengths(T), T)


def band_reference(case, drop=None, dtype=torch.float64):
    """{y, dq, dk, dv} of band_ref.sdpa under autograd, evaluated in `dtype` -> float64 numpy"""
    regime, T, span, dk, j0 = case
    q, k, v, g, mask = band_inputs(case)
    lt = [t.to(dtype).requires_grad_() for t in (q, k, v)]
    ctx, _ = Bn.sdpa(*(V.split_heads(t, BAND_H) for t in lt), span, mask.to(dtype).unsqueeze(1), None if drop is None else drop.to(dtype))
    y = ctx.permute(0, 2, 1, 3).reshape(BAND_B, T, BAND_H * dk)
    y.backward(g.to(dtype))
    return {"y": y.detach().double().numpy(), "dq": lt[0].grad.double().numpy(), "dk": lt[1].grad.double().numpy(),
            "dv": lt[2].grad.double().numpy()}


def band_scores(case):
    """S' (B, h, T, T) of the bf16 operands, blanked query rows as Q' = 0"""
    q, k, v, g, mask = band_inputs(case)
    return V.log2_scores(q * mask, k, BAND_H)


def band_probs_reference(case):
    """value_regimes.probs_reference's fp64 softmax with the band's visibility -> (B, h, T, T), exact zeros outside the band"""
    regime, T, span, dk, j0 = case
    S_ = band_scores(case).masked_fill(Bn.outside_band(T, span), float("-inf"))
    return torch.softmax(S_ * E.LN2, dim=-1)


def band_sweep(S_, T, span):
    """the rescale decisions of band_ref._forward_value's downward sweep on scores S_ (B, h, T, T): (B, h, query tile, key tile) bool
    (True where the running maximum moved at that key tile), and the set of swept (query tile, key tile) pairs"""
    B, h = S_.shape[:2]
    nt = -(-T // 32)
    sp = min(span, T)
    Sp = torch.zeros(B, h, nt * 32, T, dtype=S_.dtype)
    Sp[:, :, :T] = S_
    Sp = Sp.masked_fill(Bn.outside_band(T, sp, nt * 32), float("-inf"))
    moves = torch.zeros(B, h, nt, nt, dtype=torch.bool)
    swept = []
    for qt in range(nt):
        Sq = Sp[:, :, 32 * qt: 32 * qt + 32]
        m = None
        for kt in range(qt, Bn.band_lo_tile(qt, sp) - 1, -1):
            tmax = Sq[..., 32 * kt: min(T, 32 * kt + 32)].amax(dim=-1)
            if kt == qt:
                m = tmax
                continue
            swept.append((qt, kt))
            rel = tmax - m
            mv = (rel > E.RESCALE_THR).any(dim=-1)
            m = torch.where(mv.unsqueeze(-1), m + rel.clamp(min=0.0), m)
            moves[:, :, qt, kt] = mv
    return moves, swept


def synthetic_drop(case, s=0):
    """a p = 0.1 mask from torch's CPU generator (the kernels' own bits need a GPU): the train-mode roundings of the reference"""
    regime, T, span, dk, j0 = case
    g = torch.Generator().manual_seed(4321 + T + dk + span + 1000 * s)
    return (torch.rand(BAND_B, BAND_H, T, T, generator=g) >= P_TRAIN).double() / (1.0 - P_TRAIN)


def worst(figs):
    """the element-wise maximum of (rel-L2, per-row maximum) pairs"""
    figs = list(figs)
    return tuple(max(f[i] for f in figs) for i in range(2))


# ------------------------------------------------------------------------------------------------ part C: the recurrent steps
REC_B = 2
REC_T = {"overflow": V.OVERFLOW_T, "long_memory": 130, "peaked": 9}
TAP_PEAK = 60.0
SAT_STRIDE = 7                                                  # value_regimes.saturate's
MFN_MODS, MFN_WIDTHS = ["acoustic", "emotient"], [12, 16]      # tests/test_gpu_mfn_stream.py's two-modality case
# (family, shape): lstm (in, E, H, layers, taps); dec (d, h_dim, layers); ed (in, E, H, 1, taps); ar (in, E, H, layers, taps, K)
REC_SHAPES = [("lstm", (12, 12, 20, 1, 3)), ("lstm", (16, 8, 8, 2, 3)), ("dec", (40, 128, 1)), ("dec", (128, 128, 2)),
              ("ed", (12, 12, 20, 1, 3)), ("ar", (12, 12, 20, 1, 3, 3)), ("mfn", ())]


def rec_cases():
    """(family, shape, regime); the decoder has no softmax to peak"""
    return [(f, sh, r) for f, sh in REC_SHAPES for r in ("overflow", "long_memory", "peaked") if not (f == "dec" and r == "peaked")]


def sat_count(case):
    """how many gate pre-activations of the whole walk carry +-SAT: per LSTM layer or cell (4H rows; the ED tail's decoder cell is one
    more) or per gamma (MEM_DIM rows), times B and T"""
    fam, sh, regime = case
    n = lambda rows: int(sum(m.sum() for m in sat_rows(rows)))      # noqa: E731
    per_step = {"lstm": lambda: sh[3] * n(4 * sh[2]), "dec": lambda: sh[2] * n(4 * sh[0]), "ed": lambda: 2 * n(4 * sh[2]),
                "ar": lambda: sh[3] * n(4 * sh[2]), "mfn": lambda: 2 * n(128)}[fam]()
    return per_step * REC_B * REC_T[regime]


def rec_id(case):
    fam, sh, regime = case
    return "%s%s_%s" % (fam, "".join("_%d" % n for n in sh), regime)


def sat_rows(n):
    """the rows of a length-n bias that take +SAT and -SAT"""
    idx = torch.arange(n)
    return idx % SAT_STRIDE == 0, idx % SAT_STRIDE == 3


def _saturate_bias(b):
    hi, lo = sat_rows(b.numel())
    b = b.clone()
    b.reshape(-1)[hi] += V.SAT
    b.reshape(-1)[lo] -= V.SAT
    return b


def _open_forget(b):
    H = b.numel() // 4                                          # gate order i, f, g, o
    b = b.clone()
    b[H:2 * H] += V.FORGET_SHIFT
    return b


def rec_params(case):
    """-> {name: fp64 tensor} under the family's own names (MFN: MFN's state_dict names), the regime applied"""
    fam, sh, regime = case
    tag = "svr:%s" % fam
    if fam == "lstm":
        import lstm_stream_ref as LS
        p = LS.params(*sh, tag=tag)
    elif fam == "dec":
        import decoder_stream_ref as DS
        p = DS.params(*sh, tag=tag)
    elif fam == "ed":
        import lstm_feedback_stream_ref as FR
        p = FR.ed_params(sh[0], sh[1], sh[2], sh[4], tag=tag)
    elif fam == "ar":
        import lstm_feedback_stream_ref as FR
        p = FR.ar_params(*sh, tag=tag)
    else:
        p = {k: v.double() for k, v in R.gen_params(mfn_shapes(), 11).items()}
    bias_ih = [k for k in p if ".bias_ih" in k]                  # one per LSTM layer or cell, the ED tail's decoder cell included
    assert bias_ih
    if regime == "overflow":
        for k in (["gamma1_fc2.bias", "gamma2_fc2.bias"] if fam == "mfn" else bias_ih):
            p[k] = _saturate_bias(p[k])
    elif regime == "long_memory":
        for k in bias_ih:
            p[k] = _open_forget(p[k])
        if fam == "mfn":
            p["gamma1_fc2.bias"] = p["gamma1_fc2.bias"] + V.FORGET_SHIFT
    else:
        k = "att1_fc2.weight" if fam == "mfn" else "attn.2.weight"
        p[k] = p[k] * TAP_PEAK
    return p


def mfn_shapes():
    """the state_dict shapes of MFN(MFN_MODS, widths, 1), written out from the module's constructor (the GPU file asserts them against
    the module's own)"""
    from collections import OrderedDict
    from oracle.mfn_ref import HIDDEN, MEM_DIM
    s = OrderedDict()
    for m, w in zip(MFN_MODS, MFN_WIDTHS):
        H = HIDDEN[m]
        s["lstm_%s.weight_ih" % m], s["lstm_%s.weight_hh" % m] = (4 * H, w), (4 * H, H)
        s["lstm_%s.bias_ih" % m], s["lstm_%s.bias_hh" % m] = (4 * H,), (4 * H,)
    A = 2 * sum(HIDDEN[m] for m in MFN_MODS)
    for name, o, i in (("att1_fc1", 128, A), ("att1_fc2", A, 128), ("att2_fc1", 256, A), ("att2_fc2", MEM_DIM, 256),
                       ("gamma1_fc1", 64, A + MEM_DIM), ("gamma1_fc2", MEM_DIM, 64), ("gamma2_fc1", 64, A + MEM_DIM),
                       ("gamma2_fc2", MEM_DIM, 64), ("out_fc1", 64, A // 2 + MEM_DIM), ("out_fc2", 1, 64)):
        s[name + ".weight"], s[name + ".bias"] = (o, i), (o,)
    return s


def rec_inputs(case):
    """-> x (B, T, in) (MFN: {mod: (T, B, width)}) and mask (B, T), fp32.  long_memory: ones with a hole in sequence 0; else a prefix
    mask [T, 2T/3]"""
    fam, sh, regime = case
    T = REC_T[regime]
    if regime == "long_memory":
        mask = torch.ones(REC_B, T)
        mask[0, T // 2] = 0.0
    else:
        mask = R.prefix_mask([T, (2 * T) // 3], T).reshape(REC_B, T)
    if fam == "mfn":
        return {m: R.gen_normal("svr:mfn:%s:%d" % (m, T), (T, REC_B, w), 11) for m, w in zip(MFN_MODS, MFN_WIDTHS)}, mask
    return R.gen_normal("svr:%s:x:%d:%d" % (fam, sh[0], T), (REC_B, T, sh[0]), 11), mask


def rec_reference(case, dtype=torch.float64, x=None):
    """the family's stepped reference, rounding on -> (B, T, 1) (MFN: (B, T, output_dim)) float64 numpy.  x: other inputs"""
    fam, sh, regime = case
    p = {k: v.to(dtype) for k, v in rec_params(case).items()}
    xin, mask = rec_inputs(case)
    if x is not None:
        xin = x
    mask = mask.to(dtype)
    with torch.no_grad():
        if fam == "mfn":
            import mfn_stream_ref as MS
            y = MS.mfn_gate(p, "", {m: v.to(dtype) for m, v in xin.items()}, MFN_MODS, mask.unsqueeze(-1))
        elif fam == "lstm":
            import lstm_stream_ref as LS
            y = LS.stepped(p, xin.to(dtype), mask)
        elif fam == "dec":
            import decoder_stream_ref as DS
            y = DS.stepped(p, "", sh[2], xin.to(dtype), mask)
        else:
            import lstm_feedback_stream_ref as FR
            step = FR.EdStep if fam == "ed" else FR.ArStep
            y = FR.stepped(lambda: step(p, REC_B), xin.to(dtype), mask)
    return y.double().numpy()


def first_window_changed(case):
    """the inputs with window 0 of every sequence replaced by other draws"""
    fam, sh, regime = case
    x, _ = rec_inputs(case)
    if fam == "mfn":
        out = {m: v.clone() for m, v in x.items()}
        for m in out:
            out[m][0] = R.gen_normal("svr:mfn:other:%s" % m, tuple(out[m][0].shape), 11)
        return out
    out = x.clone()
    out[:, 0] = R.gen_normal("svr:%s:other" % fam, tuple(out[:, 0].shape), 11)
    return out


class capture:
    """records the arguments of torch.sigmoid / torch.tanh and the (logits, result) pairs of torch.softmax while a reference runs: what
    the gates of its cells were given, without a hook in any reference"""

    def __enter__(self):
        self.gates, self.softmax = [], []
        self._orig = (torch.sigmoid, torch.tanh, torch.softmax)
        sg, th, sm = self._orig

        def sigmoid(z):
            self.gates.append(("sigmoid", z.detach().clone()))
            return sg(z)

        def tanh(z):
            self.gates.append(("tanh", z.detach().clone()))
            return th(z)

        def softmax(z, *a, **kw):
            out = sm(z, *a, **kw)
            self.softmax.append((z.detach().clone(), out.detach().clone()))
            return out

        torch.sigmoid, torch.tanh, torch.softmax = sigmoid, tanh, softmax
        return self

    def __exit__(self, *a):
        torch.sigmoid, torch.tanh, torch.softmax = self._orig


def tap_logits(case):
    """z (B, T, taps) of the LSTM families' tap softmax, by lstm_stream_ref.LstmStep's own three affine maps"""
    fam, sh, regime = case
    p = rec_params(case)
    x, _ = rec_inputs(case)
    embed = E.linear(x.double(), p["embed.1.weight"], p["embed.1.bias"], act=1)
    hid = E.linear(embed, p["attn.0.weight"], p["attn.0.bias"], act=1)
    return E.linear(hid, p["attn.2.weight"], p["attn.2.bias"])
