"""The value regimes of tests/value_regimes.py, held on the references alone (no GPU): every regime is reached at every shape the GPU
tests use, and the reference stays finite there.  These are conditions on the inputs, not measurements of any kernel.

The second half holds the yardsticks behind every bound of tests/test_gpu_value_regimes.py that is wider than the bound the same tensor
has in its own tier.  A yardstick involves no kernel:
  * fp32: the same reference evaluated with float32 tensors against its fp64 result (what one fp32 evaluation order costs when scores
    of magnitude ~600 carry ~6e-5 absolute, or a row of mean 1000 is centred in fp32);
  * jitter: the reference against itself under bf16_ref.jitter(6e-8) (a tipped rounding that is carried instead of forgotten).
A bound is 4x its yardstick, the factor the other tiers use.  The recorded constants are checked here against a fresh evaluation: a
constant may understate its yardstick, never overstate it.
"""
import numpy as np
import pytest
import torch

import bf16_ref as E
import value_regimes as V
from gpu_harness import measures

CASES = V.sdpa_cases()
IDS = [V.case_id(c) for c in CASES]
LN2 = 0.6931471805599453


def _valid(T):
    """(B, 1, T) bool: query rows that are not blanked"""
    out = torch.zeros(V.ATTN_B, 1, T, dtype=torch.bool)
    for b, n in enumerate(V.attn_lengths(T)):
        out[b, :, :n] = True
    return out


def _scores(case):
    q, k, v, g, mask, kl = V.sdpa_inputs(case)
    return V.log2_scores(q, k, V.ATTN_H), V.visible(case)


def _row_L(case):
    """L = log2 sum 2^S' over the visible keys of every row, (B, h, T)"""
    S, vis = _scores(case)
    return torch.logsumexp(S.masked_fill(~vis, float("-inf")) * LN2, dim=-1) / LN2


def _of(regime):
    return [c for c in CASES if c[1] == regime]


def _ids(cs):
    return [V.case_id(c) for c in cs]


# ------------------------------------------------------------------------------------------------ attention regimes
@pytest.mark.parametrize("case", _of("peaked"), ids=_ids(_of("peaked")))
def test_peaked_rows_are_nearly_one_hot(case):
    T = case[2]
    top = V.probs_reference(case).amax(dim=-1)[_valid(T).expand(-1, V.ATTN_H, -1)]
    share = float((top > 0.99).double().mean())
    print("%s: %.0f %% of valid rows have a probability above 0.99" % (V.case_id(case), 100 * share))
    assert share >= 0.2


@pytest.mark.parametrize("case", _of("cold") + _of("hot"), ids=_ids(_of("cold") + _of("hot")))
def test_cold_and_hot_rows_leave_the_exponent_range(case):
    """every valid row's L is beyond +-140: 2^(0 - L) of a zero key fragment, or 2^(S' - 0), is outside fp32"""
    T = case[2]
    if case[0] == "keyed":
        T = min(V.key_lengths_of(case))                          # rows every sequence has below its key length
    L = _row_L(case)[:, :, :T][_valid(case[2])[:, :, :T].expand(-1, V.ATTN_H, -1)]
    print("%s: L in [%.0f, %.0f]" % (V.case_id(case), float(L.min()), float(L.max())))
    assert torch.isfinite(L).all()
    assert float(L.max()) < -140 if case[1] == "cold" else float(L.min()) > 140


def _moves(S, T, causal):
    """the rescale decisions of the forward sweep (bf16_ref._attn_forward_value / causal_ref._forward_value): (B, h, query tile, key
    tile) bool, and the final running maximum (B, h, nt, 32)"""
    B, h = S.shape[:2]
    nt = -(-T // 32)
    Sp = torch.zeros(B, h, nt * 32, T, dtype=S.dtype)
    Sp[:, :, :T] = S
    if causal:
        Sp = Sp.masked_fill(torch.arange(T).reshape(1, T) > torch.arange(nt * 32).reshape(-1, 1), float("-inf"))
    St = Sp.reshape(B, h, nt, 32, T)
    moves = torch.zeros(B, h, nt, nt, dtype=torch.bool)
    for kt in range(nt):
        tmax = St[..., 32 * kt: min(T, 32 * kt + 32)].amax(dim=-1)
        if kt == 0:
            m = tmax
            continue
        rel = tmax - m
        mv = (rel > E.RESCALE_THR).any(dim=-1, keepdim=True)
        m = torch.where(mv, m + rel.clamp(min=0.0), m)
        moves[:, :, :, kt] = mv[..., 0]
    return moves, m, St


@pytest.mark.parametrize("case", _of("rising"), ids=_ids(_of("rising")))
def test_rising_keys_move_the_running_maximum_at_every_tile(case):
    """in every query tile that holds a valid row (a tile of blanked rows only has Q' = 0 and nothing to move), at every key tile after
    the first; causally, at every key tile up to the diagonal"""
    sel, _, T, dk, _ = case
    q, k, v, g, mask, kl = V.sdpa_inputs(case)
    moves, _, _ = _moves(V.log2_scores(q * mask, k, V.ATTN_H), T, sel == "causal")
    nt = moves.shape[-1]
    for b, n in enumerate(V.attn_lengths(T)):
        for qt in range(-(-n // 32)):
            last = qt if sel == "causal" else nt - 1
            assert moves[b, :, qt, 1:last + 1].all(), (b, qt)
    assert nt > 1


@pytest.mark.parametrize("case", _of("falling"), ids=_ids(_of("falling")))
def test_falling_keys_never_move_it_and_underflow(case):
    sel, _, T, dk, _ = case
    q, k, v, g, mask, kl = V.sdpa_inputs(case)
    moves, m, St = _moves(V.log2_scores(q * mask, k, V.ATTN_H), T, False)
    assert not moves.any()
    if T == 290:                                                 # ten tiles: the last one is below 2^-149 of the first for every valid query
        p = torch.exp2((St[:, :, 0, :, 288:] - m[:, :, 0].unsqueeze(-1)).float())
        assert (p == 0).all()
        whole = torch.exp2((St[:, :, 0, :, 256:288] - m[:, :, 0].unsqueeze(-1)).float())
        assert (whole == 0).all()                                # a whole 32 x 32 tile


def _hazard_margin(case):
    """min over the hazard pairs of (masked S') - (L of the row's visible keys): the pairs of a valid query with a masked key of the
    boundary tile (keyed) or of its diagonal tile (causal)"""
    sel, _, T, dk, j0 = case
    S, vis = _scores(case)
    L = _row_L(case)
    t0, t1 = 32 * (j0 // 32), min(T, 32 * (j0 // 32) + 32)       # the tile that holds j0
    if sel == "keyed" and j0 % 32 == 0:
        return float("inf"), 0                                   # (33, 32): the tile of the first masked key lies wholly behind the length
    worst, pairs = float("inf"), 0
    for b, n in enumerate(V.attn_lengths(T)):
        rows = range(min(n, T)) if sel == "keyed" else range(t0, min(j0, n))
        for t in rows:
            margin = S[b, :, t, j0:t1] - L[b, :, t].unsqueeze(-1)
            worst, pairs = min(worst, float(margin.min())), pairs + margin.numel()
    return worst, pairs


@pytest.mark.parametrize("case", _of("step"), ids=_ids(_of("step")))
def test_step_keys_overflow_against_the_visible_normaliser(case):
    worst, pairs = _hazard_margin(case)
    print("%s: %d hazard pairs, smallest S' - L = %.0f" % (V.case_id(case), pairs, worst))
    if (case[2], case[4]) == (33, 32):
        assert pairs == 0
        return
    assert pairs > 0 and worst >= 140


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_attention_references_stay_finite(case):
    for n, t in V.sdpa_reference(case).items():
        assert np.isfinite(t).all(), n


# ------------------------------------------------------------------------------------------------ LayerNorm regimes
LN_SHAPES = [(50, 40), (50, 128), (50, 256)]


@pytest.mark.parametrize("M,d", LN_SHAPES)
@pytest.mark.parametrize("regime", V.LN_REGIMES)
def test_layer_norm_regimes(regime, M, d):
    x, a, b, g = (t.double() for t in V.layer_norm_input(regime, M, d))
    sigma = x.std(dim=-1)
    if regime == "one_constant_row":
        assert sigma[1] == 0 and (sigma[[0] + list(range(2, M))] > 0.5).all()
        y = V.layer_norm_fp64(x, a, b)
        assert torch.isfinite(y).all() and torch.equal(y[1], b)
        return
    lo, hi = V.LN_DECADE[regime]
    assert (sigma > lo).all() and (sigma < hi).all()
    y, wrong = V.layer_norm_fp64(x, a, b), V.layer_norm_fp64(x, a, b, inside=True)
    assert torch.isfinite(y).all()
    rel = float((wrong - y).norm() / y.norm())
    print("LayerNorm %s d %d: sqrt(var + eps) differs by %.2e rel-L2" % (regime, d, rel))
    if regime in ("tiny", "sub_eps"):
        assert rel > 0.5
    assert torch.allclose(y, E.oracle.layer_norm(x, a, b), rtol=1e-12, atol=1e-12)       # the spelled-out form is the reference's


# ------------------------------------------------------------------------------------------------ scan regimes
def lstm_reference(regime, T, B, H, jitter=None, seed=0, dtype=torch.float64):
    gx, W, h0, c0, gh, gc, hi, lo = V.lstm(regime, T, B, H)
    leaves = [t.to(dtype).requires_grad_() for t in (gx, W, h0, c0)]
    gh, gc = gh.to(dtype), gc.to(dtype)
    if jitter is None:
        h, c = E.lstm_scan(*leaves)
    else:
        with E.jitter(jitter, seed=seed):
            h, c = E.lstm_scan(*leaves)
            ((h * gh).sum() + (c * gc).sum()).backward()
    if jitter is None:
        ((h * gh).sum() + (c * gc).sum()).backward()
    out = {"h": h.detach().double().numpy(), "c": c.detach().double().numpy()}
    out.update(zip(("dgx", "dW", "dh0", "dc0"), (t.grad.double().numpy() for t in leaves)))
    return out


def mfn_reference(regime, T, B, jitter=None, seed=0, dtype=torch.float64):
    apre, chat, Wm, W2, b2, g, hi, lo = V.mfn(regime, T, B)
    leaves = [t.to(dtype).requires_grad_() for t in (apre, chat, Wm, W2, b2)]
    g = g.to(dtype)
    if jitter is None:
        mem = E.mfn_mem_scan(*leaves)
        (mem * g).sum().backward()
    else:
        with E.jitter(jitter, seed=seed):
            mem = E.mfn_mem_scan(*leaves)
            (mem * g).sum().backward()
    return dict(zip(("mem", "dapre", "dchat", "dWm", "dW2", "db2"), [mem.detach().double().numpy()] + [t.grad.double().numpy() for t in leaves]))


def _norm(a):
    return float(np.linalg.norm(a))


@pytest.mark.parametrize("T", V.LONG_T)
@pytest.mark.parametrize("fam,B,H", V.LSTM_FAMILIES, ids=[f[0] for f in V.LSTM_FAMILIES])
def test_lstm_long_memory_carries_the_last_gradient_to_step_0(fam, B, H, T):
    ref = lstm_reference("long_memory", T, B, H)
    d = ref["dgx"]
    r0, rh, cmax = _norm(d[0]) / _norm(d[T - 1]), _norm(d[T // 2]) / _norm(d[T - 1]), float(np.abs(ref["c"]).max())
    print("lstm long_memory %s T %d: |dgx[0]| / |dgx[T-1]| = %.2g, |dgx[T/2]| / |dgx[T-1]| = %.2g, max |c| = %.1f" % (fam, T, r0, rh, cmax))
    assert all(np.isfinite(t).all() for t in ref.values())
    assert r0 > 0.1 and rh > 0.1 and cmax < 100


@pytest.mark.parametrize("T", V.LONG_T)
@pytest.mark.parametrize("fam,B", V.MFN_FAMILIES, ids=[f[0] for f in V.MFN_FAMILIES])
def test_mfn_long_memory_carries_the_last_gradient_to_step_0(fam, B, T):
    ref = mfn_reference("long_memory", T, B)
    d = ref["dapre"]
    r0, rh, mmax = _norm(d[0]) / _norm(d[T - 1]), _norm(d[T // 2]) / _norm(d[T - 1]), float(np.abs(ref["mem"]).max())
    print("mfn long_memory %s T %d: |dapre[0]| / |dapre[T-1]| = %.2g, |dapre[T/2]| / |dapre[T-1]| = %.2g, max |mem| = %.1f" % (fam, T, r0, rh, mmax))
    assert all(np.isfinite(t).all() for t in ref.values())
    assert r0 > 0.1 and rh > 0.1 and mmax < 100


@pytest.mark.parametrize("fam,B,H", V.LSTM_FAMILIES, ids=[f[0] for f in V.LSTM_FAMILIES])
def test_lstm_overflow_saturates_exactly(fam, B, H):
    T = V.OVERFLOW_T
    gx, W, h0, c0, gh, gc, hi, lo = V.lstm("overflow", T, B, H)
    ref = lstm_reference("overflow", T, B, H)
    assert all(np.isfinite(t).all() for t in ref.values())
    hprev = torch.cat([h0.double().unsqueeze(0), torch.from_numpy(ref["h"])[:-1]])
    pre = gx.double() + E.bf16(hprev) @ E.bf16(W.double()).t()
    tanh_cols = torch.zeros(4 * H, dtype=torch.bool)
    tanh_cols[2 * H:3 * H] = True
    act = torch.where(tanh_cols, torch.tanh(pre), torch.sigmoid(pre)).float()
    assert (act[hi] == 1).all()
    assert torch.equal(act[lo], torch.where(tanh_cols.expand_as(lo)[lo], -1.0, 0.0).float())
    rms = float(np.sqrt((ref["dgx"] ** 2).mean()))
    assert float(np.abs(ref["dgx"][(hi | lo).numpy()]).max()) < 1e-6 * rms
    print("lstm overflow %s: max |c| = %.1f" % (fam, float(np.abs(ref["c"]).max())))


@pytest.mark.parametrize("fam,B", V.MFN_FAMILIES, ids=[f[0] for f in V.MFN_FAMILIES])
def test_mfn_overflow_stays_finite(fam, B):
    """apre = -200 closes the ReLU (no gradient, exactly); apre = +200 drives the two gates of the units it feeds to 0 or 1"""
    apre, chat, Wm, W2, b2, g, hi, lo = V.mfn("overflow", V.OVERFLOW_T, B)
    ref = mfn_reference("overflow", V.OVERFLOW_T, B)
    assert all(np.isfinite(t).all() for t in ref.values())
    assert (ref["dapre"][lo.numpy()] == 0).all()
    assert float(np.abs(ref["mem"]).max()) < V.OVERFLOW_T        # |chat| < 1 and both gates <= 1: at most one unit per step


# ------------------------------------------------------------------------------------------------ yardsticks
# Yardstick of the stand-alone attention, (rel-L2, per-row maximum) per tensor: the worst over T, the selections and the regimes of one
# family at one d_k (sdpa_fp32_yardstick).  Only the entries that test_gpu_value_regimes.py widens a bound from are recorded; the bound
# is 4x the entry.  Measured on the MI355X (worst over the family's cases, both modes), rel-L2 / per row:
#   cold, hot     d_k 16: dq 1.2e-2 / 1.6e-1, dk 5.1e-3 / 6.2e-2, dv 1.5e-3 / 3.0e-2;  d_k 64: y 4.6e-4 / 5.3e-3, dq 1.6e-2 / 2.4e-1,
#                 dk 4.0e-3 / 6.4e-2 (dq = sum_j dS_j K_j cancels a component of 40 per key: scores of 600 carry 6e-5 absolute in fp32)
#   step          d_k 16: dk 1.1e-3 / 2.6e-2 (p = 0.1; sdpa_fp32_yardstick says why);  d_k 64: dq 1.8e-3 / 3.8e-2
#   rising, falling  d_k 16: dq 1.9e-3 / 4.3e-2, dk 2.2e-3 / 5.2e-2, dv 1.1e-3 / 2.4e-2;  d_k 64: dq 1.8e-3 / 2.5e-2, dk 2.2e-3 / 3.7e-2
# Everything else holds the bounds of test_gpu_bf16_faithful (peaked: y 6.3e-5 / 9.2e-4, gradients 5.7e-4 / 1.3e-2).
_CH, _ST, _RF = ("cold", "hot"), ("step",), ("rising", "falling")
SDPA_FP32_YARD = {
    (_CH, 16, "dq"): (1.3e-2, 1.6e-1), (_CH, 16, "dk"): (2.6e-3, 4.9e-2), (_CH, 16, "dv"): (1.4e-3, 2.9e-2),
    (_CH, 64, "y"): (8.4e-4, 4.9e-3), (_CH, 64, "dq"): (3.2e-2, 2.2e-1), (_CH, 64, "dk"): (3.9e-3, 8.9e-2),
    (_ST, 16, "dk"): (5.6e-4, 1.3e-2), (_ST, 64, "dq"): (8.3e-3, 9.5e-2),
    (_RF, 16, "dq"): (2.7e-3, 4.6e-2), (_RF, 16, "dk"): (2.1e-3, 4.5e-2), (_RF, 16, "dv"): (1.0e-3, 2.4e-2),
    (_RF, 64, "dq"): (5.6e-3, 6.9e-2), (_RF, 64, "dk"): (2.8e-3, 6.3e-2),
}


_SDPA_YARDS = {}


SDPA_MASKS = 4


def _synthetic_drop(case, s=0):
    """a p = 0.1 mask from torch's CPU generator (the kernels' own bits need a GPU): the train-mode roundings of the reference"""
    T = case[2]
    g = torch.Generator().manual_seed(1234 + T + case[3] + 1000 * s)
    return (torch.rand(V.ATTN_B, V.ATTN_H, T, T, generator=g) >= 0.1).double() / 0.9


def sdpa_fp32_yardstick(family, dk):
    """{tensor: (rel-L2, per-row maximum)}: bf16_ref / causal_ref against themselves, evaluated in float32, and in float64 under
    jitter(6e-8) (nearly one-hot rows put a whole key's gradient on a few bf16 roundings); eval mode and SDPA_MASKS p = 0.1 masks; the
    worst over the cases of `family` (a tuple of regimes) at d_k.
    Several masks, because the train-mode figure of `step` is one event that a mask shows or not: dk of the key that nearly every query
    attends is a sum of residues P (dP m - delta) that cancel to 1e-3 of their terms, the float32 evaluation moves the sum by 6e-4
    relative, and where that crosses a bf16 midpoint of the OUTPUT the row moves by one output ulp (0.125 at 23, in a row 5.8x the rms
    row: 2.64e-2 with the mask the kernels draw for keyed step(270), T = 290, d_k = 16, where the float32 reference lands on the
    kernels' very value; 1.3e-2 under mask 1 here)."""
    if (family, dk) in _SDPA_YARDS:
        return _SDPA_YARDS[(family, dk)]
    out = {}
    for case in CASES:
        if case[1] in family and case[3] == dk:
            for i, drop in enumerate([None] + [_synthetic_drop(case, s) for s in range(SDPA_MASKS)]):
                r64 = V.sdpa_reference(case, drop)
                others = [V.sdpa_reference(case, drop, dtype=torch.float32)]
                if i < 2:
                    with E.jitter(6e-8):
                        others.append(V.sdpa_reference(case, drop))
                for o in others:
                    for n in r64:
                        rel, row = V.sdpa_measures(o, r64, n)
                        out[n] = (max(rel, out.get(n, (0, 0))[0]), max(row, out.get(n, (0, 0))[1]))
    _SDPA_YARDS[(family, dk)] = out
    return out


@pytest.mark.parametrize("key", sorted(SDPA_FP32_YARD), ids=lambda k: "%s_dk%d_%s" % ("-".join(k[0]), k[1], k[2]))
def test_recorded_attention_yardsticks_do_not_overstate(key):
    family, dk, tensor = key
    got = sdpa_fp32_yardstick(family, dk)[tensor]
    print("fp32 yardstick %s: %.2e / %.2e (recorded %.2e / %.2e)" % ((key,) + got + SDPA_FP32_YARD[key]))
    assert SDPA_FP32_YARD[key][0] <= got[0] and SDPA_FP32_YARD[key][1] <= got[1]


def ln_fp32_yardstick(regime, M, d):
    """y, dx, da, db of the fp64 formula evaluated in float32 against float64 -> {tensor: (rel-L2, per-row maximum)}"""
    res = []
    for dt in (torch.float64, torch.float32):
        x, a, b, g = (t.to(dt) for t in V.layer_norm_input(regime, M, d))
        lv = [t.requires_grad_() for t in (x, a, b)]
        y = V.layer_norm_fp64(*lv)
        y.backward(g)
        res.append({"y": y.detach().numpy(), "dx": lv[0].grad.numpy(), "da": lv[1].grad.numpy(), "db": lv[2].grad.numpy()})
    return {n: measures(res[1][n], res[0][n]) for n in res[0]}


# LayerNorm `offset` (rows of mean 1000 centred in fp32: an ulp of 1000 is 6e-5 of the unit spread): the worst over d in {40, 128, 256}.
# y: yardstick 5.5e-5, bound 2.2e-4, measured 5.0e-5 (d 40); dx, da, db hold the default 3e-4 (measured <= 5e-5)
LN_OFFSET_YARD = {"y": 5.5e-5}


def test_recorded_layer_norm_yardstick_does_not_overstate():
    worst = {}
    for M, d in LN_SHAPES:
        for n, (rel, row) in ln_fp32_yardstick("offset", M, d).items():
            worst[n] = max(worst.get(n, 0.0), rel)
    print("LayerNorm offset fp32 yardstick: " + "  ".join("%s %.2e" % kv for kv in worst.items()))
    for n, v in LN_OFFSET_YARD.items():
        assert v <= worst[n], n


# Yardsticks of long_memory (scan_yardstick: jitter seeds and the float32 evaluation), per (family, T).  "step" is the
# per-time-step measure (value_regimes.per_step) of dgx / dapre; a tensor's entry is (rel-L2, per-row maximum, per-sequence maximum) and
# is recorded only where test_gpu_value_regimes.py widens that tensor's bound from it; "<name>_scale" the least-squares scale.
# Measured per-step values on the MI355X (bound: 4x "step", or the tier's per-row bound of the tensor where that is wider):
#   lstm  u1 1.2e-3 / 6.9e-3 (T 70 / 130), u2 1.4e-3 / 4.1e-3, gen 1.7e-3 / 6.6e-3, cl4 1.3e-3 / 4.9e-3, s256 2.7e-3 / 1.1e-2
#   mfn   sw1 5.1e-2 (the float32 reference: 5.1e-2) / 2.3e-1, sw2 2.9e-2 / 4.4e-2, gen 2.7e-2 / 3.9e-2;  stack 2.4e-3 / 3.7e-3;  fb 5.6e-4 / 4.7e-4
# The widened tensors measure at or below their yardstick x 1.3, e.g. lstm gen T 70 dgx 5.4e-3 per sequence (yardstick 5.3e-3: jitter
# seed 1 tips the very rounding the kernels tip), s256 T 130 dW scale 3.3e-4 (2.0e-4), mfn gen T 130 db2 4.6e-2 per entry (6.8e-2).
LSTM_LONG_YARD = {
    ("u1", 70): {"step": 2.5e-04},
    ("u1", 130): {"step": 2.2e-02, "dW_scale": 1.3e-03, "dgx": (5.8e-03, 3.1e-02, 7.5e-03), "dh0": (6.8e-03, 8.7e-03)},
    ("u2", 70): {"step": 4.7e-04, "dgx": (1.6e-04, 4.7e-03, 1.4e-03)},
    ("u2", 130): {"step": 3.5e-03, "dW_scale": 7.7e-05, "dgx": (9.4e-04, 4.7e-02, 1.2e-02), "dh0": (1.0e-03, 1.2e-02),
                  "h": (1.2e-04, 4.0e-03, 1.2e-03)},
    ("gen", 70): {"step": 4.3e-04, "dgx": (3.8e-04, 1.4e-02, 5.3e-03), "h": (4.2e-05, 1.2e-03, 5.3e-04)},
    ("gen", 130): {"step": 3.0e-03, "c": (5.5e-05, 1.5e-03, 7.6e-04), "dW_scale": 6.2e-05, "dc0": (7.1e-04, 8.9e-03),
                   "dgx": (6.8e-04, 4.4e-02, 8.4e-03), "dh0": (9.4e-04, 8.9e-03), "h": (1.0e-04, 4.0e-03, 1.2e-03)},
    ("cl4", 70): {"step": 6.8e-03},
    ("cl4", 130): {"step": 2.0e-02, "dW_scale": 2.2e-03, "dgx": (4.8e-03, 2.8e-02, 6.6e-03)},
    ("s256", 70): {"step": 4.1e-03, "dW_scale": 4.9e-05, "dgx": (1.3e-03, 1.0e-02, 3.5e-03)},
    ("s256", 130): {"step": 1.6e-02, "dW_scale": 2.0e-04, "dc0": (4.0e-03, 9.4e-03), "dgx": (4.1e-03, 3.8e-02, 1.0e-02),
                    "dh0": (4.6e-03, 8.7e-03), "h": (1.0e-03, 7.3e-03, 2.6e-03)},
}
MFN_LONG_YARD = {
    ("sw1", 70): {"step": 5.1e-02, "dW2_scale": 8.7e-04, "dWm_scale": 5.8e-04},
    ("sw1", 130): {"step": 2.4e-01, "dW2": (2.6e-02, 1.2e-01), "dW2_scale": 2.7e-03, "dWm_scale": 2.4e-03, "db2": (2.5e-02, 2.9e-02),
                   "dchat": (3.0e-02, 4.7e-02, 3.7e-02)},
    ("sw2", 70): {"step": 2.3e-02, "dchat": (2.6e-03, 3.0e-02, 2.3e-02)},
    ("sw2", 130): {"step": 3.5e-02, "db2": (6.3e-03, 2.3e-02), "dchat": (7.2e-03, 5.5e-02, 4.0e-02)},
    ("gen", 70): {"step": 2.2e-02, "dapre": (8.2e-03, 3.6e-01, 6.3e-02), "dchat": (3.9e-03, 4.8e-02, 3.0e-02)},
    ("gen", 130): {"step": 2.7e-02, "dapre": (1.1e-02, 4.4e-01, 6.8e-02), "db2": (1.8e-02, 6.8e-02), "dchat": (6.7e-03, 5.4e-02, 3.8e-02)},
}
STACK_STEP_YARD = {70: 2.1e-3, 130: 7.1e-3}                    # per T: the per-time-step measure of dgx0
FB_STEP_YARD = {70: 4.1e-4, 130: 0.0}                          # ... of dgxc (T = 130: nothing tips)


def _figures(a, b, tb, weights):
    from gpu_harness import ls_scale, seq_max
    out = {}
    for n in a:
        rows = (lambda t: t.ravel()) if n == "db2" else (lambda t: t)         # db2: a row is one entry, as the GPU tests measure it
        out[n] = measures(rows(b[n]), rows(a[n])) + ((seq_max(b[n], a[n]),) if n in tb else ())
        if n in weights:
            out[n + "_scale"] = abs(ls_scale(b[n], a[n]))
    return out


def _worst(figs):
    out = {}
    for f in figs:
        for n, v in f.items():
            out[n] = v if n not in out else (max(out[n], v) if isinstance(v, float) else tuple(max(a, b) for a, b in zip(out[n], v)))
    return out


def scan_yardstick(kind, fam, T, regime="long_memory"):
    """the reference against itself under jitter(6e-8), the worst of seeds 0 .. 3 (0 .. 7 at B <= 3, where one seed tips a rounding or
    none at all: u1 at T = 130 moves by 2.3e-2 per step under seed 1 and not at all under seeds 0, 2, 3, 4), and the reference evaluated
    in float32: jitter perturbs what is rounded to bf16, not the fp32 sums themselves, and the MFN's ReLU flips on those (sw1 at T = 70
    has a pre-activation of 3.7e-7, which any fp32 evaluation puts on the other side of 0: one entry of dapre, 5.1e-2 of a step)."""
    if kind == "lstm":
        B, H = next(f[1:] for f in V.LSTM_FAMILIES if f[0] == fam)
        a = lstm_reference(regime, T, B, H)
        runs = [lstm_reference(regime, T, B, H, jitter=6e-8, seed=s) for s in range(8 if B <= 3 else 4)]
        runs.append(lstm_reference(regime, T, B, H, dtype=torch.float32))
        return _worst({"step": V.per_step(b["dgx"], a["dgx"]), **_figures(a, b, ("h", "c", "dgx"), ("dW",))} for b in runs)
    B = next(f[1] for f in V.MFN_FAMILIES if f[0] == fam)
    a = mfn_reference(regime, T, B)
    runs = [mfn_reference(regime, T, B, jitter=6e-8, seed=s) for s in range(8 if B <= 3 else 4)]
    runs.append(mfn_reference(regime, T, B, dtype=torch.float32))
    return _worst({"step": V.per_step(b["dapre"], a["dapre"]), **_figures(a, b, ("mem", "dapre", "dchat"), ("dWm", "dW2"))} for b in runs)


def _fmt(v):
    return "%.2e" % v if isinstance(v, float) else "(" + ", ".join("%.2e" % x for x in v) + ")"


@pytest.mark.parametrize("T", V.LONG_T)
@pytest.mark.parametrize("kind,fam", [("lstm", f[0]) for f in V.LSTM_FAMILIES] + [("mfn", f[0]) for f in V.MFN_FAMILIES])
def test_recorded_scan_yardsticks_do_not_overstate(kind, fam, T):
    fresh = scan_yardstick(kind, fam, T)
    print("%s %s T %d jitter yardstick: {%s}" % (kind, fam, T, ", ".join('"%s": %s' % (n, _fmt(v)) for n, v in fresh.items())))
    for n, rec in (LSTM_LONG_YARD if kind == "lstm" else MFN_LONG_YARD).get((fam, T), {}).items():
        assert np.all(np.asarray(rec) <= np.asarray(fresh[n])), n


def stacked_reference(kind, regime, T, jitter=None):
    from test_gpu_bf16_stack_fb import fb_ref, stack_ref
    inp, w, sat = (V.stack_inputs if kind == "stack" else V.fb_inputs)(regime, T)
    c = (V.stack_case if kind == "stack" else V.fb_case)(T)
    fn = stack_ref if kind == "stack" else fb_ref
    if jitter is None:
        return fn(c, inputs=(inp, w)), sat
    with E.jitter(jitter):
        return fn(c, inputs=(inp, w)), sat


@pytest.mark.parametrize("T", V.LONG_T)
@pytest.mark.parametrize("kind", ["stack", "fb"])
def test_stacked_and_feedback_long_memory(kind, T):
    ref, _ = stacked_reference(kind, "long_memory", T)
    jit, _ = stacked_reference(kind, "long_memory", T, jitter=6e-8)
    d = ref["dgx0" if kind == "stack" else "dgxc"]
    r0, rh, cmax = _norm(d[0]) / _norm(d[T - 1]), _norm(d[T // 2]) / _norm(d[T - 1]), float(np.abs(ref["c_all"]).max())
    yard = V.per_step(jit["dgx0" if kind == "stack" else "dgxc"], d)
    print("%s long_memory T %d: step 0 / last = %.2g, T/2 / last = %.2g, max |c| = %.1f; per-step jitter yardstick %.2e" % (kind, T, r0, rh, cmax, yard))
    assert all(np.isfinite(t).all() for t in ref.values())
    assert r0 > 0.1 and rh > 0.1 and cmax < 100
    assert (STACK_STEP_YARD if kind == "stack" else FB_STEP_YARD)[T] <= yard


@pytest.mark.parametrize("kind", ["stack", "fb"])
def test_stacked_and_feedback_overflow(kind):
    ref, sat = stacked_reference(kind, "overflow", V.OVERFLOW_T)
    assert all(np.isfinite(t).all() for t in ref.values())
    d = ref["dgx0" if kind == "stack" else "dgxc"]
    assert float(np.abs(d[sat.numpy()]).max()) < 1e-6 * float(np.sqrt((d ** 2).mean()))


# fp32 yardstick of the local attention at logits x 60: the fp64 restatement evaluated in float32 (dz; out and dh sit at 3e-8).
# bound 6e-5, measured 1.50e-5 (the CPU's float32 evaluation lands on the same figure)
LA_DZ_YARD = 1.5e-5
# ... of the encoder stack on the offset input (d = 128): bf16_ref.encoder_stack in float32 against float64; the smallest over the
# tensors the widened bound is applied to (dx and the gradients held to ENC_GRAD: 1.0e-2 .. 2.1e-2 rel-L2).  Bound 4e-2, measured
# 8.9e-3 (dx) to 1.3e-2 (layer 0's first LayerNorm gain)
ENC_OFFSET_GRAD_YARD = 1.0e-2


def test_recorded_local_attention_yardstick_does_not_overstate():
    import test_gpu_value_regimes as G
    z, h, valid, g = G.la_inputs()
    res = []
    for dt in (torch.float64, torch.float32):
        zd, hd = z.to(dt).requires_grad_(), h.to(dt).requires_grad_()
        G._local_attention_fp64(zd, hd, valid.to(dt)).backward(g.to(dt))
        res.append(zd.grad.double().numpy())
    rel = measures(res[1], res[0])[0]
    print("local attention dz fp32 yardstick %.2e" % rel)
    assert LA_DZ_YARD <= rel


def test_recorded_encoder_offset_yardstick_does_not_overstate():
    import test_gpu_value_regimes as G
    res = []
    for dt in (torch.float64, torch.float32):
        pd = {k: v.to(dt).clone().requires_grad_() for k, v in G.enc_params(128, G.ENC_N, False).items()}
        x, g, mask = G.enc_inputs(128, "offset")
        xd = x.to(dt).requires_grad_()
        E.encoder_stack(pd, "", xd, mask.to(dt), 8).backward(g.to(dt))
        res.append(dict({k: v.grad.double().numpy() for k, v in pd.items()}, dx=xd.grad.double().numpy()))
    for name in res[0]:
        if G.enc_offset_widened(name):
            rel = measures(res[1][name], res[0][name])[0]
            print("encoder offset fp32 yardstick %-44s %.2e" % (name, rel))
            assert ENC_OFFSET_GRAD_YARD <= rel, name


# MFN scans at `overflow`: u = ReLU(apre + mem Wm) near 200 is an MFMA operand, and a bf16 ulp there is 1.  Among the ~75 000 such u
# of a case some lie within fp32 resolution (2^-24 relative) of a bf16 midpoint: a tie that fp64 breaks one way and an fp32 sum either
# way.  The yardstick tips every such rounding in the reference itself (none, if no u is that near a midpoint) and measures
# the reference against that: (rel-L2, per-row maximum, per-sequence maximum) of mem.  gen (B = 513): u = 200.4999936 at t = 5,
# sequence 499, 3.2e-8 from the midpoint; bound 4x; measured 2.4e-5 / 9.29e-3 / 5.48e-3 — the kernels against the TIPPED reference
# measure 2.4e-5 / 1.5e-3 / 5.4e-4, inside the default.
MFN_OVERFLOW_YARD = {"gen": {"mem": (2.3e-5, 9.2e-3, 5.4e-3)}}


def mfn_overflow_tie_yardstick(B):
    apre, chat, Wm, W2, b2, g, hi, lo = V.mfn("overflow", V.OVERFLOW_T, B)
    lv = [t.double() for t in (apre, chat, Wm, W2, b2)]
    with torch.no_grad():
        mem = E.mfn_mem_scan(*lv)
        prev = torch.cat([torch.zeros_like(mem[:1]), mem[:-1]])
        u = torch.relu(lv[0] + E.bf16(prev) @ E.bf16(lv[2]).t())
        ulp = 2.0 ** (torch.floor(torch.log2(u.clamp(min=1e-30))) - 7)
        frac = u / ulp - torch.floor(u / ulp)
        dist = torch.where(u > 0, (frac - 0.5).abs() * ulp / u.clamp(min=1e-30), torch.ones_like(u))
        tie = dist < 2.0 ** -24                                  # every rounding fp32 cannot resolve, each tipped to its other neighbour
        if not tie.any():
            return [], {"mem": (0.0, 0.0, 0.0)}
        nudge = torch.where(frac > 0.5, -4e-7, 4e-7)

        def tip(t, r, dt):
            return torch.where(tie[t], r * (1 + nudge[t]), r)
        tipped = E.mfn_mem_scan(*lv, mutate={"u": tip})
    where = [(int(t), int(b), int(j), float(u[t, b, j])) for t, b, j in zip(*np.nonzero(tie.numpy()))]
    return where, _figures({"mem": mem.numpy()}, {"mem": tipped.numpy()}, ("mem",), ())


@pytest.mark.parametrize("fam,B", V.MFN_FAMILIES, ids=[f[0] for f in V.MFN_FAMILIES])
def test_recorded_overflow_tie_yardstick_does_not_overstate(fam, B):
    where, fresh = mfn_overflow_tie_yardstick(B)
    print("mfn %s overflow: nearest tie %s -> mem %s" % (fam, where, _fmt(fresh["mem"])))
    for n, rec in MFN_OVERFLOW_YARD.get(fam, {}).items():
        assert np.all(np.asarray(rec) <= np.asarray(fresh[n])), n
