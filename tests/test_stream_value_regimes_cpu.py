"""The value regimes of tests/stream_value_regimes.py, held on the references alone (no GPU): every regime is reached at every shape
that tests/test_gpu_stream_value_regimes.py runs, and the reference stays finite there.  These are conditions on the inputs, not
measurements of any kernel: with COLD_C, STEP_S, the x 12 factor or pos_w at unit scale they fail.

The second half holds the yardsticks behind every bound of the GPU file that is wider than the imported one.  A yardstick involves no
kernel: the same reference evaluated with float32 tensors against its float64 result, or against itself under bf16_ref.jitter(6e-8).
A bound is 4x its yardstick.  The recorded constants are checked here against a fresh evaluation: a constant may understate its
yardstick, never overstate it (they stand about 15 % under it: another CPU's float32 sums land a few percent away).
"""
import numpy as np
import pytest
import torch

import band_ref as Bn
import bf16_ref as E
import stream_value_regimes as SV
import value_regimes as V
from gpu_harness import measures

LN2 = E.LN2
ENC_CASES = SV.enc_cases()
ENC_IDS = [SV.enc_id(c) for c in ENC_CASES]
BAND_CASES = SV.band_cases()
BAND_IDS = [SV.band_id(c) for c in BAND_CASES]
_SCORES = {}


def _enc(case):
    """y, per-layer scores, the visible-key scores, their row maxima and log-normalisers, and the valid rows (B, h, T)"""
    if case not in _SCORES:
        kind, regime, d, h, n, T, span = case
        y, Ss = SV.enc_scores(case)
        vis = SV.enc_visible(case)
        layers = []
        for S_ in Ss:
            Sv = S_.masked_fill(~vis, float("-inf"))
            layers.append((S_, Sv, Sv.amax(dim=-1), torch.logsumexp(Sv * LN2, dim=-1) / LN2))
        _SCORES[case] = (y, layers, SV.valid_rows(T).unsqueeze(1).expand(-1, h, -1), vis)
    return _SCORES[case]


def _of(cases, *regimes):
    return [c for c in cases if (c[1] if len(c) == 7 else c[0]) in regimes]


def _eids(cs):
    return [SV.enc_id(c) for c in cs]


def _bids(cs):
    return [SV.band_id(c) for c in cs]


# ------------------------------------------------------------------------------------------------ part A: the encoder streams
@pytest.mark.parametrize("case", _of(ENC_CASES, "cold", "hot"), ids=_eids(_of(ENC_CASES, "cold", "hot")))
def test_cold_and_hot_stream_rows_leave_the_exponent_range(case):
    """every valid row's maximum is below -140 / above +140, in every layer that carries the shift (the N = 2 case: in both)"""
    y, layers, valid, vis = _enc(case)
    assert len(layers) == case[4]
    for i, (S_, Sv, m, L) in enumerate(layers):
        print("%s layer %d: row maxima in [%.0f, %.0f]" % (SV.enc_id(case), i, float(m[valid].min()), float(m[valid].max())))
        assert torch.isfinite(m[valid]).all()
        assert float(m[valid].max()) < -140 if case[1] == "cold" else float(m[valid].min()) > 140


def _hazard_rows(case):
    """the rows named in the issue and the masked keys that are hot for them: step_up: t < j0, keys j >= j0 (above the diagonal of an
    extend tile); step_down: t >= j0 + span - 1, keys j < j0 (older than the band; key t - span sat in the ring row step t overwrites)"""
    kind, regime, d, h, n, T, span = case
    t, j0 = torch.arange(T), SV.j0_of(case)
    if regime == "step_up":
        return t < j0, t >= j0
    return t >= j0 + span - 1, t < j0


@pytest.mark.parametrize("case", _of(ENC_CASES, "step_up", "step_down"), ids=_eids(_of(ENC_CASES, "step_up", "step_down")))
def test_masked_stream_keys_overflow_against_the_visible_normaliser(case):
    y, layers, valid, vis = _enc(case)
    S_, Sv, m, L = layers[0]
    rows, hot = _hazard_rows(case)
    assert not (vis[rows][:, hot]).any()                        # none of them is visible to such a row
    sel = valid & rows
    margin = (S_[:, :, :, hot] - L.unsqueeze(-1)).amin(dim=-1)[sel]
    print("%s: %d hazard rows, smallest S' - L over their %d masked keys = %.0f"
          % (SV.enc_id(case), int(sel.sum()), int(hot.sum()), float(margin.min())))
    assert int(sel.sum()) >= case[3] * 8 and float(margin.min()) > 140
    if case[1] == "step_down":                                  # the key that left the band at the first such step was a hot one
        t0 = SV.j0_of(case) + case[6] - 1
        assert bool(hot[t0 - case[6]]) and bool(valid[0, 0, t0])


@pytest.mark.parametrize("case", _of(ENC_CASES, "newest", "oldest"), ids=_eids(_of(ENC_CASES, "newest", "oldest")))
def test_ramps_put_the_maximum_on_the_newest_or_the_oldest_visible_key(case):
    """in every valid row; and at least half of a full row's keys have 2^(S - m) below the smallest bf16 subnormal"""
    kind, regime, d, h, n, T, span = case
    y, layers, valid, vis = _enc(case)
    S_, Sv, m, L = layers[0]
    t = torch.arange(T)
    want = t if regime == "newest" else (t - ((span or T) - 1)).clamp(min=0)
    assert bool((Sv.argmax(dim=-1) == want)[valid].all())
    top2 = Sv[:, :, 1:].topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1])[valid[:, :, 1:]].min())
    nk = vis.sum(dim=-1)
    full = nk == nk.max()
    under = (((Sv - m.unsqueeze(-1)) < SV.SUBNORMAL) & vis).sum(dim=-1)
    share = float((under.double() / nk)[:, :, full][valid[:, :, full]].min())
    print("%s: the runner-up is at least %.1f below; %.0f %% of a full row's %d keys underflow" % (SV.enc_id(case), gap, 100 * share, int(nk.max())))
    assert gap > 8 and share >= 0.5 and bool(valid[:, :, full].any())


@pytest.mark.parametrize("case", _of(ENC_CASES, "peaked"), ids=_eids(_of(ENC_CASES, "peaked")))
def test_peaked_stream_rows_are_nearly_one_hot(case):
    y, layers, valid, vis = _enc(case)
    top = torch.softmax(layers[0][1] * LN2, dim=-1).amax(dim=-1)[valid]
    share = float((top > 0.99).double().mean())
    print("%s: %.0f %% of valid rows have a probability above 0.99" % (SV.enc_id(case), 100 * share))
    assert share >= 0.2


@pytest.mark.parametrize("case", ENC_CASES, ids=ENC_IDS)
def test_the_stream_references_stay_finite(case):
    assert np.isfinite(_enc(case)[0]).all()
    if SV.has_flat(case):
        flat = SV.enc_reference(case, flat=True)
        assert np.isfinite(flat).all()
        rows, _ = _hazard_rows(case)                             # N = 1: a row depends only on its visible windows
        assert np.array_equal(flat[:, rows.numpy()], _enc(case)[0][:, rows.numpy()])
        assert not np.array_equal(flat, _enc(case)[0])


@pytest.mark.parametrize("case", SV.PREFILL_CASES, ids=_eids(SV.PREFILL_CASES))
def test_the_prefill_references_stay_finite(case):
    assert np.isfinite(SV.prefill_reference(case)).all()
    assert SV.PREFILL + sum(SV.PREFILL_GROUPS) < case[5]


def test_the_cases_cover_what_the_issue_names():
    for d, h in SV.ENC_SHAPES:
        for span in SV.SPANS:
            assert ("ring", "step_down", d, h, 1, 70, span) in ENC_CASES and ("ring", "oldest", d, h, 1, 70, span) in ENC_CASES
        assert ("plain", "step_up", d, h, 1, 70, None) in ENC_CASES
    assert ("plain", "cold", 128, 8, 2, 70, None) in ENC_CASES and ("plain", "newest", 128, 8, 1, 130, None) in ENC_CASES
    assert all(c in ENC_CASES for c in SV.PREFILL_CASES + SV.SLOT_CASES)
    assert all(sum(g) == T for T, g in SV.GROUPS.items())
    assert SV.enc_lengths(70) == [70, 46] and SV.enc_lengths(130) == [130, 86]


# ------------------------------------------------------------------------------------------------ part B: the band's lower edge
def _band_L(case):
    regime, T, span, dk, j0 = case
    S_ = SV.band_scores(case)
    Sv = S_.masked_fill(Bn.outside_band(T, span), float("-inf"))
    return S_, torch.logsumexp(Sv * LN2, dim=-1) / LN2


def _band_valid(T):
    return (SV.R.prefix_mask(V.attn_lengths(T), T).reshape(SV.BAND_B, 1, T) != 0).expand(-1, SV.BAND_H, -1)


@pytest.mark.parametrize("case", _of(BAND_CASES, "step_down"), ids=_bids(_of(BAND_CASES, "step_down")))
def test_keys_older_than_the_band_overflow_in_a_working_tile(case):
    """pairs (valid query t, key j < t - span + 1) whose key tile the downward sweep of t's query tile visits: some have S' - L > 140"""
    regime, T, span, dk, j0 = case
    S_, L = _band_L(case)
    valid = _band_valid(T)
    pairs, worst = 0, float("-inf")
    for t in range(T):
        lo = 32 * Bn.band_lo_tile(t // 32, min(span, T))
        if t - span + 1 <= lo or not bool(valid[:, 0, t].any()):
            continue
        margin = (S_[:, :, t, lo:t - span + 1] - L[:, :, t].unsqueeze(-1))[valid[:, :, t]]
        pairs += int((margin > 140).sum())
        worst = max(worst, float(margin.max()))
    print("%s: %d pairs of a query with a masked key older than its band beyond 140, the largest S' - L = %.0f" % (SV.band_id(case), pairs, worst))
    assert pairs > 0
    if span == 64:                                              # rows without a visible key in tile qt - 2, which is swept
        assert Bn.band_lo_tile(8, span) == 6 and 287 - span + 1 >= 224


@pytest.mark.parametrize("case", _of(BAND_CASES, "falling", "rising"), ids=_bids(_of(BAND_CASES, "falling", "rising")))
def test_the_downward_sweep_moves_its_maximum_at_every_tile_or_never(case):
    """falling (older tiles hotter): in every query tile that holds a valid row the running maximum moves at every key tile below the
    diagonal; rising: it never moves, and the tiles seven and more below the diagonal round to P = 0 in bf16"""
    regime, T, span, dk, j0 = case
    S_ = SV.band_scores(case)
    moves, swept = SV.band_sweep(S_, T, span)
    assert max(qt - kt for qt, kt in swept) >= 3
    if regime == "rising":
        assert not moves.any()
        if span == 200:
            far = S_[0, :, 288:290, 64:96] - S_[0, :, 288:290, 256:290].amax(dim=-1, keepdim=True)
            assert (torch.exp2(far).to(torch.bfloat16) == 0).all() and (9, 2) in swept
        return
    for b, n in enumerate(V.attn_lengths(T)):
        for qt, kt in swept:
            if 32 * qt < n:
                assert moves[b, :, qt, kt].all(), (b, qt, kt)


@pytest.mark.parametrize("case", _of(BAND_CASES, "peaked"), ids=_bids(_of(BAND_CASES, "peaked")))
def test_peaked_band_rows_are_nearly_one_hot(case):
    top = SV.band_probs_reference(case).amax(dim=-1)[_band_valid(case[1])]
    share = float((top > 0.99).double().mean())
    print("%s: %.0f %% of valid rows have a probability above 0.99" % (SV.band_id(case), 100 * share))
    assert share >= 0.2


@pytest.mark.parametrize("case", _of(BAND_CASES, "cold"), ids=_bids(_of(BAND_CASES, "cold")))
def test_cold_band_rows_leave_the_exponent_range(case):
    L = _band_L(case)[1][_band_valid(case[1])]
    assert torch.isfinite(L).all() and float(L.max()) < -140


@pytest.mark.parametrize("case", BAND_CASES, ids=BAND_IDS)
def test_the_band_references_stay_finite(case):
    for n, t in SV.band_reference(case).items():
        assert np.isfinite(t).all(), n


@pytest.mark.parametrize("case", SV.band_probs_cases(), ids=_bids(SV.band_probs_cases()))
def test_the_band_map_reference_is_a_distribution_over_the_band(case):
    regime, T, span, dk, j0 = case
    P = SV.band_probs_reference(case)
    assert torch.isfinite(P).all() and (P.masked_select(Bn.outside_band(T, span).expand_as(P)) == 0).all()
    assert float((P.sum(dim=-1) - 1).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ yardsticks
# Part A.  (rel-L2, per-row maximum) of y: stream_ref / ring_stream_ref / prefill_ref evaluated in float32 against float64, and in
# float64 under jitter(6e-8); the worst over the cases of a family (kind, regime family, d), the flat twins and prefill walks included.
# Only the families whose 4x exceeds ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3 in either figure are recorded; every other family holds the
# imported bounds.
# fresh: plain 2.6e-4 / 3.0e-3, ring 2.6e-4 / 3.0e-3 (the float32 evaluation; nearly one-hot rows put a whole row's context on one tipped
# rounding of V) -> bound 2e-3 / 1.0e-2; measured on the MI355X: see tests/test_gpu_stream_value_regimes.py
STREAM_YARD = {
    ("plain", "peaked", 128): (2.2e-4, 2.6e-3),
    ("ring", "peaked", 128): (2.2e-4, 2.6e-3),
}
_STREAM_YARDS = {}


def stream_yardstick(family):
    if family not in _STREAM_YARDS:
        figs = [(0.0, 0.0)]
        for case in ENC_CASES:
            if SV.enc_family(case) != family:
                continue
            runs = [(False, SV.enc_reference)] + ([(True, SV.enc_reference)] if SV.has_flat(case) else [])
            for flat, fn in runs:
                a = fn(case, flat)
                figs.append(measures(fn(case, flat, dtype=torch.float32), a))
                with E.jitter(6e-8):
                    figs.append(measures(fn(case, flat), a))
            if case in SV.PREFILL_CASES:
                a = SV.prefill_reference(case)
                figs.append(measures(SV.prefill_reference(case, dtype=torch.float32), a))
        _STREAM_YARDS[family] = SV.worst(figs)
    return _STREAM_YARDS[family]


STREAM_FAMILIES = sorted({SV.enc_family(c) for c in ENC_CASES})


@pytest.mark.parametrize("family", STREAM_FAMILIES, ids=["%s_%s_d%d" % f for f in STREAM_FAMILIES])
def test_recorded_stream_yardsticks_do_not_overstate(family):
    fresh = stream_yardstick(family)
    rec = STREAM_YARD.get(family)
    print("stream yardstick %s: %.2e / %.2e (recorded %s)" % ((family,) + fresh + (rec,)))
    if rec is not None:
        assert rec[0] <= fresh[0] and rec[1] <= fresh[1]


# Part B.  band_ref.sdpa in float32 against float64 and under jitter(6e-8), eval mode and one p = 0.1 mask from torch's CPU generator:
# the worst over the cases of a family (regime family, d_k), per tensor as (rel-L2, per-row maximum), value_regimes.zero_scale's rule
# included.
# Recorded for every family; the bound is the imported one or 4x the entry, whichever is wider:
# 4x exceeds SDPA_OUT 4e-4 / SDPA_OUT_ROW 1e-2 (y) or SDPA_GRAD 2e-3 / SDPA_GRAD_ROW 2e-2 (gradients).
# The figures of a fresh evaluation stand about 15 % above these.  dq = sum_j dS_j K_j cancels a component of 30 to 40 per key where q and
# k are shifted along u (the note at test_value_regimes_cpu.SDPA_FP32_YARD), hence dq of `cold` and `step`.
BAND_YARD = {
    ("cold", 64): {"y": (4.5e-4, 2.5e-3), "dq": (1.85e-2, 2.0e-1), "dk": (2.4e-3, 3.0e-2), "dv": (8.2e-4, 8.2e-3)},
    ("peaked", 16): {"y": (1.3e-4, 1.4e-3), "dq": (5.4e-4, 4.9e-3), "dk": (4.4e-4, 3.6e-3), "dv": (2.0e-4, 4.3e-3)},
    ("peaked", 64): {"y": (5.6e-5, 1.3e-3), "dq": (3.1e-4, 7.4e-3), "dk": (2.9e-4, 6.9e-3), "dv": (7.3e-6, 8.1e-5)},
    ("step", 16): {"y": (1.6e-4, 2.9e-3), "dq": (4.0e-3, 7.3e-2), "dk": (1.9e-3, 4.4e-2), "dv": (4.6e-4, 9.1e-3)},
    ("step", 64): {"y": (4.7e-4, 4.4e-3), "dq": (1.65e-2, 1.8e-1), "dk": (2.0e-3, 2.1e-2), "dv": (8.0e-4, 8.4e-3)},
    ("sweep", 16): {"y": (1.75e-4, 2.6e-3), "dq": (7.4e-4, 1.5e-2), "dk": (5.5e-4, 1.17e-2), "dv": (1.75e-4, 3.7e-3)},
    ("sweep", 64): {"y": (3.3e-4, 3.3e-3), "dq": (2.2e-3, 2.8e-2), "dk": (9.0e-4, 9.7e-3), "dv": (3.2e-4, 4.9e-3)},
}
_BAND_YARDS = {}


def band_yardstick(family):
    if family not in _BAND_YARDS:
        out = {}
        for case in BAND_CASES:
            if SV.band_family(case) != family:
                continue
            for drop in (None, SV.synthetic_drop(case)):
                a = SV.band_reference(case, drop)
                others = [SV.band_reference(case, drop, dtype=torch.float32)]
                with E.jitter(6e-8):
                    others.append(SV.band_reference(case, drop))
                for o in others:
                    for n in a:
                        out[n] = SV.worst([out.get(n, (0.0, 0.0)), V.sdpa_measures(o, a, n)])
        _BAND_YARDS[family] = out
    return _BAND_YARDS[family]


BAND_FAMILIES = sorted({SV.band_family(c) for c in BAND_CASES})


@pytest.mark.parametrize("family", BAND_FAMILIES, ids=["%s_dk%d" % f for f in BAND_FAMILIES])
def test_recorded_band_yardsticks_do_not_overstate(family):
    fresh = band_yardstick(family)
    print("band yardstick %s: %s" % (family, {n: "%.2e / %.2e" % v for n, v in fresh.items()}))
    for n, rec in BAND_YARD.get(family, {}).items():
        assert rec[0] <= fresh[n][0] and rec[1] <= fresh[n][1], n


# ------------------------------------------------------------------------------------------------ part C: the recurrent steps
REC_CASES = SV.rec_cases()
REC_IDS = [SV.rec_id(c) for c in REC_CASES]
_REC = {}


def _rec_of(regime):
    return [c for c in REC_CASES if c[2] == regime]


def _rids(cs):
    return [SV.rec_id(c) for c in cs]


def _rec(case):
    """the reference's output and what its gates and softmaxes were given"""
    if case not in _REC:
        with SV.capture() as cap:
            y = SV.rec_reference(case)
        _REC[case] = (y, cap)
    return _REC[case]


def _row_rms(y):
    return float(np.sqrt(np.mean(np.sum(y.reshape(-1, y.shape[-1]) ** 2, axis=1))))


@pytest.mark.parametrize("case", REC_CASES, ids=REC_IDS)
def test_the_recurrent_references_stay_finite(case):
    y = _rec(case)[0]
    assert np.isfinite(y).all() and y.shape[:2] == (SV.REC_B, SV.REC_T[case[2]])


@pytest.mark.parametrize("case", _rec_of("overflow"), ids=_rids(_rec_of("overflow")))
def test_overflow_saturates_the_step_gates_exactly(case):
    """every gate pre-activation of the walk is either ordinary (|z| < 60) or carries the +-200 (|z| > 150), exactly as many of them as
    the biases place, and there the activation is exactly 0, 1 or -1 as a float32 (test_lstm_overflow_saturates_exactly's form)"""
    y, cap = _rec(case)
    n = 0
    for kind, z in cap.gates:
        sat = z.abs() > 150
        assert not ((z.abs() >= 60) & ~sat).any()
        n += int(sat.sum())
        act = (torch.sigmoid(z) if kind == "sigmoid" else torch.tanh(z)).float()[sat]
        want = torch.where(z[sat] > 0, 1.0, 0.0 if kind == "sigmoid" else -1.0).float()
        assert torch.equal(act, want)
    print("%s: %d saturated gate entries" % (SV.rec_id(case), n))
    assert n == SV.sat_count(case) > 0


@pytest.mark.parametrize("case", _rec_of("long_memory"), ids=_rids(_rec_of("long_memory")))
def test_long_memory_carries_the_first_window_to_the_last_output(case):
    """with other draws in window 0 the LAST output moves by more than the case's per-row bound: the carried state is what the GPU
    comparison measures at T = 130"""
    import test_gpu_stream_value_regimes as G
    y = _rec(case)[0]
    other = SV.rec_reference(case, x=SV.first_window_changed(case))
    T = SV.REC_T["long_memory"]
    assert np.array_equal(other[:, 0] != y[:, 0], np.ones_like(y[:, 0], dtype=bool)) and T > 12
    moved = float(np.linalg.norm(other[:, -1] - y[:, -1], axis=-1).max()) / _row_rms(y)
    bound = G.rec_bounds(case)[1]
    print("%s: the last output moves by %.2e of the rms row (bound %.1e)" % (SV.rec_id(case), moved, bound))
    assert moved > bound
    _, mask = SV.rec_inputs(case)
    assert float(mask[0, T // 2]) == 0 and float(mask.sum()) == mask.numel() - 1          # one hole


@pytest.mark.parametrize("case", _rec_of("peaked"), ids=_rids(_rec_of("peaked")))
def test_peaked_tap_and_gate_softmaxes(case):
    """the tap softmax of the LSTM families is nearly one-hot in a good share of rows, those of steps 0 and 1 (taps reaching before
    position 0) included.  The MFN's softmax runs over 2 x 64 cell entries: at x 60 its logits spread over 12 to 29 in every row
    behind the first (0.5 at most at x 1; e^(lg - mx) is below 1e-5 at the far entries) and its top probability has a median of 0.4
    (uniform: 0.008), but it is NOT one-hot: that is what x 60 gives on these parameters, and what is asserted here."""
    fam, sh, regime = case
    if fam == "mfn":
        y, cap = _rec(case)
        lg = torch.stack([z for z, _ in cap.softmax])
        top = torch.stack([p for _, p in cap.softmax]).amax(dim=-1)
        spread = (lg.amax(dim=-1) - lg.amin(dim=-1))
        print("mfn peaked: logit spread %.0f .. %.0f, top probability median %.2f" % (float(spread.min()), float(spread.max()), float(top.median())))
        assert len(cap.softmax) == SV.REC_T[regime] and float(spread[1:].min()) > 10 and float(top.median()) > 0.3
        return
    P = torch.softmax(SV.tap_logits(case), dim=-1).amax(dim=-1)             # (B, T)
    share = float((P > 0.99).double().mean())
    print("%s: %.0f %% of the tap rows have a probability above 0.99" % (SV.rec_id(case), 100 * share))
    assert share >= 0.2 and bool((P[:, :2] > 0.99).any()) and sh[4] == 3


# Yardsticks of part C: the family's stepped reference in float32 against float64, and in float64 under jitter(6e-8), seeds 0 .. 15 (a
# walk of 9 or 130 steps at B = 2 tips a bf16 rounding under one seed and none under the next; the worst of sixteen says what ONE
# tipped rounding, carried on by the recurrence, costs).  (rel-L2, per-row maximum) of the output and, for long_memory, the per-step
# measure (value_regimes.per_step).  Recorded where a fresh evaluation shows anything beyond fp32 noise; every other case holds the
# imported bounds of its family's stream test.
REC_SEEDS = 16
# Fresh (rel-L2 / per row / per step), all from a jitter seed: lstm (12, 12, 20) long_memory 4.9e-4 / 5.5e-3 / 3.9e-3; the stacked decoder
# (d = 128: 1024 carried values a step) overflow 1.7e-3 / 6.3e-3 / 4.4e-3 and long_memory 2.3e-2 / 1.3e-1 / 9.2e-2 (one tipped h, 130 steps
# of open forget gates behind it); mfn long_memory 9.4e-4 / 6.5e-3 / 4.7e-3, peaked 1.2e-3 / 5.1e-3 / 3.6e-3 (overflow 2.9e-5 / 1.2e-4:
# inside MFN_STEP_OUT / _ROW).  Every other case moves by fp32 noise only (<= 3.2e-7) under all sixteen seeds.
REC_YARD = {
    "lstm_12_12_20_1_3_long_memory": (4.1e-4, 4.6e-3, 3.3e-3),
    "dec_128_128_2_overflow": (1.4e-3, 5.3e-3, 3.8e-3),
    "dec_128_128_2_long_memory": (2.0e-2, 1.1e-1, 7.8e-2),
    "mfn_long_memory": (7.9e-4, 5.5e-3, 4.0e-3),
    "mfn_peaked": (1.0e-3, 4.3e-3, 3.1e-3),
}
_REC_YARDS = {}


def rec_yardstick(case):
    if case not in _REC_YARDS:
        y = _rec(case)[0]
        runs = [SV.rec_reference(case, dtype=torch.float32)]
        for s in range(REC_SEEDS):
            with E.jitter(6e-8, seed=s):
                runs.append(SV.rec_reference(case))
        figs = [measures(r, y) + (V.per_step(r.transpose(1, 0, 2), y.transpose(1, 0, 2)),) for r in runs]
        _REC_YARDS[case] = tuple(max(f[i] for f in figs) for i in range(3))
    return _REC_YARDS[case]


@pytest.mark.parametrize("case", REC_CASES, ids=REC_IDS)
def test_recorded_recurrent_yardsticks_do_not_overstate(case):
    fresh = rec_yardstick(case)
    rec = REC_YARD.get(SV.rec_id(case))
    print("recurrent yardstick %s: %.2e / %.2e, per step %.2e (recorded %s)" % ((SV.rec_id(case),) + fresh + (rec,)))
    if rec is not None:
        assert all(r <= f for r, f in zip(rec, fresh))
