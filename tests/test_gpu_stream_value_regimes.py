"""The STREAM kernels and the band's lower edge on peaked, saturated and degenerate VALUES (tests/stream_value_regimes.py): what
tests/test_gpu_value_regimes.py does for the batch kernels, for the hand-written step kernels that came after it.

What each regime pins (tests/test_stream_value_regimes_cpu.py holds, on the references alone, that it is reached at every shape used here):
  A. encoder streams (csrc/encoder_step.h, encoder_extend.h, step_ring.h, step_prefill.h; step and extend, plain and ring, slots)
     * `cold` / `hot`: every row's exact maximum beyond -+140.  The softmax reference point is the row's own maximum over ALL visible
       keys, key t's own score and the other key groups' included: a sentinel start value, a maximum taken before the cross-group
       exchange or without st gives inf or an all-zero row here and is exact at unit scale;
     * `step_up`: hot keys above the diagonal of an extend tile's rows, 2^260 and more over the row's normaliser; `step_down`: hot keys
       older than a ring's band, the one in the row that step t overwrites included.  Such a key must be dropped by a SELECT: a
       multiplier gives inf x 0.  The rows that see no hot key have the bits of the flat input's rows;
     * `newest` / `oldest`: the whole row sits on the key kept in LDS / on the oldest ring row: ring_keys / ring_first_row / ring_row off
       by one costs the whole row, not 1 / span of it;
     * `peaked`: nearly one-hot rows.
  B. the batch band kernels (csrc/attn.h *_band_kernel): `step_down` puts keys older than the band, 2^300 over the visible normaliser,
     into the far-edge tile of the downward sweep (span 64: rows without a visible key in tile qt - 2); `falling` moves the running
     maximum at every tile of that sweep, `rising` never; `peaked`; `cold` at d_k = 64; the materialised band map on the same inputs.
  C. the recurrent steps (csrc/lstm_step.h with the fb / ar tails, decoder_step.h, mfn_step.h): `overflow` (gate pre-activations of
     +-200 through sigmoid_f / tanh_f, carried in c, h, mem), `long_memory` (130 steps with open forget gates: the last output depends on
     window 0, so a carry dropped anywhere shows; per step as well), `peaked` (la_row_softmax and the MFN's softmax at logits x 60).

Bounds: the imported ones of the tier that already tests the same tensor.  A bound is wider only where
test_stream_value_regimes_cpu.py holds a yardstick for it that involves no kernel, and is then 4x that yardstick.  Measured values on
the MI355X stand in the docstrings below.

Every GPU run happens in a child process (gpu_harness.run_child -> child_main), one per part, each with its own time limit: a child
that dies takes no other test with it.
"""
import numpy as np
import pytest
import torch

import band_ref as Bn
import recipe as R
import stream_value_regimes as SV
import test_stream_value_regimes_cpu as SC
import value_regimes as V
from gpu_harness import check, run_child, tmp_dir  # noqa: F401 (tmp_dir: a fixture)
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW, SDPA_GRAD, SDPA_GRAD_ROW, SDPA_OUT, SDPA_OUT_ROW
from test_gpu_decoder_stream import DEC_STEP_OUT, DEC_STEP_ROW
from test_gpu_lstm_feedback_stream import AR_STEP_OUT, AR_STEP_ROW, FB_STEP_OUT, FB_STEP_ROW
from test_gpu_lstm_stream import LSTM_STEP_OUT, LSTM_STEP_ROW
from test_gpu_mfn_stream import MFN_STEP_OUT, MFN_STEP_ROW

pytestmark = pytest.mark.gpu

ENC_CASES = SV.enc_cases()
ENC_IDS = [SV.enc_id(c) for c in ENC_CASES]
FLAT_CASES = [c for c in ENC_CASES if SV.has_flat(c)]
BAND_CASES = SV.band_cases()
BAND_IDS = [SV.band_id(c) for c in BAND_CASES]
PROBS_CASES = SV.band_probs_cases()
REC_CASES = SV.rec_cases()
REC_IDS = [SV.rec_id(c) for c in REC_CASES]
MODES = [0.0, SV.P_TRAIN]
MODE_IDS = ["eval", "p0.1"]
_SWITCHES = {"default": {}}


def _seed(case, p):
    return 2000 + case[1] + case[2] + case[3] + (7 if p else 0)


# ------------------------------------------------------------------------------------------------ child process
def _encoder(MT, case, dev):
    kind, regime, d, h, n, T, span = case
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, R.D_FF, 0.1), 0.1), n)
    enc.load_state_dict(SV.enc_params(case))
    enc = enc.to(dev).eval()
    if span is None:
        MT.causal_attention(enc)
    else:
        MT.causal_attention(enc, True, span=span)
    return enc


def _open(enc, case, slots=False):
    kind, regime, d, h, n, T, span = case
    if slots:
        s = enc.slot_stream(SV.ENC_B, T) if span is None else enc.ring_slot_stream(SV.ENC_B)
        s.reset()
        return s
    return enc.stream(SV.ENC_B, T) if span is None else enc.ring_stream(SV.ENC_B)


def _step_all(s, x, mask, t0, t1):
    return torch.stack([s.step(x[:, t], mask[:, t]) for t in range(t0, t1)], dim=1)


def _extend_all(s, x, mask, groups, t=0, slots=False):
    rows = []
    for g in groups:
        xs, ms = x[:, t:t + g].contiguous(), mask[:, t:t + g].contiguous()
        rows.append(s.extend(list(range(SV.ENC_B)), xs, [g] * SV.ENC_B, ms) if slots else s.extend(xs, ms))
        t += g
    return torch.cat(rows, dim=1)


def _enc_section(MT, dev, out):
    for case in ENC_CASES:
        kind, regime, d, h, n, T, span = case
        enc = _encoder(MT, case, dev)
        mask = SV.enc_mask(T).to(dev)
        key = "enc:%s:" % SV.enc_id(case)
        for flat in ([False, True] if SV.has_flat(case) else [False]):
            x = SV.enc_x(case, flat).to(dev)
            step = _step_all(_open(enc, case), x, mask, 0, T)
            ext = _extend_all(_open(enc, case), x, mask, SV.GROUPS[T])
            f = "flat:" if flat else ""
            out[key + f + "step"], out[key + f + "ext"] = step.cpu().numpy(), ext.cpu().numpy()
            if not flat:
                again = (_step_all(_open(enc, case), x, mask, 0, T), _extend_all(_open(enc, case), x, mask, SV.GROUPS[T]))
                out[key + "same"] = np.array([torch.equal(step, again[0]), torch.equal(ext, again[1])])
                if case in SV.SLOT_CASES:
                    zs = _step_all(_open(enc, case, True), x, mask, 0, T)
                    ze = _extend_all(_open(enc, case, True), x, mask, SV.GROUPS[T], slots=True)
                    out[key + "slots"] = np.array([torch.equal(step, zs), torch.equal(ext, ze)])
                if case in SV.PREFILL_CASES:
                    s = _open(enc, case)
                    P = SV.PREFILL
                    rows = [s.prefill(x[:, :P].contiguous(), mask[:, :P].contiguous()), _extend_all(s, x, mask, SV.PREFILL_GROUPS, P)]
                    t = P + sum(SV.PREFILL_GROUPS)
                    assert s.t == t
                    rows.append(_step_all(s, x, mask, t, T))
                    out[key + "prefill"] = torch.cat(rows, dim=1).cpu().numpy()


def _band_section(F, dev, out):
    h, B = SV.BAND_H, SV.BAND_B
    for case in BAND_CASES:
        regime, T, span, dk, j0 = case
        q, k, v, g, mask = SV.band_inputs(case)
        for p in MODES:
            key = "band:%s:p%g:" % (SV.band_id(case), p)
            leaves = [t.to(dev).requires_grad_() for t in (q, k, v)]
            y = F.sdpa(*leaves, mask.to(dev), h, dropout_p=p, seed=_seed(case, p), causal=True, span=span)
            y.backward(g.to(dev))
            for n, t in zip(("y", "dq", "dk", "dv"), [y.detach()] + [t.grad for t in leaves]):
                out[key + n] = t.cpu().numpy()
            if p > 0:
                Tp = -(-T // 32) * 32
                keep, sc = F.dropout_mask(p, _seed(case, p), 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
                out[key + "keep"] = keep.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu().numpy()
                out[key + "scale"] = np.array(sc)
    for case in PROBS_CASES:
        regime, T, span, dk, j0 = case
        q, k, v, g, mask = SV.band_inputs(case)
        out["probs:" + SV.band_id(case)] = F.attn_probs(q.to(dev), k.to(dev), mask.to(dev), h, causal=True, span=span).cpu().numpy()


def _rec_stream(m, case, dev, slots):
    """the family's functional layer as a stream (the _Fn of its own stream test), host-t or positioned; MFN: the gate's stream"""
    fam, sh, regime = case
    T, B = SV.REC_T[regime], SV.REC_B
    p = SV.rec_params(case)
    if fam == "lstm":
        import test_gpu_lstm_stream as G
        return G._Fn(sh + (B, T), G._device_params(p, dev), dev, slots=slots)
    if fam == "dec":
        import test_gpu_decoder_stream as G
        return G._Fn(sh + (B, T), G._device_params(p, dev), dev, slots=slots)
    if fam in ("ed", "ar"):
        import test_gpu_lstm_feedback_stream as G
        c = sh + (B, T) if fam == "ed" else sh[:5] + (B, T, sh[5])
        return G._Fn(fam, c, G._device_params(fam, p, dev), dev, slots=slots)
    gate = m.multiTransformer.MFN(SV.MFN_MODS, dict(zip(SV.MFN_MODS, SV.MFN_WIDTHS)), 1, device=dev)
    assert R.shapes_of(gate.state_dict()) == SV.mfn_shapes()
    gate.load_state_dict({k: v.float() for k, v in p.items()})
    gate = gate.eval()
    if slots:
        s = gate.slot_stream(B)
        s.reset()
        return s
    return gate.stream(B)


def _rec_record(s, case, x, mask):
    T = SV.REC_T[case[2]]
    if case[0] == "mfn":
        return torch.stack([s.step({k: v[t] for k, v in x.items()}, mask[:, t].reshape(-1, 1).contiguous()) for t in range(T)], dim=1)
    return torch.stack([s.step(x[:, t].contiguous(), mask[:, t].contiguous()) for t in range(T)], dim=1)


def _rec_section(m, dev, out):
    for case in REC_CASES:
        x, mask = SV.rec_inputs(case)
        x = {k: v.to(dev) for k, v in x.items()} if case[0] == "mfn" else x.to(dev)
        mask = mask.to(dev)
        y = _rec_record(_rec_stream(m, case, dev, False), case, x, mask)
        out["rec:%s:y" % SV.rec_id(case)] = y.cpu().numpy()
        if case[2] == "overflow":                                # one slots run per family
            out["rec:%s:slots" % SV.rec_id(case)] = np.array([torch.equal(y, _rec_record(_rec_stream(m, case, dev, True), case, x, mask))])


def child_main(kind, out_path, payload_json):
    """kind "enc": part A; "band": part B; "rec": part C"""
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import functional as F
    dev = torch.device("cuda:0")
    out = {}
    with torch.no_grad():
        if kind == "enc":
            _enc_section(m.multiTransformer, dev, out)
        elif kind == "rec":
            _rec_section(m, dev, out)
    if kind == "band":
        _band_section(F, dev, out)
    torch.cuda.synchronize()
    F.check_device_errors()
    np.savez(out_path, **out)


def _run(kind, tmp_dir):
    return run_child(__name__, kind, "default", None, tmp_dir, _SWITCHES, timeout={"enc": 240, "band": 180, "rec": 180}[kind])


def _widen(default, yard):
    return default if yard is None else tuple(max(d, 4 * y) for d, y in zip(default, yard))


def _finish(failures):
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ part A: encoder streams
_ENC_REFS = {}


def _enc_ref(case, flat=False):
    if (case, flat) not in _ENC_REFS:
        _ENC_REFS[(case, flat)] = SV.enc_reference(case, flat)
    return _ENC_REFS[(case, flat)]


def enc_bounds(case):
    return _widen((ENC_OUT, ENC_OUT_ROW), SC.STREAM_YARD.get(SV.enc_family(case)))


@pytest.mark.parametrize("case", ENC_CASES, ids=ENC_IDS)
def test_stepped_stream_against_its_reference(tmp_dir, case):
    """every row of the stepped stream (plain: encoder_step_kernel; ring: encoder_step_ring_kernel) against stream_ref /
    ring_stream_ref under ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3 (peaked at d = 128: 8e-3 -> 1.0e-2 per row, from the float32 yardstick
    2.6e-3); all rows finite; the flat twin of a step case likewise.
    Measured worst on the MI355X (rel-L2 / per row): cold, hot 2.8e-4 / 9.9e-4 (the N = 2 stack; N = 1: 1.9e-4 / 8.3e-4); step_up,
    step_down and their flat twins 1.8e-4 / 8.5e-4; newest, oldest 5.2e-5 / 8.0e-4 (newest at d 40 and d 256: 1e-7, no rounding tips);
    peaked 1.1e-4 / 1.3e-3 (d 128, against 2e-3 / 1.0e-2)."""
    run = _run("enc", tmp_dir)
    key = "enc:%s:" % SV.enc_id(case)
    rel, row = enc_bounds(case)
    failures = []
    check("svr step %s" % SV.enc_id(case), run[key + "step"], _enc_ref(case), rel, row, failures=failures)
    if SV.has_flat(case):
        check("svr step %s flat" % SV.enc_id(case), run[key + "flat:step"], _enc_ref(case, True), rel, row, failures=failures)
    _finish(failures)


@pytest.mark.parametrize("case", ENC_CASES, ids=ENC_IDS)
def test_extend_against_its_reference_and_the_stepped_stream(tmp_dir, case):
    """extend in the groupings of tests/test_gpu_stream_extend.py ([7, 16, 30, 17] at T = 70: a tile boundary and j0 = 40 fall inside
    a call; [5, 64, 61] at T = 130) against the reference under the same bounds, and against the stepped stream under twice those.
    Measured worst on the MI355X: against the reference 2.9e-4 / 9.9e-4 (the N = 2 cold stack), peaked d 128 1.1e-4 / 1.3e-3; against
    the stepped stream 9.0e-5 / 7.1e-4 (oldest d 256 span 16 / step_down d 256 span 5), 6e-8 / 2e-7 where no rounding tips."""
    run = _run("enc", tmp_dir)
    key = "enc:%s:" % SV.enc_id(case)
    rel, row = enc_bounds(case)
    failures = []
    check("svr extend %s" % SV.enc_id(case), run[key + "ext"], _enc_ref(case), rel, row, failures=failures)
    check("svr extend %s vs stepped" % SV.enc_id(case), run[key + "ext"], run[key + "step"], 2 * rel, 2 * row, failures=failures)
    if SV.has_flat(case):
        check("svr extend %s flat" % SV.enc_id(case), run[key + "flat:ext"], _enc_ref(case, True), rel, row, failures=failures)
    _finish(failures)


@pytest.mark.parametrize("case", FLAT_CASES, ids=[SV.enc_id(c) for c in FLAT_CASES])
def test_rows_that_see_no_hot_key_have_the_flat_inputs_bits(tmp_dir, case):
    """N = 1, so a row depends only on its visible windows: under step_up the rows t < j0 (plain and ring; step and extend, where the
    hot keys sit above the diagonal of the same tile), under step_down the ring rows t >= j0 + span - 1 (step and extend; the hot key
    t - span is in the ring row that step t writes over) have the bits of the same rows under c_j = 0 with the same parameters; the
    other rows differ."""
    run = _run("enc", tmp_dir)
    key = "enc:%s:" % SV.enc_id(case)
    rows = SC._hazard_rows(case)[0].numpy()
    for form in ("step", "ext"):
        got, flat = run[key + form], run[key + "flat:" + form]
        assert np.isfinite(got).all() and np.isfinite(flat).all()
        assert np.array_equal(got[:, rows], flat[:, rows]), form
        assert not np.array_equal(got[:, ~rows], flat[:, ~rows]), form


@pytest.mark.parametrize("case", ENC_CASES, ids=ENC_IDS)
def test_two_stream_runs_give_the_same_bits(tmp_dir, case):
    same = _run("enc", tmp_dir)["enc:%s:same" % SV.enc_id(case)]
    assert same.all(), same


@pytest.mark.parametrize("case", SV.SLOT_CASES, ids=[SV.enc_id(c) for c in SV.SLOT_CASES])
def test_slots_forms_have_the_host_forms_bits(tmp_dir, case):
    """the positioned step and extend bodies (plain: step_up; ring: step_down), every slot seated at 0: the host forms' bits"""
    same = _run("enc", tmp_dir)["enc:%s:slots" % SV.enc_id(case)]
    assert same.all(), same


@pytest.mark.parametrize("case", SV.PREFILL_CASES, ids=[SV.enc_id(c) for c in SV.PREFILL_CASES])
def test_prefill_then_extend_then_step(tmp_dir, case):
    """prefill(10), extend [16, 30], steps to T = 70 against prefill_ref under the same bounds; the stepped rows behind on their own.
    Measured on the MI355X: cold 1.3e-4 / 5.7e-4, step_up 1.5e-4 / 5.4e-4."""
    got = _run("enc", tmp_dir)["enc:%s:prefill" % SV.enc_id(case)]
    want = SV.prefill_reference(case)
    rel, row = enc_bounds(case)
    t = SV.PREFILL + sum(SV.PREFILL_GROUPS)
    failures = []
    check("svr prefill walk %s" % SV.enc_id(case), got, want, rel, row, failures=failures)
    check("svr prefill walk %s: the stepped rows behind" % SV.enc_id(case), got[:, t:], want[:, t:], rel, row, failures=failures)
    _finish(failures)


# ------------------------------------------------------------------------------------------------ part B: the band's lower edge
def band_bounds(case, tensor):
    default = (SDPA_OUT, SDPA_OUT_ROW) if tensor == "y" else (SDPA_GRAD, SDPA_GRAD_ROW)
    return _widen(default, SC.BAND_YARD.get(SV.band_family(case), {}).get(tensor))


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", BAND_CASES, ids=BAND_IDS)
def test_band_sdpa(tmp_dir, case, p):
    """y, dq, dk, dv of sdpa(causal=True, span=s) against band_ref.sdpa in fp64 under autograd, eval mode and p = 0.1 (the keep mask
    from F.dropout_mask): finite, inside the bounds, dq exactly 0 on blanked rows.
    Measured worst on the MI355X per family (rel-L2 / per row; the bound is the imported 4e-4 / 1e-2 for y and 2e-3 / 2e-2 for the
    gradients, or 4x test_stream_value_regimes_cpu.BAND_YARD where that is wider):
      step_down  d_k 16: y 9.2e-5 / 1.1e-3, dq 3.5e-3 / 8.2e-2, dk 4.2e-4 / 1.0e-2, dv 6.0e-4 / 1.4e-2;
                 d_k 64: y 2.9e-4 / 4.9e-3, dq 1.4e-2 / 1.5e-1, dk 1.8e-3 / 2.5e-2, dv 8.2e-4 / 1.3e-2
      falling, rising  d_k 16: y 2.0e-4 / 3.2e-3, dq 9.8e-4 / 1.9e-2, dk 6.7e-4 / 1.4e-2, dv 1.7e-4 / 2.5e-3;
                 d_k 64: y 2.5e-4 / 3.1e-3, dq 1.6e-3 / 2.5e-2, dk 7.1e-4 / 1.4e-2, dv 2.5e-4 / 4.8e-3
      peaked     y 3.3e-5 / 7.9e-4, gradients 2.7e-4 / 6.5e-3
      cold       d_k 64: y 2.5e-4 / 2.5e-3, dq 1.1e-2 / 1.0e-1, dk 1.7e-3 / 3.2e-2, dv 9.7e-4 / 1.0e-2
    Everything sits at or below its yardstick (dq of step_down at d_k 16: 8.2e-2 per row against a yardstick of 8.7e-2)."""
    regime, T, span, dk, j0 = case
    run = _run("band", tmp_dir)
    key = "band:%s:p%g:" % (SV.band_id(case), p)
    drop = torch.from_numpy(run[key + "keep"]).double() * float(run[key + "scale"]) if p else None
    ref = SV.band_reference(case, drop)
    got = {n: run[key + n] for n in ("y", "dq", "dk", "dv")}
    tag = "svr band %s p%g" % (SV.band_id(case), p)
    failures = []
    for n in got:
        if not np.isfinite(got[n]).all():
            failures.append("%s %s: %d entries are not finite" % (tag, n, int((~np.isfinite(got[n])).sum())))
    for b, n in enumerate(V.attn_lengths(T)):
        if (got["dq"][b, n:] != 0).any():
            failures.append("%s: dq on the blanked rows of sequence %d" % (tag, b))
    for n in got:
        rel, row = band_bounds(case, n)
        check("%s %s" % (tag, n), np.nan_to_num(got[n].astype(np.float64)), ref[n], rel, row, scale_ref=V.zero_scale(ref, n), failures=failures)
    _finish(failures)


@pytest.mark.parametrize("case", PROBS_CASES, ids=[SV.band_id(c) for c in PROBS_CASES])
def test_band_attn_probs(tmp_dir, case):
    """the materialised band map against the fp64 softmax of the bf16 operands over the band; exact zeros outside the band; rows sum
    to 1 within 1e-5.  Measured on the MI355X: 2.0e-5 / 8.9e-5 (cold, d_k 64); row sums within 2.0e-7."""
    regime, T, span, dk, j0 = case
    P = _run("band", tmp_dir)["probs:" + SV.band_id(case)]
    ref = SV.band_probs_reference(case).numpy()
    outside = Bn.outside_band(T, span).expand(SV.BAND_B, SV.BAND_H, -1, -1).numpy()
    assert np.isfinite(P).all() and (P >= 0).all()
    assert (P[outside] == 0).all()
    err = float(np.abs(P.astype(np.float64).sum(axis=-1) - 1.0).max())
    print("svr band probs %s row-sum error %.2e" % (SV.band_id(case), err))
    assert err <= 1e-5
    rel, row = band_bounds(case, "y")
    check("svr band probs %s" % SV.band_id(case), P.reshape(-1, T), ref.reshape(-1, T), rel, row)


# ------------------------------------------------------------------------------------------------ part C: the recurrent steps
_REC_DEFAULT = {"lstm": (LSTM_STEP_OUT, LSTM_STEP_ROW), "dec": (DEC_STEP_OUT, DEC_STEP_ROW), "ed": (FB_STEP_OUT, FB_STEP_ROW),
                "ar": (AR_STEP_OUT, AR_STEP_ROW), "mfn": (MFN_STEP_OUT, MFN_STEP_ROW)}
_REC_REFS = {}


def rec_bounds(case):
    """(rel-L2, per-row maximum) of the case: its family's every-case pair, or 4x the recorded yardstick where that is wider"""
    yard = SC.REC_YARD.get(SV.rec_id(case))
    return _widen(_REC_DEFAULT[case[0]], None if yard is None else yard[:2])


@pytest.mark.parametrize("case", REC_CASES, ids=REC_IDS)
def test_recurrent_step_against_its_reference(tmp_dir, case):
    """every window of the host-t step kernel against the family's stepped reference (rounding on); long_memory also per time step
    (value_regimes.per_step) under 4x its yardstick or the per-row bound, whichever is wider; blanked windows exact zeros.
    Measured on the MI355X (rel-L2 / per row; long_memory: then per step), bound in brackets where a yardstick widens it:
      lstm (12, 12, 20)  overflow 3.4e-8 / 3.7e-8, long_memory 5.5e-6 / 8.9e-5, 6.3e-5 [1.9e-3 / 1.8e-2], peaked 2.3e-8 / 4.6e-8
      lstm (16, 8, 8, 2 layers)  4.8e-8 / 5.8e-8, 1.9e-8 / 2.2e-8, 2.2e-8, 0 / 0
      decoder (40, 128, 1)  overflow 7.2e-8 / 2.0e-7, long_memory 4.7e-8 / 1.5e-7, 1.1e-7 (DEC_STEP_OUT 1.4e-7 / DEC_STEP_ROW 3.4e-7)
      decoder (128, 128, 2)  overflow 1.8e-7 / 7.4e-7 [5.6e-3 / 2.1e-2], long_memory 5.2e-3 / 2.1e-2, 1.5e-2 [8.0e-2 / 4.4e-1]
      ed  5.5e-8 / 1.1e-7, 5.3e-8 / 2.2e-7, 1.6e-7, 3.1e-8 / 8.1e-8;  ar  5.1e-8 / 1.5e-7, 6.6e-8 / 2.4e-7, 1.8e-7, 5.9e-8 / 1.3e-7
      mfn  overflow 6.3e-8 / 1.5e-7, long_memory 5.1e-4 / 4.3e-3, 3.0e-3 [3.2e-3 / 2.2e-2], peaked 3.6e-8 / 6.9e-8 [4.0e-3 / 1.7e-2]"""
    fam, sh, regime = case
    run = _run("rec", tmp_dir)
    if case not in _REC_REFS:
        _REC_REFS[case] = SV.rec_reference(case)
    got, ref = run["rec:%s:y" % SV.rec_id(case)], _REC_REFS[case]
    rel, row = rec_bounds(case)
    tag = "svr %s" % SV.rec_id(case)
    failures = []
    check(tag, got, ref, rel, row, failures=failures)
    if regime == "long_memory":
        yard = SC.REC_YARD.get(SV.rec_id(case))
        s, bound = V.per_step(got.transpose(1, 0, 2), ref.transpose(1, 0, 2)), max(4 * (yard[2] if yard else 0.0), row)
        print("%-52s per-step %.2e (bound %.1e)" % (tag, s, bound))
        if not s <= bound:
            failures.append("%s: per-step maximum %.3e > %.1e" % (tag, s, bound))
    mask = SV.rec_inputs(case)[1].numpy()
    if (got[mask == 0] != 0).any():
        failures.append("%s: a blanked window is not an exact zero" % tag)
    _finish(failures)


@pytest.mark.parametrize("case", [c for c in REC_CASES if c[2] == "overflow"], ids=[SV.rec_id(c) for c in REC_CASES if c[2] == "overflow"])
def test_recurrent_slots_forms_have_the_host_forms_bits(tmp_dir, case):
    assert _run("rec", tmp_dir)["rec:%s:slots" % SV.rec_id(case)].all()
