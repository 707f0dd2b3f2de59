"""GPU: the LSTM baselines one window at a time (csrc/lstm_step.h lstm_step_kernel / lstm_step_slots_kernel, mmt_lstm_stream_*,
functional.lstm_stream_*, streaming.LSTMStream / LSTMSlotStream, and stream / slot_stream of MultiLSTM, MultiLSTMB1 and MultiCNNLSTM).

The reference is tests/lstm_stream_ref.py (tests/test_lstm_stream_cpu.py holds its stepped form to its batch form, that to the restated
model in fp64 and, rounded, to the batch composition of bf16_ref's pieces: one function serves the step and the batch path).  What is
left between the kernel and it is fp32 summation order, the hardware exp2 / reciprocal of the activations, expf of the softmax, and the
few bf16 roundings that this noise tips.  The bounds are the measured worst values on the MI355X times about 3 (the project's
practice, see tests/test_gpu_decoder_stream.py), and every case is also held under D, the distance that the rounding itself moves the
reference of that case (computed here).  Everything between two runs of the new kernels carries NO tolerance: the positioned form
against the host-t form, a recording again, a sequence alone, any contents of the state, a replayed graph.
"""
import pytest
import torch

import lstm_stream_ref as LS
import recipe as R
from gpu_harness import (FILLS, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named, measures, mta,  # noqa: F401
                         same_bits)

pytestmark = pytest.mark.gpu

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# (in, E, H, layers, taps, B, steps)
CASES = [(8, 8, 4, 1, 1, 1, 1),                 # position 0 only, one tap
         (12, 12, 20, 1, 3, 3, 5),              # k padded to 8, ring wraps
         (300, 128, 256, 1, 5, 3, 12),          # the checkpoint's configuration, ring wraps twice; the mask has a hole
         (40, 64, 32, 4, 16, 2, 4),             # deepest stack, most taps, every step has taps reaching before 0
         (1556, 512, 256, 1, 5, 2, 3),          # B1's widths, 1024 gate rows
         (2048, 512, 512, 1, 16, 1, 2),         # the limits; reference only (the batch path does not take H = 512)
         (16, 8, 8, 2, 3, 33, 4)]               # 33 workgroups
IDS = ["in%d_E%d_H%d_N%d_L%d_B%d_T%d" % c for c in CASES]
HOLE = CASES[2]

# rel-L2 / per-row maximum of the host-t form against lstm_stream_ref.stepped (rounding on).  Measured worst over CASES on the MI355X:
# 6.44e-4 / 1.58e-3, both in the B1 case (in 1556), and there because of ONE tipped bf16 rounding: element 339 of the embed row of
# (b = 1, t = 1) is 0.2822266 in the kernel's fp32 summation order, exactly the midpoint of the bf16 neighbours 0.28125 and 0.283203125
# (ties to even: up), and 0.28222647 in fp64 (down).  Found by restating step_matvec's order (one thread, k ascending, fma) in numpy on
# the CPU: that is the only one of the case's 3072 embed values that the two orders round differently, and the reference with that one
# value rounded up lies 6.441e-4 / 1.578e-3 from the reference, all of it in row (1, 1): the measured distance to the digit.  Every other case has no visible tip: worst 2.83e-7 (in 2048) / 7.92e-7 (B 33), fp32 summation order, the
# hardware exp2 / reciprocal and expf only.  So there are two pairs of bounds.  LSTM_STEP_OUT / _ROW hold for every case: the measured
# worst x 3.0 = 1.9e-3 for the rel-L2, under the smallest D of a case (2.6e-3, in 300); per row x 3 = 4.7e-3 would not fit under the
# smallest D (4.26e-3, in 2048), so it takes the largest margin that does, x 2.7.  LSTM_STEP_CLEAN / _ROW, x 3.0 of the worst of the
# other six cases, hold for those: three orders under what a missing rounding site moves (about D).
# THESE BOUNDS HOLD FOR THESE DETERMINISTIC INPUTS ONLY (recipe's generators, fixed tags and seeds), for the reason written beside
# DEC_STEP_OUT in tests/test_gpu_decoder_stream.py: inputs, seeds or a summation order changed here will sooner or later meet another
# tip that shows; the failure then reads three orders outside the clean bounds in ONE sequence's rows, which is a new measurement to
# make, not a missing rounding site (that moves every row).
LSTM_STEP_OUT, LSTM_STEP_ROW = 1.9e-3, 4.2e-3
LSTM_STEP_CLEAN, LSTM_STEP_CLEAN_ROW = 8.5e-7, 2.4e-6
TIPPED = CASES[4]
# stream() against the model's own eval batch forward (attend_over_taps on), in lockstep on SHORT recordings (8 windows, 5 behind the
# window encoder), for the reason given beside DEC_STEP_VS_STREAM in tests/test_gpu_decoder_stream.py: the two routes have the same
# rounding sites and differ by fp32 summation order, which now and then tips a bf16 rounding of a carried h, and a recurrence carries a
# tipped rounding on.  Measured on the MI355X: MultiLSTM (300 wide) 9.31e-8 / 2.21e-7; the two-layer B1-shaped model, the wrapper and
# every recording of the refresh test exactly 0.  x 3.0 of the worst; no tip shows in these recordings.
LSTM_LOCKSTEP, LSTM_LOCKSTEP_ROW = 2.8e-7, 6.6e-7
_CACHE = {}


def _mask(c):
    B, T = c[5], c[6]
    mask = R.prefix_mask([max(1, T - b % T) for b in range(B)], T).reshape(B, T)
    if c == HOLE:
        mask[0, 4] = 0.0                                     # a blanked window inside a recording: the ring holds m_t * h_t
    return mask


def _device_params(p, dev):
    """(embed, attn, lstm, dec) of lstm_stream_prepare from the reference's parameters, fp32 on the device"""
    g = {k: v.float().to(dev) for k, v in p.items()}
    lstm = [[g["lstm.%s_l%d" % (n, l)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for l in range(LS.n_layers_of(p))]
    return ([g["embed.1.weight"], g["embed.1.bias"]], [g["attn.0.weight"], g["attn.0.bias"], g["attn.2.weight"], g["attn.2.bias"]], lstm,
            [g["decoder.0.weight"], g["decoder.0.bias"], g["decoder.2.weight"], g["decoder.2.bias"]])


class _Fn:
    """the functional layer as a stream: host-t form (positions None) or positioned form"""

    def __init__(self, c, params, dev, slots=False, B=None, limit=None):
        self.F = mta().functional
        self.B, self.dims, self.limit = (c[5] if B is None else B), tuple(c[:5]), limit
        self.params = params
        self.state = self.F.lstm_stream_state(self.B, *self.dims, dev)
        self.positions = torch.zeros(self.B, dtype=torch.int32, device=dev) if slots else None
        self.t = 0
        self.refresh()

    def refresh(self):
        self.F.lstm_stream_prepare(*self.params, self.state, self.B, *self.dims)

    def reset(self):
        self.t = 0
        if self.positions is not None:
            self.positions.zero_()

    def step(self, x, m, advance=True):
        if self.positions is not None:
            return self.F.lstm_stream_step_slots(x, m, self.state, self.positions, *self.dims, limit=self.limit, advance=advance)
        y = self.F.lstm_stream_step(x, m, self.state, self.t, *self.dims)
        self.t += 1
        return y


def _record(s, xg, mg):
    """every window through s.step, in order -> (B, T, 1) on the CPU"""
    return torch.stack([s.step(xg[:, t].contiguous(), mg[:, t].contiguous()) for t in range(xg.shape[1])], dim=1).cpu()


def _run(c, dev):
    """every GPU result and the CPU references of one case, computed once"""
    key = IDS[CASES.index(c)]
    if key in _CACHE:
        return _CACHE[key]
    I, E, H, NL, L, B, T = c
    p = LS.params(I, E, H, NL, L, tag="gpu_lstm_stream")
    x = R.gen_normal("gpu_lstm_stream:x:%d:%d" % (I, T), (B, T, I), 11)
    mask = _mask(c)
    xg, mg = x.to(dev), mask.to(dev)
    params = _device_params(p, dev)
    out = {"params": params, "x": xg, "mask": mg}
    s = _Fn(c, params, dev)
    out["host"] = _record(s, xg, mg)
    s.reset()
    out["after_reset"] = _record(s, xg, mg)                                      # nothing was cleared or re-read
    out["again"] = _record(_Fn(c, params, dev), xg, mg)
    z = _Fn(c, params, dev, slots=True)
    out["slots"] = _record(z, xg, mg)
    out["slots_pos"] = z.positions.cpu().tolist()
    z.reset()                                                                    # re-seating: pos = 0 and nothing else
    out["slots_reseated"] = _record(z, xg, mg)
    torch.cuda.synchronize()
    out["ref"] = LS.stepped(p, x.double(), mask.double()).numpy()
    out["exact"] = LS.stepped(p, x.double(), mask.double(), rounding=False).numpy()
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_step_against_the_stream_reference(dev, c):
    """all rows of the host-t kernel against lstm_stream_ref.stepped (rounding on) under LSTM_STEP_OUT / LSTM_STEP_ROW, and under D, what
    the rounding itself moves this case's reference by (printed); the cases without a tipped rounding also under LSTM_STEP_CLEAN /
    LSTM_STEP_CLEAN_ROW.  Measured (rel-L2 / per row, then D / D per row): in8 0 / 0, 1.7e-2 / 1.7e-2; in12 4.6e-8 / 1.8e-7, 1.5e-2 /
    3.1e-2; in300 6.5e-8 / 1.3e-7, 2.6e-3 / 5.8e-3; in40 N4 1.4e-7 / 3.0e-7, 9.1e-3 / 2.0e-2; in1556 6.44e-4 / 1.58e-3 (one tipped
    embed value, see the bounds' comment), 3.4e-3 / 7.8e-3; in2048 2.8e-7 / 3.2e-7, 3.0e-3 / 4.3e-3; B33 2.2e-7 / 7.9e-7, 2.3e-2 / 7.4e-2."""
    r = _run(c, dev)
    tag = IDS[CASES.index(c)]
    Dd, D_row = measures(r["ref"], r["exact"])
    print("lstm step %s: rounding on vs off rel-L2 %.3e per-row %.3e" % (tag, Dd, D_row))
    assert Dd > 1e-4                                               # the reference rounds
    check("lstm step %s y" % tag, r["host"], r["ref"], min(LSTM_STEP_OUT, Dd), min(LSTM_STEP_ROW, D_row))
    if c != TIPPED:
        check("lstm step %s y (no tipped rounding)" % tag, r["host"], r["ref"], LSTM_STEP_CLEAN, LSTM_STEP_CLEAN_ROW)
    mask = r["mask"].cpu().unsqueeze(-1)
    assert (r["host"][mask == 0] == 0).all()                       # a blanked window is an exact zero
    assert r["host"].shape == (c[5], c[6], 1)


# ------------------------------------------------------------------------------------------------ 2. exact facts, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_positioned_form_has_the_bits_of_the_host_t_form(dev, c):
    """every slot seated at call 0: every step of lstm_step_slots_kernel against lstm_step_kernel; a second recording, a reset and a
    re-seated slot give the same bits again"""
    r = _run(c, dev)
    failures = []
    same_bits("positioned form", {"y": r["slots"]}, {"y": r["host"]}, failures)
    same_bits("a second, fresh stream", {"y": r["again"]}, {"y": r["host"]}, failures)
    same_bits("the same stream after reset()", {"y": r["after_reset"]}, {"y": r["host"]}, failures)
    same_bits("re-seated slots", {"y": r["slots_reseated"]}, {"y": r["host"]}, failures)
    assert not failures, failures
    assert r["slots_pos"] == [c[6]] * c[5]


@pytest.mark.parametrize("c", [c for c in CASES if c[5] > 1], ids=[i for i, c in zip(IDS, CASES) if c[5] > 1])
def test_a_sequence_does_not_depend_on_its_batch(dev, c):
    """the last sequence stepped alone (B = 1) has the bits of its row in the whole batch: one workgroup per sequence, nothing shared"""
    r = _run(c, dev)
    b = c[5] - 1
    alone = _record(_Fn(c, r["params"], dev, B=1), r["x"][b:b + 1], r["mask"][b:b + 1])
    failures = []
    same_bits("sequence %d alone" % b, {"y": alone[0]}, {"y": r["host"][b]}, failures)
    assert not failures, failures
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_state_may_hold_any_contents(dev, c, fill):
    """the whole state (both copies of (h, c) and the ring with it) filled with each pattern before step 0, the parameters prepared
    afterwards: the same bits.  Step 0 reads no dynamic state, and a later step only what the steps before it wrote."""
    r = _run(c, dev)
    s = _Fn(c, r["params"], dev, slots=True)
    before = s.state.clone()
    fill_bytes(s.state.view(-1), fill)
    assert not torch.equal(before, s.state)
    s.refresh()
    failures = []
    same_bits("state filled with %s" % fill, {"y": _record(s, r["x"], r["mask"])}, {"y": r["host"]}, failures)
    assert not failures, failures
    torch.cuda.synchronize()


def test_idle_and_full_slots_give_zero_rows_and_are_not_touched(dev):
    """limit 4, positions [0, -1, INT_MIN, limit, limit + 1, INT_MAX]: slot 0 gives its batch-1 row and advances; every other slot gives
    a zero row and keeps its position.  With every slot idle or full, the state and the positions are bit-identical before and after.
    advance=False leaves a seated slot where it is."""
    c, lim = CASES[1], 4
    r = _run(c, dev)
    edge = [0, -1, INT_MIN, lim, lim + 1, INT_MAX]
    x = R.gen_normal("gpu_lstm_stream:edge", (6, c[0]), 5).to(dev)
    z = _Fn(c, r["params"], dev, slots=True, B=6, limit=lim)
    z.positions.copy_(torch.tensor(edge, dtype=torch.int32))
    y = z.step(x, None)
    assert z.positions.cpu().tolist() == [1] + edge[1:]
    one = _Fn(c, r["params"], dev, B=1)
    assert (y[1:] == 0).all() and torch.equal(y[0], one.step(x[:1].contiguous(), None)[0]) and y[0].abs().max() > 0
    z.positions.copy_(torch.tensor([-1, INT_MIN, lim, lim + 1, INT_MAX, -7], dtype=torch.int32))
    before, pos = z.state.clone(), z.positions.cpu().tolist()
    y = z.step(x, None)
    assert (y == 0).all() and torch.equal(z.state, before) and z.positions.cpu().tolist() == pos
    z.positions[2] = 0
    y0 = z.step(x, None, advance=False)
    assert z.positions.cpu().tolist()[2] == 0
    y1 = z.step(x, None)
    assert z.positions.cpu().tolist()[2] == 1 and torch.equal(y0, y1) and y1[2].abs().max() > 0
    torch.cuda.synchronize()


def test_seat_and_release_mid_recording(dev):
    """MultiLSTM's slot_stream, B = 3, limit 9: slot 0 seated at call 0, slot 1 at call 2, slot 1 released at call 5 and seated again at
    call 6 with another recording (over the (h, c) and the ring the first one left), slot 2 never seated.  The slots stand at different
    positions in every call; each seated row is, bit for bit, that recording stepped alone in a batch-1 stream, every other row zero."""
    MM = mta().models
    model = MM.MultiLSTM(24, embed_dim=16, h_dim=12, n_layers=2, attn_len=4, device=dev)
    load_named(model, 17)
    MM.attend_over_taps(model)
    model.eval()
    calls, lim = 11, 9
    recs = {r: R.gen_normal("gpu_lstm_stream:seat%d" % r, (calls, 24), 5).to(dev) for r in range(3)}
    sched = {0: [("seat", 0, 0)], 2: [("seat", 1, 1)], 5: [("release", 1, None)], 6: [("seat", 1, 2)]}
    z = model.slot_stream(3, lim)
    assert z.slots is True and z.capacity == lim and z.positions.cpu().tolist() == [-1] * 3
    with pytest.raises(AttributeError, match=r"\.positions"):
        z.t
    seated, window, rows, cells = {}, {}, [], []
    for call in range(calls):
        for what, slot, rec in sched.get(call, []):
            if what == "seat":
                z.seat([slot])
                seated[slot], window[slot] = rec, 0
            else:
                z.release([slot])
                seated.pop(slot)
        live = {s: (rec, window[s]) for s, rec in seated.items() if window[s] < lim}
        want_pos = [window[s] if s in seated else -1 for s in range(3)]
        assert z.positions.cpu().tolist() == want_pos, (call, want_pos)
        x = torch.stack([recs[live[s][0]][live[s][1]] if s in live else torch.full((24,), 3.0, device=dev) for s in range(3)])
        rows.append(z.step(x))
        cells.append(live)
        for s in live:
            window[s] += 1
    got = torch.stack(rows).cpu()
    assert z.positions.cpu().tolist() == [9, 5, -1] and z.full().cpu().tolist() == [True, False, False]
    assert any(len(set(w for _, w in live.values())) > 1 for live in cells)              # slots at different positions in one call
    alone = {}
    for rec in range(3):
        s = model.stream(1)
        alone[rec] = torch.stack([s.step(recs[rec][t:t + 1]) for t in range(lim)]).cpu().reshape(lim, 1)
    for call, live in enumerate(cells):
        for s in range(3):
            if s in live:
                assert torch.equal(got[call, s], alone[live[s][0]][live[s][1]]), (call, s, live[s])
            else:
                assert (got[call, s] == 0).all(), (call, s)
    assert cells[9].get(0) is None and cells[8][0] == (0, 8) and cells[6][1] == (2, 0)   # slot 0 full from call 9 on
    torch.cuda.synchronize()


def test_replays_have_the_bits_of_the_eager_slot_stream(dev):
    """graphs.capture_stream on MultiLSTM's slot_stream, unchanged: capturing leaves the state and the positions bit-identical; replays
    fed through copy_ equal the eager stream; a slot seated between two replays starts its recording; a full slot gives a zero row"""
    from multimodal_transformer_amd import graphs
    MM = mta().models
    model = MM.MultiLSTM(24, embed_dim=16, h_dim=12, attn_len=4, device=dev)
    load_named(model, 19)
    MM.attend_over_taps(model)
    model.eval()
    B, T, lim = 3, 9, 20
    x = R.gen_normal("gpu_lstm_stream:graph", (B, T, 24), 5).to(dev)
    mask = R.prefix_mask([9, 5, 1], T).to(dev)
    z, e = model.slot_stream(B, lim), model.slot_stream(B, lim)
    z.seat([1])
    z.step(x[:, 0].contiguous(), mask[:, 0].contiguous())                                # a carried state and a position for the capture to leave alone
    before, pos = z.state.clone(), z.positions.cpu().tolist()
    assert pos == [-1, 1, -1]
    g = graphs.capture_stream(z, x[:, 0], mask[:, 0])
    assert torch.equal(z.state, before) and z.positions.cpu().tolist() == pos
    assert g.inputs.shape == (B, 24) and g.output.shape == (B, 1)
    z.reset(), e.reset()
    for t in range(7):
        g.inputs.copy_(x[:, t])
        g.mask.copy_(mask[:, t])
        assert torch.equal(g.replay(), e.step(x[:, t].contiguous(), mask[:, t].contiguous())), t
    assert z.positions.cpu().tolist() == e.positions.cpu().tolist() == [7] * B
    for s in (z, e):                                                                     # between two replays: seat slot 1 anew, fill slot 2
        s.seat([1])
        s.positions[2] = lim
    g.inputs.copy_(x[:, 7])
    g.mask.copy_(mask[:, 0])
    y = g.replay().clone()
    assert torch.equal(y, e.step(x[:, 7].contiguous(), mask[:, 0].contiguous()))
    assert (y[2] == 0).all() and y[0].abs().max() > 0
    one = model.stream(1)
    assert torch.equal(y[1], one.step(x[1:2, 7].contiguous(), mask[1:2, 0].contiguous())[0])      # window 0 of a new recording
    assert z.positions.cpu().tolist() == [8, 1, lim] and z.full().cpu().tolist() == [False, False, True]
    torch.cuda.synchronize()


def test_a_step_is_one_hand_written_launch(dev):
    """a warmed step of both functional forms and of both model streams: exactly one device kernel, the step kernel of that form, and no
    library kernel"""
    c = CASES[1]
    r = _run(c, dev)
    s, z = _Fn(c, r["params"], dev), _Fn(c, r["params"], dev, slots=True)
    x, m = r["x"][:, 0].contiguous(), r["mask"][:, 0].contiguous()
    MM = mta().models
    model = MM.MultiLSTM(24, embed_dim=16, h_dim=12, attn_len=4, device=dev)
    load_named(model, 19)
    MM.attend_over_taps(model)
    model.eval()
    ms, mz = model.stream(2), model.slot_stream(2)
    mz.reset()
    xm = R.gen_normal("gpu_lstm_stream:launch", (2, 24), 5).to(dev)
    torch.cuda.synchronize()
    names = [device_kernel_names(fn, warm=True)[1] for fn in (lambda: s.step(x, m), lambda: z.step(x, m), lambda: ms.step(xm), lambda: mz.step(xm))]
    torch.cuda.synchronize()
    if any(n is None for n in names):
        pytest.skip("torch.profiler reports no device kernels on this box")
    for got, want in zip(names, ("lstm_step_kernel", "lstm_step_slots_kernel", "lstm_step_kernel", "lstm_step_slots_kernel")):
        assert len(got) == 1 and want in got[0] and library_kernels(got) == [], (want, got)


# ------------------------------------------------------------------------------------------------ 3. the models
def _model(which, dev):
    MM = mta().models
    if which == "multilstm":
        model = MM.MultiLSTM(300, device=dev)                                            # E 128, H 256, L 5: the checkpoint's configuration
    else:
        model = MM.MultiLSTMB1(40, embed_dim=32, h_dim=16, n_layers=2, attn_len=5, device=dev)
    load_named(model, 13)
    MM.attend_over_taps(model)
    return model.eval()


@pytest.mark.parametrize("which", ["multilstm", "b1_two_layers"])
def test_model_stream_against_its_batch_forward(dev, which):
    """stream() rows of MultiLSTM (300-wide, three sequences, 8 windows) and of a two-layer MultiLSTMB1-shaped model at small widths,
    attend_over_taps on, against the rows of the model's own eval batch forward, under LSTM_LOCKSTEP / LSTM_LOCKSTEP_ROW; padded
    windows exact zeros; the slots form in bits; a second recording after reset() in bits.  Measured: multilstm 9.31e-8 / 2.21e-7,
    b1_two_layers 0 / 0."""
    model = _model(which, dev)
    width = model.embed[1].in_features
    T, lengths = 8, [8, 5, 1]
    x = R.gen_normal("gpu_lstm_stream:model:%s" % which, (3, T, width), 5).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, mask, lengths).cpu()
    s, z = model.stream(3), model.slot_stream(3)
    assert s.slots is False and s.t == 0 and s.capacity is None and z.capacity is None
    recs = []
    for rec in range(2):
        s.reset()
        recs.append(torch.stack([s.step(x[:, t].contiguous(), mask[:, t].contiguous()) for t in range(T)], dim=1).cpu())
    assert s.t == T
    z.reset()
    slots = torch.stack([z.step(x[:, t].contiguous(), mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
    got = recs[0]
    assert got.shape == want.shape == (3, T, 1) and torch.isfinite(got).all() and want.abs().max() > 0
    check("%s stream vs its batch forward" % which, got.numpy(), want.numpy(), LSTM_LOCKSTEP, LSTM_LOCKSTEP_ROW)
    for b, n in enumerate(lengths):
        assert (got[b, n:] == 0).all()
    assert torch.equal(recs[0], recs[1]) and torch.equal(slots, got) and z.positions.cpu().tolist() == [T] * 3
    torch.cuda.synchronize()


def test_wrapper_streams_against_its_batch_forward(dev):
    """the window encoder in front (T = 5, two modalities): MultiCNNLSTM.stream against the wrapper's own eval forward under the lockstep
    bound, its slot_stream against stream in bits.  Measured: 0 / 0."""
    MM = mta().models
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    T, lengths, W = 5, [5, 3], 3
    model = MM.MultiCNNLSTM(mods, dims, device=dev, lstm_cls=MM.MultiLSTM)
    model.LSTM = MM.MultiLSTM(model.LSTM.embed[1].in_features, embed_dim=32, h_dim=16, device=dev)
    load_named(model)
    MM.attend_over_taps(model)
    model.eval()
    x = {mod: R.gen_normal("gpu_lstm_stream_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, lengths, mask).cpu()
    s, z = model.stream(2), model.slot_stream(2)
    assert z.slots is True and z.capacity is None and s.capacity is None and s.t == 0
    with pytest.raises(AttributeError, match=r"\.positions"):
        z.t
    z.reset()
    a = torch.stack([s.step({mod: x[mod][:, t].contiguous() for mod in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
    b = torch.stack([z.step({mod: x[mod][:, t].contiguous() for mod in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
    assert a.shape == want.shape == (2, T, 1) and s.t == T and z.positions.cpu().tolist() == [T, T]
    check("MultiCNNLSTM stream vs its batch forward", a.numpy(), want.numpy(), LSTM_LOCKSTEP, LSTM_LOCKSTEP_ROW)
    assert torch.equal(a, b) and (a[1, 3:] == 0).all() and a.abs().max() > 0
    torch.cuda.synchronize()


def test_refresh_follows_the_parameters(dev):
    """every parameter the step reads is a copy in the state: a changed matrix or bias shows after refresh() only, and then as the batch
    forward shows it"""
    model = _model("b1_two_layers", dev)
    T = 3
    x = R.gen_normal("gpu_lstm_stream:refresh", (2, T, 40), 5).to(dev)
    mask = R.prefix_mask([3, 2], T).to(dev)
    z = model.slot_stream(2)

    def record():
        z.reset()
        return torch.stack([z.step(x[:, t].contiguous(), mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()

    a = record()
    for change in (lambda: model.embed[1].weight.mul_(0.5), lambda: model.attn[2].bias.add_(torch.arange(5.0, device=dev)),
                   lambda: model.lstm.weight_hh_l1.mul_(0.5), lambda: model.lstm.bias_ih_l0.add_(0.25),
                   lambda: model.decoder[0].weight.mul_(0.5), lambda: model.decoder[3].bias.add_(1.0)):
        with torch.no_grad():
            change()
        stale = record()
        z.refresh()
        fresh = record()
        with torch.no_grad():
            want = model(x, mask, [3, 2]).cpu()
        assert torch.equal(a, stale) and not torch.equal(a, fresh)
        check("after refresh()", fresh.numpy(), want.numpy(), LSTM_LOCKSTEP, LSTM_LOCKSTEP_ROW)
        a = fresh
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. refusals before any launch
def test_refusals_come_before_any_launch(dev):
    MM, F = mta().models, mta().functional
    model = _model("b1_two_layers", dev)
    off = MM.MultiLSTM(24, embed_dim=16, h_dim=12, device=dev).eval()
    ed = MM.MultiEDLSTM(24, embed_dim=16, h_dim=12, device=dev).eval()
    wrap = MM.MultiCNNLSTM(["emotient"], {"emotient": 8}, device=dev).eval()
    MM.attend_over_taps(ed)
    opened = model.slot_stream(2)
    st = F.lstm_stream_state(2, 40, 32, 16, 2, 5, dev)
    x = torch.zeros(2, 40, device=dev)
    small = torch.zeros(16, dtype=torch.uint8, device=dev)
    good = torch.zeros(2, dtype=torch.int32, device=dev)
    narrow, x64, xcpu, mask3, pos64 = x[:, :16].contiguous(), x.double(), x.cpu(), torch.ones(3, device=dev), good.long()
    torch.cuda.synchronize()
    calls = [(lambda: model.train().stream(2), ValueError, r"\.eval\(\)"),
             (lambda: model.train().slot_stream(2), ValueError, r"\.eval\(\)"),
             (lambda: off.stream(2), ValueError, r"attend_over_taps\(model\)"),
             (lambda: off.slot_stream(2), ValueError, r"attend_over_taps\(model\)"),
             (lambda: wrap.stream(2), ValueError, r"attend_over_taps\(model\)"),
             (lambda: wrap.train().slot_stream(2), ValueError, r"\.eval\(\)"),
             (lambda: ed.stream(2), NotImplementedError, "state of its own"),
             (lambda: opened.step(narrow), ValueError, "shape"),
             (lambda: opened.step(x64), ValueError, "float32"),
             (lambda: opened.step(xcpu), ValueError, "float32 tensor on"),
             (lambda: opened.step(x, mask3), ValueError, "mask_t"),
             (lambda: F.lstm_stream_step(x, None, st, -1, 40, 32, 16, 2, 5), ValueError, "negative"),
             (lambda: F.lstm_stream_step(x, None, small, 0, 40, 32, 16, 2, 5), ValueError, "state must be"),
             (lambda: F.lstm_stream_step_slots(x, None, small, good, 40, 32, 16, 2, 5), ValueError, "state must be"),
             (lambda: F.lstm_stream_step_slots(x, None, st, pos64, 40, 32, 16, 2, 5), ValueError, "positions must be"),
             (lambda: F.lstm_stream_step(x, None, st, 0, 40, 32, 16, 5, 5), ValueError, "n_layers > 4")]
    for call, exc, match in calls:
        def run():
            with pytest.raises(exc, match=match):
                call()
        names = device_kernel_names(run)[1]
        assert not names, (match, names)
        model.eval(), wrap.eval()
    assert opened.positions.cpu().tolist() == [-1, -1]
    torch.cuda.synchronize()
