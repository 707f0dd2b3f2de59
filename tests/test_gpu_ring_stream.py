"""GPU: a causal encoder stack with a span, one window at a time from a ring K/V cache (csrc/step_ring.h; encoder_step_ring_kernel,
encoder_step_ring_slots_kernel; mmt_encoder_stream_step_ring*; streaming.encoder_ring_step*, Encoder.ring_stream / ring_slot_stream,
streaming.ring_stream on the models and their wrappers; graphs.capture_stream on the slots forms).

The reference is tests/ring_stream_ref.py (tests/test_ring_stream_cpu.py holds it to band_ref's exact function in fp64); the bounds
are those of tests/test_gpu_bf16_faithful.py, imported as tests/test_gpu_stream.py imports them: per product the arithmetic is the
plain step's.  Against the batch forward with the span the bound grows by the distance D between the two references, computed here
on the CPU for each case.  Everything that the age order of the ring makes exact is held bit for bit: the first span rows against the
plain stream, the independence of a row from the ring's phase and from windows behind its receptive field, recordings, resets, batches,
fills, slots and replays.
"""
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

import band_ref as BD
import conftest
import recipe as R
import ring_stream_ref as RS
import slot_stream_ref as SL
from conftest import rel_l2
from gpu_harness import (FILLS, OUT_RTOL, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named, measures, mta,  # noqa: F401
                         seeded_encoder)
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
# (d, h, N, span, T): the smallest shapes that reach each branch; lengths [T, about 2T/3, 1]
CASES = [(32, 2, 1, 1, 4),                      # a ring of one row that is never read: ctx == bf16(v)
         (32, 2, 1, 2, 5),
         (40, 4, 2, 5, 23),                     # d_k = 10 padded to 16: two chunks; many wraps; two layers
         (128, 8, 2, 33, 70),                   # d_k = 16; the span crosses one key-group row of 32
         (64, 2, 3, 40, 130),                   # d_k = 32, three layers
         (256, 4, 1, 40, 90),                   # d_k = 64; the span exceeds one trip of 32 keys
         (128, 8, 1, 131, 270)]                 # more than one trip of 128 keys, and a wrap
IDS = ["d%d_h%d_n%d_span%d_T%d" % c for c in CASES]
PHASE = [c for c in CASES if c[3] in (5, 33)]
PHASE_IDS = [i for i, c in zip(IDS, CASES) if c[3] in (5, 33)]
_CACHE = {}


def _lengths(T):
    return [T, max(1, (2 * T) // 3), 1]


def _encoder(d, h, n, span, dev, seed=17):
    enc, p32 = seeded_encoder(d, h, n, dev, seed)
    mta().multiTransformer.causal_attention(enc, True, span=span)
    return enc, p32


def _record(stream, x, mask):
    """every window of x through stream.step, in order -> (B, T, d) on the CPU"""
    rows = [stream.step(x[:, t], mask[:, t]) for t in range(x.shape[1])]
    return torch.stack(rows, dim=1).cpu()


def _run(c, dev):
    """every GPU result and both CPU references of one case, computed once"""
    if c in _CACHE:
        return _CACHE[c]
    d, h, n, span, T = c
    lengths = _lengths(T)
    B = len(lengths)
    enc, p32 = _encoder(d, h, n, span, dev)
    x = R.gen_normal("gpu_ring_d%d_T%d:x" % (d, T), (B, T, d), 17)
    mask = R.prefix_mask(lengths, T)
    xg, mg = x.to(dev), mask.to(dev)
    out = {"enc": enc, "x": xg, "mask": mg, "ones": torch.ones_like(mg)}
    with torch.no_grad():
        out["batch"] = enc(xg, mg).cpu()
    s = enc.ring_stream(B)
    assert (s.t, s.capacity, s.span, s.slots) == (0, None, span, False)
    out["stream"] = _record(s, xg, mg)
    assert s.t == T
    s.reset()
    assert s.t == 0
    out["after_reset"] = _record(s, xg, mg)
    out["again"] = _record(enc.ring_stream(B), xg, mg)
    torch.cuda.synchronize()
    pd = {k: v.double() for k, v in p32.items()}
    with torch.no_grad():
        out["ref"] = RS.encoder_stack(pd, "", x.double(), mask.double(), h, span).numpy()
        out["batch_ref"] = BD.encoder_stack(pd, "", x.double(), mask.double(), h, span).detach().numpy()
    _CACHE[c] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_ring_stream_against_the_ring_reference(dev, c):
    """all rows of y against ring_stream_ref.encoder_stack under ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3 (rel-L2 / per-row maximum).
    Measured worst over the cases: 3.0e-4 / 1.5e-3 (d 64, three layers); d 128 span 33 2.1e-4 / 9.8e-4; the cases in which fp32 noise
    tips no bf16 rounding (d 32, d 40) sit at 8e-8 .. 7e-7."""
    r = _run(c, dev)
    check("ring %s y" % IDS[CASES.index(c)], r["stream"], r["ref"], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. against the batch path
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_ring_stream_against_the_batch_forward(dev, c):
    """the streamed rows against Encoder.forward (causal with the span, eval) of the same inputs on the GPU.  The two paths round the
    softmax at different reference points, so the bound is ENC_OUT + D and ENC_OUT_ROW + D_row, D the distance between the two
    REFERENCES of this case (ring_stream_ref and band_ref), computed here on the CPU: the rule of
    test_gpu_stream.py::test_stream_against_the_batch_forward, nothing is measured against the code under test alone.
    Measured worst: 1.05e-3 / 2.84e-3 (d 64) with D = 1.04e-3 / 2.86e-3: the distance is the references', not the kernels'.  D is
    exactly 0 at span 1."""
    r = _run(c, dev)
    D, D_row = measures(r["ref"], r["batch_ref"])
    print("ring %s: distance of the two references rel-L2 %.3e per-row %.3e" % (IDS[CASES.index(c)], D, D_row))
    check("ring %s y vs batch forward" % IDS[CASES.index(c)], r["stream"], r["batch"], ENC_OUT + D, ENC_OUT_ROW + D_row)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. exact facts, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_first_span_rows_are_those_of_the_plain_stream(dev, c):
    """while t < span the ring step is the plain step instruction for instruction (r0 = 0, row = position): the first span rows equal
    those of stream(B, span) of the same encoder with causal_attention(enc) and no span"""
    d, h, n, span, T = c
    r = _run(c, dev)
    plain, _ = seeded_encoder(d, h, n, dev, 17)
    mta().multiTransformer.causal_attention(plain)
    got = _record(plain.stream(3, span), r["x"][:, :span], r["mask"][:, :span])
    assert torch.isfinite(got).all() and torch.equal(got, r["stream"][:, :span])
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", PHASE, ids=PHASE_IDS)
def test_a_row_does_not_depend_on_the_phase_of_the_ring(dev, c):
    """mask all ones: the recording cut to x[:, s:], s no multiple of the span, gives at t' >= N (span - 1) the bits of the full
    recording's row t' + s: the same windows stand in other rows of the ring, and meet the same lanes in the same order.
    At (128,8,2,33,70) the cut at s = 7 leaves 63 windows, none at t' >= 64, so there the recording is the case's 70 windows and 5 more:
    every cut then has at least 4 rows to compare."""
    d, h, n, span, T = c
    r = _run(c, dev)
    first = n * (span - 1)
    L = max(T, first + 7 + 4)
    x = torch.cat([r["x"], R.gen_normal("gpu_ring_phase_d%d:x" % d, (3, L - T, d), 17).to(dev)], dim=1) if L > T else r["x"]
    ones = torch.ones(3, L, 1, device=dev)
    full = _record(r["enc"].ring_stream(3), x, ones)
    assert torch.equal(full[:, :T], _record(r["enc"].ring_stream(3), r["x"], r["ones"]))
    for s in (3, 7):
        assert s % span and L - s >= first + 4
        cut = _record(r["enc"].ring_stream(3), x[:, s:], ones[:, s:])
        assert torch.isfinite(cut).all() and torch.equal(cut[:, first:], full[:, first + s:]), s
        assert not torch.equal(cut[:, :first], full[:, s:first + s])             # the rows before that see another past
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", PHASE, ids=PHASE_IDS)
def test_a_row_depends_on_its_receptive_field_only(dev, c):
    """row t of an N-layer stack sees windows t - N (span - 1) .. t: other values in every older window leave its bits, another value
    in the oldest window inside moves them"""
    d, h, n, span, T = c
    r = _run(c, dev)
    t, oldest = T - 1, T - 1 - n * (span - 1)
    assert oldest > 0
    full = _record(r["enc"].ring_stream(3), r["x"], r["ones"])
    x = r["x"].clone()
    x[:, :oldest] = R.gen_normal("gpu_ring_local:x", (3, oldest, d), 23).to(dev)
    behind = _record(r["enc"].ring_stream(3), x, r["ones"])
    assert torch.equal(behind[:, t], full[:, t]) and not torch.equal(behind[:, t - 1], full[:, t - 1])
    x = r["x"].clone()
    x[:, oldest] = R.gen_normal("gpu_ring_local:oldest", (3, d), 23).to(dev)
    inside = _record(r["enc"].ring_stream(3), x, r["ones"])
    assert not torch.equal(inside[:, t], full[:, t]) and torch.equal(inside[:, :oldest], full[:, :oldest])
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_two_recordings_and_a_reset_give_the_same_bits(dev, c):
    r = _run(c, dev)
    assert torch.isfinite(r["stream"]).all()
    assert torch.equal(r["stream"], r["again"])                   # a second, fresh stream
    assert torch.equal(r["stream"], r["after_reset"])             # the same stream after reset(): the ring stood at T mod span, nothing was cleared
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_a_sequence_does_not_depend_on_its_batch(dev, c):
    r = _run(c, dev)
    alone = _record(r["enc"].ring_stream(1), r["x"][:1], r["mask"][:1])
    assert torch.equal(alone[0], r["stream"][0])
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_state_may_hold_any_contents(dev, c, fill):
    """the whole state (the ring with it) filled with each pattern before step 0, the weights prepared afterwards: the same bits.
    Rows that hold no position of this recording yet, and the pad columns of every row, never reach a result."""
    r = _run(c, dev)
    s = r["enc"].ring_stream(3)
    before = s.state.clone()
    fill_bytes(s.state.view(-1), fill)
    assert not torch.equal(before, s.state)
    s.refresh()
    assert torch.equal(_record(s, r["x"], r["mask"]), r["stream"])
    torch.cuda.synchronize()


def test_a_ring_of_one_row_gives_the_value_itself(dev):
    """span 1: a window attends itself alone, P = 1, so the batch path and the step round the same numbers: rows agree with the
    batch forward within twice ENC_OUT (each within ENC_OUT of the one reference), with D exactly 0"""
    r = _run(CASES[0], dev)
    D, D_row = measures(r["ref"], r["batch_ref"])
    assert D == 0 and D_row == 0
    assert rel_l2(r["stream"].numpy(), r["batch"].numpy()) <= 2 * ENC_OUT


# ------------------------------------------------------------------------------------------------ 4. slots
def _positions(z):
    return z.positions.cpu().tolist()


SCHEDULE = [(0, 0, "seat", 0), (2, 1, "seat", 1), (9, 1, "release", None), (11, 1, "seat", 2), (13, 2, "seat", 3)]


def test_staggered_slots_have_the_bits_of_each_recording_alone(dev):
    """(40,4,2) span 5, B = 3, 30 calls; slot 1 released at call 9 and seated again at call 11 with another recording, over the ring
    the first one left: each computed row has the bits of that recording alone in the host-t ring stream, idle rows are exact zeros"""
    d, h, n, span, calls, B = 40, 4, 2, 5, 30, 3
    enc, _ = _encoder(d, h, n, span, dev)
    recs = {r: R.gen_normal("gpu_ring_stag:x%d" % r, (calls, d), 17) for r in range(4)}
    masks = {r: R.prefix_mask([[30, 4, 12, 9][r]], calls).reshape(-1) for r in range(4)}
    table, positions = SL.timetable(SCHEDULE, calls, B)
    xin = SL.call_inputs(table, recs, torch.full((d,), 3.0)).to(dev)
    min_ = SL.call_inputs(table, {r: m.reshape(-1, 1) for r, m in masks.items()}, torch.ones(1)).to(dev)
    z = enc.ring_slot_stream(B)
    assert _positions(z) == [-1] * B and z.slots and z.capacity is None and z.span == span
    rows = []
    for call in range(calls):
        for c_, slot, what, _ in SCHEDULE:
            if c_ == call:
                (z.seat if what == "seat" else z.release)([slot])
        assert _positions(z) == positions[call], call
        rows.append(z.step(xin[call], min_[call]))
    got = torch.stack(rows).cpu()
    assert _positions(z) == [30, 19, 17] and not z.full().any()
    for rec, nwin in SL.windows_used(table).items():
        s = enc.ring_stream(1)
        xr, mr = recs[rec].to(dev), masks[rec].to(dev)
        alone = torch.stack([s.step(xr[t:t + 1], mr[t:t + 1]) for t in range(nwin)]).cpu().reshape(nwin, d)
        for call, row in enumerate(table):
            for slot, cell in enumerate(row):
                if cell is not None and cell[0] == rec:
                    assert torch.equal(got[call, slot], alone[cell[1]]), (call, slot, cell)
    n_idle = sum(cell is None for row in table for cell in row)
    assert n_idle == 2 + 2 + 13
    for call, row in enumerate(table):
        for slot, cell in enumerate(row):
            if cell is None:
                assert (got[call, slot] == 0).all(), (call, slot)
    assert torch.isfinite(got).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", PHASE, ids=PHASE_IDS)
def test_a_position_moved_by_a_multiple_of_the_span_changes_nothing(dev, c):
    """after t0 >= span steps, adding a multiple of the span to a position leaves every later row bit-equal: the ring's rows are where
    they were.  Slot 1 is moved so that it steps past 4096 (the plain stream's last capacity), slot 2 beyond 2^30; neither becomes
    full, and both arrive where they should."""
    d, h, n, span, T = c
    r = _run(c, dev)
    z, e = r["enc"].ring_slot_stream(3), r["enc"].ring_slot_stream(3)
    z.reset(), e.reset()
    t0 = span + 3
    for t in range(t0):
        assert torch.equal(z.step(r["x"][:, t], r["ones"][:, t]), e.step(r["x"][:, t], r["ones"][:, t]))
    near = (4096 - t0 - 1) // span * span                                        # slot 1 then crosses 4096 within the next steps
    far = (2 ** 30 // span + 1) * span
    assert t0 + near < 4096 < t0 + near + (T - t0) and t0 + far > 2 ** 30
    z.positions.add_(torch.tensor([0, near, far], dtype=torch.int32, device=dev))
    for t in range(t0, T):
        y = z.step(r["x"][:, t], r["ones"][:, t])
        assert torch.equal(y, e.step(r["x"][:, t], r["ones"][:, t])), t
        assert y[1].abs().max() > 0 and y[2].abs().max() > 0
    assert _positions(z) == [T, T + near, T + far] and _positions(e) == [T] * 3
    assert not z.full().any()
    torch.cuda.synchronize()


def _ring_check_passes():
    """tools/ring_plan_check.cpp under ASan / UBSan on the host -> True (passed), False (failed), None (no compiler here)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ring_plan_check")
        src = os.path.join(conftest.ROOT, "tools", "ring_plan_check.cpp")
        if subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                          capture_output=True, timeout=300).returncode != 0:
            return None
        return subprocess.run([exe], capture_output=True, timeout=300).returncode == 0


def test_edge_positions(dev):
    """positions [-1, INT_MAX, INT_MAX - 1]: the first two give zero rows and keep their positions, the third runs once, the last
    position there is, and stands at INT_MAX; then every slot is idle or at INT_MAX and the whole state is bit-identical before and
    after.  The host check of the rule (tools/ring_plan_check.cpp under ASan / UBSan, which walks the positions up to INT_MAX - 1)
    is run here first where a compiler is present, and nothing is launched if it fails."""
    ok = _ring_check_passes()
    assert ok is not False, "tools/ring_plan_check.cpp fails on the host: not running edge positions on the GPU"
    enc, _ = _encoder(40, 4, 2, 5, dev)
    x = R.gen_normal("gpu_ring_edge:x", (3, 40), 17).to(dev)
    z = enc.ring_slot_stream(3)
    fill_bytes(z.state.view(-1), "zeros")                                        # the rows of a ring nobody stepped: defined values
    z.refresh()
    z.positions.copy_(torch.tensor([-1, INT_MAX, INT_MAX - 1], dtype=torch.int32))
    assert z.full().cpu().tolist() == [False, True, False]
    y = z.step(x)
    assert _positions(z) == [-1, INT_MAX, INT_MAX]
    assert (y[:2] == 0).all() and torch.isfinite(y[2]).all() and y[2].abs().max() > 0
    before = z.state.clone()
    y = z.step(x)
    assert (y == 0).all() and torch.equal(z.state, before) and _positions(z) == [-1, INT_MAX, INT_MAX]
    y = z.step(x, advance=False)
    assert (y == 0).all() and torch.equal(z.state, before) and _positions(z) == [-1, INT_MAX, INT_MAX]
    # the host-t stream refuses INT_MAX itself, before any launch
    s = enc.ring_stream(3)
    s.t = INT_MAX
    with pytest.raises(ValueError, match="INT_MAX"):
        s.step(x)
    assert s.t == INT_MAX
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. launches
def _stepper(stream, xs, ms):
    t = [-1]

    def step():
        t[0] += 1
        return stream.step(xs[t[0]], ms[t[0]])
    return step, t


def test_one_step_is_one_launch_of_the_ring_kernel(dev):
    r = _run(CASES[3], dev)
    xs = [r["x"][:, t].contiguous() for t in range(3)]          # the caller's slicing is not the step's
    ms = [r["mask"][:, t].contiguous() for t in range(3)]
    s = r["enc"].ring_stream(3)
    step, _ = _stepper(s, xs, ms)
    torch.cuda.synchronize()
    _, names = device_kernel_names(step, warm=True)
    z = r["enc"].ring_slot_stream(3)
    z.reset()
    zstep, _ = _stepper(z, xs, ms)
    torch.cuda.synchronize()
    _, znames = device_kernel_names(zstep, warm=True)
    torch.cuda.synchronize()
    if names is None or znames is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert len(names) == 1 and "encoder_step_ring_kernel" in names[0], names
    assert len(znames) == 1 and "encoder_step_ring_slots_kernel" in znames[0], znames


def _small_model(dev, span=5):
    MT = mta().multiTransformer
    model = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    load_named(model)
    MT.causal_attention(model, True, span=span)
    return model.eval()


def test_a_warmed_model_step_launches_no_library_kernel(dev):
    MT = mta().multiTransformer
    model = _small_model(dev)
    x = R.gen_normal("gpu_ring_nolib:x", (3, 6, 48), 5).to(dev)
    mask = R.prefix_mask([6, 3, 1], 6).to(dev)
    xs, ms = [x[:, t].contiguous() for t in range(6)], [mask[:, t].contiguous() for t in range(6)]
    s = MT.ring_stream(model, 3)
    step, t = _stepper(s, xs, ms)
    step(), step()                                           # warm-up: the pool's workspaces of these shapes exist
    s.reset()
    t[0] = -1
    torch.cuda.synchronize()
    _, first = device_kernel_names(step)
    _, later = device_kernel_names(step)
    torch.cuda.synchronize()
    if first is None or later is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(first) == [] and library_kernels(later) == [], (first, later)
    assert sum("encoder_step_ring_kernel" in n for n in later) == 1 and not any("encoder_step_kernel" in n for n in later), later


def test_replays_have_the_bits_of_the_eager_slots_stream(dev):
    """(40,4,2) span 5: capturing changes neither the state nor the positions; T = 23 > 2 span replays fed through copy_ equal the
    eager ring slots stream, wraps of the ring included: the position is read from device memory by every replay"""
    from multimodal_transformer_amd import graphs
    c = CASES[2]
    d, h, n, span, T = c
    r = _run(c, dev)
    x, mask = r["x"], r["mask"]
    z, e = r["enc"].ring_slot_stream(3), r["enc"].ring_slot_stream(3)
    z.seat([1])
    z.step(x[:, 0], mask[:, 0])
    before, pos = z.state.clone(), _positions(z)
    assert pos == [-1, 1, -1]
    g = graphs.capture_stream(z, x[:, 0], mask[:, 0])
    assert torch.equal(z.state, before) and _positions(z) == pos
    z.reset(), e.reset()
    assert T > 2 * span
    rows = []
    for t in range(T):
        g.inputs.copy_(x[:, t])
        g.mask.copy_(mask[:, t])
        y = g.replay().clone()
        assert torch.equal(y, e.step(x[:, t], mask[:, t])), t
        rows.append(y)
    assert torch.equal(torch.stack(rows, dim=1).cpu(), r["stream"])              # and those of the host-t ring stream
    assert _positions(z) == _positions(e) == [T] * 3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. models
def _model_case(which, dev):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    T, lengths = 20, [20, 7, 1]
    mask = R.prefix_mask(lengths, T).to(dev)
    if which.startswith("sft"):
        model = _small_model(dev)
        x = R.gen_normal("gpu_ring_model_sft:x", (3, T, 48), 5).to(dev)
        forward = lambda: model(x, mask, lengths)                                # noqa: E731
        window = lambda t: x[:, t]                                               # noqa: E731
    elif which.startswith("mft"):
        mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
        model = MT.MultiTransformer(mods, wes, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32})
        load_named(model)
        x = {mod: R.gen_normal("gpu_ring_model_mft:" + mod, (3, T, wes[mod]), 5).to(dev) for mod in mods}
        forward = lambda: model(x, mask, lengths)                                # noqa: E731
        window = lambda t: {mod: x[mod][:, t].contiguous() for mod in mods}      # noqa: E731
    else:
        mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
        model = MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=dev)
        model.Transformer = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
        load_named(model)
        x = {mod: R.gen_normal("gpu_ring_model_wrap:" + mod, (3, T, 3, dims[mod]), 5).to(dev) for mod in mods}
        forward = lambda: model(x, lengths, mask)                                # noqa: E731
        window = lambda t: {mod: x[mod][:, t] for mod in mods}                   # noqa: E731
    MT.causal_attention(model, True, span=5)
    model.eval()
    return model, forward, window, mask, T, lengths


@pytest.mark.parametrize("which", ["sft_host", "sft_slots", "mft_slots", "wrapper_host", "wrapper_slots"])
def test_model_ring_stream_against_its_batch_forward(dev, which):
    """streamed predictions at span 5, T = 20 against the model's own eval forward with the span: rel-L2 <= OUT_RTOL, the bound
    tests/test_gpu_stream.py uses for that comparison without a span; padded windows are exact zeros; a second recording starts anew.
    Measured, both recordings and both forms alike: the SFT 4.8e-3, the MFT 2.2e-3, the two-modality wrapper 3.6e-3."""
    MT = mta().multiTransformer
    model, forward, window, mask, T, lengths = _model_case(which, dev)
    slots = which.endswith("slots")
    with torch.no_grad():
        want = forward().cpu()
    s = MT.ring_stream(model, 3, slots=slots)
    assert s.capacity is None and bool(getattr(s, "slots", False)) == slots
    for rec in range(2):
        s.reset()
        got = torch.stack([s.step(window(t), mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
        assert got.shape == want.shape == (3, T, 1)
        err = rel_l2(got.numpy(), want.numpy())
        print("ring stream model %s recording %d: rel_l2 %.3e" % (which, rec, err))
        assert torch.isfinite(got).all() and err <= OUT_RTOL
        for b, nwin in enumerate(lengths):
            assert (got[b, nwin:] == 0).all() and got[b, :nwin].abs().min() > 0
        assert (s.positions.cpu().tolist() == [T] * 3 and not s.full().any()) if slots else s.t == T
    torch.cuda.synchronize()


def test_a_model_slots_stream_replays(dev):
    """graphs.capture_stream works unchanged on the slots=True form of a model: replays equal the eager stream"""
    from multimodal_transformer_amd import graphs
    MT = mta().multiTransformer
    model, _, window, mask, T, _ = _model_case("mft_slots", dev)
    z, e = MT.ring_stream(model, 3, slots=True), MT.ring_stream(model, 3, slots=True)
    g = graphs.capture_stream(z, window(0), mask[:, 0].contiguous())
    assert _positions(z) == [-1] * 3
    z.reset(), e.reset()
    for t in range(12):
        w = window(t)
        for mod in w:
            g.inputs[mod].copy_(w[mod])
        g.mask.copy_(mask[:, t])
        assert torch.equal(g.replay(), e.step(w, mask[:, t].contiguous())), t
    assert _positions(z) == [12] * 3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. refusals before any launch
def _refused(call, exc, match):
    def run():
        with pytest.raises(exc, match=match):
            call()
    return device_kernel_names(run)[1]


def test_refusals_come_before_any_launch(dev):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    x = torch.zeros(2, 32, device=dev)
    plain, _ = seeded_encoder(32, 2, 1, dev, 3)
    MT.causal_attention(plain)
    dense, _ = seeded_encoder(32, 2, 1, dev, 3)
    banded, _ = _encoder(32, 2, 1, 4, dev, 3)
    wide, _ = seeded_encoder(32, 2, 1, dev, 3)
    MT.causal_attention(wide, True, span=4097)
    training, _ = _encoder(32, 2, 1, 4, dev, 3)
    opened = banded.ring_stream(2)
    zopened = banded.ring_slot_stream(2)
    ended = banded.ring_stream(2)
    ended.t = INT_MAX
    stacked = MT.NLPTransformer(48, embed_dim=40, h=4, N=1, n_layers=2, device=dev).eval()
    MT.causal_attention(stacked, True, span=4)
    b3 = MT.MultiTransformerB3(["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}, device=dev).eval()
    lstm = MM.MultiLSTM(24, embed_dim=16, h_dim=16, device=dev).eval()
    x64, xcpu, narrow, mask3 = x.double(), x.cpu(), x[:, :16].contiguous(), torch.ones(3, device=dev)
    floatpos = torch.zeros(2, device=dev)                                        # positions must be int32
    torch.cuda.synchronize()
    for call, exc, match in ((lambda: plain.ring_stream(2), ValueError, r"causal_attention\(model, span=W\)"),
                             (lambda: MT.ring_stream(plain, 2, slots=True), ValueError, r"causal_attention\(model, span=W\)"),
                             (lambda: dense.ring_stream(2), ValueError, r"causal_attention\(model\)"),
                             (lambda: training.train().ring_stream(2), ValueError, r"\.eval\(\)"),
                             (lambda: wide.ring_stream(2), ValueError, "capacity > 4096"),
                             (lambda: banded.stream(2, 8), ValueError, r"span = 4.*ring cache"),
                             (lambda: banded.slot_stream(2, 8), ValueError, r"span = 4.*ring cache"),
                             (lambda: banded.ring_slot_stream(2, floatpos), ValueError, "positions"),
                             (lambda: ended.step(x), ValueError, "INT_MAX"),
                             (lambda: opened.step(narrow), ValueError, "shape"),
                             (lambda: opened.step(x64), ValueError, "float32"),
                             (lambda: opened.step(xcpu), ValueError, "float32 tensor on"),
                             (lambda: zopened.step(x, mask3), ValueError, "mask_t"),
                             (lambda: MT.ring_stream(stacked, 2), NotImplementedError, "n_layers"),
                             (lambda: MT.ring_stream(b3, 2), ValueError, r"stream\(batch\)"),
                             (lambda: MT.ring_stream(lstm, 2, slots=True), ValueError, r"stream\(batch\)")):
        names = _refused(call, exc, match)
        assert not names, (match, names)
    assert opened.t == 0 and zopened.positions.cpu().tolist() == [-1, -1]
    torch.cuda.synchronize()
