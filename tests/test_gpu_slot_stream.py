"""GPU: slots streams (csrc/step_slots.h; encoder_step_slots_kernel, mfn_step_slots_kernel; mmt_*_stream_step_slots;
functional.*_stream_step_slots; the slot_stream methods of Encoder, MFN, MultiTransformer, MultiTransformerB3 and their wrappers;
graphs.capture_stream).

The positioned kernels are the bodies of the host-t kernels with t read from device memory, one workgroup per sequence, and this change
does not alter the host-t form.  So the claims against the host-t streams carry NO tolerance: a seated row equals, bit for bit, the row
of that recording stepped alone in a batch-1 host-t stream, an idle or full row is exact zeros, and a replayed step equals the eager
one.  Against tests/slot_stream_ref.py the bounds are those tests/test_gpu_stream.py and tests/test_gpu_mfn_stream.py already use for
these kernels, imported.
"""
import os
import shutil
import subprocess

import pytest
import torch

import conftest
import recipe as R
import slot_stream_ref as SL
from conftest import rel_l2
from gpu_harness import OUT_RTOL, check, dev, device_kernel_names, library_kernels, load_named, measures, mta, seeded_encoder  # noqa: F401
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW
from test_gpu_mfn_stream import CASES as GATE_CASES
from test_gpu_mfn_stream import MFN_STEP_OUT, MFN_STEP_ROW, _b3, _gate, _small_mft

pytestmark = pytest.mark.gpu

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
_CACHE = {}


def _encoder(d, h, n, dev, seed=17):
    enc, p32 = seeded_encoder(d, h, n, dev, seed)
    mta().multiTransformer.causal_attention(enc)
    return enc, p32


def _positions(z):
    return z.positions.cpu().tolist()


# ------------------------------------------------------------------------------------------------ 1. lockstep
@pytest.mark.parametrize("c", [(32, 2, 1, 1, [1]), (40, 4, 2, 45, [45, 30, 1]), (64, 2, 3, 130, [130, 86, 1])],
                         ids=["d32_h2_n1_T1", "d40_h4_n2_T45", "d64_h2_n3_T130"])
def test_encoder_lockstep_has_the_bits_of_the_host_t_stream(dev, c):
    """every slot seated at call 0: every step of the slots stream against the host-t stream on the same inputs and prefix masks"""
    d, h, n, T, lengths = c
    B = len(lengths)
    enc, _ = _encoder(d, h, n, dev)
    x = R.gen_normal("gpu_slot_lock_d%d:x" % d, (B, T, d), 17).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    s, z = enc.stream(B, T), enc.slot_stream(B, T)
    assert _positions(z) == [-1] * B and z.slots and not s.slots
    z.reset()
    a = torch.stack([s.step(x[:, t], mask[:, t]) for t in range(T)], dim=1)
    b = torch.stack([z.step(x[:, t], mask[:, t]) for t in range(T)], dim=1)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert _positions(z) == [T] * B and z.full().all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [GATE_CASES[0], GATE_CASES[2], GATE_CASES[3]], ids=["emo_B1_T1", "lin+aco+ima_B3_T12", "all_four_B2_T5"])
def test_gate_lockstep_has_the_bits_of_the_host_t_stream(dev, c):
    mods, widths, lengths, T = c
    B = len(lengths)
    gate, _ = _gate(c, dev)
    x = {m: R.gen_normal("gpu_slot_lock:%s:%d" % (m, T), (T, B, w), 11).to(dev) for m, w in zip(mods, widths)}
    mask = R.prefix_mask(lengths, T).to(dev)
    s, z = gate.stream(B), gate.slot_stream(B)
    assert _positions(z) == [-1] * B and z.capacity is None
    z.reset()
    a = torch.stack([s.step({m: x[m][t] for m in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1)
    b = torch.stack([z.step({m: x[m][t] for m in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert _positions(z) == [T] * B and not z.full().any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. staggered
def _events(schedule, call):
    return [(slot, what) for c, slot, what, _ in schedule if c == call]


def _apply(z, schedule, call):
    for slot, what in _events(schedule, call):
        (z.seat if what == "seat" else z.release)([slot])


ENC_SCHEDULE = [(0, 0, "seat", 0), (1, 1, "seat", 1), (40, 1, "release", None), (50, 1, "seat", 4), (60, 2, "seat", 2), (129, 3, "seat", 3)]
ENC_LENGTHS = [130, 30, 70, 1, 60]          # windows of each recording that are not blanked: 1 and 4 run past theirs (blanked, yet windows)


def _staggered_encoder(dev):
    if "enc" in _CACHE:
        return _CACHE["enc"]
    d, h, n, cap, B, calls = 64, 2, 3, 130, 4, 130
    enc, p32 = _encoder(d, h, n, dev)
    recs = {r: R.gen_normal("gpu_slot_stag:x%d" % r, (cap, d), 17) for r in range(5)}
    masks = {r: R.prefix_mask([ENC_LENGTHS[r]], cap).reshape(-1) for r in range(5)}
    table, positions = SL.timetable(ENC_SCHEDULE, calls, B, limit=cap)
    xin = SL.call_inputs(table, recs, torch.full((d,), 3.0)).to(dev)                     # an idle slot is fed values, and is NOT blanked
    min_ = SL.call_inputs(table, {r: m.reshape(-1, 1) for r, m in masks.items()}, torch.ones(1)).to(dev)
    z = enc.slot_stream(B, cap)
    rows, seen = [], []
    for call in range(calls):
        _apply(z, ENC_SCHEDULE, call)
        if call in (0, 41, 50, 129):
            seen.append((call, _positions(z), positions[call]))
        rows.append(z.step(xin[call], min_[call]))
    got = torch.stack(rows).cpu()                                                        # (calls, B, d)
    alone = {}
    for rec, nwin in SL.windows_used(table).items():
        s = enc.stream(1, cap)
        xr, mr = recs[rec].to(dev), masks[rec].to(dev)
        alone[rec] = torch.stack([s.step(xr[t:t + 1], mr[t:t + 1]) for t in range(nwin)]).cpu().reshape(nwin, d)
    torch.cuda.synchronize()
    _CACHE["enc"] = dict(got=got, alone=alone, table=table, seen=seen, recs=recs, masks=masks, p32=p32, h=h, final=_positions(z))
    return _CACHE["enc"]


def _cells(table):
    return [(call, slot, cell) for call, row in enumerate(table) for slot, cell in enumerate(row)]


def test_encoder_staggered_rows_are_those_of_each_recording_alone(dev):
    """(64,2,3,130), B = 4, seats at calls 0, 1, 60 and 129; slot 1 released at call 40 and seated again at call 50 with another
    recording, over the rows the first one left in the cache.  Bit for bit against batch-1 host-t streams; idle rows exact zeros."""
    r = _staggered_encoder(dev)
    for call, have, want in r["seen"]:
        assert have == want, (call, have, want)
    assert r["final"] == [130, 80, 70, 1]
    n_idle = 0
    for call, slot, cell in _cells(r["table"]):
        if cell is None:
            n_idle += 1
            assert (r["got"][call, slot] == 0).all(), (call, slot)
        else:
            assert torch.equal(r["got"][call, slot], r["alone"][cell[0]][cell[1]]), (call, slot, cell)
    assert n_idle == 1 + 10 + 60 + 129
    assert torch.isfinite(r["got"]).all() and r["got"][129, 3].abs().max() > 0


def test_encoder_staggered_against_the_slot_reference(dev):
    """the computed cells against slot_stream_ref (every recording alone through stream_ref) under ENC_OUT / ENC_OUT_ROW"""
    r = _staggered_encoder(dev)
    pd = {k: v.double() for k, v in r["p32"].items()}
    ref = SL.encoder_slots(pd, "", r["h"], {k: v.double() for k, v in r["recs"].items()}, {k: v.double() for k, v in r["masks"].items()},
                           r["table"])
    on = [(call, slot) for call, slot, cell in _cells(r["table"]) if cell is not None]
    got = torch.stack([r["got"][c, s] for c, s in on])
    want = torch.stack([ref[c, s] for c, s in on])
    check("slots staggered encoder y", got, want.numpy(), ENC_OUT, ENC_OUT_ROW)


GATE_SCHEDULE = [(0, 0, "seat", 0), (1, 1, "seat", 1), (4, 1, "release", None), (5, 1, "seat", 4), (6, 2, "seat", 2), (11, 3, "seat", 3)]
GATE_LENGTHS = [12, 2, 4, 1, 5]


def _staggered_gate(dev):
    if "gate" in _CACHE:
        return _CACHE["gate"]
    c = GATE_CASES[2]
    mods, widths = c[0], c[1]
    B, calls = 4, 12
    gate, p32 = _gate(c, dev)
    recs = {r: {m: R.gen_normal("gpu_slot_stag:%s%d" % (m, r), (calls, w), 11) for m, w in zip(mods, widths)} for r in range(5)}
    masks = {r: R.prefix_mask([GATE_LENGTHS[r]], calls).reshape(-1) for r in range(5)}
    table, positions = SL.timetable(GATE_SCHEDULE, calls, B)
    xin = {m: SL.call_inputs(table, {r: recs[r][m] for r in recs}, torch.full((w,), 3.0)).to(dev) for m, w in zip(mods, widths)}
    min_ = SL.call_inputs(table, {r: m.reshape(-1, 1) for r, m in masks.items()}, torch.ones(1)).to(dev)
    z = gate.slot_stream(B)
    rows = []
    for call in range(calls):
        _apply(z, GATE_SCHEDULE, call)
        rows.append(z.step({m: xin[m][call] for m in mods}, min_[call]))
    got = torch.stack(rows).cpu()
    alone = {}
    for rec, nwin in SL.windows_used(table).items():
        s = gate.stream(1)
        xr, mr = {m: recs[rec][m].to(dev) for m in mods}, masks[rec].to(dev)
        alone[rec] = torch.stack([s.step({m: xr[m][t:t + 1] for m in mods}, mr[t:t + 1]) for t in range(nwin)]).cpu().reshape(nwin, -1)
    torch.cuda.synchronize()
    _CACHE["gate"] = dict(got=got, alone=alone, table=table, recs=recs, masks=masks, p32=p32, mods=mods, final=_positions(z))
    return _CACHE["gate"]


def test_gate_staggered_rows_are_those_of_each_recording_alone(dev):
    """the schedule shortened to 12 calls for the three-modality gate: seats at calls 0, 1, 6 and 11, slot 1 released at call 4 and
    seated again at call 5: the carried (h, c, mem) the first recording left, in either copy, cannot reach the second"""
    r = _staggered_gate(dev)
    assert r["final"] == [12, 7, 6, 1]
    for call, slot, cell in _cells(r["table"]):
        if cell is None:
            assert (r["got"][call, slot] == 0).all(), (call, slot)
        else:
            assert torch.equal(r["got"][call, slot], r["alone"][cell[0]][cell[1]]), (call, slot, cell)
    assert torch.isfinite(r["got"]).all() and r["got"][11, 3].abs().max() > 0


def test_gate_staggered_against_the_slot_reference(dev):
    """the computed cells against slot_stream_ref (every recording alone through mfn_stream_ref) under MFN_STEP_OUT / MFN_STEP_ROW,
    and under D, what the rounding itself moves this reference by, as tests/test_gpu_mfn_stream.py holds its cases"""
    r = _staggered_gate(dev)
    pd = {k: v.double() for k, v in r["p32"].items()}
    xd = {k: {m: v.double() for m, v in rec.items()} for k, rec in r["recs"].items()}
    md = {k: v.double() for k, v in r["masks"].items()}
    ref = SL.mfn_slots(pd, "", r["mods"], xd, md, r["table"])
    exact = SL.mfn_slots(pd, "", r["mods"], xd, md, r["table"], rounding=False)
    on = [(call, slot) for call, slot, cell in _cells(r["table"]) if cell is not None]
    got = torch.stack([r["got"][c, s] for c, s in on])
    want = torch.stack([ref[c, s] for c, s in on]).numpy()
    D, D_row = measures(want, torch.stack([exact[c, s] for c, s in on]).numpy())
    print("slots staggered gate: rounding on vs off rel-L2 %.3e per-row %.3e" % (D, D_row))
    assert D > 1e-4
    check("slots staggered gate y", got, want, min(MFN_STEP_OUT, D), min(MFN_STEP_ROW, D_row))


# ------------------------------------------------------------------------------------------------ 3. positions
def _decode_check_passes():
    """tools/slot_pos_check.cpp under ASan / UBSan on the host -> True (passed), False (failed), None (no compiler here)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "slot_pos_check")
        src = os.path.join(conftest.ROOT, "tools", "slot_pos_check.cpp")
        if subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                          capture_output=True, timeout=300).returncode != 0:
            return None
        return subprocess.run([exe], capture_output=True, timeout=300).returncode == 0


def test_advance_moves_seated_slots_only(dev):
    """advance off leaves the positions as they were; advance on adds 1 to the seated slots and to no other"""
    enc, _ = _encoder(40, 4, 2, dev)
    x = R.gen_normal("gpu_slot_adv:x", (3, 40), 17).to(dev)
    z = enc.slot_stream(3, 4)
    z.seat([0, 2])
    z.step(x), z.step(x)
    z.release([2])
    assert _positions(z) == [2, -1, -1]
    y0 = z.step(x, advance=False)
    assert _positions(z) == [2, -1, -1]
    y1 = z.step(x)
    assert _positions(z) == [3, -1, -1]
    assert torch.equal(y0, y1) and (y1[1:] == 0).all() and y1[0].abs().max() > 0         # the same window again: the same row
    gate, _ = _gate(GATE_CASES[1], dev)
    g = gate.slot_stream(3, limit=4)
    xs = {"acoustic": torch.ones(3, 12, device=dev), "emotient": torch.ones(3, 16, device=dev)}
    g.seat([1])
    g.step(xs, advance=False)
    assert _positions(g) == [-1, 0, -1]
    g.step(xs)
    assert _positions(g) == [-1, 1, -1]
    torch.cuda.synchronize()


def test_edge_positions_are_refused_by_the_kernel(dev):
    """capacity 4, positions [0, -1, INT_MIN, capacity, capacity + 1, INT_MAX]: slot 0 gives its batch-1 row and advances; every other
    slot gives a zero row and keeps its position.  With every slot idle or full the whole state is bit-identical before and after.
    The purpose is the refusal path of slot_decode, whose host check (tools/slot_pos_check.cpp under ASan / UBSan) must have passed
    in this tree: it is run here first where a compiler is present, and nothing is launched if it fails."""
    ok = _decode_check_passes()
    assert ok is not False, "tools/slot_pos_check.cpp fails on the host: not running edge positions on the GPU"
    cap = 4
    edge = [0, -1, INT_MIN, cap, cap + 1, INT_MAX]
    enc, _ = _encoder(40, 4, 2, dev)
    x = R.gen_normal("gpu_slot_edge:x", (6, 40), 17).to(dev)
    z = enc.slot_stream(6, cap)
    z.positions.copy_(torch.tensor(edge, dtype=torch.int32))
    y = z.step(x)
    assert _positions(z) == [1] + edge[1:]
    assert (y[1:] == 0).all() and torch.equal(y[0], enc.stream(1, cap).step(x[:1])[0])
    z.positions.copy_(torch.tensor([-1, INT_MIN, cap, cap + 1, INT_MAX, -7], dtype=torch.int32))
    before, pos = z.state.clone(), _positions(z)
    y = z.step(x)
    assert (y == 0).all() and torch.equal(z.state, before) and _positions(z) == pos
    # the gate, with the limit a composite stream gives it
    gate, _ = _gate(GATE_CASES[1], dev)
    xs = {"acoustic": torch.ones(6, 12, device=dev), "emotient": torch.ones(6, 16, device=dev)}
    g = gate.slot_stream(6, limit=cap)
    g.positions.copy_(torch.tensor(edge, dtype=torch.int32))
    y = g.step(xs)
    assert _positions(g) == [1] + edge[1:]
    assert (y[1:] == 0).all() and torch.equal(y[0], gate.stream(1).step({k: v[:1] for k, v in xs.items()})[0])
    g.positions.copy_(torch.tensor([-1, INT_MIN, cap, cap + 1, INT_MAX, -7], dtype=torch.int32))
    before, pos = g.state.clone(), _positions(g)
    y = g.step(xs)
    assert (y == 0).all() and torch.equal(g.state, before) and _positions(g) == pos
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. launches
def _stepper(stream, xs, ms):
    t = [-1]

    def step():
        t[0] += 1
        return stream.step(xs[t[0]], ms[t[0]])
    return step, t


def test_a_slots_step_is_one_launch_of_the_positioned_kernel(dev):
    enc, _ = _encoder(128, 8, 2, dev)
    x = R.gen_normal("gpu_slot_launch:x", (3, 3, 128), 17).to(dev)
    mask = R.prefix_mask([3, 2, 1], 3).to(dev)
    z = enc.slot_stream(3, 8)
    z.reset()
    step, _ = _stepper(z, [x[:, t].contiguous() for t in range(3)], [mask[:, t].contiguous() for t in range(3)])
    torch.cuda.synchronize()
    _, names = device_kernel_names(step, warm=True)
    gate, _ = _gate(GATE_CASES[2], dev)
    g = gate.slot_stream(3)
    g.reset()
    mods, widths = GATE_CASES[2][0], GATE_CASES[2][1]
    xs = [{m: torch.ones(3, w, device=dev) for m, w in zip(mods, widths)} for _ in range(3)]
    gstep, _ = _stepper(g, xs, [mask[:, t].contiguous() for t in range(3)])
    torch.cuda.synchronize()
    _, gnames = device_kernel_names(gstep, warm=True)
    torch.cuda.synchronize()
    if names is None or gnames is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert len(names) == 1 and "encoder_step_slots_kernel" in names[0], names
    assert len(gnames) == 1 and "mfn_step_slots_kernel" in gnames[0], gnames


def test_an_mft_slots_step_launches_what_the_host_t_step_launches(dev):
    """the same number of kernels as the host-t step, the positioned kernels in place of the two step kernels, no library kernel"""
    model, mods, wes = _small_mft(dev)
    x = {m: R.gen_normal("gpu_slot_nolib:" + m, (3, 6, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask([6, 3, 1], 6).to(dev)
    xs = [{m: x[m][:, t].contiguous() for m in mods} for t in range(6)]
    ms = [mask[:, t].contiguous() for t in range(6)]
    found = {}
    for kind in ("host", "slots"):
        s = model.stream(3, 6) if kind == "host" else model.slot_stream(3, 6)
        step, t = _stepper(s, xs, ms)
        s.reset()
        step(), step()                                       # warm-up: the pool's workspaces of these shapes exist
        s.reset()
        t[0] = -1
        torch.cuda.synchronize()
        _, first = device_kernel_names(step)
        _, later = device_kernel_names(step)
        torch.cuda.synchronize()
        if first is None or later is None:
            pytest.skip("torch.profiler reports no device kernels on this box")
        found[kind] = (first, later)
    for i in range(2):
        host, slots = found["host"][i], found["slots"][i]
        print(slots)
        assert len(slots) == len(host), (host, slots)
        assert library_kernels(slots) == [], slots
        assert sum("encoder_step_slots_kernel" in n for n in slots) == len(mods) and not any("encoder_step_kernel" in n for n in slots), slots
        assert sum("mfn_step_slots_kernel" in n for n in slots) == 1 and "mfn_step_slots_kernel" in slots[-1], slots
        assert not any("mfn_step_kernel" in n for n in slots), slots


# ------------------------------------------------------------------------------------------------ 5. graph
def test_encoder_replays_have_the_bits_of_the_eager_slots_stream(dev):
    """(40,4,2,45): capturing changes neither the state nor the positions; 10 replays fed through copy_ equal the eager slots stream;
    a slot seated between two replays starts its recording; a full slot gives a zero row and the other rows are unaffected"""
    from multimodal_transformer_amd import graphs
    d, h, n, cap, B = 40, 4, 2, 45, 3
    enc, _ = _encoder(d, h, n, dev)
    x = R.gen_normal("gpu_slot_graph:x", (B, 12, d), 17).to(dev)
    mask = R.prefix_mask([12, 5, 1], 12).to(dev)
    z, e = enc.slot_stream(B, cap), enc.slot_stream(B, cap)
    z.seat([1])
    z.step(x[:, 0], mask[:, 0])                                                          # a cache row and a position for the capture to leave alone
    before, pos = z.state.clone(), _positions(z)
    assert pos == [-1, 1, -1]
    g = graphs.capture_stream(z, x[:, 0], mask[:, 0])
    assert torch.equal(z.state, before) and _positions(z) == pos
    assert g.inputs.shape == (B, d) and g.mask.shape == mask[:, 0].shape and g.output.shape == (B, d)
    z.reset(), e.reset()
    for t in range(10):
        g.inputs.copy_(x[:, t])
        g.mask.copy_(mask[:, t])
        assert torch.equal(g.replay(), e.step(x[:, t], mask[:, t])), t
    assert _positions(z) == _positions(e) == [10] * B
    for s in (z, e):                                                                     # between two replays: seat slot 1 anew, fill slot 2
        s.seat([1])
        s.positions[2] = cap
    g.inputs.copy_(x[:, 10])
    g.mask.copy_(mask[:, 0])
    y = g.replay().clone()
    assert torch.equal(y, e.step(x[:, 10], mask[:, 0]))
    assert (y[2] == 0).all() and y[0].abs().max() > 0
    assert torch.equal(y[1], enc.stream(1, cap).step(x[1:2, 10], mask[1:2, 0])[0])       # window 0 of a new recording
    assert _positions(z) == [11, 1, cap] and z.full().cpu().tolist() == [False, False, True]
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["mft", "b3"])
def test_model_replays_have_the_bits_of_the_eager_slots_stream(dev, which):
    """the small MFT (N = 2, embed 40 / 32, h = 4) at T = 12 with lengths [12, 5, 1], and B3-MFN: capture leaves every state and the
    positions as they were, and the replays equal the eager slots stream of a second, identical stream"""
    from multimodal_transformer_amd import graphs
    model, mods, wes = _small_mft(dev) if which == "mft" else _b3(dev)
    T, lengths = 12, [12, 5, 1]
    x = {m: R.gen_normal("gpu_slot_graph_%s:%s" % (which, m), (3, T, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    z, e = model.slot_stream(3, T), model.slot_stream(3, T)
    first = {m: x[m][:, 0].contiguous() for m in mods}
    states = [z.gate.state] + [s.state for s in (z.encs or {}).values()]
    before = [s.clone() for s in states]
    g = graphs.capture_stream(z, first, mask[:, 0].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(states, before)) and _positions(z) == [-1] * 3
    z.reset(), e.reset()
    rows = []
    for t in range(T):
        for m in mods:
            g.inputs[m].copy_(x[m][:, t])
        g.mask.copy_(mask[:, t])
        y = g.replay().clone()
        assert torch.equal(y, e.step({m: x[m][:, t].contiguous() for m in mods}, mask[:, t].contiguous())), t
        rows.append(y)
    got = torch.stack(rows, dim=1).cpu()
    assert got.shape == (3, T, 1) and torch.isfinite(got).all() and got[0].abs().min() > 0
    for b, nwin in enumerate(lengths):
        assert (got[b, nwin:] == 0).all()
    assert _positions(z) == [T] * 3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. models
def _run_schedule(z, schedule, calls, feed):
    rows = []
    for call in range(calls):
        _apply(z, schedule, call)
        rows.append(z.step(*feed(call)))
    return torch.stack(rows).cpu()                           # (calls, slots, 1)


def _against_forward(tag, got, table, want, lengths, beyond=()):
    """each recording's computed rows against its own eval forward, under OUT_RTOL; its padded windows exact zeros; idle and full
    cells exact zeros.  beyond: (call, slot) cells that ran past the forward's last window and are not compared"""
    rows = {}
    for call, slot, cell in _cells(table):
        if (call, slot) in beyond:
            continue
        if cell is None:
            assert (got[call, slot] == 0).all(), (tag, call, slot)
        else:
            rows.setdefault(cell[0], []).append((cell[1], got[call, slot]))
    for rec, lst in rows.items():
        n = len(lst)
        assert [w for w, _ in lst] == list(range(n))
        y = torch.stack([v for _, v in lst])
        err = rel_l2(y.numpy(), want[rec][:n].numpy())
        print("%s recording %d (%d windows): rel_l2 %.3e" % (tag, rec, n, err))
        assert torch.isfinite(y).all() and err <= OUT_RTOL, (tag, rec, err)
        assert (y[lengths[rec]:] == 0).all()


def test_mft_slots_stream_against_its_batch_forward(dev):
    """MultiTransformer.slot_stream on a staggered schedule (capacity 12, 14 calls: recording 0 fills its slot, slot 1 is released and
    idle at the end): each recording against the model's own causal eval forward of that recording alone"""
    model, mods, wes = _small_mft(dev)
    T, lengths = 12, [12, 5, 1]
    x = {m: R.gen_normal("gpu_slot_mft:" + m, (3, T, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = [model({m: x[m][r:r + 1] for m in mods}, mask[r:r + 1], lengths[r:r + 1]).cpu()[0] for r in range(3)]
    sched = [(0, 0, "seat", 0), (2, 1, "seat", 1), (5, 2, "seat", 2), (9, 1, "release", None)]
    table, _ = SL.timetable(sched, 14, 3, limit=T)

    def feed(call):
        win = [0 if c is None else c[1] for c in table[call]]
        rec = [0 if c is None else c[0] for c in table[call]]
        return ({m: torch.stack([x[m][r, w] for r, w in zip(rec, win)]) for m in mods},
                torch.stack([mask[r, w] for r, w in zip(rec, win)]))

    z = model.slot_stream(3, T)
    got = _run_schedule(z, sched, 14, feed)
    assert _positions(z) == [12, -1, 9] and z.full().cpu().tolist() == [True, False, False]
    assert table[12][0] is None and table[11][0] == (0, 11)
    _against_forward("MFT slots", got, table, want, lengths)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["mft_stream_modalities", "b3_stream"])
def test_wrapper_slots_stream_against_its_batch_forward(dev, which):
    """the window encoder in front (T = 5): slot_stream of MultiCNNTransformerMFT and MultiCNNTransformerB3, recording 1 seated one
    call after recording 0, each against the wrapper's own eval forward of that recording alone"""
    m = mta()
    MT, MM = m.multiTransformer, m.models
    T, lengths, W = 5, [5, 3], 3
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    if which == "mft_stream_modalities":
        model = MM.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=dev)
        model.Transformer = MT.MultiTransformer(mods, model.window_embed_size, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32})
    else:
        model = MM.MultiCNNTransformerB3(mods, dims, device=dev)
    load_named(model)
    MT.causal_attention(model)
    model.eval()
    x = {mod: R.gen_normal("gpu_slot_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = [model({mod: x[mod][r:r + 1] for mod in mods}, lengths[r:r + 1], mask[r:r + 1]).cpu()[0] for r in range(2)]
    sched = [(0, 0, "seat", 0), (1, 1, "seat", 1)]
    table, _ = SL.timetable(sched, 6, 2, limit=T if which == "mft_stream_modalities" else None)

    def feed(call):
        win = [0 if c is None else min(c[1], T - 1) for c in table[call]]
        return ({mod: torch.stack([x[mod][r, w] for r, w in enumerate(win)]) for mod in mods},
                torch.stack([mask[r, w] for r, w in enumerate(win)]))

    z = model.slot_stream(2, T)
    with pytest.raises(AttributeError, match=r"\.positions"):
        z.t
    got = _run_schedule(z, sched, 6, feed)
    if which == "mft_stream_modalities":
        assert _positions(z) == [5, 5] and z.full().all() and (got[5, 0] == 0).all()
    else:                                                    # no cache, no limit: recording 0 went on to a sixth window
        assert _positions(z) == [6, 5] and not z.full().any()
    _against_forward("wrapper slots %s" % which, got, table, want, lengths, beyond=() if which == "mft_stream_modalities" else ((5, 0),))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. refusals before any launch
def _refused(call, exc, match):
    def run():
        with pytest.raises(exc, match=match):
            call()
    return device_kernel_names(run)[1]


def test_refusals_come_before_any_launch(dev):
    from multimodal_transformer_amd import graphs
    m = mta()
    MT, MM, F = m.multiTransformer, m.models, m.functional
    enc, _ = _encoder(32, 2, 1, dev, 3)
    opened = enc.slot_stream(2, 4)
    host = enc.stream(2, 4)
    x = torch.zeros(2, 32, device=dev)
    gate, _ = _gate(GATE_CASES[1], dev)
    gopen, ghost = gate.slot_stream(2), gate.stream(2)
    xs = [torch.zeros(2, 12, device=dev), torch.zeros(2, 16, device=dev)]
    sft = MT.NLPTransformer(48, embed_dim=40, h=4, N=1, device=dev).eval()
    uni = MT.UniTransformer(48, embed_dim=40, h=4, N=1, device=dev).eval()
    b2 = MT.UniFullTransformer(48, embed_dim=40, h=4, N=1, device=dev).eval()
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    wsft = MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=dev).eval()
    wb2 = MM.MultiCNNTransformerB2(["emotient"], {"emotient": 8}, device=dev).eval()
    one = MM.MultiCNNTransformerMFT(["emotient"], {"emotient": 8}, {"emotient": 16}, device=dev).eval()
    for model in (sft, uni, b2, wsft, wb2, one):
        MT.causal_attention(model)
    causal, _, wes = _small_mft(dev)
    noncausal = MT.MultiTransformer(mods, wes, N=1, h=2, device=dev, embed_dim={"acoustic": 32, "emotient": 16}).eval()

    def enc_step(positions):
        return F.encoder_stream_step_slots(x, None, opened._flat, opened.state, positions, opened.h, opened.d_ff, opened.n_layers, 4)

    def gate_step(positions):
        return F.mfn_stream_step_slots(xs, None, gopen.state, positions, gopen.in_dims, gopen.hidden, 1)

    narrow, mask3 = x[:, :16].contiguous(), torch.ones(3, device=dev)                    # made here: the refused calls launch nothing
    i32 = dict(dtype=torch.int32, device=dev)
    bad = [torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32), torch.zeros(3, **i32),
           torch.zeros(4, **i32)[::2], torch.zeros(2, 1, **i32)]
    torch.cuda.synchronize()
    calls = [((lambda mdl: (lambda: mdl.slot_stream(2, 4)))(mdl), NotImplementedError, "host-side state") for mdl in (sft, uni, b2, wsft, wb2, one)]
    calls += [((lambda p: (lambda: enc_step(p)))(p), ValueError, "positions must be") for p in bad]
    calls += [((lambda p: (lambda: gate_step(p)))(p), ValueError, "positions must be") for p in bad]
    calls += [(lambda: enc.train().slot_stream(2, 4), ValueError, r"\.eval\(\)"),
              (lambda: gate.train().slot_stream(2), ValueError, r"\.eval\(\)"),
              (lambda: causal.train().slot_stream(2, 4), ValueError, r"\.eval\(\)"),
              (lambda: noncausal.slot_stream(2, 4), ValueError, r"causal_attention\(model\)"),
              (lambda: enc.slot_stream(2, 4097), ValueError, "capacity"),
              (lambda: opened.step(narrow), ValueError, "shape"),
              (lambda: opened.step(x, mask3), ValueError, "mask_t"),
              (lambda: graphs.capture_stream(host, x), ValueError, r"slot_stream\("),
              (lambda: graphs.capture_stream(ghost, {"acoustic": xs[0], "emotient": xs[1]}), ValueError, r"slot_stream\(")]
    for call, exc, match in calls:
        names = _refused(call, exc, match)
        assert not names, (match, names)
        enc.eval(), gate.eval(), causal.eval()
    assert _positions(opened) == [-1, -1] and host.t == 0
    torch.cuda.synchronize()
