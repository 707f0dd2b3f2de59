"""GPU: a stream opened from its history in one forward (csrc/step_prefill.h encoder_prefill_kernel / decoder_prefill_kernel,
mmt_*_stream_prefill, functional.*_stream_prefill and ``prefill`` of the stream classes).

The reference is tests/prefill_ref.py: the batch path's reference over the history, its K and V handed to the step's reference, which
steps on (tests/test_prefill_cpu.py holds it to the exact function).  Rows t >= P are held to it under the bounds of
tests/test_gpu_bf16_faithful.py, imported: per product the arithmetic is that of the two paths the reference composes.  Against the
fully stepped stream on the GPU the bound grows by the distance D between prefill_ref and stream_ref (ring_stream_ref), computed here
on the CPU for each case; nothing is bounded by the code under test alone.  The cache a prefill fills holds the BATCH path's K and V,
so what it returns for the prefix, and every exact fact below, is bit for bit.
"""
import pytest
import torch

import prefill_ref as PF
import recipe as R
import ring_stream_ref as RS
import stream_ref as S
from conftest import rel_l2
from gpu_harness import (FILLS, OUT_RTOL, FilledPoolGet, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named,  # noqa: F401
                         measures, mta, seeded_encoder)
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW
from test_gpu_stream import _small_model

pytestmark = pytest.mark.gpu

# (d, h, N, P, T, lengths at prefill): the smallest shapes that reach each branch, a step reading the cache after the prefill
CASES = [(32, 4, 1, 1, 3, [1]),                      # d_k = 8: DKP 16 against dkp 8, one chunk
         (40, 4, 2, 33, 45, [33, 17, 1]),            # d_k = 10: pad columns, tile edge 32 / 33
         (128, 8, 2, 32, 70, [32, 9, 1]),            # the fixed-shape chains, P exactly one tile
         (80, 2, 1, 5, 9, [5, 2]),                   # d_k = 40: DKP 64 against dkp 40, five of eight chunks
         (256, 4, 1, 33, 40, [33, 2]),               # d_k = 64, the d = 256 chains
         (64, 2, 3, 70, 75, [70, 40, 1])]            # three layers, more than two tiles
IDS = ["d%d_h%d_n%d_P%d" % c[:4] for c in CASES]
# (d, h, N, span, P): P <, =, > span; a span above one tile; span 1
RING = [(40, 4, 2, 5, 3), (40, 4, 2, 5, 5), (40, 4, 2, 5, 13), (128, 8, 2, 33, 70), (40, 4, 2, 1, 4)]
RING_IDS = ["d%d_h%d_n%d_span%d_P%d" % c for c in RING]
RING_MORE = 7                                        # windows stepped behind a ring's prefix: past the span's edge for span 5
_CACHE = {}


def _mask(B, P, T):
    """every window counts but one inside the history and one behind it (where the case has room): a blanked query row on both paths"""
    m = torch.ones(B, T, 1)
    if P > 2:
        m[0, P // 2] = 0
    if T - P > 1:
        m[B - 1, T - 1] = 0
    return m


def _steps(stream, x, mask, t0, t1):
    """windows t0 .. t1 - 1 of x through a host stream -> (B, t1 - t0, ...) on the CPU"""
    rows = [stream.step(x[:, t], mask[:, t]) for t in range(t0, t1)]
    return torch.stack(rows, dim=1).cpu() if rows else torch.zeros(x.shape[0], 0, x.shape[2])


def _slot_steps(stream, x, mask, starts, T):
    """every slot from its own position until it stands at T: call j hands slot b window starts[b] + j -> per slot (T - starts[b], ...)
    on the CPU.  A slot behind T is full where the stream has a capacity (a zero row); its input is window T - 1 again."""
    B = len(starts)
    out = [[] for _ in range(B)]
    for j in range(T - min(starts)):
        at = [min(starts[b] + j, T - 1) for b in range(B)]
        y = stream.step(torch.stack([x[b, at[b]] for b in range(B)]), torch.stack([mask[b, at[b]] for b in range(B)])).cpu()
        for b in range(B):
            if starts[b] + j < T:
                out[b].append(y[b])
            elif stream.capacity is not None:
                assert (y[b] == 0).all()
    return [torch.stack(o) if o else None for o in out]


def _run(c, dev):
    """every GPU result and the CPU references of one plain case, computed once"""
    if c[:4] in _CACHE:
        return _CACHE[c[:4]]
    d, h, n, P, T, lengths = c
    B = len(lengths)
    MT = mta().multiTransformer
    enc, p32 = seeded_encoder(d, h, n, dev, 29)
    MT.causal_attention(enc)
    x = R.gen_normal("gpu_prefill_d%d_P%d:x" % (d, P), (B, T, d), 29)
    mask = _mask(B, P, T)
    m_slots = mask.clone()                                       # the slots form: the prefix mask of the lengths, then the windows' own
    for b, nb in enumerate(lengths):
        m_slots[b, :nb] = 1
    xg, mg, msg = x.to(dev), mask.to(dev), m_slots.to(dev)
    xp, mp = xg[:, :P].contiguous(), mg[:, :P].contiguous()
    out = {"enc": enc, "x": xg, "mask": mg, "m_slots": msg, "xp": xp, "mp": mp}
    with torch.no_grad():
        out["head_want"] = enc(xp, mp).cpu()
    s = enc.stream(B, T)
    out["head"] = s.prefill(xp, mp).cpu()
    assert s.t == P
    out["host"] = _steps(s, xg, mg, P, T)
    assert s.t == T
    s.reset()
    assert s.t == 0
    s.prefill(xp, mp)
    out["after_reset"] = _steps(s, xg, mg, P, T)
    s2 = enc.stream(B, T)
    s2.prefill(xp, mp)
    out["again"] = _steps(s2, xg, mg, P, T)
    out["stepped"] = _steps(enc.stream(B, T), xg, mg, 0, T)
    ss = enc.slot_stream(B, T)
    out["slots_head"] = ss.prefill(list(range(B)), xp, lengths).cpu()            # mask: the prefix mask of the lengths
    out["positions"] = ss.positions.cpu()
    out["slots"] = _slot_steps(ss, xg, msg, lengths, T)
    st = enc.slot_stream(B, T)
    st.reset()
    out["slots_stepped"] = _slot_steps(st, xg, msg, [0] * B, T)
    torch.cuda.synchronize()
    pd = {k: v.double() for k, v in p32.items()}
    xd, md, msd = x.double(), mask.double(), m_slots.double()
    out["ref_host"] = PF.encoder_rows(pd, "", h, xd, md, [P] * B, P).numpy()
    out["ref_slots"] = PF.encoder_rows(pd, "", h, xd, msd, lengths, P).numpy()
    out["ref_stepped"] = S.encoder_stack(pd, "", xd, md, h).numpy()
    out["ref_slots_stepped"] = S.encoder_stack(pd, "", xd, msd, h).numpy()
    _CACHE[c[:4]] = out
    return out


def _ragged(rows, lengths, ref=None):
    """the rows t >= lengths[b] of every sequence, one under the other: from the per-slot lists of _slot_steps, or cut out of a (B, T, d)
    reference"""
    if ref is None:
        return torch.cat([r for r in rows if r is not None]).numpy()
    return torch.cat([torch.as_tensor(ref[b, nb:]) for b, nb in enumerate(lengths)]).numpy()


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_prefilled_stream_against_the_prefill_reference(dev, c):
    """rows t >= P of the host form, and rows t >= len[b] of the slots form with ragged lengths, against prefill_ref under ENC_OUT 2e-3 /
    ENC_OUT_ROW 8e-3 (rel-L2 / per-row maximum).  Measured worst over the cases on the MI355X: 5.1e-4 / 1.5e-3 (d 128, host form);
    the cases in which fp32 noise tips no bf16 rounding (d 32, d 40, d 80) sit at 1e-7."""
    r = _run(c, dev)
    P, lengths = c[3], c[5]
    check("prefill %s host rows" % IDS[CASES.index(c)], r["host"], r["ref_host"][:, P:], ENC_OUT, ENC_OUT_ROW)
    check("prefill %s slots rows" % IDS[CASES.index(c)], _ragged(r["slots"], lengths), _ragged(None, lengths, r["ref_slots"]), ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_prefilled_stream_against_the_stepped_stream(dev, c):
    """the same rows against the fully stepped GPU stream.  The history's K and V come from the batch path's layers in one and from the
    step's in the other, so the bound is ENC_OUT + D and ENC_OUT_ROW + D_row, D the distance between prefill_ref and stream_ref for this
    case (triangle inequality), computed here on the CPU.
    Measured worst: 1.40e-3 / 2.03e-3 (d 64) with D = 1.405e-3 / 2.033e-3, and 9.7e-4 / 2.35e-3 (d 128) with D = 9.5e-4 / 2.375e-3: the
    distance is the references', not the kernels'.  D is exactly 0 where one key tile makes the two rules coincide (d 32, d 80, d 256)."""
    r = _run(c, dev)
    P, lengths = c[3], c[5]
    D, D_row = measures(r["ref_host"][:, P:], r["ref_stepped"][:, P:])
    print("prefill %s: distance of the two references rel-L2 %.3e per-row %.3e" % (IDS[CASES.index(c)], D, D_row))
    check("prefill %s host vs stepped" % IDS[CASES.index(c)], r["host"], r["stepped"][:, P:], ENC_OUT + D, ENC_OUT_ROW + D_row)
    a, b = _ragged(None, lengths, r["ref_slots"]), _ragged(None, lengths, r["ref_slots_stepped"])
    D, D_row = measures(a, b)
    print("prefill %s slots: distance of the two references rel-L2 %.3e per-row %.3e" % (IDS[CASES.index(c)], D, D_row))
    stepped = [None if s is None else s[nb:] for s, nb in zip(r["slots_stepped"], lengths)]
    check("prefill %s slots vs stepped" % IDS[CASES.index(c)], _ragged(r["slots"], lengths),
          torch.cat([s for s in stepped if s is not None and len(s)]).numpy(), ENC_OUT + D, ENC_OUT_ROW + D_row)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. exact facts, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_returned_rows_are_the_batch_forwards(dev, c):
    r = _run(c, dev)
    assert torch.isfinite(r["head"]).all() and torch.equal(r["head"], r["head_want"])
    with torch.no_grad():
        want = r["enc"](r["xp"], mta().functional.prefill_table("t", range(len(c[5])), c[5], c[3], len(c[5]), None, dev)[2]).cpu()
    assert torch.equal(r["slots_head"], want)
    s = r["enc"].stream(len(c[5]), c[4])                          # a strided view of the recording: the same bits
    assert torch.equal(s.prefill(r["x"][:, :c[3]], r["mask"][:, :c[3]]).cpu(), r["head"]) and s.t == c[3]
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_two_recordings_and_a_reset_give_the_same_bits(dev, c):
    r = _run(c, dev)
    assert torch.isfinite(r["host"]).all()
    assert torch.equal(r["host"], r["again"])                     # a second, fresh stream
    assert torch.equal(r["host"], r["after_reset"])               # the same stream after reset(): nothing was cleared or re-read
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_positions_after_a_slots_prefill(dev, c):
    """positions equal the lengths at the indices and are unchanged elsewhere (a stream of two more slots, one idle and one seated far)"""
    r = _run(c, dev)
    lengths = c[5]
    assert r["positions"].tolist() == lengths
    B = len(lengths)
    ss = r["enc"].slot_stream(B + 2, c[4])
    ss.seat([B + 1])
    ss.positions[B + 1] = 3
    idx = list(range(B - 1, -1, -1))                              # a permuted, partial dst
    ss.prefill(idx, r["xp"].flip(0).contiguous(), lengths[::-1])
    assert ss.positions.tolist() == lengths + [-1, 3]
    torch.cuda.synchronize()


def test_a_prefill_to_capacity_leaves_the_stream_full(dev):
    r = _run(CASES[1], dev)
    B, P = len(CASES[1][5]), CASES[1][3]
    s = r["enc"].stream(B, P)
    s.prefill(r["xp"], r["mp"])
    assert s.t == P == s.capacity
    with pytest.raises(ValueError, match="full"):
        s.step(r["x"][:, P], r["mask"][:, P])
    ss = r["enc"].slot_stream(B, P)
    ss.prefill([1], r["xp"][:1], [P])
    assert ss.full().tolist() == [False, True, False]
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_a_slot_prefilled_alone_is_the_host_stream_of_that_recording(dev, c):
    """prefill([i], x1, [P]) and steps: the bits of a host stream of that recording alone after prefill(x1) (the same forward dims, then
    the slot-equals-alone guarantee of the step)"""
    r = _run(c, dev)
    P, T, B = c[3], c[4], len(c[5])
    x1, m1 = r["xp"][1:2].contiguous(), r["mp"][1:2].contiguous()
    alone = r["enc"].stream(1, T)
    head = alone.prefill(x1, m1).cpu()
    want = _steps(alone, r["x"][1:2], r["mask"][1:2], P, T)
    ss = r["enc"].slot_stream(B, T)
    got_head = ss.prefill([2 % B], x1, [P], m1).cpu()
    assert torch.equal(got_head, head)
    rows = []
    for t in range(P, T):
        xt = torch.zeros(B, c[0], device=dev)
        xt[2 % B] = r["x"][1, t]
        mt = torch.ones(B, device=dev)
        mt[2 % B] = r["mask"][1, t, 0]
        rows.append(ss.step(xt, mt)[2 % B].cpu())
    assert torch.equal(torch.stack(rows), want[0])
    torch.cuda.synchronize()


def _cache_view(stream):
    """the K/V cache of an encoder stream's state as int16 (N, 2, B, h, rows, dkp) and the bytes in front of it (the prepared weights)"""
    rows = stream.span if stream.capacity is None else stream.capacity
    dkp = (stream.d // stream.h + 7) // 8 * 8
    elems = stream.n_layers * 2 * stream.batch * stream.h * rows * dkp
    tail = (elems * 2 + 255) // 256 * 256
    off = stream.state.numel() - tail
    assert mta().functional.encoder_stream_bytes(stream.batch, rows, stream.d, stream.h, stream.d_ff, stream.n_layers) == stream.state.numel()
    return stream.state[off:off + 2 * elems].view(torch.int16).view(stream.n_layers, 2, stream.batch, stream.h, rows, dkp), stream.state[:off]


def test_a_neighbour_is_untouched(dev):
    """slot 0 steps a recording; between two of its steps slot 2 is prefilled (indices [2], then [2, 1] in that order): slot 0's rows are
    those of the run without any prefill, and of the state only the rows < len of the named slots changed, not a byte else"""
    c = CASES[1]
    r = _run(c, dev)
    d, P, T, B = c[0], c[3], c[4], 3
    x0, m0 = r["x"][0], r["mask"][0]

    def record(prefills):
        ss = r["enc"].slot_stream(B, T)
        ss.seat([0])
        rows = []
        for t in range(12):
            if t in prefills:
                idx, lens = prefills[t]
                before = ss.state.clone()
                ss.prefill(idx, r["xp"][:len(idx)], lens)
                cache0, weights0 = _cache_view(type("S", (), dict(vars(ss), state=before, capacity=ss.capacity))())
                cache1, weights1 = _cache_view(ss)
                assert torch.equal(weights0, weights1)
                changed = (cache0 != cache1).any(dim=-1).any(dim=0).any(dim=0).any(dim=1)          # (B, rows)
                allowed = torch.zeros_like(changed)
                for i, nb in zip(idx, lens):
                    allowed[i, :nb] = True
                assert not (changed & ~allowed).any()
                assert ss.positions.tolist()[0] == t
            xt = torch.zeros(B, d, device=dev)
            xt[0] = x0[t]
            mt = torch.ones(B, device=dev)
            mt[0] = m0[t, 0]
            rows.append(ss.step(xt, mt)[0].cpu())
        return torch.stack(rows)

    want = record({})
    got = record({3: ([2], [P]), 7: ([2, 1], [5, P])})
    assert torch.isfinite(want).all() and torch.equal(got, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_state_may_hold_any_contents(dev, c, fill):
    """the whole state filled with each pattern before refresh() + prefill: the later rows have the same bits.  This pins the zeros of
    the pad columns (d_k = 10, 40: dkp > d_k) and that no row the prefill did not write is read."""
    r = _run(c, dev)
    s = r["enc"].stream(len(c[5]), c[4])
    before = s.state.clone()
    fill_bytes(s.state.view(-1), fill)
    assert not torch.equal(before, s.state)
    s.refresh()
    s.prefill(r["xp"], r["mp"])
    assert torch.equal(_steps(s, r["x"], r["mask"], c[3], c[4]), r["host"])
    ss = r["enc"].slot_stream(len(c[5]), c[4])
    fill_bytes(ss.state.view(-1), fill)
    ss.refresh()
    ss.prefill(list(range(len(c[5]))), r["xp"], c[5])
    for got, want in zip(_slot_steps(ss, r["x"], r["m_slots"], c[5], c[4]), r["slots"]):
        assert (got is None and want is None) or torch.equal(got, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
def test_the_workspace_may_hold_any_contents(dev, fill, monkeypatch):
    """the pool workspace of the prefill's forward filled with each pattern before it is handed out: the returned rows and the later rows
    have the same bits.  The shape is d = 128, P = 32: d, d_ff, h x DKP and P are whole tiles there, so the forward has no pad row or
    column that it reads without writing.  Elsewhere the pool's contract is "zero at creation, never written" for such pads
    (_lib.WorkspacePool), the forward relies on it, and its own rows change under a fill (measured: d = 40 / P = 33 and d = 80 / P = 5
    with the 0xFF and the bf16 +Inf fill); those shapes are held to the contract the pool does give in the next test."""
    c = CASES[2]
    r = _run(c, dev)
    pool = mta()._lib.POOL
    pool.clear()                                                  # a buffer of this tag that is handed out below is new or filled
    sub = FilledPoolGet(pool.get, fill, "encoder")
    monkeypatch.setattr(pool, "get", sub)
    s = r["enc"].stream(len(c[5]), c[4])
    head = s.prefill(r["xp"], r["mp"]).cpu()
    monkeypatch.undo()
    pool.clear()                                                  # nobody after this test is handed a filled buffer
    assert sub.calls == 1
    assert torch.equal(head, r["head"])
    assert torch.equal(_steps(s, r["x"], r["mask"], c[3], c[4]), r["host"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_a_workspace_another_call_left_dirty(dev, c, monkeypatch):
    """the pool's own contract at the shapes with pads: a prefill of the same dims whose history holds Inf and NaN leaves them in K and V
    of the workspace; the next prefill is handed that very buffer and gives the bits of a run on a fresh pool"""
    r = _run(c, dev)
    pool = mta()._lib.POOL
    pool.clear()
    got = []
    real = pool.get

    def get(nbytes, device, tag=None):
        buf = real(nbytes, device, tag=tag)
        if tag is not None and tag[0] == "encoder":
            got.append(buf.data_ptr())
        return buf

    monkeypatch.setattr(pool, "get", get)
    B, T = len(c[5]), c[4]
    dirty = r["xp"].clone()
    dirty[0, 0, 0], dirty[B - 1, c[3] - 1, 1] = float("inf"), float("nan")
    r["enc"].stream(B, T).prefill(dirty, r["mp"])
    s = r["enc"].stream(B, T)
    head = s.prefill(r["xp"], r["mp"]).cpu()
    monkeypatch.undo()
    pool.clear()
    assert len(got) == 2 and got[0] == got[1]
    assert torch.equal(head, r["head"])
    assert torch.equal(_steps(s, r["x"], r["mask"], c[3], c[4]), r["host"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the ring
def _ring_run(c, dev):
    if ("ring",) + c in _CACHE:
        return _CACHE[("ring",) + c]
    d, h, n, span, P = c
    T, B = P + RING_MORE, 3
    lengths = [P, (P + 1) // 2, 1]
    MT = mta().multiTransformer
    enc, p32 = seeded_encoder(d, h, n, dev, 31)
    MT.causal_attention(enc, span=span)
    x = R.gen_normal("gpu_prefill_ring_d%d_s%d_P%d:x" % (d, span, P), (B, T, d), 31)
    mask = _mask(B, P, T)
    m_slots = mask.clone()
    for b, nb in enumerate(lengths):
        m_slots[b, :nb] = 1
    xg, mg, msg = x.to(dev), mask.to(dev), m_slots.to(dev)
    xp, mp = xg[:, :P].contiguous(), mg[:, :P].contiguous()
    out = {"enc": enc, "lengths": lengths}
    with torch.no_grad():
        out["head_want"] = enc(xp, mp).cpu()
    s = enc.ring_stream(B)
    out["head"] = s.prefill(xp, mp).cpu()
    assert s.t == P and s.capacity is None
    out["host"] = _steps(s, xg, mg, P, T)
    s2 = enc.ring_stream(B)
    for fill in FILLS[1:2]:                                       # a ring row that the prefill did not write is never read
        fill_bytes(s2.state.view(-1), fill)
    s2.refresh()
    s2.prefill(xp, mp)
    out["again"] = _steps(s2, xg, mg, P, T)
    out["stepped"] = _steps(enc.ring_stream(B), xg, mg, 0, T)
    ss = enc.ring_slot_stream(B)
    ss.prefill([2, 0, 1], xp[[1, 2, 0]].contiguous(), [lengths[1], lengths[2], lengths[0]])       # row i fills slot idx[i]
    out["positions"] = ss.positions.cpu()
    out["slots"] = _slot_steps(ss, xg[[2, 0, 1]], msg[[2, 0, 1]], [lengths[2], lengths[0], lengths[1]], T)
    torch.cuda.synchronize()
    pd = {k: v.double() for k, v in p32.items()}
    xd, md, msd = x.double(), mask.double(), m_slots.double()
    out["ref_host"] = PF.encoder_rows(pd, "", h, xd, md, [P] * B, P, span).numpy()
    out["ref_slots"] = PF.encoder_rows(pd, "", h, xd[[2, 0, 1]], msd[[2, 0, 1]], [lengths[2], lengths[0], lengths[1]], P, span).numpy()
    out["ref_stepped"] = RS.encoder_stack(pd, "", xd, md, h, span).numpy()
    _CACHE[("ring",) + c] = out
    return out


@pytest.mark.parametrize("c", RING, ids=RING_IDS)
def test_ring_prefill(dev, c):
    """a ring of span rows filled with the last min(len, span) windows of each history (P <, =, > span; span 33 with P = 70; span 1): the
    returned rows are the band forward's, bit for bit; rows t >= P (t >= len[b] in the permuted slots form) against prefill_ref under
    ENC_OUT / ENC_OUT_ROW and against the stepped ring stream under ENC_OUT + D, ENC_OUT_ROW + D_row, D between prefill_ref and
    ring_stream_ref; a state of any contents gives the same bits.
    Measured worst: 7.4e-4 / 2.0e-3 against the reference (d 128, span 33); 1.06e-3 / 1.64e-3 against the stepped ring with D = 1.03e-3 /
    1.41e-3 (the same case)."""
    r = _ring_run(c, dev)
    P, tag = c[4], RING_IDS[RING.index(c)]
    lens = [r["lengths"][2], r["lengths"][0], r["lengths"][1]]
    assert torch.equal(r["head"], r["head_want"]) and torch.equal(r["host"], r["again"])
    assert r["positions"].tolist() == lens
    check("ring prefill %s host rows" % tag, r["host"], r["ref_host"][:, P:], ENC_OUT, ENC_OUT_ROW)
    check("ring prefill %s slots rows" % tag, _ragged(r["slots"], lens), _ragged(None, lens, r["ref_slots"]), ENC_OUT, ENC_OUT_ROW)
    D, D_row = measures(r["ref_host"][:, P:], r["ref_stepped"][:, P:])
    print("ring prefill %s: distance of the two references rel-L2 %.3e per-row %.3e" % (tag, D, D_row))
    check("ring prefill %s host vs stepped" % tag, r["host"], r["stepped"][:, P:], ENC_OUT + D, ENC_OUT_ROW + D_row)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. models
M_T, M_P, M_LENGTHS = 20, 11, [20, 7, 1]


def _model_inputs(kind, dev):
    x = R.gen_normal("gpu_prefill_model_%s:x" % kind, (3, M_T, 48), 5).to(dev)
    return x, R.prefix_mask(M_LENGTHS, M_T).to(dev), [min(n, M_P) for n in M_LENGTHS]


@pytest.mark.parametrize("form", ["stream", "device_stream"])
@pytest.mark.parametrize("kind", ["sft", "b2", "uni"])
def test_sequence_model_prefill_against_its_batch_forward(dev, kind, form):
    """T = 20, P = 11, lengths [20, 7, 1] clipped to P at prefill: what prefill returns is the model's eval forward over the prefix, bit
    for bit; rows t >= P (device_stream: t >= the slot's own length) against the model's eval forward over all T under OUT_RTOL; padded
    windows are exact zeros.
    Measured (both forms alike): sft 1.02e-2, b2 3.3e-3, uni 5.5e-3."""
    model = _small_model(kind, dev)
    x, mask, clipped = _model_inputs(kind, dev)
    xp, mp = x[:, :M_P].contiguous(), mask[:, :M_P].contiguous()
    with torch.no_grad():
        want = model(x, mask, M_LENGTHS).cpu()
        head_want = model(xp, mp, clipped).cpu()
    if form == "stream":
        s = model.stream(3, M_T)
        head = s.prefill(xp, mp).cpu()
        assert s.t == M_P
        got = torch.stack([s.step(x[:, t], mask[:, t]) for t in range(M_P, M_T)], dim=1).cpu()
        ref, starts = want[:, M_P:], [M_P] * 3
        rows = [got[b] for b in range(3)]
    else:
        s = model.device_stream(3, M_T)
        head = s.prefill([0, 1, 2], xp, clipped, mp).cpu()
        assert s.positions.tolist() == clipped
        rows, starts = _slot_steps(s, x, mask, clipped, M_T), clipped
    assert head.shape == (3, M_P, 1) and torch.equal(head, head_want)
    got = torch.cat(rows).numpy()
    ref = torch.cat([want[b, starts[b]:] for b in range(3)]).numpy()
    err = rel_l2(got, ref)
    print("prefill model %s %s: rel_l2 %.3e" % (kind, form, err))
    assert torch.isfinite(torch.cat(rows)).all() and err <= OUT_RTOL
    for b, n in enumerate(M_LENGTHS):
        assert (rows[b][max(n - starts[b], 0):] == 0).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["stream", "device_stream"])
@pytest.mark.parametrize("which", ["sft_two_modalities", "b2_one_modality"])
def test_wrapper_prefill_against_its_batch_forward(dev, which, form):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    T, P, lengths, W = 7, 4, [7, 3], 3
    if which == "sft_two_modalities":
        mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
        model = MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=dev)
        model.Transformer = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    else:
        mods, dims = ["emotient"], {"emotient": 8}
        model = MM.MultiCNNTransformerB2(mods, dims, device=dev)
        model.Transformer = MT.UniFullTransformer(20, embed_dim=40, h=4, N=2, device=dev)
    load_named(model)
    MT.causal_attention(model)
    model.eval()
    x = {mod: R.gen_normal("gpu_prefill_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    clipped = [min(n, P) for n in lengths]
    xp, mp = {mod: x[mod][:, :P].contiguous() for mod in mods}, mask[:, :P].contiguous()
    with torch.no_grad():
        want = model(x, lengths, mask).cpu()
        head_want = model(xp, clipped, mp).cpu()
    if form == "stream":
        s = model.stream(2, T)
        head = s.prefill(xp, mask=mp).cpu()
        starts = [P, P]
    else:
        s = model.device_stream(2, T)
        head = s.prefill([0, 1], xp, clipped, mask=mp).cpu()
        starts = clipped
    assert torch.equal(head, head_want)
    rows = [[] for _ in starts]
    for j in range(T - min(starts)):
        at = [min(st + j, T - 1) for st in starts]
        y = s.step({mod: torch.stack([x[mod][b, at[b]] for b in range(2)]) for mod in mods},
                   torch.stack([mask[b, at[b]] for b in range(2)])).cpu()
        for b in range(2):
            if starts[b] + j < T:
                rows[b].append(y[b])
    got = torch.cat([torch.stack(r) for r in rows]).numpy()
    ref = torch.cat([want[b, starts[b]:] for b in range(2)]).numpy()
    err = rel_l2(got, ref)
    print("prefill wrapper %s %s: rel_l2 %.3e" % (which, form, err))
    assert err <= OUT_RTOL
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["sft", "b2"])
def test_ring_stream_of_a_model_prefills(dev, kind):
    """ring_stream(model, batch, slots=...) returns streams whose prefill works the same way, with no limit on P (P = 11 > span = 4): the
    returned rows are the model's forward over the prefix, bit for bit, and the positions are the lengths.  Rows t >= P are held to the
    fully STEPPED ring stream of the same model: with a span every K and V a row reads lies at most N (span - 1) = 6 windows back, so from
    t = P + 6 on nothing the batch path computed reaches the encoder's row, and for the model without a decoder ("b2") the prefilled and
    the stepped stream agree bit for bit there.  The LSTM decoder ("sft") carries its state through, so it is held to the model's eval
    forward as the stepped stream is: neither may be further from it than OUT_RTOL plus the other's distance (triangle inequality)."""
    m = mta()
    MT = m.multiTransformer
    x, mask, clipped = _model_inputs(kind, dev)
    model = (MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev) if kind == "sft"
             else MT.UniFullTransformer(48, embed_dim=128, h=8, N=2, device=dev))
    load_named(model)
    MT.causal_attention(model, span=4)
    model.eval()
    mask = torch.ones_like(mask)                                  # every window counts: the tail is compared bit for bit
    xp, mp = x[:, :M_P].contiguous(), mask[:, :M_P].contiguous()
    with torch.no_grad():
        want = model(x, mask, [M_T] * 3).cpu()
        head_want = model(xp, mp, [M_P] * 3).cpu()
    s = m.streaming.ring_stream(model, 3)
    assert torch.equal(s.prefill(xp, mp).cpu(), head_want) and s.t == M_P and s.capacity is None
    got = torch.stack([s.step(x[:, t], mask[:, t]) for t in range(M_P, M_T)], dim=1).cpu()
    full = m.streaming.ring_stream(model, 3)
    stepped = torch.stack([full.step(x[:, t], mask[:, t]) for t in range(M_T)], dim=1).cpu()[:, M_P:]
    e_pre, e_step = rel_l2(got.numpy(), want[:, M_P:].numpy()), rel_l2(stepped.numpy(), want[:, M_P:].numpy())
    print("prefill ring model %s: prefilled vs forward %.3e, stepped vs forward %.3e" % (kind, e_pre, e_step))
    assert torch.isfinite(got).all() and e_pre <= OUT_RTOL + e_step
    if kind == "b2":
        assert e_pre <= OUT_RTOL and torch.equal(got[:, 6:], stepped[:, 6:])
    ss = m.streaming.ring_stream(model, 3, slots=True)
    assert torch.equal(ss.prefill([0, 1, 2], xp, clipped, mp).cpu(), head_want) and ss.positions.tolist() == clipped
    rows = _slot_steps(ss, x, mask, clipped, M_T)
    e_slots = rel_l2(torch.cat(rows).numpy(), torch.cat([want[b, clipped[b]:] for b in range(3)]).numpy())
    print("prefill ring model %s slots: prefilled vs forward %.3e" % (kind, e_slots))
    assert e_slots <= OUT_RTOL + e_step
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. graphs and launches
def test_a_captured_step_replays_after_a_prefill(dev):
    """graphs.capture_stream of a device_stream captured BEFORE a prefill replays, after it, to the bits of the eager step"""
    m = mta()
    model = _small_model("sft", dev)
    x, mask, clipped = _model_inputs("sft", dev)
    xp, mp = x[:, :M_P].contiguous(), mask[:, :M_P].contiguous()
    s, eager = model.device_stream(3, M_T), model.device_stream(3, M_T)
    g = m.graphs.capture_stream(s, x[:, 0].contiguous(), mask[:, 0].contiguous())
    s.prefill([0, 1, 2], xp, clipped, mp)
    eager.prefill([0, 1, 2], xp, clipped, mp)
    for j in range(3):
        xt = torch.stack([x[b, clipped[b] + j] for b in range(3)])
        mt = torch.stack([mask[b, clipped[b] + j] for b in range(3)])
        g.inputs.copy_(xt)
        g.mask.copy_(mt)
        got = g.replay().clone()
        assert torch.equal(got, eager.step(xt, mt))
    assert s.positions.tolist() == eager.positions.tolist() == [n + 3 for n in clipped]
    torch.cuda.synchronize()


def test_a_prefill_launches_one_fill_kernel_and_no_library_kernel(dev):
    r = _run(CASES[1], dev)
    B, T = len(CASES[1][5]), CASES[1][4]
    r["enc"].stream(B, T).prefill(r["xp"], r["mp"])              # warm-up: the pool's workspace of this shape exists
    s, ss = r["enc"].stream(B, T), r["enc"].slot_stream(B, T)
    torch.cuda.synchronize()
    _, host = device_kernel_names(lambda: s.prefill(r["xp"], r["mp"]))
    _, slots = device_kernel_names(lambda: ss.prefill(list(range(B)), r["xp"], CASES[1][5]))
    model = _small_model("sft", dev)
    x, mask, clipped = _model_inputs("sft", dev)
    xp, mp = x[:, :M_P].contiguous(), mask[:, :M_P].contiguous()
    ds, hs = model.device_stream(3, M_T), model.stream(3, M_T)
    model.device_stream(3, M_T).prefill([0, 1, 2], xp, clipped, mp)      # warm-up: the pool's workspaces of these shapes exist
    model.stream(3, M_T).prefill(xp, mp)
    torch.cuda.synchronize()
    _, dnames = device_kernel_names(lambda: ds.prefill([0, 1, 2], xp, clipped, mp))
    _, hnames = device_kernel_names(lambda: hs.prefill(xp, mp))
    torch.cuda.synchronize()
    if host is None or slots is None or dnames is None or hnames is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    for tag, names in (("host", host), ("slots", slots), ("device_stream", dnames), ("stream", hnames)):
        print("prefill launches %s: %s" % (tag, [n[:60] for n in names]))
    for names, dec in ((host, 0), (slots, 0), (dnames, 1), (hnames, 0)):
        assert library_kernels(names) == [], names
        assert sum("encoder_prefill" in n for n in names) == 1, names
        assert sum("decoder_prefill" in n for n in names) == dec, names
    assert sum("encoder_step" in n for n in host + slots + dnames + hnames) == 0


# ------------------------------------------------------------------------------------------------ 6. refusals before any launch
def _refused(call, exc, match):
    def run():
        with pytest.raises(exc, match=match):
            call()
    return device_kernel_names(run)[1]


def test_refusals_come_before_any_launch(dev):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    r = _run(CASES[1], dev)
    enc, xp, mp = r["enc"], r["xp"], r["mp"]
    B, P, T, d = 3, CASES[1][3], CASES[1][4], CASES[1][0]
    host, small, slots = enc.stream(B, T), enc.stream(B, P - 1), enc.slot_stream(B, T)
    moved = enc.stream(B, T)
    moved.step(r["x"][:, 0], r["mask"][:, 0])
    slots.seat([1])
    sft = _small_model("sft", dev)
    seq, dseq = sft.stream(3, M_T), sft.device_stream(3, M_T)
    stacked = MT.NLPTransformer(48, embed_dim=40, h=4, N=1, n_layers=2, device=dev).eval()
    MT.causal_attention(stacked)
    dstacked = stacked.device_stream(3, M_T)
    xm = torch.zeros(3, M_P, 48, device=dev)
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    mfn = MT.MultiTransformer(mods, wes, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32}).eval()
    MT.causal_attention(mfn)
    gate, gate_slots, gate_alone = mfn.stream(2, 4), mfn.slot_stream(2, 4), mfn.mfn.stream(2)
    wrap = MM.MultiCNNTransformerMFT(mods, {"acoustic": 12, "emotient": 8}, {"acoustic": 16, "emotient": 16}, device=dev).eval()
    MT.causal_attention(wrap)
    wrapped = wrap.stream_modalities(2, 4)
    none, two, narrow, x64, xcpu, m5, xm40 = xp[:, :0], xp[:2], xp[:, :, :32].contiguous(), xp.double(), xp.cpu(), mp[:, :5], xm[:, :, :40].contiguous()
    torch.cuda.synchronize()
    calls = [(lambda: moved.prefill(xp, mp), ValueError, r"reset\(\)"),
             (lambda: small.prefill(xp, mp), ValueError, "capacity"),
             (lambda: host.prefill(none, None), ValueError, "P >= 1"),
             (lambda: host.prefill(two, None), ValueError, "shape"),
             (lambda: host.prefill(narrow, None), ValueError, "shape"),
             (lambda: host.prefill(x64, None), ValueError, "float32"),
             (lambda: host.prefill(xcpu, None), ValueError, "float32 tensor on"),
             (lambda: host.prefill(xp, m5), ValueError, "mask"),
             (lambda: slots.prefill([0, 0], xp[:2], [1, 1]), ValueError, "distinct"),
             (lambda: slots.prefill([3], xp[:1], [1]), ValueError, "distinct"),
             (lambda: slots.prefill([0], xp[:1], [P + 1]), ValueError, "lengths"),
             (lambda: slots.prefill([0], xp[:1], [0]), ValueError, "lengths"),
             (lambda: slots.prefill([0, 1], xp[:2], [1]), ValueError, "one length"),
             (lambda: slots.prefill([0, 1, 2, 1], xp, [1] * 4), ValueError, "slots"),
             (lambda: slots.prefill([0], xp[:2], [1]), ValueError, "shape"),
             (lambda: seq.prefill(xm40), ValueError, "shape"),
             (lambda: dseq.prefill([0, 4], xm[:2], [1, 1]), ValueError, "distinct"),
             (lambda: dstacked.prefill([0], xm[:1], [1]), NotImplementedError, "n_layers = 2"),
             (lambda: gate.prefill({}, None), NotImplementedError, "window 0"),
             (lambda: gate_slots.prefill([0], {}, [1]), NotImplementedError, "window 0"),
             (lambda: gate_alone.prefill({}, None), NotImplementedError, "window 0"),
             (lambda: wrapped.prefill({}), NotImplementedError, "window 0")]
    for call, exc, match in calls:
        names = _refused(call, exc, match)
        assert not names, (match, names)
    assert (host.t, small.t, moved.t, seq.t) == (0, 0, 1, 0)
    assert slots.positions.tolist() == [-1, 0, -1] and dseq.positions.tolist() == [-1, -1, -1]
    torch.cuda.synchronize()


def test_the_lstm_streams_refuse_a_prefill(dev):
    """the LSTM baselines' streams and the feedback streams open at window 0 only: NotImplementedError before any launch, t as it was"""
    MM = mta().models
    base = MM.MultiLSTM(24, embed_dim=16, h_dim=12, attn_len=4, device=dev).eval()
    ed = MM.MultiEDLSTM(24, embed_dim=16, h_dim=12, device=dev).eval()
    MM.attend_over_taps(base)
    MM.attend_over_taps(ed)
    streams = [base.stream(2), base.slot_stream(2), ed.feedback_stream(2), ed.feedback_slot_stream(2)]
    torch.cuda.synchronize()
    x = torch.zeros(2, 3, 24, device=dev)
    for s in streams:
        call = (lambda: s.prefill([0], x[:1], [3])) if s.slots else (lambda: s.prefill(x))
        assert not _refused(call, NotImplementedError, "window 0")
    assert streams[0].t == 0 and streams[2].t == 0 and streams[1].positions.tolist() == [-1, -1]
    torch.cuda.synchronize()
