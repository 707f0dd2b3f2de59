"""GPU: extend, a stream moved forward by C windows from any position, sixteen windows per launch (csrc/encoder_extend.h,
mmt_encoder_stream_extend*, streaming.encoder_stream_extend, EncoderStream.extend and the extend() of the sequence models' host
streams and their wrappers).

The references are tests/stream_ref.py (plain) and tests/ring_stream_ref.py (ring), the step's own rounding rule, which extend keeps
per row: only the fp32 summation order differs.  The bounds are ENC_OUT / ENC_OUT_ROW of tests/test_gpu_bf16_faithful.py, imported,
which the stepped stream already meets against the same references; against the stepped stream on the GPU the bound is twice that, by
the triangle inequality through the one reference.  A "grouping" is how a case's T windows are split into extend calls.
"""
import pytest
import torch

import prefill_ref as PF
import recipe as R
import ring_stream_ref as RS
import stream_ref as S
from conftest import rel_l2
from gpu_harness import (FILLS, OUT_RTOL, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named, mta,  # noqa: F401
                         seeded_encoder)
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW

pytestmark = pytest.mark.gpu

# (d, h, N, T, lengths; grouping)
PLAIN = [((32, 2, 1, 1, [1]), [1]),                                 # one key, capacity 1
         ((40, 4, 2, 45, [45, 30, 1]), [1, 16, 17, 11]),            # d_k = 10 padded; starts at t = 0, 1, 17, 34; a tile boundary inside a call; blank rows inside a tile
         ((128, 8, 2, 70, [70, 33, 1]), [33, 37]),                  # 16 + 16 + 1 rows in one call
         ((64, 2, 3, 130, [130, 86, 1]), [5, 64, 61]),              # d_k = 32, key counts crossing 64 and 128
         ((256, 4, 1, 33, [33, 2]), [32, 1]),                       # d_k = 64
         ((512, 8, 1, 3, [3]), [3])]                                # the widest row
PLAIN_IDS = ["d%d_h%d_n%d_T%d" % c[:4] for c, _ in PLAIN]
RING_T, RING_GROUPS, RING_LENGTHS = 70, [7, 16, 30, 17], [70, 46, 1]
RING = [(d, h, 2, span) for d, h in ((40, 4), (128, 8)) for span in (1, 5, 16, 33)]       # a span below, equal to and above the tile; a wrap inside a tile
RING_IDS = ["d%d_span%d" % (c[0], c[3]) for c in RING]
_CACHE = {}


def _extend_all(stream, x, mask, groups):
    """the windows of x through stream.extend, group by group -> (B, sum(groups), d) on the CPU"""
    rows, t = [], 0
    for g in groups:
        rows.append(stream.extend(x[:, t:t + g].contiguous(), mask[:, t:t + g].contiguous()))
        t += g
    return torch.cat(rows, dim=1).cpu()


def _step_all(stream, x, mask, t0, t1):
    return torch.stack([stream.step(x[:, t], mask[:, t]) for t in range(t0, t1)], dim=1).cpu()


def _encoder(d, h, n, span, dev):
    enc, p32 = seeded_encoder(d, h, n, dev, 17)
    MT = mta().multiTransformer
    if span is None:
        MT.causal_attention(enc)
    else:
        MT.causal_attention(enc, True, span=span)
    return enc, p32


def _open(enc, B, T, span):
    return enc.stream(B, T) if span is None else enc.ring_stream(B)


def _run(key, dev):
    """every GPU result and the CPU reference of one case, computed once.  key: (d, h, N, T, lengths, grouping, span)"""
    ident = (key[0], key[1], key[2], key[3], key[6])
    if ident in _CACHE:
        return _CACHE[ident]
    d, h, n, T, lengths, groups, span = key
    B = len(lengths)
    enc, p32 = _encoder(d, h, n, span, dev)
    x = R.gen_normal("gpu_extend_d%d_T%d:x" % (d, T), (B, T, d), 17)
    mask = R.prefix_mask(lengths, T)
    xg, mg = x.to(dev), mask.to(dev)
    out = {"enc": enc, "x": xg, "mask": mg, "p": {k: v.double() for k, v in p32.items()}, "xd": x.double(), "md": mask.double()}
    s = _open(enc, B, T, span)
    out["ext"] = _extend_all(s, xg, mg, groups)
    assert s.t == T
    s.reset()
    out["after_reset"] = _extend_all(s, xg, mg, groups)
    out["again"] = _extend_all(_open(enc, B, T, span), xg, mg, groups)
    out["stepped"] = _step_all(_open(enc, B, T, span), xg, mg, 0, T)
    torch.cuda.synchronize()
    with torch.no_grad():
        out["ref"] = (S.encoder_stack(out["p"], "", out["xd"], out["md"], h) if span is None
                      else RS.encoder_stack(out["p"], "", out["xd"], out["md"], h, span)).numpy()
    _CACHE[ident] = out
    return out


def _plain(i, dev):
    c, groups = PLAIN[i]
    return _run(c + (groups, None), dev)


def _ring(c, dev):
    d, h, n, span = c
    return _run((d, h, n, RING_T, RING_LENGTHS, RING_GROUPS, span), dev)


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("i", range(len(PLAIN)), ids=PLAIN_IDS)
def test_extend_against_the_stream_reference(dev, i):
    """all rows of extend against stream_ref.encoder_stack under ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3 (rel-L2 / per-row maximum).
    Measured worst over the cases on the MI355X: 1.6e-4 (d 64, three layers) / 1.5e-3 (d 40); the cases in which fp32 noise tips no bf16
    rounding (d 32, d 512) sit at 1e-7."""
    r = _plain(i, dev)
    check("extend %s y" % PLAIN_IDS[i], r["ext"], r["ref"], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", RING, ids=RING_IDS)
def test_ring_extend_against_the_ring_reference(dev, c):
    """T = 70 in groups [7, 16, 30, 17] against ring_stream_ref.encoder_stack under ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3.
    Measured worst on the MI355X: 1.3e-4 / 1.3e-3 (d 128, span 1); d 40 at spans 1, 5 and 16 sits at 1e-7."""
    r = _ring(c, dev)
    check("ring extend %s y" % RING_IDS[RING.index(c)], r["ext"], r["ref"], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


def test_steps_and_extends_mix(dev):
    """step x3, extend 20, step x2, extend 7, then one more step from the extended state: all 33 rows against the one reference.
    Measured on the MI355X: 9.0e-8 / 1.7e-7."""
    r = _plain(1, dev)
    x, m = r["x"], r["mask"]
    s = r["enc"].stream(3, 45)
    rows = [_step_all(s, x, m, 0, 3), s.extend(x[:, 3:23].contiguous(), m[:, 3:23].contiguous()).cpu(), _step_all(s, x, m, 23, 25),
            s.extend(x[:, 25:32].contiguous(), m[:, 25:32].contiguous()).cpu()]
    assert s.t == 32
    rows.append(_step_all(s, x, m, 32, 33))
    got = torch.cat(rows, dim=1)
    check("extend mixed with steps y", got, r["ref"][:, :33], ENC_OUT, ENC_OUT_ROW)
    check("extend mixed with steps, the stepped row behind", got[:, 32], r["ref"][:, 32], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


def test_prefill_then_extend_then_step(dev):
    """prefill 10, extend 12, step x2: all 24 rows against the one reference, prefill_ref (the history's rows and cache are the batch
    path's, every later row the stream rule's from that cache).  Measured on the MI355X: 7.1e-5 / 6.0e-4."""
    r = _plain(1, dev)
    x, m = r["x"], r["mask"]
    s = r["enc"].stream(3, 45)
    rows = [s.prefill(x[:, :10].contiguous(), m[:, :10].contiguous()).cpu(), s.extend(x[:, 10:22].contiguous(), m[:, 10:22].contiguous()).cpu()]
    assert s.t == 22
    rows.append(_step_all(s, x, m, 22, 24))
    got = torch.cat(rows, dim=1)
    with torch.no_grad():
        want = PF.encoder_rows(r["p"], "", 4, r["xd"][:, :24], r["md"][:, :24], [10, 10, 10], 10).numpy()
    check("prefill, extend, step y", got, want, ENC_OUT, ENC_OUT_ROW)
    check("prefill, extend, step: the stepped rows behind", got[:, 22:], want[:, 22:], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. against the stepped stream
@pytest.mark.parametrize("i", range(len(PLAIN)), ids=PLAIN_IDS)
def test_extend_against_the_stepped_stream(dev, i):
    """extend against step on the GPU: each is within ENC_OUT / ENC_OUT_ROW of the one reference, so twice that (triangle inequality).
    Measured worst on the MI355X: 1.7e-4 / 1.2e-3 (d 64); 1e-7 where no rounding tips."""
    r = _plain(i, dev)
    check("extend %s y vs stepped" % PLAIN_IDS[i], r["ext"], r["stepped"], ENC_OUT + ENC_OUT, ENC_OUT_ROW + ENC_OUT_ROW)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", RING, ids=RING_IDS)
def test_ring_extend_against_the_stepped_ring_stream(dev, c):
    """as above for the ring.  Measured worst on the MI355X: 1.6e-4 / 8.8e-4 (d 128)"""
    r = _ring(c, dev)
    check("ring extend %s y vs stepped" % RING_IDS[RING.index(c)], r["ext"], r["stepped"], ENC_OUT + ENC_OUT, ENC_OUT_ROW + ENC_OUT_ROW)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. exact facts, bit for bit
@pytest.mark.parametrize("i", range(len(PLAIN)), ids=PLAIN_IDS)
def test_two_runs_give_the_same_bits(dev, i):
    r = _plain(i, dev)
    assert torch.isfinite(r["ext"]).all()
    assert torch.equal(r["ext"], r["again"]) and torch.equal(r["ext"], r["after_reset"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", RING, ids=RING_IDS)
def test_two_ring_runs_give_the_same_bits(dev, c):
    r = _ring(c, dev)
    assert torch.isfinite(r["ext"]).all()
    assert torch.equal(r["ext"], r["again"]) and torch.equal(r["ext"], r["after_reset"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("i", [i for i, (c, _) in enumerate(PLAIN) if len(c[4]) > 1], ids=[n for n, (c, _) in zip(PLAIN_IDS, PLAIN) if len(c[4]) > 1])
def test_a_sequence_does_not_depend_on_its_batch(dev, i):
    """sequence 0 extended alone (B = 1) has the bits of sequence 0 of the whole batch: one workgroup per sequence, nothing shared"""
    r = _plain(i, dev)
    c, groups = PLAIN[i]
    alone = _extend_all(r["enc"].stream(1, c[3]), r["x"][:1], r["mask"][:1], groups)
    assert torch.equal(alone[0], r["ext"][0])
    torch.cuda.synchronize()


def test_a_ring_sequence_does_not_depend_on_its_batch(dev):
    r = _ring(RING[1], dev)
    alone = _extend_all(r["enc"].ring_stream(1), r["x"][:1], r["mask"][:1], RING_GROUPS)
    assert torch.equal(alone[0], r["ext"][0])
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("i", range(len(PLAIN)), ids=PLAIN_IDS)
def test_the_state_may_hold_any_contents(dev, i, fill):
    """the whole state filled with each pattern before the run, the weights prepared afterwards: the same bits.  Rows behind t, and
    the pad columns of every row, never reach a result"""
    r = _plain(i, dev)
    c, groups = PLAIN[i]
    s = r["enc"].stream(len(c[4]), c[3])
    fill_bytes(s.state.view(-1), fill)
    s.refresh()
    assert torch.equal(_extend_all(s, r["x"], r["mask"], groups), r["ext"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", [RING[1], RING[7]], ids=[RING_IDS[1], RING_IDS[7]])
def test_the_ring_state_may_hold_any_contents(dev, c, fill):
    r = _ring(c, dev)
    s = r["enc"].ring_stream(len(RING_LENGTHS))
    fill_bytes(s.state.view(-1), fill)
    s.refresh()
    assert torch.equal(_extend_all(s, r["x"], r["mask"], RING_GROUPS), r["ext"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", RING, ids=RING_IDS)
def test_ring_rows_below_the_span_are_the_plain_rows(dev, c):
    """ring extend rows at positions < span have the bits of the plain extend of the same stack without the span, same grouping"""
    r = _ring(c, dev)
    d, h, n, span = c
    plain, _ = _encoder(d, h, n, None, dev)
    want = _extend_all(plain.stream(len(RING_LENGTHS), RING_T), r["x"], r["mask"], RING_GROUPS)
    assert torch.equal(r["ext"][:, :span], want[:, :span])
    assert span >= RING_T or not torch.equal(r["ext"], want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("ring", [False, True], ids=["plain", "ring"])
def test_slots_extend_gives_the_host_forms_bits(dev, ring):
    """every slot seated at 0 and extended with the host form's grouping: the same kernel body, the same bits; and rows of x behind
    a slot's len change nothing: the ragged recording extended by its lengths, with NaN behind them, has the bits of its prefix"""
    r = _ring(RING[5], dev) if ring else _plain(1, dev)
    enc, x, m = r["enc"], r["x"], r["mask"]
    B, T = x.shape[0], x.shape[1]
    groups = RING_GROUPS if ring else PLAIN[1][1]
    lengths = RING_LENGTHS if ring else PLAIN[1][0][4]
    s = enc.ring_slot_stream(B) if ring else enc.slot_stream(B, T)
    s.reset()
    rows, t = [], 0
    for g in groups:
        rows.append(s.extend(list(range(B)), x[:, t:t + g].contiguous(), [g] * B, m[:, t:t + g].contiguous()))
        t += g
    assert torch.equal(torch.cat(rows, dim=1).cpu(), r["ext"])
    assert s.positions.tolist() == [T] * B
    # ragged: slot b gets only its own windows, group by group; what lies behind them in x is NaN
    s.reset()
    poisoned = x.clone()
    for b, n in enumerate(lengths):
        poisoned[b, n:] = float("nan")
    rows, t = [], 0
    for g in groups:
        idx = [b for b, n in enumerate(lengths) if n > t]
        lens = [min(g, lengths[b] - t) for b in idx]
        y = s.extend(idx, poisoned[idx, t:t + g].contiguous(), lens)
        full = torch.zeros(B, g, x.shape[2], device=x.device)
        full[idx] = y
        rows.append(full)
        t += g
    got = torch.cat(rows, dim=1).cpu()
    assert torch.isfinite(got).all()
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :n], r["ext"][b, :n]) and (got[b, n:] == 0).all()
    assert s.positions.tolist() == lengths
    torch.cuda.synchronize()


def test_slots_are_all_or_nothing(dev):
    """B = 4: seated at 17, idle, seated at 0, full.  extend([2, 0, 1, 3], x, [3, 17, 5, 2]): the idle and the full slot get zero rows
    and keep their positions and every byte of their cache (against a clone of the state); the other two run their lengths and
    advance by them; and a call that names only those two leaves the same bytes behind"""
    r = _plain(1, dev)
    enc, x = r["enc"], r["x"]
    d, h, N, cap = 40, 4, 2, 40
    s = enc.slot_stream(4, cap)
    s.seat([0, 3])
    s.extend([0, 3], x[[0, 1], :17].contiguous(), [17, 17])
    s.extend([3], x[1:2, 17:40].contiguous(), [23])
    s.seat([2])
    assert s.positions.tolist() == [17, -1, 0, cap]
    before, pos_before = s.state.clone(), s.positions.clone()
    xs = torch.stack([x[0, :17], x[0, 17:34], x[1, :17], x[1, :17]]).contiguous()
    y = s.extend([2, 0, 1, 3], xs, [3, 17, 5, 2]).cpu()
    assert s.positions.tolist() == [34, -1, 3, cap]
    assert torch.isfinite(y).all() and (y[2] == 0).all() and (y[3] == 0).all() and (y[0, 3:] == 0).all()
    check("slots extend, slot 0 from 17", y[1], r["ref"][0, 17:34], ENC_OUT, ENC_OUT_ROW)
    check("slots extend, slot 2 from 0", y[0, :3], r["ref"][0, :3], ENC_OUT, ENC_OUT_ROW)
    # the layout of csrc/encoder_step_plan.h: the cache is the tail of the queried size, [layer][K | V][b][head][row][d_k padded to 8]
    nb = mta().functional.encoder_stream_bytes(4, cap, d, h, R.D_FF, N)
    seq = h * cap * 16 * 2                                           # bytes of one sequence's K (or V) of one layer; d_k = 10 padded to 16
    cache0 = nb - (N * 2 * 4 * seq + 255) // 256 * 256
    after = s.state
    for layer in range(N):
        for kv in range(2):
            for b in (1, 3):
                o = cache0 + ((layer * 2 + kv) * 4 + b) * seq
                assert torch.equal(after[o:o + seq], before[o:o + seq]), (layer, kv, b)
            o = cache0 + ((layer * 2 + kv) * 4 + 2) * seq
            assert not torch.equal(after[o:o + seq], before[o:o + seq])      # ... and slot 2's did change
    assert torch.equal(after[:cache0], before[:cache0])              # the prepared weights
    # the same call without the two skipped pairs, on the state as it was
    after, pos_after = s.state.clone(), s.positions.clone()
    s.state.copy_(before)
    s.positions.copy_(pos_before)
    y2 = s.extend([2, 0], xs[:2].contiguous(), [3, 17]).cpu()
    assert torch.equal(y2, y[:2]) and torch.equal(s.state, after) and torch.equal(s.positions, pos_after)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("C", [1, 16, 17, 40])
def test_an_extend_is_one_launch_per_sixteen_windows(dev, C):
    r = _plain(2, dev)
    s = r["enc"].stream(3, 70)
    x, m = r["x"][:, :C].contiguous(), r["mask"][:, :C].contiguous()
    torch.cuda.synchronize()

    def run():
        s.reset()
        return s.extend(x, m)

    _, names = device_kernel_names(run, warm=True)
    torch.cuda.synchronize()
    if names is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert len(names) == (C + 15) // 16 and all("encoder_extend_kernel" in n for n in names), names


def _small_model(kind, dev):
    MT = mta().multiTransformer
    if kind == "sft":
        model = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    elif kind == "uni":
        model = MT.UniTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    else:
        model = MT.UniFullTransformer(48, embed_dim=128, h=8, N=2, device=dev)
    load_named(model)
    MT.causal_attention(model)
    return model.eval()


def test_a_model_extend_launches_no_library_kernel(dev):
    model = _small_model("sft", dev)
    x = R.gen_normal("gpu_extend_nolib:x", (3, 24, 48), 5).to(dev)
    mask = R.prefix_mask([24, 9, 1], 24).to(dev)
    chunks = [(x[:, a:b].contiguous(), mask[:, a:b].contiguous()) for a, b in ((0, 4), (4, 21))]
    s = model.stream(3, 24)
    s.extend(*chunks[0]), s.extend(*chunks[1])               # warm-up: the pool's workspaces of these shapes exist
    s.reset()
    torch.cuda.synchronize()
    _, first = device_kernel_names(lambda: s.extend(*chunks[0]))     # from t = 0: the h0 W_hh row rides in
    _, later = device_kernel_names(lambda: s.extend(*chunks[1]))
    torch.cuda.synchronize()
    if first is None or later is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(first) == [] and library_kernels(later) == [], (first, later)
    assert sum("encoder_extend_kernel" in n for n in first) == 1 and sum("encoder_extend_kernel" in n for n in later) == 2, (first, later)


# ------------------------------------------------------------------------------------------------ 5. models
MODEL_GROUPS = [4, 17, 3]


@pytest.mark.parametrize("kind", ["sft", "b2", "uni"])
def test_sequence_model_extend_against_its_stepped_stream(dev, kind):
    """extend in groups [4, 17, 3] and one step behind them against the model's stepped stream(): rel-L2 <= OUT_RTOL, the bound
    tests/test_gpu_stream.py holds the stepped stream to against the batch forward; padded windows are exact zeros"""
    model = _small_model(kind, dev)
    T, lengths = 25, [25, 7, 1]
    x = R.gen_normal("gpu_extend_model_%s:x" % kind, (3, T, 48), 5).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    stepped = model.stream(3, T)
    want = torch.stack([stepped.step(x[:, t], mask[:, t]) for t in range(T)], dim=1).cpu()
    s = model.stream(3, T)
    for rec in range(2):                                     # the second recording after reset(): the carried LSTM state starts anew
        rows, t = [], 0
        for g in MODEL_GROUPS:
            rows.append(s.extend(x[:, t:t + g].contiguous(), mask[:, t:t + g].contiguous()))
            t += g
            assert s.t == t
        rows.append(s.step(x[:, t], mask[:, t]).view(3, 1, 1))
        got = torch.cat(rows, dim=1).cpu()
        assert got.shape == want.shape == (3, T, 1) and s.t == T
        err, err_last = rel_l2(got.numpy(), want.numpy()), rel_l2(got[:, -1].numpy(), want[:, -1].numpy())
        print("extend model %s recording %d: rel_l2 %.3e, the stepped window behind %.3e" % (kind, rec, err, err_last))
        assert torch.isfinite(got).all() and err <= OUT_RTOL and err_last <= OUT_RTOL
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()
        s.reset()
    torch.cuda.synchronize()


def test_wrapper_extend_against_its_stepped_stream(dev):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    T, lengths, W = 25, [25, 9], 3
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    model = MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=dev)
    model.Transformer = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    load_named(model)
    MT.causal_attention(model)
    model.eval()
    x = {mod: R.gen_normal("gpu_extend_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    stepped = model.stream(2, T)
    want = torch.stack([stepped.step({mod: x[mod][:, t] for mod in mods}, mask[:, t]) for t in range(T)], dim=1).cpu()
    s = model.stream(2, T)
    rows, t = [], 0
    for g in MODEL_GROUPS:
        rows.append(s.extend({mod: x[mod][:, t:t + g].contiguous() for mod in mods}, mask[:, t:t + g].contiguous()))
        t += g
    rows.append(s.step({mod: x[mod][:, t] for mod in mods}, mask[:, t]).view(2, 1, 1))
    got = torch.cat(rows, dim=1).cpu()
    err = rel_l2(got.numpy(), want.numpy())
    print("extend wrapper: rel_l2 %.3e" % err)
    assert got.shape == want.shape and s.t == T and torch.isfinite(got).all() and err <= OUT_RTOL
    ring_model = MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=dev)
    ring_model.Transformer = MT.NLPTransformer(48, embed_dim=40, h=4, N=2, device=dev)
    load_named(ring_model)
    MT.causal_attention(ring_model, True, span=T)             # a span that is never reached: the plain model's function
    ring_model.eval()
    rs = m.streaming.ring_stream(ring_model, 2)
    got_ring = torch.cat([rs.extend({mod: x[mod][:, a:b].contiguous() for mod in mods}, mask[:, a:b].contiguous())
                          for a, b in ((0, 4), (4, 21), (21, 24))], dim=1).cpu()
    assert rs.t == 24 and rs.capacity is None and torch.equal(got_ring, got[:, :24])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. refusals before any launch
def _refused(call, exc, match):
    """call() raises exc naming the remedy -> the device kernels it launched before that (None or empty: none)"""
    def run():
        with pytest.raises(exc, match=match):
            call()
    return device_kernel_names(run)[1]


def test_refusals_come_before_any_launch(dev):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    r = _plain(1, dev)
    enc, x, mk = r["enc"], r["x"], r["mask"]
    host, slots = enc.stream(3, 20), enc.slot_stream(3, 20)
    host.extend(x[:, :5].contiguous(), mk[:, :5].contiguous())
    slots.seat([1])
    trained, _ = seeded_encoder(40, 4, 2, dev, 17)
    MT.causal_attention(trained)
    in_train = trained.stream(3, 20)
    trained.train()
    sft = _small_model("sft", dev)
    seq, dseq = sft.stream(3, 20), sft.device_stream(3, 20)
    xm = torch.zeros(3, 6, 48, device=dev)
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    mfn = MT.MultiTransformer(mods, wes, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32}).eval()
    MT.causal_attention(mfn)
    gate, gate_slots, gate_alone = mfn.stream(2, 4), mfn.slot_stream(2, 4), mfn.mfn.stream(2)
    base = MM.MultiLSTM(24, embed_dim=16, h_dim=12, attn_len=4, device=dev).eval()
    ed = MM.MultiEDLSTM(24, embed_dim=16, h_dim=12, device=dev).eval()
    MM.attend_over_taps(base)
    MM.attend_over_taps(ed)
    lstms = [base.stream(2), base.slot_stream(2), ed.feedback_stream(2), ed.feedback_slot_stream(2)]
    x6, x16 = x[:, :6].contiguous(), x[:, :16].contiguous()
    narrow, x64, xcpu, none = x6[:, :, :32].contiguous(), x6.double(), x6.cpu(), x6[:, :0]
    xl = torch.zeros(2, 3, 24, device=dev)
    xm40, xm21 = xm[:, :, :40].contiguous(), torch.zeros(3, 21, 48, device=dev)      # made here: a copy or a fill is a launch too
    torch.cuda.synchronize()
    calls = [(lambda: host.extend(x16), ValueError, "ring"),                         # 5 + 16 > 20, and the remedy is named
             (lambda: in_train.extend(x6), ValueError, r"\.eval\(\)"),
             (lambda: host.extend(narrow), ValueError, "shape"),
             (lambda: host.extend(x64), ValueError, "float32"),
             (lambda: host.extend(xcpu), ValueError, "float32 tensor on"),
             (lambda: host.extend(none), ValueError, "P >= 1"),
             (lambda: host.extend(x6, mk[:, :5]), ValueError, "mask"),
             (lambda: slots.extend([0, 0], x6[:2], [1, 1]), ValueError, "distinct"),
             (lambda: slots.extend([3], x6[:1], [1]), ValueError, "distinct"),
             (lambda: slots.extend([0], x6[:1], [7]), ValueError, "lengths"),
             (lambda: slots.extend([0], x6[:1], [0]), ValueError, "lengths"),
             (lambda: slots.extend([0, 1], x6[:2], [1]), ValueError, "one length"),
             (lambda: slots.extend([0], x6[:2], [1]), ValueError, "shape"),
             (lambda: seq.extend(xm40), ValueError, "shape"),
             (lambda: seq.extend(xm21), ValueError, "capacity"),
             (lambda: dseq.extend(xm), NotImplementedError, "step"),
             (lambda: gate.extend({}), NotImplementedError, "step"),
             (lambda: gate_slots.extend({}), NotImplementedError, "step"),
             (lambda: gate_alone.extend({}), NotImplementedError, "step")]
    calls += [(lambda s=s: s.extend(xl), NotImplementedError, "step") for s in lstms]
    for call, exc, match in calls:
        names = _refused(call, exc, match)
        assert not names, (match, names)
    assert (host.t, in_train.t, seq.t, lstms[0].t, lstms[2].t) == (5, 0, 0, 0, 0)
    assert slots.positions.tolist() == [-1, 0, -1] and dseq.positions.tolist() == [-1, -1, -1]
    torch.cuda.synchronize()
