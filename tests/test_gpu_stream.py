"""GPU: a causal encoder stack one window at a time (csrc/encoder_step.h encoder_step_kernel, mmt_encoder_stream_*,
functional.encoder_stream_step, Encoder.stream / EncoderStream and the stream() of the sequence models and their wrappers).

The reference is tests/stream_ref.py, the step's own rounding (tests/test_stream_cpu.py holds it to the exact function in fp64 and
measures its distance from the batch path's reference); the bounds are those of tests/test_gpu_bf16_faithful.py, imported: per product
the arithmetic is the batch path's.  Against the batch path on the GPU the bound grows by the distance D between the two references,
computed here on the CPU for each case.  Measured worst values on the MI355X stand beside each use.
"""
import pytest
import torch

import causal_ref as C
import recipe as R
import stream_ref as S
from conftest import rel_l2
from gpu_harness import (FILLS, OUT_RTOL, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named, measures, mta,  # noqa: F401
                         seeded_encoder)
from test_gpu_bf16_faithful import ENC_OUT, ENC_OUT_ROW

pytestmark = pytest.mark.gpu

# (d, h, N, capacity = steps, lengths): the smallest shapes that reach each branch
CASES = [(32, 2, 1, 1, [1]),                    # one key, capacity 1, B = 1
         (40, 4, 2, 45, [45, 30, 1]),           # d_k = 10 padded to 16: two 16-byte chunks, pad columns
         (128, 8, 2, 70, [70, 33, 1]),          # the headline width, d_k = 16
         (64, 2, 3, 130, [130, 86, 1]),         # d_k = 32: 16 keys per sweep, more keys than a wave's lanes twice over; three layers
         (256, 4, 1, 33, [33, 2]),              # d_k = 64: eight chunks per key
         (512, 8, 1, 3, [3])]                   # the widest row: two outputs per thread in every product
IDS = ["d%d_h%d_n%d_T%d" % c[:4] for c in CASES]
_CACHE = {}


def _record(stream, x, mask):
    """every window of x through stream.step, in order -> (B, T, d) on the CPU"""
    rows = [stream.step(x[:, t], mask[:, t]) for t in range(x.shape[1])]
    return torch.stack(rows, dim=1).cpu()


def _run(c, dev):
    """every GPU result and both CPU references of one case, computed once"""
    if c[:4] in _CACHE:
        return _CACHE[c[:4]]
    d, h, n, T, lengths = c
    B = len(lengths)
    MT = mta().multiTransformer
    enc, p32 = seeded_encoder(d, h, n, dev, 17)
    MT.causal_attention(enc)
    x = R.gen_normal("gpu_stream_d%d_T%d:x" % (d, T), (B, T, d), 17)
    mask = R.prefix_mask(lengths, T)
    xg, mg = x.to(dev), mask.to(dev)
    out = {"enc": enc, "x": xg, "mask": mg}
    with torch.no_grad():
        out["batch"] = enc(xg, mg).cpu()
    s = enc.stream(B, T)
    assert (s.t, s.capacity) == (0, T)
    out["stream"] = _record(s, xg, mg)
    assert s.t == T
    s.reset()
    assert s.t == 0
    out["after_reset"] = _record(s, xg, mg)
    out["again"] = _record(enc.stream(B, T), xg, mg)
    torch.cuda.synchronize()
    pd = {k: v.double() for k, v in p32.items()}
    with torch.no_grad():
        out["ref"] = S.encoder_stack(pd, "", x.double(), mask.double(), h).numpy()
        out["batch_ref"] = C.encoder_stack(pd, "", x.double(), mask.double(), h).detach().numpy()
    _CACHE[c[:4]] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_stream_against_the_stream_reference(dev, c):
    """all rows of y against stream_ref.encoder_stack under ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3 (rel-L2 / per-row maximum).
    Measured worst over the cases: 5.2e-4 (d 128) / 2.5e-3 (d 64, three layers); the cases in which fp32 noise tips no bf16 rounding
    (d 32, d 40, d 256) sit at 1e-7."""
    r = _run(c, dev)
    check("stream %s y" % IDS[CASES.index(c)], r["stream"], r["ref"], ENC_OUT, ENC_OUT_ROW)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. against the batch path
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_stream_against_the_batch_forward(dev, c):
    """the streamed rows against Encoder.forward (causal, eval) of the same inputs on the GPU.  The two paths round the softmax at
    different reference points, so the bound is ENC_OUT + D and ENC_OUT_ROW + D_row, D the distance between the two REFERENCES of this
    case (triangle inequality), computed here on the CPU; nothing is measured against the code under test alone.
    Measured worst: 9.9e-4 / 3.4e-3 (d 64) with D = 9.9e-4 / 3.4e-3: the distance is the references', not the kernels'.  D is exactly 0
    where the two rules coincide: one key tile, or a tile maximum that never moves, at a d_k whose batch normaliser sums fp32 values."""
    r = _run(c, dev)
    D, D_row = measures(r["ref"], r["batch_ref"])
    print("stream %s: distance of the two references rel-L2 %.3e per-row %.3e" % (IDS[CASES.index(c)], D, D_row))
    check("stream %s y vs batch forward" % IDS[CASES.index(c)], r["stream"], r["batch"], ENC_OUT + D, ENC_OUT_ROW + D_row)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. exact facts, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_two_recordings_and_a_reset_give_the_same_bits(dev, c):
    r = _run(c, dev)
    assert torch.isfinite(r["stream"]).all()
    assert torch.equal(r["stream"], r["again"])                   # a second, fresh stream
    assert torch.equal(r["stream"], r["after_reset"])             # the same stream after reset(): nothing was cleared or re-read
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [c for c in CASES if len(c[4]) > 1], ids=[i for i, c in zip(IDS, CASES) if len(c[4]) > 1])
def test_a_sequence_does_not_depend_on_its_batch(dev, c):
    """sequence 0 stepped alone (B = 1) has the bits of sequence 0 of the whole batch: one workgroup per sequence, nothing shared"""
    r = _run(c, dev)
    alone = _record(r["enc"].stream(1, c[3]), r["x"][:1], r["mask"][:1])
    assert torch.equal(alone[0], r["stream"][0])
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_state_may_hold_any_contents(dev, c, fill):
    """the whole state (the cache region with it) filled with each pattern before step 0, the weights prepared afterwards: the same
    bits as a run on a state as the allocator left it.  Rows behind t, and the pad columns of every row, never reach a result."""
    r = _run(c, dev)
    s = r["enc"].stream(len(c[4]), c[3])
    before = s.state.clone()
    fill_bytes(s.state.view(-1), fill)
    assert not torch.equal(before, s.state)
    s.refresh()
    assert torch.equal(_record(s, r["x"], r["mask"]), r["stream"])
    torch.cuda.synchronize()


def test_refresh_follows_the_parameters(dev):
    """the prepared weights are a copy: a changed matrix shows after refresh() only (biases and LayerNorm weights are read live)"""
    MT = mta().multiTransformer
    enc, _ = seeded_encoder(40, 4, 1, dev, 23)
    MT.causal_attention(enc)
    x = R.gen_normal("gpu_stream_refresh:x", (2, 40), 23).to(dev)
    s = enc.stream(2, 4)
    a = s.step(x).cpu()
    with torch.no_grad():
        enc.layers[0].feed_forward.w_2.weight.mul_(0.5)
    s.reset()
    stale = s.step(x).cpu()
    s.reset()
    s.refresh()
    fresh = s.step(x).cpu()
    with torch.no_grad():
        want = enc(x.view(2, 1, 40), torch.ones(2, 1, 1, device=dev)).cpu().view(2, 40)
    assert torch.equal(a, stale) and not torch.equal(a, fresh)
    # one key: P = 1 in both paths, so both references coincide and each path is within ENC_OUT of that one reference
    assert rel_l2(fresh.numpy(), want.numpy()) <= 2 * ENC_OUT
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. launches
def test_one_step_is_one_launch(dev):
    r = _run(CASES[2], dev)
    s = r["enc"].stream(3, 8)
    xs = [r["x"][:, t].contiguous() for t in range(3)]          # the caller's slicing is not the step's
    ms = [r["mask"][:, t].contiguous() for t in range(3)]
    torch.cuda.synchronize()
    t = [-1]

    def step():
        t[0] += 1
        return s.step(xs[t[0]], ms[t[0]])

    _, names = device_kernel_names(step, warm=True)
    torch.cuda.synchronize()
    if names is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert len(names) == 1 and "encoder_step_kernel" in names[0], names


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


def test_a_model_step_launches_no_library_kernel(dev):
    model = _small_model("sft", dev)
    x = R.gen_normal("gpu_stream_nolib:x", (3, 6, 48), 5).to(dev)
    mask = R.prefix_mask([6, 3, 1], 6).to(dev)
    xs, ms = [x[:, t].contiguous() for t in range(6)], [mask[:, t].contiguous() for t in range(6)]     # the caller's slicing is not the step's
    s = model.stream(3, 6)
    t = [-1]

    def step():
        t[0] += 1
        return s.step(xs[t[0]], ms[t[0]])

    step(), step()                                           # warm-up: the pool's workspaces of these shapes exist (a new one is zero-filled)
    s.reset()
    t[0] = -1
    torch.cuda.synchronize()
    _, first = device_kernel_names(step)                     # step 0: the h0 W_hh row rides in
    _, later = device_kernel_names(step)
    torch.cuda.synchronize()
    if first is None or later is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(first) == [] and library_kernels(later) == [], (first, later)
    assert sum("encoder_step_kernel" in n for n in later) == 1, later


# ------------------------------------------------------------------------------------------------ 5. models
@pytest.mark.parametrize("kind", ["sft", "b2", "uni"])
def test_sequence_model_stream_against_its_batch_forward(dev, kind):
    """streamed predictions against the model's own eval forward (causal): rel-L2 <= OUT_RTOL; padded windows are exact zeros"""
    model = _small_model(kind, dev)
    T, lengths = 20, [20, 7, 1]
    x = R.gen_normal("gpu_stream_model_%s:x" % kind, (3, T, 48), 5).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, mask, lengths).cpu()
    s = model.stream(3, T)
    for rec in range(2):                                     # the second recording after reset(): the carried LSTM state starts anew
        got = torch.stack([s.step(x[:, t], mask[:, t]) for t in range(T)], dim=1).cpu()
        assert got.shape == want.shape == (3, T, 1)
        err = rel_l2(got.numpy(), want.numpy())
        print("stream model %s recording %d: rel_l2 %.3e" % (kind, rec, err))
        assert torch.isfinite(got).all() and err <= OUT_RTOL
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()
        assert s.t == T
        s.reset()
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["sft_two_modalities", "b2_one_modality"])
def test_wrapper_stream_against_its_batch_forward(dev, which):
    m = mta()
    MT, MM = m.multiTransformer, m.models
    T, lengths, W = 5, [5, 3], 3
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
    x = {mod: R.gen_normal("gpu_stream_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, lengths, mask).cpu()
    s = model.stream(2, T)
    got = torch.stack([s.step({mod: x[mod][:, t] for mod in mods}, mask[:, t]) for t in range(T)], dim=1).cpu()
    err = rel_l2(got.numpy(), want.numpy())
    print("stream wrapper %s: rel_l2 %.3e" % (which, err))
    assert got.shape == want.shape and torch.isfinite(got).all() and err <= OUT_RTOL
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
    enc, _ = seeded_encoder(32, 2, 1, dev, 3)
    x = torch.zeros(2, 32, device=dev)
    causal, _ = seeded_encoder(32, 2, 1, dev, 3)
    MT.causal_attention(causal)
    full = causal.stream(2, 1)
    full.step(x)
    stacked = MT.NLPTransformer(48, embed_dim=40, h=4, N=1, n_layers=2, device=dev).eval()
    MT.causal_attention(stacked)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    mft = MM.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=dev).eval()
    MT.causal_attention(mft)
    big, _ = seeded_encoder(32, 2, 1, dev, 3)
    MT.causal_attention(big)
    opened = big.stream(2, 4)
    x64, xcpu, narrow, mask3 = x.double(), x.cpu(), x[:, :16].contiguous(), torch.ones(3, device=dev)
    torch.cuda.synchronize()
    for call, exc, match in ((lambda: enc.stream(2, 4), ValueError, r"causal_attention\(model\)"),
                             (lambda: causal.train().stream(2, 4), ValueError, r"\.eval\(\)"),
                             (lambda: full.step(x), ValueError, "full"),
                             (lambda: big.stream(2, 4097), ValueError, "capacity"),
                             (lambda: opened.step(narrow), ValueError, "shape"),
                             (lambda: opened.step(x64), ValueError, "float32"),
                             (lambda: opened.step(xcpu), ValueError, "float32 tensor on"),
                             (lambda: opened.step(x, mask3), ValueError, "mask_t"),
                             (lambda: stacked.stream(2, 4), NotImplementedError, "n_layers"),
                             (lambda: mft.stream(2, 4), NotImplementedError, "MFN")):
        names = _refused(call, exc, match)
        assert not names, (match, names)
    assert opened.t == 0
    torch.cuda.synchronize()
