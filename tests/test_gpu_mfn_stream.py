"""GPU: the MFN gate one window at a time (csrc/mfn_step.h mfn_step_kernel, mmt_mfn_stream_*, functional.mfn_stream_step, MFN.stream /
MFNStream, and the stream methods of MultiTransformer, MultiTransformerB3, MultiCNNTransformerB3 and
MultiCNNTransformerMFT.stream_modalities).

The reference is tests/mfn_stream_ref.py (tests/test_mfn_stream_cpu.py holds it to oracle.mfn_gate in fp64 and, rounded, to the batch
composition of bf16_ref's pieces: one function serves the step and the batch path).  What is left between the kernel and it is fp32
summation order, the hardware exp2 / reciprocal, and the few bf16 roundings that this noise tips.  The bounds are the measured worst
values on the MI355X times at most 4 (the project's practice: LSTM_OUT 7e-4 over a measured 1.7e-4), and every case is also held under
D, the distance that the rounding itself moves the reference of that case (computed here, 4e-3 .. 7e-3).
"""
import pytest
import torch

import mfn_stream_ref as S
import recipe as R
from conftest import rel_l2
from gpu_harness import (FILLS, OUT_RTOL, check, dev, device_kernel_names, fill_bytes, library_kernels, load_named, measures, mta,  # noqa: F401
                         same_bits)

pytestmark = pytest.mark.gpu

# (modalities, input widths, lengths (B of them), steps): the smallest shapes that reach every path
CASES = [(["emotient"], [8], [1], 1),                                                          # one modality, one window, B = 1
         (["acoustic", "emotient"], [12, 16], [3, 2, 1], 3),                                   # width 12: k padded to 8
         (["linguistic", "acoustic", "image"], [40, 24, 32], [12, 5, 1], 12),                  # sum H = 224
         (["linguistic", "emotient", "acoustic", "image"], [256, 16, 256, 256], [5, 3], 5),    # sum H = 240, the reference widths
         (["acoustic", "emotient"], [16, 16], [4, 3, 2, 1] * 8 + [4], 4)]                      # 33 workgroups
IDS = ["%s_B%d_T%d" % ("+".join(m[:3] for m in c[0]), len(c[2]), c[3]) for c in CASES]

# rel-L2 / per-row maximum against mfn_stream_ref (rounding on).  Measured worst over CASES on the MI355X: 4.08e-4 / 1.61e-3
# (lin+aco+ima, 12 steps: fp32 noise tips a bf16 rounding and the recurrences carry it; the cases without a tipped rounding sit at
# 5e-8): x 2.9 / x 3.1.
MFN_STEP_OUT, MFN_STEP_ROW = 1.2e-3, 5e-3
# the stepped gate against the GPU batch path (MFN.forward; MultiTransformerB3.stream against its forward): the same rounding sites, so
# fp32 order and a tipped rounding on either side.  Measured worst: 2.33e-5 / 2.67e-4 (aco+emo, B = 33; every other case at most
# 1.3e-7 / 1.4e-7, B3 exactly 0): x 3.9 / x 3.7.
MFN_STEP_VS_BATCH, MFN_STEP_VS_BATCH_ROW = 9e-5, 1e-3
_CACHE = {}


def _gate(c, dev, seed=11):
    MT = mta().multiTransformer
    gate = MT.MFN(c[0], dict(zip(c[0], c[1])), 1, device=dev)
    p32 = load_named(gate, seed)
    return gate.eval(), p32


def _inputs(c, dev, seed=11):
    mods, widths, lengths, T = c
    x = {m: R.gen_normal("gpu_mfn_stream:%s:%d" % (m, T), (T, len(lengths), w), seed) for m, w in zip(mods, widths)}
    mask = R.prefix_mask(lengths, T)
    return x, mask, {m: v.to(dev) for m, v in x.items()}, mask.to(dev)


def _record(stream, xg, mg):
    """every window through stream.step, in order -> (B, T, output_dim) on the CPU"""
    mods = list(xg)
    T = xg[mods[0]].shape[0]
    rows = [stream.step({m: xg[m][t] for m in mods}, mg[:, t].contiguous()) for t in range(T)]
    return torch.stack(rows, dim=1).cpu()


def _run(c, dev):
    """every GPU result and the CPU references of one case, computed once"""
    key = IDS[CASES.index(c)]
    if key in _CACHE:
        return _CACHE[key]
    gate, p32 = _gate(c, dev)
    x, mask, xg, mg = _inputs(c, dev)
    out = {"gate": gate, "x": xg, "mask": mg}
    with torch.no_grad():
        out["batch"] = gate._gate(xg, mg).cpu()
    s = gate.stream(len(c[2]))
    assert s.t == 0
    out["stream"] = _record(s, xg, mg)
    assert s.t == c[3]
    s.reset()
    assert s.t == 0
    out["after_reset"] = _record(s, xg, mg)
    out["again"] = _record(gate.stream(len(c[2])), xg, mg)
    torch.cuda.synchronize()
    pd = {k: v.double() for k, v in p32.items()}
    xd = {m: v.double() for m, v in x.items()}
    out["ref"] = S.mfn_gate(pd, "", xd, c[0], mask.double()).numpy()
    out["exact"] = S.mfn_gate(pd, "", xd, c[0], mask.double(), rounding=False).numpy()
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_step_against_the_stream_reference(dev, c):
    """all rows against mfn_stream_ref (rounding on) under MFN_STEP_OUT / MFN_STEP_ROW, and under D, what the rounding itself moves this
    case's reference by.  Measured (rel-L2 / per row, then D / D per row): emo 0 / 0, 1.4e-2 / 1.4e-2; aco+emo 4.8e-8 / 1.4e-7,
    3.8e-3 / 7.5e-3; lin+aco+ima 4.08e-4 / 1.61e-3, 6.1e-3 / 1.7e-2; all four 5.1e-8 / 1.5e-7, 4.5e-3 / 9.0e-3; aco+emo B 33
    2.5e-5 / 2.7e-4, 5.1e-3 / 1.9e-2."""
    r = _run(c, dev)
    tag = IDS[CASES.index(c)]
    D, D_row = measures(r["ref"], r["exact"])
    print("mfn step %s: rounding on vs off rel-L2 %.3e per-row %.3e" % (tag, D, D_row))
    assert D > 1e-4                                                # the reference rounds
    check("mfn step %s y" % tag, r["stream"], r["ref"], min(MFN_STEP_OUT, D), min(MFN_STEP_ROW, D_row))
    mask = r["mask"].cpu()
    assert (r["stream"][mask.expand_as(r["stream"]) == 0] == 0).all()          # a blanked window is an exact zero
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. against the batch path
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_step_against_the_batch_forward(dev, c):
    """MFNStream against MFN.forward (eval) of the same inputs on the GPU: the same rounding sites in both.
    Measured: emo 1.3e-7 / 1.3e-7; aco+emo 7.2e-8 / 1.4e-7; lin+aco+ima 3.7e-8 / 1.2e-7 (the batch path tips the same rounding as the
    step: both sit 4.08e-4 from the reference); all four 3.1e-8 / 9.8e-8; aco+emo B 33 2.33e-5 / 2.67e-4."""
    r = _run(c, dev)
    tag = IDS[CASES.index(c)]
    D, D_row = measures(r["ref"], r["exact"])
    check("mfn step %s y vs MFN.forward" % tag, r["stream"], r["batch"], min(MFN_STEP_VS_BATCH, D), min(MFN_STEP_VS_BATCH_ROW, D_row))
    torch.cuda.synchronize()


def _b3(dev):
    MT = mta().multiTransformer
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    model = MT.MultiTransformerB3(mods, wes, device=dev)
    load_named(model)
    return model.eval(), mods, wes


def test_b3_stream_against_its_batch_forward(dev):
    """MultiTransformerB3.stream (embeds + the MFN step; no cache, no causal_attention) against its eval forward, T = 5.
    Measured: exactly 0 in both recordings."""
    model, mods, wes = _b3(dev)
    T, lengths = 5, [5, 3, 1]
    x = {m: R.gen_normal("gpu_mfn_stream_b3:" + m, (3, T, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, mask, lengths).cpu()
    s = model.stream(3)
    assert s.capacity is None
    for rec in range(2):
        got = torch.stack([s.step({m: x[m][:, t].contiguous() for m in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
        assert got.shape == want.shape == (3, T, 1)
        check("B3 stream recording %d vs forward" % rec, got, want, MFN_STEP_VS_BATCH, MFN_STEP_VS_BATCH_ROW)
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()
        assert s.t == T
        s.reset()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the models' own eval forward
def _small_mft(dev):
    MT = mta().multiTransformer
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    model = MT.MultiTransformer(mods, wes, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32})
    load_named(model)
    MT.causal_attention(model)
    return model.eval(), mods, wes


def test_mft_stream_against_its_batch_forward(dev):
    """MultiTransformer.stream (N = 2, embed_dim 40 / 32, h = 4) against its own causal eval forward: rel-L2 <= OUT_RTOL, padded windows
    exact zeros; a second recording after reset() starts anew.  Measured 1.59e-3 in both recordings (the encoders' step and batch kernels round the softmax at different reference
    points)."""
    model, mods, wes = _small_mft(dev)
    T, lengths = 12, [12, 5, 1]
    x = {m: R.gen_normal("gpu_mfn_stream_mft:" + m, (3, T, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, mask, lengths).cpu()
    s = model.stream(3, T)
    assert (s.t, s.capacity) == (0, T)
    for rec in range(2):
        got = torch.stack([s.step({m: x[m][:, t].contiguous() for m in mods}, mask[:, t].contiguous()) for t in range(T)], dim=1).cpu()
        err = rel_l2(got.numpy(), want.numpy())
        print("MFT stream recording %d: rel_l2 %.3e" % (rec, err))
        assert got.shape == want.shape == (3, T, 1) and torch.isfinite(got).all() and err <= OUT_RTOL
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()
        assert s.t == T
        s.reset()
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["mft_stream_modalities", "b3_stream"])
def test_wrapper_stream_against_its_batch_forward(dev, which):
    """the window encoder in front (T = 5): MultiCNNTransformerMFT.stream_modalities and MultiCNNTransformerB3.stream against the
    wrapper's own eval forward, rel-L2 <= OUT_RTOL, padded windows exact zeros.  Measured 1.66e-3 (MFT), exactly 0 (B3)."""
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
    x = {mod: R.gen_normal("gpu_mfn_stream_wrap:" + mod, (2, T, W, dims[mod]), 5).to(dev) for mod in mods}
    mask = R.prefix_mask(lengths, T).to(dev)
    with torch.no_grad():
        want = model(x, lengths, mask).cpu()
    s = model.stream_modalities(2, T) if which == "mft_stream_modalities" else model.stream(2)
    got = torch.stack([s.step({mod: x[mod][:, t] for mod in mods}, mask[:, t]) for t in range(T)], dim=1).cpu()
    err = rel_l2(got.numpy(), want.numpy())
    print("stream wrapper %s: rel_l2 %.3e" % (which, err))
    assert got.shape == want.shape == (2, T, 1) and torch.isfinite(got).all() and err <= OUT_RTOL
    for b, n in enumerate(lengths):
        assert (got[b, n:] == 0).all()
    assert s.t == T
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. exact facts, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_two_recordings_and_a_reset_give_the_same_bits(dev, c):
    r = _run(c, dev)
    failures = []
    same_bits("a second, fresh stream", {"y": r["stream"]}, {"y": r["again"]}, failures)
    same_bits("the same stream after reset()", {"y": r["stream"]}, {"y": r["after_reset"]}, failures)      # nothing was cleared or re-read
    assert not failures, failures
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [c for c in CASES if len(c[2]) > 1], ids=[i for i, c in zip(IDS, CASES) if len(c[2]) > 1])
def test_a_sequence_does_not_depend_on_its_batch(dev, c):
    """sequence 0 stepped alone (B = 1) has the bits of sequence 0 of the whole batch: one workgroup per sequence, nothing shared"""
    r = _run(c, dev)
    alone = _record(r["gate"].stream(1), {m: v[:, :1].contiguous() for m, v in r["x"].items()}, r["mask"][:1])
    failures = []
    same_bits("sequence 0 alone", {"y": alone[0]}, {"y": r["stream"][0]}, failures)
    assert not failures, failures
    torch.cuda.synchronize()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_state_may_hold_any_contents(dev, c, fill):
    """the whole state (both copies of (h, c, mem) with it) filled with each pattern before step 0, the parameters prepared afterwards:
    the same bits as a run on a state as the allocator left it.  Step 0 reads no carried state, and a later step only what the step
    before it wrote."""
    r = _run(c, dev)
    s = r["gate"].stream(len(c[2]))
    before = s.state.clone()
    fill_bytes(s.state.view(-1), fill)
    assert not torch.equal(before, s.state)
    s.refresh()
    failures = []
    same_bits("state filled with %s" % fill, {"y": _record(s, r["x"], r["mask"])}, {"y": r["stream"]}, failures)
    assert not failures, failures
    torch.cuda.synchronize()


def test_refresh_follows_the_parameters(dev):
    """the prepared weights AND biases are copies: a changed matrix or a changed bias shows after refresh() only"""
    c = CASES[1]
    gate, _ = _gate(c, dev, seed=23)
    _, _, xg, mg = _inputs(c, dev, seed=23)
    s = gate.stream(len(c[2]))
    a = _record(s, xg, mg)
    for change in (lambda: gate.att2_fc1.weight.mul_(0.5), lambda: gate.lstm["emotient"].bias_hh.add_(0.25), lambda: gate.out_fc2.bias.add_(1.0)):
        with torch.no_grad():
            change()
        s.reset()
        stale = _record(s, xg, mg)
        s.reset()
        s.refresh()
        fresh = _record(s, xg, mg)
        with torch.no_grad():
            want = gate._gate(xg, mg).cpu()
        assert torch.equal(a, stale) and not torch.equal(a, fresh)
        check("refreshed stream vs MFN.forward", fresh, want, MFN_STEP_VS_BATCH, MFN_STEP_VS_BATCH_ROW)      # measured 2.9e-8, 0, 0
        a = fresh
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. launches
def test_one_step_is_one_launch(dev):
    r = _run(CASES[2], dev)
    s = r["gate"].stream(3)
    mods = list(r["x"])
    xs = [{m: r["x"][m][t].contiguous() for m in mods} for t in range(3)]        # the caller's slicing is not the step's
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
    assert len(names) == 1 and "mfn_step_kernel" in names[0], names


def test_an_mft_step_launches_no_library_kernel(dev):
    """a warmed MultiTransformer.stream step: per modality the embed affine map (one row GEMM with its operand preparation) and ONE
    encoder_step_kernel, then ONE mfn_step_kernel, which is the last launch; no library kernel, at step 0 and later"""
    model, mods, wes = _small_mft(dev)
    x = {m: R.gen_normal("gpu_mfn_stream_nolib:" + m, (3, 6, wes[m]), 5).to(dev) for m in mods}
    mask = R.prefix_mask([6, 3, 1], 6).to(dev)
    xs = [{m: x[m][:, t].contiguous() for m in mods} for t in range(6)]
    ms = [mask[:, t].contiguous() for t in range(6)]
    s = model.stream(3, 6)
    t = [-1]

    def step():
        t[0] += 1
        return s.step(xs[t[0]], ms[t[0]])

    step(), step()                                           # warm-up: the pool's workspaces of these shapes exist (a new one is zero-filled)
    s.reset()
    t[0] = -1
    torch.cuda.synchronize()
    _, first = device_kernel_names(step)
    _, later = device_kernel_names(step)
    torch.cuda.synchronize()
    if first is None or later is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    for names in (first, later):
        print(names)
        assert library_kernels(names) == [], names
        assert sum("encoder_step_kernel" in n for n in names) == len(mods), names
        assert sum("rowgemm" in n for n in names) == len(mods), names
        assert sum("mfn_step_kernel" in n for n in names) == 1 and "mfn_step_kernel" in names[-1], names
        assert all(any(k in n for k in ("encoder_step_kernel", "rowgemm", "mfn_step_kernel", "pad_cast_kernel", "pad_f32_kernel"))
                   for n in names), names


# ------------------------------------------------------------------------------------------------ 6. refusals before any launch
def _refused(call, exc, match):
    """call() raises exc naming the remedy -> the device kernels it launched before that (None or empty: none)"""
    def run():
        with pytest.raises(exc, match=match):
            call()
    return device_kernel_names(run)[1]


def test_refusals_come_before_any_launch(dev):
    m = mta()
    MT = m.multiTransformer
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    gate, _ = _gate(CASES[1], dev)
    opened = gate.stream(2)
    x = {"acoustic": torch.zeros(2, 12, device=dev), "emotient": torch.zeros(2, 16, device=dev)}
    noncausal = MT.MultiTransformer(mods, wes, N=1, h=2, device=dev, embed_dim={"acoustic": 32, "emotient": 16}).eval()
    causal, _, _ = _small_mft(dev)
    full = causal.stream(2, 1)
    full.step(x, torch.ones(2, device=dev))
    b3, _, _ = _b3(dev)
    b3s = b3.stream(2)

    class Wide(MT.MFN):                                      # sum H = 4 x 88 > 256: outside the step kernel's domain
        hidden_dim = {"linguistic": 88, "emotient": 88, "acoustic": 88, "image": 88}

    class Odd(MT.MFN):                                       # H = 18: not a multiple of 4
        hidden_dim = {"acoustic": 18, "emotient": 16}

    wide = Wide(["linguistic", "emotient", "acoustic", "image"], {k: 8 for k in Wide.hidden_dim}, 1, device=dev).eval()
    odd = Odd(mods, wes, 1, device=dev).eval()
    only = {"acoustic": x["acoustic"]}
    narrow = dict(x, emotient=torch.zeros(2, 12, device=dev))
    x64 = dict(x, acoustic=x["acoustic"].double())
    xcpu = dict(x, emotient=x["emotient"].cpu())
    mask3 = torch.ones(3, device=dev)
    torch.cuda.synchronize()
    for call, exc, match in ((lambda: gate.train().stream(2), ValueError, r"\.eval\(\)"),
                             (lambda: causal.train().stream(2, 4), ValueError, r"\.eval\(\)"),
                             (lambda: noncausal.stream(2, 4), ValueError, r"causal_attention\(model\)"),
                             (lambda: full.step(x), ValueError, "full"),
                             (lambda: opened.step(only), ValueError, "every modality"),
                             (lambda: b3s.step(only), ValueError, "every modality"),
                             (lambda: opened.step(narrow), ValueError, "shape"),
                             (lambda: b3s.step(narrow), ValueError, "shape"),
                             (lambda: opened.step(x64), ValueError, "float32"),
                             (lambda: opened.step(xcpu), ValueError, "float32 tensor on"),
                             (lambda: b3s.step(xcpu), ValueError, "float32 tensor on"),
                             (lambda: opened.step(x, mask3), ValueError, "mask_t"),
                             (lambda: wide.stream(2), ValueError, "hidden sizes > 256"),
                             (lambda: odd.stream(2), ValueError, "multiples of 4")):
        names = _refused(call, exc, match)
        assert not names, (match, names)
        gate.eval(), causal.eval()
    assert opened.t == 0 and b3s.t == 0
    torch.cuda.synchronize()
