"""CPU: the reference of the banded one-window step (tests/ring_stream_ref.py) against the band reference's exact function and against
stream_ref, the surface of the ring streams (mmt_encoder_stream_step_ring*, streaming.encoder_ring_step*, Encoder.ring_stream /
ring_slot_stream, streaming.ring_stream) with their refusals, the C boundary's refusals, and the host check of the ring rule
(tools/ring_plan_check.cpp under ASan / UBSan).  No GPU: the library is loaded, nothing is launched."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import band_ref as BD
import bf16_ref as E
import conftest
import oracle
import recipe as R
import ring_stream_ref as RS
import stream_ref as S

MMT_EINVAL, MMT_EUNSUPPORTED, MMT_EWORKSPACE = 1, 2, 3
INT_MAX = 2 ** 31 - 1
# (d, h, N, T, span, lengths)
CASES = [(40, 4, 2, 45, 5, [45, 30, 1]), (128, 8, 2, 70, 33, [70, 47, 1]), (64, 2, 3, 130, 40, [130, 86, 1])]
IDS = ["d%d_h%d_n%d_T%d_span%d" % c[:5] for c in CASES]


def case_inputs(c, seed=17):
    d, h, n, T, span, lengths = c
    p = {k: v.double() for k, v in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), seed).items()}
    x = R.gen_normal("ring_d%d_T%d:x" % (d, T), (len(lengths), T, d), seed).double()
    return p, x, R.prefix_mask(lengths, T).double()


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_reference_is_the_exact_band_function(c):
    """rounding=False: row t of the window-by-window walk over the trimmed lists == row t of band_ref's batch function, blanked rows
    included, to 1e-12 (the figure tests/test_stream_cpu.py holds stream_ref to)"""
    p, x, mask = case_inputs(c)
    with torch.no_grad():
        got = RS.encoder_stack(p, "", x, mask, c[1], c[4], rounding=False)
        want = BD.encoder_stack(p, "", x, mask, c[1], c[4], rounding=False).detach()
    err = (got - want).abs().max().item()
    print("ring ref exact %s: max abs %.3e" % (IDS[CASES.index(c)], err))
    assert torch.isfinite(got).all() and err <= 1e-12
    # and the band is there: without the span the rows behind it differ
    full = S.encoder_stack(p, "", x, mask, c[1], rounding=False)
    assert torch.equal(full[:, :c[4]], got[:, :c[4]]) or (full[:, :c[4]] - got[:, :c[4]]).abs().max() <= 1e-12
    assert (full[0, c[4]:] - got[0, c[4]:]).abs().max() > 1e-6


@pytest.mark.parametrize("rounding", [True, False])
def test_a_span_that_covers_the_recording_is_stream_ref_bit_for_bit(rounding):
    c = CASES[0]
    p, x, mask = case_inputs(c)
    T = 12
    want = S.encoder_stack(p, "", x[:, :T], mask[:, :T], c[1], rounding=rounding)
    for span in (T, T + 1, 4096):
        assert torch.equal(RS.encoder_stack(p, "", x[:, :T], mask[:, :T], c[1], span, rounding=rounding), want), span
    assert not torch.equal(RS.encoder_stack(p, "", x[:, :T], mask[:, :T], c[1], T - 1, rounding=rounding), want)


def test_a_blanked_row_is_uniform_over_its_band():
    """one layer, every window blanked: Q' = 0, so the context of window t is the plain mean of V over its min(t + 1, span) keys"""
    d, h, span, T = 40, 4, 5, 9
    p = {k: v.double() for k, v in R.gen_params(E.encoder_param_shapes(d, R.D_FF, 1), 17).items()}
    x = R.gen_normal("ring_blank:x", (2, T, d), 17).double()
    ident = lambda z: z                                                          # noqa: E731
    got = RS.encoder_stack(p, "", x, torch.zeros(2, T, 1).double(), h, span, rounding=False)
    L = "layers.0."
    n0 = oracle.layer_norm(x, p[L + "sublayer.0.norm.a_2"], p[L + "sublayer.0.norm.b_2"])
    v = E._affine(p, L + "self_attn.linears.2", n0, ident)                       # (B, T, d)
    for t in range(T):
        nkeys = min(t + 1, span)
        ctx = v[:, t + 1 - nkeys:t + 1].mean(dim=1)
        x1 = x[:, t] + E._affine(p, L + "self_attn.linears.3", ctx, ident)
        n1 = oracle.layer_norm(x1, p[L + "sublayer.1.norm.a_2"], p[L + "sublayer.1.norm.b_2"])
        x2 = x1 + E._affine(p, L + "feed_forward.w_2", torch.relu(E._affine(p, L + "feed_forward.w_1", n1, ident)), ident)
        want = oracle.layer_norm(x2, p["norm.a_2"], p["norm.b_2"])
        assert (got[:, t] - want).abs().max() <= 1e-12, (t, nkeys)


def test_reference_refuses_a_bad_span():
    p, x, mask = case_inputs(CASES[0])
    for span in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="span"):
            RS.EncoderStream(p, "", 4, span)


# ------------------------------------------------------------------------------------------------ 2. surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib, streaming as ST
    MT = m.multiTransformer
    assert _params(ST.encoder_ring_step) == ["x_t", "mask_t", "flat_params", "state", "t", "h", "d_ff", "n_layers", "span", "eps"]
    assert _params(ST.encoder_ring_step_slots) == ["x_t", "mask_t", "flat_params", "state", "positions", "h", "d_ff", "n_layers", "span",
                                                   "eps", "advance"]
    assert inspect.signature(ST.encoder_ring_step).parameters["eps"].default == 1e-6
    assert inspect.signature(ST.encoder_ring_step_slots).parameters["advance"].default is True
    assert _params(ST.ring_stream) == ["model", "batch", "slots"] and inspect.signature(ST.ring_stream).parameters["slots"].default is False
    assert MT.ring_stream is ST.ring_stream
    assert _params(MT.Encoder.ring_stream) == ["self", "batch"]
    assert _params(MT.Encoder.ring_slot_stream) == ["self", "batch", "positions"]
    assert issubclass(ST.EncoderRingStream, ST.EncoderStream) and not ST.EncoderRingStream.slots
    assert ST.EncoderRingSlotStream.__mro__[1:3] == (ST._Slots, ST.EncoderRingStream) and ST.EncoderRingSlotStream.slots
    assert _params(ST.EncoderRingStream.step) == ["self", "x_t", "mask_t"]
    assert _params(ST.EncoderRingSlotStream.step) == ["self", "x_t", "mask_t", "advance"]
    # what exists keeps its parameter lists
    assert _params(MT.Encoder.stream) == ["self", "batch", "capacity"]
    assert _params(MT.Encoder.slot_stream) == ["self", "batch", "capacity", "positions"]
    assert _params(m.functional.encoder_stream_step_slots) == ["x_t", "mask_t", "flat_params", "state", "positions", "h", "d_ff", "n_layers",
                                                               "capacity", "eps", "advance"]
    assert not hasattr(m.functional, "encoder_ring_step")                        # the wrappers live in streaming
    lib = _lib.load()
    for ring, twin in (("mmt_encoder_stream_step_ring", "mmt_encoder_stream_step"),
                       ("mmt_encoder_stream_step_ring_slots", "mmt_encoder_stream_step_slots")):
        assert hasattr(lib, ring) and _lib.SIGNATURES[ring] == _lib.SIGNATURES[twin], ring
    assert lib.mmt_abi_version() == 1
    with open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")) as f:
        header = " ".join(f.read().split())
    assert ("int mmt_encoder_stream_step_ring(const float* x_t, const float* mask_t, const float* params, float* y_t, void* state, "
            "size_t state_bytes, int t, int B, int span, int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);") in header
    assert ("int mmt_encoder_stream_step_ring_slots(const float* x_t, const float* mask_t, const float* params, float* y_t, void* state, "
            "size_t state_bytes, int* pos, int advance, int B, int span, int d, int h, int f, int n_layers, float eps, "
            "mmt_stream_t stream);") in header
    with open(os.path.join(conftest.ROOT, "multimodal_transformer_amd", "csrc", "step_ring.h")) as f:
        rule = f.read()
    for word in ("MMT_SLOT_HD static inline int ring_keys(int t, int span)", "MMT_SLOT_HD static inline int ring_first_row(int t, int n, int span)",
                 "MMT_SLOT_HD static inline int ring_row(int r0, int i, int span)"):
        assert word in rule, word


# ------------------------------------------------------------------------------------------------ 3. refusals in Python
def _cpu_encoder(span=4, n=2):
    import multimodal_transformer_amd as m
    MT = m.multiTransformer
    enc = MT.Encoder(MT.EncoderLayer(32, MT.MultiHeadedAttention(2, 32), MT.PositionwiseFeedForward(32, 64, 0.1), 0.1), n).eval()
    MT.causal_attention(enc, True, span=span)
    return MT, enc


def test_encoder_ring_stream_refusals_on_cpu():
    """every refusal of Encoder.ring_stream / ring_slot_stream names its remedy and comes before anything touches a device; the
    checks of stream() come in stream()'s order, with the span check turned round"""
    from multimodal_transformer_amd import streaming as ST
    MT, enc = _cpu_encoder()
    for open_ in (lambda e: e.ring_stream(2), lambda e: e.ring_slot_stream(2), lambda e: ST.ring_stream(e, 2),
                  lambda e: ST.ring_stream(e, 2, slots=True)):
        MT, enc = _cpu_encoder()
        with pytest.raises(ValueError, match=r"HIP device"):
            open_(enc)
        enc.train()
        with pytest.raises(ValueError, match=r"\.eval\(\)"):
            open_(enc)
        enc.eval()
        MT.causal_attention(enc)                                                 # causal, no span
        with pytest.raises(ValueError, match=r"causal_attention\(model, span=W\)"):
            open_(enc)
        MT.causal_attention(enc, False)
        with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
            open_(enc)
        MT.causal_attention(enc, True, span=4)
        enc.layers[1].self_attn.span = 5                                         # the layers disagree on the span: not the fused stack
        with pytest.raises(ValueError, match="standard composition"):
            open_(enc)
        enc.layers[1].self_attn.span = 4
        for l in enc.layers:
            l.self_attn.mask_keys = True
        with pytest.raises(ValueError, match="mask_keys"):
            open_(enc)
        for l in enc.layers:
            l.self_attn.mask_keys = False
        MT.keep_attention(enc)
        with pytest.raises(ValueError, match="standard composition"):
            open_(enc)


def test_the_plain_streams_still_refuse_a_span_and_name_the_ring():
    MT, enc = _cpu_encoder()
    for call in (lambda: enc.stream(2, 8), lambda: enc.slot_stream(2, 8)):
        with pytest.raises(ValueError, match=r"span = 4.*ring cache") as e:
            call()
        assert "ring_stream(" in str(e.value)


def test_model_ring_stream_refusals_on_cpu():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import streaming as ST
    MT, M = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    stacked = MT.NLPTransformer(24, embed_dim=32, h=2, N=1, n_layers=2, device=cpu).eval()
    MT.causal_attention(stacked, True, span=4)
    with pytest.raises(NotImplementedError, match="n_layers"):
        ST.ring_stream(stacked, 2)
    with pytest.raises(ValueError, match="HIP device"):                          # slots=True serves the stacked decoder, as device_stream
        ST.ring_stream(stacked, 2, slots=True)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    models = [MT.NLPTransformer(24, embed_dim=32, h=2, N=1, device=cpu), MT.UniTransformer(24, embed_dim=32, h=2, N=1, device=cpu),
              MT.UniFullTransformer(24, embed_dim=32, h=2, N=1, device=cpu),
              MT.MultiTransformer(mods, {"acoustic": 12, "emotient": 8}, N=1, h=2, device=cpu, embed_dim={"acoustic": 16, "emotient": 16}),
              M.MultiCNNTransformer(mods, dims, fuse_embed_size=32, device=cpu), M.MultiCNNTransformerB2(["emotient"], {"emotient": 8}, device=cpu),
              M.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=cpu),
              M.MultiCNNTransformerMFT(["emotient"], {"emotient": 8}, {"emotient": 16}, device=cpu)]
    for model in models:
        for slots in (False, True):
            name = "%s slots=%s" % (type(model).__name__, slots)
            MT.causal_attention(model, False)
            with pytest.raises(ValueError, match=r"\.eval\(\)"):
                ST.ring_stream(model.train(), 2, slots=slots)
            with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
                ST.ring_stream(model.eval(), 2, slots=slots)
            MT.causal_attention(model)
            with pytest.raises(ValueError, match=r"causal_attention\(model, span=W\)"):
                ST.ring_stream(model, 2, slots=slots)
            MT.causal_attention(model, True, span=4)
            with pytest.raises(ValueError, match="HIP device"):
                ST.ring_stream(model, 2, slots=slots)
            print("refused:", name)
    # no attention: no cache, nothing to lift
    for model in (MT.MultiTransformerB3(mods, {"acoustic": 12, "emotient": 8}, device=cpu), M.MultiCNNTransformerB3(mods, dims, device=cpu),
                  M.MultiLSTM(24, embed_dim=16, h_dim=16, device=cpu), M.MultiLSTMB1(24, embed_dim=16, h_dim=16, device=cpu)):
        for slots in (False, True):
            with pytest.raises(ValueError, match=r"stream\(batch\)"):
                ST.ring_stream(model.eval(), 2, slots=slots)


def test_the_wrappers_refuse_autograd_bad_positions_and_cpu_tensors():
    from multimodal_transformer_amd import streaming as ST
    x = torch.zeros(2, 32, requires_grad=True)
    state, flat = torch.zeros(4, dtype=torch.uint8), torch.zeros(4)
    with pytest.raises(NotImplementedError, match="autograd"):
        ST.encoder_ring_step(x, None, flat, state, 0, 2, 64, 1, 8)
    for t in (-1, INT_MAX, INT_MAX + 1):
        with pytest.raises(ValueError, match="INT_MAX"):
            ST.encoder_ring_step(x.detach(), None, flat, state, t, 2, 64, 1, 8)
    with pytest.raises(ValueError, match="span"):
        ST.encoder_ring_step(x.detach(), None, flat, state, 0, 2, 64, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):                       # t far beyond any capacity is a position here
        ST.encoder_ring_step(x.detach(), None, flat, state, 100000, 2, 64, 1, 8)
    with pytest.raises(ValueError, match="positions"):
        ST.encoder_ring_step_slots(x.detach(), None, flat, state, torch.zeros(2), 2, 64, 1, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ST.encoder_ring_step_slots(x.detach(), None, flat, state, torch.zeros(2, dtype=torch.int32), 2, 64, 1, 8)


# ------------------------------------------------------------------------------------------------ 4. C ABI without a GPU
def test_c_refusals_before_any_launch():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    dims = (4, 33, 128, 8, 128, 2)                                               # B, span, d, h, f, n_layers
    fake = ctypes.c_void_p(4096)                                                 # never dereferenced: each call below is refused first
    big = 1 << 40
    # span < 1, t < 0, t == INT_MAX: MMT_EINVAL with a message before anything else is looked at, null pointers included
    for args in ((None, None, None, None, None, 0), (fake, None, fake, fake, fake, big)):
        for t in (-1, -2 ** 31, INT_MAX):
            assert lib.mmt_encoder_stream_step_ring(*args, t, *dims, 1e-6, None) == MMT_EINVAL, t
            assert b"position t" in lib.mmt_last_error() and b"INT_MAX" in lib.mmt_last_error()
        for span in (0, -1):
            assert lib.mmt_encoder_stream_step_ring(*args, 0, 4, span, 128, 8, 128, 2, 1e-6, None) == MMT_EINVAL, span
            assert b"span" in lib.mmt_last_error()
            assert lib.mmt_encoder_stream_step_ring_slots(*args, fake, 1, 4, span, 128, 8, 128, 2, 1e-6, None) == MMT_EINVAL, span
            assert b"span" in lib.mmt_last_error()
    assert lib.mmt_encoder_stream_step_ring(None, None, None, None, None, 0, 0, *dims, 1e-6, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_encoder_stream_step_ring_slots(fake, None, fake, fake, fake, big, None, 1, *dims, 1e-6, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    # the size check is against mmt_encoder_stream_bytes(B, span, ...): one byte short is refused, for any t
    need = lib.mmt_encoder_stream_bytes(*dims)
    assert need > 0
    for t in (0, 32, 33, 4096, 100000, INT_MAX - 1):
        assert lib.mmt_encoder_stream_step_ring(fake, None, fake, fake, fake, need - 1, t, *dims, 1e-6, None) == MMT_EWORKSPACE, t
    assert lib.mmt_encoder_stream_step_ring_slots(fake, None, fake, fake, fake, need - 1, fake, 1, *dims, 1e-6, None) == MMT_EWORKSPACE
    # a span above the plan's limit: that limit's message
    assert lib.mmt_encoder_stream_step_ring(fake, None, fake, fake, fake, big, 0, 4, 4097, 128, 8, 128, 2, 1e-6, None) == MMT_EUNSUPPORTED
    assert b"capacity > 4096" in lib.mmt_last_error()
    assert lib.mmt_encoder_stream_step_ring_slots(fake, None, fake, fake, fake, big, fake, 1, 4, 4097, 128, 8, 128, 2, 1e-6, None) \
        == MMT_EUNSUPPORTED
    assert lib.mmt_encoder_stream_step_ring(fake, None, fake, fake, fake, big, 0, 4, 33, 256, 2, 128, 2, 1e-6, None) == MMT_EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ 5. the host check of the rule
def test_ring_plan_check_under_sanitizers(tmp_path):
    """tools/ring_plan_check.cpp, a stand-alone program built with -fsanitize=address,undefined (nothing is preloaded), walks the ring
    rule for every span in 1..70, 4095 and 4096 over the first steps, the steps around 4096 and the last positions below INT_MAX"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "ring_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "ring_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])
