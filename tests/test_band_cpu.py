"""CPU: the reference of band attention (tests/band_ref.py) against the exact function, and the surface of the feature (mmt_*_band,
the ``span`` keyword of functional, MultiHeadedAttention.span, multiTransformer.causal_attention(span=)).  No GPU: the library is
loaded, nothing is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import band_ref as Bn
import bf16_ref as E
import causal_ref as C
import recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = ["mmt_sdpa_forward_band", "mmt_sdpa_backward_band", "mmt_attn_probs_forward_band", "mmt_encoder_forward_band",
        "mmt_encoder_backward_band", "mmt_encoder_forward_band_devseed", "mmt_encoder_backward_band_devseed"]
MMT_EINVAL = 1


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def _inputs(T, d, lengths):
    B = len(lengths)
    q, k, v, g = (R.gen_normal("band_cpu" + n, (B, T, d), 5).double() for n in "qkvg")
    return q, k, v, g, R.prefix_mask(lengths, T).double()


def _ref(fn, q, k, v, g, h, *args, **kw):
    a = [t.clone().requires_grad_() for t in (q, k, v)]
    ctx, _ = fn(*(_split(t, h) for t in a), *args, **kw)
    ctx.permute(0, 2, 1, 3).reshape(q.shape).backward(g)
    return [ctx.detach()] + [t.grad for t in a]


@pytest.mark.parametrize("span", [1, 5, 32, 33, 64, 500])
def test_the_reference_is_the_exact_function(span):
    """band_ref.sdpa(rounding=False) == torch.softmax over scores with -inf outside the band, in fp64 to 1e-12: values and the three
    gradients, blanked query rows (Q' = 0: uniform over the min(t + 1, span) visible keys, no gradient to q) included"""
    T, d, h, lengths = 70, 40, 4, [70, 33, 1]
    dk = d // h
    q, k, v, g, rowm = _inputs(T, d, lengths)
    got = _ref(Bn.sdpa, q, k, v, g, h, span, rowm.unsqueeze(1), None, rounding=False)
    b = [t.clone().requires_grad_() for t in (q, k, v)]
    Q, K, V = (_split(t, h) for t in b)
    S = (Q * rowm.unsqueeze(1)) @ K.transpose(-2, -1) / dk ** 0.5
    t_ = torch.arange(T)
    out = (t_.reshape(1, T) > t_.reshape(T, 1)) | (t_.reshape(1, T) < t_.reshape(T, 1) - span + 1)      # written out, not band_ref's
    assert torch.equal(out, Bn.outside_band(T, span))
    P = torch.softmax(S.masked_fill(out, float("-inf")), dim=-1)
    assert (P.masked_select(out.expand_as(P)) == 0).all()
    direct = P @ V
    direct.permute(0, 2, 1, 3).reshape(len(lengths), T, d).backward(g)
    assert (got[0] - direct).abs().max().item() <= 1e-12
    for name, x, y in zip("qkv", got[1:], b):
        assert (x - y.grad).abs().max().item() <= 1e-12, name
    for bi, n in enumerate(lengths):
        assert (got[1][bi, n:] == 0).all()
        for t in range(n, T):
            lo, cnt = max(0, t - span + 1), min(t + 1, span)
            assert (P[bi, :, t, lo:t + 1] - 1.0 / cnt).abs().max().item() <= 1e-15
    if span == 1:
        assert (got[0] - _split(v, h)).abs().max().item() <= 1e-15          # a query sees itself only


@pytest.mark.parametrize("span", [70, 71, 500])
def test_a_span_of_at_least_T_is_causal_attention(span):
    T, d, h, lengths = 70, 40, 4, [70, 33, 1]
    q, k, v, g, rowm = _inputs(T, d, lengths)
    a = _ref(Bn.sdpa, q, k, v, g, h, span, rowm.unsqueeze(1), None, rounding=False)
    b = _ref(C.sdpa, q, k, v, g, h, rowm.unsqueeze(1), None, rounding=False)
    for x, y in zip(a, b):
        assert (x - y).abs().max().item() <= 1e-12


@pytest.mark.parametrize("span", [1, 7, 32, 40])
def test_truncation_identity(span):
    """row t of band attention == the last row of plain bf16_ref.sdpa(rounding=False) on the sequence cut to windows
    t - span + 1 .. t, to 1e-12"""
    T, d, h = 45, 16, 2
    q, k, v, _, _ = _inputs(T, d, [T, T])
    ctx, _ = Bn.sdpa(_split(q, h), _split(k, h), _split(v, h), span, None, None, rounding=False)
    for t in range(T):
        lo = max(0, t - span + 1)
        cut, _ = E.sdpa(_split(q[:, lo:t + 1], h), _split(k[:, lo:t + 1], h), _split(v[:, lo:t + 1], h), None, None, rounding=False)
        assert (ctx[:, :, t] - cut[:, :, -1]).abs().max().item() <= 1e-12, t


@pytest.mark.parametrize("T,span", [(70, 33), (290, 40), (290, 100)])
def test_rounded_reference_stays_near_the_exact_function(T, span):
    """the bf16 roundings move the band reference by what they move the plain one: well under 2 % rel-L2 on values and gradients (a
    wrong tile sweep, a mask taken after the maximum or a NaN from an all-masked tile moves them by tens of percent); T = 290 has rows
    whose lower-edge tile holds no visible key"""
    d, h, lengths = 32, 2, [T, (2 * T) // 3]
    q, k, v, g, rowm = _inputs(T, d, lengths)
    res = [_ref(Bn.sdpa, q, k, v, g, h, span, rowm.unsqueeze(1), None, rounding=r) for r in (True, False)]
    for x, y in zip(*res):
        assert torch.isfinite(x).all() and ((x - y).norm() / y.norm()).item() < 2e-2


def test_the_reference_stack_is_the_causal_one_at_a_full_span():
    d, h, n, T = 32, 2, 2, 40
    p = {k_: v_.double() for k_, v_ in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17).items()}
    x = R.gen_normal("band_cpu:x", (2, T, d), 17).double()
    mask = R.prefix_mask([T, 11], T).double()
    a = Bn.encoder_stack(p, "", x, mask, h, T, rounding=False)
    b = C.encoder_stack(p, "", x, mask, h, rounding=False)
    c = Bn.encoder_stack(p, "", x, mask, h, 3, rounding=False)
    assert (a - b).abs().max().item() <= 1e-12 and (a - c).abs().max().item() > 1e-3
    x2 = x.clone()
    x2[:, :10] += 1.0                                            # two layers of span 3 reach back 4 windows
    c2 = Bn.encoder_stack(p, "", x2, mask, h, 3, rounding=False)
    assert torch.equal(c[:, 14:], c2[:, 14:]) and not torch.equal(c[:, 10:14], c2[:, 10:14])


# ------------------------------------------------------------------------------------------------ yardsticks of the widened bounds
# tests/test_gpu_band.py runs `cold` and `hot` of tests/value_regimes.py (d = 32, h = 2, two sequences) through the band kernels.  There
# the scores are ~ +-600 and carry ~6e-5 absolute in fp32, and dq = sum_j dS_j K_j cancels a component of 40 per key (the note at
# test_value_regimes_cpu.SDPA_FP32_YARD), so the bounds of test_gpu_bf16_faithful do not hold for any fp32 evaluation.  The rule of the
# other tiers: a bound is the default or 4x a yardstick that involves no kernel, whichever is wider.  The yardstick is band_ref.sdpa
# evaluated in float32 against its float64 result, the worst over the two regimes in eval mode and under one p = 0.25 mask from
# torch's CPU generator, per (T, span) and tensor as (rel-L2, per-row maximum).  Recorded here, checked below against a fresh
# evaluation: a constant may understate its yardstick, never overstate it.  (jitter(6e-8), seeds 0 .. 3, moves these cases by at most
# 3.8e-4 / 9.2e-3, dq at T = 290: the float32 evaluation is the wider yardstick throughout.)  The evaluation gives, T = 70: y 3.8e-4 /
# 3.2e-3, dq 1.3e-2 / 1.2e-1, dk 2.5e-3 / 2.0e-2, dv 4.0e-4 / 4.4e-3; T = 290: y 2.0e-4 / 2.4e-3, dq 1.1e-2 / 1.4e-1, dk 2.4e-3 / 4.3e-2,
# dv 7.0e-4 / 1.1e-2.  The constants stand about 15 % under it: another CPU's float32 sums land a few percent away.
BAND_VR_SHAPE = (2, 32, 2)                                      # B, d, h
BAND_VR_CASES = ((70, 33), (290, 40))                           # (T, span)
BAND_FP32_YARD = {
    (70, 33): {"y": (3.2e-4, 2.7e-3), "dq": (1.1e-2, 1.0e-1), "dk": (2.1e-3, 1.7e-2), "dv": (3.4e-4, 3.7e-3)},
    (290, 40): {"y": (1.6e-4, 2.0e-3), "dq": (9.0e-3, 1.2e-1), "dk": (2.0e-3, 3.7e-2), "dv": (5.9e-4, 9.0e-3)},
}


def band_vr_inputs(regime, T):
    """-> q, k, v, g (B, T, d) and the query-row mask (B, T, 1) of the regime"""
    import value_regimes as V
    B, d, h = BAND_VR_SHAPE
    return V.attention(regime, B, T, d, h) + (R.prefix_mask(V.attn_lengths(T), T),)


def band_vr_reference(regime, T, span, drop=None, dtype=torch.float64):
    """{y, dq, dk, dv} of band_ref.sdpa on the regime's inputs, evaluated in `dtype`"""
    B, d, h = BAND_VR_SHAPE
    q, k, v, g, mask = band_vr_inputs(regime, T)
    lt = [t.to(dtype).requires_grad_() for t in (q, k, v)]
    ctx, _ = Bn.sdpa(*(_split(t, h) for t in lt), span, mask.to(dtype).unsqueeze(1), None if drop is None else drop.to(dtype))
    y = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    y.backward(g.to(dtype))
    return {"y": y.detach().double(), "dq": lt[0].grad.double(), "dk": lt[1].grad.double(), "dv": lt[2].grad.double()}


def band_fp32_yardstick(T, span):
    from gpu_harness import measures
    B, d, h = BAND_VR_SHAPE
    keep = (torch.rand(B, h, T, T, generator=torch.Generator().manual_seed(1)) >= 0.25).double() / 0.75
    worst = {}
    for regime in ("cold", "hot"):
        for drop in (None, keep):
            a = band_vr_reference(regime, T, span, drop)
            b = band_vr_reference(regime, T, span, drop, dtype=torch.float32)
            for n in a:
                rel, row = measures(b[n].numpy(), a[n].numpy())
                worst[n] = (max(rel, worst.get(n, (0, 0))[0]), max(row, worst.get(n, (0, 0))[1]))
    return worst


@pytest.mark.parametrize("T,span", BAND_VR_CASES)
def test_recorded_band_yardsticks_do_not_overstate(T, span):
    fresh = band_fp32_yardstick(T, span)
    print("band fp32 yardstick T %d span %d: %s" % (T, span, {n: "%.2e / %.2e" % v for n, v in fresh.items()}))
    for n, (rel, row) in BAND_FP32_YARD[(T, span)].items():
        assert rel <= fresh[n][0] and row <= fresh[n][1], n


# ------------------------------------------------------------------------------------------------ the surface
def test_band_entries_are_declared_exported_and_bound():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmt_hip.h")).read(), flags=re.S)
    for name in BAND:
        plain = name.replace("_band", "")
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[plain]
        assert _lib.SIGNATURES[name] == (res, args[:-1] + [ctypes.c_int] + args[-1:]), name      # int span in front of the stream

        def params(n):
            return re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, header).group(1))
        assert params(name) == params(plain).replace("mmt_stream_t stream", "int span, mmt_stream_t stream"), name
    assert lib.mmt_abi_version() == 1
    assert _lib.entry_name("mmt_sdpa_forward", causal=True, band=True) == "mmt_sdpa_forward_band"
    assert _lib.entry_name("mmt_encoder_backward", causal=True, band=True, devseed=True) == "mmt_encoder_backward_band_devseed"
    assert _lib.entry_name("mmt_sdpa_forward", causal=True) == "mmt_sdpa_forward_causal"
    with pytest.raises(ValueError, match="span"):
        _lib.entry_name("mmt_sdpa_forward", band=True)


@pytest.mark.parametrize("span", [0, -3])
def test_band_entries_refuse_a_span_below_one(span):
    """MMT_EINVAL naming the span, before any pointer is looked at and without a device"""
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the refusal comes first
    enc = (2, 33, 128, 8, 128, 2, 1e-6, 0.0)
    calls = [lambda s: lib.mmt_sdpa_forward_band(one, one, one, one, one, one, 1 << 30, 2, 33, 32, 2, 0.0, 0, s, None),
             lambda s: lib.mmt_sdpa_backward_band(one, one, one, one, one, one, 1 << 30, 2, 33, 32, 2, 0.0, 0, s, None),
             lambda s: lib.mmt_attn_probs_forward_band(one, one, one, one, 2, 33, 32, 2, 0.0, 0, s, None),
             lambda s: lib.mmt_encoder_forward_band(one, one, one, one, one, 1 << 30, *enc, 0, s, None),
             lambda s: lib.mmt_encoder_backward_band(one, one, one, one, one, one, one, 1 << 30, *enc, 0, s, None),
             lambda s: lib.mmt_encoder_forward_band_devseed(one, one, one, one, one, 1 << 30, *enc, one, s, None),
             lambda s: lib.mmt_encoder_backward_band_devseed(one, one, one, one, one, one, one, 1 << 30, *enc, s, None)]
    for i, call in enumerate(calls):
        assert call(span) == MMT_EINVAL, i
        assert b"span" in lib.mmt_last_error(), i
    # with a valid span the plain entry's refusals follow
    assert lib.mmt_sdpa_forward_band(None, None, None, None, None, None, 0, 2, 33, 32, 2, 0.0, 0, 4, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_encoder_forward_band_devseed(one, one, one, one, one, 1 << 30, *enc, None, 4, None) == MMT_EINVAL
    assert b"seed state" in lib.mmt_last_error()
    assert lib.mmt_attn_probs_forward_band(one, one, one, one, 2, 33, 33, 2, 0.0, 0, 4, None) == MMT_EINVAL


def test_python_surface():
    from multimodal_transformer_amd import _lib, functional as F, multiTransformer as MT
    for fn in (F.sdpa, F.attn_probs, F.encoder_stack, F.encoder_stack_params, _lib.launch, MT.causal_attention):
        assert inspect.signature(fn).parameters["span"].default is None, fn.__name__
    mha = MT.MultiHeadedAttention(2, 8)
    assert MT.MultiHeadedAttention.span is None and "span" not in mha.__dict__
    assert mha.attention_mode() == (False, False) and mha.attention_span() is None
    assert MT.causal_attention(mha, span=5) == {"": mha} and mha.causal is True and mha.span == 5
    assert mha.attention_mode() == (False, True) and mha.attention_span() == 5              # two values, as before
    MT.causal_attention(mha)
    assert mha.causal is True and mha.span is None
    MT.causal_attention(mha, span=5)
    MT.causal_attention(mha, False)
    assert mha.causal is False and mha.span is None                                         # on=False clears the span
    model = MT.MultiTransformer(["acoustic", "emotient"], {"acoustic": 12, "emotient": 20}, N=2, d_ff=16, h=2, device=torch.device("cpu"),
                                embed_dim={"acoustic": 16, "emotient": 8})
    found = MT.causal_attention(model, span=7)
    assert len(found) == 2 * (2 + 1) and all(m.causal and m.span == 7 for m in found.values())
    enc = next(m for m in model.modules() if isinstance(m, MT.Encoder))
    assert enc._fusable()                                # a span does not force the layer-by-layer path ...
    enc.layers[1].self_attn.span = 8
    assert not enc._fusable()                            # ... layers that disagree about it do
    MT.causal_attention(model, False)
    assert enc._fusable() and not any(m.causal or m.span is not None for m in found.values())


def test_every_refusal_of_a_span():
    """ValueError naming the reason, raised by the argument check, which runs on any device: nothing is launched"""
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    kl = torch.tensor([3, 1], dtype=torch.int32)
    x = torch.zeros(2, 8, 16)
    mask = torch.ones(2, 8, 1)
    flat = torch.zeros(10)
    assert F._check_span("sdpa", None, True, 4) == 4 and F._check_span("sdpa", kl, False, None) is None

    def calls(**kw):
        return (lambda: F.sdpa(x, x, x, mask, 2, **kw), lambda: F.attn_probs(x, x, mask, 2, **kw),
                lambda: F.encoder_stack(x, mask, flat, 2, 16, 1, **kw),
                lambda: F.encoder_stack_params(x, mask, [flat], 2, 16, 1, flat=flat, **kw))

    for kw, words in [(dict(span=4), "without causal=True"), (dict(span=4, causal=False), "without causal=True"),
                      (dict(span=4, causal=True, key_lengths=kl), "key_lengths and span"),
                      (dict(span=4, key_lengths=kl), "key_lengths and span"),
                      (dict(span=0, causal=True), "span must be >= 1"), (dict(span=-2, causal=True), "span must be >= 1"),
                      (dict(span=True, causal=True), "must be an int"), (dict(span=4.0, causal=True), "must be an int"),
                      (dict(span="4", causal=True), "must be an int")]:
        for call in calls(**kw):
            with pytest.raises(ValueError, match=words):
                call()
    # the module path: the call raises before anything else happens (CPU tensors would be refused next)
    for attrs, words in [(dict(span=4), "without causal=True"), (dict(span=4, mask_keys=True), "key_lengths and span"),
                         (dict(span=0, causal=True), "span must be >= 1"), (dict(span=True, causal=True), "must be an int"),
                         (dict(span=2.5, causal=True), "must be an int"), (dict(span=4, causal=True, mask_keys=True), "mask_keys.*causal")]:
        mha = MT.MultiHeadedAttention(2, 16)
        for k_, v_ in attrs.items():
            setattr(mha, k_, v_)
        with pytest.raises(ValueError, match=words):
            mha(x, x, x, mask)
        enc = MT.Encoder(MT.EncoderLayer(16, MT.MultiHeadedAttention(2, 16), MT.PositionwiseFeedForward(16, 16), 0.1), 2)
        for layer in enc.layers:
            for k_, v_ in attrs.items():
                setattr(layer.self_attn, k_, v_)
        assert enc._fusable()
        with pytest.raises(ValueError, match=words):
            enc(x, mask)
    for bad, words in [(0, "span must be >= 1"), (True, "must be an int"), (3.0, "must be an int")]:
        with pytest.raises(ValueError, match=words):
            MT.causal_attention(MT.MultiHeadedAttention(2, 16), span=bad)
    with pytest.raises(ValueError, match="without causal=True"):
        MT.causal_attention(MT.MultiHeadedAttention(2, 16), False, span=4)
    # the refusals of causal alone keep their words
    with pytest.raises(ValueError, match="key_lengths.*causal"):
        F.sdpa(x, x, x, mask, 2, key_lengths=kl, causal=True)


def test_streams_refuse_a_span_on_cpu():
    """every stream that opens an encoder stream on layers with a span raises at open, naming the follow-up, before the device check"""
    import multimodal_transformer_amd as m
    MT, M = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    enc = MT.Encoder(MT.EncoderLayer(32, MT.MultiHeadedAttention(2, 32), MT.PositionwiseFeedForward(32, 64, 0.1), 0.1), 2).eval()
    MT.causal_attention(enc, span=4)
    for open_ in (lambda: enc.stream(2, 8), lambda: enc.slot_stream(2, 8)):
        with pytest.raises(ValueError, match=r"span = 4.*ring cache"):
            open_()
    MT.causal_attention(enc)
    with pytest.raises(ValueError, match="HIP device"):                  # without a span: the next refusal, as before
        enc.stream(2, 8)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    single = ("stream", "device_stream")                                 # (their slot_stream is refused for every model)
    models = [(MT.NLPTransformer(24, embed_dim=32, h=2, N=1, device=cpu), single),
              (MT.UniTransformer(24, embed_dim=32, h=2, N=1, device=cpu), single),
              (MT.UniFullTransformer(24, embed_dim=32, h=2, N=1, device=cpu), single),
              (MT.MultiTransformer(mods, dims, N=1, d_ff=16, h=2, device=cpu, embed_dim={"acoustic": 16, "emotient": 8}),
               ("stream", "slot_stream")),
              (M.MultiCNNTransformer(mods, dims, fuse_embed_size=32, device=cpu), single)]
    for model, methods in models:
        MT.causal_attention(model.eval(), span=4)
        for method in methods:
            with pytest.raises(ValueError, match=r"span = 4.*ring cache"):
                getattr(model, method)(2, 8)
