"""GPU: banded causal self-attention (csrc/attn.h *_band_kernel, csrc/attn_probs.h, the ``span`` keyword of functional.sdpa / attn_probs /
encoder_stack, MultiHeadedAttention.span, multiTransformer.causal_attention(span=)): query t attends keys max(0, t-span+1) .. t.

The reference is tests/band_ref.py (tests/test_band_cpu.py holds it to the exact function in fp64); the bounds are those of
tests/test_gpu_bf16_faithful.py, imported as tests/test_gpu_causal.py imports them: the arithmetic per score is the same, with fewer
terms per row.  Measured worst values on the MI355X stand beside each use.
"""
import numpy as np
import pytest
import torch

import band_ref as Bn
import bf16_ref as E
import recipe as R
import test_band_cpu as BC
from gpu_harness import check, dev, device_kernel_names, library_kernels, mta  # noqa: F401 (dev: fixture)
from test_gpu_bf16_faithful import (ENC_GRAD, ENC_OUT, ENC_OUT_ROW, ENC_RELU_GRAD, ENC_ROW, ENC_W_SCALE, SDPA_GRAD, SDPA_GRAD_ROW, SDPA_OUT,
                                    SDPA_OUT_ROW)
from test_gpu_causal import _CAUSAL, _PLAIN, _enc_drops, _launched, _split

pytestmark = pytest.mark.gpu

# (T, d, h, span): the smallest shapes that reach every sweep bound, both edge tiles, the idle states at both ends and every DKP
CASES = [(1, 32, 2, 1),          # smallest shape
         (33, 32, 2, 1),         # self only
         (33, 32, 2, 5),         # edges and diagonal in one tile
         (70, 32, 2, 32),        # span = one tile
         (70, 32, 2, 33),        # one key into the next tile
         (70, 40, 4, 500),       # span >= T, d_k = 10 padded
         (130, 64, 2, 40),       # d_k = 32, a quad boundary
         (130, 128, 2, 64),      # d_k = 64, two launches per kernel
         (290, 32, 2, 40),       # three quads, 10 tiles
         (290, 32, 2, 100),      # same, wider band
         (290, 32, 2, 200)]      # same, wider still
IDS = ["T%d_d%d_h%d_s%d" % c for c in CASES]
P_TRAIN, SEED = 0.25, 20261020
MODES = [0.0, P_TRAIN]
MODE_IDS = ["eval", "train"]
_BAND = ("attn_fwd_band_kernel", "attn_bwd_dkv_band_kernel", "attn_bwd_dq_band_kernel", "attn_probs_band_kernel")

_CACHE = {}


def _lengths(T):
    return [T, max(1, (2 * T) // 3), 1]


def _sdpa_call(F, q, k, v, g, mask, h, p, **kw):
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    y = F.sdpa(*leaves, mask, h, dropout_p=p, seed=SEED if p else 0, **kw)
    y.backward(g)
    return dict(zip(("y", "dq", "dk", "dv"), [y.detach().cpu()] + [t.grad.cpu() for t in leaves]))


def _run(case, p, dev):
    """every GPU result of one (case, mode), computed once: the band call, twice, and the band and plain maps"""
    key = (case, p)
    if key in _CACHE:
        return _CACHE[key]
    T, d, h, span = case
    lengths = _lengths(T)
    B = len(lengths)
    F = mta().functional
    tag = "band%d_%d_%d" % case[:3]
    q, k, v, g = (R.gen_normal(tag + n, (B, T, d), 13) for n in "qkvg")
    q = 2 * q
    mask = R.prefix_mask(lengths, T)
    qg, kg, vg, gg, mg = (t.to(dev) for t in (q, k, v, g, mask))
    seed = SEED if p else 0
    scale = F.dropout_mask(p, seed, 0, 1024, dev, attn_Tp=32)[1] if p else 1.0        # of a kept probability: 1/(1-p) at the generator's resolution
    out = {"scale": scale, "q": q, "k": k, "v": v, "g": g, "mask": mask, "lengths": lengths, "gpu": (qg, kg, vg, gg, mg),
           "band": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, causal=True, span=span),
           "again": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, causal=True, span=span),
           "map": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed, causal=True, span=span).cpu(),
           "map_plain": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed).cpu()}
    torch.cuda.synchronize()
    F.check_device_errors()
    _CACHE[key] = out
    return out


def _against_ref(tag, got, q, k, v, g, mask, h, span, drop, yard=None):
    """ctx, dq, dk, dv of `got` against band_ref.sdpa under the imported bounds, or 4x the yardstick of a tensor where that is wider"""
    def bounds(name, default):
        return default if yard is None else tuple(max(d_, 4 * y_) for d_, y_ in zip(default, yard[name]))

    B, T, d = q.shape
    lt = [t.double().requires_grad_() for t in (q, k, v)]
    ctx, _ = Bn.sdpa(*(_split(t, h) for t in lt), span, mask.double().unsqueeze(1), drop)
    y = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    y.backward(g.double())
    failures = []
    for name in got:
        if not torch.isfinite(got[name]).all():
            failures.append("%s %s: %d entries are not finite" % (tag, name, int((~torch.isfinite(got[name])).sum())))
    check(tag + " y", got["y"], y.detach(), *bounds("y", (SDPA_OUT, SDPA_OUT_ROW)), failures=failures)
    for name, t in zip(("dq", "dk", "dv"), lt):
        # with one visible key per row dq and dk are analytically zero (the softmax is constant): measured on dv's scale
        zero = name != "dv" and float(t.grad.norm()) < 1e-9 * float(lt[2].grad.norm())
        check(tag + " " + name, got[name], t.grad, *bounds(name, (SDPA_GRAD, SDPA_GRAD_ROW)), scale_ref=lt[2].grad if zero else None,
              failures=failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sdpa_against_the_band_reference(dev, case, p):
    """ctx, dq, dk, dv against band_ref.sdpa.  Train mode: the drop multipliers are those of the band map for the same seed (0 where it
    is 0 inside the band, 1/(1-p) elsewhere; entries outside the band are never read).
    Measured worst (rel-L2 / per-row maximum) over the cases: see DESIGN.md 4.10."""
    T, d, h, span = case
    c = _run(case, p, dev)
    drop = None
    if p:
        drop = ((c["map"] != 0) | Bn.outside_band(T, span)).double() * c["scale"]
    _against_ref("band sdpa T%d d%d s%d p%g" % (T, d, span, p), c["band"], c["q"], c["k"], c["v"], c["g"], c["mask"], h, span, drop)


# ------------------------------------------------------------------------------------------------ 2. exact facts
@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_facts(dev, case, p):
    T, d, h, span = case
    c = _run(case, p, dev)
    P, got = c["map"], c["band"]
    B = len(c["lengths"])
    out = Bn.outside_band(T, span)
    assert P.shape == (B, h, T, T) and torch.isfinite(P).all() and (P >= 0).all()
    assert (P.masked_select(out.expand_as(P)) == 0).all()                          # exact zeros on both sides, written by the kernel
    for name in got:                                                               # two runs are bit-identical
        assert torch.isfinite(got[name]).all() and torch.equal(got[name], c["again"][name]), name
    for b, n in enumerate(c["lengths"]):
        assert (got["dq"][b, n:] == 0).all(), b                                    # blanked query rows pass no gradient to q
    if p:
        # the keep decisions are the plain map's, per position
        assert torch.equal((P == 0) & ~out, (c["map_plain"] == 0) & ~out)
        return
    err = (P.double().sum(dim=-1) - 1.0).abs().max().item()
    print("band map T%d span %d row-sum error %.3e" % (T, span, err))
    assert err <= 1e-5
    for b, n in enumerate(c["lengths"]):
        for t in range(n, T):                                                      # a blanked query row: uniform over its visible keys
            cnt = min(t + 1, span)
            uniform = torch.full((cnt,), 1 / cnt, dtype=torch.float32)
            for head in range(h):
                assert torch.equal(P[b, head, t, t + 1 - cnt:t + 1], uniform), (b, head, t)
    if span == 1:
        assert torch.equal(got["y"], c["v"].bfloat16().float())                    # a query sees itself only: ctx = bf16(v), bit for bit
    else:
        assert torch.equal(got["y"][:, 0], c["v"][:, 0].bfloat16().float())


# ------------------------------------------------------------------------------------------------ 3. locality in both directions
LOC = CASES[8]                   # T = 290, span = 40


def _perturbed(c, lo, hi):
    """q, k, v changed at windows < lo and at windows >= hi"""
    out = []
    for i, t in enumerate(c["gpu"][:3]):
        t = t.clone()
        t[:, :lo] = 1.5 * t[:, :lo] + 0.25 * (i + 1)
        t[:, hi:] = 1.5 * t[:, hi:] + 0.25 * (i + 1)
        out.append(t)
    return out


@pytest.mark.parametrize("qt", [2, 4, 5, 7, 8])
def test_locality_of_sdpa(dev, qt):
    """q, k, v changed at windows >= 32 qt + 32 (ahead) or < 32 qt - span + 1 (behind): every row of query tile qt stays bit-equal
    (tile granularity: the rescale decision is per 32-query tile).  The causal call fails the look-behind half, the plain call both."""
    T, d, h, span = LOC
    F = mta().functional
    c = _run(LOC, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]
    rows = slice(32 * qt, 32 * qt + 32)
    lo, hi = 32 * qt - span + 1, 32 * qt + 32
    ahead, behind = _perturbed(c, 0, hi), _perturbed(c, lo, T)
    with torch.no_grad():
        def run(ops, **kw):
            return F.sdpa(*ops, mg, h, **kw).cpu()[:, rows]
        base = (qg, kg, vg)
        band = dict(causal=True, span=span)
        a = run(base, **band)
        assert torch.equal(a, c["band"]["y"][:, rows])
        assert torch.equal(a, run(ahead, **band)) and torch.equal(a, run(behind, **band))
        both = _perturbed(c, lo, hi)
        assert torch.equal(a, run(both, **band))
        inside = _perturbed(c, lo + 1, T)                                          # one window into the band: seen
        assert not torch.equal(a, run(inside, **band))
        ca = run(base, causal=True)
        assert torch.equal(ca, run(ahead, causal=True)) and not torch.equal(ca, run(behind, causal=True))
        pa = run(base)
        assert not torch.equal(pa, run(ahead)) and not torch.equal(pa, run(behind))
    F.check_device_errors()


@pytest.mark.parametrize("d,h", [(128, 8), (40, 4)])
@pytest.mark.parametrize("qt", [4, 7])
def test_locality_through_the_encoder_stack(dev, d, h, qt):
    """two layers, eval mode, T = 290, span = 40, x changed ahead of query tile qt or behind its receptive field of two layers: y is
    bit-equal on the rows of tile qt (d = 128: the fixed-shape chains; d = 40: the generic ones).  The receptive field widens by
    span - 1 per layer as a function; bit for bit the first layer's rows must come from clean TILES, so the look-behind edge is that
    of the tile that holds window 32 qt - span + 1.  The causal stack fails the look-behind half, the plain stack both."""
    T, span = LOC[0], LOC[3]
    F = mta().functional
    B, n = 2, 2
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev)
    x = R.gen_normal("band_local_d%d:x" % d, (B, T, d), 17).to(dev)
    mask = R.prefix_mask([T, 250], T).to(dev)
    rows = slice(32 * qt, 32 * qt + 32)
    hi = 32 * qt + 32
    lo = 32 * ((32 * qt - span + 1) // 32) - span + 1
    assert 0 < lo <= 32 * qt - 2 * (span - 1)
    ahead, behind = x.clone(), x.clone()
    ahead[:, hi:] = 1.5 * ahead[:, hi:] + 0.25
    behind[:, :lo] = 1.5 * behind[:, :lo] + 0.25
    with torch.no_grad():
        def run(t, **kw):
            return F.encoder_stack(t, mask, flat, h, R.D_FF, n, **kw).cpu()[:, rows]
        band = dict(causal=True, span=span)
        a = run(x, **band)
        assert torch.isfinite(a).all() and torch.equal(a, run(ahead, **band)) and torch.equal(a, run(behind, **band))
        ca = run(x, causal=True)
        assert torch.equal(ca, run(ahead, causal=True)) and not torch.equal(ca, run(behind, causal=True))
        pa = run(x)
        assert not torch.equal(pa, run(ahead)) and not torch.equal(pa, run(behind))
    F.check_device_errors()


# ------------------------------------------------------------------------------------------------ 4. value regimes
@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("regime", ["cold", "hot"])
@pytest.mark.parametrize("T,span", BC.BAND_VR_CASES)
def test_value_regimes(dev, T, span, regime, p):
    """`cold` (row maxima below -128) and `hot` (above +128) of tests/value_regimes.py: rows whose swept tiles below the diagonal hold
    no visible key.  Every output and gradient is finite and inside the bounds: those of test_gpu_bf16_faithful, or 4x the fp32
    yardstick of the case where that is wider (test_band_cpu.BAND_FP32_YARD says why, as test_gpu_value_regimes does for these
    regimes).  Measured: DESIGN.md 4.10."""
    B, d, h = BC.BAND_VR_SHAPE
    F = mta().functional
    q, k, v, g, mask = BC.band_vr_inputs(regime, T)
    qg, kg, vg, gg, mg = (t.to(dev) for t in (q, k, v, g, mask))
    got = _sdpa_call(F, qg, kg, vg, gg, mg, h, p, causal=True, span=span)
    drop = None
    if p:
        P = F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=SEED, causal=True, span=span).cpu()
        assert torch.isfinite(P).all()
        drop = ((P != 0) | Bn.outside_band(T, span)).double() * F.dropout_mask(p, SEED, 0, 1024, dev, attn_Tp=32)[1]
    F.check_device_errors()
    _against_ref("band %s T%d s%d p%g" % (regime, T, span, p), got, q, k, v, g, mask, h, span, drop, BC.BAND_FP32_YARD[(T, span)])


# ------------------------------------------------------------------------------------------------ 5. kernel names
@pytest.mark.parametrize("case", [CASES[2], CASES[8]], ids=[IDS[2], IDS[8]])
def test_kernel_names(dev, case):
    T, d, h, span = case
    F = mta().functional
    c = _run(case, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]

    def call():
        _sdpa_call(F, qg, kg, vg, gg, mg, h, 0.0, causal=True, span=span)
        F.attn_probs(qg, kg, mg, h, causal=True, span=span)

    _, names = device_kernel_names(call)
    if names is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert _launched(names, _BAND) == sorted(_BAND), names
    assert _launched(names, _PLAIN + _CAUSAL) == [], names              # no plain, keyed or causal kernel, no one-kernel backward: also at T = 290


# ------------------------------------------------------------------------------------------------ 6. encoder stack
ENC = [(128, 8, 2, 3, 70, [70, 33, 1], 40),        # the fixed-shape chains
       (40, 4, 2, 2, 45, [45, 20], 7)]             # the generic chains
ENC_IDS = ["d%d_n%d_T%d_s%d" % (c[0], c[2], c[4], c[6]) for c in ENC]
_ENC_REF = {}


def _enc_inputs(c):
    d, h, n, B, T, lengths, span = c
    cid = "band_enc_d%d_T%d" % (d, T)
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    return p32, R.gen_normal(cid + ":x", (B, T, d), 17), R.prefix_mask(lengths, T), R.gen_normal(cid + ":g", (B, T, d), 17)


def _enc_ref(F, c, p, seed, dev):
    key = (c[0], c[4], p, seed)
    if key not in _ENC_REF:
        d, h, n, B, T, lengths, span = c
        p32, x, mask, g = _enc_inputs(c)
        pd = {k: v.double().clone().requires_grad_() for k, v in p32.items()}
        xd = x.double().requires_grad_()
        y = Bn.encoder_stack(pd, "", xd, mask.double(), h, span, _enc_drops(F, c[:6], p, seed, dev) if p else None)
        y.backward(g.double())
        _ENC_REF[key] = (y.detach().numpy(), xd.grad.numpy(), {k: v.grad.numpy() for k, v in pd.items()})
    return _ENC_REF[key]


@pytest.mark.parametrize("mode", ["eval", "train", "train_devseed"])
@pytest.mark.parametrize("c", ENC, ids=ENC_IDS)
def test_encoder_stack_against_the_band_reference(dev, c, mode):
    """y, dx and every parameter gradient against band_ref.encoder_stack under the bounds and per-tensor rules of
    test_gpu_bf16_faithful.test_encoder_stack; train mode at p = 0.25 with the seed by value and with a device-resident seed (the
    _band_devseed twins), whose first forward uses the value it was made with: the two give the same bits."""
    d, h, n, B, T, lengths, span = c
    F = mta().functional
    p = 0.0 if mode == "eval" else P_TRAIN
    value = 4343 + d + T
    seed = mta()._lib.DeviceSeed(dev, value) if mode == "train_devseed" else value
    if mode == "train_devseed":
        assert seed.peek() == value
    p32, x, mask, g = _enc_inputs(c)

    def run(sd):
        flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
        xg = x.to(dev).requires_grad_()
        y = F.encoder_stack(xg, mask.to(dev), flat, h, R.D_FF, n, dropout_p=p, seed=sd if p else 0, causal=True, span=span)
        y.backward(g.to(dev))
        F.check_device_errors()
        return y, xg, flat

    y, xg, flat = run(seed)
    if mode == "train_devseed":                          # a by-value seed and a device seed give the same bits
        other = run(value)
        assert all(torch.equal(a_, b_) for a_, b_ in zip((y, xg.grad, flat.grad), (other[0], other[1].grad, other[2].grad)))
    y_ref, dx_ref, grads = _enc_ref(F, c, p, value if p else 0, dev)
    tag = "band enc d%d n%d T%d s%d %s" % (d, n, T, span, mode)
    failures = []
    check(tag + " y", y.detach().cpu(), y_ref, ENC_OUT, ENC_OUT_ROW, failures=failures)
    check(tag + " dx", xg.grad.cpu(), dx_ref, ENC_GRAD, ENC_ROW, failures=failures)
    got_flat, off = flat.grad.cpu().numpy(), 0
    for name, shape in E.encoder_param_shapes(d, R.D_FF, n).items():
        size = int(np.prod(shape))
        got = got_flat[off: off + size].reshape(shape)
        off += size
        scale = grads[name.replace("linears.1.bias", "linears.0.bias")] if "linears.1.bias" in name else None     # analytically zero
        flips = ".w_1." in name or "sublayer.1.norm" in name
        check(tag + " " + name, got, grads[name], ENC_RELU_GRAD if flips else ENC_GRAD, None if flips else ENC_ROW, scale_ref=scale,
              failures=failures)
        if len(shape) == 2:
            r = grads[name].astype(np.float64).ravel()
            s = float(np.dot(got.astype(np.float64).ravel() - r, r) / np.dot(r, r))
            if abs(s) > ENC_W_SCALE:
                failures.append("%s %s: scale %.3e > %.1e" % (tag, name, s, ENC_W_SCALE))
    assert off == got_flat.size
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 7. training, capture
def test_train_step_with_a_span(dev):
    """one train step of the SFT with a span: finite gradients for every parameter that gets one without it, hand-written kernels
    only, the band attention kernels and no other; causal_attention(model, False) restores the launch sequence of a run made before"""
    MT, F = mta().multiTransformer, mta().functional
    B, T, lengths = 4, 40, [40, 33, 20, 5]
    model = MT.NLPTransformer(512, embed_dim=128, h=8, N=2, device=dev).train()
    x = torch.tanh(R.gen_normal("band_train:x", (B, T, 512), 3)).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("band_train:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        torch.manual_seed(77)
        F.mse_sum_loss_backward(model(x, mask, lengths), tgt, sum(lengths))

    _, before = device_kernel_names(step, warm=True)                 # the flag was never set
    with_grad = [q.grad is not None for q in params]
    found = MT.causal_attention(model, span=12)
    assert found and all(m.causal and m.span == 12 for m in found.values())
    _, names = device_kernel_names(step, warm=True)
    assert [q.grad is not None for q in params] == with_grad and any(with_grad)
    assert all(torch.isfinite(q.grad).all() for q in params if q.grad is not None)
    MT.causal_attention(model, False)
    _, after = device_kernel_names(step, warm=True)
    F.check_device_errors()
    if names is None or before is None or after is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(names) == [], library_kernels(names)
    assert _launched(names, _BAND) == sorted(set(_BAND) - {"attn_probs_band_kernel"}), names
    assert _launched(names, _PLAIN + _CAUSAL) == [], names
    assert _launched(before, _BAND + _CAUSAL) == [] and _launched(before, _PLAIN)
    assert sorted(after) == sorted(before)


def test_captured_step_with_a_span(dev):
    """a forward + backward with a span, captured in a hipGraph and replayed on other inputs: every replay reproduces the eager step of
    its own inputs bit for bit (eval mode); keep_attention shows the zeros on both sides of the band"""
    MT, F = mta().multiTransformer, mta().functional
    from multimodal_transformer_amd import graphs
    span = 7
    model = MT.UniFullTransformer(24, embed_dim=32, h_dim=16, N=2, d_ff=32, h=2, dropout=0.0, device=dev).eval()
    model.load_state_dict(R.gen_params(R.shapes_of(model.state_dict()), 31))
    x0 = R.gen_normal("band_capture", (2, 45, 24), 31).to(dev)
    mask0 = R.prefix_mask([21, 45], 45).to(dev)
    MT.causal_attention(model, span=span)
    inputs = [(x0, mask0), (x0.flip(0).contiguous(), R.prefix_mask([45, 8], 45).to(dev)), (0.5 * x0, R.prefix_mask([33, 1], 45).to(dev))]
    x, mask = x0.clone(), mask0.clone()
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        y = model(x, mask, [45, 45])
        (y * y).sum().backward()
        return y.detach()

    refs = []
    for xi, mi in inputs:
        x.copy_(xi)
        mask.copy_(mi)
        y = step().clone()
        refs.append((y, [q.grad.detach().clone() for q in params]))
    g, y_static = graphs.capture_step(step, warmup=1)
    for i in (1, 2, 0):
        x.copy_(inputs[i][0])
        mask.copy_(inputs[i][1])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_static, refs[i][0]), "replay %d" % i
        assert all(torch.equal(q.grad, r) for q, r in zip(params, refs[i][1])), "replay %d" % i
    assert not torch.equal(refs[0][0], refs[2][0])
    MT.causal_attention(model)
    with torch.no_grad():
        assert not torch.equal(model(x, mask, [45, 45]), refs[0][0])               # the span changes the function
    MT.causal_attention(model, span=span)
    maps = MT.keep_attention(model)
    with torch.no_grad():
        model(x, mask, [45, 45])
    for m in maps.values():
        assert m.attn is not None and (m.attn.cpu().masked_select(Bn.outside_band(45, span).expand_as(m.attn)) == 0).all()
        assert (m.attn.cpu().sum(dim=-1) - 1.0).abs().max().item() <= 1e-5
    F.check_device_errors()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_before_any_launch(dev):
    MT, F = mta().multiTransformer, mta().functional
    q = torch.zeros(2, 8, 16, device=dev)
    mask = torch.ones(2, 8, 1, device=dev)
    kl = F.key_lengths(mask)
    flat = torch.zeros(int(mta()._lib.load().mmt_encoder_param_count(16, 16, 1)), device=dev)
    mha = MT.MultiHeadedAttention(2, 16).to(dev)
    mha.span = 4
    models = [MT.NLPTransformer(24, embed_dim=32, h=2, N=1, device=dev).eval(), MT.UniFullTransformer(24, embed_dim=32, h=2, N=1, device=dev).eval()]
    enc = MT.Encoder(MT.EncoderLayer(32, MT.MultiHeadedAttention(2, 32), MT.PositionwiseFeedForward(32, 64, 0.1), 0.1), 2).to(dev).eval()
    for m in models + [enc]:
        MT.causal_attention(m, span=4)
    torch.cuda.synchronize()

    def refused():
        with pytest.raises(ValueError, match="without causal=True"):
            F.sdpa(q, q, q, mask, 2, span=4)
        with pytest.raises(ValueError, match="key_lengths and span"):
            F.attn_probs(q, q, mask, 2, key_lengths=kl, causal=True, span=4)
        with pytest.raises(ValueError, match="span must be >= 1"):
            F.encoder_stack(q, mask, flat, 2, 16, 1, causal=True, span=0)
        with pytest.raises(ValueError, match="must be an int"):
            F.sdpa(q, q, q, mask, 2, causal=True, span=True)
        with pytest.raises(ValueError, match="without causal=True"):
            mha(q, q, q, mask)
        for m in models:                                 # a model with a span refuses every stream at open
            for method in ("stream", "device_stream"):
                with pytest.raises(ValueError, match=r"span = 4.*ring cache"):
                    getattr(m, method)(2, 8)
        for method in ("stream", "slot_stream"):
            with pytest.raises(ValueError, match=r"span = 4.*ring cache"):
                getattr(enc, method)(2, 8)

    _, names = device_kernel_names(refused)
    assert names is None, names
    with pytest.raises(RuntimeError, match="span"):                    # the library's own refusal, through the loader
        mta()._lib.launch("mmt_attn_probs_forward", q, q, mask, torch.empty(2, 2, 8, 8, device=dev), 2, 8, 16, 2, 0.0, 0, causal=True, span=0)
