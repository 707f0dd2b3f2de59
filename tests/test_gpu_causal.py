"""GPU: causal self-attention (csrc/attn.h *_causal_kernel, csrc/attn_probs.h, the ``causal`` keyword of functional.sdpa / attn_probs /
encoder_stack, MultiHeadedAttention.causal, multiTransformer.causal_attention): query t attends keys 0 .. t of its sequence.

The reference is tests/causal_ref.py (tests/test_causal_cpu.py holds it to the exact function in fp64); the bounds are those of
tests/test_gpu_bf16_faithful.py, imported: the arithmetic per score is the same, with fewer terms per row.  Measured worst values on the
MI355X stand beside each use.
"""
import re

import numpy as np
import pytest
import torch

import bf16_ref as E
import causal_ref as C
import recipe as R
from gpu_harness import check, dev, device_kernel_names, library_kernels, mta  # noqa: F401 (dev: fixture)
from test_gpu_bf16_faithful import (ENC_GRAD, ENC_OUT, ENC_OUT_ROW, ENC_RELU_GRAD, ENC_ROW, ENC_W_SCALE, SDPA_GRAD, SDPA_GRAD_ROW, SDPA_OUT,
                                    SDPA_OUT_ROW)

pytestmark = pytest.mark.gpu

# (T, d, h): the smallest shapes that reach every branch
CASES = [(1, 32, 2),          # one key
         (32, 32, 2),         # one full tile: the diagonal tile is the last tile and T % 32 == 0
         (33, 32, 2),         # a one-window tail tile
         (70, 40, 4),         # d_k 10 padded to 16
         (130, 64, 2),        # d_k 32; five tiles: a second tile quad with one live wave
         (40, 128, 2),        # d_k 64: two feature-block launches
         (290, 32, 2)]        # the plain backward is the one-kernel form here; three tile quads
IDS = ["T%d_d%d_h%d" % c for c in CASES]
P_TRAIN, SEED = 0.25, 20261019
MODES = [0.0, P_TRAIN]
MODE_IDS = ["eval", "train"]

_CACHE = {}
_PLAIN = ("attn_fwd_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq_kernel", "attn_probs_kernel", "attn_bwd_pair16",
          "attn_fwd_keys_kernel", "attn_bwd_dkv_keys_kernel", "attn_bwd_dq_keys_kernel", "attn_probs_keys_kernel")
_CAUSAL = ("attn_fwd_causal_kernel", "attn_bwd_dkv_causal_kernel", "attn_bwd_dq_causal_kernel", "attn_probs_causal_kernel")


def _launched(names, which):
    """those of `which` that were launched (whole identifiers: encoder_post_attn_fwd_kernel is no attn_fwd_kernel)"""
    return sorted(set(w for w in which for n in names if re.search(r"\b%s" % w, n)))


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def _lengths(T):
    return [T, max(1, (2 * T) // 3), 1]


def _sdpa_call(F, q, k, v, g, mask, h, p, causal=True):
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    y = F.sdpa(*leaves, mask, h, dropout_p=p, seed=SEED if p else 0, causal=causal)
    y.backward(g)
    return dict(zip(("y", "dq", "dk", "dv"), [y.detach().cpu()] + [t.grad.cpu() for t in leaves]))


def _run(case, p, dev):
    """every GPU result of one (case, mode), computed once: the causal call, twice, the plain call, and the two maps"""
    key = (case, p)
    if key in _CACHE:
        return _CACHE[key]
    T, d, h = case
    lengths = _lengths(T)
    B = len(lengths)
    F = mta().functional
    tag = "causal%d_%d_%d" % case
    q, k, v, g = (R.gen_normal(tag + n, (B, T, d), 13) for n in "qkvg")
    q = 2 * q
    mask = R.prefix_mask(lengths, T)
    qg, kg, vg, gg, mg = (t.to(dev) for t in (q, k, v, g, mask))
    seed = SEED if p else 0
    scale = F.dropout_mask(p, seed, 0, 1024, dev, attn_Tp=32)[1] if p else 1.0        # of a kept probability: 1/(1-p) at the generator's resolution
    out = {"scale": scale, "q": q, "k": k, "v": v, "g": g, "mask": mask, "lengths": lengths, "gpu": (qg, kg, vg, gg, mg),
           "causal": _sdpa_call(F, qg, kg, vg, gg, mg, h, p),
           "again": _sdpa_call(F, qg, kg, vg, gg, mg, h, p),
           "plain": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, causal=False),
           "map": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed, causal=True).cpu(),
           "map_plain": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed).cpu()}
    torch.cuda.synchronize()
    F.check_device_errors()
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sdpa_against_the_causal_reference(dev, case, p):
    """ctx, dq, dk, dv against causal_ref.sdpa.  Train mode: the drop multipliers are those of the causal map for the same seed (0 where
    it is 0 on or below the diagonal, 1/(1-p) elsewhere; entries above the diagonal are never read).
    Measured worst (rel-L2 / per-row maximum) over the cases: y 7.9e-5 / 2.3e-3 (T 290, eval) against SDPA_OUT 4e-4 / SDPA_OUT_ROW 1e-2,
    gradients 3.3e-4 / 8.1e-3 (dk, T 290, eval) against SDPA_GRAD 2e-3 / SDPA_GRAD_ROW 2e-2."""
    T, d, h = case
    c = _run(case, p, dev)
    B = len(c["lengths"])
    drop = None
    if p:
        drop = ((c["map"] != 0) | C.above_diagonal(T)).double() * c["scale"]
    lt = [t.double().requires_grad_() for t in (c["q"], c["k"], c["v"])]
    ctx, _ = C.sdpa(*(_split(t, h) for t in lt), c["mask"].double().unsqueeze(1), drop)
    y = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    y.backward(c["g"].double())
    got = c["causal"]
    tag = "causal sdpa T%d d%d p%g" % (T, d, p)
    check(tag + " y", got["y"], y.detach(), SDPA_OUT, SDPA_OUT_ROW)
    for name, t in zip(("dq", "dk", "dv"), lt):
        # at T = 1 dq and dk are analytically zero (one key: the softmax is constant): measured on dv's scale
        zero = name != "dv" and float(t.grad.norm()) < 1e-9 * float(lt[2].grad.norm())
        check(tag + " " + name, got[name], t.grad, SDPA_GRAD, SDPA_GRAD_ROW, scale_ref=lt[2].grad if zero else None)


# ------------------------------------------------------------------------------------------------ 2. exact facts
@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_facts(dev, case, p):
    T, d, h = case
    c = _run(case, p, dev)
    P, got = c["map"], c["causal"]
    B = len(c["lengths"])
    assert P.shape == (B, h, T, T) and torch.isfinite(P).all() and (P >= 0).all()
    assert (P.masked_select(C.above_diagonal(T).expand_as(P)) == 0).all()          # exact zeros, written by the kernel
    for name in got:                                                               # two runs are bit-identical
        assert torch.isfinite(got[name]).all() and torch.equal(got[name], c["again"][name]), name
    for b, n in enumerate(c["lengths"]):
        assert (got["dq"][b, n:] == 0).all(), b                                    # blanked query rows pass no gradient to q
    if p:
        # the keep decisions are the plain map's, per position
        low = ~C.above_diagonal(T).expand_as(P)
        assert torch.equal((P == 0) & low, (c["map_plain"] == 0) & low)
        return
    err = (P.double().sum(dim=-1) - 1.0).abs().max().item()
    print("causal map T%d row-sum error %.3e" % (T, err))
    assert err <= 1e-5
    for b, n in enumerate(c["lengths"]):
        for t in range(n, T):                                                      # a blanked query row: uniform over its t + 1 visible keys
            uniform = torch.full((t + 1,), 1 / (t + 1), dtype=torch.float32)
            for head in range(h):
                assert torch.equal(P[b, head, t, :t + 1], uniform), (b, head, t)
    assert torch.equal(got["y"][:, 0], c["v"][:, 0].bfloat16().float())            # row 0 attends one key: ctx = bf16(v), bit for bit


# ------------------------------------------------------------------------------------------------ 3. no look-ahead
def _perturbed(c, t0, dev):
    out = []
    for i, t in enumerate(c["gpu"][:3]):
        t = t.clone()
        t[:, t0:] = 1.5 * t[:, t0:] + 0.25 * (i + 1)
        out.append(t)
    return out


@pytest.mark.parametrize("case,t0", [(CASES[2], 32), (CASES[3], 32), (CASES[3], 64), (CASES[4], 96), (CASES[4], 45), (CASES[5], 32),
                                     (CASES[6], 128), (CASES[6], 45)], ids=lambda v: str(v))
def test_no_look_ahead_in_sdpa(dev, case, t0):
    """q, k, v changed at windows >= t0: ctx of the rows in tiles wholly before t0 is bit-equal (t0 = 45: rows < 32; the tile that
    straddles t0 shares one rescale decision with changed rows and is covered by the reference test only).  The plain call differs."""
    T, d, h = case
    F = mta().functional
    c = _run(case, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]
    q2, k2, v2 = _perturbed(c, t0, dev)
    safe = (t0 // 32) * 32
    with torch.no_grad():
        a = F.sdpa(qg, kg, vg, mg, h, causal=True).cpu()
        b = F.sdpa(q2, k2, v2, mg, h, causal=True).cpu()
        pa = F.sdpa(qg, kg, vg, mg, h).cpu()
        pb = F.sdpa(q2, k2, v2, mg, h).cpu()
    assert torch.equal(a, c["causal"]["y"])
    assert torch.equal(a[:, :safe], b[:, :safe])
    assert not torch.equal(a[:, safe:], b[:, safe:])
    assert not torch.equal(pa[:, :safe], pb[:, :safe])                              # the plain call looks ahead
    F.check_device_errors()


@pytest.mark.parametrize("d,h,T,t0", [(128, 8, 70, 64), (128, 8, 70, 45), (40, 4, 70, 32), (40, 4, 70, 45)])
def test_no_look_ahead_through_the_encoder_stack(dev, d, h, T, t0):
    """two layers, eval mode, x changed at windows >= t0: every other kernel of a layer is row-local, so y is bit-equal on the rows in
    tiles wholly before t0 (d = 128: the fixed-shape chains; d = 40: the generic ones).  The plain stack differs."""
    F = mta().functional
    B, n = 2, 2
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev)
    x = R.gen_normal("causal_ahead_d%d:x" % d, (B, T, d), 17).to(dev)
    mask = R.prefix_mask([T, 50], T).to(dev)
    x2 = x.clone()
    x2[:, t0:] = 1.5 * x2[:, t0:] + 0.25
    safe = (t0 // 32) * 32
    with torch.no_grad():
        a, b = (F.encoder_stack(t, mask, flat, h, R.D_FF, n, causal=True).cpu() for t in (x, x2))
        pa, pb = (F.encoder_stack(t, mask, flat, h, R.D_FF, n).cpu() for t in (x, x2))
    assert torch.isfinite(a).all() and torch.equal(a[:, :safe], b[:, :safe])
    assert not torch.equal(a[:, safe:], b[:, safe:])
    assert not torch.equal(pa[:, :safe], pb[:, :safe])
    F.check_device_errors()


# ------------------------------------------------------------------------------------------------ 4. kernel names
@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=[IDS[2], IDS[6]])
def test_kernel_names(dev, case):
    T, d, h = case
    F = mta().functional
    c = _run(case, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]

    def call(causal):
        out = _sdpa_call(F, qg, kg, vg, gg, mg, h, 0.0, causal=causal)
        F.attn_probs(qg, kg, mg, h, causal=causal)
        return out

    _, causal = device_kernel_names(lambda: call(True))
    _, plain = device_kernel_names(lambda: call(False))
    if causal is None or plain is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert _launched(causal, _CAUSAL) == sorted(_CAUSAL), causal
    assert _launched(causal, _PLAIN) == [], causal                   # no plain or keyed kernel, no one-kernel backward: also at T = 290
    assert _launched(plain, _CAUSAL) == [], plain
    assert _launched(plain, _PLAIN) == sorted(("attn_fwd_kernel", "attn_probs_kernel") + (("attn_bwd_pair16",) if T == 290 else
                                                                                           ("attn_bwd_dkv_kernel", "attn_bwd_dq_kernel"))), plain


# ------------------------------------------------------------------------------------------------ 5. encoder stack
ENC = [(128, 8, 2, 3, 70, [70, 33, 1]),        # the fixed-shape chains
       (40, 4, 2, 2, 45, [45, 20])]            # the generic chains
ENC_IDS = ["d%d_n%d_T%d" % (c[0], c[2], c[4]) for c in ENC]
_ENC_REF = {}


def _enc_inputs(c):
    d, h, n, B, T, lengths = c
    cid = "causal_enc_d%d_T%d" % (d, T)
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    return p32, R.gen_normal(cid + ":x", (B, T, d), 17), R.prefix_mask(lengths, T), R.gen_normal(cid + ":g", (B, T, d), 17)


def _enc_drops(F, c, p, seed, dev):
    """the multipliers of the stack's four dropout streams per layer, as the kernels draw them for `seed`"""
    d, h, n, B, T, lengths = c
    Tp, DP, FP, M = -(-T // 32) * 32, -(-d // 64) * 64, -(-R.D_FF // 64) * 64, B * T
    drops = []
    for l in range(n):
        ka, sa = F.dropout_mask(p, seed, 4 * l + 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
        k0, s0 = F.dropout_mask(p, seed, 4 * l + 1, M * DP, dev)
        kf, sf = F.dropout_mask(p, seed, 4 * l + 2, M * FP, dev)
        k1, s1 = F.dropout_mask(p, seed, 4 * l + 3, M * DP, dev)
        drops.append({"attn": ka.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu().double() * sa, "sub0": k0.reshape(B, T, DP)[:, :, :d].cpu().double() * s0,
                      "ffn": kf.reshape(B, T, FP)[:, :, :R.D_FF].cpu().double() * sf, "sub1": k1.reshape(B, T, DP)[:, :, :d].cpu().double() * s1})
    return drops


def _enc_ref(F, c, p, seed, dev):
    key = (c[0], c[4], p, seed)
    if key not in _ENC_REF:
        d, h, n, B, T, lengths = c
        p32, x, mask, g = _enc_inputs(c)
        pd = {k: v.double().clone().requires_grad_() for k, v in p32.items()}
        xd = x.double().requires_grad_()
        y = C.encoder_stack(pd, "", xd, mask.double(), h, _enc_drops(F, c, p, seed, dev) if p else None)
        y.backward(g.double())
        _ENC_REF[key] = (y.detach().numpy(), xd.grad.numpy(), {k: v.grad.numpy() for k, v in pd.items()})
    return _ENC_REF[key]


@pytest.mark.parametrize("mode", ["eval", "train", "train_devseed"])
@pytest.mark.parametrize("c", ENC, ids=ENC_IDS)
def test_encoder_stack_against_the_causal_reference(dev, c, mode):
    """y, dx and every parameter gradient against causal_ref.encoder_stack under the bounds and per-tensor rules of
    test_gpu_bf16_faithful.test_encoder_stack; train mode at p = 0.25 with the seed by value and with a device-resident seed (the
    _causal_devseed twins), whose first forward uses the value it was made with.  Measured worst (rel-L2 / per-row maximum): y 2.5e-4 /
    1.1e-3 (d 40, eval) against ENC_OUT 2e-3 / ENC_OUT_ROW 8e-3; dx 3.0e-3 / 7.7e-3 (train) and the parameter gradients 6.2e-3 / 1.7e-2
    (layer 0's first LayerNorm bias at d 40, its query bias at d 128; train) against ENC_GRAD 1e-2 / ENC_ROW 5e-2; the first FFN
    projection's and the FFN LayerNorm's 3.8e-3 against ENC_RELU_GRAD 4e-2.  The two seed forms give the same figures."""
    d, h, n, B, T, lengths = c
    F = mta().functional
    p = 0.0 if mode == "eval" else P_TRAIN
    value = 4242 + d + T
    seed = mta()._lib.DeviceSeed(dev, value) if mode == "train_devseed" else value
    if mode == "train_devseed":
        assert seed.peek() == value
    p32, x, mask, g = _enc_inputs(c)
    flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
    xg = x.to(dev).requires_grad_()
    y = F.encoder_stack(xg, mask.to(dev), flat, h, R.D_FF, n, dropout_p=p, seed=seed if p else 0, causal=True)
    y.backward(g.to(dev))
    F.check_device_errors()
    y_ref, dx_ref, grads = _enc_ref(F, c, p, value if p else 0, dev)
    tag = "causal enc d%d n%d T%d %s" % (d, n, T, mode)
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


# ------------------------------------------------------------------------------------------------ 6. training
def _train_model(which, dev):
    MT = mta().multiTransformer
    B, T, lengths = 4, 40, [40, 33, 20, 5]
    if which == "mft":
        mods, dims = ["acoustic", "linguistic"], {"acoustic": 88, "linguistic": 300}
        model = MT.MultiTransformer(mods, dims, N=2, device=dev).train()
        x = {m: R.gen_normal("causal_train:" + m, (B, T, dims[m]), 3).to(dev) for m in mods}
    else:
        model = MT.NLPTransformer(512, embed_dim=128, h=8, N=2, device=dev).train()
        x = torch.tanh(R.gen_normal("causal_train:x", (B, T, 512), 3)).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("causal_train:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    return model, x, mask, tgt, lengths


@pytest.mark.parametrize("which", ["sft", "mft"])
def test_train_step_with_causal_attention(dev, which):
    """one train step with the flag on: finite gradients for every parameter that gets one without it, hand-written kernels only, the
    causal attention kernels and no other; causal_attention(model, False) restores the launch sequence of a run made before"""
    MT, F = mta().multiTransformer, mta().functional
    model, x, mask, tgt, lengths = _train_model(which, dev)
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        torch.manual_seed(77)
        F.mse_sum_loss_backward(model(x, mask, lengths), tgt, sum(lengths))

    _, before = device_kernel_names(step, warm=True)                 # the flag was never set
    with_grad = [q.grad is not None for q in params]
    found = MT.causal_attention(model)
    assert found and all(m.causal for m in found.values())
    _, names = device_kernel_names(step, warm=True)
    assert [q.grad is not None for q in params] == with_grad and any(with_grad)
    assert all(torch.isfinite(q.grad).all() for q in params if q.grad is not None)
    MT.causal_attention(model, False)
    _, after = device_kernel_names(step, warm=True)
    F.check_device_errors()
    if names is None or before is None or after is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(names) == [], library_kernels(names)
    assert _launched(names, _CAUSAL) == sorted(set(_CAUSAL) - {"attn_probs_causal_kernel"}), names
    assert _launched(names, _PLAIN) == [], names
    assert _launched(before, _CAUSAL) == [] and _launched(before, _PLAIN)
    assert sorted(after) == sorted(before)               # (sorted: the modalities of the MFT run on streams of their own)


def test_captured_step_with_causal_attention(dev):
    """a forward + backward with the flag on, captured in a hipGraph and replayed on other inputs: every replay reproduces the eager step
    of its own inputs bit for bit (eval mode), as the existing capture tests ask of the plain path; keep_attention shows the zeros"""
    MT, F = mta().multiTransformer, mta().functional
    from multimodal_transformer_amd import graphs
    model = MT.UniFullTransformer(24, embed_dim=32, h_dim=16, N=2, d_ff=32, h=2, dropout=0.0, device=dev).eval()
    model.load_state_dict(R.gen_params(R.shapes_of(model.state_dict()), 31))
    x0 = R.gen_normal("causal_capture", (2, 45, 24), 31).to(dev)
    mask0 = R.prefix_mask([21, 45], 45).to(dev)
    MT.causal_attention(model)
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
    maps = MT.keep_attention(model)
    with torch.no_grad():
        model(x, mask, [45, 45])
    for m in maps.values():
        assert m.attn is not None and (m.attn.cpu().masked_select(C.above_diagonal(45).expand_as(m.attn)) == 0).all()
    F.check_device_errors()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_come_before_any_launch(dev):
    MT, F = mta().multiTransformer, mta().functional
    q = torch.zeros(2, 8, 16, device=dev)
    mask = torch.ones(2, 8, 1, device=dev)
    kl = F.key_lengths(mask)
    flat = torch.zeros(int(mta()._lib.load().mmt_encoder_param_count(16, 16, 1)), device=dev)
    mha = MT.MultiHeadedAttention(2, 16).to(dev)
    mha.mask_keys = mha.causal = True
    torch.cuda.synchronize()

    def refused():
        with pytest.raises(ValueError, match="key_lengths.*causal"):
            F.sdpa(q, q, q, mask, 2, key_lengths=kl, causal=True)
        with pytest.raises(ValueError, match="key_lengths.*causal"):
            F.attn_probs(q, q, mask, 2, key_lengths=kl, causal=True)
        with pytest.raises(ValueError, match="key_lengths.*causal"):
            F.encoder_stack(q, mask, flat, 2, 16, 1, key_lengths=kl, causal=True)
        with pytest.raises(ValueError, match="mask_keys.*causal"):
            mha(q, q, q, mask)

    _, names = device_kernel_names(refused)
    assert names is None, names
    dense = torch.ones(2, 1, 8, 8, device=dev)                      # the existing refusal keeps its words
    with pytest.raises(NotImplementedError, match="query-row mask"):
        F.attn_probs(q, q, dense, 2, causal=True)
