"""GPU: the key-length mask (csrc/attn.h *_keys_kernel, csrc/attn_probs.h, functional.key_lengths / sdpa / attn_probs / encoder_stack
with key_lengths, MultiHeadedAttention.mask_keys, multiTransformer.mask_padded_keys): sequence b attends keys < len[b] only.

Reference by truncation: keyed attention of sequence b IS plain attention of that sequence cut to its first len[b] windows and run alone
(tests/test_key_mask_cpu.py checks the equality in fp64), down to the tile order and the per-wave rescale decision; the same holds for
the whole encoder stack on rows < len[b].  So the reference is tests/bf16_ref.py as it stands, applied per truncated sequence with the
upstream gradient zeroed on rows >= len[b] and the parameter gradients summed over the sequences, and the bounds are those of
tests/test_gpu_bf16_faithful.py, imported: the arithmetic is the same.  Measured worst values on the MI355X stand beside each use.
"""
import re

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import check, dev, device_kernel_names, library_kernels, mta  # noqa: F401 (dev: fixture)
from test_gpu_bf16_faithful import (ENC_CLEAN, ENC_GRAD, ENC_OUT, ENC_OUT_ROW, ENC_RELU_GRAD, ENC_ROW, ENC_W_SCALE, SDPA_GRAD, SDPA_GRAD_ROW,
                                    SDPA_OUT, SDPA_OUT_ROW)

pytestmark = pytest.mark.gpu

# (T, d, h, lengths): the smallest shapes that reach every branch
CASES = [(33, 32, 2, [33, 32, 1, 17]),        # two tiles, a one-key tail, a length on the tile edge, length 1
         (70, 40, 4, [70, 64, 33, 5]),        # d_k 10 padded to 16; whole tiles skipped
         (130, 64, 2, [130, 97, 128, 1]),     # d_k 32; five tiles: a second tile quad with one live wave
         (40, 128, 2, [40, 9]),               # d_k 64: two feature-block launches
         (290, 32, 2, [290, 257, 100])]       # a shape whose plain backward is the one-kernel form
IDS = ["T%d_d%d_h%d" % c[:3] for c in CASES]
P_TRAIN, SEED = 0.25, 20251019
MODES = [0.0, P_TRAIN]
MODE_IDS = ["eval", "train"]

_CACHE = {}
_PLAIN = ("attn_fwd_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq_kernel", "attn_probs_kernel", "attn_bwd_pair16")
_KEYED = ("attn_fwd_keys_kernel", "attn_bwd_dkv_keys_kernel", "attn_bwd_dq_keys_kernel", "attn_probs_keys_kernel", "key_lengths_kernel")


def _launched(names, which):
    """those of `which` that were launched (whole identifiers: encoder_post_attn_fwd_kernel is no attn_fwd_kernel)"""
    return sorted(set(w for w in which for n in names if re.search(r"\b%s" % w, n)))


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def _sdpa_call(F, q, k, v, g, mask, h, p, kl):
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    y = F.sdpa(*leaves, mask, h, dropout_p=p, seed=SEED if p else 0, key_lengths=kl)
    y.backward(g)
    return dict(zip(("y", "dq", "dk", "dv"), [y.detach().cpu()] + [t.grad.cpu() for t in leaves]))


def _run(case, p, dev):
    """every GPU result of one (case, mode), computed once: the keyed call at the case's lengths, the keyed call at full lengths, the
    plain call, and the three maps"""
    key = (tuple(case[:3]), p)
    if key in _CACHE:
        return _CACHE[key]
    T, d, h, lengths = case
    B = len(lengths)
    F = mta().functional
    tag = "kmask%d_%d_%d" % (T, d, h)
    q, k, v, g = (R.gen_normal(tag + n, (B, T, d), 13) for n in "qkvg")
    q = 2 * q
    mask = R.prefix_mask(lengths, T)
    g = g * mask                                                    # no upstream gradient on rows >= len
    qg, kg, vg, gg, mg = (t.to(dev) for t in (q, k, v, g, mask))
    kl = F.key_lengths(mg)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    seed = SEED if p else 0
    scale = F.dropout_mask(p, seed, 0, 1024, dev, attn_Tp=32)[1] if p else 1.0        # of a kept probability: 1/(1-p) at the generator's resolution
    out = {"scale": scale, "q": q, "k": k, "v": v, "g": g, "mask": mask, "gpu": (qg, kg, vg, gg, mg), "kl": kl,
           "keyed": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, kl),
           "keyed_full": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, full),
           "plain": _sdpa_call(F, qg, kg, vg, gg, mg, h, p, None),
           "map": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed, key_lengths=kl).cpu(),
           "map_full": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed, key_lengths=full).cpu(),
           "map_plain": F.attn_probs(qg, kg, mg, h, dropout_p=p, seed=seed).cpu()}
    torch.cuda.synchronize()
    F.check_device_errors()
    _CACHE[key] = out
    return out


def test_key_lengths_of_a_mask(dev):
    F = mta().functional
    m = R.prefix_mask([33, 32, 1, 17, 0], 33)                       # an all-zero row counts as length 1
    m[3, 4] = 0.0                                                   # a hole inside the prefix stays attended: the LAST non-zero entry counts
    got = F.key_lengths(m.to(dev))
    assert got.dtype == torch.int32 and got.shape == (5,) and got.tolist() == [33, 32, 1, 17, 1]
    long = torch.zeros(3, 1000, 1)                                  # more windows than threads in the workgroup
    long[0, 999] = 1.0
    long[1, :257] = 1.0
    assert F.key_lengths(long.to(dev)).tolist() == [1000, 257, 1]
    assert F.key_lengths(m.reshape(5, 33).to(dev)).tolist() == [33, 32, 1, 17, 1]
    assert F.key_lengths(m.reshape(5, 1, 33, 1).to(dev)).tolist() == [33, 32, 1, 17, 1]


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sdpa_against_the_truncated_reference(dev, case, p):
    """ctx, dq, dk, dv on rows < len against bf16_ref.sdpa of each sequence cut to its length.  Train mode: the drop multipliers are
    those of the keyed map for the same seed (0 where it is 0, 1/(1-p) elsewhere).
    Measured worst (rel-L2 / per-row maximum) over the cases: y 9.0e-5 / 8.1e-4 (T 40, d_k 64, train), gradients 1.7e-4 (dq, T 70) /
    3.2e-3 (dk, T 290, train): each under a quarter of its bound."""
    T, d, h, lengths = case
    c = _run(case, p, dev)
    assert c["kl"].tolist() == lengths
    got = c["keyed"]
    ref = {n: torch.zeros(len(lengths), T, d, dtype=torch.float64) for n in ("y", "dq", "dk", "dv")}
    for b, n in enumerate(lengths):
        lt = [t[b:b + 1, :n].double().requires_grad_() for t in (c["q"], c["k"], c["v"])]
        drop = None
        if p:
            drop = (c["map"][b:b + 1, :, :n, :n] != 0).double() * c["scale"]
        ctx, _ = E.sdpa(*(_split(t, h) for t in lt), None, drop, fused_attn_bwd=False)
        y = ctx.permute(0, 2, 1, 3).reshape(1, n, d)
        y.backward(c["g"][b:b + 1, :n].double())
        ref["y"][b, :n] = y.detach()[0]
        for name, t in zip(("dq", "dk", "dv"), lt):
            ref[name][b, :n] = t.grad[0]
        for name in ("dq", "dk", "dv"):                             # blanked query rows pass no gradient to q; masked keys get none
            assert (got[name][b, n:] == 0).all(), (name, b)
    tag = "kmask sdpa T%d d%d p%g" % (T, d, p)
    rows = c["mask"].double()
    check(tag + " y", got["y"].double() * rows, ref["y"], SDPA_OUT, SDPA_OUT_ROW)
    for name in ("dq", "dk", "dv"):
        check(tag + " " + name, got[name], ref[name], SDPA_GRAD, SDPA_GRAD_ROW)


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_zeros_and_the_keyed_map(dev, case, p):
    T, d, h, lengths = case
    c = _run(case, p, dev)
    P = c["map"]
    assert P.shape == (len(lengths), h, T, T) and torch.isfinite(P).all() and (P >= 0).all()
    for b, n in enumerate(lengths):
        assert (c["keyed"]["dk"][b, n:] == 0).all() and (c["keyed"]["dv"][b, n:] == 0).all()
        assert (P[b, :, :, n:] == 0).all(), b                       # columns >= len: exact zeros, written by the kernel
        if p:
            continue
        err = (P[b].double().sum(dim=-1) - 1.0).abs().max().item()
        print("kmask map T%d len %d row-sum error %.3e" % (T, n, err))
        assert err <= 1e-5
        uniform = torch.full((n,), 1 / n, dtype=torch.float32)
        for t in range(n, T):                                       # a blanked query row: uniform over the visible keys
            for head in range(h):
                assert torch.equal(P[b, head, t, :n], uniform), (b, head, t)


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_full_lengths_give_the_plain_call_bit_for_bit(dev, case, p):
    """every length equal to T: the keyed kernels run the plain kernels' instruction sequence per element.  T = 290 is left out of the
    gradient comparison: there the plain call runs the one-kernel backward, the keyed call never does."""
    T = case[0]
    c = _run(case, p, dev)
    assert torch.equal(c["keyed_full"]["y"], c["plain"]["y"])
    assert torch.equal(c["map_full"], c["map_plain"])
    if T != 290:
        for name in ("dq", "dk", "dv"):
            assert torch.equal(c["keyed_full"][name], c["plain"][name]), name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_keep_decisions(dev, case):
    """train mode: on the visible columns the keyed map drops exactly the positions the plain map drops for the same seed"""
    T, d, h, lengths = case
    c = _run(case, P_TRAIN, dev)
    dropped = 0
    for b, n in enumerate(lengths):
        assert torch.equal(c["map"][b, :, :, :n] == 0, c["map_plain"][b, :, :, :n] == 0), b
        dropped += int((c["map"][b, :, :, :n] == 0).sum())
    total = sum(h * T * n for n in lengths)
    assert abs(dropped / total - P_TRAIN) < 0.05                    # and they are dropout decisions, not a constant


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_kernel_names(dev, case):
    T, d, h, lengths = case
    F = mta().functional
    c = _run(case, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]

    def call(kl):
        out = _sdpa_call(F, qg, kg, vg, gg, mg, h, 0.0, kl)
        F.attn_probs(qg, kg, mg, h, key_lengths=kl)
        return out

    _, keyed = device_kernel_names(lambda: call(F.key_lengths(mg)))
    _, plain = device_kernel_names(lambda: call(None))
    if keyed is None or plain is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert _launched(keyed, _KEYED) == sorted(_KEYED), keyed
    assert _launched(keyed, _PLAIN) == [], keyed                     # no plain kernel, and no one-kernel backward: also at T = 290
    assert _launched(plain, _KEYED) == [], plain
    assert _launched(plain, _PLAIN) == sorted(("attn_fwd_kernel", "attn_probs_kernel") + (("attn_bwd_pair16",) if T == 290 else
                                                                                           ("attn_bwd_dkv_kernel", "attn_bwd_dq_kernel"))), plain


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lengths_are_clamped(dev, case):
    """lengths of 0 and T + 5 give the results of 1 and T"""
    T, d, h, lengths = case
    F = mta().functional
    c = _run(case, 0.0, dev)
    qg, kg, vg, gg, mg = c["gpu"]
    B = len(lengths)
    wild = torch.tensor([0, T + 5] + lengths[2:], dtype=torch.int32, device=dev)
    tame = torch.tensor([1, T] + lengths[2:], dtype=torch.int32, device=dev)
    a, b = _sdpa_call(F, qg, kg, vg, gg, mg, h, 0.0, wild), _sdpa_call(F, qg, kg, vg, gg, mg, h, 0.0, tame)
    for name in a:
        assert torch.isfinite(a[name]).all() and torch.equal(a[name], b[name]), name
    assert torch.equal(F.attn_probs(qg, kg, mg, h, key_lengths=wild), F.attn_probs(qg, kg, mg, h, key_lengths=tame))
    wild[0] = -7
    assert torch.equal(F.attn_probs(qg, kg, mg, h, key_lengths=wild), F.attn_probs(qg, kg, mg, h, key_lengths=tame))
    assert B >= 2


def test_key_lengths_argument_refusals(dev):
    F = mta().functional
    q = torch.zeros(2, 8, 16, device=dev)
    mask = torch.ones(2, 8, 1, device=dev)
    flat = torch.zeros(int(mta()._lib.load().mmt_encoder_param_count(16, 16, 1)), device=dev)
    for bad, what in ((torch.ones(2, device=dev), "int32"), (torch.ones(2, dtype=torch.int64, device=dev), "int32"),
                      (torch.ones(3, dtype=torch.int32, device=dev), "shape"), (torch.ones(2, 1, dtype=torch.int32, device=dev), "shape"),
                      (torch.ones(2, dtype=torch.int32), "is on")):
        with pytest.raises(ValueError, match=what):
            F.sdpa(q, q, q, mask, 2, key_lengths=bad)
        with pytest.raises(ValueError, match=what):
            F.attn_probs(q, q, mask, 2, key_lengths=bad)
        with pytest.raises(ValueError, match=what):
            F.encoder_stack(q, mask, flat, 2, 16, 1, key_lengths=bad)
    dense = torch.ones(2, 1, 8, 8, device=dev)                      # the existing refusal keeps its words
    with pytest.raises(NotImplementedError, match="query-row mask"):
        F.attn_probs(q, q, dense, 2, key_lengths=torch.ones(2, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ encoder stack
ENC = [(128, 8, 2, 3, 70, [70, 33, 1]),        # the fixed-shape chains
       (40, 4, 2, 2, 33, [33, 9]),             # the generic chains
       (256, 8, 1, 2, 45, [45, 20])]
ENC_IDS = ["d%d_n%d_T%d" % (c[0], c[2], c[4]) for c in ENC]


def _enc_inputs(c, dev):
    d, h, n, B, T, lengths = c
    cid = "kmask_enc_d%d_T%d" % (d, T)
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    x = R.gen_normal(cid + ":x", (B, T, d), 17)
    mask = R.prefix_mask(lengths, T)
    g = R.gen_normal(cid + ":g", (B, T, d), 17) * mask
    return p32, x, mask, g


def _enc_call(F, p32, x, mask, g, c, dev, p=0.0, seed=0, kl=None):
    d, h, n, B, T, lengths = c
    flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
    xg = x.to(dev).requires_grad_()
    y = F.encoder_stack(xg, mask.to(dev), flat, h, R.D_FF, n, dropout_p=p, seed=seed, key_lengths=kl)
    y.backward(g.to(dev))
    return y.detach().cpu(), xg.grad.cpu(), flat.grad.cpu()


@pytest.mark.parametrize("c", ENC, ids=ENC_IDS)
def test_encoder_stack_against_the_truncated_reference(dev, c):
    """eval mode, forward and every gradient on rows < len, dy zero elsewhere; the bounds and the per-tensor rules of
    test_gpu_bf16_faithful.test_encoder_stack.  Measured worst, all at d = 128: y 1.9e-4 / 9.4e-4, dx 1.8e-3 / 4.9e-3, parameter gradients
    4.1e-3 / 1.3e-2 (layer 0's query bias), the first FFN projection's and the FFN LayerNorm's (which a tipped ReLU reaches) 2.6e-3; d = 256
    and d = 40 stay under 1.1e-4 / 6.9e-4.  The d = 128 parameter gradients lie above a quarter of ENC_GRAD, as the plain stack's do in
    test_gpu_bf16_faithful (6.4e-3 against the same 1e-2): the imported bound is kept, not replaced by a wider one of 4 x 4.1e-3."""
    d, h, n, B, T, lengths = c
    F = mta().functional
    p32, x, mask, g = _enc_inputs(c, dev)
    kl = F.key_lengths(mask.to(dev))
    assert kl.tolist() == lengths
    y, dx, dflat = _enc_call(F, p32, x, mask, g, c, dev, kl=kl)
    F.check_device_errors()
    pd = {k: v.double().clone().requires_grad_() for k, v in p32.items()}
    y_ref, dx_ref = torch.zeros(B, T, d, dtype=torch.float64), torch.zeros(B, T, d, dtype=torch.float64)
    for b, L in enumerate(lengths):
        xb = x[b:b + 1, :L].double().requires_grad_()
        yb = E.encoder_stack(pd, "", xb, torch.ones(1, L, 1, dtype=torch.float64), h, None)
        yb.backward(g[b:b + 1, :L].double())                        # parameter gradients accumulate over the sequences
        y_ref[b, :L], dx_ref[b, :L] = yb.detach()[0], xb.grad[0]
        assert (dx[b, L:] == 0).all(), b                            # a padded window is no key, no value, and gets no upstream gradient
    grads = {k: v.grad.numpy() for k, v in pd.items()}
    tag = "kmask enc d%d n%d T%d" % (d, n, T)
    failures = []
    clean = ENC_CLEAN.get("bfe_d%d_n%d_T%d_p0" % (d, n, T))
    g_rel, g_row = clean or (ENC_GRAD, ENC_ROW)
    check(tag + " y", y.double() * mask.double(), y_ref, ENC_OUT, ENC_OUT_ROW, failures=failures)
    check(tag + " dx", dx, dx_ref, g_rel, g_row, failures=failures)
    flat, off = dflat.numpy(), 0
    for name, shape in E.encoder_param_shapes(d, R.D_FF, n).items():
        size = int(np.prod(shape))
        got = flat[off: off + size].reshape(shape)
        off += size
        scale = grads[name.replace("linears.1.bias", "linears.0.bias")] if "linears.1.bias" in name else None     # analytically zero
        flips = ".w_1." in name or "sublayer.1.norm" in name
        if clean:
            check(tag + " " + name, got, grads[name], g_rel, g_row, scale_ref=scale, failures=failures)
        else:
            check(tag + " " + name, got, grads[name], ENC_RELU_GRAD if flips else ENC_GRAD, None if flips else ENC_ROW, scale_ref=scale,
                  failures=failures)
        if len(shape) == 2:
            r = grads[name].astype(np.float64).ravel()
            s = float(np.dot(got.astype(np.float64).ravel() - r, r) / np.dot(r, r))
            if abs(s) > ENC_W_SCALE:
                failures.append("%s %s: scale %.3e > %.1e" % (tag, name, s, ENC_W_SCALE))
    assert off == flat.size
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", ENC, ids=ENC_IDS)
def test_encoder_stack_full_lengths_give_the_plain_stack(dev, c):
    """train mode (p = 0.1), one seed: the keyed stack with every length equal to T is the plain stack, bit for bit (no shape here has
    the one-kernel backward), with the seed by value and with a device-resident seed (the _devseed twins)"""
    d, h, n, B, T, lengths = c
    F = mta().functional
    p32, x, mask, g = _enc_inputs(c, dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    seed = 4242 + d
    plain = _enc_call(F, p32, x, mask, g, c, dev, p=0.1, seed=seed)
    keyed = _enc_call(F, p32, x, mask, g, c, dev, p=0.1, seed=seed, kl=full)
    for name, a, b in zip(("y", "dx", "dflat"), keyed, plain):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    DeviceSeed = mta()._lib.DeviceSeed
    plain_ds = _enc_call(F, p32, x, mask, g, c, dev, p=0.1, seed=DeviceSeed(dev, seed))
    keyed_ds = _enc_call(F, p32, x, mask, g, c, dev, p=0.1, seed=DeviceSeed(dev, seed), kl=full)
    for name, a, b in zip(("y", "dx", "dflat"), keyed_ds, plain_ds):
        assert torch.isfinite(a).all() and torch.equal(a, b), name + " (device-resident seed)"
    short = _enc_call(F, p32, x, mask, g, c, dev, p=0.1, seed=seed, kl=F.key_lengths(mask.to(dev)))
    assert not torch.equal(short[0], plain[0])                      # and the lengths do change the result
    F.check_device_errors()


# ------------------------------------------------------------------------------------------------ models
def _b2(dev):
    MT = mta().multiTransformer
    model = MT.UniFullTransformer(24, embed_dim=32, h_dim=16, N=2, d_ff=32, h=2, dropout=0.0, device=dev).eval()
    model.load_state_dict(R.gen_params(R.shapes_of(model.state_dict()), 31))
    x = torch.zeros(2, 45, 24)
    x[0, :21] = R.gen_normal("kmask_indep_a", (21, 24), 31)
    x[1] = R.gen_normal("kmask_indep_b", (45, 24), 31)
    return model, x.to(dev), R.prefix_mask([21, 45], 45).to(dev)


def test_batch_independence(dev):
    """A sequence of 21 windows alone (B = 1, T = 21, flag off: the plain kernels) and padded beside a 45-window partner.  With
    mask_padded_keys its rows agree within the stack's output bounds (measured 0 / 0: the same tiles in the same order); without, they
    differ — by 0.39 rel-L2 under the reference's own semantics (oracle.uni_full_transformer in fp64, these inputs)."""
    MT = mta().multiTransformer
    model, x, mask = _b2(dev)
    with torch.no_grad():
        alone = model(x[:1, :21].contiguous(), mask[:1, :21].contiguous(), [21]).cpu()
        padded_plain = model(x, mask, [21, 45]).cpu()
        MT.mask_padded_keys(model)
        padded_keyed = model(x, mask, [21, 45]).cpu()
    check("kmask batch independence, keys masked", padded_keyed[0, :21], alone[0], ENC_OUT, ENC_OUT_ROW)
    rel = float(np.linalg.norm(padded_plain[0, :21].double() - alone[0].double()) / np.linalg.norm(alone[0].double()))
    print("kmask batch dependence without the flag: rel-L2 %.3e" % rel)
    assert rel >= 10 * ENC_OUT


def _train_model(which, dev):
    MT = mta().multiTransformer
    B, T, lengths = 4, 40, [40, 33, 20, 5]
    if which == "mft":
        mods, dims = ["acoustic", "linguistic"], {"acoustic": 88, "linguistic": 300}
        model = MT.MultiTransformer(mods, dims, N=2, device=dev).train()
        x = {m: R.gen_normal("kmask_train:" + m, (B, T, dims[m]), 3).to(dev) for m in mods}
    else:
        model = MT.NLPTransformer(512, embed_dim=128, h=8, N=2, device=dev).train()
        x = torch.tanh(R.gen_normal("kmask_train:x", (B, T, 512), 3)).to(dev)
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("kmask_train:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    return model, x, mask, tgt, lengths


@pytest.mark.parametrize("which", ["sft", "mft"])
def test_train_step_with_masked_keys(dev, which):
    """one train step with the flag on: finite gradients, hand-written kernels only, two runs with one seed bit-identical; and
    mask_padded_keys(model, False) restores the launch sequence of a run made before the flag was ever set"""
    MT, F = mta().multiTransformer, mta().functional
    model, x, mask, tgt, lengths = _train_model(which, dev)
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        torch.manual_seed(77)
        F.mse_sum_loss_backward(model(x, mask, lengths), tgt, sum(lengths))

    _, before = device_kernel_names(step, warm=True)                 # the flag was never set
    found = MT.mask_padded_keys(model)
    assert found and all(m.mask_keys for m in found.values())
    _, names = device_kernel_names(step, warm=True)
    grads = [q.grad.detach().clone() for q in params if q.grad is not None]
    assert grads and all(torch.isfinite(t).all() for t in grads)
    step()
    again = [q.grad for q in params if q.grad is not None]
    assert len(again) == len(grads) and all(torch.equal(a, b) for a, b in zip(again, grads))
    MT.mask_padded_keys(model, False)
    _, after = device_kernel_names(step, warm=True)
    F.check_device_errors()
    if names is None or before is None or after is None:
        pytest.skip("torch.profiler reports no device kernels on this box")
    assert library_kernels(names) == [], library_kernels(names)
    assert _launched(names, _KEYED) == sorted(set(_KEYED) - {"attn_probs_keys_kernel"}), names
    assert _launched(names, _PLAIN) == [], names
    assert _launched(before, _KEYED) == [] and _launched(before, _PLAIN)
    assert sorted(after) == sorted(before)               # (sorted: the modalities of the MFT run on streams of their own)


def test_captured_step_with_masked_keys(dev):
    """a forward + backward with the flag on, captured in a hipGraph (key_lengths_kernel is one more launch of the sequence) and replayed
    on other inputs and other lengths: every replay reproduces the eager step of its own inputs bit for bit (eval mode), as the
    existing capture tests ask of the plain path"""
    MT, F = mta().multiTransformer, mta().functional
    from multimodal_transformer_amd import graphs
    model, x0, mask0 = _b2(dev)
    MT.mask_padded_keys(model)
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
    F.check_device_errors()
