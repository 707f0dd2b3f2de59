"""The hot kernels against the bf16-faithful fp64 reference (tests/bf16_ref.py).

The reference rounds to bf16 wherever the kernels form a bf16 operand, so what is left is fp32-vs-fp64 accumulation order and a few
sites it does not emulate (bf16_ref's docstring lists them).  The bounds are therefore one to two orders of magnitude tighter than
test_gpu_parity's, per tensor and per row: a kernel that is wrong by 0.5-1 % in one tile, one column block or one stage fails here.

Every check reports two measures, each parameter gradient separately:
  * rel-L2 of the tensor;
  * the per-row maximum  max_r ||got_r - ref_r|| / rms_r ||ref_r||  (a row: a window for activations and dx, an output feature for dW,
    one entry of a vector).
Bounds are about 4x the worst value measured on the MI355X.  Where fp32 accumulation noise tips bf16 roundings (and through them ReLU
masks), which no reference can emulate, they follow what that noise does to the reference itself (the constants below say where).  Each
weight-gradient matrix of the stack also has its least-squares scale bounded: noise leaves it alone, a wrongly scaled term does not.

The stack runs under the default paths, under MMT_NO_FIXED_SHAPES=1 and under MMT_NO_CHAIN4=1 MMT_NO_BWD_BOUNDARY=1; the stand-alone
attention's one-kernel backward also under MMT_NO_FUSED_ATTN_BWD=1.  The switches are read once per process, so every GPU run of sdpa
and of the stack happens in a child process (gpu_harness.run_child, which calls child_main below) that hands its arrays back through an
.npz file.  The measures (measures, check) are gpu_harness's.
"""
import json

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import _LIN, LIN_REL, _lin_inputs, check, dev, run_child, tmp_dir  # noqa: F401 (dev, tmp_dir: fixtures)

pytestmark = pytest.mark.gpu

# bounds: measured worst on the MI355X in the comments (rel-L2 / per-row maximum); the affine map's LIN_REL is gpu_harness's
SDPA_OUT, SDPA_OUT_ROW = 4e-4, 1e-2  # 9.9e-5 / 2.6e-3
SDPA_GRAD = 2e-3                     # 4.5e-4
# Per row the attention gradients reach 1.4e-2 (dv at T = 511, d_k = 16, eval), the same on the one- and the two-kernel backward.  The
# reference moves itself by 2e-3 per row there when its values are perturbed at fp32 level before rounding (test_bf16_ref.py
# test_fp32_noise_tips_bf16_roundings): a tipped bf16 rounding of the normaliser l at d_k = 16 (the ones-row sums bf16 P) rescales a whole
# row of the recomputed P.  Held at 2e-2 until that is settled.
SDPA_GRAD_ROW = 2e-2
ENC_OUT, ENC_OUT_ROW = 2e-3, 8e-3    # 7.5e-4 / 2.1e-3
# The stack's gradients are bounded by fp32 noise tipping bf16 roundings, which no reference can emulate without the kernels' own fp32
# accumulation order: perturbing the reference's values by 6e-8 (half an fp32 ulp) before each rounding moves the reference ITSELF by
# 7e-4 on the output, 5e-3 on dx and 2e-2 on the first FFN projection's and the FFN LayerNorm's gradients at d = 256 (one tipped
# operand flips a ReLU mask; test_bf16_ref.py test_fp32_noise_tips_bf16_roundings).  Measured against the kernels: dx and the other
# gradients 6.4e-3 / 3.4e-2, the first FFN projection and the FFN LayerNorm 2.7e-2 (a flipped unit lands in one row of W1 and in a few
# entries of the LayerNorm's gain and bias: no per-row bound on those).
ENC_GRAD, ENC_ROW = 1e-2, 5e-2
ENC_RELU_GRAD = 4e-2
# The d = 40 eval row (generic chains, LayerNorm backward at its smallest d, where a wrong 1/(d-1) costs most) has no tipped rounding that
# reaches a ReLU: measured 3.5e-4 / 1.8e-3 on dx and every gradient, so it is held 4x above that
ENC_CLEAN = {"bfe_d40_n2_T33_p0": (1.5e-3, 7e-3)}
# Tipped roundings are random in sign, so they hardly move the least-squares scale <got - ref, ref> / <ref, ref> of a whole weight-gradient
# matrix (measured <= 4.6e-4); a wrongly scaled term or slab moves all of it
ENC_W_SCALE = 2e-3


# ------------------------------------------------------------------------------------------------ child process
def child_main(kind, out_path, payload_json):
    """The GPU runs of every case in the payload, in a process of their own: kind "sdpa" or "enc"."""
    from multimodal_transformer_amd import functional as F
    cases = json.loads(payload_json)
    dev = torch.device("cuda:0")
    out = {}
    for c in cases:
        cid = c["id"]
        if kind == "sdpa":
            B, T, d, h, lengths, p = c["B"], c["T"], c["d"], c["h"], c["lengths"], c["p"]
            q, k, v, g = (R.gen_normal(cid + n, (B, T, d), 13) for n in "qkvg")
            mask = R.prefix_mask(lengths, T).to(dev)
            leaves = [(2 * q).to(dev).requires_grad_(), k.to(dev).requires_grad_(), v.to(dev).requires_grad_()]
            seed = 1000 + T + d
            y = F.sdpa(*leaves, mask, h, dropout_p=p, seed=seed)
            y.backward(g.to(dev))
            for n, t in zip(("y", "dq", "dk", "dv"), [y.detach()] + [t.grad for t in leaves]):
                out[cid + ":" + n] = t.cpu().numpy()
            if p > 0:
                Tp = -(-T // 32) * 32
                keep, sc = F.dropout_mask(p, seed, 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
                out[cid + ":keep"] = keep.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu().numpy()
                out[cid + ":scale"] = np.array(sc)
        else:
            d, h, n, B, T, lengths, p = c["d"], c["h"], c["n"], c["B"], c["T"], c["lengths"], c["p"]
            p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
            flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
            x = R.gen_normal(cid + ":x", (B, T, d), 17).to(dev).requires_grad_()
            g = R.gen_normal(cid + ":g", (B, T, d), 17).to(dev)
            mask = R.prefix_mask(lengths, T).to(dev)
            seed = 4242 + d + T
            y = F.encoder_stack(x, mask, flat, h, R.D_FF, n, dropout_p=p, seed=seed)
            y.backward(g)
            out[cid + ":y"], out[cid + ":dx"], out[cid + ":dflat"] = y.detach().cpu().numpy(), x.grad.cpu().numpy(), flat.grad.cpu().numpy()
            if p > 0:
                Tp, DP, FP, M = -(-T // 32) * 32, -(-d // 64) * 64, -(-R.D_FF // 64) * 64, B * T
                for l in range(n):
                    ka, sa = F.dropout_mask(p, seed, 4 * l + 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
                    k0, s0 = F.dropout_mask(p, seed, 4 * l + 1, M * DP, dev)
                    kf, sf = F.dropout_mask(p, seed, 4 * l + 2, M * FP, dev)
                    k1, s1 = F.dropout_mask(p, seed, 4 * l + 3, M * DP, dev)
                    out["%s:attn%d" % (cid, l)] = ka.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu().numpy()
                    out["%s:sub0%d" % (cid, l)] = k0.reshape(B, T, DP)[:, :, :d].cpu().numpy()
                    out["%s:ffn%d" % (cid, l)] = kf.reshape(B, T, FP)[:, :, :R.D_FF].cpu().numpy()
                    out["%s:sub1%d" % (cid, l)] = k1.reshape(B, T, DP)[:, :, :d].cpu().numpy()
                    out["%s:scales%d" % (cid, l)] = np.array([sa, s0, sf, s1])
    torch.cuda.synchronize()
    F.check_device_errors()
    np.savez(out_path, **out)


_SWITCHES = {"default": {}, "no_fused_attn_bwd": {"MMT_NO_FUSED_ATTN_BWD": "1"}, "no_fixed_shapes": {"MMT_NO_FIXED_SHAPES": "1"},
             "no_chain4_boundary": {"MMT_NO_CHAIN4": "1", "MMT_NO_BWD_BOUNDARY": "1"}}


def _child(kind, switch, cases, tmp_dir):
    return run_child(__name__, kind, switch, cases, tmp_dir, _SWITCHES, timeout=300)


# ------------------------------------------------------------------------------------------------ linear
def _lin_compare(tag, y, leaves, x, W, b, g, **kw):
    ld = [t.double().requires_grad_() for t in (x, W, b)]
    ref = E.linear(*ld, **kw)
    ref.backward(g.double())
    check(tag + " y", y.detach().cpu(), ref.detach(), LIN_REL, LIN_REL)
    for n, a, r in zip(("dx", "dW", "db"), leaves, ld):
        check(tag + " " + n, a.grad.cpu(), r.grad, LIN_REL, LIN_REL)
    return ref


@pytest.mark.parametrize("M,K,N,act,rs", _LIN)
def test_linear(dev, M, K, N, act, rs):
    tag = "bf lin%dx%dx%d a%d%s" % (M, K, N, act, " rs" if rs else "")
    x, W, b, g = _lin_inputs(M, K, N, "bflin%dx%dx%d" % (M, K, N))
    r = (R.gen_uniform("bflin_r%d" % M, (M,), 5) > 0.3).float() if rs else None
    F = pytest.importorskip("multimodal_transformer_amd").functional
    leaves = [t.to(dev).requires_grad_() for t in (x, W, b)]
    y = F.linear(*leaves, act=act, rowscale=None if r is None else r.to(dev))
    y.backward(g.to(dev))
    _lin_compare(tag, y, leaves, x, W, b, g, act=act, rowscale=None if r is None else r.double())
    if rs:
        assert (y.detach().cpu()[r == 0] == 0).all()


@pytest.mark.parametrize("M,K,N", [(70, 300, 96), (33, 43, 129), (200, 576, 5)])
@pytest.mark.parametrize("in_p,out_p", [(0.1, 0.0), (0.0, 0.5), (0.25, 0.5)])
def test_linear_dropout_replay(dev, M, K, N, in_p, out_p):
    F = pytest.importorskip("multimodal_transformer_amd").functional
    tag = "bf lin drop %dx%dx%d in %.2f out %.2f" % (M, K, N, in_p, out_p)
    x, W, b, g = _lin_inputs(M, K, N, "bflindrop%dx%dx%d" % (M, K, N))
    seed = 77 + K
    leaves = [t.to(dev).requires_grad_() for t in (x, W, b)]
    y = F.linear(*leaves, act=1, in_dropout=in_p, out_dropout=out_p, seed=seed)
    y.backward(g.to(dev))
    Kx = K + (-K) % 4                                   # functional.linear pads the input width to a multiple of 4
    KP, NP = -(-Kx // 64) * 64, -(-N // 64) * 64
    mi = mo = None
    if in_p > 0:
        kk, sc = F.dropout_mask(in_p, seed, 2000, M * KP, dev)
        mi = (kk.reshape(M, KP)[:, :K].double() * sc).cpu()
    if out_p > 0:
        kk, sc = F.dropout_mask(out_p, seed, 2001, M * NP, dev)
        mo = (kk.reshape(M, NP)[:, :N].double() * sc).cpu()
    _lin_compare(tag, y, leaves, x, W, b, g, act=1, in_drop=mi, out_drop=mo)


# ------------------------------------------------------------------------------------------------ sdpa
_SDPA_T = [1, 31, 32, 33, 65, 256, 257, 288, 319, 320, 385, 481, 511, 512, 513]


def _sdpa_cases():
    cs = []
    for dk in (16, 10):
        for T in _SDPA_T:
            cs.append((T, dk))
    for dk in (32, 48, 64):
        for T in (33, 70, 300):
            cs.append((T, dk))
    out = []
    for T, dk in cs:
        for p in (0.0, 0.1):
            h = 2
            lengths = [T, max(1, (2 * T) // 3), 1]
            out.append({"id": "bfs_T%d_dk%d_p%g" % (T, dk, p), "B": 3, "T": T, "d": h * dk, "h": h, "lengths": lengths, "p": p})
    return out


SDPA_CASES = _sdpa_cases()


def _fused(c):
    return E.one_kernel_bwd(c["d"] // c["h"], c["T"])


def _sdpa_ref(c, run, fused_attn_bwd=True):
    cid, B, T, d, h, lengths, p = c["id"], c["B"], c["T"], c["d"], c["h"], c["lengths"], c["p"]
    dk = d // h
    q, k, v, g = (R.gen_normal(cid + n, (B, T, d), 13) for n in "qkvg")
    drop = None
    if p > 0:
        drop = torch.from_numpy(run[cid + ":keep"]).double() * float(run[cid + ":scale"])

    def split(z):
        return z.reshape(B, T, h, dk).permute(0, 2, 1, 3)
    leaves = [t.double().requires_grad_() for t in (2 * q, k, v)]
    ctx, _ = E.sdpa(*(split(t) for t in leaves), R.prefix_mask(lengths, T).double().unsqueeze(1), drop, fused_attn_bwd=fused_attn_bwd)
    ref = ctx.permute(0, 2, 1, 3).reshape(B, T, d)
    ref.backward(g.double())
    return {"y": ref.detach().numpy(), "dq": leaves[0].grad.numpy(), "dk": leaves[1].grad.numpy(), "dv": leaves[2].grad.numpy()}


def _sdpa_check(tag, c, run, ref):
    for n in ("y", "dq", "dk", "dv"):
        # at T = 1 dq and dk are analytically zero (one key: the softmax is constant): measured on dv's scale
        zero = n in ("dq", "dk") and np.linalg.norm(ref[n]) < 1e-9 * np.linalg.norm(ref["dv"])
        check("%s %s" % (tag, n), run[c["id"] + ":" + n], ref[n], SDPA_OUT if n == "y" else SDPA_GRAD,
              SDPA_OUT_ROW if n == "y" else SDPA_GRAD_ROW, scale_ref=ref["dv"] if zero else None)
    for bi, L in enumerate(c["lengths"]):                  # blanked query rows pass exactly zero gradient to q
        assert (run[c["id"] + ":dq"][bi, L:] == 0).all()


@pytest.mark.parametrize("c", SDPA_CASES, ids=[c["id"] for c in SDPA_CASES])
def test_sdpa(tmp_dir, c):
    run = _child("sdpa", "default", SDPA_CASES, tmp_dir)
    ref = _sdpa_ref(c, run)
    _sdpa_check("bf sdpa T%d dk%d p%g" % (c["T"], c["d"] // c["h"], c["p"]), c, run, ref)
    if _fused(c):
        # the two-kernel backward: the same masks (same seeds), against the emulator and against the one-kernel backward
        two = _child("sdpa", "no_fused_attn_bwd", [x for x in SDPA_CASES if _fused(x)], tmp_dir)
        _sdpa_check("bf sdpa-2k T%d dk%d p%g" % (c["T"], c["d"] // c["h"], c["p"]), c, two, _sdpa_ref(c, two, False) if c["p"] > 0 else ref)
        # in eval mode the two round the same operands (only fp32 orders differ); in train mode the one-kernel backward rounds dS/c and
        # P m/c instead of dS and P m/(1-p), two different designs that each match their own emulation above, 3.5e-3 apart in dq
        if c["p"] == 0:
            for n in ("y", "dq", "dk", "dv"):
                check("bf sdpa 1k-vs-2k T%d %s" % (c["T"], n), run[c["id"] + ":" + n], two[c["id"] + ":" + n],
                      SDPA_OUT if n == "y" else SDPA_GRAD, SDPA_OUT_ROW if n == "y" else SDPA_GRAD_ROW)


# ------------------------------------------------------------------------------------------------ encoder stack
_ENC_ROWS = [(128, 8, 2, 3, 70, [70, 33, 1]), (128, 8, 1, 2, 300, [300, 170]), (256, 8, 2, 2, 45, [45, 20]), (40, 4, 2, 2, 33, [33, 9]),
             (40, 4, 1, 1, 300, [300]), (512, 8, 1, 2, 40, [40, 17]), (128, 8, 1, 1, 1, [1])]


def _enc_cases():
    out = []
    for d, h, n, B, T, lengths in _ENC_ROWS:
        for p in (0.0, 0.25 if d == 40 else 0.1):
            out.append({"id": "bfe_d%d_n%d_T%d_p%g" % (d, n, T, p), "d": d, "h": h, "n": n, "B": B, "T": T, "lengths": lengths, "p": p})
    return out


ENC_CASES = _enc_cases()
_ENC_REFS = {}


def _enc_ref(c, run):
    """The emulator's result for case c (the masks of a train-mode case are the kernels', which every switch set shares)."""
    if c["id"] in _ENC_REFS:
        return _ENC_REFS[c["id"]]
    cid, d, h, n, B, T, lengths, p = (c[k] for k in ("id", "d", "h", "n", "B", "T", "lengths", "p"))
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    drops = None
    if p > 0:
        drops = []
        for l in range(n):
            sc = run["%s:scales%d" % (cid, l)]
            drops.append({k: torch.from_numpy(run["%s:%s%d" % (cid, k, l)]).double() * float(s)
                          for k, s in zip(("attn", "sub0", "ffn", "sub1"), sc)})
    pd = {k: v.double().clone().requires_grad_() for k, v in p32.items()}
    x = R.gen_normal(cid + ":x", (B, T, d), 17).double().requires_grad_()
    g = R.gen_normal(cid + ":g", (B, T, d), 17).double()
    y = E.encoder_stack(pd, "", x, R.prefix_mask(lengths, T).double(), h, drops)
    y.backward(g)
    _ENC_REFS[cid] = (y.detach().numpy(), x.grad.numpy(), {k: v.grad.numpy() for k, v in pd.items()})
    return _ENC_REFS[cid]


@pytest.mark.parametrize("switch", ["default", "no_fixed_shapes", "no_chain4_boundary"])
@pytest.mark.parametrize("c", ENC_CASES, ids=[c["id"] for c in ENC_CASES])
def test_encoder_stack(tmp_dir, c, switch):
    run = _child("enc", switch, ENC_CASES, tmp_dir)
    y, dx, grads = _enc_ref(c, _child("enc", "default", ENC_CASES, tmp_dir))
    tag = "bf enc d%d n%d T%d p%g %s" % (c["d"], c["n"], c["T"], c["p"], switch)
    failures = []
    g_rel, g_row = ENC_CLEAN.get(c["id"], (ENC_GRAD, ENC_ROW))
    check(tag + " y", run[c["id"] + ":y"], y, ENC_OUT, ENC_OUT_ROW, failures=failures)
    check(tag + " dx", run[c["id"] + ":dx"], dx, g_rel, g_row, failures=failures)
    flat, off = run[c["id"] + ":dflat"], 0
    for name, shape in E.encoder_param_shapes(c["d"], R.D_FF, c["n"]).items():
        size = int(np.prod(shape))
        got = flat[off: off + size].reshape(shape)
        off += size
        # the key bias's gradient is analytically zero (softmax is shift-invariant): measured on the query bias's scale; at T = 1 (one
        # key: a constant softmax) the query and key projections get none at all: measured on the value projection's scale
        scale = grads[name.replace("linears.1.bias", "linears.0.bias")] if "linears.1.bias" in name else None
        if c["T"] == 1 and ("linears.0." in name or "linears.1." in name):
            scale = grads[name.replace("linears.0.", "linears.2.").replace("linears.1.", "linears.2.")]
        flips = ".w_1." in name or "sublayer.1.norm" in name
        if c["id"] in ENC_CLEAN:
            check(tag + " " + name, got, grads[name], g_rel, g_row, scale_ref=scale, failures=failures)
        else:
            check(tag + " " + name, got, grads[name], ENC_RELU_GRAD if flips else ENC_GRAD, None if flips else ENC_ROW, scale_ref=scale,
                  failures=failures)
        if len(shape) == 2 and not (c["T"] == 1 and ("linears.0." in name or "linears.1." in name)):
            r = grads[name].astype(np.float64).ravel()
            s = float(np.dot(got.astype(np.float64).ravel() - r, r) / np.dot(r, r))
            if abs(s) > ENC_W_SCALE:
                failures.append("%s %s: scale %.3e > %.1e" % (tag, name, s, ENC_W_SCALE))
    assert off == flat.size
    assert not failures, "\n".join(failures)
