"""CPU tests of the bf16-faithful reference (tests/bf16_ref.py): its primitives, that it is the plain reference with rounding off, and
how far the rounding puts it from the plain reference."""
import math
import time

import numpy as np
import pytest
import torch

import bf16_ref as E
import oracle
import recipe as R
from conftest import rel_l2


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _rne_bf16_bits(x32):
    """bf16 round-to-nearest-even of fp32 values, by integer arithmetic on the bit pattern (finite values)."""
    u = x32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    lsb = (u >> 16) & 1
    r = ((u + 0x7FFF + lsb) >> 16) << 16
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return r.view(torch.float32).double()


# ------------------------------------------------------------------------------------------ primitives
def test_round_fwd_is_round_to_nearest_even():
    """Values off a tie by less than fp32 resolves round as their fp32 value does (torch converts fp64 through fp32): the kernels round
    fp32 values, so that is the rounding to emulate."""
    ulp = 2.0 ** -7                                             # bf16 spacing in [1, 2)
    x = torch.tensor([1 + ulp / 2, 1 + 1.5 * ulp, 1 + 2.5 * ulp, -(1 + ulp / 2), -(1 + 1.5 * ulp),
                      1 + ulp / 2 + 2 ** -20, 1 + ulp / 2 - 2 ** -20, 0.0, 3.0], dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 2 * ulp, 1 + 2 * ulp, -1.0, -(1 + 2 * ulp), 1 + ulp, 1.0, 0.0, 3.0], dtype=torch.float64)
    assert torch.equal(E.round_fwd(x), want)                    # ties go to the even significand, everything else to the nearest
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(20000, generator=g) * torch.exp(4 * torch.randn(20000, generator=g))).float()
    assert torch.equal(E.round_fwd(y.double()), _rne_bf16_bits(y))


def test_round_primitives_change_only_their_own_direction():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, dtype=torch.float64, generator=g)
    up = torch.randn(300, dtype=torch.float64, generator=g)
    assert not torch.equal(E.bf16(x), x) and not torch.equal(E.bf16(up), up)
    a = x.clone().requires_grad_()
    y = E.round_fwd(a)
    assert torch.equal(y, E.bf16(x))                            # forward rounds
    y.backward(up)
    assert torch.equal(a.grad, up)                              # backward is straight-through
    b = x.clone().requires_grad_()
    z = E.round_bwd(b)
    assert torch.equal(z, x)                                    # forward untouched
    z.backward(up)
    assert torch.equal(b.grad, E.bf16(up))                      # backward rounds the incoming gradient


# ------------------------------------------------------------------------------------------ rounding off = the plain references
def _grads(leaves):
    return [t.grad.clone() for t in leaves]


@pytest.mark.parametrize("act,rs,drop", [(0, False, False), (1, True, False), (1, False, True), (0, True, True)])
def test_linear_without_rounding_is_the_plain_affine_map(act, rs, drop):
    M, K, N = 37, 43, 29
    x, W, b, g = (R.gen_normal("e_lin" + n, s, 2) for n, s in (("x", (M, K)), ("W", (N, K)), ("b", (N,)), ("g", (M, N))))
    r = (R.gen_uniform("e_lin_r", (M,), 2) > 0.3).double() if rs else None
    mi = (R.gen_uniform("e_lin_mi", (M, K), 2) > 0.1).double() / 0.9 if drop else None
    mo = (R.gen_uniform("e_lin_mo", (M, N), 2) > 0.5).double() / 0.5 if drop and act == 1 else None
    la = [t.double().requires_grad_() for t in (x, W, b)]
    y = E.linear(*la, act=act, rowscale=r, in_drop=mi, out_drop=mo, rounding=False)
    y.backward(g.double())
    lb = [t.double().requires_grad_() for t in (x, W, b)]
    ref = (lb[0] * mi if mi is not None else lb[0]) @ lb[1].t() + lb[2]
    if act:
        ref = torch.relu(ref)
    if mo is not None:
        ref = ref * mo
    if r is not None:
        ref = ref * r[:, None]
    ref.backward(g.double())
    assert _rel(y, ref) <= 1e-12
    for a, c in zip(_grads(la), _grads(lb)):
        assert _rel(a, c) <= 1e-12


def _heads(z, B, T, h):
    return z.reshape(B, T, h, -1).permute(0, 2, 1, 3)


@pytest.mark.parametrize("T,h,dk,lengths,drop", [(45, 2, 16, [45, 20], False), (70, 4, 10, [70, 1], True), (33, 1, 32, [33, 33], True)])
def test_sdpa_without_rounding_is_the_oracle(T, h, dk, lengths, drop):
    B = len(lengths)
    q, k, v, g = (R.gen_normal("e_sdpa" + n, (B, h, T, dk), 2) for n in "qkvg")
    mask = R.prefix_mask(lengths, T).double().unsqueeze(1)
    pd = (R.gen_uniform("e_sdpa_d", (B, h, T, T), 2) > 0.1).double() / 0.9 if drop else None
    la = [(t * 2).double().requires_grad_() for t in (q, k, v)]
    y, _ = E.sdpa(*la, mask, pd, rounding=False)
    y.backward(g.double())
    lb = [(t * 2).double().requires_grad_() for t in (q, k, v)]
    ref, _ = oracle.scaled_dot_attention(*lb, mask, pd)
    ref.backward(g.double())
    assert _rel(y, ref) <= 1e-12
    for a, c in zip(_grads(la), _grads(lb)):
        assert _rel(a, c) <= 1e-12


def _enc_case(d, h, n, B, T, lengths, tag):
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 5)
    x = R.gen_normal(tag + ":x", (B, T, d), 5)
    g = R.gen_normal(tag + ":g", (B, T, d), 5)
    return p32, x, g, R.prefix_mask(lengths, T)


def _enc_drops(n, B, T, d, h, p, tag):
    def m(name, shape):
        return (R.gen_uniform(tag + name, shape, 5) > p).double() / (1 - p)
    return [{"attn": m("a%d" % i, (B, h, T, T)), "sub0": m("s0%d" % i, (B, T, d)), "ffn": m("f%d" % i, (B, T, R.D_FF)),
             "sub1": m("s1%d" % i, (B, T, d))} for i in range(n)]


def _run_enc(fn, p32, x, g, mask, h, drops, **kw):
    p = {k: v.double().clone().requires_grad_() for k, v in p32.items()}
    xd = x.double().clone().requires_grad_()
    y = fn(p, "", xd, mask.double(), h, drops, **kw)
    y.backward(g.double())
    return y.detach(), xd.grad, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("drop", [False, True], ids=["eval", "train"])
def test_encoder_stack_without_rounding_is_the_oracle(drop):
    d, h, n, B, T, lengths = 40, 4, 2, 2, 33, [33, 9]
    p32, x, g, mask = _enc_case(d, h, n, B, T, lengths, "e_enc")
    drops = _enc_drops(n, B, T, d, h, 0.1, "e_enc_d") if drop else None
    ya, dxa, dpa = _run_enc(E.encoder_stack, p32, x, g, mask, h, drops, rounding=False)
    yb, dxb, dpb = _run_enc(oracle.encoder_stack, p32, x, g, mask, h, drops)
    assert _rel(ya, yb) <= 1e-12 and _rel(dxa, dxb) <= 1e-12
    for k in dpb:
        # the key bias's gradient is analytically zero (softmax is shift-invariant): compare it on the scale of the query bias's
        scale = float(dpb[k.replace("linears.1.bias", "linears.0.bias")].norm())
        assert float((dpa[k] - dpb[k]).norm()) <= 1e-12 * max(float(dpb[k].norm()), scale if "linears.1.bias" in k else 0.0), k


# ------------------------------------------------------------------------------------------ rounding on
def test_rounding_distance_from_the_oracle_at_the_error_budget_shape():
    """DESIGN §2 budgets 3.5e-3 rel-L2 for the bf16 design at T=500, d=128, N=6: the emulator must sit in that range of the oracle —
    far enough to show that it rounds, near enough to show that it rounds only where the kernels do."""
    t0 = time.time()
    d, h, n, B, T = 128, 8, 6, 1, 500
    p32, x, g, mask = _enc_case(d, h, n, B, T, [T], "e_budget")
    with torch.no_grad():
        p = {k: v.double() for k, v in p32.items()}
        y_emu = E.encoder_stack(p, "", x.double(), mask.double(), h)
        y_ref = oracle.encoder_stack(p, "", x.double(), mask.double(), h)
    r = rel_l2(y_emu.numpy(), y_ref.numpy())
    print("bf16 emulator vs fp64 oracle, T=500 d=128 N=6: rel-L2 %.3e (DESIGN §2 budget 3.5e-3)  %.1f s" % (r, time.time() - t0))
    assert 5e-4 <= r <= 2e-2


def test_lazy_rescale_emulation_is_needed():
    """The forward rounds P relative to a lazily moved running maximum (attn.h MMT_RESCALE_THR), then rescales the fp32 sums.  Rounding P
    relative to the exact row maximum instead moves the output by about as much as rounding P at all does (measured 1.1e-3 against
    0.9e-3 here): not emulating it would spend half of the sdpa output bound (2e-3), so bf16_ref emulates it tile by tile."""
    B, h, T, dk = 2, 4, 300, 16
    q, k, v = (R.gen_normal("e_lazy" + n, (B, h, T, dk), 2) for n in "qkv")
    Qp = E.bf16(q.double() * 3 * E.LOG2E / math.sqrt(dk))
    K, V = E.bf16(k.double()), E.bf16(v.double())
    lazy, _ = E._attn_forward_value(Qp, K, V, None, True)
    S = Qp @ K.transpose(-2, -1)
    P = torch.exp2(S - S.amax(dim=-1, keepdim=True))
    exact_max = (E.bf16(P) @ V) / E.bf16(P).sum(dim=-1, keepdim=True)
    ref = torch.softmax(S * E.LN2, dim=-1) @ V
    d_lazy, d_round = _rel(exact_max, lazy), _rel(lazy, ref)
    print("P rounded at the exact vs the lazy maximum: rel-L2 %.3e; lazy-rounded P vs unrounded P: %.3e" % (d_lazy, d_round))
    assert 0.3 * d_round < d_lazy < 3 * d_round


def test_fp32_noise_tips_bf16_roundings():
    """What no reference can emulate: fp32 accumulation noise (a relative 6e-8, half an fp32 ulp) that tips a bf16 rounding to the other
    neighbour.  A tipped operand moves its row by a bf16 ulp of that element, and a tipped hidden pre-activation near 0 flips a ReLU mask.
    The reference against itself with and without such noise, at the d = 256 encoder row of test_gpu_bf16_faithful.py: recorded, and
    it must reach the size measured between the kernels and the reference there (output 7.5e-4, dx 6.4e-3, FFN gradients 2.7e-2), which
    is what sets that file's encoder gradient bounds."""
    d, h, n, B, T, lengths = 256, 8, 2, 2, 45, [45, 20]
    p32, x, g, mask = _enc_case(d, h, n, B, T, lengths, "e_tip")
    ya, dxa, dpa = _run_enc(E.encoder_stack, p32, x, g, mask, h, None)
    with E.jitter(6e-8, 1):
        yb, dxb, dpb = _run_enc(E.encoder_stack, p32, x, g, mask, h, None)
    dy, ddx = _rel(yb, ya), _rel(dxb, dxa)
    dw = max(_rel(dpb[k], dpa[k]) for k in dpa if "linears.1.bias" not in k)
    print("reference vs reference with fp32-level noise, d=256 N=2: out %.2e  dx %.2e  worst parameter gradient %.2e" % (dy, ddx, dw))
    assert 1e-4 < dy < 2e-3 and 1e-3 < ddx and 3e-3 < dw
    with E.jitter(0.0, 1):                                      # the hook itself changes nothing
        yc, _, _ = _run_enc(E.encoder_stack, p32, x, g, mask, h, None)
    assert torch.equal(yc, ya)
