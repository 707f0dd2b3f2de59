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
from gpu_harness import ls_scale, measures, seq_max


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


# ------------------------------------------------------------------------------------------ scans
def _lstm_inputs(T, B, H, init, tag):
    gx = R.gen_normal(tag + "gx", (T, B, 4 * H), 3)
    W = R.gen_normal(tag + "w", (4 * H, H), 3) / np.sqrt(H)
    h0 = 0.5 * R.gen_normal(tag + "h0", (B, H), 3) if init else None
    c0 = 0.5 * R.gen_normal(tag + "c0", (B, H), 3) if init else None
    gh, gc = R.gen_normal(tag + "gh", (T, B, H), 3), R.gen_normal(tag + "gc", (T, B, H), 3)
    return gx, W, h0, c0, gh, gc


def _run_lstm(fn, inputs, **kw):
    gx, W, h0, c0, gh, gc = inputs
    leaves = [None if t is None else t.double().clone().requires_grad_() for t in (gx, W, h0, c0)]
    h, c = fn(*leaves, **kw)
    ((h * gh.double()).sum() + (c * gc.double()).sum()).backward()
    out = {"h": h.detach(), "c": c.detach(), "dgx": leaves[0].grad, "dW": leaves[1].grad}
    if h0 is not None:
        out["dh0"], out["dc0"] = leaves[2].grad, leaves[3].grad
    return out


def _mfn_inputs(T, B, tag):
    apre = R.gen_normal(tag + "a", (T, B, 128), 3)
    chat = torch.tanh(R.gen_normal(tag + "c", (T, B, 128), 3))
    Wm = R.gen_normal(tag + "wm", (128, 128), 3) / np.sqrt(128)
    W2 = R.gen_normal(tag + "w2", (2, 128, 64), 3) / 8
    b2 = 0.1 * R.gen_normal(tag + "b2", (2, 128), 3)
    return apre, chat, Wm, W2, b2, R.gen_normal(tag + "g", (T, B, 128), 3)


def _run_mfn(fn, inputs, **kw):
    *args, g = inputs
    leaves = [t.double().clone().requires_grad_() for t in args]
    mem = fn(*leaves, **kw)
    (mem * g.double()).sum().backward()
    return dict(zip(("mem", "dapre", "dchat", "dWm", "dW2", "db2"), [mem.detach()] + [t.grad for t in leaves]))


def _mfn_drop(T, B, p, tag):
    return (R.gen_uniform(tag + "drop", (T, B, 128), 3) > p).double() / (1 - p)


@pytest.mark.parametrize("init", [False, True])
def test_lstm_scan_without_rounding_is_the_oracle_loop(init):
    from test_gpu_models import _oracle_lstm
    inputs = _lstm_inputs(7, 5, 20, init, "e_lstm")
    a = _run_lstm(E.lstm_scan, inputs, rounding=False)
    b = _run_lstm(_oracle_lstm, inputs)
    for k in b:
        assert _rel(a[k], b[k]) <= 1e-12, k


@pytest.mark.parametrize("drop", [False, True])
def test_mfn_mem_scan_without_rounding_is_the_plain_recurrence(drop):
    from test_gpu_models import _oracle_mem_scan
    T, B = 6, 3
    inputs = _mfn_inputs(T, B, "e_mfn")
    d = _mfn_drop(T, B, 0.2, "e_mfn") if drop else None
    a = _run_mfn(E.mfn_mem_scan, inputs, drop=d, rounding=False)
    b = _run_mfn(_oracle_mem_scan, inputs, drop=d)
    for k in b:
        assert _rel(a[k], b[k]) <= 1e-12, k


def _lstm_case(cid):
    import test_gpu_bf16_scans as S
    return next(c for c in S.LSTM_CASES if c["id"] == cid)


def test_scan_jitter_floor():
    """The floor of the scan bounds in test_gpu_bf16_scans.py: how far fp32-level noise (half an fp32 ulp before every bf16 rounding)
    moves the reference from itself at the long shapes of that file.  Tipped bf16(h) roundings feed back through the recurrence, so the
    distance is also reported per time step.  Every bound there must sit at or above this floor."""
    import test_gpu_bf16_scans as S
    lstm_b = {"h": S.LSTM_OUT, "c": S.LSTM_OUT, "dgx": S.LSTM_DGX, "dW": S.LSTM_DW, "dh0": S.LSTM_D0, "dc0": S.LSTM_D0}
    t0 = time.time()
    for cid in ("l_T1000_B3_H48_i_hc", "l_T1000_B2_H88_n_hc", "l_T1000_B2_H256_i_hc"):
        c = _lstm_case(cid)
        a = S.lstm_ref(c)
        S._LSTM_REFS.pop(cid)
        with E.jitter(6e-8, 1):
            b = S.lstm_ref(c)
        S._LSTM_REFS.pop(cid)
        for k in a:
            rel, row = measures(b[k], a[k])
            seq = seq_max(b[k], a[k]) if a[k].ndim == 3 else 0.0
            print("jitter floor %s %-4s rel-L2 %.2e  row-max %.2e  seq-max %.2e" % (cid, k, rel, row, seq))
            bd = lstm_b[k]
            assert rel <= bd[0] and row <= bd[1] and (a[k].ndim != 3 or seq <= bd[2]), (cid, k)
        if "dW" in a:
            assert abs(ls_scale(b["dW"], a["dW"])) <= S.LSTM_W_SCALE
        d = np.linalg.norm((b["h"] - a["h"]).reshape(c["T"], -1), axis=1) / np.linalg.norm(a["h"].reshape(c["T"], -1), axis=1)
        print("jitter floor %s h per step: t < 10 %.1e, t < 100 %.1e, t < 1000 %.1e" % (cid, d[:10].max(), d[:100].max(), d.max()))
    for cid in ("m_T1000_B2_p0", "m_T300_B33_p0"):
        c = next(x for x in S.MFN_CASES if x["id"] == cid)
        inputs = S.mfn_inputs(c)
        a = _run_mfn(E.mfn_mem_scan, inputs)
        with E.jitter(6e-8, 1):
            b = _run_mfn(E.mfn_mem_scan, inputs)
        bds = S.mfn_bounds(c)
        for k in a:
            ga, gb = a[k].numpy(), b[k].numpy()
            if k == "db2":
                ga, gb = ga.ravel(), gb.ravel()
            rel, row = measures(gb, ga)
            seq = seq_max(gb, ga) if k in ("mem", "dapre", "dchat") else 0.0
            print("jitter floor %s %-5s rel-L2 %.2e  row-max %.2e  seq-max %.2e" % (cid, k, rel, row, seq))
            bd = bds[k]
            assert rel <= bd[0] and (bd[1] is None or row <= bd[1]) and (len(bd) < 3 or seq <= bd[2]), (cid, k)
        d = np.linalg.norm((b["mem"] - a["mem"]).numpy().reshape(c["T"], -1), axis=1)
        d /= np.linalg.norm(a["mem"].numpy().reshape(c["T"], -1), axis=1)
        print("jitter floor %s mem per step: t < 10 %.1e, t < 100 %.1e, t < %d %.1e" % (cid, d[:10].max(), d[:100].max(), c["T"], d.max()))
    print("%.1f s" % (time.time() - t0))


# Mutations of the reference itself, each a subtle kernel bug: each must exceed the bound test_gpu_bf16_scans.py applies, on the
# measure meant to catch it, so those bounds see such a bug without a broken kernel ever running.
def _mut_stale(inputs):
    hist = {}

    def h(t, x):                    # sequence 3 multiplies h_{t-2} instead of h_{t-1} at step 10: a one-step-stale exchange
        hist[t] = x
        if t != 10:
            return x
        x = x.clone()
        x[3] = hist[9][3]
        return x
    return _run_lstm(E.lstm_scan, inputs, mutate={"h": h})


def _mut_ragged_tile(inputs):
    gx, W, h0, c0, gh, gc = inputs
    H = W.shape[1]
    last = (H - 1) // 16 * 16        # the last, ragged 16-unit tile: rows q H + u of every gate q, u >= last
    Wt = W.clone()
    for q in range(4):
        Wt[q * H + last:(q + 1) * H] *= 1.01
    return _run_lstm(E.lstm_scan, (gx, Wt, h0, c0, gh, gc))


def _mut_dc_carry(inputs):           # the dc carry from step 10 back to c_9 dropped
    return _run_lstm(E.lstm_scan, inputs, mutate={"c": lambda t, c: c.detach() if t == 10 else c})


def _mut_dh0(inputs):
    """dh0 without the contribution of step 0: the recurrent gradient of step 1 (the loop stops one step early)"""
    kept = {}

    def h(t, x):
        if t == 1:
            kept["h"] = x + 0.0
            kept["h"].retain_grad()
            return kept["h"]
        return x
    out = _run_lstm(E.lstm_scan, inputs, mutate={"h": h})
    out["dh0"] = kept["h"].grad
    return out


def _mut_relu_mask(T, B, p, tag):
    drop = _mfn_drop(T, B, p, tag)
    sc = 1 / (1 - p)

    def u(t, r, d):                  # relu' taken from the pre-dropout value: dropped units pass their gradient (scaled) on
        return r * sc - (r * (sc - d)).detach()
    return _run_mfn(E.mfn_mem_scan, _mfn_inputs(T, B, tag), drop=drop, mutate={"u": u}), drop


def _mut_db2(T, B, tag):             # db2 summed from the unrounded dz
    return _run_mfn(E.mfn_mem_scan, _mfn_inputs(T, B, tag), mutate={"z": lambda t, g, prod, b: E.round_bwd(prod) + b})


_LSTM_MUTANTS = [("stale_exchange", _mut_stale, (20, 5, 256), "h", 1), ("stale_exchange_seq", _mut_stale, (20, 5, 256), "h", 2),
                 ("ragged_tile", _mut_ragged_tile, (13, 5, 20), "h", 1), ("ragged_tile_rel", _mut_ragged_tile, (13, 5, 20), "h", 0),
                 ("dc_carry", _mut_dc_carry, (20, 5, 48), "dgx", 1), ("dh0_step0", _mut_dh0, (20, 5, 88), "dh0", 1)]


@pytest.mark.parametrize("name,mut,shape,tensor,measure", _LSTM_MUTANTS, ids=[m[0] for m in _LSTM_MUTANTS])
def test_lstm_scan_bounds_see_a_mutant(name, mut, shape, tensor, measure):
    """measure: 0 rel-L2, 1 per-row maximum, 2 per-sequence maximum, against the bound of test_gpu_bf16_scans.py"""
    import test_gpu_bf16_scans as S
    inputs = _lstm_inputs(*shape, True, "e_mut_" + name)
    ref = _run_lstm(E.lstm_scan, inputs)
    got = mut(inputs)
    g, r = got[tensor].numpy(), ref[tensor].numpy()
    m = (measures(g, r) + (seq_max(g, r) if r.ndim == 3 else None,))[measure]
    bound = {"h": S.LSTM_OUT, "dgx": S.LSTM_DGX, "dh0": S.LSTM_D0}[tensor][measure]
    print("mutant %s: %s %s %.3e (bound %.1e)" % (name, tensor, ("rel-L2", "row-max", "seq-max")[measure], m, bound))
    assert m > bound


def test_mfn_mem_scan_bounds_see_a_mutant():
    import test_gpu_bf16_scans as S
    T, B, p = 5, 17, 0.2                                   # a short-tier case of test_gpu_bf16_scans.py
    got, drop = _mut_relu_mask(T, B, p, "e_mut_relu")
    ref = _run_mfn(E.mfn_mem_scan, _mfn_inputs(T, B, "e_mut_relu"), drop=drop)
    row = measures(got["dapre"].numpy(), ref["dapre"].numpy())[1]
    print("mutant relu' before dropout: dapre row-max %.3e (bound %.1e)" % (row, S.MFN_SHORT["dapre"][1]))
    assert row > S.MFN_SHORT["dapre"][1]
    T, B = 3, 1                                            # an exact-tier case
    got = _mut_db2(T, B, "e_mut_db2")
    ref = _run_mfn(E.mfn_mem_scan, _mfn_inputs(T, B, "e_mut_db2"))
    row = measures(got["db2"].numpy().ravel(), ref["db2"].numpy().ravel())[1]
    print("mutant db2 from the unrounded dz: db2 row-max %.3e (bound %.1e)" % (row, S.MFN_EXACT["db2"][1]))
    assert row > S.MFN_EXACT["db2"][1]
    for k in ("mem", "dapre", "dchat", "dWm", "dW2"):     # nothing else moves: only the bias's own gradient is summed differently
        assert torch.equal(got[k], ref[k]), k


# ------------------------------------------------------------------------------------------ window encoder (front end)
def _conv_small(N=23, W=9, D=20, F=37, tag="e_conv"):
    x = R.gen_normal(tag + "x", (N, W, D), 4)
    w = R.gen_normal(tag + "w", (F, D, 2), 4) / np.sqrt(2 * D)
    b = 0.1 * R.gen_normal(tag + "b", (F,), 4)
    return x, w, b, R.gen_normal(tag + "g", (N, F), 4)


def _run_conv(x, w, b, g, **kw):
    wl, bl = w.double().clone().requires_grad_(), b.double().clone().requires_grad_()
    out, arg, S = E.conv_maxpool(x.double(), wl, bl, **kw)
    out.backward(g.double())
    return {"out": out.detach(), "arg": arg, "S": S, "dW": wl.grad, "db": bl.grad}


def test_conv_maxpool_without_rounding_is_the_oracle():
    from test_gpu_frontend import _conv_fp64
    x, w, b, g = _conv_small()
    a = _run_conv(x, w, b, g, rounding=False)
    wl, bl = w.double().requires_grad_(), b.double().requires_grad_()
    out, arg = oracle.cnn_maxpool(x.double(), wl, bl)
    out.backward(g.double())
    assert _rel(a["out"], out) <= 1e-12 and torch.equal(a["arg"], arg)
    assert _rel(a["dW"], wl.grad) <= 1e-12 and _rel(a["db"], bl.grad) <= 1e-12
    y = _conv_fp64(x, w, b)
    assert _rel(a["out"], y.max(dim=1).values) <= 1e-12 and _rel(a["S"] + b.double(), y) <= 1e-12
    # a given argmax is gathered, whatever it is: the gradient of that choice
    other = (arg + 1) % (x.shape[1] - 1)
    c = _run_conv(x, w, b, g, arg=other, rounding=False)
    assert _rel(c["out"], y.gather(1, other.unsqueeze(1)).squeeze(1)) <= 1e-12
    # with rounding on: dW from bf16(dy) and bf16(x) rows at the argmax, db from the unrounded dy
    r = _run_conv(x, w, b, g)
    xr, gr = E.bf16(x.double()), E.bf16(g.double())
    n_idx = torch.arange(x.shape[0]).unsqueeze(1).expand_as(r["arg"])
    for j in range(2):
        assert _rel(r["dW"][:, :, j], (gr.unsqueeze(2) * xr[n_idx, r["arg"] + j]).sum(dim=0)) <= 1e-12
    assert _rel(r["db"], g.double().sum(0)) <= 1e-12 and not torch.equal(gr, g.double())


@pytest.mark.parametrize("act", [2, 3])
def test_linear_tanh_sigmoid_without_rounding_is_the_plain_map(act):
    M, K, N = 37, 43, 29
    x, W, b, g = (R.gen_normal("e_lin" + n, s, 2) for n, s in (("x", (M, K)), ("W", (N, K)), ("b", (N,)), ("g", (M, N))))
    r = (R.gen_uniform("e_lin_r", (M,), 2) > 0.3).double()
    la = [t.double().requires_grad_() for t in (x, W, b)]
    E.linear(*la, act=act, rowscale=r, rounding=False).backward(g.double())
    lb = [t.double().requires_grad_() for t in (x, W, b)]
    pre = lb[0] @ lb[1].t() + lb[2]
    ((torch.tanh(pre) if act == 2 else torch.sigmoid(pre)) * r[:, None]).backward(g.double())
    for a, c in zip(_grads(la), _grads(lb)):
        assert _rel(a, c) <= 1e-12
    # with rounding on, the backward's operand is ONE rounding of dy * rowscale * act'(y): db is its column sum
    lc = [t.double().requires_grad_() for t in (x, W, b)]
    y = E.linear(*lc, act=act, rowscale=r)
    y.backward(g.double())
    yy = (y.detach() / r[:, None]).nan_to_num()
    dact = 1 - yy * yy if act == 2 else yy * (1 - yy)
    assert _rel(lc[2].grad, E.bf16(g.double() * r[:, None] * dact).sum(0)) <= 1e-12


def _hw_params(n, tag):
    names = ("linear_projection.weight", "linear_projection.bias", "linear_gate.weight", "linear_gate.bias")
    return R.gen_params({k: ((n, n) if k.endswith("weight") else (n,)) for k in names}, 4), names


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("proj_act", [0, 1])
def test_highway_without_rounding_is_the_oracle(proj_act, drop):
    rows, n = 11, 44
    p32, names = _hw_params(n, "e_hw")
    x, g = R.gen_normal("e_hw:x", (rows, n), 4), R.gen_normal("e_hw:g", (rows, n), 4)
    d = (R.gen_uniform("e_hw:d", (rows, n), 4) > 0.3).double() / 0.7 if drop else None
    la = [x.double().requires_grad_()] + [p32[k].double().requires_grad_() for k in names]
    E.highway(*la, drop=d, proj_act=proj_act, rounding=False).backward(g.double())
    pd = {k: v.double().requires_grad_() for k, v in p32.items()}
    xd = x.double().requires_grad_()
    if proj_act == 0:
        ref = oracle.highway(pd, "", xd)
    else:                                                       # the B1 variant: ReLU on the projection
        gate = torch.sigmoid(xd @ pd[names[2]].t() + pd[names[3]])
        ref = gate * torch.relu(xd @ pd[names[0]].t() + pd[names[1]]) + (1 - gate) * xd
    ref = ref if d is None else ref * d
    ref.backward(g.double())
    for a, c in zip(_grads(la), [xd.grad] + [pd[k].grad for k in names]):
        assert _rel(a, c) <= 1e-12


def test_linear_pair_without_rounding_is_two_plain_maps():
    M, K = 13, 20
    x, W1, b1, W2, b2, g1, g2 = (R.gen_normal("e_pair" + n, s, 4) for n, s in (("x", (M, K)), ("w1", (9, K)), ("b1", (9,)), ("w2", (31, K)),
                                                                                  ("b2", (31,)), ("g1", (M, 9)), ("g2", (M, 31))))
    la = [t.double().requires_grad_() for t in (x, W1, b1, W2, b2)]
    y1, y2 = E.linear_pair(*la, act1=1, act2=0, rounding=False)
    ((y1 * g1.double()).sum() + (y2 * g2.double()).sum()).backward()
    lb = [t.double().requires_grad_() for t in (x, W1, b1, W2, b2)]
    r1, r2 = torch.relu(lb[0] @ lb[1].t() + lb[2]), lb[0] @ lb[3].t() + lb[4]
    ((r1 * g1.double()).sum() + (r2 * g2.double()).sum()).backward()
    assert _rel(y1, r1) <= 1e-12 and _rel(y2, r2) <= 1e-12
    for a, c in zip(_grads(la), _grads(lb)):
        assert _rel(a, c) <= 1e-12


def _chain_params(mod, Fo, D, seed=4):
    h = "highway_%s." % mod
    return R.gen_params({"cnn_%s.conv1d.weight" % mod: (Fo, D, 2), "cnn_%s.conv1d.bias" % mod: (Fo,), h + "linear_projection.weight": (Fo, Fo),
                         h + "linear_projection.bias": (Fo,), h + "linear_gate.weight": (Fo, Fo), h + "linear_gate.bias": (Fo,)}, seed)


@pytest.mark.parametrize("drop", [False, True])
def test_window_encoder_without_rounding_is_the_oracle(drop):
    mod, Fo, D, B, T, W = "acoustic", 44, 24, 2, 7, 6
    p32 = _chain_params(mod, Fo, D)
    x, g = R.gen_normal("e_we:x", (B, T, W, D), 4), R.gen_normal("e_we:g", (B, T, Fo), 4)
    d = (R.gen_uniform("e_we:d", (B * T, Fo), 4) > 0.3).double() / 0.7 if drop else None
    pa = {k: v.double().requires_grad_() for k, v in p32.items()}
    ya, _ = E.window_encoder(pa, mod, x.double(), d, rounding=False)
    ya.backward(g.double())
    pb = {k: v.double().requires_grad_() for k, v in p32.items()}
    yb = oracle.window_encoder(pb, mod, x.double(), d)
    yb.backward(g.double())
    assert _rel(ya, yb) <= 1e-12
    for k in pb:
        assert _rel(pa[k].grad, pb[k].grad) <= 1e-12, k


# The plan of every conv case of tests/test_gpu_bf16_frontend.py, from reading carve_conv (K = 2, ktap = false) and mmt_convpool_forward (csrc/api.hip):
# (wins, pairs in the fullest split, splits, windows of the last split, ONE_RT, row tiles, forward launches (CT, blocks, c_first))
_PLANS = {
    (3001, 10, 88, 256): (6, 3, 501, 1, True, 1, [(4, 1, 0)]),
    (331, 30, 1000, 256): (6, 3, 56, 1, True, 1, [(4, 1, 0)]),
    (600, 33, 300, 300): (8, 4, 75, 8, True, 1, [(4, 1, 0), (1, 1, 256)]),
    (4000, 9, 20, 20): (8, 4, 500, 8, True, 1, [(1, 1, 0)]),
    (2100, 70, 24, 32): (6, 3, 350, 6, False, 3, [(1, 1, 0)]),
    (2565, 10, 88, 256): (6, 3, 428, 3, True, 1, [(4, 1, 0)]),
    (2565, 12, 88, 256): (6, 3, 428, 3, True, 1, [(4, 1, 0)]),
    (21, 12, 88, 256): (2, 1, 11, 1, True, 1, [(4, 1, 0)]),
    (21, 40, 40, 64): (2, 1, 11, 1, False, 2, [(1, 1, 0)]),
    (40, 40, 40, 64): (2, 1, 20, 2, False, 2, [(1, 1, 0)]),
    (24, 3, 40, 64): (2, 1, 12, 2, True, 1, [(1, 1, 0)]),
    (24, 34, 40, 64): (2, 1, 12, 2, False, 2, [(1, 1, 0)]),
}
for _W, _nrt in ((2, 1), (33, 1), (34, 2), (65, 2), (66, 3)):
    _PLANS[(9, _W, 40, 64)] = (2, 1, 5, 1, _W <= 33, _nrt, [(1, 1, 0)])
    _PLANS[(2565, _W, 40, 64)] = (6, 3, 428, 3, _W <= 33, _nrt, [(1, 1, 0)])
for _N, _ns in ((1, 1), (7, 4), (8, 4), (9, 5)):
    _PLANS[(_N, 10, 88, 256)] = (2, 1, _ns, 2 - _N % 2, True, 1, [(4, 1, 0)])
for _F, _fwd in ((20, [(1, 1, 0)]), (64, [(1, 1, 0)]), (65, [(2, 1, 0)]), (128, [(2, 1, 0)]), (129, [(4, 1, 0)]), (200, [(4, 1, 0)]),
                 (256, [(4, 1, 0)]), (300, [(4, 1, 0), (1, 1, 256)]), (330, [(4, 1, 0), (2, 1, 256)]), (450, [(4, 1, 0), (4, 1, 256)]),
                 (600, [(4, 2, 0), (2, 1, 512)])):
    _PLANS[(37, 7, 52, _F)] = (2, 1, 19, 1, True, 1, _fwd)
for _D in (4, 20, 28, 32, 36, 128, 132, 260):
    _PLANS[(37, 7, _D, 70)] = (2, 1, 19, 1, True, 1, [(2, 1, 0)])


def test_conv_plan_of_every_gpu_case():
    import test_gpu_bf16_frontend as FE
    seen = set()
    for c in FE.CONV_CASES:
        key = (c["N"], c["W"], c["D"], c["F"])
        pl = E.conv_plan(*key)
        assert key in _PLANS, "no pinned plan for %s" % c["id"]
        want = _PLANS[key]
        got = (pl["wins"], pl["npairs"], pl["nsplit"], pl["last"], pl["one_rt"], pl["nrt"], pl["fwd"])
        assert got == want, (c["id"], got, want)
        seen.add(key)
    assert seen == set(_PLANS)
    plans = [E.conv_plan(c["N"], c["W"], c["D"], c["F"]) for c in FE.CONV_CASES]
    # what the file is for: ONE_RT with >= 3 pairs, several row tiles with >= 3 pairs, <4> at a non-zero c_first, <2>, <1>, an odd last split
    assert any(p["one_rt"] and p["npairs"] >= 3 for p in plans) and any(not p["one_rt"] and p["npairs"] >= 3 for p in plans)
    assert any((4, 1, 256) in p["fwd"] for p in plans) and any(p["fwd"] == [(4, 1, 0)] for p in plans)
    assert any(ct == 2 for p in plans for ct, _, _ in p["fwd"]) and any(ct == 1 for p in plans for ct, _, _ in p["fwd"])
    assert any(p["last"] == 1 and p["wins"] > 2 for p in plans) and any(p["last"] == 3 for p in plans)
    for mod, Fo, B, T in FE.CHAIN_CASES:
        pl = E.conv_plan(B * T, R.FE_WINDOW[mod], R.FE_DIMS[mod], Fo)
        assert pl["one_rt"] and pl["npairs"] >= 3, (mod, Fo, pl)


def test_conv_tie_cases_tie_in_the_reference():
    """The constructed ties of test_gpu_bf16_frontend.py are exact in the reference too: bit-identical sums at the tied positions, the
    first of them the argmax, and the tied pair the maximum of a useful number of (window, channel) pairs."""
    import test_gpu_bf16_frontend as FE
    for c in FE.CONV_CASES:
        if not c["kind"].startswith("tie"):
            continue
        x, w, b, g = FE.conv_inputs(c)
        S, _ = E.conv_sums(x.double(), w.double())
        arg = S.argmax(dim=1)
        if c["kind"] == "tie_const":
            assert bool((S == S[:, :1]).all()) and int(arg.max()) == 0
        elif c["kind"] == "tie_pad":
            W = c["W"]
            assert bool((S[:, W - 2] == 0).all())
            n = int((arg == W - 2).sum())
            print("%s: the zero sum of the last position is the maximum of %d pairs" % (c["id"], n))
            assert n == arg.numel()
        else:
            for res, (p, q) in FE.tie_positions(c).items():
                assert torch.equal(S[res::2, p], S[res::2, q])
                n = int((arg[res::2] == p).sum())
                print("%s: windows %d mod 2, positions %d = %d are the maximum of %d pairs" % (c["id"], res, p, q, n))
                assert n > 100 and int((arg[res::2] == q).sum()) == 0


def _hw_run(rows, n, tag, proj_act=0, drop=None, **kw):
    import test_gpu_bf16_frontend as FE
    *args, g = FE.hw_inputs(rows, n, tag)
    ld = [t.double().requires_grad_() for t in args]
    y = E.highway(*ld, drop=drop, proj_act=proj_act, **kw)
    y.backward(g.double())
    return [y.detach()] + [t.grad for t in ld]


def test_frontend_jitter_floor():
    """The floor of the bounds in test_gpu_bf16_frontend.py: what fp32-level noise (half an fp32 ulp before every bf16 rounding; on the
    conv's sums the random-walk size of a 2D-term fp32 accumulation, see bf16_ref.conv_maxpool) does to the reference itself.
    The conv's argmax must change in at most ARG_SHARE of the pairs for the file's own inputs (per case and over the file): that is the
    condition under which the cap holds.  The Highway's, the tanh / sigmoid map's and the chain's measures must stay within the bounds."""
    import test_gpu_bf16_frontend as FE
    t0 = time.time()
    nd = tot = 0
    for c in FE.CONV_CASES:
        if c["kind"].startswith("tie"):
            continue
        x, w, b, g = FE.conv_inputs(c)
        _, a0, _ = E.conv_maxpool(x.double(), w.double(), b.double())
        with E.jitter(6e-8, 1):
            _, a1, _ = E.conv_maxpool(x.double(), w.double(), b.double())
        d = int((a0 != a1).sum())
        print("jitter floor conv %-34s argmax changes in %d of %d pairs (%.1e)" % (c["id"], d, a0.numel(), d / a0.numel()))
        assert d <= max(FE.ARG_SHARE * a0.numel(), 0 if a0.numel() >= 10000 else 1), c["id"]
        nd, tot = nd + d, tot + a0.numel()
    print("jitter floor conv: %d of %d pairs over the file (%.1e)" % (nd, tot, nd / tot))
    assert nd <= FE.ARG_SHARE * tot
    for rows, n in ((3001, 256), (600, 300), (500, 20)):
        for proj_act in (0, 1):
            a = _hw_run(rows, n, "bffe_hw%dx%d" % (rows, n), proj_act)
            with E.jitter(6e-8, 1, inputs=False):              # stand-alone: x and the weights are given data
                b_ = _hw_run(rows, n, "bffe_hw%dx%d" % (rows, n), proj_act)
            for k, u, v in zip(("y",) + FE.HW_NAMES, b_, a):
                rel, row = measures(u.numpy(), v.numpy())
                print("jitter floor highway %dx%d a%d %-4s rel-L2 %.2e  row-max %.2e" % (rows, n, proj_act, k, rel, row))
                bd = FE.HW_OUT if k == "y" else FE.HW_GRAD
                assert rel <= bd[0] and row <= bd[1], (rows, n, k)
            for i in (2, 4):
                assert abs(ls_scale(b_[i].numpy(), a[i].numpy())) <= FE.HW_W_SCALE
    M, K, N = 200, 576, 129
    x, W, b, g = FE._lin_inputs(M, K, N, "bffe_lin%dx%dx%d" % (M, K, N))
    for act in (2, 3):
        res = []
        for jit in (False, True):
            ld = [t.double().requires_grad_() for t in (x, W, b)]
            if jit:
                with E.jitter(6e-8, 1, inputs=False):
                    y = E.linear(*ld, act=act)
                    y.backward(g.double())
            else:
                y = E.linear(*ld, act=act)
                y.backward(g.double())
            res.append([y.detach()] + [t.grad for t in ld])
        for k, u, v in zip(("y", "dx", "dW", "db"), res[1], res[0]):
            rel, row = measures(u.numpy(), v.numpy())
            print("jitter floor linear act %d %-3s rel-L2 %.2e  row-max %.2e" % (act, k, rel, row))
            bd = FE.LIN_ACT_OUT if k == "y" else FE.LIN_ACT_GRAD
            assert rel <= bd[0] and row <= bd[1], (act, k)
    mod, Fo, B, T = "acoustic", 88, 5, 513
    p32 = _chain_params(mod, Fo, R.FE_DIMS[mod], 37)
    x = R.gen_normal("bffe_chain:%s%d:x" % (mod, Fo), (B, T, R.FE_WINDOW[mod], R.FE_DIMS[mod]), 37)
    g = R.gen_normal("bffe_chain:%s%d:g" % (mod, Fo), (B, T, Fo), 37)
    res = []
    for jit in (False, True):
        pd = {k: v.double().requires_grad_() for k, v in p32.items()}
        if jit:
            with E.jitter(6e-8, 1):
                y, arg = E.window_encoder(pd, mod, x.double(), arg=res[0][1])
                y.backward(g.double())
        else:
            y, arg = E.window_encoder(pd, mod, x.double())
            y.backward(g.double())
        res.append((y.detach(), arg, {k: v.grad.reshape(v.shape[0], -1) if v.dim() == 3 else v.grad for k, v in pd.items()}))
    rel, row = measures(res[1][0].numpy(), res[0][0].numpy())
    print("jitter floor chain %s%d y rel-L2 %.2e  row-max %.2e" % (mod, Fo, rel, row))
    assert rel <= FE.CHAIN_OUT[0] and row <= FE.CHAIN_OUT[1]
    for k in res[0][2]:
        rel, row = measures(res[1][2][k].numpy(), res[0][2][k].numpy())
        print("jitter floor chain %s%d %-40s rel-L2 %.2e  row-max %.2e" % (mod, Fo, k, rel, row))
        assert rel <= FE.CHAIN_GRAD[0] and row <= FE.CHAIN_GRAD[1], k
    print("%.1f s" % (time.time() - t0))


# Mutations of the front-end reference, each a subtle kernel bug: each must fail what test_gpu_bf16_frontend.py asserts.
def _keep_value(value, grad_path):
    """the value of `value` with the gradient of `grad_path`"""
    return value.detach() + (grad_path - grad_path.detach())


def _conv_mutant_inputs(N, W, D, F, tag):
    return _conv_small(N, W, D, F, "e_cmut_" + tag)


def test_conv_bounds_see_the_pool_mutants():
    import test_gpu_bf16_frontend as FE
    # the LAST instead of the first maximum: invisible to the near-tie rule (the gap is exactly 0), seen by the exact-tie cases
    c = dict(next(x for x in FE.CONV_CASES if x["kind"] == "tie_d4d8"), N=64)
    x, w, b, g = FE.conv_inputs(c)
    last = lambda S: S.shape[1] - 1 - S.flip(1).argmax(dim=1)  # noqa: E731
    ref = _run_conv(x, w, b, g)
    mut = _run_conv(x, w, b, g, mutate={"pool": last})
    run = {"S": ref["S"], "A": E.conv_sums(x.double(), w.double())[1], "arg": mut["arg"]}
    nd, worst = FE.arg_differences(c, run)
    print("mutant last maximum: argmax differs in %d pairs, gap / slack %.1e" % (nd, worst))
    assert nd > 100 and worst == 0.0                       # a tie case fails on any difference
    # one position too many in the last row tile (row <= plim): the padding row's sum x[W-1] . w[:, :, 0] takes part in the pool
    for key in ((2565, 10, 88, 256), (9, 34, 40, 64)):
        c = next(x for x in FE.CONV_CASES if (x["N"], x["W"], x["D"], x["F"]) == key and x["kind"] in ("neg", "rt"))
        x, w, b, g = FE.conv_inputs(c)
        x, g = x[:300], g[:300]
        wl = w.double()
        S = torch.cat([E.conv_sums(x.double(), wl)[0], (E.bf16(x.double())[:, -1] @ E.bf16(wl)[:, :, 0].t()).unsqueeze(1)], dim=1)
        arg = S.argmax(dim=1)
        rel, row = measures((S.amax(dim=1)).numpy(), S[:, :-1].amax(dim=1).numpy())
        print("mutant row <= plim %s: argmax = W - 1 in %d pairs, out rel-L2 %.2e row-max %.2e" % (c["id"], int((arg == c["W"] - 1).sum()), rel, row))
        assert int(arg.max()) == c["W"] - 1 and rel > FE.CONV_OUT[0] and row > FE.CONV_OUT[1]


def test_conv_bounds_see_the_backward_mutants():
    import test_gpu_bf16_frontend as FE
    N, W, D, F = 3001, 10, 88, 256
    pl = E.conv_plan(N, W, D, F)
    x, w, b, g = _conv_mutant_inputs(N, W, D, F, "bwd")
    ref = _run_conv(x, w, b, g)

    def dist(mut, name):
        a, r = mut[name], ref[name]
        if a.dim() == 3:
            a, r = a.reshape(F, -1), r.reshape(F, -1)
        return measures(a.numpy(), r.numpy()) + (ls_scale(a.numpy(), r.numpy()),)
    # npairs = (nend - nbeg) / 2: the last window of an odd split is left out of dW (its dy still reaches db)
    keep = torch.ones(N, 1, dtype=torch.float64)
    assert pl["last"] % 2 == 1
    keep[N - 1] = 0.0
    m = _run_conv(x, w, b, g, arg=ref["arg"], mutate={"gathered": lambda s: _keep_value(s, s * keep)})
    rel, row, sc = dist(m, "dW")
    print("mutant odd last window dropped: dW rel-L2 %.2e row-max %.2e" % (rel, row))
    assert rel > FE.CONV_DW[0] and row > FE.CONV_DW[1] and torch.equal(m["db"], ref["db"])
    # the previous pair's rows as the B operand of tap 1 (a stale LDS buffer): the forward is untouched
    def stale(j, rows, wj):
        prod = rows @ wj.t()
        return prod if j == 0 else _keep_value(prod, rows.roll(2, dims=0) @ wj.t())
    m = _run_conv(x, w, b, g, arg=ref["arg"], mutate={"tap": stale})
    rel, row, sc = dist(m, "dW")
    print("mutant stale rows for tap 1: dW rel-L2 %.2e row-max %.2e" % (rel, row))
    assert torch.equal(m["out"], ref["out"]) and rel > FE.CONV_DW[0] and row > FE.CONV_DW[1]
    # dy truncated instead of rounded to bf16: a coherent -2^-9-ish scale of dW
    def trunc(t):
        bits = t.float().view(torch.int32) & -65536
        return bits.view(torch.float32).double()
    m = _run_conv(x, w, b, g, arg=ref["arg"], mutate={"round_dy": trunc})
    rel, row, sc = dist(m, "dW")
    print("mutant dy truncated: dW rel-L2 %.2e row-max %.2e scale %.2e" % (rel, row, sc))
    assert rel > FE.CONV_DW[0] and row > FE.CONV_DW[1] and abs(sc) > FE.CONV_W_SCALE
    # db counted once per row tile instead of once per window (first_rt always 1), at three row tiles
    N, W, D, F = 300, 70, 24, 32
    nrt = E.conv_plan(N, W, D, F)["nrt"]
    x, w, b, g = _conv_mutant_inputs(N, W, D, F, "db")
    ref = _run_conv(x, w, b, g)
    m = _run_conv(x, w, b, g, mutate={"b": lambda t: _keep_value(t, nrt * t)})
    rel, row = measures(m["db"].numpy(), ref["db"].numpy())
    print("mutant db once per row tile: db rel-L2 %.2e row-max %.2e" % (rel, row))
    assert nrt == 3 and rel > FE.CONV_DB[0] and row > FE.CONV_DB[1] and torch.equal(m["dW"], ref["dW"])


def test_highway_bounds_see_a_mutant():
    import test_gpu_bf16_frontend as FE
    rows, n = 600, 300
    ref = _hw_run(rows, n, "bffe_hw%dx%d" % (rows, n))
    # dgate = g * proj: the "- x" lost
    m = _hw_run(rows, n, "bffe_hw%dx%d" % (rows, n),
                mutate={"combine": lambda x, proj, gate: _keep_value(x + gate * (proj - x), x + gate.detach() * (proj - x) + gate * proj.detach())})
    assert torch.equal(m[0], ref[0])
    for i, k in ((4, "dWg"), (5, "dbg"), (1, "dx")):
        rel, row = measures(m[i].numpy(), ref[i].numpy())
        print("mutant dgate without - x: %s rel-L2 %.2e row-max %.2e" % (k, rel, row))
        assert rel > FE.HW_GRAD[0] and row > FE.HW_GRAD[1]
    # the sigmoid's derivative from the pre-activation rounded to bf16 instead of from the saved fp32 output
    def gate_act(pre):
        s = torch.sigmoid(E.bf16(pre.detach()))
        return _keep_value(torch.sigmoid(pre), pre * (s * (1 - s)))
    m = _hw_run(rows, n, "bffe_hw%dx%d" % (rows, n), mutate={"gate_act": gate_act})
    assert torch.equal(m[0], ref[0])
    rel, row = measures(m[4].numpy(), ref[4].numpy())
    print("mutant sigmoid' from bf16(pre): dWg rel-L2 %.2e row-max %.2e" % (rel, row))
    assert rel > FE.HW_GRAD[0] or row > FE.HW_GRAD[1]


# ------------------------------------------------------------------------------------------ stacked and feedback LSTM scans
def _nrel(a, b):
    a, b = (np.asarray(x.detach() if torch.is_tensor(x) else x, dtype=np.float64) for x in (a, b))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _stack_plain(inp, w):
    """lstm_stack_ref.forward / backward on a test_gpu_bf16_stack_fb input dict -> the arrays of stack_ref()"""
    import lstm_stack_ref as SR
    n = {k: None if v is None else v.numpy() for k, v in inp.items()}
    h_all, c_all, acts = SR.forward(n["gx0"], n["P"], n["bias"], n["h0"], n["c0"])
    g = SR.backward(w.numpy(), n["P"], n["h0"], n["c0"], h_all, c_all, acts)
    out = dict(h_top=h_all[-1], h_all=h_all, c_all=c_all, dgx0=g["dgx0"], dP=g["dP"], dbias=g["dbias"])
    if inp["h0"] is not None:
        out["dh0"], out["dc0"] = g["dh0"], g["dc0"]
    return out, g


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("L", [2, 4])
def test_lstm_stack_scan_without_rounding_is_the_plain_reference(L, init):
    import test_gpu_bf16_stack_fb as S
    c = S._sc(5, 3, 40, L, init=init)
    inputs = S.stack_inputs(c)
    a = S.stack_ref(c, inputs, rounding=False)
    b, _ = _stack_plain(*inputs)
    assert set(a) == set(b)
    for k in b:
        assert _nrel(a[k], b[k]) <= 1e-12, k


@pytest.mark.parametrize("init", [False, True])
def test_lstm_fb_scan_without_rounding_is_the_plain_reference(init):
    import lstm_fb_ref as FR
    import test_gpu_bf16_stack_fb as S
    c = S._fc(5, 3, 40, 24, init=init)
    inp, w = S.fb_inputs(c)
    saved = {}
    a = S.fb_ref(c, (inp, w), saved=saved, rounding=False)
    n = {k: None if v is None else v.numpy() for k, v in inp.items()}
    outs = FR.forward(**n, p_init=S.P_INIT)
    g = FR.backward(w.numpy(), n["w_p"], n["W_hh"], n["W1"], n["w2"], n["h0"], n["c0"], S.P_INIT, *outs)
    b = dict(zip(("p_all", "h_all", "c_all", "acts", "u_all"), outs))
    for k in ("p_all", "h_all", "c_all", "u_all"):
        assert _nrel(a[k], b[k]) <= 1e-12, k
    for k in S.FB_KEYS:
        if n[k] is not None:
            assert _nrel(a["d" + k], g["d" + k].reshape(a["d" + k].shape)) <= 1e-12, k
    assert "dh0" in a or not init
    gr = saved["grads"]()                               # what the C entry point's buffers are compared with
    assert _nrel(saved["acts"], b["acts"]) <= 1e-12
    for k, r in (("dG", g["dgxc"]), ("du", g["du"]), ("dp", g["dp"])):
        assert _nrel(gr[k], r) <= 1e-12, k


def test_lstm_stack_ref_bf16_mode_leaves_the_batched_gradients_unrounded():
    """lstm_stack_ref's own bf16=True mode rounds inside the recurrence only: forward, dgx0, dh0, dc0 agree with bf16_ref, dP and dbias
    (batched from the unrounded dG and states) do not."""
    import lstm_stack_ref as SR
    import test_gpu_bf16_stack_fb as S
    c = S._sc(13, 3, 40, 3)
    inp, w = S.stack_inputs(c)
    a = S.stack_ref(c, (inp, w))
    n = {k: v.numpy() for k, v in inp.items()}
    h_all, c_all, acts = SR.forward(n["gx0"], n["P"], n["bias"], n["h0"], n["c0"], bf16=True)
    g = SR.backward(w.numpy(), n["P"], n["h0"], n["c0"], h_all, c_all, acts, bf16=True)
    assert _nrel(h_all, a["h_all"]) <= 1e-12 and _nrel(c_all, a["c_all"]) <= 1e-12
    for k in ("dgx0", "dh0", "dc0"):
        assert _nrel(g[k], a[k]) <= 1e-12, k
    print("lstm_stack_ref bf16=True against bf16_ref: dP %.2e, dbias %.2e" % (_nrel(g["dP"], a["dP"]), _nrel(g["dbias"], a["dbias"])))
    assert _nrel(g["dP"], a["dP"]) > 1e-4 and _nrel(g["dbias"], a["dbias"]) > 1e-4


def _largest(cases, S):
    """per tier: the largest case (elements of the state tensor), the longest if it is another one, and the saturated runs"""
    out = []
    for t in ("short", "wide", "long"):
        cs = [c for c in cases if S.tier(c) == t]
        if not cs:
            continue
        if t == "long":                                 # the long tier: every case
            out += cs
            continue
        size = lambda c: c["T"] * c["B"] * c["H"] * c.get("L", 1) * c.get("E", 1)      # noqa: E731
        big, lng = max(cs, key=size), max(cs, key=lambda c: (c["T"], size(c)))
        out += [big] if big is lng else [big, lng]
    return out + [c for c in cases if c.get("gs", 1.0) != 1.0]                         # and the saturated runs


def _fb_with_buffers(S, c, **kw):
    saved = {}
    a = S.fb_ref(c, saved=saved, **kw)
    return a, {k: v.numpy() for k, v in saved["grads"]().items()}


def test_stack_fb_jitter_floor():
    """The floor of every bound in test_gpu_bf16_stack_fb.py: how far fp32-level noise (half an fp32 ulp before every bf16 rounding)
    moves the reference from itself, at the largest and at the longest case of every tier, on every measure that file applies.  Every
    bound there must sit at or above this floor; a per-row bound of None must be explained by it."""
    import test_gpu_bf16_stack_fb as S
    t0 = time.time()
    bad = []

    def floor(kind, c, a, b):
        for name, group, measure, v in S.figures(kind, b, a):
            bd = S.bound_of(kind, c, group, measure)
            print("jitter floor %-6s %-5s %-28s %-8s %-5s %.2e (bound %s)" % (kind, S.tier(c), c["id"], name, measure, v,
                                                                             "None" if bd is None else "%.1e" % bd))
            if bd is not None and v > bd:
                bad.append((c["id"], name, measure, v, bd))
    for c in _largest(S.STACK_CASES, S):
        a = S.stack_ref(c)
        with E.jitter(6e-8, 1):
            b = S.stack_ref(c)
        floor("stack", c, a, b)
    for c in _largest(S.FB_CASES, S):
        a = S.fb_ref(c)
        with E.jitter(6e-8, 1):
            b = S.fb_ref(c)
        floor("fb", c, a, b)
    for c in _largest(S.FB_BWD_CASES, S):               # the C entry point's buffers, at the cases that read them
        _, ga = _fb_with_buffers(S, c)
        with E.jitter(6e-8, 1):
            _, gb = _fb_with_buffers(S, c)
        floor("fb_bwd", c, ga, gb)
    print("%.1f s" % (time.time() - t0))
    assert not bad, bad


# Mutations of the two references, each a subtle kernel bug (the sizes to see: single-step faults, a 5 % bias error): each must exceed
# the bound test_gpu_bf16_stack_fb.py applies to its tier on the named tensor and measure.
_MT, _MB = 7, 1                                        # the step and the sequence of the single-step mutants


def _sm_stale_o(lv):
    hist = {}

    def xa(t, l, x):                                    # sequence _MB's layer 0 reads o_{t-2} at step _MT
        if l == 0:
            hist[t] = x
            if t == _MT:
                x = x.clone()
                x[_MB] = hist[t - 1][_MB]
        return x
    return {"xa": xa}


def _sm_drop_feedback_grad(lv):
    def xa(t, l, x):                                    # the gradient through o_{_MT-1} into the top layer is dropped for sequence _MB
        if l == 0 and t == _MT:
            x = torch.cat([x[:_MB], x[_MB:_MB + 1].detach(), x[_MB + 1:]])
        return x
    return {"xa": xa}


def _sm_ragged_bias(lv):
    L, H = lv["P"].shape[0], lv["P"].shape[2] // 2
    last = (H - 1) // 16 * 16                           # the last, ragged 16-unit tile of the top layer: its bias x 1.05

    def bias(l, b):
        if l != L - 1:
            return b
        s = torch.ones_like(b)
        for q in range(4):
            s[q * H + last:(q + 1) * H] = 1.05
        return b * s
    return {"bias": bias}


def _sm_wrong_half(lv):
    hist = {}

    def xb(t, l, x):
        hist[t, l] = x                                  # h^l_{t-1}
        return x

    def xa(t, l, x):                                    # layer 1 reads h^0_{t-1} instead of h^0_t at step _MT: the other half of the buffer
        return hist[t, 0] if (l == 1 and t == _MT) else x
    return {"xa": xa, "xb": xb}


def _sm_o_init(lv):
    L = lv["P"].shape[0]
    return {"xa": lambda t, l, x: lv["h0"][L - 1] if (t == 0 and l == 0) else x}     # o_{-1} = h0[L-1] instead of zeros


def _sm_dbias_unrounded(lv):
    return {"pre": lambda t, l, prod, b: E.round_bwd(prod) + b}                        # dbias summed from the unrounded dG


def _fm_stale_p(lv):
    hist = {}

    def p(t, x):                                        # sequence _MB is fed p_{t-2} at step _MT
        hist[t] = x
        if t == _MT:
            x = torch.cat([x[:_MB], hist[t - 1][_MB:_MB + 1], x[_MB + 1:]])
        return x
    return {"p": p}


def _fm_stale_mask(lv):
    hist = {}

    def mask(t, mk):                                    # the backward of step _MT takes the ReLU mask of u_{t-1}
        hist[t] = mk
        return hist[t - 1] if t == _MT else mk
    return {"mask": mask}


def _fm_no_wp_term(lv):
    return {"p": lambda t, x: x.detach() if t == _MT + 1 else x}                       # dp_{_MT} without dG_{_MT+1} . w_p


def _fm_db2_unrounded(lv):
    def readout(t, u, w2, b2):
        return E.fb_readout(u, w2, b2.detach()) + (b2 - b2.detach())
    return {"readout": readout}


def _fm_last_tile(inputs):
    """w2 . u without the rows of the last read-out tile: an input edit (rows >= 16 floor((E-1)/16) of w2 scaled by 0)"""
    inp, w = inputs
    E_ = inp["w2"].numel()
    w2 = inp["w2"].clone()
    w2[(E_ - 1) // 16 * 16:] = 0.0
    return dict(inp, w2=w2), w


# (name, kind, case, hooks from the leaves or None, input edit or None, tensor, measure)
def _stack_fb_mutants():
    import test_gpu_bf16_stack_fb as S
    s, f = S._sc(13, 3, 40, 3), S._fc(13, 3, 40, 24)
    return [("stale_o", "stack", s, _sm_stale_o, None, "h_all", "row"),
            ("drop_feedback_grad", "stack", s, _sm_drop_feedback_grad, None, "dP0.xb", "scale"),
            ("ragged_tile_bias", "stack", s, _sm_ragged_bias, None, "h_top", "rel"),
            ("wrong_buffer_half", "stack", s, _sm_wrong_half, None, "h_all", "row"),
            ("o_init_h0_top", "stack", s, _sm_o_init, None, "h_top", "row"),
            ("dbias_unrounded", "stack", s, _sm_dbias_unrounded, None, "dbias", "row"),
            ("stale_p", "fb", f, _fm_stale_p, None, "h_all", "row"),
            ("stale_relu_mask", "fb", f, _fm_stale_mask, None, "dgxc", "row"),
            ("last_readout_tile", "fb", f, None, _fm_last_tile, "p_all", "rel"),
            ("dp_without_wp_term", "fb", f, _fm_no_wp_term, None, "dgxc", "row"),
            ("db2_unrounded", "fb", f, _fm_db2_unrounded, None, "db2", "row")]


@pytest.mark.parametrize("i", range(11))
def test_stack_fb_bounds_see_a_mutant(i):
    import test_gpu_bf16_stack_fb as S
    name, kind, c, hooks, edit, tensor, measure = _stack_fb_mutants()[i]
    run = S.stack_ref if kind == "stack" else S.fb_ref
    inputs = (S.stack_inputs if kind == "stack" else S.fb_inputs)(c)
    ref = run(c, inputs)
    got = run(c, edit(inputs) if edit else inputs, mutate=hooks)
    figs = S.figures(kind, got, ref)
    v, bd = next((v, S.bound_of(kind, c, g, m)) for n, g, m, v in figs if n == tensor and m == measure)
    print("mutant %s (%s, tier %s): %s %s %.3e (bound %.1e)" % (name, c["id"], S.tier(c), tensor, measure, v, bd))
    assert v > bd
