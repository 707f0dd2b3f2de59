"""The K-tap window encoder (csrc/convk.h, functional.conv_maxpool_k, models.CNN with k in 1..5) against the bf16-faithful fp64
reference tests/convk_ref.py, against the reference fixtures of tests/golden/make_golden_cnn_k.py, and its refusals.

Per case, as test_gpu_bf16_frontend.py does for the 2-tap kernels:
  * `out`, dW (for the kernel's own argmax) and db at fp32 level, per tensor and per row, and dW's least-squares scale;
  * 0 <= argmax <= W - K, and the argmax EQUALS the reference's except at provable near-ties: where it differs, the reference's two sums
    are closer than  slack = 2 * (K D) * 2^-24 * max(sum|x w|), and at most ARG_SHARE of a case's (window, channel) pairs differ (a
    condition, not a measurement; cases with fewer than 1 / ARG_SHARE pairs allow none);
  * windows with repeated rows give two positions bit-identical operands: there the first maximum must win, index for index (inside a
    lane, across the two lane halves, across row tiles, never a padding position);
  * torch.profiler's kernel names show the planned convk_fwd_kernel<K, CT> / convk_bwd_kernel<ONE_RT> instances (convk_ref.conv_plan;
    tests/test_convk_cpu.py pins the plan of every case) and none of the 2-tap kernels.

Bounds.  NOT YET MEASURED ON THE MI355X: no GPU run of this file has been possible so far, so no worst values stand beside the
constants and no kernel mutant has been run against it.  Until they are, every constant comes from reasoning that is written beside
it: `out` sums K D <= 5000 products in fp32, and its bound is what the reference moves by under its own jitter of half an fp32 ulp per
term at K D = 5000 (tests/test_convk_cpu.py test_jitter_floor), times 1.2; dW and db sum over the N windows, not over K D, in the same
way as the 2-tap kernels (MFMA fp32 accumulation inside a window split, fp32 slab sums in fixed order over at most 428 splits), so they
keep test_gpu_bf16_frontend.py's bounds, which are 4x what that file measured over the same N.  None is above the plain-fp64 bounds of
test_gpu_frontend.py (2e-2 out, 1e-2 dW for the own argmax, 1e-5 db).  The first GPU run has to replace them by 4x its worst values,
floored as above, and to run the value-only mutants (swapped taps in convk_prep_kernel, the last halo row staged as zero, the later
position winning the cross-half tie, one slab scaled by 1.01, the backward's tap offset dropped).
"""
import re

import numpy as np
import pytest
import torch

import convk_ref as E
import oracle
import recipe as R
from conftest import load_golden, rel_l2
from gpu_harness import (GRAD_RTOL, OUT_RTOL, RELU_GRAD_RTOL, check, dev, device_kernel_names, library_kernels, load_named,  # noqa: F401
                         ls_scale, measures)

pytestmark = pytest.mark.gpu

CONV_OUT = (2.5e-6, 2.8e-6)            # the reference under jitter: 2.07e-6 / 2.34e-6 at K D = 5000 (many_k5_N331_W30_D1000_F256), x 1.2
CONV_DW = (1.6e-6, 3.2e-6)             # test_gpu_bf16_frontend.CONV_DW: sums over N, for the kernel's own argmax
CONV_DB = (2e-6, 1.3e-5)               # test_gpu_bf16_frontend.CONV_DB: 99 to 428 split partials summed in fp32
CONV_W_SCALE = 1.2e-7                  # test_gpu_bf16_frontend.CONV_W_SCALE
ARG_SHARE = 1e-4                       # a condition set with the feature, not a measurement

MANY_N = 2565


def _case(kind, K, N, W, D, F):
    return {"id": "%s_k%d_N%d_W%d_D%d_F%d" % (kind, K, N, W, D, F), "kind": kind, "K": K, "N": N, "W": W, "D": D, "F": F}


def _conv_cases():
    cs = [_case("many", K, MANY_N, 10, 88, 256) for K in (1, 3, 4, 5)]
    cs += [_case("many", 3, 331, 30, 1000, 256), _case("many", 5, 331, 30, 1000, 256), _case("many", 4, 600, 33, 300, 300),
           _case("many", 3, 4000, 9, 20, 20)]
    for K in (1, 3, 4, 5):                   # a single conv position: W == K
        cs += [_case("one", K, 9, K, 40, 64), _case("one", K, MANY_N, K, 40, 64)]
    for K, Ws in ((3, (34, 35, 66, 67)), (5, (36, 37))):      # W - K + 1 in {32, 33, 64, 65}: row-tile edges
        for W in Ws:
            cs += [_case("rt", K, 9, W, 40, 64), _case("rt", K, MANY_N, W, 40, 64)]
    cs += [_case("wg", 3, N, 10, 88, 256) for N in (1, 7, 8, 9)]
    cs += [_case("ch", 3, 37, 7, 52, F) for F in (20, 65, 129, 300, 600)]
    cs += [_case("dp", K, 37, 7, D, 70) for K in (3, 5) for D in (4, 28, 36, 132, 260)]
    # exact ties (see tie_positions and conv_inputs)
    cs += [_case("tie_const", 3, 21, 12, 88, 256), _case("tie_const", 5, 21, 40, 40, 64), _case("tie_d4d8", 3, MANY_N, 12, 88, 256),
           _case("tie_d32", 3, 40, 70, 40, 64), _case("tie_d32", 5, 40, 70, 40, 64)]
    for K in (3, 5):                         # the last valid position against the padding behind it: W = K + 1, and in the second row tile
        cs += [_case("tie_pad", K, 24, K + 1, 40, 64), _case("tie_pad", K, 24, K + 33, 40, 64)]
    return cs


CONV_CASES = _conv_cases()


def tie_positions(c):
    """{window residue class: (p, q)}: conv positions p < q of those windows whose K rows are bit-identical copies (q - p >= K)"""
    if c["kind"] == "tie_d4d8":
        return {0: (3, 7), 1: (1, 9)}        # even windows: rows 3 and 7 of a tile live in different lane halves; odd: 1 and 9 in the same
    if c["kind"] == "tie_d32":
        return {0: (2, 34), 1: (2, 34)}      # the same position of two row tiles
    return {}


def conv_inputs(c):
    K, N, W, D, F = c["K"], c["N"], c["W"], c["D"], c["F"]
    tag, kind = "convk:k%d_N%d_W%d_D%d_F%d" % (K, N, W, D, F), c["kind"]
    if kind.startswith("tie"):
        tag = "convk:" + c["id"]
    x = R.gen_normal(tag + "x", (N, W, D), 29)
    w = R.gen_normal(tag + "w", (F, D, K), 29) / np.sqrt(K * D)
    b = 0.1 * R.gen_normal(tag + "b", (F,), 29)
    g = R.gen_normal(tag + "g", (N, F), 29)
    if kind == "tie_const":                  # every position ties: the answer is 0
        x = x[:, :1].expand(N, W, D).contiguous()
    elif kind in ("tie_d4d8", "tie_d32"):
        for res, (p, q) in tie_positions(c).items():
            x[res::2, p:p + K] *= 2.0        # twice the spread: the tied pair is the maximum of many channels
            x[res::2, q:q + K] = x[res::2, p:p + K]
    elif kind == "tie_pad":                  # the last valid position and the padding behind it all sum to exactly 0, every other
        x, w = x.abs(), -w.abs()             # sum is negative: the answer is W - K
        x[:, W - K:] = 0.0
    return x, w, b, g


_FWD = re.compile(r"convk_fwd_kernel<\s*(\d+)\s*,\s*(\d+)\s*>")
_BWD = re.compile(r"convk_bwd_kernel<\s*(\w+)\s*>")


def check_convk_ran(tag, names, plan):
    if names is None:
        return                               # the profiler reports no device kernels on this box: only this assertion is skipped
    fwd = sorted((int(m.group(1)), int(m.group(2))) for m in map(_FWD.search, names) if m)
    bwd = [m.group(1) in ("true", "1") for m in map(_BWD.search, names) if m]
    print("%-52s ran convk_fwd_kernel%s, convk_bwd_kernel<%s>" % (tag, fwd, bwd))
    assert fwd == sorted((k, ct) for k, ct, _, _ in plan["fwd"]), "%s: forward instances %s, planned %s" % (tag, fwd, plan["fwd"])
    assert bwd == [plan["one_rt"]], "%s: backward instances %s, planned ONE_RT = %s" % (tag, bwd, plan["one_rt"])
    two_tap = [n for n in names if "convpool_" in n]
    assert not two_tap, "%s: 2-tap kernels ran: %s" % (tag, two_tap)


_CONV_RUNS = {}


def conv_run(c, dev):
    """One forward + backward of case c on the GPU and the reference's sums (cached: the file-level share reads every case)"""
    if c["id"] in _CONV_RUNS:
        return _CONV_RUNS[c["id"]]
    import multimodal_transformer_amd.functional as F
    x, w, b, g = conv_inputs(c)
    wd, bd = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    xg, gg = x.to(dev), g.to(dev)

    def step():
        out, arg = F.conv_maxpool_k(xg, wd, bd)
        out.backward(gg)
        return out.detach(), arg
    (out, arg), names = device_kernel_names(step)
    F.check_device_errors()
    S, A = E.conv_sums(x.double(), w.double())
    _CONV_RUNS[c["id"]] = {"out": out.cpu(), "arg": arg.cpu().long(), "dW": wd.grad.cpu(), "db": bd.grad.cpu(), "names": names, "S": S,
                           "A": A, "inputs": (x, w, b, g)}
    return _CONV_RUNS[c["id"]]


def arg_differences(c, run):
    """(number of (window, channel) pairs whose argmax differs from the reference's, the worst gap / slack among them)"""
    S, A, arg = run["S"], run["A"], run["arg"]
    ref = S.argmax(dim=1)
    diff = arg != ref
    if not bool(diff.any()):
        return 0, 0.0
    arg = arg.clamp(0, S.shape[1] - 1)       # an index outside the positions fails its own assertion; here it must not fault the gather
    pick = lambda T, a: T.gather(1, a.unsqueeze(1)).squeeze(1)  # noqa: E731
    gap = pick(S, ref) - pick(S, arg)
    slack = 2 * (c["K"] * c["D"]) * 2.0 ** -24 * torch.maximum(pick(A, ref), pick(A, arg))
    return int(diff.sum()), float((gap[diff] / slack[diff]).max())


@pytest.mark.parametrize("c", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_conv_maxpool_k(dev, c):
    run = conv_run(c, dev)
    K, N, W, D, F = c["K"], c["N"], c["W"], c["D"], c["F"]
    plan = E.conv_plan(N, W, D, F, K)
    tag = "convk %s" % c["id"]
    print("%-52s plan %s" % (tag, plan))
    check_convk_ran(tag, run["names"], plan)
    x, w, b, g = run["inputs"]
    S, arg = run["S"], run["arg"]
    failures = []
    ref_arg = S.argmax(dim=1)
    check(tag + " out", run["out"], S.amax(dim=1) + b.double(), *CONV_OUT, failures=failures)
    assert int(arg.min()) >= 0 and int(arg.max()) <= W - K, "%s: argmax outside [0, %d]" % (tag, W - K)
    nd, worst = arg_differences(c, run)
    print("%-52s argmax differs in %d of %d pairs (share %.2e), worst gap / slack %.2e" % (tag, nd, N * F, nd / (N * F), worst))
    if c["kind"].startswith("tie"):
        for res, (p, q) in tie_positions(c).items():
            assert torch.equal(S[res::2, p], S[res::2, q]), "the reference's own sums at the tied positions differ"
            print("%-52s windows %d mod 2: positions %d = %d tie, the maximum of %d pairs" % (tag, res, p, q, int((ref_arg[res::2] == p).sum())))
        if c["kind"] == "tie_const":
            assert int(ref_arg.max()) == 0
        if c["kind"] == "tie_pad":
            assert bool((ref_arg == W - K).all())
        if nd:
            failures.append("%s: argmax differs from the first maximum in %d pairs, e.g. kernel %s reference %s"
                            % (tag, nd, arg[arg != ref_arg][:8].tolist(), ref_arg[arg != ref_arg][:8].tolist()))
    else:
        if worst > 1.0:
            failures.append("%s: an argmax differs beyond the fp32 dot-product bound (gap / slack %.3e)" % (tag, worst))
        if nd > ARG_SHARE * N * F:
            failures.append("%s: argmax differs in %d of %d pairs (> %.0e)" % (tag, nd, N * F, ARG_SHARE))
    # gradients: the reference's for the kernel's own argmax
    wl, bl = w.double().requires_grad_(), b.double().requires_grad_()
    out_r, _, _ = E.conv_maxpool(x.double(), wl, bl, arg=arg)
    out_r.backward(g.double())
    dW, dWr = run["dW"].reshape(F, D * K).double().numpy(), wl.grad.reshape(F, D * K).numpy()
    if np.abs(dWr).max() > 0:
        check(tag + " dW (own argmax)", dW, dWr, *CONV_DW, failures=failures)
        s = ls_scale(dW, dWr)
        print("%-52s scale %.2e" % (tag + " dW", s))
        if abs(s) > CONV_W_SCALE:
            failures.append("%s dW: least-squares scale %.3e > %.1e" % (tag, s, CONV_W_SCALE))
    else:                                    # tie_pad: every row at the argmax is zeros, dW is exactly 0
        assert c["kind"] == "tie_pad"
        if np.abs(dW).max() != 0:
            failures.append("%s dW: not exactly zero" % tag)
    check(tag + " db", run["db"], bl.grad, *CONV_DB, failures=failures)
    assert not failures, "\n".join(failures)


def test_conv_argmax_share_over_the_file(dev):
    """over every case without constructed ties: at most ARG_SHARE of all (window, channel) pairs differ from the reference's argmax"""
    nd = tot = 0
    for c in CONV_CASES:
        if not c["kind"].startswith("tie"):
            nd += arg_differences(c, conv_run(c, dev))[0]
            tot += c["N"] * c["F"]
    print("convk: argmax differs in %d of %d pairs over the file (share %.2e)" % (nd, tot, nd / tot))
    assert nd <= ARG_SHARE * tot


def _step(F, fn, x, w, b, g):
    wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
    out, arg = fn(x, wl, bl)
    out.backward(g)
    return out.detach(), arg, wl.grad, bl.grad


def test_k2_is_the_two_tap_path(dev):
    """conv_maxpool_k at K = 2 is conv_maxpool: the same kernels, the same bits"""
    import multimodal_transformer_amd.functional as F
    N, W, D, Fo = 21, 12, 88, 256
    x = R.gen_normal("convk:k2:x", (N, W, D), 29).to(dev)
    w = (R.gen_normal("convk:k2:w", (Fo, D, 2), 29) / np.sqrt(2 * D)).to(dev)
    b, g = R.gen_normal("convk:k2:b", (Fo,), 29).to(dev), R.gen_normal("convk:k2:g", (N, Fo), 29).to(dev)
    for u, v in zip(_step(F, F.conv_maxpool_k, x, w, b, g), _step(F, F.conv_maxpool, x, w, b, g)):
        assert torch.equal(u, v)


def test_conv_maxpool_k_is_per_window_and_repeats(dev):
    """a window's result does not depend on its neighbours or its place in the batch (bit-exact), N not a multiple of 8; two runs of the
    same step give the same bits in out, argmax, dW and db (no atomics)"""
    import multimodal_transformer_amd.functional as F
    K, N, W, D, Fo = 3, 21, 12, 88, 256
    x = R.gen_normal("convk:pw:x", (N, W, D), 3).to(dev)
    w = (R.gen_normal("convk:pw:w", (Fo, D, K), 3) / np.sqrt(K * D)).to(dev)
    b, g = R.gen_normal("convk:pw:b", (Fo,), 3).to(dev), R.gen_normal("convk:pw:g", (N, Fo), 3).to(dev)
    first, second = _step(F, F.conv_maxpool_k, x, w, b, g), _step(F, F.conv_maxpool_k, x, w, b, g)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    out, arg = first[:2]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).to(dev)
    out2, arg2 = F.conv_maxpool_k(x[perm].contiguous(), w, b)
    assert torch.equal(out2, out[perm]) and torch.equal(arg2, arg[perm])
    out3, arg3 = F.conv_maxpool_k(x[5:6].contiguous(), w, b)
    assert torch.equal(out3[0], out[5]) and torch.equal(arg3[0], arg[5])


def test_refusals(dev):
    import multimodal_transformer_amd.functional as F
    from multimodal_transformer_amd import models as M
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(RuntimeError, match="kernel size"):
        F.conv_maxpool_k(z(3, 8, 16), z(8, 16, 6), z(8))
    with pytest.raises(RuntimeError):
        F.conv_maxpool_k(z(3, 2, 16), z(8, 16, 3), z(8))                                           # W < K
    with pytest.raises(RuntimeError):
        F.conv_maxpool_k(torch.zeros(3, 5, 16), torch.zeros(8, 16, 3), torch.zeros(8))             # CPU tensors
    with pytest.raises(NotImplementedError):
        F.conv_maxpool_k(z(3, 5, 16).requires_grad_(), z(8, 16, 3), z(8))
    with pytest.raises(NotImplementedError):
        M.CNN(16, 8, 6).to(dev).forward_windows(z(3, 8, 16))
    out = M.CNN(16, 8, 3).to(dev).forward_windows(z(3, 8, 16))
    assert out.shape == (3, 8)


# ------------------------------------------------------------------------------------------------ the reference's fixtures
CNN_K_SHAPE = (88, 256, 10, 12)              # (D, F, W, N) of tests/golden/make_golden_cnn_k.py


@pytest.mark.parametrize("K", [1, 3, 4, 5])
def test_cnn_fixture(dev, K):
    """fe_cnn_k<K>.npz at the tolerances of test_gpu_frontend.test_conv_maxpool"""
    from multimodal_transformer_amd import models as M
    D, Fo, W, N = CNN_K_SHAPE
    name = "fe_cnn_k%d" % K
    fx = load_golden(name)
    cnn = M.CNN(D, Fo, K)
    p32 = load_named(cnn)
    assert abs(R.weights_checksum(p32) - float(fx["checksum"])) <= 1e-6 * float(fx["checksum"]), "state_dict differs from the reference's"
    cnn = cnn.to(dev)
    x = R.gen_normal(name + ":x", (N, W, D), R.SEED)
    g = R.gen_normal(name + ":g", (N, Fo), R.SEED)
    out = cnn(x.permute(0, 2, 1).to(dev))
    (out * g.to(dev)).sum().backward()
    r = rel_l2(out.detach().cpu().numpy(), fx["out"])
    _, ref_arg = oracle.cnn_maxpool(x.double(), p32["conv1d.weight"].double(), p32["conv1d.bias"].double())
    import multimodal_transformer_amd.functional as F
    _, arg = F.conv_maxpool_k(x.to(dev), cnn.conv1d.weight.detach(), cnn.conv1d.bias.detach())
    agree = float((arg.cpu().long() == ref_arg).float().mean())
    print("%-14s out rel_l2 %.3e   argmax agreement %.4f" % (name, r, agree))
    assert r < OUT_RTOL and agree > 0.9
    gwk = cnn.conv1d.weight.grad.cpu().numpy()
    bound = GRAD_RTOL + 1.5 * np.sqrt(2.0 * (1.0 - agree))
    rh, rtl = rel_l2(gwk[:, :8, :], fx["gw_head"]), rel_l2(gwk[:, -8:, :], fx["gw_tail"])
    print("%-14s dW vs reference: head %.3e tail %.3e (bound %.3e from argmax agreement)" % (name, rh, rtl, bound))
    assert rh < bound and rtl < bound
    assert abs(np.sqrt((gwk.astype(np.float64) ** 2).sum()) - float(fx["gw_norm"])) < bound * float(fx["gw_norm"])
    assert rel_l2(cnn.conv1d.bias.grad.cpu().numpy(), fx["gb"]) < 1e-4


def _model(name, dev):
    from multimodal_transformer_amd import models as M
    if name == "fe_model_sft_k3":
        return M.MultiCNNTransformer(R.MODS_AVL, R.FE_DIMS, k=3, device=dev), "fe_model_sft"
    return M.MultiCNNTransformerMFT(R.MODS_AVL, R.FE_DIMS, R.FE_EMBED_MFT, k=5, device=dev), "fe_model_mft"


def _model_inputs(tag, lengths, T, dev):
    B = len(lengths)
    mask = R.prefix_mask(lengths, T)
    inputs = {m: R.gen_normal("%s:%s" % (tag, m), (B, T, R.FE_WINDOW[m], R.FE_DIMS[m]), R.SEED).to(dev) for m in R.MODS_AVL}
    target = (R.gen_uniform(tag + ":target", (B, T, 1), R.SEED) * mask).to(dev)
    return inputs, mask, target


@pytest.mark.parametrize("name", ["fe_model_sft_k3", "fe_model_mft_k5"])
def test_model_fixture(dev, name):
    """whole models at k = 3 / k = 5 against the reference, as test_gpu_frontend.test_multi_cnn_transformer_golden"""
    fx = load_golden(name)
    model, tag = _model(name, dev)
    p32 = load_named(model)
    assert abs(R.weights_checksum(p32) - float(fx["checksum"])) <= 1e-6 * float(fx["checksum"]), "state_dict differs from the reference's"
    model = model.to(dev).eval()
    lengths, T = list(fx["lengths"]), 6
    inputs, mask, target = _model_inputs(tag, lengths, T, dev)
    out = model(inputs, lengths, mask.to(dev))
    loss = ((out - target) ** 2).sum() / float(sum(lengths))
    loss.backward()
    o = out.detach().cpu().numpy()
    r = rel_l2(o, fx["out"])
    print("%-16s valence rel_l2 %.3e  loss %.6f (ref %.6f)" % (name, r, loss.item(), float(fx["loss"])))
    assert o.shape == fx["out"].shape and r < OUT_RTOL
    assert (o[mask.numpy() == 0] == 0).all()
    assert abs(loss.item() - float(fx["loss"])) < 2e-2 * max(abs(float(fx["loss"])), 1e-3)
    floor = 1e-3 * max(float(fx[k]) for k in fx if k.startswith("gnorm:"))
    worst = 0.0
    for n, p in model.named_parameters():
        ref = float(fx["gnorm:" + n])
        if ref < 0:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, n
            continue
        assert p.grad is not None, n
        got = float(p.grad.double().pow(2).sum().sqrt())
        if ref > floor:
            worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= RELU_GRAD_RTOL * ref + floor, (n, got, ref)
    print("%-16s worst |grad-norm| deviation %.3e" % (name, worst))
    for k in fx:
        if k.startswith("grad:"):
            got = dict(model.named_parameters())[k[5:]].grad.cpu().numpy()
            assert rel_l2(got, fx[k]) < RELU_GRAD_RTOL, k


def test_train_step_k3_hand_written_kernels_only_and_repeats(dev):
    """one train-mode step of MultiCNNTransformer(k=3) at the fixture shape: the K-tap kernels run, no library kernel does, and the step
    repeats bit for bit from the same generator state"""
    from multimodal_transformer_amd import functional as F
    model, tag = _model("fe_model_sft_k3", dev)
    load_named(model)
    model = model.to(dev).train()
    lengths, T = [6, 4], 6
    inputs, mask, target = _model_inputs(tag, lengths, T, dev)
    mask = mask.to(dev)
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        out = model(inputs, lengths, mask)
        F.mse_sum_loss_backward(out, target, sum(lengths))
        return out
    step()                                   # first train call: the modules' dropout seed states are created
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        y = step().detach().clone()
        torch.cuda.synchronize()
        runs.append([y] + [p.grad.detach().clone() for p in params if p.grad is not None])
    assert all(torch.isfinite(t).all() for t in runs[0])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(u, v) for u, v in zip(*runs))
    names = device_kernel_names(step)[1]
    if names is None:
        return                               # the profiler reports no device kernels on this box: only the assertions on names are skipped
    assert any("convk_fwd_kernel" in n for n in names) and any("convk_bwd_kernel" in n for n in names)
    assert not [n for n in names if "convpool_" in n]
    assert library_kernels(names) == [], "library kernels in a k = 3 train step: %s" % library_kernels(names)
