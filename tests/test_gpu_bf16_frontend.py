"""The window encoder (csrc/convpool.h, the Highway combine of csrc/glue.h, functional.conv_maxpool / highway / linear_pair and the
tanh / sigmoid epilogues of functional.linear) against the bf16-faithful fp64 reference (tests/bf16_ref.py).

test_gpu_frontend.py checks the same kernels against a plain fp64 reference: 2e-2 on outputs, an argmax agreement of 0.9, 1e-2 on dW
for the kernel's own argmax, 4e-2 on the Highway's gradients, and never more than one window pair per backward workgroup.  Here the
reference rounds x, w and dy where the kernels do, so
  * `out`, dW and db are held at fp32 level, per tensor, per row (a window of `out`, an output channel of dW, an entry of db) and, for
    dW, by its least-squares scale;
  * the argmax must EQUAL the reference's except at provable near-ties: where it differs, the reference's sums at the two positions are
    closer than  slack = 2 * (2D) * 2^-24 * sum|x w|  (the fp32 dot-product bound n u sum|a_i b_i| with n = 2D terms, once for each of
    the two compared sums; the larger sum|x w| of the two positions), and at most ARG_SHARE of a case's (window, channel) pairs differ;
  * windows with repeated rows give two positions bit-identical operands, hence bit-identical sums: there the first maximum must win,
    index for index (inside a lane, across the two lane halves, across row tiles, never a padding row);
  * dW and db are compared with the reference's gradient FOR THE KERNEL'S OWN argmax (the distance to the reference's own choice is
    printed: it is the few near-tie pairs);
  * every case asserts through torch.profiler which convpool_fwd_kernel<CT> instances and which convpool_bwd_kernel<ONE_RT> ran, against
    bf16_ref.conv_plan (tests/test_bf16_ref.py pins the plan of every case, so a case cannot silently stop reaching its branch).
None of api.hip's getenv switches is read on these paths, so everything runs in the pytest process.

Observed on the MI355X: the argmax equalled the reference's in all 6.06 M pairs of the cases without constructed ties, and in the tie cases
the sums at positions with bit-identical operands were bit-identical (the first maximum won everywhere).  Eight value-only kernel mutants,
each built from a scratch copy and run once, all fail this file: the idle LDS buffer read in the backward's MFMA loop (dW 1.1), npairs =
(nend - nbeg) / 2 (dW 1.6e-2), the later position winning the cross-half tie-break (tie_const: 4 for 0), row <= plim (argmax = W - 1),
first_rt always 1 (db x 3 at W = 70), c_first ignored in the remainder launch's bias read (out 2.4e-2 at F = 300), dgate without - x
(Highway dx 0.18), one split's slab scaled by 1.01 in convpool_finish_kernel (dW 4.5e-4).  test_gpu_frontend.py passes the tie-break and
the scaled-slab mutants.  (`op <= bp` in place of `op < bp` in that tie-break changes nothing: the two lane halves never hold the same row.)
"""
import re

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import _LIN, LIN_REL, _lin_inputs, check, dev, device_kernel_names, ls_scale, measures  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

# Bounds: about 4x the worst value measured on the MI355X over every case of this file (in the comments, rel-L2 / per-row maximum), none
# below what fp32-level noise does to the reference itself (tests/test_bf16_ref.py test_frontend_jitter_floor), none above the bound
# test_gpu_frontend.py puts on the same quantity (2e-2 outputs, 1e-2 dW for the own argmax, 1e-5 db, 4e-2 gradients).
CONV_OUT = (1e-6, 1.2e-6)              # 2.5e-7 / 2.8e-7 (D = 1000): fp32 accumulation only
CONV_DW = (1.6e-6, 3.2e-6)             # 4.0e-7 / 7.9e-7, for the kernel's own argmax (which equalled the reference's in every pair measured)
CONV_DB = (2e-6, 1.3e-5)               # 4.5e-7 / 3.2e-6 (an entry against the vector's rms; 428 to 501 split partials summed in fp32)
CONV_W_SCALE = 1.2e-7                  # 2.7e-8
ARG_SHARE = 1e-4                       # set by the issue, not measured: measured 0 of 6.06 M pairs; the reference under noise 2 of 6.06 M
PERM_DW = 7e-6                         # dW 5.2e-7 / 6.7e-7, db 5.0e-7 / 1.7e-6 between a batch and its permutation
LIN_ACT_OUT = (6e-7, 2.2e-6)           # tanh / sigmoid outputs: 1.6e-7 / 5.5e-7
# The backward operand g = bf16(dy * act'(y)) takes act' from the kernel's fp32 y, whose hardware exp2 / reciprocal differ from the
# reference's in the last bits: that tips a bf16 rounding of g now and then, a whole bf16 ulp (2^-8) of that element.  One tipped element
# among the 1000 of the 200 x 5 case is the measured worst, 1.9e-4 / 2.7e-3 (dx: a row has 5 entries); everything larger is <= 6e-6 / 1e-4.
LIN_ACT_GRAD = (8e-4, 1.1e-2)
HW_OUT = (4e-7, 9e-7)                  # 9.7e-8 / 2.2e-7: nothing is rounded between the GEMMs and the combine
HW_GRAD = (3.2e-4, 2.4e-3)             # 8.0e-5 / 5.8e-4 (500 x 20): tipped roundings of dproj and dgate as above; floor 5.3e-5 / 2.5e-4
HW_W_SCALE = 1.5e-5                    # 3.6e-6
# conv -> Highway -> dropout: the Highway's x is now a computed fp32 value, so fp32 noise tips its bf16 rounding too (the reference
# moves itself by 2.9e-5 / 5.3e-4 on y and 1.3e-4 / 4.3e-4 on the gradients under noise of half an fp32 ulp), and the conv's dy is the
# Highway's dx
CHAIN_OUT = (6.5e-5, 2.1e-3)           # 1.6e-5 / 5.2e-4
CHAIN_GRAD = (4.6e-4, 3.4e-3)          # 1.2e-4 / 8.4e-4


# ------------------------------------------------------------------------------------------------ conv cases
MANY_N = 2565                          # at D <= 128, F <= 256: 428 splits of 6 windows (3 pairs per workgroup), the last split 3 windows


def _case(kind, N, W, D, F, note=""):
    return {"id": "%s%s_N%d_W%d_D%d_F%d" % (kind, note, N, W, D, F), "kind": kind, "N": N, "W": W, "D": D, "F": F}


def _conv_cases():
    cs = [_case("many", *s) for s in [(3001, 10, 88, 256), (331, 30, 1000, 256), (600, 33, 300, 300), (4000, 9, 20, 20),
                                      (2100, 70, 24, 32)]]
    for W in (2, 33, 34, 65, 66):
        cs += [_case("rt", 9, W, 40, 64), _case("rt", MANY_N, W, 40, 64)]
    cs += [_case("wg", N, 10, 88, 256) for N in (1, 7, 8, 9)]
    cs += [_case("ch", 37, 7, 52, F) for F in (20, 64, 65, 128, 129, 200, 256, 300, 330, 450, 600)]
    cs += [_case("dp", 37, 7, D, 70) for D in (4, 20, 28, 32, 36, 128, 132, 260)]
    # exact ties (see tie_positions)
    cs += [_case("tie_const", 21, 12, 88, 256), _case("tie_const", 21, 40, 40, 64), _case("tie_d4d8", MANY_N, 12, 88, 256),
           _case("tie_d32", 40, 40, 40, 64), _case("tie_d32", 2100, 70, 24, 32), _case("tie_pad", 24, 3, 40, 64),
           _case("tie_pad", 24, 34, 40, 64)]
    # values: every sum negative (a padding row's 0 would win), a large bias, dy with zeros, of one sign, scaled
    cs += [_case(k, MANY_N, 10, 88, 256) for k in ("neg", "bigbias", "dyzeros", "dysign", "dy1e4", "dy1e-4")]
    return cs


CONV_CASES = _conv_cases()


def tie_positions(c):
    """{window residue class: (p, q)}: conv positions p < q of those windows that are built with bit-identical operands"""
    k, W = c["kind"], c["W"]
    if k == "tie_d4d8":
        return {0: (3, 7), 1: (1, 9)}        # even windows: rows 3 and 7 of a tile live in different lane halves; odd: 1 and 9 in the same
    if k == "tie_d32":
        return {0: (2, 34), 1: (2, 34)}      # the same position of two row tiles
    return {}


def conv_inputs(c):
    tag, k = "bffe:" + c["id"], c["kind"]
    N, W, D, F = c["N"], c["W"], c["D"], c["F"]
    x = R.gen_normal(tag + "x", (N, W, D), 29)
    w = R.gen_normal(tag + "w", (F, D, 2), 29) / np.sqrt(2 * D)
    b = 0.1 * R.gen_normal(tag + "b", (F,), 29)
    g = R.gen_normal(tag + "g", (N, F), 29)
    if k == "tie_const":                     # every position ties: the answer is 0
        x = x[:, :1].expand(N, W, D).contiguous()
    elif k in ("tie_d4d8", "tie_d32"):
        for res, (p, q) in tie_positions(c).items():
            x[res::2, p:p + 2] *= 2.0        # twice the spread: the tied pair is the maximum of many channels
            x[res::2, q:q + 2] = x[res::2, p:p + 2]
    elif k == "tie_pad":                     # the last valid position and the padding rows behind it all sum to exactly 0, and every
        x, w = x.abs(), -w.abs()             # other sum is negative: the answer is W - 2, in the second row tile at W = 34
        x[:, W - 2:] = 0.0
    elif k == "neg":
        x, w = x.abs(), -w.abs()
    elif k == "bigbias":
        b = 1e3 * R.gen_normal(tag + "b", (F,), 29)
    elif k == "dyzeros":
        g = g * (R.gen_uniform(tag + "z", (N, F), 29) > 0.5).float()
    elif k == "dysign":
        g = g.abs()
    elif k == "dy1e4":
        g = g * 1e4
    elif k == "dy1e-4":
        g = g * 1e-4
    return x, w, b, g


_FWD = re.compile(r"convpool_fwd_kernel<\s*(\d+)\s*>")
_BWD = re.compile(r"convpool_bwd_kernel<\s*(\w+)\s*>")


def check_conv_ran(tag, names, plan):
    if names is None:
        return                               # the profiler reports no device kernels on this box: only this assertion is skipped
    fwd = sorted(int(m.group(1)) for m in map(_FWD.search, names) if m)
    bwd = [m.group(1) in ("true", "1") for m in map(_BWD.search, names) if m]
    print("%-52s ran convpool_fwd_kernel<%s>, convpool_bwd_kernel<%s>" % (tag, ">, <".join(map(str, fwd)), bwd))
    assert fwd == sorted(ct for ct, _, _ in plan["fwd"]), "%s: forward instances %s, planned %s" % (tag, fwd, plan["fwd"])
    assert bwd == [plan["one_rt"]], "%s: backward instances %s, planned ONE_RT = %s" % (tag, bwd, plan["one_rt"])


_CONV_RUNS = {}


def conv_run(c, dev):
    """One forward + backward of case c on the GPU and the comparison's raw figures (cached: the file-level share reads every case)"""
    if c["id"] in _CONV_RUNS:
        return _CONV_RUNS[c["id"]]
    import multimodal_transformer_amd.functional as F
    x, w, b, g = conv_inputs(c)
    wd, bd = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    xg, gg = x.to(dev), g.to(dev)

    def step():
        out, arg = F.conv_maxpool(xg, wd, bd)
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
    pick = lambda T, a: T.gather(1, a.unsqueeze(1)).squeeze(1)  # noqa: E731
    gap = pick(S, ref) - pick(S, arg)
    slack = 2 * (2 * c["D"]) * 2.0 ** -24 * torch.maximum(pick(A, ref), pick(A, arg))
    return int(diff.sum()), float((gap[diff] / slack[diff]).max())


@pytest.mark.parametrize("c", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_conv_maxpool(dev, c):
    run = conv_run(c, dev)
    N, W, D, F = c["N"], c["W"], c["D"], c["F"]
    plan = E.conv_plan(N, W, D, F)
    tag = "bf conv %s" % c["id"]
    print("%-52s plan %s" % (tag, plan))
    check_conv_ran(tag, run["names"], plan)
    x, w, b, g = run["inputs"]
    S, arg = run["S"], run["arg"]
    failures = []
    ref_arg = S.argmax(dim=1)
    check(tag + " out", run["out"], S.amax(dim=1) + b.double(), *CONV_OUT, failures=failures)
    assert int(arg.min()) >= 0 and int(arg.max()) <= W - 2, "%s: argmax outside [0, %d]" % (tag, W - 2)
    nd, worst = arg_differences(c, run)
    print("%-52s argmax differs in %d of %d pairs (share %.2e), worst gap / slack %.2e" % (tag, nd, N * F, nd / (N * F), worst))
    if c["kind"].startswith("tie"):
        # bit-identical operands, bit-identical sums: the first maximum, index for index
        ties = tie_positions(c)
        for res, (p, q) in ties.items():
            assert torch.equal(S[res::2, p], S[res::2, q]), "the reference's own sums at the tied positions differ"
            print("%-52s windows %d mod 2: positions %d = %d tie, the maximum of %d pairs" % (tag, res, p, q, int((ref_arg[res::2] == p).sum())))
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
    dW, dWr = run["dW"].reshape(F, 2 * D).double().numpy(), wl.grad.reshape(F, 2 * D).numpy()
    check(tag + " dW (own argmax)", dW, dWr, *CONV_DW, failures=failures)
    s = ls_scale(dW, dWr) if np.abs(dWr).max() > 0 else 0.0        # tie_pad: both rows at the argmax are zeros, dW is exactly 0
    print("%-52s scale %.2e" % (tag + " dW", s))
    if abs(s) > CONV_W_SCALE:
        failures.append("%s dW: least-squares scale %.3e > %.1e" % (tag, s, CONV_W_SCALE))
    check(tag + " db", run["db"], bl.grad, *CONV_DB, failures=failures)
    if nd:
        wl2, bl2 = w.double().requires_grad_(), b.double().requires_grad_()
        E.conv_maxpool(x.double(), wl2, bl2)[0].backward(g.double())
        print("%-52s rel-L2 %.2e" % (tag + " dW vs the reference's own argmax", measures(dW, wl2.grad.reshape(F, 2 * D).numpy())[0]))
    assert not failures, "\n".join(failures)


def test_conv_argmax_share_over_the_file(dev):
    """over every case without constructed ties: at most ARG_SHARE of all (window, channel) pairs differ from the reference's argmax"""
    nd = tot = 0
    for c in CONV_CASES:
        if not c["kind"].startswith("tie"):
            nd += arg_differences(c, conv_run(c, dev))[0]
            tot += c["N"] * c["F"]
    print("bf conv: argmax differs in %d of %d pairs over the file (share %.2e)" % (nd, tot, nd / tot))
    assert nd <= ARG_SHARE * tot


def test_conv_maxpool_is_per_window_at_many_pairs(dev):
    """test_gpu_frontend.test_conv_maxpool_is_per_window at 3 window pairs per backward workgroup: the forward of a permuted batch is the
    permuted forward, bit for bit.  dW sums the same terms, but a permutation moves windows between splits and inside a split, so the
    fp32 sums are formed in another order: equal at fp32 level (rel-L2), not bit for bit."""
    import multimodal_transformer_amd.functional as F
    N, W, D, Fo = 3001, 10, 88, 256
    assert E.conv_plan(N, W, D, Fo)["npairs"] == 3
    x = R.gen_normal("bffe:perm:x", (N, W, D), 29).to(dev)
    w = (R.gen_normal("bffe:perm:w", (Fo, D, 2), 29) / np.sqrt(2 * D)).to(dev)
    b = R.gen_normal("bffe:perm:b", (Fo,), 29).to(dev)
    g = R.gen_normal("bffe:perm:g", (N, Fo), 29).to(dev)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).to(dev)
    res = []
    for xi, gi in ((x, g), (x[perm].contiguous(), g[perm].contiguous())):
        wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
        out, arg = F.conv_maxpool(xi, wl, bl)
        out.backward(gi)
        res.append((out.detach(), arg, wl.grad, bl.grad))
    (o1, a1, w1, b1), (o2, a2, w2, b2) = res
    assert torch.equal(o2, o1[perm]) and torch.equal(a2, a1[perm])
    o3, a3 = F.conv_maxpool(x[2999:3000].contiguous(), w, b)
    assert torch.equal(o3[0], o1[2999]) and torch.equal(a3[0], a1[2999])
    rw, rb = measures(w2.cpu().reshape(Fo, -1), w1.cpu().reshape(Fo, -1)), measures(b2.cpu(), b1.cpu())
    print("bf conv permuted batch: dW rel-L2 %.2e row-max %.2e   db rel-L2 %.2e row-max %.2e" % (rw + rb))
    assert max(rw + rb) <= PERM_DW


# ------------------------------------------------------------------------------------------------ tanh / sigmoid epilogues
@pytest.mark.parametrize("act", [2, 3])
@pytest.mark.parametrize("M,K,N,rs", [(r[0], r[1], r[2], r[4]) for r in _LIN])
def test_linear_tanh_sigmoid(dev, M, K, N, rs, act):
    import multimodal_transformer_amd.functional as F
    tag = "bf lin%dx%dx%d a%d%s" % (M, K, N, act, " rs" if rs else "")
    x, W, b, g = _lin_inputs(M, K, N, "bffe_lin%dx%dx%d" % (M, K, N))
    r = (R.gen_uniform("bffe_lin_r%d" % M, (M,), 5) > 0.3).float() if rs else None
    leaves = [t.to(dev).requires_grad_() for t in (x, W, b)]
    y = F.linear(*leaves, act=act, rowscale=None if r is None else r.to(dev))
    y.backward(g.to(dev))
    ld = [t.double().requires_grad_() for t in (x, W, b)]
    ref = E.linear(*ld, act=act, rowscale=None if r is None else r.double())
    ref.backward(g.double())
    failures = []
    check(tag + " y", y.detach().cpu(), ref.detach(), *LIN_ACT_OUT, failures=failures)
    for n, a, rr in zip(("dx", "dW", "db"), leaves, ld):
        check(tag + " " + n, a.grad.cpu(), rr.grad, *LIN_ACT_GRAD, failures=failures)
    if rs:
        assert (y.detach().cpu()[r == 0] == 0).all()
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ Highway
def hw_inputs(rows, n, tag):
    x = R.gen_normal(tag + "x", (rows, n), 31)
    Wp, Wg = (R.gen_normal(tag + k, (n, n), 31) / np.sqrt(n) for k in ("wp", "wg"))
    bp, bg = (0.1 * R.gen_normal(tag + k, (n,), 31) for k in ("bp", "bg"))
    return x, Wp, bp, Wg, bg, R.gen_normal(tag + "g", (rows, n), 31)


HW_NAMES = ("dx", "dWp", "dbp", "dWg", "dbg")


def hw_compare(tag, got, ref, out_b, grad_b, failures, scale_b=None):
    check(tag + " y", got[0], ref[0], *out_b, failures=failures)
    for n, a, r in zip(HW_NAMES, got[1:], ref[1:]):
        check("%s %s" % (tag, n), a, r, *grad_b, failures=failures)
        if scale_b is not None and n in ("dWp", "dWg") and float(np.abs(np.asarray(r)).max()) > 0:
            s = ls_scale(a, r)
            print("%-52s scale %.2e" % ("%s %s" % (tag, n), s))
            if abs(s) > scale_b:
                failures.append("%s %s: least-squares scale %.3e > %.1e" % (tag, n, s, scale_b))


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("proj_act", [0, 1])
@pytest.mark.parametrize("rows,n", [(12, 256), (7, 44), (1, 4), (500, 20), (3001, 256), (600, 300)])
def test_highway(dev, rows, n, proj_act, p):
    import multimodal_transformer_amd.functional as F
    tag = "bf hw %dx%d a%d p%g" % (rows, n, proj_act, p)
    *args, g = hw_inputs(rows, n, "bffe_hw%dx%d" % (rows, n))
    seed = 4242 + rows + n
    leaves = [t.to(dev).requires_grad_() for t in args]
    y = F.highway(*leaves, dropout_p=p, seed=seed, proj_act=proj_act)
    y.backward(g.to(dev))
    drop = None
    if p > 0:
        keep, scale = F.dropout_mask(p, seed, 3000, rows * n, dev)
        keep = keep.reshape(rows, n).cpu()
        assert abs(scale - 1.0 / (1.0 - p)) < 1e-3
        drop = keep.double() * scale
    ld = [t.double().requires_grad_() for t in args]
    ref = E.highway(*ld, drop=drop, proj_act=proj_act)
    ref.backward(g.double())
    if p > 0:
        yc = y.detach().cpu()
        assert (yc[~keep.bool()] == 0).all(), "dropped elements must be exactly zero"
        assert torch.equal(yc == 0, ~keep.bool() | (ref.detach() == 0))
    failures = []
    hw_compare(tag, [y.detach().cpu()] + [t.grad.cpu() for t in leaves], [ref.detach()] + [t.grad for t in ld], HW_OUT, HW_GRAD, failures,
               HW_W_SCALE if rows >= 12 else None)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("absent", [0, 1, 2], ids=["both", "no_dy1", "no_dy2"])
@pytest.mark.parametrize("M,K,N1,N2", [(210, 128, 128, 1024), (33, 256, 256, 512), (7, 44, 44, 80)])
def test_linear_pair(dev, M, K, N1, N2, absent):
    """The LSTM baselines' pair (ReLU attention hidden layer, LSTM input projection) of one time-major embedding; with dy1 or dy2 absent
    the node's backward receives None for that output."""
    import multimodal_transformer_amd.functional as F
    tag = "bf pair %dx%d->%d,%d %s" % (M, K, N1, N2, ("both", "no dy1", "no dy2")[absent])
    t = "bffe_pair%dx%d" % (M, K)
    x = R.gen_normal(t + "x", (M, K), 31)
    W1, W2 = R.gen_normal(t + "w1", (N1, K), 31) / np.sqrt(K), R.gen_normal(t + "w2", (N2, K), 31) / np.sqrt(K)
    b1, b2 = 0.1 * R.gen_normal(t + "b1", (N1,), 31), 0.1 * R.gen_normal(t + "b2", (N2,), 31)
    g1, g2 = R.gen_normal(t + "g1", (M, N1), 31), R.gen_normal(t + "g2", (M, N2), 31)

    def loss(y1, y2, a, b):
        return (0 if absent == 1 else (y1 * a).sum()) + (0 if absent == 2 else (y2 * b).sum())
    leaves = [v.to(dev).requires_grad_() for v in (x, W1, b1, W2, b2)]
    y1, y2 = F.linear_pair(*leaves, act1=1, act2=0)
    loss(y1, y2, g1.to(dev), g2.to(dev)).backward()
    ld = [v.double().requires_grad_() for v in (x, W1, b1, W2, b2)]
    r1, r2 = E.linear_pair(*ld, act1=1, act2=0)
    loss(r1, r2, g1.double(), g2.double()).backward()
    failures = []
    # ReLU and no activation: the single affine map's bound LIN_REL (measured here 8.8e-8 / 1.2e-7, dx 1.8e-7 / 3.1e-7)
    check(tag + " y1", y1.detach().cpu(), r1.detach(), LIN_REL, LIN_REL, failures=failures)
    check(tag + " y2", y2.detach().cpu(), r2.detach(), LIN_REL, LIN_REL, failures=failures)
    for i, n in enumerate(("dx", "dW1", "db1", "dW2", "db2")):
        dead = (absent == 1 and n in ("dW1", "db1")) or (absent == 2 and n in ("dW2", "db2"))
        got = leaves[i].grad
        if dead:                             # no gradient reaches this output's parameters: None or exact zeros
            assert got is None or float(got.abs().max()) == 0.0, n
            continue
        check("%s %s" % (tag, n), got.cpu(), ld[i].grad, LIN_REL, LIN_REL, failures=failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ conv -> Highway -> dropout
SFT_EMBED = {"linguistic": 300, "emotient": 20, "acoustic": 256, "image": 256}       # models._FrontEnd.window_embed_size
CHAIN_CASES = [("linguistic", 300, 3, 200), ("emotient", 20, 5, 513), ("acoustic", 256, 5, 513), ("acoustic", 88, 5, 513),
               ("image", 256, 1, 331)]   # (modality, window embed size of the SFT / MFT table, B, T): B T windows, >= 3 pairs per workgroup


def test_chain_cases_cover_both_embed_tables():
    have = {(m, f) for m, f, _, _ in CHAIN_CASES}
    assert have == {(m, f) for tab in (SFT_EMBED, R.FE_EMBED_MFT) for m, f in tab.items()}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mod,Fo,B,T", CHAIN_CASES, ids=["%s%d" % (c[0], c[1]) for c in CHAIN_CASES])
def test_window_encoder_chain(dev, mod, Fo, B, T, train):
    import multimodal_transformer_amd.functional as F
    W, D = R.FE_WINDOW[mod], R.FE_DIMS[mod]
    plan = E.conv_plan(B * T, W, D, Fo)
    assert plan["npairs"] >= 3 and plan["one_rt"]
    tag = "bf chain %s F%d %s" % (mod, Fo, "train" if train else "eval")
    h = "highway_%s." % mod
    shapes = {"cnn_%s.conv1d.weight" % mod: (Fo, D, 2), "cnn_%s.conv1d.bias" % mod: (Fo,), h + "linear_projection.weight": (Fo, Fo),
              h + "linear_projection.bias": (Fo,), h + "linear_gate.weight": (Fo, Fo), h + "linear_gate.bias": (Fo,)}
    p32 = R.gen_params(shapes, 37)
    x = R.gen_normal("bffe_chain:%s%d:x" % (mod, Fo), (B, T, W, D), 37)
    g = R.gen_normal("bffe_chain:%s%d:g" % (mod, Fo), (B, T, Fo), 37)
    pg = {k: v.to(dev).requires_grad_() for k, v in p32.items()}
    p, seed = (0.3, 977 + Fo) if train else (0.0, 0)
    names = list(shapes)

    def step():
        e, arg = F.conv_maxpool(x.to(dev).reshape(B * T, W, D), pg[names[0]], pg[names[1]])
        y = F.highway(e, *(pg[n] for n in names[2:]), dropout_p=p, seed=seed).reshape(B, T, Fo)
        y.backward(g.to(dev))
        return y.detach(), arg
    (y, arg), knames = device_kernel_names(step)
    check_conv_ran(tag, knames, plan)
    drop = None
    if train:
        keep, scale = F.dropout_mask(p, seed, 3000, B * T * Fo, dev)
        drop = keep.reshape(B * T, Fo).cpu().double() * scale
    pd = {k: v.double().requires_grad_() for k, v in p32.items()}
    ref, _ = E.window_encoder(pd, mod, x.double(), drop, arg=arg.cpu().long())
    ref.backward(g.double())
    failures = []
    check(tag + " y", y.cpu(), ref.detach(), *CHAIN_OUT, failures=failures)
    for n in names:
        a, r = pg[n].grad.cpu(), pd[n].grad
        if a.dim() == 3:
            a, r = a.reshape(Fo, -1), r.reshape(Fo, -1)
        check("%s %s" % (tag, n), a, r, *CHAIN_GRAD, failures=failures)
    assert not failures, "\n".join(failures)
