"""CPU checks of the K-tap window encoder: the C boundary's new entries (exported, shape queries, refusals), the bf16-faithful
reference tests/convk_ref.py against the plain oracle, against the 2-tap reference and against the closed form of its gradient, the
launch plan of every GPU case of tests/test_gpu_convk.py, and the floor of that file's bounds."""
import numpy as np
import torch

import bf16_ref as B
import convk_ref as E
import oracle
import recipe as R

MMT_EINVAL, MMT_EUNSUPPORTED = 1, 2


def _lib():
    from multimodal_transformer_amd import _lib
    return _lib.load()


def test_library_exports_the_k_tap_entries():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    for name in ("mmt_convpool_k_workspace_bytes", "mmt_convpool_k_forward", "mmt_convpool_k_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.mmt_abi_version() == 1


def test_workspace_query_and_refusals():
    lib = _lib()
    for K in (1, 2, 3, 4, 5):
        assert lib.mmt_convpool_k_workspace_bytes(37, 7, 52, 70, K) > 0, K
    for K in (0, 6):
        assert lib.mmt_convpool_k_workspace_bytes(37, 7, 52, 70, K) == 0
        assert b"kernel size" in lib.mmt_last_error()
        assert lib.mmt_convpool_k_forward(None, None, None, None, None, None, 0, 37, 7, 52, 70, K, None) == MMT_EUNSUPPORTED
    assert lib.mmt_convpool_k_workspace_bytes(37, 2, 52, 70, 3) == 0                  # W < K
    assert b"bad shape" in lib.mmt_last_error()
    assert lib.mmt_convpool_k_workspace_bytes(37, 3, 52, 70, 3) > 0                   # W == K: one position
    assert lib.mmt_convpool_k_workspace_bytes(0, 7, 52, 70, 3) == 0
    assert lib.mmt_convpool_k_workspace_bytes(37, 7, 50, 70, 3) == 0                  # D not a multiple of 4
    assert b"divisible by 4" in lib.mmt_last_error()
    assert lib.mmt_convpool_k_forward(None, None, None, None, None, None, 0, 37, 7, 52, 70, 3, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_convpool_k_backward(None, None, None, None, None, None, 0, 37, 7, 52, 70, 3, None) == MMT_EINVAL
    assert lib.mmt_convpool_k_backward(None, None, None, None, None, None, 0, 37, 2, 52, 70, 3, None) == MMT_EINVAL
    assert lib.mmt_convpool_k_forward(None, None, None, None, None, None, 0, 37, 7, 50, 70, 3, None) == MMT_EUNSUPPORTED


def _inputs(K, N=11, W=9, D=12, F=7, tag="convk_cpu"):
    x = R.gen_normal("%s:k%d:x" % (tag, K), (N, W, D), 29).double()
    w = (R.gen_normal("%s:k%d:w" % (tag, K), (F, D, K), 29) / np.sqrt(K * D)).double()
    b = (0.1 * R.gen_normal("%s:k%d:b" % (tag, K), (F,), 29)).double()
    g = R.gen_normal("%s:k%d:g" % (tag, K), (N, F), 29).double()
    return x, w, b, g


def test_plain_reference_is_the_oracle():
    for K in (1, 2, 3, 4, 5):
        for W in (K, 9):
            x, w, b, _ = _inputs(K, W=W)
            out, arg, S = E.conv_maxpool(x, w, b, rounding=False)
            ref, ref_arg = oracle.cnn_maxpool(x, w, b)
            assert S.shape == (x.shape[0], W - K + 1, w.shape[0])
            assert float((out - ref).abs().max()) <= 1e-12 and torch.equal(arg, ref_arg)


def test_two_taps_equal_bf16_ref():
    x, w, b, g = _inputs(2)
    res = []
    for mod in (E, B):
        wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
        out, arg, S = mod.conv_maxpool(x, wl, bl)
        out.backward(g)
        res.append((out.detach(), arg, S, wl.grad, bl.grad))
    for u, v in zip(*res):
        assert torch.equal(u, v)
    for u, v in zip(E.conv_sums(x, w), B.conv_sums(x, w)):
        assert torch.equal(u, v)
    assert not torch.equal(res[0][2], E.conv_maxpool(x, w, b, rounding=False)[2])     # the rounding does something


def test_gradient_for_a_given_argmax_is_the_closed_form():
    """dW[f, d, j] = sum_n bf16(dy[n, f]) bf16(x[n, arg + j, d]),  db[f] = sum_n dy[n, f], for ANY arg in range"""
    for K in (1, 3, 5):
        x, w, b, g = _inputs(K)
        N, W, D = x.shape
        F = w.shape[0]
        arg = torch.randint(0, W - K + 1, (N, F), generator=torch.Generator().manual_seed(K))
        wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
        out, arg2, _ = E.conv_maxpool(x, wl, bl, arg=arg)
        out.backward(g)
        assert torch.equal(arg2, arg)
        xr, gr = B._exact_bf16(x), B._exact_bf16(g)
        n_idx = torch.arange(N).unsqueeze(1).expand(N, F)
        want = torch.stack([(gr.unsqueeze(2) * xr[n_idx, arg + j]).sum(dim=0) for j in range(K)], dim=2)
        assert float((wl.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float((bl.grad - g.sum(0)).abs().max()) <= 1e-12


# (K, N, W, D, F): (wins, npairs, nsplit, last, one_rt, nrt, fwd launches (K, CT, channel blocks, c_first), backward grid)
_PLANS = {
    (1, 2565, 10, 88, 256): (6, 3, 428, 3, True, 1, [(1, 2, 2, 0)], (1, 428, 1)),
    (3, 2565, 10, 88, 256): (16, 8, 161, 5, True, 1, [(3, 2, 2, 0)], (3, 161, 1)),
    (4, 2565, 10, 88, 256): (22, 11, 117, 13, True, 1, [(4, 2, 2, 0)], (4, 117, 1)),
    (5, 2565, 10, 88, 256): (26, 13, 99, 17, True, 1, [(5, 2, 2, 0)], (5, 99, 1)),
    (3, 331, 30, 1000, 256): (16, 8, 21, 11, True, 1, [(3, 2, 2, 0)], (24, 21, 1)),
    (5, 331, 30, 1000, 256): (26, 13, 13, 19, True, 1, [(5, 2, 2, 0)], (40, 13, 1)),
    (4, 600, 33, 300, 300): (28, 14, 22, 12, True, 1, [(4, 2, 2, 0), (4, 1, 1, 256)], (12, 22, 2)),
    (3, 4000, 9, 20, 20): (24, 12, 167, 16, True, 1, [(3, 1, 1, 0)], (3, 167, 1)),
    (1, 9, 1, 40, 64): (2, 1, 5, 1, True, 1, [(1, 1, 1, 0)], (1, 5, 1)),
    (1, 2565, 1, 40, 64): (6, 3, 428, 3, True, 1, [(1, 1, 1, 0)], (1, 428, 1)),
    (3, 9, 3, 40, 64): (2, 1, 5, 1, True, 1, [(3, 1, 1, 0)], (3, 5, 1)),
    (3, 2565, 3, 40, 64): (16, 8, 161, 5, True, 1, [(3, 1, 1, 0)], (3, 161, 1)),
    (4, 9, 4, 40, 64): (2, 1, 5, 1, True, 1, [(4, 1, 1, 0)], (4, 5, 1)),
    (4, 2565, 4, 40, 64): (22, 11, 117, 13, True, 1, [(4, 1, 1, 0)], (4, 117, 1)),
    (5, 9, 5, 40, 64): (2, 1, 5, 1, True, 1, [(5, 1, 1, 0)], (5, 5, 1)),
    (5, 2565, 5, 40, 64): (26, 13, 99, 17, True, 1, [(5, 1, 1, 0)], (5, 99, 1)),
    (3, 9, 34, 40, 64): (2, 1, 5, 1, True, 1, [(3, 1, 1, 0)], (3, 5, 1)),
    (3, 2565, 34, 40, 64): (16, 8, 161, 5, True, 1, [(3, 1, 1, 0)], (3, 161, 1)),
    (3, 9, 35, 40, 64): (2, 1, 5, 1, False, 2, [(3, 1, 1, 0)], (3, 5, 1)),
    (3, 2565, 35, 40, 64): (16, 8, 161, 5, False, 2, [(3, 1, 1, 0)], (3, 161, 1)),
    (3, 9, 66, 40, 64): (2, 1, 5, 1, False, 2, [(3, 1, 1, 0)], (3, 5, 1)),
    (3, 2565, 66, 40, 64): (16, 8, 161, 5, False, 2, [(3, 1, 1, 0)], (3, 161, 1)),
    (3, 9, 67, 40, 64): (2, 1, 5, 1, False, 3, [(3, 1, 1, 0)], (3, 5, 1)),
    (3, 2565, 67, 40, 64): (16, 8, 161, 5, False, 3, [(3, 1, 1, 0)], (3, 161, 1)),
    (5, 9, 36, 40, 64): (2, 1, 5, 1, True, 1, [(5, 1, 1, 0)], (5, 5, 1)),
    (5, 2565, 36, 40, 64): (26, 13, 99, 17, True, 1, [(5, 1, 1, 0)], (5, 99, 1)),
    (5, 9, 37, 40, 64): (2, 1, 5, 1, False, 2, [(5, 1, 1, 0)], (5, 5, 1)),
    (5, 2565, 37, 40, 64): (26, 13, 99, 17, False, 2, [(5, 1, 1, 0)], (5, 99, 1)),
    (3, 1, 10, 88, 256): (2, 1, 1, 1, True, 1, [(3, 2, 2, 0)], (3, 1, 1)),
    (3, 7, 10, 88, 256): (2, 1, 4, 1, True, 1, [(3, 2, 2, 0)], (3, 4, 1)),
    (3, 8, 10, 88, 256): (2, 1, 4, 2, True, 1, [(3, 2, 2, 0)], (3, 4, 1)),
    (3, 9, 10, 88, 256): (2, 1, 5, 1, True, 1, [(3, 2, 2, 0)], (3, 5, 1)),
    (3, 37, 7, 52, 20): (2, 1, 19, 1, True, 1, [(3, 1, 1, 0)], (3, 19, 1)),
    (3, 37, 7, 52, 65): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (3, 19, 1)),
    (3, 37, 7, 52, 129): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0), (3, 1, 1, 128)], (3, 19, 1)),
    (3, 37, 7, 52, 300): (2, 1, 19, 1, True, 1, [(3, 2, 2, 0), (3, 1, 1, 256)], (3, 19, 2)),
    (3, 37, 7, 52, 600): (2, 1, 19, 1, True, 1, [(3, 2, 4, 0), (3, 2, 1, 512)], (3, 19, 3)),
    (3, 37, 7, 4, 70): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (3, 19, 1)),
    (3, 37, 7, 28, 70): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (3, 19, 1)),
    (3, 37, 7, 36, 70): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (3, 19, 1)),
    (3, 37, 7, 132, 70): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (6, 19, 1)),
    (3, 37, 7, 260, 70): (2, 1, 19, 1, True, 1, [(3, 2, 1, 0)], (9, 19, 1)),
    (5, 37, 7, 4, 70): (2, 1, 19, 1, True, 1, [(5, 2, 1, 0)], (5, 19, 1)),
    (5, 37, 7, 28, 70): (2, 1, 19, 1, True, 1, [(5, 2, 1, 0)], (5, 19, 1)),
    (5, 37, 7, 36, 70): (2, 1, 19, 1, True, 1, [(5, 2, 1, 0)], (5, 19, 1)),
    (5, 37, 7, 132, 70): (2, 1, 19, 1, True, 1, [(5, 2, 1, 0)], (10, 19, 1)),
    (5, 37, 7, 260, 70): (2, 1, 19, 1, True, 1, [(5, 2, 1, 0)], (15, 19, 1)),
    (3, 21, 12, 88, 256): (2, 1, 11, 1, True, 1, [(3, 2, 2, 0)], (3, 11, 1)),
    (5, 21, 40, 40, 64): (2, 1, 11, 1, False, 2, [(5, 1, 1, 0)], (5, 11, 1)),
    (3, 2565, 12, 88, 256): (16, 8, 161, 5, True, 1, [(3, 2, 2, 0)], (3, 161, 1)),
    (3, 40, 70, 40, 64): (2, 1, 20, 2, False, 3, [(3, 1, 1, 0)], (3, 20, 1)),
    (5, 40, 70, 40, 64): (2, 1, 20, 2, False, 3, [(5, 1, 1, 0)], (5, 20, 1)),
    (3, 24, 4, 40, 64): (2, 1, 12, 2, True, 1, [(3, 1, 1, 0)], (3, 12, 1)),
    (3, 24, 36, 40, 64): (2, 1, 12, 2, False, 2, [(3, 1, 1, 0)], (3, 12, 1)),
    (5, 24, 6, 40, 64): (2, 1, 12, 2, True, 1, [(5, 1, 1, 0)], (5, 12, 1)),
    (5, 24, 38, 40, 64): (2, 1, 12, 2, False, 2, [(5, 1, 1, 0)], (5, 12, 1)),
}


def test_conv_plan_of_every_gpu_case():
    import test_gpu_convk as G
    seen = set()
    for c in G.CONV_CASES:
        key = (c["K"], c["N"], c["W"], c["D"], c["F"])
        pl = E.conv_plan(c["N"], c["W"], c["D"], c["F"], c["K"])
        assert key in _PLANS, "no pinned plan for %s" % c["id"]
        got = (pl["wins"], pl["npairs"], pl["nsplit"], pl["last"], pl["one_rt"], pl["nrt"], pl["fwd"], pl["bwd_grid"])
        assert got == _PLANS[key], (c["id"], got, _PLANS[key])
        seen.add(key)
    assert seen == set(_PLANS)
    plans = list(_PLANS.values())
    # what the cases are for: both backward instances with >= 3 window pairs, 2 and 3 row tiles, CT = 2 and CT = 1 at c_first 0 and
    # beyond, odd and even last splits, more than one feature block and more than one channel block in the backward's grid
    assert any(p[4] and p[1] >= 3 for p in plans) and any(not p[4] and p[1] >= 3 for p in plans)
    assert {p[5] for p in plans} >= {1, 2, 3}
    fwd = [f for p in plans for f in p[6]]
    assert any(ct == 2 and first > 0 for _, ct, _, first in fwd) and any(ct == 1 and first > 0 for _, ct, _, first in fwd)
    assert any(ct == 1 and first == 0 for _, ct, _, first in fwd) and {k for k, _, _, _ in fwd} == {1, 3, 4, 5}
    assert any(p[3] % 2 == 1 and p[0] > 2 for p in plans) and any(p[3] % 2 == 0 for p in plans)
    assert any(p[7][0] > p[6][0][0] for p in plans) and any(p[7][2] > 1 for p in plans)


def test_forward_lds_fits_the_cu():
    """csrc/convk.h's table: the bulk geometry (CT = 2) fits the 160 KB of a CU at every K, CT = 4 does not from K = 3 on"""
    lds = lambda k, ct: 2 * (8 * (32 + k - 1) + 64 * k * ct) * 40 * 2  # noqa: E731
    assert [lds(k, E.CT_BULK) for k in (1, 3, 4, 5)] == [61440, 104960, 126720, 148480]
    assert all(lds(k, E.CT_BULK) <= 160 * 1024 for k in range(1, E.K_MAX + 1)) and lds(3, 4) > 160 * 1024


def test_tie_cases_tie_in_the_reference():
    import test_gpu_convk as G
    for c in G.CONV_CASES:
        if not c["kind"].startswith("tie"):
            continue
        x, w, b, g = G.conv_inputs(c)
        S, _ = E.conv_sums(x.double(), w.double())
        arg = S.argmax(dim=1)
        if c["kind"] == "tie_const":
            assert bool((S == S[:, :1]).all()) and int(arg.max()) == 0
        elif c["kind"] == "tie_pad":
            last = c["W"] - c["K"]
            assert bool((S[:, last] == 0).all()) and bool((S[:, :last] < 0).all()) and bool((arg == last).all())
        else:
            for res, (p, q) in G.tie_positions(c).items():
                assert q - p >= c["K"] and torch.equal(S[res::2, p], S[res::2, q])
                n = int((arg[res::2] == p).sum())
                print("%s: windows %d mod 2, positions %d = %d are the maximum of %d pairs" % (c["id"], res, p, q, n))
                assert n > 100 and int((arg[res::2] == q).sum()) == 0


def test_jitter_floor():
    """What noise of half an fp32 ulp per accumulated term does to the reference itself: `out` moves by less than CONV_OUT allows, and
    the argmax changes in at most ARG_SHARE of the pairs (the condition under which that cap can hold).  One case per K of the many-window
    group and the two longest sums."""
    import test_gpu_convk as G
    from gpu_harness import measures
    for c in G.CONV_CASES:
        if not (c["kind"] == "many" and (c["N"] == G.MANY_N or c["D"] == 1000)):
            continue
        x, w, b, g = G.conv_inputs(c)
        o0, a0, _ = E.conv_maxpool(x.double(), w.double(), b.double())
        with B.jitter(6e-8, 1):
            o1, a1, _ = E.conv_maxpool(x.double(), w.double(), b.double())
        d = int((a0 != a1).sum())
        rel, row = measures(o1.numpy(), o0.numpy())
        print("jitter floor %-32s out rel-L2 %.2e row-max %.2e, argmax changes in %d of %d pairs" % (c["id"], rel, row, d, a0.numel()))
        assert rel <= G.CONV_OUT[0] and row <= G.CONV_OUT[1], c["id"]
        assert d <= G.ARG_SHARE * a0.numel(), c["id"]
    assert G.CONV_OUT[0] <= 2e-2 and G.CONV_DW[0] <= 1e-2 and G.CONV_DB[0] <= 1e-5     # the plain-fp64 bounds of test_gpu_frontend.py
