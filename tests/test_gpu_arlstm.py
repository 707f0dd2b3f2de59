"""GPU: the LSTM baseline with an autoregressive read-out (MultiARLSTM) on the HIP path — the read-out kernels (csrc/ar_combine.h,
functional.ar_combine) and the class around them.

* the five fixtures of tests/golden/make_golden_arlstm.py through models.MultiARLSTM, with the bounds and the form of
  test_gpu_lstm_baselines.py (on the code before this class existed the import fails);
* ar_combine alone against the fp64 restatement tests/ar_ref.py (pinned to torch autograd on the reference's formula and to the
  reference's fixtures by tests/test_arlstm_cpu.py): p, the masked output, d in_part and d w, both branches, ragged masks, at the
  smallest shapes that take every path — T of 1, 2, K, K + 1, the chunk length C = 64, C + 1 and 2C + 3; K of 1, 2, 3, 8 and 16; one and
  three sequences and S + 1 = 5 (a second workgroup whose last three waves leave at once); T < K in both branches.  The bound of every
  tensor is twice the rel-L2 error of the reference's own formula evaluated in torch fp32 on the CPU, with the floor (K + 2) 2^-24
  (fused multiply-adds and another summation order within a step);
* the reference's quirks on hand-made integers; limits refused before any launch; bit-identical reruns; a train step without library
  kernels and its hipGraph replay = eager, in both branches.
"""
import numpy as np
import pytest
import torch

import ar_ref as AR
import arlstm_cases as C
import recipe as R
from conftest import rel_l2
from gpu_harness import dev, device_kernel_names, library_kernels, load_named  # noqa: F401 (dev: a fixture)
from test_arlstm_cpu import _reference_formula
from test_gpu_lstm_baselines import _run

pytestmark = pytest.mark.gpu

CHUNK = 64                              # csrc/ar_combine.h MMT_AR_CHUNK: steps per chunk of the free-running walk
SEQS = 4                                # MMT_AR_SEQS: sequences (waves) per workgroup
P_INIT = 0.375


# ---------------------------------------------------------------------------------------------------------------- model goldens
@pytest.mark.parametrize("case", C.ARLSTM_CASES, ids=[c[0] for c in C.ARLSTM_CASES])
def test_arlstm_golden(dev, case):
    from multimodal_transformer_amd.models import MultiARLSTM
    name, D, kw, lengths, T, tgt_init, teacher = case
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).to(dev)
    target = C.ar_target(name, lengths, T).to(dev) if teacher else None
    _run(name, MultiARLSTM(D, device=dev, **kw), lambda m, mask: m(x, mask, lengths, target=target, tgt_init=tgt_init), lengths, T, dev)


# ---------------------------------------------------------------------------------------------------------------- the read-out alone
def _inputs(B, T, K, tag):
    """fp32 tensors (the fp64 reference reads the same values): in_part, w with sum_k |w[b,t,k]| <= 0.9 (a contractive recurrence), a
    ragged prefix mask, a target and the incoming gradient"""
    g = lambda n, shape: R.gen_normal("ar:%s:%s" % (tag, n), shape, 9)      # noqa: E731
    w = g("w", (B, T, K))
    w = w / w.abs().sum(dim=2, keepdim=True) * (0.45 + 0.44 * R.gen_uniform("ar:%s:s" % tag, (B, T, 1), 9))
    assert float(w.abs().sum(dim=2).max()) <= 0.9
    lengths = [max(1, T - (T * b) // (B + 1)) for b in range(B)]
    return dict(c=g("c", (B, T, 1)), w=w, mask=R.prefix_mask(lengths, T), tgt=g("tgt", (B, T, 1)), g=g("g", (B, T, 1)))


def _gpu(inp, teacher, dev, p_init=P_INIT):
    from multimodal_transformer_amd import functional as F
    c, w = inp["c"].to(dev).requires_grad_(), inp["w"].to(dev).requires_grad_()
    out, p = F.ar_combine(c, w, inp["mask"].to(dev), inp["tgt"].to(dev) if teacher else None, p_init, return_p=True)
    out.backward(inp["g"].to(dev))
    torch.cuda.synchronize()
    B, T, K = w.shape
    return {k: v.detach().cpu().numpy().reshape(B, T, -1) for k, v in (("p", p), ("out", out), ("din", c.grad), ("dw", w.grad))}


def _fp64(inp, teacher, p_init=P_INIT):
    B, T, K = inp["w"].shape
    c, mask, tgt, g = (inp[k].double().numpy().reshape(B, T) for k in ("c", "mask", "tgt", "g"))
    w = inp["w"].double().numpy()
    p, out = AR.forward(c, w, mask, tgt if teacher else None, p_init)
    din, dw = AR.backward(g, mask, tgt if teacher else p, K, teacher, p_init)
    return {"p": p.reshape(B, T, 1), "out": out.reshape(B, T, 1), "din": din.reshape(B, T, 1), "dw": dw}


def _cpu_fp32(inp, teacher, p_init=P_INIT):
    """the reference's own formula (its step loop, its stack-and-sum) in torch fp32 on the CPU, differentiated by autograd"""
    c, w = inp["c"].clone().requires_grad_(), inp["w"].clone().requires_grad_()
    p, out = _reference_formula(c, w, inp["mask"], inp["tgt"] if teacher else None, p_init)
    out.backward(inp["g"])
    return {k: v.detach().numpy() for k, v in (("p", p), ("out", out), ("din", c.grad), ("dw", w.grad))}


AR_CASES = [  # (B, T, K): every T of {1, 2, K, K+1, C, C+1, 2C+3}, every K of {1, 2, 3, 8, 16}, every B of {1, 3, S+1}
    (1, 1, 1), (3, 2, 1), (5, 2, 2), (1, 3, 2), (3, 1, 3), (1, 2, 3), (3, 3, 3), (5, 4, 3), (1, 8, 8), (3, 9, 8), (5, 2, 16), (3, 16, 16), (1, 17, 16),
    (SEQS + 1, CHUNK, 1), (3, CHUNK + 1, 2), (1, CHUNK, 16), (3, 2 * CHUNK + 3, 3), (SEQS + 1, 2 * CHUNK + 3, 8), (1, 2 * CHUNK + 3, 16),
    (3, CHUNK + 1, 1),
]


def test_cases_cover_every_path():
    Ts, Ks, Bs = {c[1] for c in AR_CASES}, {c[2] for c in AR_CASES}, {c[0] for c in AR_CASES}
    assert {1, 2, CHUNK, CHUNK + 1, 2 * CHUNK + 3} <= Ts and Ks == {1, 2, 3, 8, 16} and Bs == {1, 3, SEQS + 1}
    for K in Ks:
        assert any(c[2] == K and c[1] == K for c in AR_CASES) and any(c[2] == K and c[1] == K + 1 for c in AR_CASES), K
    assert any(c[1] < c[2] for c in AR_CASES)           # both branches run every case


@pytest.mark.parametrize("teacher", [False, True], ids=["free", "teacher"])
@pytest.mark.parametrize("B,T,K", AR_CASES, ids=["B%d_T%d_K%d" % c for c in AR_CASES])
def test_ar_combine_against_fp64(dev, B, T, K, teacher):
    inp = _inputs(B, T, K, "%d_%d_%d" % (B, T, K))
    got, ref, cpu = _gpu(inp, teacher, dev), _fp64(inp, teacher), _cpu_fp32(inp, teacher)
    floor = (K + 2) * 2.0 ** -24
    bad = []
    for k in ("p", "out", "din", "dw"):
        assert got[k].shape == ref[k].shape == cpu[k].shape, k
        e, e32 = rel_l2(got[k], ref[k]), rel_l2(cpu[k], ref[k])
        bound = max(2.0 * e32, floor)
        print("B=%d T=%d K=%d %-7s %-3s kernel %.3e  cpu fp32 %.3e  bound %.3e" % (B, T, K, "teacher" if teacher else "free", k, e, e32, bound))
        if not (np.isfinite(got[k]).all() and e <= bound):
            bad.append((k, e, bound))
    assert not bad, bad
    assert (got["out"][inp["mask"].numpy() == 0] == 0).all() and (got["din"][inp["mask"].numpy() == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- semantics pins
def _exact(dev, c, w, tgt=None, p_init=0.0, g=None):
    """small integers: every product and sum is exact in fp32, so the comparisons below are equalities"""
    from multimodal_transformer_amd import functional as F
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)      # noqa: E731
    ct, wt = t(c).reshape(1, -1, 1).requires_grad_(), t(w).reshape(1, len(c), -1).requires_grad_()
    out, p = F.ar_combine(ct, wt, torch.ones_like(ct), None if tgt is None else t(tgt).reshape(1, -1, 1), p_init, return_p=True)
    out.backward(torch.ones_like(out) if g is None else t(g).reshape(1, -1, 1))
    return p.flatten().tolist(), ct.grad.flatten().tolist(), wt.grad.reshape(len(c), -1).tolist()


def test_teacher_forced_tap_0_reads_the_current_target_and_the_padding_is_zero(dev):
    p, _, dw = _exact(dev, [0, 0, 0], [[1, 0]] * 3, tgt=[1, 2, 3], p_init=7.0)
    assert p == [1, 2, 3]
    assert dw == [[1, 0], [2, 1], [3, 2]]               # tap 1 of step 0 reads the padding: 0, not tgt_init = 7
    p, _, _ = _exact(dev, [0, 0, 0], [[0, 1]] * 3, tgt=[1, 2, 3], p_init=7.0)
    assert p == [0, 1, 2]


def test_free_running_tap_order_is_reversed_and_the_padding_is_tgt_init(dev):
    p, _, dw = _exact(dev, [1, 1, 1], [[0, 1]] * 3, p_init=7.0)      # the LAST tap reads the newest prediction
    assert p == [8, 9, 10]
    assert dw == [[7, 7], [7, 8], [8, 9]]               # taps (t-2, t-1): tgt_init before step 0
    p, _, _ = _exact(dev, [1, 1, 1], [[1, 0]] * 3, p_init=7.0)       # the FIRST tap reads p[t-2]
    assert p == [8, 8, 9]


def test_the_history_carries_no_gradient(dev):
    w, g = [[2], [2], [2]], [1, 10, 100]
    p_a, din_a, _ = _exact(dev, [1, 0, 0], w, g=g)
    p_b, din_b, _ = _exact(dev, [2, 0, 0], w, g=g)
    assert p_a == [1, 2, 4] and p_b == [2, 4, 8]        # in_part[0] reaches every later prediction ...
    assert din_a == g and din_b == g                    # ... but its gradient is g[0] alone (1 + 2*10 + 4*100 with a live history)


# ---------------------------------------------------------------------------------------------------------------- limits
def _refused(call, match):
    """call() raises NotImplementedError naming the limit -> the device kernels it launched before that (None or empty: none)"""
    def run():
        with pytest.raises(NotImplementedError, match=match):
            call()
    return device_kernel_names(run)[1]


@pytest.mark.parametrize("K", [0, 17])
def test_ar_order_outside_the_limit_is_refused_before_any_launch(dev, K):
    from multimodal_transformer_amd import functional as F
    from multimodal_transformer_amd.models import MultiARLSTM
    z = lambda *s: torch.zeros(*s, device=dev)                                                                   # noqa: E731
    args, tgt = (z(2, 3, 1), z(2, 3, K), z(2, 3, 1)), z(2, 3, 1)
    model = MultiARLSTM(48, embed_dim=16, h_dim=24, attn_len=2, ar_order=K, device=dev).eval()
    x, lengths = z(2, 3, 48), [3, 2]
    mask = R.prefix_mask(lengths, 3).to(dev)
    torch.cuda.synchronize()
    for call in (lambda: F.ar_combine(*args), lambda: F.ar_combine(*args, target=tgt), lambda: model(x, mask, lengths)):
        names = _refused(call, "1 <= ar_order <= 16")
        assert not names, names


def test_h_dim_512_is_refused_before_any_launch(dev):
    from multimodal_transformer_amd.models import MultiARLSTM
    model = MultiARLSTM(48, embed_dim=16, attn_len=2, device=dev).eval()          # the reference's default h_dim = 512
    assert model.h_dim == 512
    x, lengths = torch.zeros(2, 3, 48, device=dev), [3, 2]
    mask = R.prefix_mask(lengths, 3).to(dev)
    torch.cuda.synchronize()
    names = _refused(lambda: model(x, mask, lengths), "from 4 to 256")
    assert not names, names


def test_a_target_that_requires_grad_is_refused(dev):
    from multimodal_transformer_amd import functional as F
    z = lambda *s: torch.zeros(*s, device=dev)                                                                   # noqa: E731
    with pytest.raises(NotImplementedError, match="target"):
        F.ar_combine(z(2, 3, 1), z(2, 3, 2), z(2, 3, 1), target=z(2, 3, 1).requires_grad_())


# ---------------------------------------------------------------------------------------------------------------- runtime behaviour
@pytest.mark.parametrize("teacher", [False, True], ids=["free", "teacher"])
def test_two_runs_are_bit_identical(dev, teacher):
    inp = _inputs(SEQS + 1, 2 * CHUNK + 3, 3, "repro")
    a, b = _gpu(inp, teacher, dev), _gpu(inp, teacher, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _setup(dev):
    from multimodal_transformer_amd.models import MultiARLSTM
    B, T, D = 3, 12, 48
    model = MultiARLSTM(D, embed_dim=64, h_dim=32, attn_len=3, ar_order=3, device=dev)
    load_named(model, 3)
    model.train()
    lengths = [12, 9, 4]
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("artrain:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    x = R.gen_normal("artrain:x", (B, T, D), 3).to(dev)
    return model, x, lengths, mask, tgt


def _step_fn(model, call, tgt, lengths):
    from multimodal_transformer_amd import functional as F
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        out = call()
        F.mse_sum_loss_backward(out, tgt, sum(lengths))
        return out
    return step, params


def _call(model, x, mask, lengths, tgt, teacher):
    return lambda: model(x, mask, lengths, target=tgt if teacher else None, tgt_init=0.25)


@pytest.mark.parametrize("teacher", [False, True], ids=["free", "teacher"])
def test_train_step_runs_no_library_kernel(dev, teacher):
    model, x, lengths, mask, tgt = _setup(dev)
    step, params = _step_fn(model, _call(model, x, mask, lengths, tgt, teacher), tgt, lengths)
    names = device_kernel_names(step, warm=True)[1]
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    if names is None:
        pytest.skip("torch.profiler reports no device kernels here")
    fwd = "ar_teacher_fwd" if teacher else "ar_free_fwd"
    assert any(fwd in n for n in names) and any("ar_bwd" in n for n in names), names
    assert library_kernels(names) == [], "library kernels in a MultiARLSTM train step: %s" % library_kernels(names)


@pytest.mark.parametrize("teacher", [False, True], ids=["free", "teacher"])
def test_train_step_hipgraph_replay_equals_eager(dev, monkeypatch, teacher):
    """As test_gpu_edlstm.py::test_train_step_hipgraph_replay_equals_eager, for MultiARLSTM in both branches."""
    from multimodal_transformer_amd import graphs, functional as F
    monkeypatch.setenv("MMT_DEVICE_SEED", "1")
    model, x, lengths, mask, tgt = _setup(dev)
    step, params = _step_fn(model, _call(model, x, mask, lengths, tgt, teacher), tgt, lengths)
    step()                                              # creates the seed states
    seeds = [ds.state for m in model.modules() for ds in m.__dict__.get("_dev_seeds", {}).values()]
    assert len(seeds) >= 1                               # embed dropout
    snap = [s.clone() for s in seeds]
    y_ref = step().detach().clone()
    g_ref = [p.grad.detach().clone() for p in params]
    torch.cuda.synchronize()
    g, y_static = graphs.capture_step(step, warmup=1)
    for s, v in zip(seeds, snap):
        s.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_static, y_ref)
    for p, r in zip(params, g_ref):
        assert torch.equal(p.grad, r)
    F.check_device_errors()
