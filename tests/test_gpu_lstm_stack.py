"""GPU: stacked LSTMs (n_layers > 1) on the HIP path — the stacked decoder scan (csrc/scan_stack.h, functional.lstm_stack_scan) and the
multi-layer LSTM baselines.

* the five fixtures of tests/golden/make_golden_stacked.py through the public classes, with the bounds and the form of
  test_gpu_lstm_baselines.py (on the code before this scan existed they raise NotImplementedError);
* the scan alone against the fp64 restatement tests/lstm_stack_ref.py (pinned to the reference by tests/test_lstm_stack_cpu.py), forward
  and every gradient, at the smallest shapes that take every path: T of 1, 2, the ring depth + 1 and 13; one, two and three sequences
  (one per workgroup) and 257 (two per workgroup, the last one half empty); H of 4, 40 (padded units), 64 and 128 (both HPAD); 2..4 layers;
* against the existing kernels: without feedback columns the stack is lstm_scan -> linear -> lstm_scan, and its error against fp64 may be
  at most twice the composition's;
* limits refused before any launch; bit-identical reruns; a train step without library kernels; hipGraph replay = eager;
* n_layers = 1 launches exactly the kernels it launched before the stacked scan existed (tests/golden/stack_unchanged_kernels.json).
"""
import json
import os

import numpy as np
import pytest
import torch

import lstm_stack_ref as S
import recipe as R
import stacked_cases as C
from conftest import GOLDEN, rel_l2
from gpu_harness import OUT_RTOL, GRAD_RTOL, RELU_GRAD_RTOL, CCC_MIN, check, dev, device_kernel_names, library_kernels, load_named  # noqa: F401
from test_gpu_lstm_baselines import _run

pytestmark = pytest.mark.gpu

PF = 2                                  # csrc/api.hip MMT_STACK_PF: the only ring depth instantiated


# ---------------------------------------------------------------------------------------------------------------- model goldens
def _model(cls, D, kw, dev):
    from multimodal_transformer_amd import models as M, multiTransformer as MT
    ctor = {"NLPTransformer": MT.NLPTransformer, "UniTransformer": MT.UniTransformer, "MultiLSTM": M.MultiLSTM, "MultiLSTMB1": M.MultiLSTMB1}[cls]
    return ctor(D, device=dev, **kw)


@pytest.mark.parametrize("case", C.DECODER_CASES + C.BASELINE_CASES, ids=[c[0] for c in C.DECODER_CASES + C.BASELINE_CASES])
def test_stacked_model_golden(dev, case):
    name, cls, _, D, kw, lengths, T = case
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).to(dev)
    _run(name, _model(cls, D, kw, dev), lambda m, mask: m(x, mask, lengths), lengths, T, dev)


# ---------------------------------------------------------------------------------------------------------------- the scan alone
def _scan_inputs(T, B, H, L, tag, feedback=True):
    g = lambda n, shape: R.gen_normal("stack:%s:%s" % (tag, n), shape, 7).double().numpy()      # noqa: E731
    P = g("P", (L, 4 * H, 2 * H)) / np.sqrt(2 * H)
    if not feedback:
        P[0, :, :H] = 0.0
    return dict(gx0=g("gx0", (T, B, 4 * H)), P=P, bias=0.1 * g("bias", (L - 1, 4 * H)), h0=0.5 * g("h0", (L, B, H)),
                c0=0.5 * g("c0", (L, B, H))), g("w", (T, B, H))


def _run_stack(inp, w, dev):
    from multimodal_transformer_amd import functional as F
    ts = {k: torch.tensor(v, dtype=torch.float32, device=dev).requires_grad_() for k, v in inp.items()}
    h_top, h_all, c_all = F.lstm_stack_scan(ts["gx0"], ts["P"], ts["bias"], ts["h0"], ts["c0"], return_states=True)
    h_top.backward(torch.tensor(w, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    out = {"h_top": h_top, "h_all": h_all, "c_all": c_all}
    out.update({"d" + k: t.grad for k, t in ts.items()})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _reference(inp, w):
    h_all, c_all, acts = S.forward(**inp)
    g = S.backward(w, inp["P"], inp["h0"], inp["c0"], h_all, c_all, acts)
    return dict(h_top=h_all[-1], h_all=h_all, c_all=c_all, dgx0=g["dgx0"], dP=g["dP"], dbias=g["dbias"], dh0=g["dh0"], dc0=g["dc0"])


SCAN_CASES = [  # (T, B, H, L)
    (1, 1, 4, 2), (1, 3, 128, 4), (1, 2, 40, 2), (2, 2, 40, 3), (2, 3, 4, 4), (PF + 1, 3, 64, 2), (PF + 1, 1, 128, 3),
    (13, 1, 128, 4), (13, 3, 40, 2), (13, 2, 64, 4), (13, 2, 128, 2), (13, 1, 64, 3),
    (2, 257, 40, 2), (PF + 1, 257, 128, 3),             # two sequences per workgroup; the last workgroup holds one live sequence
]


@pytest.mark.parametrize("T,B,H,L", SCAN_CASES, ids=["T%d_B%d_H%d_L%d" % c for c in SCAN_CASES])
def test_stack_scan_against_fp64(dev, T, B, H, L):
    inp, w = _scan_inputs(T, B, H, L, "%d_%d_%d_%d" % (T, B, H, L))
    got, ref = _run_stack(inp, w, dev), _reference(inp, w)
    failures = []
    for k in ("h_top", "h_all", "c_all"):
        check("T%d B%d H%d L%d %s" % (T, B, H, L, k), got[k], ref[k], OUT_RTOL, failures=failures)
    for k in ("dgx0", "dP", "dbias", "dh0", "dc0"):
        check("T%d B%d H%d L%d %s" % (T, B, H, L, k), got[k], ref[k], GRAD_RTOL, failures=failures)
    assert not failures, failures


@pytest.mark.parametrize("H", [64, 128])
def test_stack_without_feedback_against_existing_kernels(dev, H):
    """P_0's feedback columns zero: the stack is layer-by-layer composition.  Same inputs through lstm_scan -> linear -> lstm_scan; both
    against fp64; the stack's rel-L2 error may be at most 2 x the composition's (same bf16 rounding sites: 2 covers ordering noise)."""
    from multimodal_transformer_amd import functional as F
    T, B, L = 13, 2, 2
    inp, w = _scan_inputs(T, B, H, L, "compose%d" % H, feedback=False)
    ref = _reference(inp, w)
    got = _run_stack(inp, w, dev)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev).requires_grad_()       # noqa: E731
    gx0, Whh0, Wih1, Whh1, b1 = t(inp["gx0"]), t(inp["P"][0][:, H:]), t(inp["P"][1][:, :H]), t(inp["P"][1][:, H:]), t(inp["bias"][0])
    h0, c0 = t(inp["h0"]), t(inp["c0"])
    h1, _ = F.lstm_scan(gx0, Whh0, h0[0], c0[0])
    h2, _ = F.lstm_scan(F.linear(h1, Wih1, b1), Whh1, h0[1], c0[1])
    h2.backward(torch.tensor(w, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    n = lambda a: a.detach().cpu().numpy()                                                                      # noqa: E731
    pairs = {  # name: (stack, composition, fp64)
        "h_top": (got["h_top"], n(h2), ref["h_top"]), "h^0": (got["h_all"][0], n(h1), ref["h_all"][0]),
        "dgx0": (got["dgx0"], n(gx0.grad), ref["dgx0"]),
        "dW_hh_l0": (got["dP"][0][:, H:], n(Whh0.grad), ref["dP"][0][:, H:]),
        "dW_ih_l1": (got["dP"][1][:, :H], n(Wih1.grad), ref["dP"][1][:, :H]),
        "dW_hh_l1": (got["dP"][1][:, H:], n(Whh1.grad), ref["dP"][1][:, H:]),
        "dbias_l1": (got["dbias"][0], n(b1.grad), ref["dbias"][0]),
        "dh0": (got["dh0"], n(h0.grad), ref["dh0"]), "dc0": (got["dc0"], n(c0.grad), ref["dc0"]),
    }
    bad = []
    for k, (a, b, r) in pairs.items():
        ea, eb = rel_l2(a, r), rel_l2(b, r)
        print("H=%-4d %-10s stack %.3e  composition %.3e  ratio %.2f" % (H, k, ea, eb, ea / max(eb, 1e-30)))
        if ea > 2.0 * eb:
            bad.append((k, ea, eb))
    assert not bad, bad


@pytest.mark.parametrize("T,B,H,L", [(2, 1, 256, 2), (2, 1, 8, 5), (1, 513, 4, 2)], ids=["H256", "L5", "B513"])
def test_limits_are_refused_before_any_launch(dev, T, B, H, L):
    from multimodal_transformer_amd import functional as F
    z = lambda *s: torch.zeros(*s, device=dev)                                                                   # noqa: E731
    args = (z(T, B, 4 * H), z(L, 4 * H, 2 * H), z(L - 1, 4 * H), z(L, B, H), z(L, B, H))
    torch.cuda.synchronize()
    _, names = device_kernel_names(lambda: pytest.raises((NotImplementedError, ValueError), F.lstm_stack_scan, *args))
    assert not names, names


def test_two_runs_are_bit_identical(dev):
    inp, w = _scan_inputs(13, 3, 40, 3, "repro")
    a, b = _run_stack(inp, w, dev), _run_stack(inp, w, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- train step
def _sft_setup(dev, n_layers=2, train=True):
    from multimodal_transformer_amd import multiTransformer as MT
    B, T, D = 3, 12, 48
    model = MT.NLPTransformer(D, embed_dim=64, h_dim=32, N=1, h=4, n_layers=n_layers, device=dev)
    load_named(model, 3)
    model.train(train)
    lengths = [12, 9, 4]
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("stacktrain:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    x = R.gen_normal("stacktrain:x", (B, T, D), 3).to(dev)
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


def test_train_step_runs_no_library_kernel(dev):
    model, x, lengths, mask, tgt = _sft_setup(dev)
    step, params = _step_fn(model, lambda: model(x, mask, lengths), tgt, lengths)
    names = device_kernel_names(step, warm=True)[1]
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    if names is None:
        pytest.skip("torch.profiler reports no device kernels here")
    assert any("lstm_stack_fwd" in n for n in names) and any("lstm_stack_bwd" in n for n in names), names
    assert library_kernels(names) == [], "library kernels in an n_layers=2 train step: %s" % library_kernels(names)


def test_train_step_hipgraph_replay_equals_eager(dev, monkeypatch):
    """As test_gpu_lstm_baselines.py::test_b1_train_step_hipgraph_replay_equals_eager, for NLPTransformer(n_layers=2)."""
    from multimodal_transformer_amd import graphs, functional as F
    monkeypatch.setenv("MMT_DEVICE_SEED", "1")
    model, x, lengths, mask, tgt = _sft_setup(dev)
    step, params = _step_fn(model, lambda: model(x, mask, lengths), tgt, lengths)
    step()                                              # creates the seed states
    seeds = [ds.state for m in model.modules() for ds in m.__dict__.get("_dev_seeds", {}).values()]
    assert len(seeds) >= 2                               # embed dropout, encoder stack
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


# ---------------------------------------------------------------------------------------------------------------- n_layers = 1 unchanged
def unchanged_path_steps(dev):
    """name -> an eval-mode forward + backward of a one-layer model (the shapes whose kernel names the fixture records)"""
    from multimodal_transformer_amd import models as M
    model, x, lengths, mask, tgt = _sft_setup(dev, n_layers=1, train=False)
    steps = {"NLPTransformer_l1": _step_fn(model, lambda: model(x, mask, lengths), tgt, lengths)[0]}
    lstm = M.MultiLSTM(48, embed_dim=64, h_dim=32, n_layers=1, device=dev).eval()
    load_named(lstm, 3)
    steps["MultiLSTM_l1"] = _step_fn(lstm, lambda: lstm(x, mask, lengths), tgt, lengths)[0]
    return steps


@pytest.mark.parametrize("which", ["NLPTransformer_l1", "MultiLSTM_l1"])
def test_one_layer_models_launch_the_kernels_they_did(dev, which):
    with open(os.path.join(GOLDEN, "stack_unchanged_kernels.json")) as fh:
        want = json.load(fh)[which]
    names = device_kernel_names(unchanged_path_steps(dev)[which], warm=True)[1]
    if names is None:
        pytest.skip("torch.profiler reports no device kernels here")
    assert not any("lstm_stack" in n for n in names)
    assert names == want
