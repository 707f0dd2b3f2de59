"""GPU: the encoder-decoder LSTM (MultiEDLSTM) on the HIP path — the LSTM scan with the read-out MLP in its recurrence (csrc/scan_fb.h,
functional.lstm_fb_scan) and the class around it.

* the three fixtures of tests/golden/make_golden_edlstm.py through models.MultiEDLSTM, with the bounds and the form of
  test_gpu_lstm_baselines.py (on the code before this class existed the import fails);
* the scan alone against the fp64 restatement tests/lstm_fb_ref.py (pinned to torch autograd and to the reference by
  tests/test_lstm_fb_cpu.py), forward and every gradient, at the smallest shapes that take every path: T of 1, 2, the ring depth + 1 and
  13; one to three sequences (one per workgroup) and 257 (two per workgroup, the last one half empty); H of 4, 40 (padded units), 64 and
  128 (both HPAD); E of 4, 24, 40, 64 and 128 (one to eight read-out tiles per wave, one to four backward k-blocks);
* against the existing kernels: with w_p = 0 the scan is lstm_scan -> linear(ReLU) -> linear, and its error against fp64 may be at most
  twice the composition's;
* the feedback is live; limits refused before any launch; bit-identical reruns; a train step without library kernels; hipGraph replay
  = eager.
"""
import numpy as np
import pytest
import torch

import edlstm_cases as C
import lstm_fb_ref as FB
import recipe as R
from conftest import rel_l2
from gpu_harness import OUT_RTOL, GRAD_RTOL, RELU_GRAD_RTOL, check, dev, device_kernel_names, library_kernels, load_named  # noqa: F401
from test_gpu_lstm_baselines import _run

pytestmark = pytest.mark.gpu

PF = 4                                  # csrc/api.hip MMT_FB_PF: the only ring depth instantiated


# ---------------------------------------------------------------------------------------------------------------- model goldens
@pytest.mark.parametrize("case", C.EDLSTM_CASES, ids=[c[0] for c in C.EDLSTM_CASES])
def test_edlstm_golden(dev, case):
    from multimodal_transformer_amd.models import MultiEDLSTM
    name, D, kw, lengths, T, tgt_init = case
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).to(dev)
    _run(name, MultiEDLSTM(D, device=dev, **kw), lambda m, mask: m(x, mask, lengths, tgt_init=tgt_init), lengths, T, dev)


# ---------------------------------------------------------------------------------------------------------------- the scan alone
KEYS = ("gxc", "w_p", "W_hh", "W1", "b1", "w2", "b2", "h0", "c0")
P_INIT = 0.375


def _scan_inputs(T, B, H, E, tag, feedback=True):
    g = lambda n, shape: R.gen_normal("fb:%s:%s" % (tag, n), shape, 7).double().numpy()      # noqa: E731
    # fan-in scaling: w_p multiplies one input of the 1 + H the decoder LSTM reads
    inp = dict(gxc=g("gxc", (T, B, 4 * H)), w_p=g("w_p", (4 * H,)) / np.sqrt(1 + H), W_hh=g("W_hh", (4 * H, H)) / np.sqrt(H),
               W1=g("W1", (E, H)) / np.sqrt(H), b1=0.1 * g("b1", (E,)), w2=g("w2", (E,)) / np.sqrt(E), b2=0.1 * g("b2", (1,)),
               h0=0.5 * g("h0", (B, H)), c0=0.5 * g("c0", (B, H)))
    if not feedback:
        inp["w_p"] = np.zeros(4 * H)
    return inp, g("w", (T, B))


def _run_fb(inp, w, dev, p_init=P_INIT):
    from multimodal_transformer_amd import functional as F
    ts = {k: torch.tensor(v, dtype=torch.float32, device=dev).requires_grad_() for k, v in inp.items()}
    p_all, h_all, c_all, u_all = F.lstm_fb_scan(*[ts[k] for k in KEYS], p_init=p_init, return_states=True)
    p_all.backward(torch.tensor(w, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    out = {"p_all": p_all, "h_all": h_all, "c_all": c_all, "u_all": u_all}
    out.update({"d" + k: t.grad for k, t in ts.items()})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _reference(inp, w, p_init=P_INIT):
    p_all, h_all, c_all, acts, u_all = FB.forward(**inp, p_init=p_init)
    g = FB.backward(w, inp["w_p"], inp["W_hh"], inp["W1"], inp["w2"], inp["h0"], inp["c0"], p_init, p_all, h_all, c_all, acts, u_all)
    out = dict(p_all=p_all, h_all=h_all, c_all=c_all, u_all=u_all)
    out.update({"d" + k: g["d" + k] for k in KEYS})
    return out


SCAN_CASES = [  # (T, B, H, E)
    (1, 1, 4, 4), (1, 3, 128, 128), (2, 2, 40, 24), (2, 3, 4, 128), (PF + 1, 3, 64, 40), (PF + 1, 1, 128, 64),
    (13, 1, 128, 128), (13, 3, 40, 4), (13, 2, 64, 128),
    (2, 257, 40, 24),                                   # two sequences per workgroup; the last workgroup holds one live sequence
]
RELU_KEYS = ("dW1", "db1")                              # gradients behind the read-out's ReLU mask


@pytest.mark.parametrize("T,B,H,E", SCAN_CASES, ids=["T%d_B%d_H%d_E%d" % c for c in SCAN_CASES])
def test_fb_scan_against_fp64(dev, T, B, H, E):
    inp, w = _scan_inputs(T, B, H, E, "%d_%d_%d_%d" % (T, B, H, E))
    got, ref = _run_fb(inp, w, dev), _reference(inp, w)
    failures = []
    tag = "T%d B%d H%d E%d " % (T, B, H, E)
    for k in ("p_all", "h_all", "c_all", "u_all"):
        check(tag + k, got[k], ref[k], OUT_RTOL, failures=failures)
    for k in KEYS:
        check(tag + "d" + k, got["d" + k], ref["d" + k], RELU_GRAD_RTOL if "d" + k in RELU_KEYS else GRAD_RTOL, failures=failures)
    assert not failures, failures


def test_fb_scan_du_against_fp64(dev):
    """du (T,B,E), the gradient of the read-out's pre-activations, is not an autograd output: it is read through db1 = its column sums
    above, and here through the C entry point's own buffer (dp too)."""
    from multimodal_transformer_amd import _lib
    T, B, H, E = 13, 2, 64, 40
    inp, w = _scan_inputs(T, B, H, E, "du")
    p_all, h_all, c_all, acts, u_all = FB.forward(**inp, p_init=P_INIT)
    g = FB.backward(w, inp["w_p"], inp["W_hh"], inp["W1"], inp["w2"], inp["h0"], inp["c0"], P_INIT, p_all, h_all, c_all, acts, u_all)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)       # noqa: E731
    z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)                           # noqa: E731
    nbytes = _lib.load().mmt_lstm_fb_scan_workspace_bytes(H, E)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dG, du, dp, dh0, dc0 = z(T, B, 4 * H), z(T, B, E), z(T, B), z(B, H), z(B, H)
    # the saved tensors of an exact forward: du's ReLU mask is then the reference's, and the comparison sees the backward alone
    _lib.launch("mmt_lstm_fb_scan_backward", t(w), t(inp["w_p"]), t(inp["W_hh"]), t(inp["W1"]), t(inp["w2"]), t(inp["c0"]), t(c_all), t(acts),
                t(u_all), dG, du, dp, dh0, dc0, ws, nbytes, T, B, H, E)
    torch.cuda.synchronize()
    failures = []
    check("du", du.cpu().numpy(), g["du"], RELU_GRAD_RTOL, failures=failures)
    check("dp", dp.cpu().numpy(), g["dp"], GRAD_RTOL, failures=failures)
    check("dG", dG.cpu().numpy(), g["dgxc"], GRAD_RTOL, failures=failures)
    assert not failures, failures


@pytest.mark.parametrize("H", [64, 128])
def test_fb_without_feedback_against_existing_kernels(dev, H):
    """w_p = 0: the scan is lstm_scan -> linear(ReLU) -> linear.  Same inputs through both; both against fp64; the scan's rel-L2 error may
    be at most 2 x the composition's (same bf16 rounding sites: 2 covers ordering noise)."""
    from multimodal_transformer_amd import functional as F
    T, B, E = 13, 2, 64
    inp, w = _scan_inputs(T, B, H, E, "compose%d" % H, feedback=False)
    ref = _reference(inp, w)
    got = _run_fb(inp, w, dev)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev).requires_grad_()       # noqa: E731
    ts = {k: t(inp[k]) for k in KEYS if k != "w_p"}
    h, c = F.lstm_scan(ts["gxc"], ts["W_hh"], ts["h0"], ts["c0"])
    u = F.linear(h, ts["W1"], ts["b1"], act=1)
    p = F.linear(u, ts["w2"].reshape(1, E), ts["b2"])
    p.backward(torch.tensor(w, dtype=torch.float32, device=dev).reshape(T, B, 1))
    torch.cuda.synchronize()
    n = lambda a: a.detach().cpu().numpy()                                                                      # noqa: E731
    pairs = {"p_all": (got["p_all"], n(p).reshape(T, B), ref["p_all"]), "h_all": (got["h_all"], n(h), ref["h_all"]),
             "c_all": (got["c_all"], n(c), ref["c_all"]), "u_all": (got["u_all"], n(u), ref["u_all"])}
    for k in KEYS:
        if k != "w_p":
            pairs["d" + k] = (got["d" + k], n(ts[k].grad).reshape(ref["d" + k].shape), ref["d" + k])
    bad = []
    for k, (a, b, r) in pairs.items():
        ea, eb = rel_l2(a, r), rel_l2(b, r)
        print("H=%-4d %-8s scan %.3e  composition %.3e  ratio %.2f" % (H, k, ea, eb, ea / max(eb, 1e-30)))
        if ea > 2.0 * eb:
            bad.append((k, ea, eb))
    assert not bad, bad


def test_feedback_is_live(dev):
    T, B, H, E = 5, 2, 40, 24
    inp, w = _scan_inputs(T, B, H, E, "live")
    a, b = _run_fb(inp, w, dev, p_init=0.375), _run_fb(inp, w, dev, p_init=-0.5)
    assert rel_l2(b["p_all"][0], a["p_all"][0]) > OUT_RTOL, "tgt_init does not reach step 0"
    off = _run_fb(dict(inp, w_p=np.zeros(4 * H)), w, dev)
    assert rel_l2(off["p_all"], a["p_all"]) > OUT_RTOL, "the fed-back prediction does not reach the gates"
    assert np.abs(a["dw_p"]).max() > 0 and np.abs(off["dw_p"]).max() > 0


@pytest.mark.parametrize("T,B,H,E", [(2, 1, 256, 8), (2, 1, 8, 132), (1, 513, 4, 4)], ids=["H256", "E132", "B513"])
def test_limits_are_refused_before_any_launch(dev, T, B, H, E):
    from multimodal_transformer_amd import functional as F
    z = lambda *s: torch.zeros(*s, device=dev)                                                                   # noqa: E731
    args = (z(T, B, 4 * H), z(4 * H), z(4 * H, H), z(E, H), z(E), z(E), z(1), z(B, H), z(B, H))
    torch.cuda.synchronize()
    _, names = device_kernel_names(lambda: pytest.raises(NotImplementedError, F.lstm_fb_scan, *args))
    assert not names, names


def test_two_decoder_layers_are_refused_before_any_launch(dev):
    from multimodal_transformer_amd.models import MultiEDLSTM
    model = MultiEDLSTM(48, embed_dim=64, h_dim=32, n_layers=2, device=dev).eval()
    x, lengths = torch.zeros(2, 3, 48, device=dev), [3, 2]
    mask = R.prefix_mask(lengths, 3).to(dev)
    torch.cuda.synchronize()
    _, names = device_kernel_names(lambda: pytest.raises(NotImplementedError, model, x, mask, lengths))
    assert not names, names


def test_two_runs_are_bit_identical(dev):
    inp, w = _scan_inputs(13, 3, 40, 24, "repro")
    a, b = _run_fb(inp, w, dev), _run_fb(inp, w, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- train step
def _setup(dev):
    from multimodal_transformer_amd.models import MultiEDLSTM
    B, T, D = 3, 12, 48
    model = MultiEDLSTM(D, embed_dim=64, h_dim=32, device=dev)
    load_named(model, 3)
    model.train()
    lengths = [12, 9, 4]
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("edtrain:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    x = R.gen_normal("edtrain:x", (B, T, D), 3).to(dev)
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
    model, x, lengths, mask, tgt = _setup(dev)
    step, params = _step_fn(model, lambda: model(x, mask, lengths, tgt_init=0.25), tgt, lengths)
    names = device_kernel_names(step, warm=True)[1]
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    if names is None:
        pytest.skip("torch.profiler reports no device kernels here")
    assert any("lstm_fb_scan_fwd" in n for n in names) and any("lstm_fb_scan_bwd" in n for n in names), names
    assert library_kernels(names) == [], "library kernels in a MultiEDLSTM train step: %s" % library_kernels(names)


def test_train_step_hipgraph_replay_equals_eager(dev, monkeypatch):
    """As test_gpu_lstm_stack.py::test_train_step_hipgraph_replay_equals_eager, for MultiEDLSTM."""
    from multimodal_transformer_amd import graphs, functional as F
    monkeypatch.setenv("MMT_DEVICE_SEED", "1")
    model, x, lengths, mask, tgt = _setup(dev)
    step, params = _step_fn(model, lambda: model(x, mask, lengths, tgt_init=0.25), tgt, lengths)
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
