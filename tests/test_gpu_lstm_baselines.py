"""GPU: the LSTM baselines (B1-LSTM's MultiCNNLSTM, both MultiLSTM copies) and B3-MFN on the HIP path.

* functional.local_attention (csrc/local_attn.h) against an fp64 torch restatement of the reference's softmax(dim=1) + pad_packed
  zeroing + convolve (transformer/B1-LSTM/models.py:10-25,186-207), forward and both gradients, and bit-identical on a second run;
* the models against the fixtures of tests/golden/make_golden_lstm.py (eval mode, the tolerances of gpu_harness.py);
* a train-mode step: finite, not the eval result, repeatable from the same generator state, hand-written kernels only, and the same
  bits when replayed from a hipGraph.
"""
import numpy as np
import pytest
import torch

import lstm_cases as C
import recipe as R
from conftest import load_golden, rel_l2
from gpu_harness import OUT_RTOL, RELU_GRAD_RTOL, CCC_MIN, dev, device_kernel_names, library_kernels  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

LA_RTOL = 1e-5


def _local_attention_fp64(z, h, valid):
    """z (B,T,L), h (T,B,H), valid (B,T): the reference's computation restated in fp64"""
    B, T, L = z.shape
    a = torch.softmax(z, dim=1)                                        # over TIME, padded steps included
    hb = h.permute(1, 0, 2) * valid.unsqueeze(-1)                      # pad_packed_sequence's zeros
    out = torch.zeros(B, T, h.shape[2], dtype=z.dtype)
    for i in range(L):
        if i < T:
            out[:, i:, :] = out[:, i:, :] + a[:, i:, i:i + 1] * hb[:, :T - i, :]
    return out


def _lengths(B, T, ragged):
    if not ragged:
        return [T] * B
    return [max(1, T - (T * k) // (B + 1)) for k in range(B)]


def _la_inputs(B, T, H, L, ragged, tag):
    z = R.gen_normal("la:%s:z" % tag, (B, T, L), 5) * 2.0
    h = torch.tanh(R.gen_normal("la:%s:h" % tag, (T, B, H), 5))
    valid = R.prefix_mask(_lengths(B, T, ragged), T).reshape(B, T)
    g = R.gen_normal("la:%s:g" % tag, (B, T, H), 5)
    return z, h, valid, g


LA_CASES = [  # (B, T, H, L, ragged)
    (1, 1, 256, 1, False), (1, 3, 130, 5, True), (3, 3, 1024, 7, True), (3, 37, 256, 5, True), (3, 37, 130, 16, True),
    (3, 1, 130, 3, True), (25, 37, 1024, 1, True), (1, 500, 1024, 3, False), (25, 500, 256, 5, True), (25, 500, 256, 16, False),
    (3, 500, 130, 7, True), (25, 3, 256, 16, True),
]


@pytest.mark.parametrize("B,T,H,L,ragged", LA_CASES, ids=["B%d_T%d_H%d_L%d_%s" % (c[:4] + ("ragged" if c[4] else "full",)) for c in LA_CASES])
def test_local_attention_against_fp64(dev, B, T, H, L, ragged):
    from multimodal_transformer_amd import functional as F
    z, h, valid, g = _la_inputs(B, T, H, L, ragged, "%d_%d_%d_%d" % (B, T, H, L))
    zs, hs = z.to(dev).requires_grad_(), h.to(dev).requires_grad_()
    out = F.local_attention(zs, hs, valid.to(dev).reshape(B, T, 1))
    out.backward(g.to(dev))
    zd, hd = z.double().requires_grad_(), h.double().requires_grad_()
    ref = _local_attention_fp64(zd, hd, valid.double())
    ref.backward(g.double())
    e_out = rel_l2(out.detach().cpu().numpy(), ref.detach().numpy())
    e_dz = rel_l2(zs.grad.cpu().numpy(), zd.grad.numpy())
    e_dh = rel_l2(hs.grad.cpu().numpy(), hd.grad.numpy())
    print("local_attention B=%d T=%d H=%d L=%d %s: ctx %.2e dz %.2e dh %.2e" % (B, T, H, L, "ragged" if ragged else "full", e_out, e_dz, e_dh))
    assert e_out < LA_RTOL and e_dz < LA_RTOL and e_dh < LA_RTOL
    pad = valid == 0
    assert (hs.grad.cpu().permute(1, 0, 2)[pad] == 0).all(), "no gradient into h at padded steps"


def test_local_attention_is_bit_reproducible(dev):
    from multimodal_transformer_amd import functional as F
    B, T, H, L = 25, 500, 256, 5
    z, h, valid, g = _la_inputs(B, T, H, L, True, "repro")
    runs = []
    for _ in range(2):
        zs, hs = z.to(dev).requires_grad_(), h.to(dev).requires_grad_()
        out = F.local_attention(zs, hs, valid.to(dev))
        out.backward(g.to(dev))
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), zs.grad.cpu(), hs.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- model parity
def _model(cls, dev):
    from multimodal_transformer_amd import models as M, multiTransformer as MT
    if cls == "MultiLSTM":
        return lambda D: M.MultiLSTM(D, device=dev)
    if cls == "MultiLSTMB1":
        return lambda D: M.MultiLSTMB1(D, device=dev)
    if cls == "MultiCNNLSTM":
        return lambda mods, dims: M.MultiCNNLSTM(mods, dims, device=dev)
    if cls == "MultiCNNLSTM:checkpoint":
        return lambda mods, dims: M.MultiCNNLSTM(mods, dims, window_embed_size={"linguistic": 300}, lstm_cls=M.MultiLSTM, device=dev)
    if cls == "MultiCNNTransformerB3":
        return lambda mods, dims: M.MultiCNNTransformerB3(mods, dims, device=dev)
    return lambda: MT.MultiTransformerB3(R.MODS_AVL, R.EMBED_AVL, device=dev)


def _check_against_fixture(name, model, out, loss, lengths):
    from multimodal_transformer_amd import eval_ccc
    fx = load_golden(name)
    o = out.detach().cpu().numpy()
    r = rel_l2(o, fx["out"])
    print("%-22s valence rel_l2 %.3e  loss %.6f (ref %.6f)" % (name, r, loss.item(), float(fx["loss"])))
    assert o.shape == fx["out"].shape and r < OUT_RTOL
    T = o.shape[1]
    mask = R.prefix_mask(lengths, T).numpy()
    assert (o[mask == 0] == 0).all()
    rms = float(np.sqrt((fx["out"].astype(np.float64) ** 2).mean()))
    for b, n in enumerate(lengths):
        ref_b = fx["out"][b, :n, 0].astype(np.float64)
        ccc = eval_ccc(ref_b, o[b, :n, 0].astype(np.float64))
        # 1 - CCC ~ mse / (2 var): on a sequence flatter than the output tolerance resolves, the deficit that tolerance allows is larger than
        # 1e-3 (lstm_shared_e128: per-sequence std 1.1e-3 at output RMS 6.2e-3; measured CCC 0.9983 at rel-L2 7.2e-3, bf16 GEMM operands)
        floor = (OUT_RTOL * rms) ** 2 / (2.0 * max(float(ref_b.var()), 1e-30))
        assert ccc >= min(CCC_MIN, 1.0 - floor), (name, b, ccc, floor)
    assert abs(loss.item() - float(fx["loss"])) < 2e-2 * max(abs(float(fx["loss"])), 1e-3)
    floor = 1e-3 * max(float(fx[k]) for k in fx if k.startswith("gnorm:"))
    worst = 0.0
    params = dict(model.named_parameters())
    for n, p in params.items():
        ref = float(fx["gnorm:" + n])
        if ref < 0:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, n
            continue
        assert p.grad is not None, n
        got = float(p.grad.double().pow(2).sum().sqrt())
        if ref > floor:
            worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= RELU_GRAD_RTOL * ref + floor, (n, got, ref)
    for k in fx:
        if k.startswith("grad:"):
            got = params[k[5:]].grad.cpu().numpy()
            assert rel_l2(got, fx[k]) < RELU_GRAD_RTOL + floor / max(float(np.linalg.norm(fx[k])), 1e-30), k
    print("%-22s worst |grad-norm| deviation %.3e" % (name, worst))


def _run(name, model, call, lengths, T, dev):
    p32 = R.gen_params(R.shapes_of(model.state_dict()), R.SEED)
    model.load_state_dict(p32)
    fx = load_golden(name)
    assert abs(R.weights_checksum(p32) - float(fx["checksum"])) <= 1e-6 * float(fx["checksum"]), "state_dict differs from the reference's"
    model = model.to(dev).eval()
    mask = R.prefix_mask(lengths, T)
    target = (R.gen_uniform(name + ":target", (len(lengths), T, 1), R.SEED) * mask).to(dev)
    out = call(model, mask.to(dev))
    loss = ((out - target) ** 2).sum() / float(sum(lengths))
    loss.backward()
    _check_against_fixture(name, model, out, loss, lengths)


@pytest.mark.parametrize("case", C.LSTM_SEQ_CASES, ids=[c[0] for c in C.LSTM_SEQ_CASES])
def test_lstm_sequence_model_golden(dev, case):
    name, cls, D, lengths, T = case
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).to(dev)
    _run(name, _model(cls, dev)(D), lambda m, mask: m(x, mask, lengths), lengths, T, dev)


@pytest.mark.parametrize("case", C.LSTM_WINDOW_CASES, ids=[c[0] for c in C.LSTM_WINDOW_CASES])
def test_window_model_golden(dev, case):
    name, cls, mods, dims, lengths, T, W = case
    x = {m: R.gen_normal("%s:%s" % (name, m), (len(lengths), T, W[m], dims[m]), R.SEED).to(dev) for m in mods}
    _run(name, _model(cls, dev)(mods, dims), lambda m, mask: m(x, lengths, mask), lengths, T, dev)


def test_b3_sequence_model_golden(dev):
    name, lengths, T = C.B3_SEQ_CASE
    x = {m: R.gen_normal("%s:%s" % (name, m), (len(lengths), T, R.EMBED_AVL[m]), R.SEED).to(dev) for m in R.MODS_AVL}
    _run(name, _model("MultiTransformerB3", dev)(), lambda m, mask: m(x, mask, lengths), lengths, T, dev)


# ---------------------------------------------------------------------------------------------------------------- train mode
def _b1_setup(dev, mods=("linguistic",), B=3, T=12):
    from multimodal_transformer_amd import models as M
    dims = {"acoustic": 88, "linguistic": 300}
    wl = {"acoustic": 6, "linguistic": 7}
    model = M.MultiCNNLSTM(list(mods), {m: dims[m] for m in mods}, device=dev)
    p32 = R.gen_params(R.shapes_of(model.state_dict()), 3)
    model.load_state_dict(p32)
    lengths = [T, T - 3, 4][:B]
    mask = R.prefix_mask(lengths, T).to(dev)
    tgt = (R.gen_uniform("b1train:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
    x = {m: R.gen_normal("b1train:" + m, (B, T, wl[m], dims[m]), 3).to(dev) for m in mods}
    return model, x, lengths, mask, tgt


def _step_fn(model, x, lengths, mask, tgt):
    from multimodal_transformer_amd import functional as F
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        out = model(x, lengths, mask)
        F.mse_sum_loss_backward(out, tgt, sum(lengths))
        return out
    return step, params


def test_train_step_finite_differs_from_eval_and_repeats(dev):
    model, x, lengths, mask, tgt = _b1_setup(dev)
    step, params = _step_fn(model, x, lengths, mask, tgt)
    model.eval()
    y_eval = step().detach().clone()
    model.train()
    step()                                              # first train call: the modules' dropout seed states are created
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        y = step().detach().clone()
        torch.cuda.synchronize()
        runs.append((y, [p.grad.detach().clone() for p in params]))
    y, grads = runs[0]
    assert torch.isfinite(y).all() and all(torch.isfinite(g).all() for g in grads)
    assert not torch.equal(y, y_eval)
    assert float((y - y_eval).abs().max()) > 1e-4
    assert torch.equal(runs[1][0], y)
    for a, b in zip(runs[1][1], grads):
        assert torch.equal(a, b)
    assert (y.cpu()[R.prefix_mask(lengths, y.shape[1]) == 0] == 0).all()


@pytest.mark.parametrize("which", ["b1", "b3"])
def test_train_step_runs_no_library_kernel(dev, which):
    from multimodal_transformer_amd import models as M
    if which == "b1":
        model, x, lengths, mask, tgt = _b1_setup(dev, mods=("acoustic", "linguistic"))
    else:
        mods, dims, wl = ["acoustic", "linguistic"], {"acoustic": 88, "linguistic": 300}, {"acoustic": 6, "linguistic": 7}
        model = M.MultiCNNTransformerB3(mods, dims, device=dev)
        B, T = 3, 12
        lengths = [12, 9, 4]
        mask = R.prefix_mask(lengths, T).to(dev)
        tgt = (R.gen_uniform("b3nolib:t", (B, T, 1), 3) * R.prefix_mask(lengths, T)).to(dev)
        x = {m: R.gen_normal("b3nolib:" + m, (B, T, wl[m], dims[m]), 3).to(dev) for m in mods}
    model.train()
    step, params = _step_fn(model, x, lengths, mask, tgt)
    names = device_kernel_names(step, warm=True)[1]
    if names is None:
        pytest.skip("torch.profiler reports no device kernels here")
    assert len([n for n in names if "kernel" in n]) > 10, names[:10]
    if which == "b1":
        assert any("local_attn" in n for n in names)
    assert library_kernels(names) == [], "library kernels in a %s train step: %s" % (which, library_kernels(names))
    for p in params:
        assert p.grad is None or torch.isfinite(p.grad).all()


def test_b1_train_step_hipgraph_replay_equals_eager(dev, monkeypatch):
    """A train-mode B1 step captured with graphs.capture_step and replayed from the same dropout seed states gives the eager step's bits.
    MMT_DEVICE_SEED=1: the eager steps also read the device-resident seeds a captured step reads, so both draw the same masks."""
    from multimodal_transformer_amd import graphs, functional as F
    monkeypatch.setenv("MMT_DEVICE_SEED", "1")
    model, x, lengths, mask, tgt = _b1_setup(dev)
    model.train()
    step, params = _step_fn(model, x, lengths, mask, tgt)
    step()                                              # creates the seed states
    seeds = [ds.state for m in model.modules() for ds in m.__dict__.get("_dev_seeds", {}).values()]
    assert len(seeds) >= 3                               # front-end Dropout(0.3), embed dropout, decoder dropout
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
