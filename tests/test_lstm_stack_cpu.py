"""CPU: the fp64 restatement of the stacked LSTM recurrence (tests/lstm_stack_ref.py) against the reference's own runs.

The fixtures of tests/golden/make_golden_stacked.py are fp32 eval-mode runs of the reference's models with n_layers > 1 and recipe
weights (non-zero dec_h0 / dec_c0).  The same models restated in fp64 around lstm_stack_ref's numpy recurrence — forward and the
hand-derived backward — must reproduce output, loss and every stored gradient to fp32 round-off (rel-L2 <= 1e-5): that pins the helper
the GPU tests measure the kernels against, before anything runs on a GPU.  And the fixtures tell o_{-1} = 0 from o_{-1} = dec_h0[L-1].
"""
import numpy as np
import pytest
import torch

import lstm_stack_ref as S
import recipe as R
import stacked_cases as C
from conftest import load_golden, rel_l2

PIN_RTOL = 1e-5


def _params(name, shapes_from):
    p32 = R.gen_params(shapes_from, R.SEED)
    fx = load_golden(name)
    assert abs(R.weights_checksum(p32) - float(fx["checksum"])) <= 1e-6 * float(fx["checksum"]), "recipe weights differ from the fixture's"
    return {k: v.double().requires_grad_() for k, v in p32.items()}, fx


def _decoder_shapes(cls, D, embed_dim=256, h_dim=128, N=6, d_ff=128, h=8, n_layers=1):
    """state_dict names and shapes of the reference's NLPTransformer / UniTransformer (tests/golden/reference_surface.json order is not
    needed: the recipe draws every tensor from its name)"""
    d = embed_dim
    s = {("embed.1" if cls == "NLPTransformer" else "embed") + ".weight": (d, D), ("embed.1" if cls == "NLPTransformer" else "embed") + ".bias": (d,)}
    for i in range(N):
        for j in range(4):
            s["encoder.layers.%d.self_attn.linears.%d.weight" % (i, j)] = (d, d)
            s["encoder.layers.%d.self_attn.linears.%d.bias" % (i, j)] = (d,)
        s["encoder.layers.%d.feed_forward.w_1.weight" % i] = (d_ff, d)
        s["encoder.layers.%d.feed_forward.w_1.bias" % i] = (d_ff,)
        s["encoder.layers.%d.feed_forward.w_2.weight" % i] = (d, d_ff)
        s["encoder.layers.%d.feed_forward.w_2.bias" % i] = (d,)
        for j in range(2):
            s["encoder.layers.%d.sublayer.%d.norm.a_2" % (i, j)] = (d,)
            s["encoder.layers.%d.sublayer.%d.norm.b_2" % (i, j)] = (d,)
    s["encoder.norm.a_2"], s["encoder.norm.b_2"] = (d,), (d,)
    s["dec_h0"], s["dec_c0"] = (n_layers, 1, d), (n_layers, 1, d)
    for l in range(n_layers):
        s["decoder.weight_ih_l%d" % l] = (4 * d, 2 * d if l == 0 else d)
        s["decoder.weight_hh_l%d" % l] = (4 * d, d)
        s["decoder.bias_ih_l%d" % l], s["decoder.bias_hh_l%d" % l] = (4 * d,), (4 * d,)
    s["out.0.weight"], s["out.0.bias"], s["out.2.weight"], s["out.2.bias"] = (h_dim, d), (h_dim,), (1, h_dim), (1,)
    return s


def _baseline_shapes(cls, D, embed_dim=None, h_dim=256, n_layers=1, attn_len=5):
    E = embed_dim or (128 if cls == "MultiLSTM" else 512)
    last = "decoder.2" if cls == "MultiLSTM" else "decoder.3"
    s = {"embed.1.weight": (E, D), "embed.1.bias": (E,), "attn.0.weight": (E, E), "attn.0.bias": (E,),
         "attn.2.weight": (attn_len, E), "attn.2.bias": (attn_len,)}
    for l in range(n_layers):
        s["lstm.weight_ih_l%d" % l] = (4 * h_dim, E if l == 0 else h_dim)
        s["lstm.weight_hh_l%d" % l] = (4 * h_dim, h_dim)
        s["lstm.bias_ih_l%d" % l], s["lstm.bias_hh_l%d" % l] = (4 * h_dim,), (4 * h_dim,)
    s["decoder.0.weight"], s["decoder.0.bias"], s[last + ".weight"], s[last + ".bias"] = (E, h_dim), (E,), (1, E), (1,)
    return s, last


def _loss(name, out, lengths, T):
    mask = R.prefix_mask(lengths, T)
    target = (R.gen_uniform(name + ":target", (len(lengths), T, 1), R.SEED) * mask).double()
    return ((out - target) ** 2).sum() / float(sum(lengths))


def _compare(name, p, fx, out, loss):
    r = rel_l2(out.detach().numpy(), fx["out"])
    print("%-20s out rel-L2 %.2e  loss %.8f (fixture %.8f)" % (name, r, loss.item(), float(fx["loss"])))
    assert r <= PIN_RTOL
    assert abs(loss.item() - float(fx["loss"])) <= PIN_RTOL * abs(float(fx["loss"]))
    loss.backward()
    assert sorted(k[6:] for k in fx if k.startswith("gnorm:")) == sorted(p), "the restated state_dict is not the reference's"
    top = max(float(fx[k]) for k in fx if k.startswith("gnorm:"))
    for k in fx:
        if k.startswith("gnorm:"):
            got = float(p[k[6:]].grad.pow(2).sum().sqrt()) if p[k[6:]].grad is not None else -1.0
            assert abs(got - float(fx[k])) <= PIN_RTOL * float(fx[k]) + 1e-7 * top, (k, got, float(fx[k]))    # 1e-7: fp32 cancellation in tiny norms
        if k.startswith("grad:"):
            got, ref = p[k[5:]].grad.numpy(), fx[k].astype(np.float64)
            if np.linalg.norm(ref) < 1e-6 * top:
                # analytically zero (the key projection's bias: the softmax is shift-invariant); the fixture holds fp32 round-off, so the
                # difference is measured against the largest gradient norm of the model instead of against that noise
                g = float(np.linalg.norm(got - ref) / top)
            else:
                g = rel_l2(got, ref)
            print("%-20s %-50s rel-L2 %.2e" % (name, k, g))
            assert g <= PIN_RTOL, (k, g)


@pytest.mark.parametrize("case", C.DECODER_CASES, ids=[c[0] for c in C.DECODER_CASES])
def test_decoder_models_match_reference_fixtures(case):
    name, cls, _, D, kw, lengths, T = case
    p, fx = _params(name, _decoder_shapes(cls, D, **kw))
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).double()
    out = S.decoder_model(p, x, R.prefix_mask(lengths, T), kw["h"], kw["n_layers"], relu_embed=cls == "NLPTransformer")
    _compare(name, p, fx, out, _loss(name, out, lengths, T))


@pytest.mark.parametrize("case", C.BASELINE_CASES, ids=[c[0] for c in C.BASELINE_CASES])
def test_baseline_models_match_reference_fixtures(case):
    name, cls, _, D, kw, lengths, T = case
    shapes, last = _baseline_shapes(cls, D, **kw)
    p, fx = _params(name, shapes)
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).double()
    out = S.lstm_baseline(p, x, R.prefix_mask(lengths, T), kw["n_layers"], last=last)
    _compare(name, p, fx, out, _loss(name, out, lengths, T))


@pytest.mark.parametrize("case", C.DECODER_CASES[:2], ids=[c[0] for c in C.DECODER_CASES[:2]])
def test_fixtures_distinguish_zero_feedback_from_dec_h0(case):
    """o_{-1} is zeros (transformer/SFT/multiTransformer.py:469), not dec_h0[L-1]: the wrong reading misses the fixture by far more
    than the pin bound, in the output and in dec_h0's gradient."""
    name, cls, _, D, kw, lengths, T = case
    p, fx = _params(name, _decoder_shapes(cls, D, **kw))
    x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED).double()
    out = S.decoder_model(p, x, R.prefix_mask(lengths, T), kw["h"], kw["n_layers"], relu_embed=True, o_init="h0_top")
    r = rel_l2(out.detach().numpy(), fx["out"])
    _loss(name, out, lengths, T).backward()
    g = rel_l2(p["dec_h0"].grad.numpy(), fx["grad:dec_h0"])
    print("%-20s wrong o_{-1}: out rel-L2 %.2e  dec_h0 grad rel-L2 %.2e" % (name, r, g))
    assert r > 100 * PIN_RTOL and g > 100 * PIN_RTOL


def test_backward_matches_finite_differences():
    """the hand-derived backward against central differences of the forward, every input, L = 3 (independent of torch and the fixtures)"""
    rng = np.random.default_rng(5)
    T, B, H, L = 3, 2, 4, 3
    gx0, P = rng.standard_normal((T, B, 4 * H)), rng.standard_normal((L, 4 * H, 2 * H)) / np.sqrt(2 * H)
    bias, h0, c0 = 0.1 * rng.standard_normal((L - 1, 4 * H)), 0.5 * rng.standard_normal((L, B, H)), 0.5 * rng.standard_normal((L, B, H))
    w = rng.standard_normal((T, B, H))
    args = dict(gx0=gx0, P=P, bias=bias, h0=h0, c0=c0)
    g = S.backward(w, P, h0, c0, *S.forward(**args))
    for key, gk in (("gx0", "dgx0"), ("P", "dP"), ("bias", "dbias"), ("h0", "dh0"), ("c0", "dc0")):
        num = np.zeros_like(args[key])
        for idx in np.ndindex(*args[key].shape):
            vals = []
            for s in (1e-6, -1e-6):
                a = {k: v.copy() for k, v in args.items()}
                a[key][idx] += s
                vals.append((S.forward(**a)[0][-1] * w).sum())
            num[idx] = (vals[0] - vals[1]) / 2e-6
        assert rel_l2(g[gk], num) < 1e-7, (key, rel_l2(g[gk], num))


def test_bf16_mode_is_close_and_different():
    rng = np.random.default_rng(6)
    T, B, H, L = 5, 2, 8, 2
    gx0, P = rng.standard_normal((T, B, 4 * H)), rng.standard_normal((L, 4 * H, 2 * H)) / np.sqrt(2 * H)
    bias = 0.1 * rng.standard_normal((L - 1, 4 * H))
    a, b = S.forward(gx0, P, bias)[0], S.forward(gx0, P, bias, bf16=True)[0]
    assert 1e-5 < rel_l2(b, a) < 2e-2
