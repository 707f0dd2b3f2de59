"""CPU: the reference of causal attention (tests/causal_ref.py) against the exact function, and the surface of the feature
(mmt_*_causal, the ``causal`` keyword of functional, MultiHeadedAttention.causal, multiTransformer.causal_attention).  No GPU: the library
is loaded, nothing is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import bf16_ref as E
import causal_ref as C
import recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = ["mmt_sdpa_forward_causal", "mmt_sdpa_backward_causal", "mmt_attn_probs_forward_causal", "mmt_encoder_forward_causal",
          "mmt_encoder_backward_causal", "mmt_encoder_forward_causal_devseed", "mmt_encoder_backward_causal_devseed"]


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def _inputs(T, d, lengths):
    B = len(lengths)
    q, k, v, g = (R.gen_normal("causal_cpu" + n, (B, T, d), 5).double() for n in "qkvg")
    return q, k, v, g, R.prefix_mask(lengths, T).double()


def test_the_reference_is_the_exact_function():
    """causal_ref.sdpa(rounding=False) == torch.softmax over scores with -inf above the diagonal, in fp64 to 1e-12: values and the three
    gradients, blanked query rows (Q' = 0: uniform over the t + 1 visible keys, no gradient to q) included"""
    T, d, h, lengths = 70, 40, 4, [70, 33, 1]
    dk = d // h
    q, k, v, g, rowm = _inputs(T, d, lengths)
    a = [t.clone().requires_grad_() for t in (q, k, v)]
    ctx, _ = C.sdpa(*(_split(t, h) for t in a), rowm.unsqueeze(1), None, rounding=False)
    ctx.permute(0, 2, 1, 3).reshape(len(lengths), T, d).backward(g)
    b = [t.clone().requires_grad_() for t in (q, k, v)]
    Q, K, V = (_split(t, h) for t in b)
    S = (Q * rowm.unsqueeze(1)) @ K.transpose(-2, -1) / dk ** 0.5
    P = torch.softmax(S.masked_fill(C.above_diagonal(T), float("-inf")), dim=-1)
    assert (P.masked_select(C.above_diagonal(T).expand_as(P)) == 0).all()
    direct = P @ V
    direct.permute(0, 2, 1, 3).reshape(len(lengths), T, d).backward(g)
    assert (ctx - direct).abs().max().item() <= 1e-12
    for name, x, y in zip("qkv", a, b):
        assert (x.grad - y.grad).abs().max().item() <= 1e-12, name
    for bi, n in enumerate(lengths):
        assert (a[0].grad[bi, n:] == 0).all()
        for t in range(n, T):
            assert (P[bi, :, t, :t + 1] - 1.0 / (t + 1)).abs().max().item() <= 1e-15
    assert (ctx[:, :, 0] - _split(v, h)[:, :, 0]).abs().max().item() <= 1e-15       # row 0 attends one key


def test_truncation_identity():
    """row t of causal attention == row t of plain bf16_ref.sdpa(rounding=False) on the sequence cut to t + 1 windows, to 1e-12"""
    T, d, h = 40, 16, 2
    q, k, v, _, _ = _inputs(T, d, [T, T])
    ctx, _ = C.sdpa(_split(q, h), _split(k, h), _split(v, h), None, None, rounding=False)
    for t in range(T):
        cut, _ = E.sdpa(_split(q[:, :t + 1], h), _split(k[:, :t + 1], h), _split(v[:, :t + 1], h), None, None, rounding=False)
        assert (ctx[:, :, t] - cut[:, :, t]).abs().max().item() <= 1e-12, t


def test_rounded_reference_stays_near_the_exact_function():
    """the bf16 roundings move the causal reference by what they move the plain one: well under 2 % rel-L2 on values and gradients
    (a wrong tile sweep or a mask taken after the maximum moves them by tens of percent)"""
    T, d, h, lengths = 70, 40, 4, [70, 33]
    q, k, v, g, rowm = _inputs(T, d, lengths)
    res = []
    for rounding in (True, False):
        a = [t.clone().requires_grad_() for t in (q, k, v)]
        ctx, _ = C.sdpa(*(_split(t, h) for t in a), rowm.unsqueeze(1), None, rounding=rounding)
        ctx.permute(0, 2, 1, 3).reshape(len(lengths), T, d).backward(g)
        res.append([ctx.detach()] + [t.grad for t in a])
    for x, y in zip(*res):
        assert torch.isfinite(x).all() and ((x - y).norm() / y.norm()).item() < 2e-2


def test_causal_entries_are_declared_exported_and_bound():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmt_hip.h")).read(), flags=re.S)
    for name in CAUSAL:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_causal", "")], name        # the plain entry's exact signature

        def params(n):
            return re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, header).group(1))
        assert params(name) == params(name.replace("_causal", "")), name
    assert lib.mmt_abi_version() == 1


def test_causal_entries_refuse_null_pointers():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: every refusal below comes first
    EINVAL = 1
    enc = (2, 33, 128, 8, 128, 2, 1e-6, 0.0)
    assert lib.mmt_sdpa_forward_causal(None, None, None, None, None, None, 0, 2, 33, 32, 2, 0.0, 0, None) == EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_sdpa_backward_causal(None, None, None, None, None, None, 0, 2, 33, 32, 2, 0.0, 0, None) == EINVAL
    assert lib.mmt_attn_probs_forward_causal(None, None, None, None, 2, 33, 32, 2, 0.0, 0, None) == EINVAL
    assert lib.mmt_encoder_forward_causal(None, None, None, None, None, 0, *enc, 0, None) == EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_encoder_backward_causal(None, None, None, None, None, None, None, 0, *enc, 0, None) == EINVAL
    assert lib.mmt_encoder_forward_causal_devseed(one, one, one, one, one, 1 << 30, *enc, None, None) == EINVAL
    assert b"seed state" in lib.mmt_last_error()
    assert lib.mmt_encoder_backward_causal_devseed(None, None, None, None, None, None, None, 0, *enc, None) == EINVAL
    assert lib.mmt_sdpa_forward_causal(one, one, one, one, one, one, 1 << 30, 0, 33, 32, 2, 0.0, 0, None) == EINVAL      # and the plain entry's other refusals
    assert lib.mmt_attn_probs_forward_causal(one, one, one, one, 2, 33, 33, 2, 0.0, 0, None) == EINVAL


def test_python_surface():
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    for fn in (F.sdpa, F.attn_probs, F.encoder_stack, F.encoder_stack_params):
        assert inspect.signature(fn).parameters["causal"].default is False, fn.__name__
        assert inspect.signature(fn).parameters["key_lengths"].default is None, fn.__name__
    assert inspect.signature(mt_launch()).parameters["causal"].default is False
    assert list(inspect.signature(MT.attention).parameters) == ["query", "key", "value", "mask", "dropout"]      # the reference's five
    mha = MT.MultiHeadedAttention(2, 8)
    assert MT.MultiHeadedAttention.causal is False and "causal" not in mha.__dict__
    assert MT.causal_attention(mha) == {"": mha} and mha.causal is True
    MT.causal_attention(mha, False)
    assert mha.causal is False
    model = MT.MultiTransformer(["acoustic", "emotient"], {"acoustic": 12, "emotient": 20}, N=2, d_ff=16, h=2, device=torch.device("cpu"),
                                embed_dim={"acoustic": 16, "emotient": 8})
    found = MT.causal_attention(model)
    assert len(found) == 2 * (2 + 1) and all(m.causal for m in found.values())
    assert sorted(found) == sorted(n for n, m in model.named_modules() if isinstance(m, MT.MultiHeadedAttention))
    enc = next(m for m in model.modules() if isinstance(m, MT.Encoder))
    assert enc._fusable()                                # the flag does not force the layer-by-layer path ...
    enc.layers[1].self_attn.causal = False
    assert not enc._fusable()                            # ... layers that disagree about it do
    MT.causal_attention(model, False)
    assert enc._fusable() and not any(m.causal for m in found.values())


def mt_launch():
    from multimodal_transformer_amd import _lib
    return _lib.launch


def test_causal_and_key_lengths_are_not_combined():
    """ValueError naming both, raised by the argument check, which runs on any device: nothing is launched"""
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    kl = torch.tensor([3, 1], dtype=torch.int32)
    assert F._check_causal("sdpa", None, True) is True and F._check_causal("sdpa", kl, False) is False
    assert F._check_causal("sdpa", None, 0) is False
    with pytest.raises(ValueError, match="key_lengths.*causal"):
        F._check_causal("sdpa", kl, True)
    x = torch.zeros(2, 8, 16)
    mask = torch.ones(2, 8, 1)
    for call in (lambda: F.sdpa(x, x, x, mask, 2, key_lengths=kl, causal=True),
                 lambda: F.attn_probs(x, x, mask, 2, key_lengths=kl, causal=True),
                 lambda: F.encoder_stack(x, mask, torch.zeros(10), 2, 16, 1, key_lengths=kl, causal=True),
                 lambda: F.encoder_stack_params(x, mask, [torch.zeros(10)], 2, 16, 1, flat=torch.zeros(10), key_lengths=kl, causal=True)):
        with pytest.raises(ValueError, match="key_lengths.*causal"):
            call()
    # both flags on a module: the call raises before anything else happens (CPU tensors would be refused next)
    mha = MT.MultiHeadedAttention(2, 16)
    mha.mask_keys = mha.causal = True
    with pytest.raises(ValueError, match="mask_keys.*causal"):
        mha(x, x, x, mask)
    enc = MT.Encoder(MT.EncoderLayer(16, MT.MultiHeadedAttention(2, 16), MT.PositionwiseFeedForward(16, 16), 0.1), 2)
    MT.mask_padded_keys(enc)
    MT.causal_attention(enc)
    assert enc._fusable()
    with pytest.raises(ValueError, match="mask_keys.*causal"):
        enc(x, mask)
