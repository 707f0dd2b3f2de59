"""CPU: the surface of the key-length mask (mmt_*_keys, functional.key_lengths, MultiHeadedAttention.mask_keys,
multiTransformer.mask_padded_keys) and the equality its GPU tests rest on: attention with keys >= len[b] masked IS plain attention of
sequence b cut to its first len[b] windows and run alone (tests/test_gpu_key_mask.py takes tests/bf16_ref.py per truncated sequence as
its reference for that reason).  No GPU: the library is loaded, nothing is launched."""
import ctypes
import os
import re

import torch

import bf16_ref as E
import recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYED = ["mmt_key_lengths", "mmt_sdpa_forward_keys", "mmt_sdpa_backward_keys", "mmt_attn_probs_forward_keys", "mmt_encoder_forward_keys",
         "mmt_encoder_backward_keys", "mmt_encoder_forward_keys_devseed", "mmt_encoder_backward_keys_devseed"]


def test_keyed_entries_are_declared_exported_and_bound():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmt_hip.h")).read(), flags=re.S)
    for name in KEYED:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # a keyed entry is the plain entry plus one trailing pointer
    for name in KEYED[1:]:
        plain = name.replace("_keys", "")
        assert _lib.SIGNATURES[name] == (_lib.SIGNATURES[plain][0], _lib.SIGNATURES[plain][1] + [ctypes.c_void_p]), name
    assert lib.mmt_abi_version() == 1


def test_keyed_entries_refuse_null_pointers():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: every refusal below comes first
    EINVAL = 1
    assert lib.mmt_encoder_forward(None, None, None, None, None, 0, 4, 50, 128, 8, 128, 2, 1e-6, 0.0, 0, None) == EINVAL     # the code itself
    # null key_lengths, everything else in place
    assert lib.mmt_sdpa_forward_keys(one, one, one, one, one, one, 1 << 30, 2, 33, 32, 2, 0.0, 0, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    assert lib.mmt_sdpa_backward_keys(one, one, one, one, one, one, 1 << 30, 2, 33, 32, 2, 0.0, 0, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    assert lib.mmt_attn_probs_forward_keys(one, one, one, one, 2, 33, 32, 2, 0.0, 0, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    enc = (2, 33, 128, 8, 128, 2, 1e-6, 0.0)
    assert lib.mmt_encoder_forward_keys(one, one, one, one, one, 1 << 30, *enc, 0, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    assert lib.mmt_encoder_backward_keys(one, one, one, one, one, one, one, 1 << 30, *enc, 0, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    assert lib.mmt_encoder_forward_keys_devseed(one, one, one, one, one, 1 << 30, *enc, one, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    assert lib.mmt_encoder_backward_keys_devseed(one, one, one, one, one, one, one, 1 << 30, *enc, None, None) == EINVAL
    assert b"key_lengths" in lib.mmt_last_error()
    # key_lengths given, the plain entry's own pointers null: the plain entry's refusal
    assert lib.mmt_sdpa_forward_keys(None, None, None, None, None, None, 0, 2, 33, 32, 2, 0.0, 0, None, one) == EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_encoder_forward_keys(None, None, None, None, None, 0, *enc, 0, None, one) == EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_attn_probs_forward_keys(None, None, None, None, 2, 33, 32, 2, 0.0, 0, None, one) == EINVAL
    # mmt_key_lengths
    assert lib.mmt_key_lengths(one, one, 0, 33, None) == EINVAL and b"non-positive" in lib.mmt_last_error()
    assert lib.mmt_key_lengths(one, one, -3, 33, None) == EINVAL
    assert lib.mmt_key_lengths(one, one, 2, 0, None) == EINVAL
    assert lib.mmt_key_lengths(None, one, 2, 33, None) == EINVAL and b"null" in lib.mmt_last_error()
    assert lib.mmt_key_lengths(one, None, 2, 33, None) == EINVAL


def test_python_surface():
    import inspect
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    for fn in (F.sdpa, F.attn_probs, F.encoder_stack, F.encoder_stack_params):
        assert inspect.signature(fn).parameters["key_lengths"].default is None, fn.__name__
    assert callable(F.key_lengths)
    assert list(inspect.signature(MT.attention).parameters) == ["query", "key", "value", "mask", "dropout"]      # the reference's five
    mha = MT.MultiHeadedAttention(2, 8)
    assert MT.MultiHeadedAttention.mask_keys is False and "mask_keys" not in mha.__dict__
    assert MT.mask_padded_keys(mha) == {"": mha} and mha.mask_keys is True
    MT.mask_padded_keys(mha, False)
    assert mha.mask_keys is False
    model = MT.MultiTransformer(["acoustic", "emotient"], {"acoustic": 12, "emotient": 20}, N=2, d_ff=16, h=2, device=torch.device("cpu"),
                                embed_dim={"acoustic": 16, "emotient": 8})
    found = MT.mask_padded_keys(model)
    # every modality's stack, every layer (and the reference's unused attn{mod} prototypes, registered for the checkpoint keys)
    assert len(found) == 2 * (2 + 1) and all(m.mask_keys for m in found.values())
    assert sorted(found) == sorted(n for n, m in model.named_modules() if isinstance(m, MT.MultiHeadedAttention))
    enc = next(m for m in model.modules() if isinstance(m, MT.Encoder))
    assert enc._fusable()                                # the flag does not force the layer-by-layer path ...
    enc.layers[1].self_attn.mask_keys = False
    assert not enc._fusable()                            # ... layers that disagree about it do
    MT.mask_padded_keys(model, False)
    assert enc._fusable() and not any(m.mask_keys for m in found.values())


def test_key_lengths_argument_is_checked_before_any_launch():
    """dtype and shape are refused with ValueError by the argument check itself, which runs on any device (nothing is launched)"""
    import pytest
    from multimodal_transformer_amd import functional as F
    cpu = torch.device("cpu")
    ok = torch.tensor([3, 1], dtype=torch.int32)
    assert F._check_key_lengths("sdpa", None, 2, cpu) is None
    assert torch.equal(F._check_key_lengths("sdpa", ok, 2, cpu), ok)
    with pytest.raises(ValueError, match="int32"):
        F._check_key_lengths("sdpa", ok.long(), 2, cpu)
    with pytest.raises(ValueError, match="int32"):
        F._check_key_lengths("sdpa", [3, 1], 2, cpu)
    with pytest.raises(ValueError, match="shape"):
        F._check_key_lengths("sdpa", ok, 3, cpu)
    with pytest.raises(ValueError, match="shape"):
        F._check_key_lengths("sdpa", ok.reshape(2, 1), 2, cpu)
    with pytest.raises(ValueError, match="is on"):
        F._check_key_lengths("sdpa", ok, 2, torch.device("cuda:0"))


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def test_truncation_equals_key_masking_in_fp64():
    """bf16_ref.sdpa(rounding=False) of sequence b cut to len[b] windows == a direct softmax with -inf on the key columns >= len[b],
    on rows < len[b], to 1e-12: forward and the gradients of q, k, v (zero upstream gradient on rows >= len[b]; the masked form gives
    exactly zero dk, dv on rows >= len[b])."""
    T, d, h, lengths = 70, 40, 4, [70, 64, 33, 5, 1]
    B, dk = len(lengths), d // h
    q, k, v, g = (R.gen_normal("kmask_cpu" + n, (B, T, d), 5).double() for n in "qkvg")
    rowm = R.prefix_mask(lengths, T).double()
    g = g * rowm
    # masked form, whole batch: the reference's query-row blanking (Q' = 0) plus -inf on key columns >= len
    lm = [t.clone().requires_grad_() for t in (q, k, v)]
    Q, K, V = (_split(t, h) for t in lm)
    S = (Q * rowm.unsqueeze(1)) @ K.transpose(-2, -1) / dk ** 0.5
    cols = torch.arange(T).reshape(1, 1, 1, T) >= torch.tensor(lengths).reshape(B, 1, 1, 1)
    P = torch.softmax(S.masked_fill(cols, float("-inf")), dim=-1)
    assert (P.masked_select(cols.expand_as(P)) == 0).all()
    ctx = (P @ V).permute(0, 2, 1, 3).reshape(B, T, d)
    ctx.backward(g)
    for b, n in enumerate(lengths):
        lt = [t[b:b + 1, :n].clone().requires_grad_() for t in (q, k, v)]
        ref, _ = E.sdpa(*(_split(t, h) for t in lt), None, None, rounding=False)
        ref = ref.permute(0, 2, 1, 3).reshape(1, n, d)
        ref.backward(g[b:b + 1, :n])
        assert (ctx[b, :n] - ref[0]).abs().max().item() <= 1e-12
        for name, full, cut in zip("qkv", lm, lt):
            assert (full.grad[b, :n] - cut.grad[0]).abs().max().item() <= 1e-12, (b, name)
        assert (lm[1].grad[b, n:] == 0).all() and (lm[2].grad[b, n:] == 0).all()
        # a blanked query row is uniform over the visible keys
        if n < T:
            assert (P[b, :, n:, :n] - 1.0 / n).abs().max().item() <= 1e-15
