"""CPU: the surface of the attention-map request (MultiHeadedAttention.keep_attn, multiTransformer.keep_attention,
multiTransformer.attention_with_map, functional.attn_probs).  The flag is a class attribute, not a constructor argument and not a
buffer: the reference's constructor signature and its state_dict keys stay as tests/golden/reference_surface.json records them.
Construction only; nothing runs on the HIP path."""
import inspect
import json
import os

import pytest
import torch

import conftest

with open(os.path.join(conftest.GOLDEN, "reference_surface.json")) as _fh:
    REF = json.load(_fh)["multitransformer"]["SFT"]

CPU = torch.device("cpu")


def _mt():
    from multimodal_transformer_amd import multiTransformer
    return multiTransformer


def test_keep_attn_defaults_to_false_and_is_no_constructor_argument():
    MT = _mt()
    assert MT.MultiHeadedAttention.keep_attn is False
    mha = MT.MultiHeadedAttention(4, 64)
    assert mha.keep_attn is False and mha.attn is None
    assert "keep_attn" not in mha.__dict__                          # the class attribute, until keep_attention sets one on the instance
    names = [n for n in inspect.signature(MT.MultiHeadedAttention.__init__).parameters if n != "self"]
    assert names == [n for n, _ in REF["classes"]["MultiHeadedAttention"]["init"]]
    assert [n for n in inspect.signature(MT.attention).parameters] == REF["attention"]
    assert [n for n in inspect.signature(MT.attention_with_map).parameters] == REF["attention"]


def test_state_dict_keys_unchanged_by_the_flag():
    MT = _mt()
    mha = MT.MultiHeadedAttention(4, 64)
    before = list(mha.state_dict().keys())
    assert before == ["linears.%d.%s" % (i, n) for i in range(4) for n in ("weight", "bias")]
    assert MT.keep_attention(mha) == {"": mha}
    assert mha.keep_attn is True and list(mha.state_dict().keys()) == before and not list(mha.buffers())
    for args, kw, key in (((512,), {}, "NLPTransformer(512)"), ((512,), {"embed_dim": 128}, "NLPTransformer(512, embed_dim=128)")):
        model = MT.NLPTransformer(*args, device=CPU, **kw)
        MT.keep_attention(model)
        state = model.state_dict()
        assert list(state.keys()) == [k for k, _ in REF["state"][key]]
        for k, shape in REF["state"][key]:
            assert tuple(state[k].shape) == tuple(shape), k


def test_keep_attention_names_nlp_transformer():
    MT = _mt()
    model = MT.NLPTransformer(64, embed_dim=64, N=3, h=4, device=CPU)
    found = MT.keep_attention(model)
    assert list(found) == ["encoder.layers.%d.self_attn" % i for i in range(3)]
    assert all(type(m) is MT.MultiHeadedAttention and m.keep_attn is True for m in found.values())
    assert found["encoder.layers.1.self_attn"] is model.encoder.layers[1].self_attn
    assert model.encoder._fusable() is False                        # the fused stack never forms the map
    found["encoder.layers.0.self_attn"].attn = torch.zeros(1, 4, 2, 2)          # as a forward with the flag set leaves one
    again = MT.keep_attention(model, False)
    assert list(again) == list(found) and not any(m.keep_attn for m in again.values())
    assert all(m.attn is None for m in again.values())              # turning the flag off drops the maps kept so far
    assert model.encoder._fusable() is True


def test_keep_attention_names_multi_transformer():
    MT = _mt()
    mods = ["acoustic", "linguistic"]
    model = MT.MultiTransformer(mods, {"acoustic": 88, "linguistic": 300}, N=2, device=CPU)
    found = MT.keep_attention(model)
    # registration order (:273-277): the prototype attn{mod} (a dead parameter set the reference registers too), then the stack
    expect = []
    for mod in mods:
        expect += ["attn%s" % mod] + ["transformer_%s.layers.%d.self_attn" % (mod, i) for i in range(2)]
    assert list(found) == expect
    assert all(m.keep_attn for m in found.values())
    assert not any(model.transformer[mod]._fusable() for mod in mods)
    MT.keep_attention(model.transformer["acoustic"], False)          # a sub-module: only what lies below it
    assert model.transformer["acoustic"]._fusable() and not model.transformer["linguistic"]._fusable()


def test_attn_probs_refuses_cpu_tensors():
    from multimodal_transformer_amd import functional as F
    q = torch.zeros(1, 4, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.attn_probs(q, q, None, 1)
