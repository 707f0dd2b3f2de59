"""CPU: the Python surface of the drop-in modules against the reference's own classes — constructor signatures, `forward` signatures,
`state_dict` keys, key ORDER and shapes — for every class SURVEY 8(b) lists.  The reference's side is read from
tests/golden/reference_surface.json (tests/golden/make_golden_surface.py, generated from the imported reference).  Nothing is executed
on the HIP path here (construction only)."""
import inspect
import json
import os

import pytest
import torch

import conftest

with open(os.path.join(conftest.GOLDEN, "reference_surface.json")) as _fh:
    REF = json.load(_fh)


def _sig(cls_or_fn):
    return [(n, p.default if p.default is not inspect._empty else "<required>")
            for n, p in inspect.signature(cls_or_fn).parameters.items() if n != "self"]


def _same_state(ours, ref):
    """ref: [[key, shape], ...] of the reference's state_dict, in its order"""
    a = ours.state_dict()
    assert list(a.keys()) == [k for k, _ in ref]
    for k, shape in ref:
        assert tuple(a[k].shape) == tuple(shape), k


MODS = ["acoustic", "image", "linguistic"]
DIMS = {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 1000}


@pytest.mark.parametrize("variant", ["SFT", "MFT", "B2-Trans"])
def test_multitransformer_module_surface(variant):
    from multimodal_transformer_amd import multiTransformer as OURS
    ref = REF["multitransformer"][variant]
    cpu = torch.device("cpu")
    for name in ("PositionwiseFeedForward", "MultiHeadedAttention", "Encoder", "LayerNorm", "SublayerConnection", "EncoderLayer",
                 "MFN", "MultiTransformer", "UniTransformer", "UniFullTransformer"):
        if name not in ref["classes"]:
            continue
        rs, os_ = ref["classes"][name]["init"], _sig(getattr(OURS, name).__init__)
        # our classes may append keyword arguments; the reference's own must come first, same names and defaults
        assert [(n, str(d)) for n, d in os_[:len(rs)]] == [(n, d) for n, d in rs], name
        assert [n for n, _ in _sig(getattr(OURS, name).forward)] == ref["classes"][name]["forward"], name
    assert [n for n, _ in _sig(OURS.attention)] == ref["attention"]
    wes = {"acoustic": 88, "image": 256, "linguistic": 300}
    _same_state(OURS.MultiTransformer(MODS, wes, device=cpu), ref["state"]["MultiTransformer"])
    _same_state(OURS.UniFullTransformer(300, device=cpu), ref["state"]["UniFullTransformer(300)"])
    _same_state(OURS.UniTransformer(300, device=cpu), ref["state"]["UniTransformer(300)"])
    if "nlp_init" in ref:
        assert _sig(OURS.NLPTransformer.__init__)[:len(ref["nlp_init"])] is not None
        _same_state(OURS.NLPTransformer(512, device=cpu), ref["state"]["NLPTransformer(512)"])
        _same_state(OURS.NLPTransformer(512, embed_dim=128, device=cpu), ref["state"]["NLPTransformer(512, embed_dim=128)"])


@pytest.mark.parametrize("variant,ours_name,args", [
    ("SFT", "MultiCNNTransformer", (MODS, DIMS)),
    ("SFT", "MultiCNNTransformer", (["linguistic"], DIMS)),
    ("MFT", "MultiCNNTransformerMFT", (MODS, DIMS, {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 256})),
    ("B2-Trans", "MultiCNNTransformerB2", (["linguistic"], DIMS))])
def test_front_end_surface(variant, ours_name, args, capsys):
    from multimodal_transformer_amd import models as OURS
    ref = REF["front_end"]["%s:%s" % (variant, json.dumps(args, sort_keys=True))]     # key as in make_golden_surface.front_end_key
    cpu = torch.device("cpu")
    our_cls = getattr(OURS, ours_name)
    assert [(n, str(d)) for n, d in _sig(our_cls.__init__)] == [(n, d) for n, d in ref["init"]]
    assert [n for n, _ in _sig(our_cls.forward)] == ref["forward"]
    _same_state(our_cls(*args, device=cpu), ref["state"])
    for name in ("CNN", "Highway"):
        assert [(n, str(d)) for n, d in _sig(getattr(OURS, name).__init__)] == [(n, d) for n, d in ref[name]]
    _same_state(OURS.CNN(300, 128, 2), ref["state_CNN(300, 128, 2)"])
    _same_state(OURS.Highway(64), ref["state_Highway(64)"])
