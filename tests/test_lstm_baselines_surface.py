"""CPU: the Python surface of the LSTM baselines (B1-LSTM) and of B3-MFN against the reference's classes, read from
tests/golden/lstm_baselines_surface.json (tests/golden/make_golden_lstm.py): constructor and `forward` signatures, `state_dict` keys,
order and shapes; the shipped B1-LSTM-L.pth checkpoint's key and shape list; and the argument checks of the local-attention C ABI,
which fail before anything touches a GPU."""
import inspect
import json
import os

import pytest
import torch

import conftest

with open(os.path.join(conftest.GOLDEN, "lstm_baselines_surface.json")) as _fh:
    REF = json.load(_fh)

CPU = torch.device("cpu")
MODS = ["acoustic", "image", "linguistic"]
DIMS = {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 1000}
EMBED_AVL = {"acoustic": 88, "image": 256, "linguistic": 300}


def _sig(fn):
    return [[n, str(p.default) if p.default is not inspect._empty else "<required>"]
            for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def _state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _checkpoint_model():
    from multimodal_transformer_amd import models as M
    return M.MultiCNNLSTM(["linguistic"], {"linguistic": 300}, window_embed_size={"linguistic": 300}, lstm_cls=M.MultiLSTM, device=CPU)


@pytest.mark.parametrize("ours,ref,args", [("MultiLSTM", "MultiLSTM", (300,)), ("MultiLSTMB1", "MultiLSTMB1", (1024,))])
def test_lstm_sequence_models(ours, ref, args):
    from multimodal_transformer_amd import models as M
    cls = getattr(M, ours)
    assert _sig(cls.__init__) == REF[ref]["init"]
    assert [n for n, _ in _sig(cls.forward)] == REF[ref]["forward"]
    assert _state(cls(*args, device=CPU)) == REF[ref]["state(%d)" % args[0]]


def test_multi_cnn_lstm():
    from multimodal_transformer_amd import models as M
    ref = REF["MultiCNNLSTM"]
    ours = _sig(M.MultiCNNLSTM.__init__)
    # the reference's positional signature first, then the keyword-only extensions
    assert ours[:len(ref["init"])] == ref["init"]
    kw = [n for n, p in inspect.signature(M.MultiCNNLSTM.__init__).parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert [n for n, _ in ours[len(ref["init"]):]] == kw == ["window_embed_size", "lstm_cls"]
    assert [n for n, _ in _sig(M.MultiCNNLSTM.forward)] == ref["forward"]
    assert _state(M.MultiCNNLSTM(["linguistic"], {"linguistic": 1024}, device=CPU)) == ref["state(linguistic 1024)"]
    assert _state(_checkpoint_model()) == ref["state(checkpoint)"]
    assert _sig(M.HighwayB1.__init__) == REF["HighwayB1"]["init"]
    assert _state(M.HighwayB1(64)) == REF["HighwayB1"]["state(64)"]
    m = M.MultiCNNLSTM(["acoustic", "linguistic"], {"acoustic": 88, "linguistic": 300}, device=CPU)
    assert all(type(h) is M.HighwayB1 for h in m.Highway.values())
    assert type(m.LSTM) is M.MultiLSTMB1


def test_b3_models():
    from multimodal_transformer_amd import models as M, multiTransformer as MT
    ref = REF["MultiCNNTransformerB3"]
    assert _sig(M.MultiCNNTransformerB3.__init__) == ref["init"]
    assert [n for n, _ in _sig(M.MultiCNNTransformerB3.forward)] == ref["forward"]
    assert _state(M.MultiCNNTransformerB3(MODS, DIMS, device=CPU)) == ref["state(avl)"]
    assert _state(M.MultiCNNTransformerB3(["linguistic"], DIMS, device=CPU)) == ref["state(linguistic)"]
    ref = REF["MultiTransformerB3"]
    assert _sig(MT.MultiTransformerB3.__init__) == ref["init"]
    assert [n for n, _ in _sig(MT.MultiTransformerB3.forward)] == ref["forward"]
    st = _state(MT.MultiTransformerB3(MODS, EMBED_AVL, device=CPU))
    assert st == ref["state(avl)"]
    assert all(k.startswith(("embed_", "mfn.")) for k, _ in st)


def test_checkpoint_configuration_strict_loads():
    ck = REF["checkpoint:B1-LSTM-L.pth"]
    assert ck["modalities"] == ["linguistic"]
    model = _checkpoint_model()
    assert _state(model) == ck["state"]
    sd = {k: torch.full(tuple(shape), 0.25) for k, shape in ck["state"]}       # the checkpoint's keys and shapes (never its values)
    model.load_state_dict(sd, strict=True)
    assert float(model.LSTM.decoder[2].bias.detach()) == 0.25
    L = model.LSTM
    assert (L.embed_dim, L.h_dim, L.attn_len, L.embed[0].p) == (128, 256, 5, 0.1)


def test_local_attn_abi_rejects_bad_arguments():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    assert lib.mmt_abi_version() == 1
    assert lib.mmt_local_attn_workspace_bytes(25, 500, 256, 5) >= 25 * 500 * 5 * 4
    assert lib.mmt_local_attn_workspace_bytes(25, 500, 256, 0) == 0
    assert b"attn_len" in lib.mmt_last_error()
    assert lib.mmt_local_attn_workspace_bytes(25, 500, 256, 17) == 0
    assert b"> 16" in lib.mmt_last_error()
    assert lib.mmt_local_attn_workspace_bytes(0, 500, 256, 5) == 0
    fake = 4096                                               # never dereferenced: every call below fails its checks first
    p5 = [fake] * 5
    assert lib.mmt_local_attn_forward(*p5, 2, 10, 256, 0, None) == 1
    assert lib.mmt_local_attn_forward(*p5, 2, 10, 256, 17, None) == 2
    assert lib.mmt_local_attn_forward(*p5, 2, 0, 256, 5, None) == 1
    assert lib.mmt_local_attn_forward(None, fake, fake, fake, fake, 2, 10, 256, 5, None) == 1
    assert b"null" in lib.mmt_last_error()
    p7 = [fake] * 7
    assert lib.mmt_local_attn_backward(*p7, 1 << 20, 2, 10, 256, 0, None) == 1
    assert lib.mmt_local_attn_backward(*p7, 1 << 20, 2, 10, 256, 17, None) == 2
    assert lib.mmt_local_attn_backward(fake, fake, fake, fake, fake, fake, None, 1 << 20, 2, 10, 256, 5, None) == 1
    assert lib.mmt_local_attn_backward(*p7, 16, 2, 10, 256, 5, None) == 3            # workspace too small
    assert b"workspace" in lib.mmt_last_error()


def test_lstm_model_rejects_what_it_cannot_do():
    from multimodal_transformer_amd import models as M
    m = M.MultiLSTM(16, device=CPU)
    with pytest.raises(ValueError, match="max\\(lengths\\)"):
        m(torch.zeros(2, 5, 16), torch.ones(2, 5, 1), [4, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 5, 16), torch.ones(2, 5, 1), [5, 3])
