#!/usr/bin/env python3
"""Generate the LSTM-baseline and B3-MFN fixtures (tests/golden/lstm_*.npz, b3_*.npz, lstm_baselines_surface.json) from the REFERENCE
implementation (build container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lstm.py <reference checkout>/transformer

Same rules as make_golden_frontend.py: the reference's classes (transformer/{B1-LSTM,SFT,B3-MFN}/models.py and the multiTransformer.py
each imports) are imported from the reference checkout, filled with recipe.py's deterministic weights and run in eval mode on CPU in
fp32; only inputs-by-recipe, expected outputs, the loss (MSE-sum / sum of lengths, the training loss) and gradients are stored — never
weights.  The surface file records signatures, state_dict keys / order / shapes, and the key and shape list of the shipped checkpoint
ModelSave/B1-LSTM/B1-LSTM-L.pth (shapes only).
"""
import importlib
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lstm_cases as C  # noqa: E402
import recipe as R  # noqa: E402

REF = None
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
CPU = torch.device("cpu")

# full gradients are stored for these parameters (small); every parameter's gradient norm is stored
FULL_GRAD_SUFFIXES = ("bias", "attn.2.weight", "decoder.2.weight", "decoder.3.weight", "out_fc2.weight")


def load_variant(variant):
    for name in ("models", "multiTransformer"):
        sys.modules.pop(name, None)
    sys.path.insert(0, os.path.join(REF, variant))
    try:
        mt = importlib.import_module("multiTransformer")
        md = importlib.import_module("models")
    finally:
        sys.path.pop(0)
        for name in ("models", "multiTransformer"):
            sys.modules.pop(name, None)
    return mt, md


def sig(cls_or_fn):
    return [[n, str(p.default) if p.default is not inspect._empty else "<required>"]
            for n, p in inspect.signature(cls_or_fn).parameters.items() if n != "self"]


def state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def fill(module, seed):
    params = R.gen_params(R.shapes_of(module.state_dict()), seed)
    module.load_state_dict(params)
    module.eval()
    return params


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%-28s %8.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


def checkpoint_construction(b1, sft):
    """B1's MultiCNNLSTM as the shipped checkpoint was built: linguistic window_embed_size 300 and the shared MultiLSTM (the file was
    saved from an older B1 models.py; the Highway is B1's)."""
    m = b1.MultiCNNLSTM(["linguistic"], {"linguistic": 300}, device=CPU)
    m.window_embed_size = dict(m.window_embed_size, linguistic=300)
    m.CNN["linguistic"] = b1.CNN(300, 300, 2)
    m.Highway["linguistic"] = b1.Highway(300)
    m.cnn_linguistic = m.CNN["linguistic"]
    m.highway_linguistic = m.Highway["linguistic"]
    m.LSTM = sft.MultiLSTM(300, device=CPU)
    return m


def run_case(name, model, inputs, lengths, T, call):
    """call(model, inputs, lengths, mask) -> (B,T,1) output; stores out, loss, checksum, lengths, gnorm:* and grad:* of small tensors"""
    w = fill(model, R.SEED)
    mask = R.prefix_mask(lengths, T)
    target = R.gen_uniform(name + ":target", (len(lengths), T, 1), R.SEED) * mask
    out = call(model, inputs, lengths, mask)
    loss = ((out - target) ** 2).sum() / float(sum(lengths))
    loss.backward()
    arrays = dict(out=R.to_np(out), loss=np.float64(loss.item()), checksum=R.weights_checksum(w), lengths=np.array(lengths))
    for k, p in model.named_parameters():
        arrays["gnorm:" + k] = np.float64(-1.0 if p.grad is None else float(p.grad.double().pow(2).sum().sqrt()))
        if p.grad is not None and k.endswith(FULL_GRAD_SUFFIXES):
            arrays["grad:" + k] = R.to_np(p.grad)
    save(name, **arrays)


def main():
    torch.manual_seed(1)
    torch.set_num_threads(4)
    b1_mt, b1 = load_variant("B1-LSTM")
    sft_mt, sft = load_variant("SFT")
    b3_mt, b3 = load_variant("B3-MFN")

    def seq_call(model, x, lengths, mask):
        return model(x, mask, lengths)

    def windows_call(model, x, lengths, mask):
        return model(x, lengths, mask)

    for name, cls, D, lengths, T in C.LSTM_SEQ_CASES:
        model = (sft.MultiLSTM if cls == "MultiLSTM" else b1.MultiLSTM)(D, device=CPU)
        x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED)
        run_case(name, model, x, lengths, T, seq_call)

    for name, cls, mods, dims, lengths, T, W in C.LSTM_WINDOW_CASES:
        if cls == "MultiCNNLSTM":
            model = b1.MultiCNNLSTM(mods, dims, device=CPU)
        elif cls == "MultiCNNLSTM:checkpoint":
            model = checkpoint_construction(b1, sft)
        else:
            model = b3.MultiCNNTransformer(mods, dims, device=CPU)
        x = {m: R.gen_normal("%s:%s" % (name, m), (len(lengths), T, W[m], dims[m]), R.SEED) for m in mods}
        run_case(name, model, x, lengths, T, windows_call)

    name, lengths, T = C.B3_SEQ_CASE
    model = b3_mt.MultiTransformer(R.MODS_AVL, R.EMBED_AVL, device=CPU)
    x = {m: R.gen_normal("%s:%s" % (name, m), (len(lengths), T, R.EMBED_AVL[m]), R.SEED) for m in R.MODS_AVL}
    run_case(name, model, x, lengths, T, seq_call)

    # ---- surface --------------------------------------------------------------------------------------------------------------
    ck = torch.load(os.path.join(REF, "ModelSave", "B1-LSTM", "B1-LSTM-L.pth"), map_location="cpu", weights_only=False)
    surface = {
        "MultiLSTM": {"init": sig(sft.MultiLSTM.__init__), "forward": [n for n, _ in sig(sft.MultiLSTM.forward)],
                      "state(300)": state(sft.MultiLSTM(300, device=CPU))},
        "MultiLSTMB1": {"init": sig(b1.MultiLSTM.__init__), "forward": [n for n, _ in sig(b1.MultiLSTM.forward)],
                        "state(1024)": state(b1.MultiLSTM(1024, device=CPU))},
        "MultiCNNLSTM": {"init": sig(b1.MultiCNNLSTM.__init__), "forward": [n for n, _ in sig(b1.MultiCNNLSTM.forward)],
                         "state(linguistic 1024)": state(b1.MultiCNNLSTM(["linguistic"], {"linguistic": 1024}, device=CPU)),
                         "state(checkpoint)": state(checkpoint_construction(b1, sft))},
        "HighwayB1": {"init": sig(b1.Highway.__init__), "state(64)": state(b1.Highway(64))},
        "MultiCNNTransformerB3": {"init": sig(b3.MultiCNNTransformer.__init__), "forward": [n for n, _ in sig(b3.MultiCNNTransformer.forward)],
                                  "state(avl)": state(b3.MultiCNNTransformer(R.MODS_AVL, R.FE_DIMS, device=CPU)),
                                  "state(linguistic)": state(b3.MultiCNNTransformer(["linguistic"], R.FE_DIMS, device=CPU))},
        "MultiTransformerB3": {"init": sig(b3_mt.MultiTransformer.__init__), "forward": [n for n, _ in sig(b3_mt.MultiTransformer.forward)],
                               "state(avl)": state(b3_mt.MultiTransformer(R.MODS_AVL, R.EMBED_AVL, device=CPU))},
        "checkpoint:B1-LSTM-L.pth": {"modalities": ck["modalities"], "window_size": ck["window_size"],
                                     "mod_dimension": ck["mod_dimension"],
                                     "state": [[k, list(v.shape)] for k, v in ck["model"].items()]},
    }
    path = os.path.join(HERE, "lstm_baselines_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-28s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_lstm.py <reference checkout>/transformer")
    REF = sys.argv[1]
    main()
