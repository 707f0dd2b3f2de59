#!/usr/bin/env python3
"""Generate tests/golden/reference_surface.json from the REFERENCE implementation (build container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surface.py <reference checkout>/transformer

The Python surface of every drop-in class as data: constructor signatures (names and defaults), `forward` parameter
names, and the `state_dict` keys, order and shapes of the constructions tests/test_reference_surface.py checks.  The reference's
classes are imported from the reference's checkout (read-only, never copied) and constructed on CPU; nothing is executed.
"""
import importlib
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = None                      # <reference checkout>/transformer, from the command line
OUT = os.path.join(HERE, "reference_surface.json")
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

MODS = ["acoustic", "image", "linguistic"]
DIMS = {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 1000}
WES = {"acoustic": 88, "image": 256, "linguistic": 300}
CLASSES = ("PositionwiseFeedForward", "MultiHeadedAttention", "Encoder", "LayerNorm", "SublayerConnection", "EncoderLayer",
           "MFN", "MultiTransformer", "UniTransformer", "UniFullTransformer")
# (variant, name of our class, constructor arguments) -- the cases of test_front_end_surface
FRONT_ENDS = [
    ("SFT", "MultiCNNTransformer", (MODS, DIMS)),
    ("SFT", "MultiCNNTransformer", (["linguistic"], DIMS)),
    ("MFT", "MultiCNNTransformerMFT", (MODS, DIMS, {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 256})),
    ("B2-Trans", "MultiCNNTransformerB2", (["linguistic"], DIMS)),
]


def front_end_key(variant, args):
    return "%s:%s" % (variant, json.dumps(args, sort_keys=True))


def load_variant(variant):
    """import <variant>/multiTransformer.py and models.py under their own names, then drop them from sys.modules again"""
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
    """[[name, str(default) or "<required>"], ...] without self"""
    return [[n, str(p.default) if p.default is not inspect._empty else "<required>"]
            for n, p in inspect.signature(cls_or_fn).parameters.items() if n != "self"]


def names(cls_or_fn):
    return [n for n, _ in sig(cls_or_fn)]


def state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def main():
    global REF
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_golden_surface.py <reference checkout>/transformer")
    REF = sys.argv[1]
    torch.manual_seed(1)
    cpu = torch.device("cpu")
    out = {"multitransformer": {}, "front_end": {}}
    for variant in ("SFT", "MFT", "B2-Trans"):
        mt, _ = load_variant(variant)
        entry = {"classes": {}, "attention": names(mt.attention), "state": {}}
        for name in CLASSES:
            if hasattr(mt, name):
                entry["classes"][name] = {"init": sig(getattr(mt, name).__init__), "forward": names(getattr(mt, name).forward)}
        entry["state"]["MultiTransformer"] = state(mt.MultiTransformer(MODS, WES, device=cpu))
        entry["state"]["UniFullTransformer(300)"] = state(mt.UniFullTransformer(300, device=cpu))
        entry["state"]["UniTransformer(300)"] = state(mt.UniTransformer(300, device=cpu))
        if hasattr(mt, "NLPTransformer"):
            entry["nlp_init"] = sig(mt.NLPTransformer.__init__)
            entry["state"]["NLPTransformer(512)"] = state(mt.NLPTransformer(512, device=cpu))
            entry["state"]["NLPTransformer(512, embed_dim=128)"] = state(mt.NLPTransformer(512, embed_dim=128, device=cpu))
        out["multitransformer"][variant] = entry
    for variant, _, args in FRONT_ENDS:
        _, md = load_variant(variant)
        out["front_end"][front_end_key(variant, args)] = {
            "init": sig(md.MultiCNNTransformer.__init__), "forward": names(md.MultiCNNTransformer.forward),
            "state": state(md.MultiCNNTransformer(*args, device=cpu)),
            "CNN": sig(md.CNN.__init__), "Highway": sig(md.Highway.__init__),
            "state_CNN(300, 128, 2)": state(md.CNN(300, 128, 2)), "state_Highway(64)": state(md.Highway(64))}
    with open(OUT, "w") as fh:
        json.dump(out, fh, sort_keys=True)
        fh.write("\n")
    print("%s %8.1f KB" % (os.path.basename(OUT), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
