#!/usr/bin/env python3
"""Generate the encoder-decoder LSTM fixtures (tests/golden/lstm_ed_*.npz, edlstm_surface.json) from the REFERENCE implementation
(build container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edlstm.py <reference checkout>/transformer

The mechanism of make_golden_lstm.py: the reference's MultiEDLSTM (transformer/MFT/models.py:222-308) is imported from the reference
checkout, filled with recipe.py's deterministic weights and run in eval mode on CPU in fp32; only inputs-by-recipe, the output, the loss
(MSE-sum / sum of lengths), the full gradients of the small parameters and every parameter's gradient norm are stored — never weights.
The recipe must leave enc_h0, enc_c0, dec_h0 and dec_c0 non-zero (the class initialises them to zeros, which would hide a wrong initial
state): checked here.  The surface file records the signatures and the state_dict keys / order / shapes.
"""
import json
import os
import sys

import torch

import edlstm_cases as C
import make_golden_lstm as G
import recipe as R

FULL_GRAD_SUFFIXES = G.FULL_GRAD_SUFFIXES + ("dec_h0", "dec_c0", "enc_h0", "enc_c0", "out.2.weight")


def main():
    torch.manual_seed(1)
    torch.set_num_threads(4)
    G.FULL_GRAD_SUFFIXES = FULL_GRAD_SUFFIXES
    _, md = G.load_variant("MFT")
    for name, D, kw, lengths, T, tgt_init in C.EDLSTM_CASES:
        model = md.MultiEDLSTM(D, device=G.CPU, **kw)
        x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED)
        G.run_case(name, model, x, lengths, T, lambda m, inp, ln, mask: m(inp, mask, ln, tgt_init=tgt_init))
        for k in ("enc_h0", "enc_c0", "dec_h0", "dec_c0"):
            v = getattr(model, k).detach()
            assert float(v.abs().min()) > 0.0 or float(v.abs().mean()) > 1e-3, "%s: %s is (nearly) zero under the recipe" % (name, k)
            print("%-28s %s rms %.3e" % (name, k, float(v.pow(2).mean().sqrt())))
    surface = {"MultiEDLSTM": {"init": G.sig(md.MultiEDLSTM.__init__), "forward": G.sig(md.MultiEDLSTM.forward),
                               "state(96, embed_dim=24, h_dim=40)": G.state(md.MultiEDLSTM(96, embed_dim=24, h_dim=40, device=G.CPU))}}
    path = os.path.join(G.HERE, "edlstm_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-28s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_edlstm.py <reference checkout>/transformer")
    G.REF = sys.argv[1]
    main()
