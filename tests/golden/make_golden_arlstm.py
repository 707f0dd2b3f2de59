#!/usr/bin/env python3
"""Generate the autoregressive LSTM fixtures (tests/golden/lstm_ar_*.npz, arlstm_surface.json) from the REFERENCE implementation (build
container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_arlstm.py <reference checkout>/transformer

The mechanism of make_golden_edlstm.py: the reference's MultiARLSTM (transformer/MFT/models.py:310-400) is imported from the reference
checkout, filled with recipe.py's deterministic weights and run in eval mode on CPU in fp32; only inputs-by-recipe, the output, the loss
(MSE-sum / sum of lengths), the full gradients of the small parameters (autoreg's among them) and every parameter's gradient norm are
stored — never weights.  A free-running case whose recipe weights made the recurrence explode would make every comparison meaningless:
max|p| < 1e3 is asserted for each (shorten T or scale the case if it ever fails).  The surface file records the signatures and the
state_dict keys / order / shapes.
"""
import json
import os
import sys

import torch

import arlstm_cases as C
import make_golden_lstm as G
import recipe as R

FULL_GRAD_SUFFIXES = G.FULL_GRAD_SUFFIXES + ("autoreg.weight",)          # autoreg.bias is covered by "bias"


def main():
    torch.manual_seed(1)
    torch.set_num_threads(4)
    G.FULL_GRAD_SUFFIXES = FULL_GRAD_SUFFIXES
    _, md = G.load_variant("MFT")
    for name, D, kw, lengths, T, tgt_init, teacher in C.ARLSTM_CASES:
        model = md.MultiARLSTM(D, device=G.CPU, **kw)
        x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED)
        target = C.ar_target(name, lengths, T) if teacher else None
        seen = {}

        def call(m, inp, ln, mask):
            seen["p"] = m(inp, torch.ones_like(mask), ln, target=target, tgt_init=tgt_init).detach()       # unmasked predictions
            return m(inp, mask, ln, target=target, tgt_init=tgt_init)
        G.run_case(name, model, x, lengths, T, call)
        pmax = float(seen["p"].abs().max())
        print("%-28s max|p| %.3e" % (name, pmax))
        assert teacher or pmax < 1e3, "%s: the recurrence explodes under the recipe (max|p| = %g)" % (name, pmax)
    surface = {"MultiARLSTM": {"init": G.sig(md.MultiARLSTM.__init__), "forward": G.sig(md.MultiARLSTM.forward),
                               "state(96, embed_dim=24, h_dim=40, ar_order=3)":
                                   G.state(md.MultiARLSTM(96, embed_dim=24, h_dim=40, ar_order=3, device=G.CPU))}}
    path = os.path.join(G.HERE, "arlstm_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-28s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_arlstm.py <reference checkout>/transformer")
    G.REF = sys.argv[1]
    main()
