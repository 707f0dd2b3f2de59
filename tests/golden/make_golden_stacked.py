#!/usr/bin/env python3
"""Generate the stacked-LSTM fixtures (tests/golden/model_sft_l*.npz, model_uni_l2.npz, lstm_shared_l2.npz, lstm_b1_l3.npz) from the
REFERENCE implementation (build container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stacked.py <reference checkout>/transformer

The mechanism of make_golden_lstm.py: the reference's classes are imported from the reference checkout, filled with recipe.py's
deterministic weights (dec_h0 / dec_c0 non-zero) and run in eval mode on CPU in fp32; only inputs-by-recipe, the output, the loss
(MSE-sum / sum of lengths), the full gradients of the small parameters and every parameter's gradient norm are stored — never weights.
"""
import sys

import torch

import make_golden_lstm as G
import recipe as R
import stacked_cases as C

FULL_GRAD_SUFFIXES = G.FULL_GRAD_SUFFIXES + ("dec_h0", "dec_c0", "out.2.weight")


def main():
    torch.manual_seed(1)
    torch.set_num_threads(4)
    G.FULL_GRAD_SUFFIXES = FULL_GRAD_SUFFIXES
    variants = {}
    for name, cls, variant, D, kw, lengths, T in C.DECODER_CASES + C.BASELINE_CASES:
        if variant not in variants:
            variants[variant] = G.load_variant(variant)
        mt, md = variants[variant]
        ref_cls = getattr(mt, cls) if hasattr(mt, cls) else getattr(md, "MultiLSTM")
        model = ref_cls(D, device=G.CPU, **kw)
        x = R.gen_normal(name + ":x", (len(lengths), T, D), R.SEED)
        G.run_case(name, model, x, lengths, T, lambda m, inp, ln, mask: m(inp, mask, ln))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_stacked.py <reference checkout>/transformer")
    G.REF = sys.argv[1]
    main()
