#!/usr/bin/env python3
"""Generate the fixtures of the window encoder at kernel sizes other than 2 (tests/golden/fe_cnn_k*.npz, fe_model_sft_k3.npz,
fe_model_mft_k5.npz) from the REFERENCE implementation (build container only).

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cnn_k.py

Same rules as make_golden_frontend.py, whose helpers it uses: the reference's classes are imported from the reference tree, filled with
recipe.py's deterministic weights, run in eval mode on CPU in fp32; only inputs-by-recipe and expected outputs / gradients are stored.
The reference passes k straight to nn.Conv1d (transformer/SFT/models.py:57-79, :82-93).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import recipe as R  # noqa: E402
from make_golden_frontend import fill, load_models, save  # noqa: E402

CNN_K = (1, 3, 4, 5)
CNN_K_SHAPE = (88, 256, 10, 12)             # (D, F, W, N)
MODEL_EXTRA = {"fe_model_sft_k3": ("fusionLayer.bias", "cnn_acoustic.conv1d.bias", "highway_image.linear_gate.bias", "Transformer.out.2.weight"),
               "fe_model_mft_k5": ("cnn_linguistic.conv1d.bias", "highway_acoustic.linear_projection.bias", "Transformer.mfn.out_fc2.weight")}


def main():
    torch.manual_seed(1)
    torch.set_num_threads(4)
    cpu = torch.device("cpu")
    sft = load_models("SFT")

    D, F, W, N = CNN_K_SHAPE
    for k in CNN_K:
        name = "fe_cnn_k%d" % k
        cnn = sft.CNN(D, F, k)
        w = fill(cnn, R.SEED)
        x = R.gen_normal(name + ":x", (N, W, D), R.SEED)
        g = R.gen_normal(name + ":g", (N, F), R.SEED)
        y = cnn(x.permute(0, 2, 1))
        (y * g).sum().backward()
        gw = R.to_np(cnn.conv1d.weight.grad)
        save(name, out=R.to_np(y), checksum=R.weights_checksum(w), gb=R.to_np(cnn.conv1d.bias.grad),
             gw_norm=np.float64(np.sqrt((gw.astype(np.float64) ** 2).sum())), gw_head=gw[:, :8, :].copy(),
             gw_tail=gw[:, -8:, :].copy())

    def model_case(name, tag, model, mods, dims, lengths, T):
        """tag: the k = 2 fixture whose inputs and target this one shares"""
        w = fill(model, R.SEED)
        B = len(lengths)
        mask = R.prefix_mask(lengths, T)
        inputs = {m: R.gen_normal("%s:%s" % (tag, m), (B, T, R.FE_WINDOW[m], dims[m]), R.SEED) for m in mods}
        target = R.gen_uniform(tag + ":target", (B, T, 1), R.SEED) * mask
        out = model(inputs, lengths, mask)
        loss = ((out - target) ** 2).sum() / float(sum(lengths))
        loss.backward()
        arrays = dict(out=R.to_np(out), loss=np.float64(loss.item()), checksum=R.weights_checksum(w), lengths=np.array(lengths))
        for k, p in model.named_parameters():
            arrays["gnorm:" + k] = np.float64(-1.0 if p.grad is None else float(p.grad.double().pow(2).sum().sqrt()))
        for k in MODEL_EXTRA[name]:
            arrays["grad:" + k] = R.to_np(dict(model.named_parameters())[k].grad)
        save(name, **arrays)

    mods, lengths = R.MODS_AVL, [6, 4]
    model_case("fe_model_sft_k3", "fe_model_sft", sft.MultiCNNTransformer(mods, R.FE_DIMS, k=3, device=cpu), mods, R.FE_DIMS, lengths, 6)
    mftm = load_models("MFT")
    model_case("fe_model_mft_k5", "fe_model_mft", mftm.MultiCNNTransformer(mods, R.FE_DIMS, R.FE_EMBED_MFT, k=5, device=cpu), mods, R.FE_DIMS, lengths, 6)


if __name__ == "__main__":
    main()
