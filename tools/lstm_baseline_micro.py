#!/usr/bin/env python3
"""Train-step timing of the B1-LSTM baseline (models.MultiCNNLSTM) at B1's own configuration (transformer/B1-LSTM/train.py:527-529,591):
linguistic only, raw dim 1024, 5 words per window, window_embed_size 1024, B1's MultiLSTM (E = 512, H = 256, L = 5).

    python tools/lstm_baseline_micro.py [--batches 10,25] [--T 500] [--steps 20] [--warmup 3]

One line per batch size: ms per train-mode step (forward, MSE-sum loss, backward; no optimiser), wall clock around `steps` eager steps
ending in a device synchronise.  For the kernel split run it once under `rocprofv3 --kernel-trace --stats -- python ...` (a run of its
own; the stats file lists every kernel of the timed and warm-up steps)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="10,25")
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from multimodal_transformer_amd import models as M, functional as F
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    T, D, W = args.T, 1024, 5
    for B in [int(b) for b in args.batches.split(",")]:
        model = M.MultiCNNLSTM(["linguistic"], {"linguistic": D}, device=dev).train()
        x = {"linguistic": torch.randn(B, T, W, D, device=dev)}
        lengths = [T] + [max(2, T - 7 * i) for i in range(1, B)]
        mask = torch.zeros(B, T, 1, device=dev)
        for b, n in enumerate(lengths):
            mask[b, :n] = 1.0
        tgt = torch.rand(B, T, 1, device=dev) * mask
        params = list(model.parameters())

        def step():
            for p in params:
                p.grad = None
            F.mse_sum_loss_backward(model(x, lengths, mask), tgt, sum(lengths))

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        F.check_device_errors()
        print("MultiCNNLSTM B1 config B=%d T=%d W=%d D=%d F=1024 E=512 H=256 L=5: %.3f ms/train step (%d steps)"
              % (B, T, W, D, dt * 1e3, args.steps), flush=True)
        del model, x


if __name__ == "__main__":
    main()
