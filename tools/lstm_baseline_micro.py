#!/usr/bin/env python3
"""Train-step timing of the LSTM baselines.

    python tools/lstm_baseline_micro.py [--model b1] [--batches 10,25] [--T 500] [--steps 20] [--warmup 3] [--runs 1]

--model b1 (default): the B1-LSTM baseline (models.MultiCNNLSTM) at B1's own configuration (transformer/B1-LSTM/train.py:527-529,591):
linguistic only, raw dim 1024, 5 words per window, window_embed_size 1024, B1's MultiLSTM (E = 512, H = 256, L = 5).
--model lstm,ar-free,ar-teacher (any comma list of these): the sequence models alone on (B,T,300) window embeddings with E = 128,
--h-dim H (default 256), attn_len 5 and ar_order --ar-order: models.MultiLSTM, and models.MultiARLSTM free-running / teacher-forced.
The two classes differ only in the read-out, so their difference at one shape is the read-out's cost.  The listed models are built once
and timed in turn, --runs times over (alternating, so that a drift of the machine shows up as spread and not as a difference).

One line per model, batch size and run: ms per train-mode step (forward, MSE-sum loss, backward; no optimiser), wall clock around
`steps` eager steps ending in a device synchronise.  --fwd-kernel adds the device-event time of functional.ar_combine's free-running
forward alone at each batch size ((B,T,K) = (B, --T, --ar-order); per call, over --steps calls).  For the kernel split run it once under
`rocprofv3 --kernel-trace --stats -- python ...` (a run of its own; the stats file lists every kernel of the timed and warm-up steps)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _build(kind, B, T, args, dev):
    """-> (description, step()) of one model at one batch size"""
    from multimodal_transformer_amd import models as M, functional as F
    lengths = [T] + [max(2, T - 7 * i) for i in range(1, B)]
    mask = torch.zeros(B, T, 1, device=dev)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1.0
    tgt = torch.rand(B, T, 1, device=dev) * mask
    if kind == "b1":
        D, W = 1024, 5
        model = M.MultiCNNLSTM(["linguistic"], {"linguistic": D}, device=dev).train()
        x = {"linguistic": torch.randn(B, T, W, D, device=dev)}
        what = "MultiCNNLSTM B1 config B=%d T=%d W=%d D=%d F=1024 E=512 H=256 L=5" % (B, T, W, D)
        call = lambda: model(x, lengths, mask)                                                      # noqa: E731
    else:
        D, H, K = 300, args.h_dim, args.ar_order
        x = torch.randn(B, T, D, device=dev)
        if kind == "lstm":
            model = M.MultiLSTM(D, embed_dim=128, h_dim=H, attn_len=5, device=dev).train()
            what = "MultiLSTM B=%d T=%d D=%d E=128 H=%d L=5" % (B, T, D, H)
            call = lambda: model(x, mask, lengths)                                                  # noqa: E731
        else:
            model = M.MultiARLSTM(D, embed_dim=128, h_dim=H, attn_len=5, ar_order=K, device=dev).train()
            what = "MultiARLSTM %s B=%d T=%d D=%d E=128 H=%d L=5 K=%d" % (kind[3:], B, T, D, H, K)
            target = tgt if kind == "ar-teacher" else None
            call = lambda: model(x, mask, lengths, target=target, tgt_init=0.25)                    # noqa: E731
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        F.mse_sum_loss_backward(call(), tgt, sum(lengths))
    return what, step


def _fwd_kernel(B, T, K, steps, warmup, dev):
    from multimodal_transformer_amd import functional as F
    c, mask = torch.randn(B, T, 1, device=dev), torch.ones(B, T, 1, device=dev)
    w = torch.randn(B, T, K, device=dev)
    w = 0.9 * w / w.abs().sum(dim=2, keepdim=True)
    for _ in range(warmup):
        F.ar_combine(c, w, mask, None, 0.25)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        F.ar_combine(c, w, mask, None, 0.25)
    b.record()
    torch.cuda.synchronize()
    print("ar_combine free-running forward B=%d T=%d K=%d: %.2f us/call (%d calls between two device events, launch gaps included)"
          % (B, T, K, a.elapsed_time(b) * 1e3 / steps, steps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b1")
    ap.add_argument("--batches", default="10,25")
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--h-dim", type=int, default=256)
    ap.add_argument("--ar-order", type=int, default=1)
    ap.add_argument("--fwd-kernel", action="store_true")
    args = ap.parse_args()
    kinds = args.model.split(",")
    for k in kinds:
        if k not in ("b1", "lstm", "ar-free", "ar-teacher"):
            ap.error("--model: b1, lstm, ar-free or ar-teacher, got %r" % k)
    from multimodal_transformer_amd import functional as F
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    for B in [int(b) for b in args.batches.split(",")]:
        built = [_build(k, B, args.T, args, dev) for k in kinds]
        for _, step in built:
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        for run in range(args.runs):
            for what, step in built:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.steps
                F.check_device_errors()
                print("%s: %.3f ms/train step (%d steps, run %d)" % (what, dt * 1e3, args.steps, run + 1), flush=True)
        del built
        if args.fwd_kernel:
            _fwd_kernel(B, args.T, args.ar_order, args.steps, args.warmup, dev)


if __name__ == "__main__":
    main()
