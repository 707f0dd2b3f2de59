"""Developer tool (not bench.py): what one window costs when a causal encoder stack is run online.

    python tools/stream_bench.py [--batch 32] [--d 128] [--h 8] [--layers 2 6] [--capacity 512] [--blocks 5] [--out FILE.json]

Per stack depth it times, with device events around repeated calls on one stream, after a warm-up of every shape timed:
  * EncoderStream.step at t = 0, 100, 300 and 499 (the cache holds a full recording; the step at a fixed t is repeated, which rewrites
    cache row t with the same values), and the whole 500-window recording;
  * the only online route without the stream: Encoder.forward (causal, eval) on the prefix x[:, :t + 1] at the same t, and one batch
    forward at T = 500.
The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and highest block
beside it.  A step is timed as a caller sees it: host enqueue included, so it cannot drop below the launch rate of the host.
One JSON line per depth on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402

STEPS_AT = (0, 100, 300, 499)
WINDOWS = 500


def bench_depth(args, n_layers, dev):
    MT = m.multiTransformer
    B, d, T = args.batch, args.d, WINDOWS
    torch.manual_seed(1234 + n_layers)
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(args.h, d), MT.PositionwiseFeedForward(d, args.d_ff, 0.1), 0.1), n_layers)
    enc = enc.to(dev).eval()
    MT.causal_attention(enc)
    x = torch.randn(B, T, d, device=dev)
    mask = torch.ones(B, T, 1, device=dev)
    rows = [x[:, t].contiguous() for t in range(T)]
    prefixes = {t: (x[:, :t + 1].contiguous(), mask[:, :t + 1].contiguous()) for t in STEPS_AT}
    s = enc.stream(B, args.capacity)

    def recording():
        s.reset()
        for t in range(T):
            s.step(rows[t])

    def step_at(t):
        def fn():
            s.t = t
            s.step(rows[t])
        return fn

    def prefix_at(t):
        xp, mp = prefixes[t]
        return lambda: enc(xp, mp)

    with torch.no_grad():
        recording()                                            # warm-up of every shape; the cache now holds all 500 windows
        for t in STEPS_AT:
            step_at(t)()
            prefix_at(t)()
        enc(x, mask)
        torch.cuda.synchronize()
        res = {"step": {t: [] for t in STEPS_AT}, "prefix_forward": {t: [] for t in STEPS_AT}, "recording": [], "batch_forward_T500": []}
        for _ in range(args.blocks):                           # alternating blocks
            for t in STEPS_AT:
                res["step"][t].append(timed_us(step_at(t), 300))
                res["prefix_forward"][t].append(timed_us(prefix_at(t), 30))
            res["recording"].append(timed_us(recording, 2))
            res["batch_forward_T500"].append(timed_us(lambda: enc(x, mask), 20))
        y_batch = enc(x, mask)                                 # the two routes agree on the last row (the cache is whole after a recording)
        s.t = T - 1
        y_step = s.step(rows[T - 1])
        torch.cuda.synchronize()
        agree = float((y_step - y_batch[:, T - 1]).norm() / y_batch[:, T - 1].norm())
    return {"what": "encoder stream step vs prefix recomputation", "B": B, "d": d, "h": args.h, "d_ff": args.d_ff, "n_layers": n_layers,
            "capacity": args.capacity, "blocks": args.blocks,
            "step_us": {str(t): spread(v) for t, v in res["step"].items()},
            "prefix_forward_us": {str(t): spread(v) for t, v in res["prefix_forward"].items()},
            "recording_500_windows_us": spread(res["recording"]), "batch_forward_T500_us": spread(res["batch_forward_T500"]),
            "row_499_rel_l2_step_vs_batch": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--h", type=int, default=8)
    ap.add_argument("--d-ff", dest="d_ff", type=int, default=128)
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.capacity < WINDOWS:
        raise SystemExit("stream_bench: capacity must hold the %d-window recording" % WINDOWS)
    dev = torch.device("cuda:0")
    lines = [json.dumps(bench_depth(args, n, dev)) for n in args.layers]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
