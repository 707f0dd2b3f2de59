"""Developer tool (not bench.py): what it costs to move an encoder stream forward by C windows from position t, by ONE extend
against C steps (and, at t = 0, against one prefill).

    python tools/extend_bench.py [--batch 32] [--d 128] [--h 8] [--layers 2 6] [--C 1 4 16 64] [--t 0 483] [--blocks 5] [--out FILE.json]

Per stack depth, start position and chunk it times, with device events on one stream, after a warm-up of every shape timed:
  * EncoderStream.extend of the C windows (ceil(C / 16) launches of encoder_extend_kernel), the stream set back to t before each call;
  * C calls of EncoderStream.step of the same stream from the same t: the only route to the same state without extend.  The step path
    is not changed by extend, so this is the baseline;
  * at t = 0, EncoderStream.prefill of the C windows (the fused stack's eval forward and the fill kernel).
The cache holds t windows of the same recording before anything is timed (one extend from 0), and every route leaves it as it found
it below t.  The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and
highest block beside it, and `extend_wins` says whether the two medians lie further apart than both spreads together.  All routes are
timed as a caller sees them: host enqueue included.  One JSON line per (depth, t, C) on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402


def bench(args, n_layers, t0, C, dev):
    MT = m.multiTransformer
    B, d, h, f = args.batch, args.d, args.h, args.d_ff
    torch.manual_seed(1234 + n_layers)
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, 0.1), 0.1), n_layers).to(dev).eval()
    MT.causal_attention(enc)
    torch.manual_seed(99)
    T = t0 + C
    x = torch.randn(B, T, d, device=dev)
    mask = torch.ones(B, T, 1, device=dev)
    xc, mc = x[:, t0:].contiguous(), mask[:, t0:].contiguous()
    rows, mrows = [x[:, t].contiguous() for t in range(t0, T)], [mask[:, t].contiguous() for t in range(t0, T)]
    s = enc.stream(B, T)

    def extend():
        s.t = t0
        s.extend(xc, mc)

    def stepped():
        s.t = t0
        for i in range(C):
            s.step(rows[i], mrows[i])

    def prefill():
        s.reset()
        s.prefill(xc, mc)

    routes = {"extend": (extend, 20), "stepped": (stepped, max(2, 20 // C))}
    if t0 == 0:
        routes["prefill"] = (prefill, 20)
    with torch.no_grad():
        if t0:
            s.extend(x[:, :t0].contiguous(), mask[:, :t0].contiguous())      # the history every route starts from
        for fn, _ in routes.values():                                        # warm-up
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in routes}
        for _ in range(args.blocks):                                         # alternating blocks
            for k, (fn, reps) in routes.items():
                res[k].append(timed_us(fn, reps))
        torch.cuda.synchronize()
    out = {"what": "encoder stream extend vs C steps", "B": B, "d": d, "h": h, "d_ff": f, "n_layers": n_layers, "t": t0, "C": C,
           "blocks": args.blocks}
    for k in routes:
        out[("C_steps" if k == "stepped" else k) + "_us"] = spread(res[k])
    e, st = out["extend_us"], out["C_steps_us"]
    gap = st["median_us"] - e["median_us"]
    noise = (e["max_us"] - e["min_us"]) + (st["max_us"] - st["min_us"])
    out["steps_over_extend"] = round(st["median_us"] / e["median_us"], 2)
    out["extend_wins"] = bool(gap > noise)
    out["steps_win"] = bool(-gap > noise)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--h", type=int, default=8)
    ap.add_argument("--d-ff", dest="d_ff", type=int, default=128)
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--C", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--t", type=int, nargs="+", default=[0, 483])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if any(C < 1 for C in args.C) or any(t < 0 for t in args.t) or max(args.t) + max(args.C) > 4096:
        raise SystemExit("extend_bench: C >= 1, t >= 0 and t + C <= 4096, the limit of a plain cache")
    dev = torch.device("cuda:0")
    lines = []
    for n in args.layers:
        for t0 in args.t:
            for C in args.C:
                lines.append(json.dumps(bench(args, n, t0, C, dev)))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
