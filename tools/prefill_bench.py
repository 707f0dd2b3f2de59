"""Developer tool (not bench.py): what it costs to open a recording from a history of P windows, by ONE prefill against P steps.

    python tools/prefill_bench.py [--batch 32] [--d 128] [--h 8] [--layers 2 6] [--P 64 499] [--blocks 5] [--out FILE.json]

Per stack depth and history length it times, with device events on one stream, after a warm-up of every shape timed:
  * EncoderStream.prefill of the P windows (the fused stack's eval forward and the fill kernel), the stream reset before each call;
  * P calls of EncoderStream.step of the same stream from t = 0: the route a recording with a history takes without prefill.  The step
    path is not changed by prefill, so this is the baseline;
  * the fill kernel alone (functional's C entry on the workspace the last forward left), against the bytes it moves:
    2 N B h P dkp 2 written and the same read.
The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and highest block
beside it.  Both routes are timed as a caller sees them: host enqueue included.  One JSON line per (depth, P) on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402

CAPACITY = 512
FILL_REPS = 200


def bench(args, n_layers, P, dev):
    MT, F, L = m.multiTransformer, m.functional, m._lib
    B, d, h, f = args.batch, args.d, args.h, args.d_ff
    torch.manual_seed(1234 + n_layers)
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, 0.1), 0.1), n_layers).to(dev).eval()
    MT.causal_attention(enc)
    torch.manual_seed(99)
    x = torch.randn(B, P, d, device=dev)
    mask = torch.ones(B, P, 1, device=dev)
    rows, mrows = [x[:, t].contiguous() for t in range(P)], [mask[:, t].contiguous() for t in range(P)]
    s = enc.stream(B, CAPACITY)

    def prefill():
        s.reset()
        s.prefill(x, mask)

    def stepped():
        s.reset()
        for t in range(P):
            s.step(rows[t], mrows[t])

    # the fill alone: the workspace as one forward of these dims left it (held out of the pool while it is timed)
    dims = (B, P, d, h, f, n_layers)
    lib = L.load()
    nbytes = lib.mmt_encoder_workspace_bytes_eval(*dims)
    dkp = (d // h + 7) // 8 * 8
    moved = 2 * n_layers * B * h * P * dkp * 2

    with torch.no_grad():
        prefill(), stepped()                                   # warm-up
        ws = L.POOL.get(nbytes, dev, tag=("encoder",) + dims + (False,))
        y = torch.empty_like(x)
        L.launch("mmt_encoder_forward", x, mask.view(B, P), s._flat, y, ws, nbytes, *dims, 1e-6, 0.0, 0, causal=True)

        def fill():
            L.launch("mmt_encoder_stream_prefill", ws, nbytes, s.state, s.state.numel(), None, None, None, B, P, B, CAPACITY, 0, d, h, f, n_layers)

        fill()
        torch.cuda.synchronize()
        res = {"prefill": [], "stepped": [], "fill": []}
        for _ in range(args.blocks):                           # alternating blocks
            res["prefill"].append(timed_us(prefill, 20))
            res["stepped"].append(timed_us(stepped, 2))
            res["fill"].append(timed_us(fill, FILL_REPS))
        L.POOL.put(ws)
        torch.cuda.synchronize()
    fill_us = spread(res["fill"])
    return {"what": "encoder stream prefill vs P steps", "B": B, "d": d, "h": h, "d_ff": f, "n_layers": n_layers, "P": P, "blocks": args.blocks,
            "prefill_us": spread(res["prefill"]), "P_steps_us": spread(res["stepped"]), "fill_kernel_us": fill_us,
            "fill_bytes_written": moved, "fill_GBps_read_plus_written": round(2 * moved / (fill_us["median_us"] * 1e-6) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--h", type=int, default=8)
    ap.add_argument("--d-ff", dest="d_ff", type=int, default=128)
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--P", type=int, nargs="+", default=[64, 499])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if any(not 1 <= P <= CAPACITY for P in args.P):
        raise SystemExit("prefill_bench: P must lie in [1, %d], the stream's capacity here" % CAPACITY)
    dev = torch.device("cuda:0")
    lines = [json.dumps(bench(args, n, P, dev)) for n in args.layers for P in args.P]
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
