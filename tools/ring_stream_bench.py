"""Developer tool (not bench.py): what one window costs when a causal encoder stack with a span is run online from a ring K/V cache,
against the plain stream of the same stack without a span.

    python tools/ring_stream_bench.py [--batch 32] [--d 128] [--h 8] [--layers 2 6] [--spans 32 64 128] [--blocks 5] [--out FILE.json]

Per stack depth it times, with device events around repeated calls on one stream, after a warm-up of every shape timed:
  * EncoderRingStream.step at spans 32, 64 and 128, at t = 0, span - 1, 499, 5000 and 100 000.  The positions are SET, not stepped to:
    a ring that has been walked round twice holds defined values in every row, and the step at a fixed t is repeated, which rewrites
    ring row t mod span with the same values;
  * EncoderStream.step of the same weights without a span (capacity 512, the cache filled by one recording) at t = 0, span - 1 and 499.
The claim to check is "constant cost": a ring step at any t >= span - 1 against the plain step at t = span - 1, which sweeps the same
number of keys with the kernel the ring form was derived from.  The margin to read the comparison with is the plain step's own
spread over the blocks, which is reported beside it.
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

RING_AT = (0, None, 499, 5000, 100000)          # None: span - 1
PLAIN_CAPACITY = 512
REPS = 300


def _encoder(args, n_layers, dev, span):
    MT = m.multiTransformer
    torch.manual_seed(1234 + n_layers)                       # the same weights with and without the span
    enc = MT.Encoder(MT.EncoderLayer(args.d, MT.MultiHeadedAttention(args.h, args.d), MT.PositionwiseFeedForward(args.d, args.d_ff, 0.1),
                                     0.1), n_layers).to(dev).eval()
    MT.causal_attention(enc, True, span=span)
    return enc


def bench_depth(args, n_layers, dev):
    B, d = args.batch, args.d
    torch.manual_seed(99)
    rows = [torch.randn(B, d, device=dev) for _ in range(PLAIN_CAPACITY)]
    plain = _encoder(args, n_layers, dev, None).stream(B, PLAIN_CAPACITY)
    rings = {span: _encoder(args, n_layers, dev, span).ring_stream(B) for span in args.spans}
    plain_at = sorted({0, 499} | {span - 1 for span in args.spans})
    ring_at = {span: [span - 1 if t is None else t for t in RING_AT] for span in args.spans}

    def step_at(s, t):
        def fn():
            s.t = t
            s.step(rows[t % PLAIN_CAPACITY])
        return fn

    with torch.no_grad():
        for t in range(PLAIN_CAPACITY):                        # warm-up; the cache then holds a whole recording
            plain.step(rows[t])
        for span, s in rings.items():
            for t in range(2 * span):                          # every row of the ring holds a window
                s.step(rows[t])
            for t in ring_at[span]:
                step_at(s, t)()
        for t in plain_at:
            step_at(plain, t)()
        torch.cuda.synchronize()
        res = {"plain": {t: [] for t in plain_at}, "ring": {span: {t: [] for t in ring_at[span]} for span in args.spans}}
        for _ in range(args.blocks):                           # alternating blocks
            for span in args.spans:
                res["plain"][span - 1].append(timed_us(step_at(plain, span - 1), REPS))
                for t in ring_at[span]:
                    res["ring"][span][t].append(timed_us(step_at(rings[span], t), REPS))
            for t in (0, 499):
                res["plain"][t].append(timed_us(step_at(plain, t), REPS))
        # while t < span the ring step is the plain step: the two routes give the same row, bit for bit, at t = min span - 1
        t = min(args.spans) - 1
        s, p = rings[min(args.spans)], plain
        s.reset(), p.reset()
        same = all(torch.equal(s.step(rows[i]), p.step(rows[i])) for i in range(t + 1))
        torch.cuda.synchronize()
    return {"what": "encoder ring stream step vs plain stream step", "B": B, "d": d, "h": args.h, "d_ff": args.d_ff, "n_layers": n_layers,
            "blocks": args.blocks, "reps": REPS,
            "plain_step_us": {str(t): spread(v) for t, v in res["plain"].items()},
            "ring_step_us": {str(span): {str(t): spread(v) for t, v in by_t.items()} for span, by_t in res["ring"].items()},
            "rows_below_span_bit_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--h", type=int, default=8)
    ap.add_argument("--d-ff", dest="d_ff", type=int, default=128)
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--spans", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ring_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if any(not 1 <= span <= PLAIN_CAPACITY for span in args.spans):
        raise SystemExit("ring_stream_bench: spans must lie in [1, %d], the plain stream's capacity here" % PLAIN_CAPACITY)
    dev = torch.device("cuda:0")
    lines = [json.dumps(bench_depth(args, n, dev)) for n in args.layers]
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
