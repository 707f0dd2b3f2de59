"""Developer tool (not bench.py): what one window costs when MultiEDLSTM and MultiARLSTM are run online, free-running.

    python tools/lstm_feedback_stream_bench.py [--batch 32] [--prefix 64] [--blocks 5] [--width 300] [--out FILE.json]

Four shapes at B = 32, models.attend_over_taps on, eval mode: MultiEDLSTM(E 128, H 128, L 3) (the batch path's limit) and
MultiEDLSTM(E 128, H 512, L 3) (the reference's default h_dim, which the batch path refuses), MultiARLSTM(E 128, H 256, L 7, K 1) and
MultiARLSTM(E 128, H 512, L 7, K 1) (the default).  With device events around repeated calls on one stream, after a warm-up of every
route timed, it times at position --prefix - 1 (nothing in a step depends on how long the recording already is, only on whether the
position is 0)
  * the step of feedback_stream() (the position by value), of feedback_slot_stream() (positions on the device, advance off so that
    the position stays) and of feedback_slot_stream() replayed from a graph (graphs.capture_stream);
  * the same three for the plain MultiLSTM of the same E, H, L, from the same run: what the tail adds to a step.
The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and highest block
beside it.  A step is timed as a caller sees it: host enqueue included, so an eager step cannot drop below the launch rate of the
host; the replayed graph shows the kernel (plus one small fill that puts the position back, timed on its own).  Nothing is gated on
these times.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402

# name -> (class, h_dim, attn_len, ar_order or None)
SHAPES = {"ed_E128_H128_L3": ("MultiEDLSTM", 128, 3, None), "ed_E128_H512_L3": ("MultiEDLSTM", 512, 3, None),
          "ar_E128_H256_L7_K1": ("MultiARLSTM", 256, 7, 1), "ar_E128_H512_L7_K1": ("MultiARLSTM", 512, 7, 1)}


def routes_of(host, slots, graphed, rows, ones, T):
    """the three routes of one model at position T - 1: (callable, repetitions) by name, and the fill the replay needs"""
    with torch.no_grad():
        for stream in (slots, graphed):                        # a whole recording each: the state of position T - 1 is a real one
            stream.reset()
            for t in range(T - 1):
                stream.step(rows[t], ones)
        for t in range(T):
            host.step(rows[t], ones)
        graph = m.graphs.capture_stream(graphed, rows[T - 1], ones)

    def host_step():
        host.t = T - 1
        host.step(rows[T - 1], ones)

    def slot_step():
        slots.step(rows[T - 1], ones, advance=False)

    def replay():
        graphed.positions.fill_(T - 1)                         # the captured step advances; one small fill per replay puts it back
        graph.replay()

    return {"stream_step": (host_step, 300), "slot_stream_step": (slot_step, 300), "slot_stream_graph_replay": (replay, 300)}


def bench_shape(cls, H, L, K, args, dev):
    B, T, width = args.batch, args.prefix, args.width
    torch.manual_seed(1234)
    kw = {} if K is None else {"ar_order": K}
    model = getattr(m.models, cls)(width, embed_dim=128, h_dim=H, attn_len=L, device=dev, **kw).eval()
    plain = m.models.MultiLSTM(width, embed_dim=128, h_dim=H, attn_len=L, device=dev).eval()
    m.models.attend_over_taps(model)
    m.models.attend_over_taps(plain)
    rows = [torch.randn(B, width, device=dev) for _ in range(T)]
    ones = torch.ones(B, device=dev)
    routes = {}
    for prefix, (a, b, c) in (("feedback_", (model.feedback_stream(B, 0.25), model.feedback_slot_stream(B, tgt_init=0.25),
                                             model.feedback_slot_stream(B, tgt_init=0.25))),
                              ("plain_", (plain.stream(B), plain.slot_stream(B), plain.slot_stream(B)))):
        for k, v in routes_of(a, b, c, rows, ones, T).items():
            routes[prefix + k] = v
    with torch.no_grad():
        for fn, _ in routes.values():
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in routes}
        for _ in range(args.blocks):                           # alternating blocks
            for k, (fn, reps) in routes.items():
                res[k].append(timed_us(fn, reps))
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        fill_only = [timed_us(lambda: pos.fill_(T - 1), 300) for _ in range(args.blocks)]
    out = {k + "_us": spread(v) for k, v in res.items()}
    out["positions_fill_us"] = spread(fill_only)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--prefix", type=int, default=64, help="the steps run at position prefix - 1 of a real recording")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--width", type=int, default=300, help="window_embed_size, the width of the input row")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_feedback_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.prefix < 2:
        raise SystemExit("lstm_feedback_stream_bench: --prefix must be at least 2")
    dev = torch.device("cuda:0")
    out = {"what": "MultiEDLSTM / MultiARLSTM feedback stream step beside the plain MultiLSTM step", "B": args.batch, "prefix": args.prefix,
           "blocks": args.blocks, "width": args.width}
    for name, (cls, H, L, K) in SHAPES.items():
        out[name] = bench_shape(cls, H, L, K, args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
