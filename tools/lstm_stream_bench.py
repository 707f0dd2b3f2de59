"""Developer tool (not bench.py): what one window costs when the LSTM baselines (MultiLSTM, MultiLSTMB1) are run online.

    python tools/lstm_stream_bench.py [--batch 32] [--prefix 64] [--blocks 5] [--out FILE.json]

Two shapes at B = 32: the shared copy (300 -> E 128, H 256, L 5: the shipped checkpoint's configuration) and B1's (1556 -> E 512, H 256,
L 5), both with models.attend_over_taps on, eval mode.  With device events around repeated calls on one stream, after a warm-up of
every shape timed, it times
  * the step of stream() (lstm_step_kernel, the position by value), of slot_stream() (lstm_step_slots_kernel, positions on the device,
    advance off so that the position stays) and of slot_stream() replayed from a graph (graphs.capture_stream), all at position
    --prefix - 1: nothing in a step depends on how long the recording already is, only on whether the position is 0;
  * what a user must do today for one new window: the model's batch forward over the --prefix-window prefix, and the same forward at
    T = 1 (which gives the first window only: it is the floor of that route, not an alternative).
The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and highest block
beside it.  A step is timed as a caller sees it: host enqueue included, so an eager step cannot drop below the launch rate of the
host; the replayed graph shows the kernel.  The last window of a --prefix-window recording is also compared between the stream and
the batch forward (rel-L2, printed).  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402

SHAPES = {"shared_300_E128_H256_L5": ("MultiLSTM", 300), "b1_1556_E512_H256_L5": ("MultiLSTMB1", 1556)}


def bench_shape(cls, width, args, dev):
    B, T = args.batch, args.prefix
    torch.manual_seed(1234)
    model = getattr(m.models, cls)(width, device=dev).eval()
    m.models.attend_over_taps(model)
    x = torch.randn(B, T, width, device=dev)
    mask = torch.ones(B, T, 1, device=dev)
    rows = [x[:, t].contiguous() for t in range(T)]
    ones = torch.ones(B, device=dev)
    s, z, zg = model.stream(B), model.slot_stream(B), model.slot_stream(B)
    with torch.no_grad():
        for stream in (z, zg):                                 # a whole recording each: the state of position T - 1 is a real one
            stream.reset()
            for t in range(T - 1):
                stream.step(rows[t], ones)
        last = None
        for t in range(T):
            last = s.step(rows[t], ones)
        y_batch = model(x, mask, [T] * B)
        agree = float((last - y_batch[:, T - 1]).norm() / y_batch[:, T - 1].norm())
        graph = m.graphs.capture_stream(zg, rows[T - 1], ones)
        x1, mask1 = x[:, :1].contiguous(), mask[:, :1].contiguous()

        def host_step():
            s.t = T - 1
            s.step(rows[T - 1], ones)

        def slot_step():
            z.step(rows[T - 1], ones, advance=False)

        def replay():
            zg.positions.fill_(T - 1)                          # the captured step advances; one small fill per replay puts it back
            graph.replay()

        routes = {"stream_step": (host_step, 300), "slot_stream_step": (slot_step, 300), "slot_stream_graph_replay": (replay, 300),
                  "batch_forward_prefix": (lambda: model(x, mask, [T] * B), 20), "batch_forward_T1": (lambda: model(x1, mask1, [1] * B), 50)}
        for fn, _ in routes.values():
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in routes}
        for _ in range(args.blocks):                           # alternating blocks
            for k, (fn, reps) in routes.items():
                res[k].append(timed_us(fn, reps))
        fill_only = [timed_us(lambda: zg.positions.fill_(T - 1), 300) for _ in range(args.blocks)]
    out = {k + "_us": spread(v) for k, v in res.items()}
    out["positions_fill_us"] = spread(fill_only)
    out["last_window_rel_l2_stream_vs_batch"] = agree
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--prefix", type=int, default=64, help="windows of the prefix the batch forward recomputes; the steps run at position prefix - 1")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.prefix < 2:
        raise SystemExit("lstm_stream_bench: --prefix must be at least 2")
    dev = torch.device("cuda:0")
    out = {"what": "LSTM baseline stream step vs batch recomputation", "B": args.batch, "prefix": args.prefix, "blocks": args.blocks}
    for name, (cls, width) in SHAPES.items():
        out[name] = bench_shape(cls, width, args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
