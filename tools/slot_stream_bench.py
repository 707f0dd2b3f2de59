"""Developer tool (not bench.py): what the slots form of a stream step costs beside the host-t form, eager and replayed.

    python tools/slot_stream_bench.py [--batch 32] [--capacity 512] [--blocks 5] [--reps 200] [--out FILE.json]

Three routes of ONE step at a fixed position t, for an encoder stack (d = 128, h = 8, d_ff = 128, N = 2 and 6) and for the AVL MFT at
the reference sizes (window embeds 88 / 256 / 300, d = 256, h = 8, d_ff = 128, N = 6, modality streams on):
  (a) host_t      Encoder.stream / MultiTransformer.stream: t a launch argument, set on the host before every call;
  (b) slots       slot_stream, eager: every position set to t once, steps with advance off so that it stays there (the kernel then
                  skips only its last store, one dword by one thread);
  (c) replay      the same step captured once (graphs.capture_step, every slot idle during the capture) and replayed.
Protocol of DESIGN 4.5: device events around `reps` back-to-back calls on one stream, every shape and route warmed up (the caches hold a
full recording), the routes alternating in blocks in one process; each figure is the median over the blocks with the lowest and the
highest block beside it.  A step is timed as its caller sees it, host enqueue included.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402
from multimodal_transformer_amd import graphs  # noqa: E402

STEPS_AT = (0, 100, 300, 499)
WINDOWS = 500
MODS = ["acoustic", "image", "linguistic"]
EMBED = {"acoustic": 88, "image": 256, "linguistic": 300}


def capture(z, step):
    """`step` (a call of z.step with advance off) as a graph, captured with every slot idle -> the graph"""
    saved = z.positions.clone()
    z.positions.fill_(-1)
    g, _ = graphs.capture_step(step)
    z.positions.copy_(saved)
    return g


def run_routes(args, set_host_t, host_step, z, slots_step, record):
    """The three routes at every t of STEPS_AT -> {route: {t: [block values]}}.  record(): a whole recording through both streams, so
    that their caches and carried states hold all the windows before a step at a fixed t is repeated."""
    record()
    g = capture(z, slots_step)

    def host_at(t):
        def fn():
            set_host_t(t)
            host_step()
        return fn

    res = {k: {t: [] for t in STEPS_AT} for k in ("host_t", "slots", "replay")}
    for t in STEPS_AT:                                       # warm-up of every route at every t
        host_at(t)()
        z.positions.fill_(t)
        slots_step()
        g.replay()
    torch.cuda.synchronize()
    for _ in range(args.blocks):                             # alternating blocks
        for t in STEPS_AT:
            res["host_t"][t].append(timed_us(host_at(t), args.reps))
            z.positions.fill_(t)
            res["slots"][t].append(timed_us(slots_step, args.reps))
            res["replay"][t].append(timed_us(g.replay, args.reps))
    pos = z.positions.cpu().tolist()
    assert pos == [STEPS_AT[-1]] * len(pos), pos             # advance off: the positions stayed where they were put
    return {k: {str(t): spread(v) for t, v in r.items()} for k, r in res.items()}


def bench_encoder(args, dev, n_layers):
    MT = m.multiTransformer
    B, d, h, f = args.batch, 128, 8, 128
    torch.manual_seed(1234)
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, 0.1), 0.1), n_layers).to(dev).eval()
    MT.causal_attention(enc)
    x = torch.randn(B, WINDOWS, d, device=dev)
    rows = [x[:, t].contiguous() for t in range(WINDOWS)]
    s, z = enc.stream(B, args.capacity), enc.slot_stream(B, args.capacity)
    row = rows[1]

    def record():
        s.reset(), z.reset()
        for t in range(WINDOWS):
            s.step(rows[t]), z.step(rows[t])

    def set_t(t):
        s.t = t

    out = run_routes(args, set_t, lambda: s.step(row), z, lambda: z.step(row, advance=False), record)
    s.t = 7
    z.positions.fill_(7)
    out["rows_equal_at_t7"] = bool(torch.equal(s.step(row), z.step(row)))
    return out


def bench_mft(args, dev):
    MT = m.multiTransformer
    B = args.batch
    torch.manual_seed(1234)
    mft = MT.MultiTransformer(MODS, EMBED, N=6, device=dev).eval()
    MT.causal_attention(mft)
    x = {k: torch.randn(B, WINDOWS, EMBED[k], device=dev) for k in MODS}
    rows = [{k: x[k][:, t].contiguous() for k in MODS} for t in range(WINDOWS)]
    s, z = mft.stream(B, args.capacity), mft.slot_stream(B, args.capacity)
    row = rows[1]

    def record():
        s.reset(), z.reset()
        for t in range(WINDOWS):
            s.step(rows[t]), z.step(rows[t])

    def set_t(t):
        s.gate.t = t
        for e in s.encs.values():
            e.t = t

    out = run_routes(args, set_t, lambda: s.step(row), z, lambda: z.step(row, advance=False), record)
    set_t(7)
    z.positions.fill_(7)
    out["rows_equal_at_t7"] = bool(torch.equal(s.step(row), z.step(row)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slot_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.capacity < WINDOWS:
        raise SystemExit("slot_stream_bench: capacity must hold the %d-window recording" % WINDOWS)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        out = {"what": "stream step: host-t, slots eager, slots replayed", "B": args.batch, "capacity": args.capacity, "blocks": args.blocks,
               "reps": args.reps, "encoder": {"d": 128, "h": 8, "d_ff": 128},
               "mft": {"mods": MODS, "window_embed": EMBED, "d": 256, "h": 8, "d_ff": 128, "n_layers": 6}}
        out["encoder_n2_us"] = bench_encoder(args, dev, 2)
        out["encoder_n6_us"] = bench_encoder(args, dev, 6)
        out["mft_avl_us"] = bench_mft(args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
