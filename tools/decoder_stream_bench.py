"""Developer tool (not bench.py): what a step of the SFT costs as stream() runs it and as device_stream() runs it, eager and replayed.

    python tools/decoder_stream_bench.py [--batch 32] [--capacity 512] [--blocks 5] [--reps 200] [--out FILE.json]

Three routes of ONE step at a fixed position t of NLPTransformer(512, embed_dim 128, h_dim 128, h = 8, d_ff = 128), N = 2 and N = 6:
  (a) stream          model.stream: t and the decoder's (h, c) on the host; the embed affine map, encoder_step_kernel, then the decoder
                      as the batch kernels at T = 1 (linear, add_row0 at t == 0, lstm_scan, two read-out linears);
  (b) device_stream   model.device_stream, eager: every position set to t once, steps with advance off so that it stays there; three
                      kernels (the embed's row GEMM, encoder_step_slots_kernel, decoder_step_slots_kernel);
  (c) replay          (b) captured once (graphs.capture_step, every slot idle during the capture) and replayed.
Protocol of DESIGN 4.5 / 4.7: device events around `reps` back-to-back calls on one stream, every shape and route warmed up (the caches
hold a full recording), the routes alternating in blocks in one process; each figure is the median over the blocks with the lowest and
the highest block beside it.  A step is timed as its caller sees it, host enqueue included.  The rows of (a) and (b) at t = 7 of one
recording stepped in lockstep are held under the lockstep bound of the tests (tests/decoder_stream_ref.py DEC_STEP_VS_STREAM / _ROW):
the JSON line is written first, to stdout and --out, and rows outside the bound end the tool with exit status 1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import multimodal_transformer_amd as m  # noqa: E402
from stream_bench_common import spread, timed_us  # noqa: E402
from multimodal_transformer_amd import graphs  # noqa: E402
from decoder_stream_ref import DEC_STEP_VS_STREAM as VS_STREAM, DEC_STEP_VS_STREAM_ROW as VS_STREAM_ROW  # noqa: E402

STEPS_AT = (0, 100, 300, 499)
WINDOWS = 500
WIDTH, D, H = 512, 128, 8


def bench_sft(args, dev, n_layers):
    MT = m.multiTransformer
    B = args.batch
    torch.manual_seed(1234)
    model = MT.NLPTransformer(WIDTH, embed_dim=D, h=H, N=n_layers, device=dev).eval()
    with torch.no_grad():
        model.dec_h0.normal_(0.0, 0.1)
        model.dec_c0.normal_(0.0, 0.1)
    MT.causal_attention(model)
    x = torch.randn(B, WINDOWS, WIDTH, device=dev)
    rows = [x[:, t].contiguous() for t in range(WINDOWS)]
    s, z = model.stream(B, args.capacity), model.device_stream(B, args.capacity)
    row = rows[1]

    # the rows of both routes at t = 7 of one recording, in lockstep
    s.reset(), z.reset()
    for t in range(8):
        ya, yb = s.step(rows[t]), z.step(rows[t])
    ya, yb = ya.double().cpu().numpy(), yb.double().cpu().numpy()
    rel = float(np.linalg.norm(yb - ya) / np.linalg.norm(ya))
    per_row = float(np.abs(yb - ya).max() / np.sqrt(np.mean(ya * ya)))

    s.reset(), z.reset()
    for t in range(WINDOWS):                                 # the caches and the carried states hold a whole recording
        s.step(rows[t]), z.step(rows[t])

    def host_at(t):
        def fn():
            s.enc.t = t
            s.step(row)
        return fn

    def dev_step():
        return z.step(row, advance=False)

    saved = z.positions.clone()
    z.positions.fill_(-1)
    g, _ = graphs.capture_step(dev_step)
    z.positions.copy_(saved)
    res = {k: {t: [] for t in STEPS_AT} for k in ("stream", "device_stream", "replay")}
    for t in STEPS_AT:                                       # warm-up of every route at every t
        host_at(t)()
        z.positions.fill_(t)
        dev_step()
        g.replay()
    torch.cuda.synchronize()
    for _ in range(args.blocks):                             # alternating blocks
        for t in STEPS_AT:
            res["stream"][t].append(timed_us(host_at(t), args.reps))
            z.positions.fill_(t)
            res["device_stream"][t].append(timed_us(dev_step, args.reps))
            res["replay"][t].append(timed_us(g.replay, args.reps))
    pos = z.positions.cpu().tolist()
    assert pos == [STEPS_AT[-1]] * len(pos), pos             # advance off: the positions stayed where they were put
    out = {k: {str(t): spread(v) for t, v in r.items()} for k, r in res.items()}
    out["rows_at_t7"] = {"rel_l2": rel, "per_row": per_row, "bound_rel_l2": VS_STREAM, "bound_per_row": VS_STREAM_ROW,
                         "within_bound": bool(rel <= VS_STREAM and per_row <= VS_STREAM_ROW)}
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
        raise SystemExit("decoder_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.capacity < WINDOWS:
        raise SystemExit("decoder_stream_bench: capacity must hold the %d-window recording" % WINDOWS)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        out = {"what": "SFT step: stream(), device_stream() eager, device_stream() replayed", "B": args.batch, "capacity": args.capacity,
               "blocks": args.blocks, "reps": args.reps,
               "sft": {"window_embed": WIDTH, "d": D, "h": H, "d_ff": 128, "h_dim": 128, "decoder_layers": 1}}
        out["sft_n2_us"] = bench_sft(args, dev, 2)
        out["sft_n6_us"] = bench_sft(args, dev, 6)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    outside = [k for k in ("sft_n2_us", "sft_n6_us") if not out[k]["rows_at_t7"]["within_bound"]]
    if outside:
        raise SystemExit("decoder_stream_bench: the rows of stream() and device_stream() at t = 7 are outside the lockstep bound "
                         "%.1e / %.1e in %s: %s" % (VS_STREAM, VS_STREAM_ROW, outside, [out[k]["rows_at_t7"] for k in outside]))


if __name__ == "__main__":
    main()
