"""Developer tool (not bench.py): what one window costs when the MFT (MultiTransformer) and B3-MFN are run online.

    python tools/mfn_stream_bench.py [--batch 32] [--layers 6] [--capacity 512] [--blocks 5] [--out FILE.json]

The model is the AVL configuration at the reference sizes (window embeds 88 / 256 / 300, d = 256, h = 8, d_ff = 128).  With device
events around repeated calls on one stream, after a warm-up of every shape timed, it times
  * MultiTransformer.stream's step at t = 0, 100, 300 and 499 (the caches hold a full recording; the step at a fixed t is repeated,
    which rewrites cache row t and the carried state with the same values), on one stream and with the per-modality launches forked
    onto the modality streams, the MFN step alone (MFNStream.step: its share of the whole step), and a whole 500-window recording;
  * the only online route without the stream: MultiTransformer.forward (causal, eval) on the prefix x[:, :t + 1] at the same t (the
    slice is made contiguous inside the timed call: it is part of that route), a whole recording that way (500 forwards), and the
    one offline batch forward at T = 500;
  * MultiTransformerB3.stream's step (embeds + the MFN step; nothing depends on t), on one stream and forked.
The blocks alternate between the routes in one process; each figure is the median over the blocks with the lowest and highest block
beside it.  A step is timed as a caller sees it: host enqueue included, so it cannot drop below the launch rate of the host.
One JSON line on stdout (and in --out)."""
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
MODS = ["acoustic", "image", "linguistic"]
EMBED = {"acoustic": 88, "image": 256, "linguistic": 300}


def bench(args, dev):
    MT = m.multiTransformer
    B, T = args.batch, WINDOWS
    torch.manual_seed(1234)
    mft = MT.MultiTransformer(MODS, EMBED, N=args.layers, device=dev).eval()
    MT.causal_attention(mft)
    b3 = MT.MultiTransformerB3(MODS, EMBED, device=dev).eval()
    x = {k: torch.randn(B, T, EMBED[k], device=dev) for k in MODS}
    mask = torch.ones(B, T, 1, device=dev)
    lengths = [T] * B
    rows = [{k: x[k][:, t].contiguous() for k in MODS} for t in range(T)]
    s = mft.stream(B, args.capacity)
    sb = b3.stream(B)
    gate_rows = {k: torch.randn(B, mft.embed_dim[k], device=dev) for k in MODS}

    def recording():
        s.reset()
        for t in range(T):
            s.step(rows[t])

    def recording_by_prefix():
        for t in range(T):
            mft({k: x[k][:, :t + 1].contiguous() for k in MODS}, mask[:, :t + 1], lengths)

    def step_at(t, forked):
        def fn():
            s.modality_streams = forked
            s.gate.t = t
            for e in s.encs.values():
                e.t = t
            s.step(rows[t])
        return fn

    def gate_at(t):
        def fn():
            s.gate.t = t
            s.gate.step(gate_rows)
        return fn

    def prefix_at(t):
        return lambda: mft({k: x[k][:, :t + 1].contiguous() for k in MODS}, mask[:, :t + 1], lengths)

    def b3_step(forked):
        def fn():
            sb.modality_streams = forked
            sb.gate.t = 1
            sb.step(rows[1])
        return fn

    with torch.no_grad():
        recording()                                            # warm-up of every shape; the caches now hold all 500 windows
        for t in STEPS_AT:
            step_at(t, False)(), step_at(t, True)(), gate_at(t)(), prefix_at(t)()
        b3_step(False)(), b3_step(True)()
        y_batch = mft(x, mask, lengths)
        torch.cuda.synchronize()
        keys = ("step_one_stream", "step_forked", "mfn_step", "prefix_forward")
        res = {k: {t: [] for t in STEPS_AT} for k in keys}
        res.update(recording=[], recording_by_prefix=[], batch_forward_T500=[], b3_step_one_stream=[], b3_step_forked=[])
        for blk in range(args.blocks):                         # alternating blocks
            for t in STEPS_AT:
                res["step_one_stream"][t].append(timed_us(step_at(t, False), 200))
                res["step_forked"][t].append(timed_us(step_at(t, True), 200))
                res["mfn_step"][t].append(timed_us(gate_at(t), 300))
                res["prefix_forward"][t].append(timed_us(prefix_at(t), 10))
            s.modality_streams = True                               # the recording runs as a caller gets it: forked
            res["recording"].append(timed_us(recording, 1))
            if blk < args.prefix_blocks:
                res["recording_by_prefix"].append(timed_us(recording_by_prefix, 1))
            res["batch_forward_T500"].append(timed_us(lambda: mft(x, mask, lengths), 5))
            res["b3_step_one_stream"].append(timed_us(b3_step(False), 300))
            res["b3_step_forked"].append(timed_us(b3_step(True), 300))
        s.modality_streams = True                               # the two routes agree on the last window
        s.reset()
        last = None
        for t in range(T):
            last = s.step(rows[t])
        torch.cuda.synchronize()
        agree = float((last - y_batch[:, T - 1]).norm() / y_batch[:, T - 1].norm())
    out = {"what": "MFT stream step vs prefix recomputation", "B": B, "mods": MODS, "window_embed": EMBED, "d": 256, "h": 8, "d_ff": 128,
           "n_layers": args.layers, "capacity": args.capacity, "blocks": args.blocks}
    for k in keys:
        out[k + "_us"] = {str(t): spread(v) for t, v in res[k].items()}
    for k in ("recording", "recording_by_prefix", "batch_forward_T500", "b3_step_one_stream", "b3_step_forked"):
        out[k + "_us"] = spread(res[k])
    out["window_499_rel_l2_step_vs_batch"] = agree
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--prefix-blocks", dest="prefix_blocks", type=int, default=3, help="blocks that also time a whole recording by prefix forwards")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mfn_stream_bench: no HIP device (a timing needs the GPU; there is no CPU path)")
    if args.capacity < WINDOWS:
        raise SystemExit("mfn_stream_bench: capacity must hold the %d-window recording" % WINDOWS)
    line = json.dumps(bench(args, torch.device("cuda:0")))
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
