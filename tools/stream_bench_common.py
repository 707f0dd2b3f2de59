"""What the stream bench tools (tools/*stream_bench.py) share: the timing of a route and the summary of its blocks."""
import statistics

import torch


def timed_us(fn, reps):
    """microseconds per call of fn over `reps` back-to-back calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def spread(vals):
    return {"median_us": round(statistics.median(vals), 2), "min_us": round(min(vals), 2), "max_us": round(max(vals), 2)}
