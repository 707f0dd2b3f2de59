"""The stacked and the feedback LSTM scans against the bf16-faithful fp64 reference (tests/bf16_ref.py lstm_stack_scan / lstm_fb_scan).

test_gpu_lstm_stack.py and test_gpu_edlstm.py check csrc/scan_stack.h and csrc/scan_fb.h against plain fp64 loops with one rel-L2 per
tensor: 2e-2 on outputs, 4e-2 on gradients, 9e-2 behind the read-out's ReLU (dW1, db1, du), and no case longer than T = 13.  Here the
reference rounds where the kernels round, and every tensor is measured four ways:
  * rel-L2 of the tensor;
  * the per-row maximum (gpu_harness.measures): a row is one (t, b) for h, c, p, u, dgx0, dgxc, dG, du and dp, one sequence for dh0 and
    dc0, one output feature for the weight gradients (dw2 is one feature), one entry for the bias vectors;
  * the per-sequence maximum  max_b ||got[:, b] - ref[:, b]|| / rms_b ||ref[:, b]||  of the (T, B, .) tensors;
  * the least-squares scale <got - ref, ref> / <ref, ref> of every weight gradient.

Tiers, by shape (tier()); the measurements separate by how many bf16 roundings fp32 noise can tip, not by instance:
  * SHORT: T <= 13 and H <= 64.  Every tensor carries all of its measures.  Most cases agree with the reference to fp32 (the
    medians are 1e-7); the worst ones show single tipped roundings (a row or a sequence off by a bf16 ulp of one element);
  * WIDE:  T <= 13 and H > 64 (HPAD = 128): more units, more tips; the saturated run (gx0 x 6) sets the weight-gradient rows;
  * LONG:  T = 300, the first long runs of either kernel.  In the feedback scan at H = 40, E = 24 one read-out unit whose
    pre-activation sits at the ReLU's edge flips; the reference against itself under noise of 3e-7 flips the same unit and shows
    the same figures (dgxc 1.1e-3 / 2.4e-2 / 1.6e-3, dW1 1.2e-3 / 5.7e-3), so that is the tier's size, not a fault.
Each bound is max(4 x the worst value measured on the MI355X over the tier's cases, the reference against itself under half an fp32
ulp of noise: tests/test_bf16_ref.py test_stack_fb_jitter_floor), rounded up to two digits; where nothing tips (fp32 agreement) it
is at least 4e-7.  Beside each constant: the measured worst as rel-L2 / per-row / per-sequence, then the reference against itself.
No per-row bound is None.  Nothing is measured against the kernels' own earlier output.

Ratio of each rel-L2 bound to the plain tests' bound for the same tensor (2e-2 outputs, 4e-2 gradients, 9e-2 dW1 / db1 / du), by
tier (test_bounds_are_tighter_than_the_plain_tests prints every one and asserts it is < 1):
  * stacked: SHORT out 0.024, dgx0 0.045, dP 0.048, dbias 0.017, dh0 / dc0 0.065; WIDE 0.015, 0.080, 0.16, 0.035, 0.065;
    LONG 0.065, 0.16, 0.21, 0.060, 0.085;
  * feedback: SHORT p 8e-4, h / c 3e-4, u 2e-3, dgxc 8e-4, dW_hh 0.013, dw_p 0.017, dW1 6e-4, db1 and db2 below 2e-5, dw2 5e-3,
    dh0 / dc0 0.012; WIDE 6e-3, 1e-3, 6e-3, 5e-3, 0.021, 0.019, 7e-4, 7e-4, 1e-5 (db2), 0.015, 0.035; LONG p 0.027, h / c 7e-3,
    u 0.024, dgxc 0.11, dW_hh 0.13, dw_p 0.075, dW1 0.053, db1 0.057, dw2 0.045, db2 0.11, dh0 / dc0 0.040;
  * the backward's own buffers: du and dp below 3e-5 (fp32 agreement), dG 2e-5 SHORT and 0.018 WIDE.

Cases: the smallest that reach every instance of the dispatch (csrc/api.hip with_stack_shape, the seqs / kblocks lambdas of
mmt_lstm_fb_scan_*; scan_stack_plan.h, scan_fb_plan.h): stack_plan() and fb_plan() below mirror it, test_every_instance_has_a_case
holds the case lists to the full grid, and each case asserts through torch.profiler which instance ran (the template arguments where
the name shows them).  These kernels read no environment switch, so everything runs in this process.
"""
import re

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import check_scan, dev, device_kernel_names, ls_scale, measures, seq_max  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

P_INIT = 0.375
PLAIN = {"out": 2e-2, "grad": 4e-2, "relu": 9e-2}      # gpu_harness OUT_RTOL, GRAD_RTOL, RELU_GRAD_RTOL: what the plain tests apply

# ------------------------------------------------------------------------------------------------ bounds
# group -> (rel-L2, per-row maximum[, per-sequence maximum]) = max(4 x measured, the reference against itself), rounded up; beside each
# the measured worst over the tier's cases as rel-L2 / per-row / per-sequence.  Groups: out = h_top, h_all, c_all; d0 = dh0, dc0;
# hc = h_all, c_all; du, dp, dG = the backward's own buffers (test_fb_scan_backward_buffers: SHORT and WIDE cases only).
STACK_SHORT = {
    "out":   (4.8e-04, 1.5e-03, 8.4e-04),   # 1.2e-04 / 3.6e-04 / 2.1e-04 (the reference against itself: 4.5e-05 / 7.0e-04 / 4.5e-04)
    "dgx0":  (1.8e-03, 1.3e-02, 1.3e-02),   # 4.4e-04 / 3.1e-03 / 3.1e-03 (the reference against itself: 1.9e-04 / 1.6e-03 / 1.4e-03)
    "dP":    (1.9e-03, 8.7e-03),            # 4.6e-04 / 2.2e-03 (the reference against itself: 5.1e-04 / 2.9e-03)
    "dbias": (6.8e-04, 4.6e-03),            # 1.7e-04 / 1.1e-03 (the reference against itself: 1.6e-04 / 9.4e-04)
    "d0":    (2.6e-03, 4.5e-03),            # 6.4e-04 / 1.1e-03 (the reference against itself: 2.6e-04 / 1.9e-03)
}
STACK_WIDE = {
    "out":   (3.0e-04, 2.9e-03, 2.3e-03),   # 7.4e-05 / 7.1e-04 / 5.5e-04 (the reference against itself: 1.8e-04 / 5.3e-04 / 3.1e-04)
    "dgx0":  (3.2e-03, 1.6e-02, 1.2e-02),   # 8.0e-04 / 3.9e-03 / 2.9e-03 (the reference against itself: 7.9e-04 / 3.2e-03 / 2.4e-03)
    "dP":    (6.5e-03, 7.0e-02),            # 1.6e-03 / 1.7e-02 (the reference against itself: 1.4e-03 / 8.8e-03)
    "dbias": (1.4e-03, 1.5e-02),            # 3.4e-04 / 3.7e-03 (the reference against itself: 2.4e-04 / 2.9e-03)
    "d0":    (2.6e-03, 5.9e-03),            # 6.4e-04 / 1.5e-03 (the reference against itself: 3.5e-04 / 1.1e-03)
}
STACK_LONG = {
    "out":   (1.3e-03, 4.2e-03, 1.4e-03),   # 3.2e-04 / 1.0e-03 / 3.4e-04 (the reference against itself: 2.7e-04 / 7.9e-04 / 3.2e-04)
    "dgx0":  (6.4e-03, 1.4e-02, 6.6e-03),   # 1.6e-03 / 3.3e-03 / 1.6e-03 (the reference against itself: 1.5e-03 / 2.9e-03 / 1.6e-03)
    "dP":    (8.4e-03, 3.0e-02),            # 2.1e-03 / 7.3e-03 (the reference against itself: 2.1e-03 / 7.6e-03)
    "dbias": (2.4e-03, 2.2e-02),            # 6.0e-04 / 5.5e-03 (the reference against itself: 4.7e-04 / 3.8e-03)
    "d0":    (3.4e-03, 4.1e-03),            # 8.5e-04 / 1.0e-03 (the reference against itself: 7.9e-04 / 1.0e-03)
}
STACK_SCALE = {"short": 7.8e-05, "wide": 7.4e-04, "long": 5.7e-04}
# least-squares scale of dP's halves: measured short 1.9e-05 (floor 8.0e-06), wide 1.8e-04 (floor 9.6e-05), long 1.4e-04 (floor 8.9e-05)
FB_SHORT = {
    "p":     (1.6e-05, 4.7e-04, 2.7e-04),   # 3.8e-06 / 1.2e-04 / 6.7e-05 (the reference against itself: 0.0e+00 / 0.0e+00 / 0.0e+00)
    "hc":    (5.9e-06, 1.9e-04, 1.1e-04),   # 1.5e-06 / 4.7e-05 / 2.7e-05 (the reference against itself: 0.0e+00 / 0.0e+00 / 0.0e+00)
    "u":     (4.4e-05, 1.2e-03, 6.7e-04),   # 1.1e-05 / 2.9e-04 / 1.7e-04 (the reference against itself: 0.0e+00 / 0.0e+00 / 0.0e+00)
    "dgxc":  (3.1e-05, 5.6e-04, 3.9e-04),   # 7.6e-06 / 1.4e-04 / 9.7e-05 (the reference against itself: 4.6e-08 / 1.6e-06 / 1.0e-06)
    "dW_hh": (5.1e-04, 6.4e-03),            # 1.3e-04 / 1.6e-03 (the reference against itself: 2.6e-07 / 4.1e-06)
    "dw_p":  (6.6e-04, 8.3e-03),            # 1.6e-04 / 2.1e-03 (the reference against itself: 2.1e-08 / 3.3e-07)
    "dW1":   (5.8e-05, 1.9e-04),            # 1.4e-05 / 4.6e-05 (the reference against itself: 0.0e+00 / 0.0e+00)
    "db1":   (4.0e-07, 6.0e-07),            # 3.6e-08 / 1.5e-07 (the reference against itself: 0.0e+00 / 0.0e+00)
    "dw2":   (2.0e-04, 2.0e-04),            # 4.8e-05 / 4.8e-05 (the reference against itself: 0.0e+00 / 0.0e+00)
    "db2":   (5.1e-07, 5.1e-07),            # 1.3e-07 / 1.3e-07 (the reference against itself: 0.0e+00 / 0.0e+00)
    "d0":    (4.8e-04, 7.7e-03),            # 1.2e-04 / 1.9e-03 (the reference against itself: 0.0e+00 / 0.0e+00)
    "du":    (4.0e-07, 8.2e-07, 4.6e-07),   # 7.2e-08 / 2.0e-07 / 1.1e-07 (the reference against itself: 0.0e+00 / 0.0e+00 / 0.0e+00)
    "dp":    (4.0e-07, 8.4e-07, 4.8e-07),   # 6.4e-08 / 2.1e-07 / 1.2e-07 (the reference against itself: 0.0e+00 / 0.0e+00 / 0.0e+00)
    "dG":    (9.0e-07, 1.9e-05, 1.3e-05),   # 2.2e-07 / 4.7e-06 / 3.1e-06 (the reference against itself: 2.6e-07 / 7.2e-06 / 4.2e-06)
}
FB_WIDE = {
    "p":     (1.2e-04, 1.6e-03, 8.8e-04),   # 1.1e-05 / 3.8e-04 / 2.2e-04 (the reference against itself: 1.1e-04 / 1.1e-03 / 6.4e-04)
    "hc":    (2.4e-05, 3.9e-04, 2.8e-04),   # 5.8e-06 / 9.6e-05 / 6.8e-05 (the reference against itself: 2.8e-06 / 6.2e-05 / 3.6e-05)
    "u":     (1.2e-04, 1.9e-03, 1.9e-03),   # 2.9e-05 / 4.7e-04 / 4.7e-04 (the reference against itself: 5.6e-05 / 5.1e-04 / 3.0e-04)
    "dgxc":  (2.1e-04, 8.7e-04, 6.7e-04),   # 5.2e-05 / 1.6e-04 / 1.0e-04 (the reference against itself: 1.1e-04 / 8.3e-04 / 6.3e-04)
    "dW_hh": (8.4e-04, 1.1e-02),            # 2.1e-04 / 2.7e-03 (the reference against itself: 3.0e-04 / 2.4e-03)
    "dw_p":  (7.6e-04, 7.9e-03),            # 1.9e-04 / 2.0e-03 (the reference against itself: 3.6e-04 / 1.9e-03)
    "dW1":   (6.3e-05, 3.7e-04),            # 1.3e-05 / 4.3e-05 (the reference against itself: 5.9e-05 / 3.5e-04)
    "db1":   (6.1e-05, 4.1e-04),            # 1.9e-08 / 1.9e-07 (the reference against itself: 5.7e-05 / 3.8e-04)
    "dw2":   (5.9e-04, 5.9e-04),            # 1.5e-04 / 1.5e-04 (the reference against itself: 2.6e-04 / 2.6e-04)
    "db2":   (4.0e-07, 4.0e-07),            # 0.0e+00 / 0.0e+00 (the reference against itself: 0.0e+00 / 0.0e+00)
    "d0":    (1.4e-03, 2.2e-02),            # 3.4e-04 / 5.4e-03 (the reference against itself: 3.3e-04 / 1.9e-03)
    "du":    (9.2e-07, 6.8e-06, 4.8e-06),   # 2.3e-07 / 7.6e-07 / 3.7e-07 (the reference against itself: 2.8e-07 / 6.4e-06 / 4.5e-06)
    "dp":    (9.2e-07, 7.9e-06, 5.6e-06),   # 2.3e-07 / 7.4e-07 / 3.7e-07 (the reference against itself: 3.3e-07 / 7.5e-06 / 5.3e-06)
    "dG":    (7.4e-04, 1.7e-02, 1.2e-02),   # 1.8e-04 / 4.2e-03 / 3.0e-03 (the reference against itself: 1.9e-04 / 4.2e-03 / 3.0e-03)
}
FB_LONG = {
    "p":     (5.4e-04, 5.8e-03, 7.6e-04),   # 1.3e-04 / 1.4e-03 / 1.9e-04 (the reference against itself: 9.5e-06 / 1.8e-04 / 1.3e-05)
    "hc":    (1.5e-04, 1.7e-03, 2.1e-04),   # 3.6e-05 / 4.2e-04 / 5.0e-05 (the reference against itself: 2.8e-06 / 4.9e-05 / 4.0e-06)
    "u":     (4.8e-04, 7.4e-03, 6.8e-04),   # 1.2e-04 / 1.8e-03 / 1.7e-04 (the reference against itself: 1.3e-05 / 2.9e-04 / 1.9e-05)
    "dgxc":  (4.4e-03, 9.6e-02, 6.3e-03),   # 1.1e-03 / 2.4e-02 / 1.6e-03 (the reference against itself: 7.0e-05 / 5.1e-04 / 9.0e-05)
    "dW_hh": (5.1e-03, 3.2e-02),            # 1.3e-03 / 7.9e-03 (the reference against itself: 2.6e-04 / 1.4e-03)
    "dw_p":  (3.0e-03, 2.2e-02),            # 7.5e-04 / 5.3e-03 (the reference against itself: 3.3e-04 / 2.9e-03)
    "dW1":   (4.8e-03, 2.3e-02),            # 1.2e-03 / 5.7e-03 (the reference against itself: 1.8e-05 / 6.1e-05)
    "db1":   (5.1e-03, 2.5e-02),            # 1.3e-03 / 6.2e-03 (the reference against itself: 1.4e-05 / 6.2e-05)
    "dw2":   (1.8e-03, 1.8e-03),            # 4.4e-04 / 4.4e-04 (the reference against itself: 9.4e-05 / 9.4e-05)
    "db2":   (4.3e-03, 4.3e-03),            # 1.1e-03 / 1.1e-03 (the reference against itself: 0.0e+00 / 0.0e+00)
    "d0":    (1.6e-03, 2.2e-03),            # 3.8e-04 / 5.3e-04 (the reference against itself: 4.0e-04 / 4.9e-04)
}
FB_SCALE = {"short": 9.3e-05, "wide": 5.0e-04, "long": 5.0e-04}
# least-squares scale of dW_hh, dw_p, dW1, dw2: measured short 2.3e-05 (floor 1.7e-09), wide 1.2e-04 (floor 4.8e-05), long 1.2e-04 (floor 5.4e-05)

# which plain bound each group is held to in test_gpu_lstm_stack.py / test_gpu_edlstm.py
PLAIN_OF = {"out": "out", "p": "out", "hc": "out", "u": "out", "dW1": "relu", "db1": "relu", "du": "relu"}


def tier(c):
    return "long" if c["T"] > 13 else "short" if c["H"] <= 64 else "wide"


def bounds(kind, c):
    t = tier(c)
    if kind == "stack":
        return {"short": STACK_SHORT, "wide": STACK_WIDE, "long": STACK_LONG}[t], STACK_SCALE[t]
    return {"short": FB_SHORT, "wide": FB_WIDE, "long": FB_LONG}[t], FB_SCALE[t]


# ------------------------------------------------------------------------------------------------ dispatch (csrc/api.hip, the plan headers)
def stack_plan(c):
    """(HPAD, NR, L) of scan_stack_plan.h for a case"""
    hp16 = -(-c["H"] // 16) * 16
    return (64 if hp16 <= 64 else 128, 2 if c["B"] > 256 else 1, c["L"])


def fb_plan(c):
    """(HPAD, NR, ES, KE) of scan_fb_plan.h for a case"""
    hp16 = -(-c["H"] // 16) * 16
    nw, tiles = hp16 // 16, -(-c["E"] // 16)
    per_wave, es = -(-tiles // nw), 1
    while es < per_wave:
        es *= 2
    return (64 if hp16 <= 64 else 128, 2 if c["B"] > 256 else 1, es, -(-c["E"] // 32))


_KNAME = re.compile(r"(lstm_stack_fwd_kernel|lstm_stack_bwd_kernel|lstm_fb_scan_fwd_kernel|lstm_fb_scan_bwd_kernel)(?:<([^>]*)>)?")


def ran(names):
    """{kernel name: template arguments as a tuple of ints, or None where the name does not show them} of the scan kernels"""
    out = {}
    for n in names:
        m = _KNAME.search(n)
        if m:
            args = None
            if m.group(2):
                try:
                    args = tuple(int(a.strip().rstrip("uUlL")) for a in m.group(2).split(","))
                except ValueError:
                    args = None
            assert out.setdefault(m.group(1), args) == args, names
    return out


def expected_instances(kind, c):
    """{kernel name: template arguments} api.hip launches for the case (MMT_STACK_PF = 2, MMT_FB_PF = 4)"""
    if kind == "stack":
        hpad, nr, L = stack_plan(c)
        return {"lstm_stack_fwd_kernel": (hpad // 32, 4 * hpad, 2, nr, L), "lstm_stack_bwd_kernel": (hpad // 8, 4 * hpad, nr, L)}
    hpad, nr, es, ke = fb_plan(c)
    return {"lstm_fb_scan_fwd_kernel": (hpad // 32, 4 * hpad, 4, nr, es), "lstm_fb_scan_bwd_kernel": (hpad // 8, ke, 4 * hpad, nr)}


def check_ran(tag, names, want):
    if names is None:
        print("%s: the profiler reports no device activity; instance not asserted" % tag)
        return                              # only this assertion is skipped
    got = ran(names)
    for k, args in want.items():
        assert k in got, "%s: %s did not run (%s)" % (tag, k, names)
        print("%s: ran %s<%s>" % (tag, k, got[k]))
        assert got[k] is None or got[k] == args, "%s: ran %s<%s>, labelled <%s>" % (tag, k, got[k], args)
    assert set(got) == set(want), "%s: ran %s" % (tag, sorted(got))


# ------------------------------------------------------------------------------------------------ cases
def _sc(T, B, H, L, init=True, wgrad=True, gs=1.0):
    cid = "s_T%d_B%d_H%d_L%d_%s%s%s" % (T, B, H, L, "i" if init else "n", "" if wgrad else "_nowgrad", "_x%g" % gs if gs != 1.0 else "")
    return {"id": cid, "T": T, "B": B, "H": H, "L": L, "init": init, "wgrad": wgrad, "gs": gs}


STACK_CASES = [
    # one sequence per workgroup, HPAD = 64: H = 4 (12 of 16 units padding), 40 (ragged tile), 64 (the last of HPAD 64)
    _sc(13, 3, 40, 2), _sc(13, 3, 40, 3), _sc(2, 1, 4, 4, init=False), _sc(3, 256, 64, 2), _sc(1, 3, 64, 3, init=False), _sc(13, 1, 64, 4),
    # HPAD = 128: H = 68 (five waves, HP16 = 80, 48 zero k-columns per half), 100, 128
    _sc(13, 3, 68, 2), _sc(3, 1, 100, 3, init=False), _sc(13, 3, 128, 4), _sc(2, 256, 128, 2, init=False), _sc(1, 3, 68, 4),
    # two sequences per workgroup: 257 (the last workgroup half empty), 512 (the limit)
    _sc(2, 257, 40, 2), _sc(3, 512, 4, 3, init=False), _sc(1, 257, 64, 4),
    _sc(3, 257, 68, 2, init=False), _sc(2, 512, 128, 3), _sc(1, 257, 100, 4), _sc(3, 257, 128, 4),
    # P and bias without a gradient (the batched branch is skipped); saturated gates (gx0 x 6)
    _sc(13, 3, 40, 3, wgrad=False), _sc(13, 3, 40, 2, gs=6.0), _sc(13, 3, 128, 3, gs=6.0),
    # long
    _sc(300, 2, 128, 4), _sc(300, 2, 40, 3),
]


def _fc(T, B, H, Ew, init=True, wp0=False, w2pos=False):
    cid = "f_T%d_B%d_H%d_E%d_%s%s%s" % (T, B, H, Ew, "i" if init else "n", "_wp0" if wp0 else "", "_w2pos" if w2pos else "")
    return {"id": cid, "T": T, "B": B, "H": H, "E": Ew, "init": init, "wp0": wp0, "w2pos": w2pos}


FB_CASES = [
    # one sequence per workgroup, HPAD = 64.  (H, E) -> read-out tiles per wave ES: (40, 24) 1, (64, 64) 1, (40, 68) 2, (64, 100) 2,
    # (4, 48) 4 with one empty tile, (4, 128) 8; backward k-blocks KE = ceil(E / 32)
    _fc(13, 3, 40, 24), _fc(13, 3, 64, 64, init=False), _fc(13, 1, 40, 68), _fc(2, 3, 4, 48), _fc(3, 1, 4, 128, init=False),
    _fc(5, 3, 64, 100), _fc(1, 256, 40, 4), _fc(13, 3, 4, 40),
    # HPAD = 128: E = 4 at H = 128 (seven of eight waves hold no live read-out row); (68, 96) and (100, 128) ES 2
    _fc(13, 3, 128, 4), _fc(13, 3, 128, 64, init=False), _fc(5, 1, 68, 96), _fc(2, 3, 100, 128), _fc(13, 2, 128, 128), _fc(3, 256, 68, 40),
    # two sequences per workgroup
    _fc(2, 257, 40, 24), _fc(3, 512, 64, 40, init=False), _fc(1, 257, 40, 96), _fc(2, 257, 4, 128), _fc(3, 257, 4, 48),
    _fc(2, 257, 128, 4), _fc(3, 512, 68, 64), _fc(1, 257, 100, 68, init=False), _fc(3, 257, 68, 128),
    # w_p = 0; w2 of one sign (every u > 0 contributes to p: the fixed-order sum cannot cancel an error)
    _fc(13, 3, 40, 24, wp0=True), _fc(13, 3, 64, 64, w2pos=True), _fc(13, 3, 128, 128, w2pos=True),
    # long
    _fc(300, 2, 128, 64), _fc(300, 2, 40, 24),
]
# the backward alone through the C entry point, with the reference's saved tensors handed in
FB_BWD_CASES = [_fc(13, 2, 64, 40), _fc(13, 3, 128, 128), _fc(3, 257, 40, 24), _fc(2, 257, 100, 68)]


def stack_inputs(c):
    """the inputs of test_gpu_lstm_stack._scan_inputs (fan-in scaling 1 / sqrt(2H)), from recipe.gen_normal"""
    g = lambda n, shape: R.gen_normal("bfstack:%s:%s" % (c["id"], n), shape, 29).double()      # noqa: E731
    T, B, H, L = c["T"], c["B"], c["H"], c["L"]
    inp = dict(gx0=c["gs"] * g("gx0", (T, B, 4 * H)), P=g("P", (L, 4 * H, 2 * H)) / np.sqrt(2 * H), bias=0.1 * g("bias", (L - 1, 4 * H)),
               h0=0.5 * g("h0", (L, B, H)) if c["init"] else None, c0=0.5 * g("c0", (L, B, H)) if c["init"] else None)
    return inp, g("w", (T, B, H))


FB_KEYS = ("gxc", "w_p", "W_hh", "W1", "b1", "w2", "b2", "h0", "c0")


def fb_inputs(c):
    """the inputs of test_gpu_edlstm._scan_inputs (w_p multiplies one input of the 1 + H the decoder LSTM reads), from recipe.gen_normal"""
    g = lambda n, shape: R.gen_normal("bffb:%s:%s" % (c["id"], n), shape, 29).double()      # noqa: E731
    T, B, H, Ew = c["T"], c["B"], c["H"], c["E"]
    inp = dict(gxc=g("gxc", (T, B, 4 * H)), w_p=g("w_p", (4 * H,)) / np.sqrt(1 + H), W_hh=g("W_hh", (4 * H, H)) / np.sqrt(H),
               W1=g("W1", (Ew, H)) / np.sqrt(H), b1=0.1 * g("b1", (Ew,)), w2=g("w2", (Ew,)) / np.sqrt(Ew), b2=0.1 * g("b2", (1,)),
               h0=0.5 * g("h0", (B, H)) if c["init"] else None, c0=0.5 * g("c0", (B, H)) if c["init"] else None)
    if c["wp0"]:
        inp["w_p"] = torch.zeros(4 * H, dtype=torch.float64)
    if c["w2pos"]:
        inp["w2"] = inp["w2"].abs()
    return inp, g("w", (T, B))


# ------------------------------------------------------------------------------------------------ the reference (CPU, fp64)
def _leaves(inp, frozen=()):
    return {k: None if v is None else (v.clone() if k in frozen else v.clone().requires_grad_()) for k, v in inp.items()}


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def stack_ref(c, inputs=None, **kw):
    """h_top, h_all, c_all and the gradients of case c from bf16_ref.lstm_stack_scan (kw: rounding, mutate), as numpy arrays"""
    inp, w = inputs or stack_inputs(c)
    lv = _leaves(inp, () if c["wgrad"] else ("P", "bias"))
    if callable(kw.get("mutate")):
        kw["mutate"] = kw["mutate"](lv)                 # hooks that need the leaves
    h_top, h_all, c_all = E.lstm_stack_scan(lv["gx0"], lv["P"], lv["bias"], lv["h0"], lv["c0"], **kw)
    (h_top * w).sum().backward()
    out = {"h_top": _np(h_top), "h_all": _np(h_all), "c_all": _np(c_all)}
    out.update({"d" + k: _np(t.grad) for k, t in lv.items() if t is not None and t.requires_grad})
    return out


def fb_ref(c, inputs=None, saved=None, **kw):
    """p_all, h_all, c_all, u_all and the nine gradients of case c from bf16_ref.lstm_fb_scan, as numpy arrays"""
    inp, w = inputs or fb_inputs(c)
    lv = _leaves(inp)
    if callable(kw.get("mutate")):
        kw["mutate"] = kw["mutate"](lv)
    p, h, cc, u = E.lstm_fb_scan(*[lv[k] for k in FB_KEYS], p_init=P_INIT, saved=saved, **kw)
    (p * w).sum().backward()
    out = {"p_all": _np(p), "h_all": _np(h), "c_all": _np(cc), "u_all": _np(u)}
    out.update({"d" + k: _np(t.grad) for k, t in lv.items() if t is not None})
    return out


# ------------------------------------------------------------------------------------------------ what is measured
def views(kind, d):
    """[(name, group, array, what)] of a result dict: what = "tb" (a (T, B, ...) tensor: rows (t, b), per-sequence maximum), "row"
    (rows as shaped), "w" (a weight gradient: rows = output features, least-squares scale)."""
    v = []
    if kind == "stack":
        L, T, B, H = d["h_all"].shape
        v.append(("h_top", "out", d["h_top"], "tb"))
        for n in ("h_all", "c_all"):
            v.append((n, "out", d[n].transpose(1, 2, 0, 3), "tb"))             # (T, B, L, H): a row is one (t, b, l)
        v.append(("dgx0", "dgx0", d["dgx0"], "tb"))
        if "dP" in d:
            for l in range(L):
                v.append(("dP%d.xa" % l, "dP", d["dP"][l][:, :H], "w"))
                v.append(("dP%d.xb" % l, "dP", d["dP"][l][:, H:], "w"))
            v.append(("dbias", "dbias", d["dbias"].reshape(-1), "row"))
        for n in ("dh0", "dc0"):
            if n in d:
                v.append((n, "d0", d[n].transpose(1, 0, 2).reshape(B, L * H), "row"))     # a row is one sequence
    elif kind == "fb":
        v.append(("p_all", "p", d["p_all"][..., None], "tb"))
        v += [("h_all", "hc", d["h_all"], "tb"), ("c_all", "hc", d["c_all"], "tb"), ("u_all", "u", d["u_all"], "tb"),
              ("dgxc", "dgxc", d["dgxc"], "tb"), ("dW_hh", "dW_hh", d["dW_hh"], "w"), ("dw_p", "dw_p", d["dw_p"].reshape(-1, 1), "w"),
              ("dW1", "dW1", d["dW1"], "w"), ("db1", "db1", d["db1"].reshape(-1), "row"), ("dw2", "dw2", d["dw2"].reshape(1, -1), "w"),
              ("db2", "db2", d["db2"].reshape(-1), "row")]
        for n in ("dh0", "dc0"):
            if n in d:
                v.append((n, "d0", d[n], "row"))
    else:                                                                       # "fb_bwd": the C entry point's own buffers
        v += [("du", "du", d["du"], "tb"), ("dp", "dp", d["dp"][..., None], "tb"), ("dG", "dG", d["dG"], "tb")]
    return v


def figures(kind, got, ref):
    """[(name, group, measure, value)] with measure in rel / row / seq / scale: every figure compare() bounds, for the CPU tests"""
    out = []
    for (name, group, g, what), (_, _, r, _) in zip(views(kind, got), views(kind, ref)):
        if not r.any():                                 # an analytically zero tensor (dP_0's x_a half at T = 1): compare() wants exact zeros
            continue
        rel, row = measures(g, r)
        out += [(name, group, "rel", rel), (name, group, "row", row)]
        if what == "tb":
            out.append((name, group, "seq", seq_max(g, r)))
        if what == "w":
            out.append((name, group, "scale", abs(ls_scale(g, r))))
    return out


def bound_of(kind, c, group, measure):
    """the bound compare() applies to a figure (None: not bounded)"""
    bd, scale = bounds("fb" if kind == "fb_bwd" else kind, c)
    return scale if measure == "scale" else bd[group][("rel", "row", "seq").index(measure)]


def compare(kind, tag, c, got, ref, failures):
    bd, scale = bounds("fb" if kind == "fb_bwd" else kind, c)
    gv, rv = views(kind, got), views(kind, ref)
    assert [x[0] for x in gv] == [x[0] for x in rv], (tag, [x[0] for x in gv], [x[0] for x in rv])
    for (name, group, g, what), (_, _, r, _) in zip(gv, rv):
        assert g.shape == r.shape, (tag, name, g.shape, r.shape)
        if not r.any():                                 # dP_0's x_a half at T = 1: the zeros tile times dG, exactly zero
            print("%-52s zero in the reference" % ("%s %s" % (tag, name)))
            if g.any():
                failures.append("%s %s: not zero where the reference is (max %.3e)" % (tag, name, np.abs(g).max()))
            continue
        check_scan("%s %s" % (tag, name), g, r, bd[group], failures, seq=(what == "tb"), scale=scale if what == "w" else None)


# ------------------------------------------------------------------------------------------------ GPU runs
def _dev_leaves(inp, dev, frozen=()):
    out = {}
    for k, v in inp.items():
        out[k] = None if v is None else v.float().to(dev)
        if v is not None and k not in frozen:
            out[k].requires_grad_()
    return out


def run_stack(c, dev):
    from multimodal_transformer_amd import functional as F
    inp, w = stack_inputs(c)
    lv = _dev_leaves(inp, dev, () if c["wgrad"] else ("P", "bias"))
    wd = w.float().to(dev)

    def step():
        h_top, h_all, c_all = F.lstm_stack_scan(lv["gx0"], lv["P"], lv["bias"], lv["h0"], lv["c0"], return_states=True)
        h_top.backward(wd)
        return h_top, h_all, c_all
    (h_top, h_all, c_all), names = device_kernel_names(step)
    out = {"h_top": _np(h_top), "h_all": _np(h_all), "c_all": _np(c_all)}
    out.update({"d" + k: _np(t.grad) for k, t in lv.items() if t is not None and t.requires_grad})
    return out, names


def run_fb(c, dev):
    from multimodal_transformer_amd import functional as F
    inp, w = fb_inputs(c)
    lv = _dev_leaves(inp, dev)
    wd = w.float().to(dev)

    def step():
        outs = F.lstm_fb_scan(*[lv[k] for k in FB_KEYS], p_init=P_INIT, return_states=True)
        outs[0].backward(wd)
        return outs
    (p, h, cc, u), names = device_kernel_names(step)
    out = {"p_all": _np(p), "h_all": _np(h), "c_all": _np(cc), "u_all": _np(u)}
    out.update({"d" + k: _np(t.grad).reshape(inp[k].shape) for k, t in lv.items() if t is not None})
    return out, names


def _finish(failures):
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", STACK_CASES, ids=[c["id"] for c in STACK_CASES])
def test_stack_scan(dev, c):
    tag = "bf stack %s %s" % (tier(c), c["id"])
    got, names = run_stack(c, dev)
    check_ran(tag, names, expected_instances("stack", c))
    if not c["wgrad"]:
        assert "dP" not in got and "dbias" not in got
    failures = []
    compare("stack", tag, c, got, stack_ref(c), failures)
    _finish(failures)


@pytest.mark.parametrize("c", FB_CASES, ids=[c["id"] for c in FB_CASES])
def test_fb_scan(dev, c):
    tag = "bf fb %s %s" % (tier(c), c["id"])
    got, names = run_fb(c, dev)
    check_ran(tag, names, expected_instances("fb", c))
    failures = []
    compare("fb", tag, c, got, fb_ref(c), failures)
    _finish(failures)


@pytest.mark.parametrize("c", FB_BWD_CASES, ids=[c["id"] for c in FB_BWD_CASES])
def test_fb_scan_backward_buffers(dev, c):
    """du (T, B, E), dp (T, B) and dG are not autograd outputs; here they are read from the C entry point's own buffers, the backward
    given the REFERENCE's saved tensors (c_all, acts, u_all), so du's ReLU mask is the reference's and the comparison sees the backward
    kernel alone."""
    from multimodal_transformer_amd import _lib
    tag = "bf fb bwd %s %s" % (tier(c), c["id"])
    inp, w = fb_inputs(c)
    saved = {}
    ref = fb_ref(c, saved=saved)
    want = {k: _np(v) for k, v in saved["grads"]().items()}
    T, B, H, Ew = c["T"], c["B"], c["H"], c["E"]
    t = lambda a: torch.as_tensor(a).float().contiguous().to(dev)              # noqa: E731
    z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)           # noqa: E731
    nbytes = _lib.load().mmt_lstm_fb_scan_workspace_bytes(H, Ew)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dG, du, dp, dh0, dc0 = z(T, B, 4 * H), z(T, B, Ew), z(T, B), z(B, H), z(B, H)
    args = (t(w), t(inp["w_p"]), t(inp["W_hh"]), t(inp["W1"]), t(inp["w2"]), t(inp["c0"]), t(ref["c_all"]), t(saved["acts"]), t(ref["u_all"]))

    def step():
        _lib.launch("mmt_lstm_fb_scan_backward", *args, dG, du, dp, dh0, dc0, ws, nbytes, T, B, H, Ew)
    _, names = device_kernel_names(step)
    inst = expected_instances("fb", c)
    check_ran(tag, names, {"lstm_fb_scan_bwd_kernel": inst["lstm_fb_scan_bwd_kernel"]})
    failures = []
    compare("fb_bwd", tag, c, {"du": _np(du), "dp": _np(dp), "dG": _np(dG)}, want, failures)
    bd, _ = bounds("fb", c)
    check_scan(tag + " dh0", _np(dh0), ref["dh0"], bd["d0"], failures)
    check_scan(tag + " dc0", _np(dc0), ref["dc0"], bd["d0"], failures)
    _finish(failures)


# ------------------------------------------------------------------------------------------------ the case lists and the bounds themselves
def test_every_instance_has_a_case():
    """every instance of the dispatch has a case, and the shape edges the kernels pad or split at are all there"""
    assert {stack_plan(c) for c in STACK_CASES} == {(hp, nr, L) for hp in (64, 128) for nr in (1, 2) for L in (2, 3, 4)}
    for inst in {stack_plan(c) for c in STACK_CASES}:
        assert any(c["T"] in (1, 2, 3, 13) for c in STACK_CASES if stack_plan(c) == inst), inst
    assert {c["H"] for c in STACK_CASES} >= {4, 40, 64, 68, 100, 128} and {c["B"] for c in STACK_CASES} >= {1, 3, 256, 257, 512}
    assert {c["T"] for c in STACK_CASES} >= {1, 2, 3, 13, 300}
    assert all(c["T"] <= 3 for c in STACK_CASES + FB_CASES + FB_BWD_CASES if c["B"] >= 256)
    fwd = {fb_plan(c)[:3] for c in FB_CASES}
    assert fwd == {(64, nr, es) for nr in (1, 2) for es in (1, 2, 4, 8)} | {(128, nr, es) for nr in (1, 2) for es in (1, 2)}, sorted(fwd)
    bwd = {(p[0], p[1], p[3]) for p in map(fb_plan, FB_CASES)}
    assert bwd == {(hp, nr, ke) for hp in (64, 128) for nr in (1, 2) for ke in (1, 2, 3, 4)}, sorted(bwd)
    assert {c["E"] for c in FB_CASES} >= {4, 24, 40, 64, 68, 96, 100, 128} and {c["B"] for c in FB_CASES} >= {1, 3, 256, 257, 512}
    assert any(c["H"] == 4 and c["E"] == 48 for c in FB_CASES) and any(c["H"] == 128 and c["E"] == 4 for c in FB_CASES)


def ratios():
    """{(kind, tier, group): the rel-L2 bound over the plain test's bound for the same tensor}"""
    out = {}
    for kind, tiers in (("stack", (STACK_SHORT, STACK_WIDE, STACK_LONG)), ("fb", (FB_SHORT, FB_WIDE, FB_LONG))):
        for tname, bd in zip(("short", "wide", "long"), tiers):
            for group, b in bd.items():
                out[kind, tname, group] = b[0] / PLAIN[PLAIN_OF.get(group, "grad")]
    return out


def test_bounds_are_tighter_than_the_plain_tests():
    for k, r in sorted(ratios().items()):
        print("%-6s %-6s %-6s bound / plain bound = %.3f" % (k + (r,)))
        assert r < 1, k
    for bd in (STACK_SHORT, FB_SHORT):                  # in the tier that holds T <= 13 and H <= 64 every tensor carries all of its measures
        assert all(x is not None for b in bd.values() for x in b)
