"""The batch MFN gate in training (functional._MfnGateFn / mfn_gate and MFN._gate) against the bf16-faithful fp64 reference
(tests/mfn_stream_ref.py gate_from_states / batch_composition: bf16_ref's pieces under autograd).

test_gpu_models.py holds the gate's gradients with one rel-L2 per tensor at 9e-2 against the unrounded oracle, at three modalities of
one width.  A term wrong by a few percent, a contribution missing in one modality's column block or one gamma half scaled wrongly
passes that.  Here the reference rounds where the kernels round, and every tensor is measured as test_gpu_bf16_scans.py measures:
rel-L2, the per-row maximum (a row is one (t, b) of out, d_hs, d_cs and dx, one output feature of a weight gradient, one entry of a bias
gradient), the per-sequence maximum of the (T, B, .) tensors and the least-squares scale of every weight matrix.  d_cs is measured per
modality block and again for t = 0, 0 < t < T - 1 and t = T - 1 alone, where a wrong one-step shift shows.

Two entries: F.mfn_gate(hs, cs, params) with hs, cs as leaves of their own (test_mfn_gate), and MFN._gate / MFN.forward of the module
with the LSTM cells in front (test_mfn_module).  Both in eval and in train mode (gamma dropout 0.2, out dropout 0.5, fixed seeds); the
masks are rebuilt with F.dropout_mask and handed to the reference as multipliers.  Every case asserts through torch.profiler which
mfn_mem_scan kernels ran and that no library kernel did.  No getenv switch of api.hip is read on these paths at H <= 88
(MMT_NO_CLUSTER_SCAN decides only at HPAD = 256), so everything runs in the pytest process.

Observed on the MI355X: 32 tests in 6 s.  With B = 1 and T <= 2 nothing tips and the kernels sit at fp32 level (at most 1.3e-7; the
bias gradients are bit-equal to the reference); beyond that the distance is a few tipped bf16 roundings, 1e-4 .. 6e-4 rel-L2 on the
gradients, the size of the reference's own movement under fp32-level noise.

Value-only mutants of the host composition and the glue, each applied to a scratch copy and run once against this file and against
test_gpu_models.py's test_mfn_gate_train_mode_mask_replay and test_mfn_gate_golden (addresses, row counts, leading dimensions and
destination sizes unchanged).  The worst tensor of this file's failures (measured against its bound); "old pass": both old tests pass.
  * d_att2 copied over d_att instead of added (acc=True dropped): all 32 fail; d_cs 4.95e-2 rel-L2 at t = T - 1 against 1.3e-3 (T = 40),
    8.3e-2 per sequence against 2.9e-3 (B = 257), att1_fc1.bias 4.9e-2 against 2.2e-3.  Old pass.
  * the prev part's contribution to d_cs dropped for the LAST modality only: 24 fail; d_cs of that modality 0.85 at t = 0,
    0.70 .. 0.81 at 0 < t < T - 1, nothing at t = T - 1, against 6.9e-4 / 1.3e-3.  The 8 that pass: T = 1, the masked module runs
    at (T, B) = (2, 1), whose one sequence has one window, and the module's eval run at T = 40, which sees d_cs only through the
    LSTM backward: the direct d_cs of test_mfn_gate is what holds the shift.  Old pass.
  * the prev part of block 0 read at the new part's src_off (one block width further, inside d cStar): 25 fail (all with a second
    unmasked step); d_cs of modality 0 1.3 at t = 0 and at 0 < t < T - 1, 3.2 per sequence (B = 257); through the module dx 2.1e-2
    and the cell's biases 2.6e-2 at T = 2.  Old pass.
  * gamma1's and gamma2's halves of db1 swapped: all 32 fail; gamma2_fc1.bias 1.44 against 7.8e-4 (T = 40), gamma1_fc1.bias 42 where
    the bound is 0 (T = 2: gamma1's own gradient has one term).  Old pass (the two tensors are small against the old absolute floor).
  * v left out of the dot product of softmax_mul_bwd_kernel: all 32 fail; att1_fc2's gradients 0.69, att1_fc1's 0.60 .. 0.76, d_cs
    5.0e-2 at 0 < t < T - 1 and 0.15 per sequence.  Old pass.
  * one of the two dW2 halves (gamma1_fc2.weight) times 1.01: 25 fail (all but T = 1 and the masked module runs at (2, 1), where
    that gradient is zero); rel-L2 1.00e-2 against 4.4e-4 / 5.9e-4, and the least-squares scale 1.0e-2 against 3.6e-5 / 1.3e-4.
    Old pass.
  * add2 writes bias_ih alone in the forward: 18 fail (every module test; F.mfn_gate has no cell); dx 1.06 .. 1.44 per sequence, the
    gamma gradients 0.75 .. 0.92.  The old tests fail it too.
  * the backward's out-dropout seed off by one: CHANGES NOTHING, here or anywhere: every printed figure of that run equals the clean
    run's.  The backward does not regenerate the out-dropout mask: linear_backward_impl (csrc/api.hip) hands grad_prep_kernel the
    scale 1 / (1 - p) only, and the mask is the zeros of the saved fp32 output hid, whose ReLU derivative they switch off; the seed
    reaches the INPUT dropout's stream alone, which the gate does not use.  No measure can see an equivalent mutant.  In its place,
    the forward's out-dropout seed off by one (another mask than the one this file rebuilds from stream 2001): the 18 train-mode
    tests fail, out 6.5e-2 .. 1.05 against 1.8e-7, d_hs 2.1; the old mask-replay test fails it too, the golden test (eval) passes.
"""
import numpy as np
import pytest
import torch

import mfn_stream_ref as S
import recipe as R
import test_gpu_bf16_scans as SC
from conftest import rel_l2
from gpu_harness import check, check_scan, dev, device_kernel_names, library_kernels, load_named, mta  # noqa: F401

pytestmark = pytest.mark.gpu

PG, PO = 0.2, 0.5                      # the reference's gamma and out dropout (transformer/MFT/multiTransformer.py:168,172,176)
GATE_NAMES = [l + s for l in ("att1_fc1", "att1_fc2", "att2_fc1", "att2_fc2", "gamma1_fc1", "gamma1_fc2", "gamma2_fc1", "gamma2_fc2",
                              "out_fc1", "out_fc2") for s in (".weight", ".bias")]       # the order of _MfnGateFn.NP


def _case(mods, widths, T, B):
    return {"id": "%s_T%d_B%d" % ("+".join(m[:3] for m in mods), T, B), "mods": mods, "widths": widths, "T": T, "B": B}


# the smallest shapes that reach every branch of the composition
CASES = [_case(["emotient"], [8], 1, 1),                       # A = 32 < 64 lanes of a softmax row; M - B = 0 rows in the shifted segments
         _case(["emotient"], [8], 2, 1),                       # the first step whose prev part is not zero
         _case(["acoustic", "emotient"], [12, 16], 3, 5),      # width 12 padded in K; two column blocks
         _case(["linguistic", "acoustic", "image"], [40, 24, 32], 7, 33),       # sum H = 224, block offsets 88 and 136, 33 scan workgroups
         _case(["linguistic", "emotient", "acoustic", "image"], [256, 16, 256, 256], 5, 3),      # sum H = 240, A = 480, the reference widths
         _case(["acoustic", "emotient"], [16, 16], 2, 257),    # two sequences per scan workgroup; B no multiple of 4 in the B A + col offset
         _case(R.MODS_AVL, [256, 256, 256], 40, 3)]            # a longer recurrence; test_gpu_models runs (20, 3)
IDS = [c["id"] for c in CASES]
MODES = ("eval", "train")

STATE_KEYS = ["out", "d_hs", "d_cs", "dx"]                             # (rel-L2, per row, per sequence)
VECTOR_KEYS = ["d_cs_t", "lstm.bias"] + [n for n in GATE_NAMES if n.endswith(".bias")]           # (rel-L2, per row)
MATRIX_KEYS = ["lstm.weight_ih", "lstm.weight_hh"] + [n for n in GATE_NAMES if n.endswith(".weight")]      # (rel-L2, per row, scale)
# Bounds, per tier (tier() below) and per tensor: (rel-L2, per-row maximum, third), third the per-sequence maximum of the per-window tensors
# and the least-squares scale of a weight matrix.  d_hs, d_cs and dx stand for every modality's, lstm.* for every cell's; d_cs_t holds
# d_cs of one modality at t = 0, at 0 < t < T - 1 and at t = T - 1 alone.  Each bound is at most 4x the worst value measured on the
# MI355X over the tier's cases, both modes and both entries (in the comment, in the same order), rounded down to two digits; none is
# below the floor (tests/test_mfn_gate_cpu.py test_mfn_gate_jitter_floor: what noise of half an fp32 ulp on every COMPUTED value in
# front of its bf16 rounding does to the reference itself, behind "floor"), none above test_gpu_models' 2e-2 (out) / 9e-2 (gradients).
# Every tensor of every tier keeps its per-row bound; in the exact and short tiers (T <= 7) every gradient bound is at most 9e-3, a
# tenth of test_gpu_models' 9e-2: four per-row bounds that 4x the measurement would put at 1.0e-2 .. 1.6e-2 are held at 9e-3, above
# their floors.  A bound of 0.0: exact arithmetic (the bias gradients of the exact tier are sums of at most two bf16 values, gamma1's
# and W_hh's gradients there have one nonzero term; out_fc2.bias is the sum of the given g), measured 0.
BOUNDS = {
    "exact": {
        "out":                 (1.8e-07, 2.6e-07, 3.4e-07),     # 4.61e-08 / 6.52e-08 / 8.61e-08; floor 0 / 0 / 0
        "d_hs":                (1.1e-07, 1.6e-07, 1.1e-07),     # 3.00e-08 / 4.24e-08 / 3.00e-08; floor 0 / 0 / 0
        "d_cs":                (4.9e-07, 5.1e-07, 4.9e-07),     # 1.23e-07 / 1.28e-07 / 1.23e-07; floor 0 / 0 / 0
        "dx":                  (1.7e-07, 2.4e-07, 1.7e-07),     # 4.30e-08 / 6.08e-08 / 4.30e-08; floor 0 / 0 / 0
        "d_cs_t":              (4.9e-07, 4.9e-07),              # 1.23e-07 / 1.23e-07; floor 0 / 0
        "lstm.bias":           (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "att1_fc1.bias":       (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "att1_fc2.bias":       (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "att2_fc1.bias":       (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "att2_fc2.bias":       (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "gamma1_fc1.bias":     (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "gamma1_fc2.bias":     (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "gamma2_fc1.bias":     (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "gamma2_fc2.bias":     (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "out_fc1.bias":        (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "out_fc2.bias":        (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "lstm.weight_ih":      (3.5e-08, 1.9e-07, 2.4e-09),     # 8.78e-09 / 4.84e-08 / 6.15e-10; floor 0 / 0 / 0
        "lstm.weight_hh":      (0.0, 0.0, 0.0),                 # 0 / 0 / 0; floor 0 / 0 / 0
        "att1_fc1.weight":     (1.8e-08, 2.1e-07, 1.3e-09),     # 4.68e-09 / 5.30e-08 / 3.31e-10; floor 0 / 0 / 0
        "att1_fc2.weight":     (4.9e-08, 1.7e-07, 8.7e-10),     # 1.24e-08 / 4.43e-08 / 2.18e-10; floor 0 / 0 / 0
        "att2_fc1.weight":     (4.4e-08, 4.3e-07, 1.5e-09),     # 1.12e-08 / 1.09e-07 / 3.77e-10; floor 0 / 0 / 0
        "att2_fc2.weight":     (3.3e-08, 2.7e-07, 2.4e-10),     # 8.33e-09 / 6.89e-08 / 6.09e-11; floor 0 / 0 / 0
        "gamma1_fc1.weight":   (0.0, 0.0, 0.0),                 # 0 / 0 / 0; floor 0 / 0 / 0
        "gamma1_fc2.weight":   (0.0, 0.0, 0.0),                 # 0 / 0 / 0; floor 0 / 0 / 0
        "gamma2_fc1.weight":   (5.0e-08, 2.6e-07, 2.0e-09),     # 1.26e-08 / 6.58e-08 / 5.04e-10; floor 0 / 0 / 0
        "gamma2_fc2.weight":   (3.0e-08, 2.0e-07, 8.3e-10),     # 7.67e-09 / 5.10e-08 / 2.09e-10; floor 0 / 0 / 0
        "out_fc1.weight":      (1.3e-08, 1.0e-07, 7.4e-10),     # 3.26e-09 / 2.60e-08 / 1.86e-10; floor 0 / 0 / 0
        "out_fc2.weight":      (0.0, 0.0, 0.0),                 # 0 / 0 / 0; floor 0 / 0 / 0
    },
    "short": {
        "out":                 (2.7e-04, 6.1e-03, 4.3e-03),     # 6.88e-05 / 1.53e-03 / 1.08e-03; floor 5.43e-05 / 1.23e-03 / 8.69e-04
        "d_hs":                (1.5e-07, 5.4e-07, 3.9e-07),     # 3.76e-08 / 1.36e-07 / 9.88e-08; floor 0 / 0 / 0
        "d_cs":                (4.2e-04, 3.5e-03, 2.9e-03),     # 1.06e-04 / 8.78e-04 / 7.46e-04; floor 1.34e-04 / 2.04e-03 / 1.97e-03
        "dx":                  (3.7e-04, 2.3e-03, 1.6e-03),     # 9.29e-05 / 5.92e-04 / 4.19e-04; floor 6.60e-06 / 1.31e-04 / 9.26e-05
        "d_cs_t":              (6.9e-04, 3.8e-03),              # 1.73e-04 / 9.59e-04; floor 1.73e-04 / 2.68e-03
        "lstm.bias":           (2.5e-04, 3.5e-03),              # 6.50e-05 / 8.93e-04; floor 9.54e-06 / 1.32e-04
        "att1_fc1.bias":       (1.9e-03, 9.0e-03),              # 4.82e-04 / 2.60e-03; floor 3.82e-04 / 2.93e-03; held at 9e-3: x 3.5
        "att1_fc2.bias":       (1.4e-03, 9.0e-03),              # 3.70e-04 / 4.19e-03; floor 2.50e-04 / 2.19e-03; held at 9e-3: x 2.1
        "att2_fc1.bias":       (2.8e-04, 3.5e-03),              # 7.19e-05 / 8.77e-04; floor 9.89e-05 / 7.27e-04
        "att2_fc2.bias":       (7.2e-05, 7.9e-04),              # 1.81e-05 / 1.99e-04; floor 4.05e-05 / 4.10e-04
        "gamma1_fc1.bias":     (9.1e-04, 7.1e-03),              # 2.29e-04 / 1.79e-03; floor 5.79e-05 / 4.62e-04
        "gamma1_fc2.bias":     (2.7e-04, 3.1e-03),              # 6.94e-05 / 7.85e-04; floor 3.00e-05 / 3.39e-04
        "gamma2_fc1.bias":     (7.1e-04, 4.7e-03),              # 1.78e-04 / 1.20e-03; floor 5.48e-05 / 3.08e-04
        "gamma2_fc2.bias":     (2.5e-04, 2.7e-03),              # 6.48e-05 / 6.86e-04; floor 4.65e-05 / 4.12e-04
        "out_fc1.bias":        (1.0e-07, 6.9e-07),              # 2.66e-08 / 1.74e-07; floor 0 / 0
        "out_fc2.bias":        (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "lstm.weight_ih":      (3.5e-04, 4.8e-03, 9.6e-06),     # 8.86e-05 / 1.22e-03 / 2.41e-06; floor 1.10e-05 / 1.52e-04 / 2.86e-07
        "lstm.weight_hh":      (1.6e-04, 1.8e-03, 3.7e-06),     # 4.12e-05 / 4.58e-04 / 9.41e-07; floor 0 / 0 / 0
        "att1_fc1.weight":     (1.6e-03, 9.0e-03, 3.1e-05),     # 4.14e-04 / 2.38e-03 / 7.98e-06; floor 2.90e-04 / 2.22e-03 / 1.67e-05; held at 9e-3: x 3.8
        "att1_fc2.weight":     (1.2e-03, 9.0e-03, 4.8e-05),     # 3.14e-04 / 3.55e-03 / 1.22e-05; floor 2.57e-04 / 1.66e-03 / 6.40e-06; held at 9e-3: x 2.5
        "att2_fc1.weight":     (4.8e-04, 3.5e-03, 7.8e-06),     # 1.20e-04 / 8.94e-04 / 1.97e-06; floor 1.24e-04 / 9.60e-04 / 7.73e-07
        "att2_fc2.weight":     (7.2e-05, 7.9e-04, 8.0e-06),     # 1.81e-05 / 1.99e-04 / 2.01e-06; floor 4.25e-05 / 4.14e-04 / 1.42e-06
        "gamma1_fc1.weight":   (9.7e-04, 7.2e-03, 2.4e-04),     # 2.45e-04 / 1.80e-03 / 6.04e-05; floor 8.61e-05 / 4.61e-04 / 1.71e-05
        "gamma1_fc2.weight":   (4.4e-04, 3.1e-03, 3.6e-05),     # 1.12e-04 / 7.85e-04 / 9.04e-06; floor 2.99e-05 / 3.39e-04 / 1.41e-06
        "gamma2_fc1.weight":   (1.0e-03, 5.0e-03, 1.8e-04),     # 2.52e-04 / 1.27e-03 / 4.60e-05; floor 7.25e-05 / 5.45e-04 / 3.27e-06
        "gamma2_fc2.weight":   (2.8e-04, 2.6e-03, 5.8e-05),     # 7.23e-05 / 6.61e-04 / 1.46e-05; floor 1.13e-04 / 4.06e-04 / 1.62e-05
        "out_fc1.weight":      (9.1e-05, 2.8e-04, 3.8e-06),     # 2.29e-05 / 7.11e-05 / 9.57e-07; floor 2.21e-06 / 6.10e-06 / 1.26e-08
        "out_fc2.weight":      (7.8e-04, 7.8e-04, 1.0e-04),     # 1.96e-04 / 1.96e-04 / 2.68e-05; floor 1.98e-05 / 1.98e-05 / 1.63e-06
    },
    "long": {
        "out":                 (3.2e-04, 2.7e-03, 4.4e-04),     # 8.21e-05 / 6.99e-04 / 1.11e-04; floor 0 / 0 / 0
        "d_hs":                (1.0e-07, 3.5e-07, 1.3e-07),     # 2.74e-08 / 8.92e-08 / 3.25e-08; floor 0 / 0 / 0
        "d_cs":                (1.3e-03, 1.0e-02, 2.3e-03),     # 3.36e-04 / 2.71e-03 / 5.81e-04; floor 2.78e-05 / 2.21e-04 / 4.82e-05
        "dx":                  (2.4e-03, 1.7e-02, 3.5e-03),     # 6.13e-04 / 4.31e-03 / 8.83e-04; floor 1.28e-05 / 1.34e-04 / 2.21e-05
        "d_cs_t":              (1.3e-03, 1.0e-02),              # 3.39e-04 / 2.66e-03; floor 2.82e-05 / 2.18e-04
        "lstm.bias":           (1.4e-03, 1.6e-02),              # 3.53e-04 / 4.04e-03; floor 7.28e-06 / 1.31e-04
        "att1_fc1.bias":       (2.2e-03, 6.9e-03),              # 5.73e-04 / 1.73e-03; floor 3.54e-04 / 1.00e-03
        "att1_fc2.bias":       (1.7e-03, 1.0e-02),              # 4.26e-04 / 2.57e-03; floor 2.76e-04 / 2.36e-03
        "att2_fc1.bias":       (8.1e-04, 7.2e-03),              # 2.03e-04 / 1.81e-03; floor 1.18e-04 / 9.26e-04
        "att2_fc2.bias":       (2.3e-04, 2.6e-03),              # 5.94e-05 / 6.72e-04; floor 4.86e-05 / 5.50e-04
        "gamma1_fc1.bias":     (1.1e-03, 5.2e-03),              # 2.98e-04 / 1.31e-03; floor 5.54e-05 / 3.26e-04
        "gamma1_fc2.bias":     (3.0e-04, 3.0e-03),              # 7.74e-05 / 7.55e-04; floor 1.68e-05 / 1.91e-04
        "gamma2_fc1.bias":     (7.8e-04, 6.0e-03),              # 1.96e-04 / 1.51e-03; floor 3.68e-07 / 2.94e-06
        "gamma2_fc2.bias":     (1.5e-04, 1.0e-03),              # 3.84e-05 / 2.63e-04; floor 2.90e-06 / 3.28e-05
        "out_fc1.bias":        (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "out_fc2.bias":        (0.0, 0.0),                      # 0 / 0; floor 0 / 0
        "lstm.weight_ih":      (2.4e-03, 2.8e-02, 8.8e-05),     # 6.04e-04 / 7.12e-03 / 2.22e-05; floor 1.20e-05 / 2.15e-04 / 5.34e-08
        "lstm.weight_hh":      (1.9e-03, 2.3e-02, 7.1e-05),     # 4.91e-04 / 5.86e-03 / 1.79e-05; floor 1.06e-05 / 1.93e-04 / 2.99e-07
        "att1_fc1.weight":     (2.3e-03, 7.9e-03, 1.2e-04),     # 5.81e-04 / 1.98e-03 / 3.14e-05; floor 3.86e-04 / 1.10e-03 / 3.18e-06
        "att1_fc2.weight":     (1.7e-03, 1.0e-02, 4.8e-05),     # 4.37e-04 / 2.64e-03 / 1.20e-05; floor 2.77e-04 / 2.38e-03 / 1.44e-05
        "att2_fc1.weight":     (1.2e-03, 1.0e-02, 2.5e-05),     # 3.13e-04 / 2.50e-03 / 6.30e-06; floor 1.65e-04 / 1.29e-03 / 3.66e-06
        "att2_fc2.weight":     (2.3e-04, 2.6e-03, 2.3e-05),     # 5.94e-05 / 6.72e-04 / 5.85e-06; floor 4.86e-05 / 5.50e-04 / 5.55e-06
        "gamma1_fc1.weight":   (1.2e-03, 5.2e-03, 2.0e-04),     # 3.07e-04 / 1.32e-03 / 5.19e-05; floor 5.64e-05 / 3.32e-04 / 5.24e-07
        "gamma1_fc2.weight":   (5.9e-04, 3.1e-03, 1.3e-04),     # 1.48e-04 / 7.90e-04 / 3.26e-05; floor 1.99e-05 / 2.25e-04 / 1.16e-07
        "gamma2_fc1.weight":   (9.1e-04, 7.0e-03, 2.7e-04),     # 2.28e-04 / 1.76e-03 / 6.88e-05; floor 4.29e-07 / 3.43e-06 / 1.08e-07
        "gamma2_fc2.weight":   (4.2e-04, 1.1e-03, 6.4e-05),     # 1.05e-04 / 2.97e-04 / 1.62e-05; floor 2.94e-06 / 3.33e-05 / 1.41e-07
        "out_fc1.weight":      (3.3e-04, 1.0e-03, 1.2e-05),     # 8.30e-05 / 2.50e-04 / 3.08e-06; floor 0 / 0 / 0
        "out_fc2.weight":      (1.0e-03, 1.0e-03, 9.9e-05),     # 2.60e-04 / 2.60e-04 / 2.48e-05; floor 0 / 0 / 0
    },
}


def tier(c):
    return "exact" if c["B"] == 1 and c["T"] <= 2 else "short" if c["T"] <= 7 else "long"


def bounds(c):
    return BOUNDS[tier(c)]


# ------------------------------------------------------------------------------------------------ inputs (CPU)
_P32 = {}


def params32(c):
    """the recipe's fp32 parameters of an MFN over the case's modalities"""
    if c["id"] not in _P32:
        gate = mta().multiTransformer.MFN(c["mods"], dict(zip(c["mods"], c["widths"])), 1, device=torch.device("cpu"))
        _P32[c["id"]] = R.gen_params(R.shapes_of(gate.state_dict()), 37)
    return _P32[c["id"]]


def hidden_sizes(c):
    return [mta().multiTransformer.MFN.hidden_dim[m] for m in c["mods"]]


def state_inputs(c):
    """hs, cs as leaves of their own: tanh-limited normals, cs scaled to [-2, 2]; g the gradient of the (T, B, 1) output"""
    tag, T, B = "bfgate:" + c["id"], c["T"], c["B"]
    hs = [torch.tanh(R.gen_normal("%s:h%d" % (tag, i), (T, B, H), 37)) for i, H in enumerate(hidden_sizes(c))]
    cs = [2.0 * torch.tanh(R.gen_normal("%s:c%d" % (tag, i), (T, B, H), 37)) for i, H in enumerate(hidden_sizes(c))]
    return hs, cs, R.gen_normal(tag + ":g", (T, B, 1), 37)


def module_inputs(c):
    """x of every modality, a ragged prefix mask whose last sequence has one window, g the gradient of the (B, T, 1) output"""
    tag, T, B = "bfgate:" + c["id"], c["T"], c["B"]
    x = {m: R.gen_normal("%s:x:%s" % (tag, m), (T, B, w), 37) for m, w in zip(c["mods"], c["widths"])}
    lengths = [max(1, T - (3 * b) % T) for b in range(B - 1)] + [1]
    return x, R.prefix_mask(lengths, T), R.gen_normal(tag + ":gm", (B, T, 1), 37)


def seeds(c, entry):
    return 880001 + 2 * (IDS.index(c["id"]) * 2 + entry), 880002 + 2 * (IDS.index(c["id"]) * 2 + entry)


def synthetic_drops(c):
    """dropout multipliers of the kernels' probabilities without a GPU (the CPU jitter floor): Bernoulli keeps from the recipe"""
    T, B = c["T"], c["B"]
    gd = (R.gen_uniform("bfgate:gd:" + c["id"], (T, B, 128), 37) >= PG).double() / (1 - PG)
    od = (R.gen_uniform("bfgate:od:" + c["id"], (T, B, 64), 37) >= PO).double() / (1 - PO)
    return gd, od


# ------------------------------------------------------------------------------------------------ the reference (CPU, fp64)
def ref_gate(c, gd=None, od=None, rounding=True):
    """gate_from_states on the case's leaves -> {"out", "d_hs:i", "d_cs:i", "grad:<gate tensor>"} as fp64 arrays"""
    pd = {k: v.double().requires_grad_() for k, v in params32(c).items()}
    hs, cs, g = state_inputs(c)
    hs, cs = [t.double().requires_grad_() for t in hs], [t.double().requires_grad_() for t in cs]
    y = S.gate_from_states(pd, "", hs, cs, gd, od, rounding=rounding)
    y.backward(g.double())
    out = {"out": y.detach().numpy()}
    for i in range(len(hs)):
        out["d_hs:%d" % i], out["d_cs:%d" % i] = hs[i].grad.numpy(), cs[i].grad.numpy()
    out.update({"grad:" + n: pd[n].grad.numpy() for n in GATE_NAMES})
    return out


def ref_module(c, gd=None, od=None, masked=True, rounding=True):
    """batch_composition on the case's inputs -> {"out" (B, T, 1), "dx:<mod>", "grad:<every parameter>"} as fp64 arrays"""
    pd = {k: v.double().requires_grad_() for k, v in params32(c).items()}
    x, mask, g = module_inputs(c)
    xd = {m: v.double().requires_grad_() for m, v in x.items()}
    y = S.batch_composition(pd, "", xd, c["mods"], rounding=rounding, gamma_drop=gd, out_drop=od, mask=mask.double() if masked else None)
    y.backward(g.double())
    out = {"out": y.detach().numpy()}
    out.update({"dx:" + m: xd[m].grad.numpy() for m in c["mods"]})
    out.update({"grad:" + n: v.grad.numpy() for n, v in pd.items()})
    return out


# ------------------------------------------------------------------------------------------------ the comparison
def group_of(name):
    """the entry of BOUNDS a tensor is held to: its own name for a gate tensor, the kind for the tensors every modality has"""
    if name == "out" or name.startswith(("d_hs", "d_cs", "dx")):
        return name.split(":")[0]
    if name.startswith("grad:lstm_"):
        return "lstm.bias" if ".bias_" in name else "lstm." + name.rsplit(".", 1)[1]
    return name[len("grad:"):]


def compare(tag, got, ref, bd, failures, batch_major_out=False):
    """every tensor of `ref` against its twin in `got` under the bounds bd: {group_of(name): (rel-L2, per row, third)}, third the
    per-sequence maximum of a per-window tensor and the least-squares scale of a weight matrix.  A reference that is exactly zero
    (dW_hh at T = 1: h_{-1} = 0) asks for exact zeros."""
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    for name in ref:
        g, r = np.asarray(got[name], dtype=np.float64), ref[name]
        assert g.shape == r.shape, (tag, name, g.shape, r.shape)
        grp, t = group_of(name), "%s|%s" % (tag, name)
        if not np.isfinite(g).all():
            failures.append("%s: not finite" % t)
        elif not r.any():
            print("%-52s zero reference, got max abs %.2e" % (t, np.abs(g).max() if g.size else 0.0))
            if g.any():
                failures.append("%s: the reference is exactly zero, got max abs %.3e" % (t, np.abs(g).max()))
        elif grp in STATE_KEYS:
            if name == "out" and batch_major_out:
                g, r = np.swapaxes(g, 0, 1), np.swapaxes(r, 0, 1)
            check_scan(t, g, r, bd[grp], failures, seq=True)
            if grp == "d_cs":                       # t = 0 / inner steps / t = T - 1 alone: a shift applied to the wrong part shows here
                T = r.shape[0]
                for lab, sl in (("t0", slice(0, 1)), ("mid", slice(1, T - 1)), ("last", slice(T - 1, T))):
                    if r[sl].size and (lab != "last" or T > 1):
                        check("%s@%s" % (t, lab), g[sl], r[sl], bd["d_cs_t"][0], bd["d_cs_t"][1], failures=failures)
        elif r.ndim == 2:
            check_scan(t, g, r, bd[grp], failures, scale=bd[grp][2])
        else:
            check_scan(t, g.ravel(), r.ravel(), bd[grp], failures)


def drops_visible(tag, with_drops, without):
    d = rel_l2(without, with_drops)
    print("%-52s the masks move the reference's output by %.2e" % (tag, d))
    assert d > 1e-2, "%s: the masks changed nothing (%.2e): the test would not see a wrong one" % (tag, d)


def check_kernels(tag, names, B):
    """the memory scan the case is labelled for ran, forward and backward, and no library kernel"""
    if names is None:
        return                              # the profiler reports no device kernels on this box: only this assertion is skipped
    SC.check_ran(tag, [n for n in names if "mfn_mem_scan" in n], SC.mfn_family(B))
    assert library_kernels(names) == [], "%s: library kernels %s" % (tag, library_kernels(names))


def device_drops(F, c, sg, so, dev):
    """the multipliers of the masks the kernels draw: gamma stream 1000, index (t B + b) 128 + unit, gamma1's 64 units first; out
    stream 2001, index m 64 + n"""
    T, B = c["T"], c["B"]
    kg, scg = F.dropout_mask(PG, sg, 1000, T * B * 128, dev)
    ko, sco = F.dropout_mask(PO, so, 2001, T * B * 64, dev)
    return (kg.reshape(T, B, 128).double() * scg).cpu(), (ko.reshape(T, B, 64).double() * sco).cpu()


def _np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ 1. F.mfn_gate(hs, cs, params)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mfn_gate(dev, c, mode):
    """F.mfn_gate on leaves of its own: out, d_hs and d_cs of every modality and the 20 gate gradients against gate_from_states"""
    F, MT = mta().functional, mta().multiTransformer
    gate = MT.MFN(c["mods"], dict(zip(c["mods"], c["widths"])), 1, device=dev)
    gate.load_state_dict(params32(c))
    params = gate._gate_params()
    hs, cs, g = state_inputs(c)
    hs, cs = [t.to(dev).requires_grad_() for t in hs], [t.to(dev).requires_grad_() for t in cs]
    g = g.to(dev)
    train = mode == "train"
    sg, so = seeds(c, 0)
    kw = dict(gamma_dropout=PG, gamma_seed=sg, out_dropout=PO, out_seed=so) if train else {}
    nm = len(hs)

    def step():
        y = F.mfn_gate(hs, cs, params, **kw)
        return (y.detach(),) + torch.autograd.grad(y, hs + cs + params, g)

    def named(res):
        out = {"out": res[0]}
        for i in range(nm):
            out["d_hs:%d" % i], out["d_cs:%d" % i] = res[1 + i], res[1 + nm + i]
        out.update({"grad:" + n: t for n, t in zip(GATE_NAMES, res[1 + 2 * nm:])})
        return out
    first, names = device_kernel_names(step, warm=True)      # the pool zero-fills a workspace it allocates: not in the profiled call
    F.check_device_errors()
    tag = "gate|%s|%s|%s" % (tier(c), c["id"], mode)
    check_kernels(tag, names, c["B"])
    again = named(step())
    first = named(first)
    for n in first:
        assert torch.equal(first[n], again[n]), "%s %s: two runs with the same seeds differ" % (tag, n)
    gd = od = None
    if train:
        gd, od = device_drops(F, c, sg, so, dev)
    ref = ref_gate(c, gd, od)
    if train:
        drops_visible(tag, ref["out"], ref_gate_eval_out(c))
    failures = []
    compare(tag, _np(first), ref, bounds(c), failures)
    F.check_device_errors()
    assert not failures, "\n".join(failures)


_EVAL_OUT = {}


def ref_gate_eval_out(c):
    if c["id"] not in _EVAL_OUT:
        with torch.no_grad():
            hs, cs, _ = state_inputs(c)
            pd = {k: v.double() for k, v in params32(c).items()}
            _EVAL_OUT[c["id"]] = S.gate_from_states(pd, "", [t.double() for t in hs], [t.double() for t in cs]).numpy()
    return _EVAL_OUT[c["id"]]


# ------------------------------------------------------------------------------------------------ 2. MFN._gate / MFN.forward
MODULE_MODES = [(c, m) for c in CASES for m in MODES] + [(c, "train_nomask") for c in CASES if c["T"] <= 3]


@pytest.mark.parametrize("c,mode", MODULE_MODES, ids=["%s-%s" % (c["id"], m) for c, m in MODULE_MODES])
def test_mfn_module(dev, c, mode, monkeypatch):
    """MFN._gate under a ragged prefix mask (train_nomask: MFN.forward, mask=None, in train mode): out, dx of every modality, the four
    tensors of every cell and the 20 gate gradients against batch_composition; the two biases of a cell share one gradient"""
    F, MT, L = mta().functional, mta().multiTransformer, mta()._lib
    gate = MT.MFN(c["mods"], dict(zip(c["mods"], c["widths"])), 1, device=dev)
    gate.load_state_dict(params32(c))
    train, masked = mode != "eval", mode != "train_nomask"
    gate = gate.train() if train else gate.eval()
    sg, so = seeds(c, 1)
    real = L.next_dropout_seed
    fixed = {2: sg, 4: so}
    monkeypatch.setattr(L, "next_dropout_seed",
                        lambda device, site, holder=None, index=0: fixed[site] if site in fixed else real(device, site, holder, index))
    x, mask, g = module_inputs(c)
    ins = {m: x[m].to(dev).requires_grad_() for m in c["mods"]}
    mask_d, g = mask.to(dev), g.to(dev)
    pnames = [n for n, _ in gate.named_parameters()]
    params = [q for _, q in gate.named_parameters()]
    leaves = [ins[m] for m in c["mods"]] + params

    def named(y, grads):
        out = {"out": y}
        out.update({"dx:" + m: t for m, t in zip(c["mods"], grads)})
        out.update({"grad:" + n: t for n, t in zip(pnames, grads[len(c["mods"]):])})
        return out

    def step():
        y = gate._gate(ins, mask_d) if masked else gate(ins)
        return named(y.detach(), torch.autograd.grad(y, leaves, g))
    first, names = device_kernel_names(step, warm=True)      # the pool zero-fills a workspace it allocates: not in the profiled call
    F.check_device_errors()
    tag = "module|%s|%s|%s" % (tier(c), c["id"], mode)
    check_kernels(tag, names, c["B"])
    # once more through .backward(): the same bits in every .grad, and the two biases of a cell share theirs
    y = gate._gate(ins, mask_d) if masked else gate(ins)
    y.backward(g)
    again = named(y.detach(), [t.grad for t in leaves])
    for n in first:
        assert torch.equal(first[n], again[n]), "%s %s: two runs with the same seeds differ" % (tag, n)
    for m in c["mods"]:
        cell = gate.lstm[m]
        assert torch.equal(cell.bias_ih.grad, cell.bias_hh.grad), "%s: bias_ih.grad and bias_hh.grad of lstm_%s differ" % (tag, m)
    if masked:
        assert (first["out"][mask_d.expand_as(first["out"]) == 0] == 0).all(), "%s: a masked window is not an exact zero" % tag
    gd = od = None
    if train:
        gd, od = device_drops(F, c, sg, so, dev)
    ref = ref_module(c, gd, od, masked)
    if train:
        drops_visible(tag, ref["out"], ref_module_eval_out(c, masked))
    failures = []
    compare(tag, _np(first), ref, bounds(c), failures, batch_major_out=True)
    F.check_device_errors()
    assert not failures, "\n".join(failures)


def ref_module_eval_out(c, masked):
    key = (c["id"], masked)
    if key not in _EVAL_OUT:
        with torch.no_grad():
            x, mask, _ = module_inputs(c)
            pd = {k: v.double() for k, v in params32(c).items()}
            _EVAL_OUT[key] = S.batch_composition(pd, "", {m: v.double() for m, v in x.items()}, c["mods"],
                                                 mask=mask.double() if masked else None).numpy()
    return _EVAL_OUT[key]
