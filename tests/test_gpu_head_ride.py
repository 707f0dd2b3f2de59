"""The head of the forward pass at the d_model = 128 fixed shape in train mode: the first launch only prepares weights (and, with a
device-resident seed, advances it in one extra workgroup) and layer 0's attention-dropout decisions are drawn by generator workgroups
riding in layer 0's `ln1+qkv` launch (rowgemm.h: encoder_ln1_qkv128_kernel) — against the head MMT_NO_MASK_RIDE=1 restores (a
`seed_advance` launch, an up-front generator for every layer with the preparation in its grid, a plain `ln1+qkv`), each in a process
of its own (the switch is read once per process).

The bits are a pure function of (seed, layer, batch*head, query, key), the seed block holds the same words whoever writes it and the
tile workgroups of `ln1+qkv` run the same arithmetic with or without riders behind them, so the output, the input gradient and every
parameter gradient of a train-mode forward + backward are BIT-identical between the two heads.

Shapes (d, h, f, N, B, T), the smallest that reach each corner of the new launch (a generator workgroup draws 256 blocks of 32x32
decisions, a tile workgroup owns 32 windows; lengths are ragged):
  (128, 8, 128, 1, 2, 70)    one layer: 144 blocks = one riding workgroup, its third wave a quarter full and its fourth empty; 5 tile
                             workgroups, the last of 12 rows; nothing else rides
  the same, device seed      two consecutive steps in one process: each equals the reference side's (the folded advance writes the
                             same block) and the two differ (the state moved exactly once per forward: an advance skipped or done
                             twice breaks one of the two comparisons)
  (128, 8, 128, 2, 2, 300)   1 600 blocks: 7 riding workgroups, the last a single wave; 19 tile workgroups; `ln1+qkv` and the layer-0
                             chain both carry riders; the one-kernel backward reads the LK layout
  (128, 8, 128, 2, 1, 1056)  the 35 riders outnumber the 33 tile workgroups; nt = 33; the two-kernel backward reads both layouts
  (128, 8, 128, 2, 2, 70)    p = 0: no rider, no seed, the preparation-only launch of the eval path"""
import os
import sys

import numpy as np
import pytest

import conftest

pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
import numpy as np
import torch
from multimodal_transformer_amd import multiTransformer as MT
d, h, f, n, B, T = (int(v) for v in sys.argv[1:7])
p, steps, out = float(sys.argv[7]), int(sys.argv[8]), sys.argv[9]
dev = torch.device("cuda:0")
torch.manual_seed(11)
enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, p), p), n).to(dev).train()
x = torch.randn(B, T, d, device=dev, requires_grad=True)
lengths = [T, max(1, T // 2), max(1, T - 7)][:B]
mask = torch.zeros(B, T, 1, device=dev)
for i, L in enumerate(lengths):
    mask[i, :L] = 1.0
torch.manual_seed(5)                    # the dropout seeds are drawn from this generator
saved = {}
for s in range(steps):
    x.grad = None
    enc.zero_grad(set_to_none=True)
    y = enc(x, mask)
    (y * torch.linspace(-1, 1, y.numel(), device=dev).view_as(y)).sum().backward()
    torch.cuda.synchronize()
    saved["y%d" % s] = y.detach().cpu().numpy()
    saved["dx%d" % s] = x.grad.cpu().numpy()
    saved["dp%d" % s] = torch.cat([q.grad.reshape(-1) for q in enc.parameters()]).cpu().numpy()
np.savez(out, **saved)
"""


def _run(shape, p, devseed, steps, ride, out):
    env = dict(os.environ)
    for k in ("MMT_NO_MASK_RIDE", "MMT_NO_FIXED_SHAPES", "MMT_NO_CHAIN4", "MMT_DEVICE_SEED"):
        env.pop(k, None)
    if not ride:
        env["MMT_NO_MASK_RIDE"] = "1"
    if devseed:
        env["MMT_DEVICE_SEED"] = "1"      # the device-seed entry points outside a graph capture
    env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    res = conftest.run_in_fresh_process([sys.executable, "-c", _CHILD] + [str(v) for v in shape] + [str(p), str(steps), out], env, timeout=600)
    if res is None:
        pytest.skip("no launcher process (tests were collected with the GPU already initialised)")
    assert res["rc"] == 0, res["stderr"][-2000:]
    return np.load(out)


_CASES = [
    pytest.param((128, 8, 128, 1, 2, 70), 0.1, False, 1, id="one-layer-one-partial-rider"),
    pytest.param((128, 8, 128, 1, 2, 70), 0.1, True, 2, id="device-seed-two-steps"),
    pytest.param((128, 8, 128, 2, 2, 300), 0.1, False, 1, id="several-riders-and-chain-riders"),
    pytest.param((128, 8, 128, 2, 1, 1056), 0.1, False, 1, id="riders-outnumber-tiles"),
    pytest.param((128, 8, 128, 2, 2, 70), 0.0, False, 1, id="no-dropout-preparation-only"),
]


@pytest.mark.parametrize("shape,p,devseed,steps", _CASES)
def test_riding_head_equals_the_upfront_head(tmp_path, shape, p, devseed, steps):
    ride = _run(shape, p, devseed, steps, True, str(tmp_path / "ride.npz"))
    upfront = _run(shape, p, devseed, steps, False, str(tmp_path / "upfront.npz"))
    for s in range(steps):
        for k in ("y%d" % s, "dx%d" % s, "dp%d" % s):
            assert np.isfinite(ride[k]).all(), "%s: non-finite values with the riding head" % k
            assert np.isfinite(upfront[k]).all(), "%s: non-finite values with the up-front head" % k
            assert np.array_equal(ride[k], upfront[k]), (
                "%s: %d of %d values differ between the riding head and the up-front head"
                % (k, int((ride[k] != upfront[k]).sum()), ride[k].size))
    if steps > 1:       # a fresh seed per forward: the state advanced between the steps (and, by the equalities above, exactly once)
        assert not np.array_equal(ride["y0"], ride["y1"]), "two consecutive device-seeded steps drew the same masks"
