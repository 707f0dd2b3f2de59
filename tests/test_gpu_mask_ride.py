"""Attention-dropout decisions drawn inside the forward row chains (rowgemm.h: the generator role of the d_model = 128 four-stage chain;
layer l's launch draws layer l+1's bits) against the single up-front generator launch (MMT_NO_MASK_RIDE=1), each in a process of its
own (the switch is read once per process).

The bits are a pure function of (seed, layer, batch*head, query, key) and the chain's arithmetic is the same kernel instance in both
runs — only the place where the bits are drawn differs —, so the output, the input gradient and every parameter gradient of a
train-mode forward + backward are BIT-identical.

Shapes (d, h, f, N, B, T), the smallest that reach each corner of the riding launch (a generator workgroup draws 256 blocks of 32x32
decisions, a chain workgroup owns 32 windows):
  (128, 8, 128, 3, 3, 70)    216 blocks per layer: one generator workgroup, its last wave partly filled; ragged lengths; two riding launches
  (128, 8, 128, 2, 2, 300)   1 600 blocks: several generator workgroups, the last one partial; the one-kernel backward reads the LK layout
  (128, 8, 128, 2, 1, 1056)  8 712 blocks: the generator workgroups (35) outnumber the chain's (33); nt = 33
  (128, 8, 128, 1, 2, 70)    one layer: nothing rides"""
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
p, out = float(sys.argv[7]), sys.argv[8]
dev = torch.device("cuda:0")
torch.manual_seed(11)
enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, p), p), n).to(dev).train()
x = torch.randn(B, T, d, device=dev, requires_grad=True)
lengths = [T, max(1, T // 2), max(1, T - 7)][:B]
mask = torch.zeros(B, T, 1, device=dev)
for i, L in enumerate(lengths):
    mask[i, :L] = 1.0
torch.manual_seed(5)                    # the dropout seeds are drawn from this generator
y = enc(x, mask)
(y * torch.linspace(-1, 1, y.numel(), device=dev).view_as(y)).sum().backward()
torch.cuda.synchronize()
np.savez(out, y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dp=torch.cat([q.grad.reshape(-1) for q in enc.parameters()]).cpu().numpy())
"""


def _run(shape, p, devseed, ride, out):
    env = dict(os.environ)
    for k in ("MMT_NO_MASK_RIDE", "MMT_NO_FIXED_SHAPES", "MMT_NO_CHAIN4", "MMT_DEVICE_SEED"):
        env.pop(k, None)
    if not ride:
        env["MMT_NO_MASK_RIDE"] = "1"
    if devseed:
        env["MMT_DEVICE_SEED"] = "1"      # the device-seed entry points outside a graph capture
    env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    res = conftest.run_in_fresh_process([sys.executable, "-c", _CHILD] + [str(v) for v in shape] + [str(p), out], env, timeout=600)
    if res is None:
        pytest.skip("no launcher process (tests were collected with the GPU already initialised)")
    assert res["rc"] == 0, res["stderr"][-2000:]
    return np.load(out)


_CASES = [
    pytest.param((128, 8, 128, 3, 3, 70), 0.1, False, id="partial-wave-group"),
    pytest.param((128, 8, 128, 3, 3, 70), 0.1, True, id="partial-wave-group-device-seed"),
    pytest.param((128, 8, 128, 2, 2, 300), 0.1, False, id="several-generator-workgroups"),
    pytest.param((128, 8, 128, 2, 1, 1056), 0.1, False, id="generators-outnumber-chain"),
    pytest.param((128, 8, 128, 1, 2, 70), 0.1, False, id="one-layer-nothing-rides"),
    pytest.param((128, 8, 128, 3, 3, 70), 0.0, False, id="no-dropout-no-generator"),
]


@pytest.mark.parametrize("shape,p,devseed", _CASES)
def test_riding_generator_draws_the_same_bits_as_the_upfront_launch(tmp_path, shape, p, devseed):
    ride = _run(shape, p, devseed, True, str(tmp_path / "ride.npz"))
    upfront = _run(shape, p, devseed, False, str(tmp_path / "upfront.npz"))
    for k in ("y", "dx", "dp"):
        assert np.isfinite(ride[k]).all(), "%s: non-finite values with the riding generator" % k
        assert np.array_equal(ride[k], upfront[k]), (
            "%s: %d of %d values differ between the riding generator and the up-front launch"
            % (k, int((ride[k] != upfront[k]).sum()), ride[k].size))
