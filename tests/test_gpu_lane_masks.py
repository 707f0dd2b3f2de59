"""The lane-mask form of the attention-dropout words (attn_mask.h): where a layer's forward is the plain d_k = 16 train kernel and
its backward the one-kernel form, the generator stores the query-side words as sixteen 64-bit lane masks per 32x32 block and the forward
applies them with one v_cndmask_b32 per accumulator register.  MMT_NO_LANE_MASKS=1 restores the 16-bit lane words everywhere.

Nothing about the decisions changes — the same bits of the same generator, and a dropped probability becomes +0 either way — so
  * both forms of the stored words decode to the same (B, h, T, T) boolean array, and
  * a train-mode forward + backward of the encoder stack is BIT-identical with and without the switch, on shapes that take the new
    form (T = 257: 9 key tiles with a one-window tail; T = 500: the headline's 16 tiles with a tail) and on shapes that must keep the
    old one (T = 200: the two-kernel backward reads the query-side words; d_model = 40, h = 4: d_k = 10).
The switch is read once per process, so each side of the comparison is one fresh child process that runs every shape."""
import os
import sys

import numpy as np
import pytest

import conftest

pytestmark = pytest.mark.gpu

_KEY = np.array([[(i & 3) + 8 * (i >> 2) + 4 * hh for i in range(16)] for hh in range(2)])      # key of accumulator register i, half hh


def _decode_lane_words(lq, nbh, nt):
    """LQ, 16-bit form: block (bh, q tile, k tile), lane 32 hh + q, bit i = (query q, key _KEY[hh, i])"""
    w = lq.view(np.uint16).reshape(nbh, nt, nt, 2, 32)
    bits = (w[..., None] >> np.arange(16, dtype=np.uint16)) & 1                                 # (.., hh, q, i)
    blk = np.zeros((nbh, nt, nt, 32, 32), dtype=bool)
    for hh in range(2):
        blk[..., _KEY[hh]] = bits[..., hh, :, :] != 0
    return blk.transpose(0, 1, 3, 2, 4).reshape(nbh, nt * 32, nt * 32)


def _decode_lane_masks(lq, nbh, nt):
    """LQ, lane-mask form: block, word i (uint64, little endian), bit r + 32 hh = (query r, key _KEY[hh, i])"""
    w = np.ascontiguousarray(lq).view(np.uint64).reshape(nbh, nt, nt, 16)
    bits = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)                      # (.., i, lane)
    blk = np.zeros((nbh, nt, nt, 32, 32), dtype=bool)
    for hh in range(2):
        blk[..., _KEY[hh]] = bits[..., 32 * hh:32 * hh + 32].swapaxes(-1, -2) != 0              # (.., r, i)
    return blk.transpose(0, 1, 3, 2, 4).reshape(nbh, nt * 32, nt * 32)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("T", [257, 288, 500])
def test_both_forms_hold_the_same_decisions(T, p):
    import torch
    from multimodal_transformer_amd import functional as F
    B, h, nt = 2, 2, (T + 31) // 32
    dev = torch.device("cuda:0")
    seed, stream = 0x5EED0000 + T, 4
    old_q, old_k = (a.cpu().numpy() for a in F._attn_mask_words(p, seed, stream, B * h, nt, dev, lanes=False))
    new_q, new_k = (a.cpu().numpy() for a in F._attn_mask_words(p, seed, stream, B * h, nt, dev, lanes=True))
    old = _decode_lane_words(old_q, B * h, nt)[:, :T, :T].reshape(B, h, T, T)
    new = _decode_lane_masks(new_q, B * h, nt)[:, :T, :T].reshape(B, h, T, T)
    print("T=%d p=%g: kept %.4f (old form) %.4f (lane masks), %d decisions differ" % (T, p, old.mean(), new.mean(), int((old != new).sum())))
    assert np.array_equal(old, new)
    assert np.array_equal(old_k, new_k), "the key-side words keep their form"
    # ... and they are the generator's decisions, not merely each other's: the replay hook expands the same blocks
    keep, _ = F.dropout_mask(p, seed, stream, B * h * (nt * 32) ** 2, dev, attn_Tp=nt * 32)
    ref = keep.cpu().numpy().reshape(B * h, nt * 32, nt * 32)[:, :T, :T].reshape(B, h, T, T)
    assert np.array_equal(new, ref)
    assert abs(new.mean() - (1.0 - p)) < 0.01          # 4 T^2 >= 264 196 draws: sigma < 0.001


# (d, h, f, N, B, T, p): the first four take the lane-mask form, the last two must keep the lane words
_SHAPES = {
    "T257-p0.1": (128, 8, 128, 2, 2, 257, 0.1),
    "T257-p0.25": (128, 8, 128, 2, 2, 257, 0.25),
    "T500-p0.1": (128, 8, 128, 2, 2, 500, 0.1),
    "T500-p0.25": (128, 8, 128, 2, 2, 500, 0.25),
    "fallback-T200": (128, 8, 128, 2, 2, 200, 0.1),
    "fallback-dk10": (40, 4, 128, 2, 2, 257, 0.1),
}

_CHILD = r"""
import sys
import numpy as np
import torch
from multimodal_transformer_amd import multiTransformer as MT
out = sys.argv[1]
dev = torch.device("cuda:0")
res = {}
for spec in sys.argv[2:]:
    name, d, h, f, n, B, T, p = spec.split(",")
    d, h, f, n, B, T, p = int(d), int(h), int(f), int(n), int(B), int(T), float(p)
    torch.manual_seed(11)
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, p), p), n).to(dev).train()
    x = torch.randn(B, T, d, device=dev, requires_grad=True)
    mask = torch.ones(B, T, 1, device=dev)
    torch.manual_seed(5)                    # the dropout seeds are drawn from this generator
    y = enc(x, mask)
    (y * torch.linspace(-1, 1, y.numel(), device=dev).view_as(y)).sum().backward()
    torch.cuda.synchronize()
    res[name + "/y"] = y.detach().cpu().numpy()
    res[name + "/dx"] = x.grad.cpu().numpy()
    for i, q in enumerate(enc.parameters()):
        res[name + "/dp%02d" % i] = q.grad.cpu().numpy()
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def both_runs(tmp_path_factory):
    """{False: arrays of the default run, True: arrays under MMT_NO_LANE_MASKS=1}, every shape in one child process per side"""
    tmp = tmp_path_factory.mktemp("lane_masks")
    runs = {}
    for off in (False, True):
        env = dict(os.environ)
        for k in ("MMT_NO_LANE_MASKS", "MMT_NO_FUSED_ATTN_BWD", "MMT_NO_MASK_RIDE", "MMT_NO_FIXED_SHAPES", "MMT_NO_CHAIN4", "MMT_DEVICE_SEED"):
            env.pop(k, None)
        if off:
            env["MMT_NO_LANE_MASKS"] = "1"
        env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = str(tmp / ("off.npz" if off else "on.npz"))
        specs = [",".join([name] + [str(v) for v in s]) for name, s in _SHAPES.items()]
        res = conftest.run_in_fresh_process([sys.executable, "-c", _CHILD, out] + specs, env, timeout=600)
        if res is None:
            pytest.skip("no launcher process (tests were collected with the GPU already initialised)")
        assert res["rc"] == 0, res["stderr"][-2000:]
        with np.load(out) as z:
            runs[off] = {k: z[k] for k in z.files}
    return runs


@pytest.mark.parametrize("name", list(_SHAPES))
def test_results_do_not_depend_on_the_form(both_runs, name):
    on, off = both_runs[False], both_runs[True]
    keys = sorted(k for k in on if k.startswith(name + "/"))
    assert len(keys) > 2 and keys == sorted(k for k in off if k.startswith(name + "/"))
    for k in keys:
        assert np.isfinite(on[k]).all(), "%s: non-finite values" % k
        assert np.array_equal(on[k], off[k]), (
            "%s: %d of %d values differ between the default forms and MMT_NO_LANE_MASKS=1" % (k, int((on[k] != off[k]).sum()), on[k].size))
