"""GPU: functional.local_attention(..., over="taps") (csrc/local_attn.h's second mode, mmt_local_attn_forward_taps / _backward_taps): the
softmax over the L taps of each row, what models.attend_over_taps turns on.

Forward, dz and dh against fp64 autograd of tests/lstm_stream_ref.local_attention_taps under the project's LA_RTOL = 1e-5 (the same fp32
arithmetic class as the time mode, with sums over <= 16 taps instead of T steps); dh exactly zero at padded steps; the same bits on a
second run; and, with NO tolerance, the prefix property: what lies behind step t0 cannot reach ctx[:, :t0 + 1].
"""
import pytest
import torch

import lstm_stream_ref as LS
import recipe as R
from conftest import rel_l2
from gpu_harness import dev  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

LA_RTOL = 1e-5                           # tests/test_gpu_lstm_baselines.py's

CASES = [  # (B, T, H, L, ragged)
    (1, 1, 256, 1, False), (1, 3, 130, 5, True), (3, 3, 1024, 7, True), (3, 37, 130, 16, True), (25, 37, 256, 5, True), (3, 70, 256, 5, False),
]
IDS = ["B%d_T%d_H%d_L%d_%s" % (c[:4] + ("ragged" if c[4] else "full",)) for c in CASES]
_CACHE = {}


def _lengths(B, T, ragged):
    return [max(1, T - (T * k) // (B + 1)) for k in range(B)] if ragged else [T] * B


def _inputs(B, T, H, L, ragged):
    tag = "%d_%d_%d_%d" % (B, T, H, L)
    z = R.gen_normal("la_taps:%s:z" % tag, (B, T, L), 5) * 2.0
    h = torch.tanh(R.gen_normal("la_taps:%s:h" % tag, (T, B, H), 5))
    valid = R.prefix_mask(_lengths(B, T, ragged), T).reshape(B, T)
    g = R.gen_normal("la_taps:%s:g" % tag, (B, T, H), 5)
    return z, h, valid, g


def _gpu(F, dev, z, h, valid, g):
    zs, hs = z.to(dev).requires_grad_(), h.to(dev).requires_grad_()
    out = F.local_attention(zs, hs, valid.to(dev), over="taps")
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), zs.grad.cpu(), hs.grad.cpu()


def _run(c, dev):
    """the GPU results (two runs) and the fp64 reference of one case, computed once"""
    if c not in _CACHE:
        from multimodal_transformer_amd import functional as F
        z, h, valid, g = _inputs(*c)
        zd, hd = z.double().requires_grad_(), h.double().requires_grad_()
        ref = LS.local_attention_taps(zd, hd, valid.double())
        ref.backward(g.double())
        _CACHE[c] = dict(valid=valid, runs=[_gpu(F, dev, z, h, valid, g) for _ in range(2)], ref=(ref.detach(), zd.grad, hd.grad))
    return _CACHE[c]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_taps_mode_against_fp64(dev, c):
    r = _run(c, dev)
    errs = [rel_l2(a.numpy(), b.numpy()) for a, b in zip(r["runs"][0], r["ref"])]
    print("local_attention over taps %s: ctx %.2e dz %.2e dh %.2e" % ((IDS[CASES.index(c)],) + tuple(errs)))
    assert all(torch.isfinite(a).all() for a in r["runs"][0])
    assert errs[0] < LA_RTOL and errs[1] < LA_RTOL and errs[2] < LA_RTOL
    pad = r["valid"] == 0
    assert (r["runs"][0][2].permute(1, 0, 2)[pad] == 0).all(), "no gradient into h at padded steps"
    assert c[3] == 1 or r["runs"][0][1].abs().max() > 0                               # dz is not trivially zero (one tap: it is)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_taps_mode_is_bit_reproducible(dev, c):
    r = _run(c, dev)
    for a, b in zip(*r["runs"]):
        assert torch.equal(a, b)


def test_taps_mode_is_not_the_time_mode(dev):
    """the two modes differ where they should (and the default is the time mode, with its own entry)"""
    from multimodal_transformer_amd import functional as F
    z, h, valid, _ = _inputs(3, 37, 130, 16, True)
    zg, hg, vg = z.to(dev), h.to(dev), valid.to(dev)
    time, taps = F.local_attention(zg, hg, vg), F.local_attention(zg, hg, vg, over="taps")
    assert torch.equal(time, F.local_attention(zg, hg, vg, over="time")) and not torch.equal(time, taps)
    torch.cuda.synchronize()


@pytest.mark.parametrize("t0", [0, 31, 32, 36])
def test_the_prefix_keeps_its_bits(dev, t0):
    """z and h at steps > t0 replaced by other values: ctx[:, :t0 + 1] keeps its bits (T = 37: t0 at the first step, on either side of
    the 32-step tile's edge and at the last step, where nothing is replaced); the time mode, whose statistics run over all T, does not"""
    from multimodal_transformer_amd import functional as F
    B, T, H, L = 3, 37, 130, 16
    z, h, valid, _ = _inputs(B, T, H, L, True)
    valid = torch.ones(B, T)                                 # every step real: nothing hides a later step
    z2, h2 = z.clone(), h.clone()
    z2[:, t0 + 1:] = R.gen_normal("la_taps:prefix:z", (B, T, L), 7)[:, t0 + 1:] * 3.0
    h2[t0 + 1:] = R.gen_normal("la_taps:prefix:h", (T, B, H), 7)[t0 + 1:]
    vg = valid.to(dev)
    a = F.local_attention(z.to(dev), h.to(dev), vg, over="taps")
    b = F.local_attention(z2.to(dev), h2.to(dev), vg, over="taps")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a[:, :t0 + 1], b[:, :t0 + 1])
    if t0 + 1 < T:                                           # t0 = T - 1: nothing lies behind it, the whole run repeats
        assert not torch.equal(a[:, t0 + 1:], b[:, t0 + 1:])
        ta = F.local_attention(z.to(dev), h.to(dev), vg)
        tb = F.local_attention(z2.to(dev), h2.to(dev), vg)
        assert not torch.equal(ta[:, :t0 + 1], tb[:, :t0 + 1])
    torch.cuda.synchronize()
