"""GPU: the attention probabilities materialised on request (csrc/attn_probs.h, functional.attn_probs, MultiHeadedAttention.keep_attn,
multiTransformer.keep_attention / attention_with_map) — the reference's p_attn / self.attn (transformer/MFT/multiTransformer.py:22-34,59).

Shapes (B, T, d, h, lengths) are the smallest that reach each code path of the kernel: a single element; d_k 10 padded with a
one-element ragged tile and T % 4 != 0; full tiles only; d_k 32; d_k 64; d_k 48; ten key tiles with several query tiles per workgroup.
Inputs as in test_gpu_parity.test_sdpa: R.gen_normal, q * 2.

Bounds.  The context formed from the map is held to OUT_RTOL like test_sdpa's (bf16 operands against an fp64 reference).  The map's own
two bounds (against the fp64 oracle, which carries the whole bf16 rounding of Q' and K, and against the same softmax on operands rounded
as the kernel rounds them, where only fp32 accumulation order and the hardware exp2 / reciprocal remain) cannot be derived: they are
4 x the worst value measured on an MI355X over the shapes below, the margin being for exp2 and for the row-sum order differing between
tile counts.  (The first of the two is the number format's: the bf16-rounded softmax computed in fp64 on the CPU lies as far from the oracle.)
"""
import math

import numpy as np
import pytest
import torch

import bf16_ref as E
import oracle
import recipe as R
from gpu_harness import OUT_RTOL, _report, dev, device_kernel_names, measures, mta, seeded_encoder  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 16, 1, [1]), (3, 33, 40, 4, [33, 32, 1]), (2, 64, 128, 8, [64, 7]), (2, 65, 256, 8, [65, 40]), (1, 70, 256, 4, [70]),
         (1, 33, 192, 4, [20]), (1, 300, 64, 4, [300])]
IDS = ["T%d_d%d_h%d" % (c[1], c[2], c[3]) for c in CASES]

# (rel-L2, per-row maximum) of the map: 4 x the worst measured over CASES
MAP_ORACLE = (1.9e-2, 1.1e-1)        # 4.82e-3 / 2.69e-2 (T 300, d_k 16): against oracle.scaled_dot_attention's p_attn
MAP_BF16 = (5.6e-7, 2.5e-6)          # 1.39e-7 (T 70, d_k 64) / 6.31e-7 (T 300): against the softmax of operands rounded as the kernel rounds them
P_DROP, SEED = 0.1, 20240917         # one python-int seed for every train-mode call

_CACHE = {}


def _split(z, h):
    B, T, d = z.shape
    return z.reshape(B, T, h, d // h).permute(0, 2, 1, 3)


def _case(c, dev):
    """inputs, references and the kernel's maps (eval and train) of one case, computed once"""
    key = c[:4]
    if key in _CACHE:
        return _CACHE[key]
    B, T, d, h, lengths = c
    tag = "probs%d_%d_%d" % (T, d, h)
    q, k, v = (R.gen_normal(tag + n, (B, T, d), 7) for n in "qkv")
    q = q * 2.0                                                     # spread the scores
    mask = R.prefix_mask(list(lengths), T)
    dk = d // h
    qd, kd, vd = (_split(t.double(), h) for t in (q, k, v))
    ctx_ref, map_ref = oracle.scaled_dot_attention(qd, kd, vd, mask.double().unsqueeze(1))
    # Q' and K as the kernel rounds them: fp32 product with the fp32 constant log2(e)/sqrt(d_k), then bf16; a blanked row is Q' = 0
    qs = torch.tensor(E.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(dk), dtype=torch.float32))
    Qp = E.bf16((q * qs * (mask != 0).float()).double())
    Kb = E.bf16(k.double())
    map_bf = torch.softmax((_split(Qp, h) @ _split(Kb, h).transpose(-2, -1)) * E.LN2, dim=-1)
    F = mta().functional
    qg, kg, vg, mg = q.to(dev), k.to(dev), v.to(dev), mask.to(dev)
    out = {"B": B, "T": T, "d": d, "h": h, "lengths": lengths, "q": qg, "k": kg, "v": vg, "mask": mg, "vb": _split(E.bf16(v.double()), h),
           "ctx_ref": ctx_ref, "map_ref": map_ref, "map_bf": map_bf,
           "eval": F.attn_probs(qg, kg, mg, h).cpu(),
           "train": F.attn_probs(qg, kg, mg, h, dropout_p=P_DROP, seed=SEED).cpu()}
    _CACHE[key] = out
    return out


def _merge(z):
    B, h, T, dk = z.shape
    return z.permute(0, 2, 1, 3).reshape(B, T, h * dk)


def _real_rows(c):
    """(B, 1, T, 1) bool: query rows the mask does not blank"""
    return (c["mask"].cpu() != 0).reshape(c["B"], 1, c["T"], 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_map_against_the_oracle_and_the_bf16_faithful_reference(dev, case):
    c = _case(case, dev)
    P = c["eval"]
    assert P.shape == (c["B"], c["h"], c["T"], c["T"]) and P.dtype == torch.float32
    tag = "probs T%d d%d h%d" % (c["T"], c["d"], c["h"])
    assert _report(tag + " P@V", _merge(P.double() @ _split(c["v"].cpu().double(), c["h"])), _merge(c["ctx_ref"])) < OUT_RTOL
    for name, ref, (rel_b, row_b) in (("oracle", c["map_ref"], MAP_ORACLE), ("bf16", c["map_bf"], MAP_BF16)):
        rel, row = measures(P.numpy(), ref.numpy())
        print("%-40s rel-L2 %.3e  row-max %.3e" % (tag + " map vs " + name, rel, row))
        assert rel <= rel_b and row <= row_b, (name, rel, row)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_sum_to_one(dev, case):
    """one rounding per element (2^-24 relative each, the elements sum to 1) plus the kernel's fp32 row sum (T additions)"""
    c = _case(case, dev)
    err = (c["eval"].double().sum(dim=-1) - 1.0).abs().max().item()
    print("probs T%d row-sum error %.3e (bound %.3e)" % (c["T"], err, 2 * (c["T"] + 1) * 2.0 ** -24))
    assert err <= 2 * (c["T"] + 1) * 2.0 ** -24


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_blanked_rows_are_exactly_uniform(dev, case):
    c = _case(case, dev)
    P, T = c["eval"], c["T"]
    assert torch.isfinite(P).all() and (P >= 0).all()
    assert torch.isfinite(c["train"]).all() and (c["train"] >= 0).all()
    uniform = torch.full((T,), 1 / T, dtype=torch.float32)
    blanked = 0
    for b, n in enumerate(c["lengths"]):
        for t in range(n, T):
            for head in range(c["h"]):
                assert torch.equal(P[b, head, t], uniform), (b, head, t)
            blanked += 1
    assert blanked == sum(T - n for n in c["lengths"])


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["eval", "train"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_agrees_with_the_forward_kernel(dev, case, p):
    """map @ bf16(v) against sdpa's context for the same (q, k, v, mask, p, seed): sdpa rounds each probability to bf16 (2^-9) before
    the value product, the rest is fp32; a wrong keep decision or tile offset shows as >= 1e-1"""
    c = _case(case, dev)
    B, T, h = c["B"], c["T"], c["h"]
    F = mta().functional
    P = c["train" if p else "eval"]
    ctx = F.sdpa(c["q"], c["k"], c["v"], c["mask"], h, dropout_p=p, seed=SEED if p else 0).cpu()
    tag = "probs-vs-sdpa T%d d%d h%d p%g" % (T, c["d"], h, p)
    assert _report(tag, _merge(P.double() @ c["vb"]), ctx) <= 2.0 ** -7
    if not p:
        return
    # the keep decisions are the generator's (stream 0), element for element
    Tp = -(-T // 32) * 32
    keep, scale = F.dropout_mask(p, SEED, 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
    keep = keep.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu() != 0
    assert (c["eval"] > 0).all()                                    # no probability underflows at these shapes: a zero is a drop
    assert torch.equal(P != 0, keep)
    # kept elements: the eval map / (1 - p), with p as the 12-bit attention stream resolves it (csrc/common.h make_drop)
    pq = round(p * 4096) / 4096
    assert abs(scale - 1 / (1 - pq)) < 1e-6
    rel, row = measures((P.double() * keep).numpy(), (c["eval"].double() * keep / (1 - pq)).numpy())
    print("%-40s rel-L2 %.3e  row-max %.3e" % (tag + " kept", rel, row))
    assert rel <= MAP_BF16[0] and row <= MAP_BF16[1]
    real = _real_rows(c).expand(B, h, T, T)
    n = int(real.sum())
    frac = float((P[real] == 0).double().mean())
    assert abs(frac - p) <= 4 * math.sqrt(p * (1 - p) / n) + abs(pq - p), (frac, n)


def test_two_runs_are_bit_identical(dev):
    c = _case(CASES[6], dev)
    F = mta().functional
    again = F.attn_probs(c["q"], c["k"], c["mask"], c["h"], dropout_p=P_DROP, seed=SEED).cpu()
    assert torch.equal(again, c["train"])
    other = F.attn_probs(c["q"], c["k"], c["mask"], c["h"], dropout_p=P_DROP, seed=SEED + 1).cpu()
    assert not torch.equal(other != 0, again != 0)                  # the seed is really used


def _mha(dev):
    MT = mta().multiTransformer
    mha = MT.MultiHeadedAttention(8, 128)
    mha.load_state_dict(R.gen_params(R.shapes_of(mha.state_dict()), R.SEED))
    return mha.to(dev).eval()


def test_module_flag_changes_nothing_else(dev):
    MT = mta().multiTransformer
    mha = _mha(dev)
    B, T = 3, 50
    mask = R.prefix_mask([50, 31, 6], T).to(dev)
    x0 = R.gen_normal("probs_mha:x", (B, T, 128), 3).to(dev)
    g = R.gen_normal("probs_mha:g", (B, T, 128), 3).to(dev)

    def run():
        x = x0.clone().requires_grad_()
        for p in mha.parameters():
            p.grad = None
        y = mha(x, x, x, mask)
        (y * g).sum().backward()
        return y.detach(), [x.grad.clone()] + [p.grad.clone() for p in mha.parameters()]

    (y_off, g_off), names = device_kernel_names(run, warm=True)
    assert mha.attn is None
    if names is not None:
        assert not [n for n in names if "attn_probs" in n]          # flag off: the new kernel is not launched
    assert MT.keep_attention(mha) == {"": mha}
    (y_on, g_on), names = device_kernel_names(run)
    if names is not None:
        assert [n for n in names if "attn_probs" in n]
    assert torch.equal(y_on, y_off)
    assert mha.attn.shape == (B, 8, T, T) and mha.attn.requires_grad is False and mha.attn.grad_fn is None
    assert len(g_on) == len(g_off) and all(torch.equal(a, b) for a, b in zip(g_on, g_off))
    MT.keep_attention(mha, False)
    mha(x0, x0, x0, mask)
    assert mha.attn is None


def test_module_train_mode_map_matches_its_context(dev):
    """train mode: the map kept by the module is the post-dropout one its own sdpa call used (same seed): map @ bf16(v) W_o^T + b_o = y"""
    MT = mta().multiTransformer
    F = mta().functional
    mha = _mha(dev).train()
    MT.keep_attention(mha)
    B, T = 2, 70
    mask = R.prefix_mask([70, 33], T).to(dev)
    x = R.gen_normal("probs_mha_tr:x", (B, T, 128), 3).to(dev)
    with torch.no_grad():
        y = mha(x, x, x, mask)
        P = mha.attn
        assert float((P == 0).float().mean()) > 0.05                 # dropout really happened
        v = F.linear(x, mha.linears[2].weight, mha.linears[2].bias)
        ctx = _merge(P.cpu().double() @ _split(E.bf16(v.cpu().double()), 8))
        y2 = F.linear(ctx.float().to(dev), mha.linears[3].weight, mha.linears[3].bias)
    assert _report("probs mha train y", y2.cpu(), y.cpu()) <= OUT_RTOL   # ctx and W_o are rounded to bf16 by the projection: the bf16-design tolerance


def test_encoder_keeps_a_map_per_layer(dev):
    MT = mta().multiTransformer
    F = mta().functional
    enc, _ = seeded_encoder(128, 8, 2, dev, 23)
    B, T = 2, 40
    x = R.gen_normal("probs_enc:x", (B, T, 128), 23).to(dev)
    mask = R.prefix_mask([40, 13], T).to(dev)
    with torch.no_grad():
        assert enc._fusable()
        y_fused = enc(x, mask)
        assert all(l.self_attn.attn is None for l in enc.layers)
        found = MT.keep_attention(enc)
        assert list(found) == ["layers.0.self_attn", "layers.1.self_attn"] and not enc._fusable()
        y = enc(x, mask)
        for l in enc.layers:
            assert l.self_attn.attn.shape == (B, 8, T, T)
        assert _report("probs enc out", y.cpu(), y_fused.cpu()) < OUT_RTOL
        l0 = enc.layers[0]
        xn = l0.sublayer[0].norm(x)
        q, k = (F.linear(xn, lin.weight, lin.bias) for lin in l0.self_attn.linears[:2])
        assert torch.equal(l0.self_attn.attn, F.attn_probs(q, k, mask, 8))
        assert not torch.equal(enc.layers[1].self_attn.attn, l0.self_attn.attn)
        MT.keep_attention(enc, False)
        assert enc._fusable()
        assert torch.equal(enc(x, mask), y_fused)
        assert all(l.self_attn.attn is None for l in enc.layers)


def test_attention_with_map(dev):
    MT = mta().multiTransformer
    F = mta().functional
    c = _case(CASES[1], dev)
    B, T, h = c["B"], c["T"], c["h"]
    qh, kh, vh = (_split(c[n], h) for n in "qkv")
    ctx0, none = MT.attention(qh, kh, vh, c["mask"].unsqueeze(1), None)
    assert none is None
    ctx, P = MT.attention_with_map(qh, kh, vh, c["mask"].unsqueeze(1), None)
    assert torch.equal(ctx, ctx0)
    assert P.requires_grad is False and torch.equal(P, F.attn_probs(c["q"], c["k"], c["mask"], h)) and torch.equal(P.cpu(), c["eval"])
    # train mode: one seed serves both kernels, so the returned map reproduces the returned context
    drop = torch.nn.Dropout(P_DROP).train()
    ctx, P = MT.attention_with_map(qh, kh, vh, c["mask"].unsqueeze(1), drop)
    assert float((P == 0).float().mean()) > 0.05
    assert _report("attention_with_map train", (P.cpu().double() @ c["vb"]), ctx.cpu()) <= 2.0 ** -7


def test_refusals_before_any_launch(dev):
    F = mta().functional
    q128 = torch.zeros(1, 8, 128, device=dev)
    qlong = torch.zeros(1, 4097, 16, device=dev)
    q = torch.zeros(2, 8, 16, device=dev)
    dense = torch.ones(2, 1, 8, 8, device=dev)
    odd = torch.zeros(2, 9, 16, device=dev)
    qcpu = torch.zeros(2, 8, 16)
    torch.cuda.synchronize()

    def attempts():
        with pytest.raises(RuntimeError, match="d_k = 128 > 64"):
            F.attn_probs(q128, q128, None, 1)
        with pytest.raises(RuntimeError, match="4096"):
            F.attn_probs(qlong, qlong, None, 1)
        with pytest.raises(RuntimeError, match="not divisible"):
            F.attn_probs(q, q, None, 3)
        with pytest.raises(NotImplementedError, match="query-row mask"):
            F.attn_probs(q, q, dense, 2)
        with pytest.raises(NotImplementedError, match="share the shape"):
            F.attn_probs(q, odd, None, 2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.attn_probs(qcpu, qcpu, None, 2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.attn_probs(q, q, torch.ones(2, 8, 1), 2)

    _, names = device_kernel_names(attempts)
    assert not names
