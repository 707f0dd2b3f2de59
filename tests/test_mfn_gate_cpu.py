"""CPU: the reference of the MFN gate's training path (tests/mfn_stream_ref.py lstm_states / gate_from_states / batch_composition under
autograd, with the dropout multipliers and the window mask) against the exact function (oracle.mfn_gate, values and every gradient),
against the stepped walk, its two entries against each other, and the floor under the bounds of tests/test_gpu_bf16_mfn_gate.py: how
far fp32-level noise moves the reference from itself at every case, mode and entry of that file."""
import time

import numpy as np
import pytest
import torch

import bf16_ref as E
import mfn_stream_ref as S
import oracle
import test_gpu_bf16_mfn_gate as G
from gpu_harness import ls_scale, measures, seq_max

EXACT_CASES = [c for c in G.CASES if c["id"] in ("emo_T2_B1", "aco+emo_T3_B5", "lin+emo+aco+ima_T5_B3")]
EXACT_IDS = [c["id"] for c in EXACT_CASES]


def _close(tag, got, want, tol):
    err = float(np.abs(got - want).max()) if want.size else 0.0
    scale = max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    print("%-60s max abs %.2e" % (tag, err))
    assert got.shape == want.shape and np.isfinite(got).all() and err <= tol * scale, (tag, err)


def _oracle_module(c, gd, od, masked):
    pd = {k: v.double().requires_grad_() for k, v in G.params32(c).items()}
    x, mask, g = G.module_inputs(c)
    xd = {m: v.double().requires_grad_() for m, v in x.items()}
    y = oracle.mfn_gate(pd, "", xd, c["mods"], gamma_drop=None if gd is None else (gd[..., :64], gd[..., 64:]), out_drop=od)
    if masked:
        y = y * mask.double()
    y.backward(g.double())
    out = {"out": y.detach().numpy()}
    out.update({"dx:" + m: xd[m].grad.numpy() for m in c["mods"]})
    out.update({"grad:" + n: v.grad.numpy() for n, v in pd.items()})
    return out


@pytest.mark.parametrize("drops,masked", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("c", EXACT_CASES, ids=EXACT_IDS)
def test_the_unrounded_composition_is_the_oracle_with_every_gradient(c, drops, masked):
    """rounding=False: out, dx of every modality, the four tensors of every LSTMCell and the 20 gate tensors equal oracle.mfn_gate's to
    1e-10 (measured at most 4e-15), with and without the dropout multipliers and the mask"""
    gd, od = G.synthetic_drops(c) if drops else (None, None)
    got = G.ref_module(c, gd, od, masked, rounding=False)
    want = _oracle_module(c, gd, od, masked)
    assert sorted(got) == sorted(want) and len([n for n in got if n.startswith("grad:")]) == 4 * len(c["mods"]) + 20
    for n in want:
        _close("exact %s drops %d mask %d %s" % (c["id"], drops, masked, n), got[n], want[n], 1e-10)
    if drops:
        plain = G.ref_module(c, None, None, masked, rounding=False)
        assert measures(plain["out"], got["out"])[0] > 1e-2                  # the multipliers are in the function


@pytest.mark.parametrize("c", EXACT_CASES, ids=EXACT_IDS)
def test_the_rounded_composition_is_the_stepped_walk(c):
    """rounding=True, now through the autograd-capable pieces and with the mask: the values equal mfn_stream_ref.mfn_gate to 1e-12"""
    pd = {k: v.double() for k, v in G.params32(c).items()}
    x, mask, _ = G.module_inputs(c)
    xd = {m: v.double() for m, v in x.items()}
    for mk in (None, mask.double()):
        got = S.batch_composition(pd, "", xd, c["mods"], mask=mk)
        want = S.mfn_gate(pd, "", xd, c["mods"], mk)
        _close("stepped %s mask %d" % (c["id"], mk is not None), got.numpy(), want.numpy(), 1e-12)
        assert not got.requires_grad


@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("c", EXACT_CASES, ids=EXACT_IDS)
def test_the_two_entries_agree(c, rounding):
    """gate_from_states fed the full entry's hs and cs as leaves: the same output, and its d_hs / d_cs are the gradients the full entry
    passes into the scans' outputs; the 20 gate gradients agree too"""
    gd, od = G.synthetic_drops(c)
    pd = {k: v.double().requires_grad_() for k, v in G.params32(c).items()}
    x, mask, g = G.module_inputs(c)
    xd = {m: v.double() for m, v in x.items()}
    st = {}
    y = S.batch_composition(pd, "", xd, c["mods"], rounding=rounding, gamma_drop=gd, out_drop=od, mask=mask.double(), states=st)
    for t in st["hs"] + st["cs"]:
        t.retain_grad()
    y.backward(g.double())
    p2 = {k: v.detach().clone().requires_grad_() for k, v in pd.items()}
    hs = [t.detach().clone().requires_grad_() for t in st["hs"]]
    cs = [t.detach().clone().requires_grad_() for t in st["cs"]]
    y2 = S.gate_from_states(p2, "", hs, cs, gd, od, rounding=rounding)
    y2.backward((g.double() * mask.double()).permute(1, 0, 2))               # the mask and the permutation sit outside this entry
    tag = "entries %s rounding %d " % (c["id"], rounding)
    _close(tag + "out", (y2.detach().permute(1, 0, 2) * mask.double()).numpy(), y.detach().numpy(), 1e-12)
    for i in range(len(hs)):
        _close(tag + "d_hs:%d" % i, hs[i].grad.numpy(), st["hs"][i].grad.numpy(), 1e-12)
        _close(tag + "d_cs:%d" % i, cs[i].grad.numpy(), st["cs"][i].grad.numpy(), 1e-12)
    for n in G.GATE_NAMES:
        _close(tag + n, p2[n].grad.numpy(), pd[n].grad.numpy(), 1e-12)


def test_gpu_cases_reach_what_they_are_labelled_for():
    """the table of the GPU file: A < 64 at one modality, the block offsets, the scan families, the T tiers"""
    H = {c["id"]: G.hidden_sizes(c) for c in G.CASES}
    assert 2 * sum(H["emo_T1_B1"]) == 32 and H["lin+aco+ima_T7_B33"] == [88, 48, 88] and 2 * sum(H["lin+emo+aco+ima_T5_B3"]) == 480
    assert [G.SC.mfn_family(c["B"]) for c in G.CASES] == ["sw1", "sw1", "sw1", "sw1", "sw1", "sw2", "sw1"]
    assert [G.tier(c) for c in G.CASES] == ["exact", "exact", "short", "short", "short", "short", "long"]
    for c in G.CASES:
        x, mask, g = G.module_inputs(c)
        assert mask.shape == (c["B"], c["T"], 1) and mask[-1].sum() == 1 and mask[:, 0].all() and (c["B"] == 1 or mask[0].all())
    assert len(G.GATE_NAMES) == 20 and set(G.BOUNDS) == {"exact", "short", "long"}


def test_gpu_bounds_sit_under_the_old_ones():
    """no bound above test_gpu_models' 2e-2 (out) / 9e-2 (gradients); at T <= 7 every gradient bound at least 10x under 9e-2; every
    tensor of every tier has a per-row bound"""
    from gpu_harness import OUT_RTOL, RELU_GRAD_RTOL
    for tr, table in G.BOUNDS.items():
        for k, bd in table.items():
            n = 3 if k in G.STATE_KEYS else 2                                # the scale of a matrix is no rel-L2
            assert all(b is not None for b in bd), (tr, k)
            top = OUT_RTOL if k == "out" else RELU_GRAD_RTOL if tr == "long" else RELU_GRAD_RTOL / 10
            assert max(bd[:n]) <= top * (1 + 1e-12), (tr, k, bd)
            if k in G.MATRIX_KEYS:
                assert bd[2] <= 1e-3, (tr, k, bd)                            # a term scaled by 1.01 moves the scale by 1e-2 of its share


# ------------------------------------------------------------------------------------------------ the floor
def test_jitter_of_computed_values_only():
    """computed_only: an element that is an fp32 number (given data, a copy, a zero) rounds as without noise; every other element is
    perturbed as under the plain jitter, so values next to a rounding boundary tip"""
    given = torch.randn(4096, generator=torch.Generator().manual_seed(3)).double()                    # fp32 numbers
    edge = (1 + 2.0 ** -8) * (1 + 1e-9 * torch.randn(4096, generator=torch.Generator().manual_seed(4), dtype=torch.float64))
    mixed = torch.cat([given, edge])                                       # the second half sits on a bf16 rounding boundary
    with E.jitter(6e-8, 1, computed_only=True):
        got = E.bf16(mixed)
    assert torch.equal(got[:4096], E.bf16(given)) and not torch.equal(got[4096:], E.bf16(edge))
    with E.jitter(6e-8, 1):
        plain = E.bf16(mixed)
    assert torch.equal(plain[4096:], got[4096:])                           # the same noise on the computed half
    assert E._JITTER is None and not E._JITTER_COMPUTED_ONLY


def _floor(a, b, batch_major_out):
    """{tensor: (rel-L2, per row, third)} of the reference under noise (b) against itself (a), measured as
    test_gpu_bf16_mfn_gate.compare measures: third is the per-sequence maximum of a per-window tensor, the least-squares scale of a
    weight matrix, None of a vector"""
    out = {}
    for n in a:
        r, g = a[n], b[n]
        if not r.any():
            continue
        grp = G.group_of(n)
        if grp in G.STATE_KEYS:
            if n == "out" and batch_major_out:
                r, g = np.swapaxes(r, 0, 1), np.swapaxes(g, 0, 1)
            out[n] = measures(g, r) + (seq_max(g, r),)
            if grp == "d_cs":
                T = r.shape[0]
                for lab, sl in (("t0", slice(0, 1)), ("mid", slice(1, T - 1)), ("last", slice(T - 1, T))):
                    if r[sl].size and (lab != "last" or T > 1):
                        out["%s@%s" % (n, lab)] = measures(g[sl], r[sl]) + (None,)
        elif r.ndim == 2:
            out[n] = measures(g, r) + (abs(ls_scale(g, r)),)
        else:
            out[n] = measures(g.ravel(), r.ravel()) + (None,)
    return out


def test_mfn_gate_jitter_floor():
    """The floor of the bounds in test_gpu_bf16_mfn_gate.py: how far fp32-level noise (half an fp32 ulp before every bf16 rounding,
    bf16_ref.jitter(6e-8, computed_only=True): weights, inputs and their copies round the same everywhere) moves the reference from
    itself, for every case, mode and entry of that file, per tensor as rel-L2, per row
    and per sequence (per weight matrix: its least-squares scale).  No bound there may lie below it, and a per-row bound may be missing
    (None) only where this floor exceeds 0.1 per row."""
    t0 = time.time()
    worst = {}                                                   # (tier, entry of BOUNDS) -> [rel, row, third]
    for c in G.CASES:
        gd, od = G.synthetic_drops(c)
        for mode in G.MODES:
            d = (gd, od) if mode == "train" else (None, None)
            runs = [(False, lambda: G.ref_gate(c, *d)), (True, lambda: G.ref_module(c, *d))]
            if (c, "train_nomask") in G.MODULE_MODES and mode == "train":
                runs.append((True, lambda: G.ref_module(c, *d, masked=False)))
            for bm, ref in runs:
                a = ref()
                with E.jitter(6e-8, 1, computed_only=True):
                    b = ref()
                for n, m in _floor(a, b, bm).items():
                    grp = "d_cs_t" if "@" in n else G.group_of(n)
                    w = worst.setdefault((G.tier(c), grp), [0.0, 0.0, 0.0])
                    for i, v in enumerate(m):
                        w[i] = max(w[i], v or 0.0)
    assert sorted(worst) == sorted((t, k) for t in G.BOUNDS for k in G.STATE_KEYS + G.VECTOR_KEYS + G.MATRIX_KEYS)
    failures = []
    for (tr, grp), w in sorted(worst.items()):
        print("jitter floor|%s|%s| %.2e %.2e %.2e" % (tr, grp, *w))
        bd = G.BOUNDS[tr][grp]
        assert set(G.BOUNDS[tr]) == set(G.STATE_KEYS + G.VECTOR_KEYS + G.MATRIX_KEYS) and len(bd) == (2 if grp in G.VECTOR_KEYS else 3)
        for i, what in enumerate(("rel-L2", "per-row", "per-sequence" if grp in G.STATE_KEYS else "scale")[:len(bd)]):
            if bd[i] is None:
                if i != 1 or w[1] <= 0.1:
                    failures.append("%s %s: no %s bound, and the floor is %.2e" % (tr, grp, what, w[i]))
            elif w[i] > bd[i]:
                failures.append("%s %s: %s bound %.1e below the floor %.2e" % (tr, grp, what, bd[i], w[i]))
    print("%.1f s" % (time.time() - t0))
    assert not failures, "\n".join(failures)
