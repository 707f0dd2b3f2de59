"""The kernels on peaked, saturated and degenerate VALUES (tests/value_regimes.py): every other numeric test draws unit-scale inputs.

What each regime pins (tests/test_value_regimes_cpu.py holds, on the references alone, that it is reached at every shape used here):
  * attention `cold` / `hot`: the stored -L beyond +-140, so 2^(S' - L) of a key that does not exist (a zero fragment behind T, a key
    behind a length, a key above the diagonal) is inf: such a pair must be zeroed by a select, a multiplier gives inf x 0 = NaN;
  * `step`: the masked keys of the boundary tile (key_lengths) or of the diagonal tile (causal) beat every visible key by > 2^140;
  * `rising` / `falling`: the lazily rescaled running maximum moves at every key tile / never, with whole tiles underflowing to P = 0;
  * `peaked`: nearly one-hot rows;
  * LayerNorm `tiny` / `sub_eps`: eps is added to the standard deviation, not inside the root (0.98 / 0.74 rel-L2 apart there, 5e-7 at
    unit spread), in all five bodies: the stand-alone kernel, the generic and the d = 128 chains, the folded final norm, the stream
    step; `offset` / `huge`: the centring and the backward's sigma = 1 / rstd - eps; `one_constant_row`: sigma = 0;
  * scans `long_memory`: the gradient enters at the last step only and reaches step 0 undamped, so dgx / dapre of every earlier step IS
    the backward carry (across prefetch depths, the four-CU exchange, chunk boundaries); measured per time step as well;
  * `overflow`: gate pre-activations of +-200 through sigmoid_f / tanh_f and the affine map's tanh / sigmoid epilogues.

Bounds: those of the tier that already tests the same tensor, imported.  A bound is wider only where test_value_regimes_cpu.py holds a
yardstick for it that involves no kernel (the reference in fp32, or against itself under jitter), and is then 4x that yardstick; the
yardstick, the bound and the value measured on the MI355X stand beside each such constant there.

Every GPU run happens in a child process (gpu_harness.run_child -> child_main): the attention and stack switches are read once per
process, and a child that dies takes no other test with it.
"""
import json

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
import stream_ref as S
import test_value_regimes_cpu as VC
import value_regimes as V
from conftest import rel_l2
from gpu_harness import LIN_REL, check, check_scan, ls_scale, run_child, tmp_dir  # noqa: F401 (tmp_dir: a fixture)
from test_gpu_bf16_faithful import (ENC_GRAD, ENC_OUT, ENC_OUT_ROW, ENC_RELU_GRAD, ENC_ROW, ENC_W_SCALE, SDPA_GRAD, SDPA_GRAD_ROW, SDPA_OUT,
                                    SDPA_OUT_ROW)
from test_gpu_bf16_scans import LSTM_D0, LSTM_DGX, LSTM_DW, LSTM_OUT, LSTM_W_SCALE, MFN_LONG, MFN_SHORT, MFN_W_SCALE
from test_gpu_arlstm import _cpu_fp32, _fp64
from test_gpu_bf16_stack_fb import FB_KEYS, P_INIT, _dev_leaves, _np, bound_of, compare, fb_ref, stack_ref
from test_gpu_lstm_baselines import LA_RTOL, _local_attention_fp64

pytestmark = pytest.mark.gpu

P_TRAIN = 0.1
MODES = [0.0, P_TRAIN]
MODE_IDS = ["eval", "p0.1"]
# the stand-alone LayerNorm's bounds are test_gpu_parity.test_layernorm_shapes' (y: 3e-5 absolute at unit scale; gradients 3e-4 rel-L2)
LN_Y, LN_GRAD = 3e-5, 3e-4
SOFTMAX_REL = 1e-5          # fp32 softmax of logits up to ~250: an entry that matters lies within 17 of the maximum, so its exponent
#                             carries 2 x 17 x 1.44 x 2^-24 = 3e-6 relative; the bound of the local attention (LA_RTOL), which is this softmax

SDPA_CASES = V.sdpa_cases()
PROBS_CASES = V.probs_cases()
TWO_KERNEL = [c for c in SDPA_CASES if c[0] == "plain" and c[2] == 290 and c[3] == 16]      # the one-kernel backward's shapes
ENC_TINY = [(40, 4), (128, 8)]                                  # (d, h): the generic chains, the fixed shapes; N = 2, B = 2, T = 33
ENC_N, ENC_B, ENC_T = 2, 2, 33
STREAM = (128, 8, 2, 8)                                         # d, h, N, T
LIN_SHAPE = (33, 43, 129)
LA_SHAPE = (2, 40, 32, 4)                                       # B, T, H, L
SM_SHAPE = (7, 200)


def _seed(case, p):
    return 1000 + case[2] + case[3] + (7 if p else 0)


# ------------------------------------------------------------------------------------------------ inputs shared with the child
def enc_params(d, n, shrink):
    """the recipe's parameters; shrink: every layer's output projection and second FFN projection (weight and bias) scaled by 1e-6, so
    that the residual stream keeps the input's spread and all five LayerNorms of the stack see it"""
    p32 = R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), 17)
    if shrink:
        for k in p32:
            if ".self_attn.linears.3." in k or ".feed_forward.w_2." in k:
                p32[k] = p32[k] * 1e-6
    return p32


def enc_inputs(d, regime):
    x, _, _, g = V.layer_norm_input(regime, ENC_B * ENC_T, d, tag="enc")
    return x.reshape(ENC_B, ENC_T, d), g.reshape(ENC_B, ENC_T, d), R.prefix_mask([ENC_T, 22], ENC_T)


def lin_inputs(act):
    M, K, N = LIN_SHAPE
    x = R.gen_normal("vr:lin:x", (M, K), V.SEED)
    W = R.gen_normal("vr:lin:w", (N, K), V.SEED) / np.sqrt(K)
    b = 0.1 * R.gen_normal("vr:lin:b", (N,), V.SEED)
    n = torch.arange(N)
    b = b + 250.0 * (n % 6 == 0).float() - 250.0 * (n % 6 == 3).float()      # a third of the columns beyond +-200
    return x, W, b, R.gen_normal("vr:lin:g", (M, N), V.SEED)


def la_inputs():
    B, T, H, L = LA_SHAPE
    z = 60.0 * R.gen_normal("vr:la:z", (B, T, L), V.SEED)
    h = torch.tanh(R.gen_normal("vr:la:h", (T, B, H), V.SEED))
    valid = R.prefix_mask([T, T - T // 3], T).reshape(B, T)
    return z, h, valid, R.gen_normal("vr:la:g", (B, T, H), V.SEED)


def sm_inputs():
    M, A = SM_SHAPE
    return tuple(R.gen_normal("vr:sm:" + n, (M, A), V.SEED) * s for n, s in (("l", 60.0), ("v", 1.0), ("g", 1.0)))


SCAN_RUNS = [("long_memory", T) for T in V.LONG_T] + [("overflow", V.OVERFLOW_T)]


# ------------------------------------------------------------------------------------------------ child process
def _sdpa_section(F, dev, cases, out):
    for case in cases:
        sel, regime, T, dk, j0 = case
        q, k, v, g, mask, kl = V.sdpa_inputs(case)
        h, B = V.ATTN_H, V.ATTN_B
        klg = None if kl is None else torch.tensor(kl, dtype=torch.int32, device=dev)
        for p in MODES:
            key = "sdpa:%s:p%g:" % (V.case_id(case), p)
            leaves = [t.to(dev).requires_grad_() for t in (q, k, v)]
            y = F.sdpa(*leaves, mask.to(dev), h, dropout_p=p, seed=_seed(case, p), key_lengths=klg, causal=sel == "causal")
            y.backward(g.to(dev))
            for n, t in zip(("y", "dq", "dk", "dv"), [y.detach()] + [t.grad for t in leaves]):
                out[key + n] = t.cpu().numpy()
            if p > 0:
                Tp = -(-T // 32) * 32
                keep, sc = F.dropout_mask(p, _seed(case, p), 0, B * h * Tp * Tp, dev, attn_Tp=Tp)
                out[key + "keep"] = keep.reshape(B, h, Tp, Tp)[:, :, :T, :T].cpu().numpy()
                out[key + "scale"] = np.array(sc)


def _enc_section(F, dev, out, rows):
    for d, h, regime in rows:
        p32 = enc_params(d, ENC_N, regime == "tiny")
        x, g, mask = enc_inputs(d, regime)
        flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
        xg = x.to(dev).requires_grad_()
        y = F.encoder_stack(xg, mask.to(dev), flat, h, R.D_FF, ENC_N)
        y.backward(g.to(dev))
        key = "enc:d%d:%s:" % (d, regime)
        out[key + "y"], out[key + "dx"], out[key + "dflat"] = y.detach().cpu().numpy(), xg.grad.cpu().numpy(), flat.grad.cpu().numpy()


def child_main(kind, out_path, payload_json):
    """kind "main": everything under the default switches; "sdpa": the attention cases the payload lists by index; "enc": the tiny stack"""
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import functional as F
    dev = torch.device("cuda:0")
    out = {}
    if kind == "sdpa":
        _sdpa_section(F, dev, [SDPA_CASES[i] for i in json.loads(payload_json)], out)
    elif kind == "enc":
        _enc_section(F, dev, out, [(d, h, "tiny") for d, h in ENC_TINY])
    else:
        _sdpa_section(F, dev, SDPA_CASES, out)
        for case in PROBS_CASES:
            q, k, v, g, mask, kl = V.sdpa_inputs(case)
            klg = None if kl is None else torch.tensor(kl, dtype=torch.int32, device=dev)
            out["probs:" + V.case_id(case)] = F.attn_probs(q.to(dev), k.to(dev), mask.to(dev), V.ATTN_H, key_lengths=klg,
                                                           causal=case[0] == "causal").cpu().numpy()
        _enc_section(F, dev, out, [(d, h, "tiny") for d, h in ENC_TINY] + [(128, 8, "offset")])
        # ---- the stand-alone LayerNorm; one_constant_row also with that row ordinary ("plain")
        for M, d in VC.LN_SHAPES:
            for regime in V.LN_REGIMES + ("plain",):
                if regime == "plain":
                    x, a, b, g = V.layer_norm_input("one_constant_row", M, d)
                    x[1] = R.gen_normal("vr:ln:row1", (d,), V.SEED)
                else:
                    x, a, b, g = V.layer_norm_input(regime, M, d)
                lv = [t.to(dev).requires_grad_() for t in (x, a, b)]
                y = F.layer_norm(*lv)
                y.backward(g.to(dev))
                for n, t in zip(("y", "dx", "da", "db"), [y.detach()] + [t.grad for t in lv]):
                    out["ln:%d:%s:%s" % (d, regime, n)] = t.cpu().numpy()
        # ---- the stream step on the tiny input
        d, h, n, T = STREAM
        MT = m.multiTransformer
        enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, R.D_FF, 0.1), 0.1), n)
        enc.load_state_dict(enc_params(d, n, True))
        enc = enc.to(dev).eval()
        MT.causal_attention(enc)
        x = V.layer_norm_input("tiny", 2 * T, d, tag="stream")[0].reshape(2, T, d).to(dev)
        mask = R.prefix_mask([T, 5], T).to(dev)
        s = enc.stream(2, T)
        out["stream:y"] = torch.stack([s.step(x[:, t], mask[:, t]) for t in range(T)], dim=1).cpu().numpy()
        # ---- scans
        for regime, T in SCAN_RUNS:
            for fam, B, H in V.LSTM_FAMILIES:
                gx, W, h0, c0, gh, gc, hi, lo = V.lstm(regime, T, B, H)
                lv = [t.to(dev).requires_grad_() for t in (gx, W, h0, c0)]
                hh, cc = F.lstm_scan(*lv)
                ((hh * gh.to(dev)).sum() + (cc * gc.to(dev)).sum()).backward()
                for n, t in zip(("h", "c", "dgx", "dW", "dh0", "dc0"), [hh.detach(), cc.detach()] + [t.grad for t in lv]):
                    out["lstm:%s:%d:%s:%s" % (regime, T, fam, n)] = t.cpu().numpy()
            for fam, B in V.MFN_FAMILIES:
                apre, chat, Wm, W2, b2, g, hi, lo = V.mfn(regime, T, B)
                lv = [t.to(dev).requires_grad_() for t in (apre, chat, Wm, W2, b2)]
                mem = F.mfn_mem_scan(*lv)
                (mem * g.to(dev)).sum().backward()
                for n, t in zip(("mem", "dapre", "dchat", "dWm", "dW2", "db2"), [mem.detach()] + [t.grad for t in lv]):
                    out["mfn:%s:%d:%s:%s" % (regime, T, fam, n)] = t.cpu().numpy()
            inp, w, _ = V.stack_inputs(regime, T)
            lv = _dev_leaves(inp, dev)
            h_top, h_all, c_all = F.lstm_stack_scan(lv["gx0"], lv["P"], lv["bias"], lv["h0"], lv["c0"], return_states=True)
            h_top.backward(w.float().to(dev))
            res = {"h_top": h_top, "h_all": h_all, "c_all": c_all}
            res.update({"d" + k: t.grad for k, t in lv.items()})
            for n, t in res.items():
                out["stack:%s:%d:%s" % (regime, T, n)] = _np(t)
            inp, w, _ = V.fb_inputs(regime, T)
            lv = _dev_leaves(inp, dev)
            outs = F.lstm_fb_scan(*[lv[k] for k in FB_KEYS], p_init=P_INIT, return_states=True)
            outs[0].backward(w.float().to(dev))
            res = dict(zip(("p_all", "h_all", "c_all", "u_all"), outs))
            res.update({"d" + k: t.grad.reshape(inp[k].shape) for k, t in lv.items()})
            for n, t in res.items():
                out["fb:%s:%d:%s" % (regime, T, n)] = _np(t)
        inp = V.ar_inputs()
        c, w = inp["c"].to(dev).requires_grad_(), inp["w"].to(dev).requires_grad_()
        o, p = F.ar_combine(c, w, inp["mask"].to(dev), None, P_INIT, return_p=True)
        o.backward(inp["g"].to(dev))
        for n, t in (("p", p), ("out", o), ("din", c.grad), ("dw", w.grad)):
            out["ar:" + n] = t.detach().cpu().numpy().reshape(V.AR_SHAPE[0], V.AR_SHAPE[1], -1)
        # ---- epilogues and glue
        for act in (2, 3):
            x, W, b, g = lin_inputs(act)
            lv = [t.to(dev).requires_grad_() for t in (x, W, b)]
            y = F.linear(*lv, act=act)
            y.backward(g.to(dev))
            for n, t in zip(("y", "dx", "dW", "db"), [y.detach()] + [t.grad for t in lv]):
                out["lin:%d:%s" % (act, n)] = t.cpu().numpy()
        z, hh, valid, g = la_inputs()
        zs, hs = z.to(dev).requires_grad_(), hh.to(dev).requires_grad_()
        o = F.local_attention(zs, hs, valid.to(dev).reshape(LA_SHAPE[0], LA_SHAPE[1], 1))
        o.backward(g.to(dev))
        out["la:out"], out["la:dz"], out["la:dh"] = o.detach().cpu().numpy(), zs.grad.cpu().numpy(), hs.grad.cpu().numpy()
        lg, v, g = (t.to(dev).contiguous() for t in sm_inputs())
        att, o, dl, dv = (torch.empty_like(lg) for _ in range(4))
        m._lib.launch("mmt_softmax_mul_forward", lg, v, att, o, *SM_SHAPE)
        m._lib.launch("mmt_softmax_mul_backward", g, att, v, dl, dv, *SM_SHAPE)
        for n, t in (("att", att), ("out", o), ("dlogits", dl), ("dv", dv)):
            out["sm:" + n] = t.cpu().numpy()
    torch.cuda.synchronize()
    F.check_device_errors()
    np.savez(out_path, **out)


_SWITCHES = {"default": {}, "no_fused_attn_bwd": {"MMT_NO_FUSED_ATTN_BWD": "1"}, "no_fixed_shapes": {"MMT_NO_FIXED_SHAPES": "1"},
             "no_chain4_boundary": {"MMT_NO_CHAIN4": "1", "MMT_NO_BWD_BOUNDARY": "1"}, "no_tail_fold": {"MMT_NO_TAIL_FOLD": "1"}}


def _main(tmp_dir):
    return run_child(__name__, "main", "default", None, tmp_dir, _SWITCHES, timeout=300)


def _finish(failures):
    assert not failures, "\n".join(failures)


def _widen(default, yard):
    """a bound tuple with 4x the yardstick where that is wider (None entries stay unbounded)"""
    if yard is None:
        return default
    return tuple(None if d is None else max(d, 4 * y) for d, y in zip(default, tuple(yard) + (0.0,) * len(default)))


# ------------------------------------------------------------------------------------------------ attention
_FAMILY = {"cold": ("cold", "hot"), "hot": ("cold", "hot"), "step": ("step",), "rising": ("rising", "falling"),
           "falling": ("rising", "falling"), "peaked": ("peaked",)}


def sdpa_bounds(case, tensor):
    default = (SDPA_OUT, SDPA_OUT_ROW) if tensor == "y" else (SDPA_GRAD, SDPA_GRAD_ROW)
    return _widen(default, VC.SDPA_FP32_YARD.get((_FAMILY[case[1]], case[3], tensor)))


def _sdpa_check(tag, case, p, run, fused=True):
    sel, regime, T, dk, j0 = case
    key = "sdpa:%s:p%g:" % (V.case_id(case), p)
    drop = torch.from_numpy(run[key + "keep"]).double() * float(run[key + "scale"]) if p else None
    ref = V.sdpa_reference(case, drop, fused_attn_bwd=fused)
    got = {n: run[key + n] for n in ("y", "dq", "dk", "dv")}
    failures = []
    for n in got:
        if not np.isfinite(got[n]).all():
            failures.append("%s %s: %d entries are not finite" % (tag, n, int((~np.isfinite(got[n])).sum())))
    rows = np.ones((V.ATTN_B, T, 1))
    if sel == "keyed":                                          # the truncated reference has the rows below the key length
        rows = R.prefix_mask(V.key_lengths_of(case), T).numpy().astype(np.float64)
        for b, n in enumerate(V.key_lengths_of(case)):          # behind a key length: no gradient to k and v, exactly
            if (got["dk"][b, n:] != 0).any() or (got["dv"][b, n:] != 0).any():
                failures.append("%s: dk / dv behind the key length of sequence %d" % (tag, b))
    for b, n in enumerate(V.attn_lengths(T)):                   # blanked query rows pass exactly zero gradient to q
        if (got["dq"][b, n:] != 0).any():
            failures.append("%s: dq on the blanked rows of sequence %d" % (tag, b))
    for n in got:
        g = np.nan_to_num(got[n].astype(np.float64)) * (rows if n in ("y", "dq") else 1.0)
        rel, row = sdpa_bounds(case, n)
        check("%s %s" % (tag, n), g, ref[n], rel, row, scale_ref=V.zero_scale(ref, n), failures=failures)
    _finish(failures)


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", SDPA_CASES, ids=[V.case_id(c) for c in SDPA_CASES])
def test_sdpa(tmp_dir, case, p):
    """y, dq, dk, dv of every selection and regime: finite, inside the bounds, dq exactly 0 on blanked rows, dk and dv exactly 0 behind a
    key length.  Before the fix of attn_fwd_body's first-tile rescale every `cold` case was NaN throughout.
    dk of keyed step(270), T = 290, d_k = 16, p = 0.1 measures 2.64e-2 per row: one bf16 ulp of one output element, which the
    reference's own float32 evaluation moves the same way (test_value_regimes_cpu.sdpa_fp32_yardstick says how)."""
    _sdpa_check("vr sdpa %s p%g" % (V.case_id(case), p), case, p, _main(tmp_dir))


@pytest.mark.parametrize("p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", TWO_KERNEL, ids=[V.case_id(c) for c in TWO_KERNEL])
def test_sdpa_two_kernel_backward(tmp_dir, case, p):
    """MMT_NO_FUSED_ATTN_BWD=1 at the shapes of the one-kernel backward: the plain dK/dV and dQ kernels at ten key tiles"""
    run = run_child(__name__, "sdpa", "no_fused_attn_bwd", [SDPA_CASES.index(c) for c in TWO_KERNEL], tmp_dir, _SWITCHES, timeout=300)
    _sdpa_check("vr sdpa-2k %s p%g" % (V.case_id(case), p), case, p, run, fused=False)


@pytest.mark.parametrize("case", PROBS_CASES, ids=[V.case_id(c) for c in PROBS_CASES])
def test_attn_probs(tmp_dir, case):
    """the materialised map against the fp64 softmax of the bf16 operands; masked entries exact zeros; rows sum to 1 within 1e-5"""
    sel, regime, T, dk, j0 = case
    P = _main(tmp_dir)["probs:" + V.case_id(case)]
    ref = V.probs_reference(case).numpy()
    vis = V.visible(case).expand(-1, V.ATTN_H, -1, -1).numpy()
    assert np.isfinite(P).all() and (P >= 0).all()
    assert (P[~vis] == 0).all()
    err = float(np.abs(P.astype(np.float64).sum(axis=-1) - 1.0).max())
    print("vr probs %s row-sum error %.2e" % (V.case_id(case), err))
    assert err <= 1e-5
    rel, row = sdpa_bounds(case, "y")
    check("vr probs %s" % V.case_id(case), P.reshape(-1, T), ref.reshape(-1, T), rel, row)


# ------------------------------------------------------------------------------------------------ LayerNorm
_LN_REFS = {}


def _ln_ref(regime, M, d):
    if (regime, d) not in _LN_REFS:
        x, a, b, g = (t.double() for t in V.layer_norm_input(regime, M, d))
        lv = [t.requires_grad_() for t in (x, a, b)]
        y = V.layer_norm_fp64(*lv)
        y.backward(g)
        _LN_REFS[(regime, d)] = {"y": y.detach().numpy(), "dx": lv[0].grad.numpy(), "da": lv[1].grad.numpy(), "db": lv[2].grad.numpy()}
    return _LN_REFS[(regime, d)]


def ln_bound(regime, tensor):
    default = LN_Y if tensor == "y" else LN_GRAD
    return max(default, 4 * VC.LN_OFFSET_YARD.get(tensor, 0.0)) if regime == "offset" else default


@pytest.mark.parametrize("M,d", VC.LN_SHAPES)
@pytest.mark.parametrize("regime", [r for r in V.LN_REGIMES if r != "one_constant_row"])
def test_layer_norm(tmp_dir, regime, M, d):
    run, ref = _main(tmp_dir), _ln_ref(regime, M, d)
    failures = []
    for n in ("y", "dx", "da", "db"):
        check("vr ln %s d%d %s" % (regime, d, n), run["ln:%d:%s:%s" % (d, regime, n)], ref[n], ln_bound(regime, n), failures=failures)
    _finish(failures)


@pytest.mark.parametrize("M,d", VC.LN_SHAPES)
def test_layer_norm_with_one_constant_row(tmp_dir, M, d):
    """sigma = 0 in row 1: y of that row is b_2 and finite; the reference's own dx of that row is 0/0, so nothing is asserted about it
    (the kernels' value is printed).  Every other row, and the gain and bias gradients, against the reference with that row's (zero)
    contribution; the other rows bit-identical to the run in which row 1 holds ordinary values."""
    run = _main(tmp_dir)
    got = {n: run["ln:%d:one_constant_row:%s" % (d, n)] for n in ("y", "dx", "da", "db")}
    plain = {n: run["ln:%d:plain:%s" % (d, n)] for n in ("y", "dx")}
    x, a, b, g = (t.double() for t in V.layer_norm_input("one_constant_row", M, d))
    others = [0] + list(range(2, M))
    print("vr ln constant row d%d: dx of that row is %s" % (d, "finite" if np.isfinite(got["dx"][1]).all() else "not finite (NaN or Inf)"))
    assert np.isfinite(got["y"]).all() and np.array_equal(got["y"][1], b.float().numpy())
    lv = [t.requires_grad_() for t in (x[others], a, b)]
    y = V.layer_norm_fp64(*lv)
    y.backward(g[others])
    # row 1: x-hat = 0, so it adds nothing to the gain's gradient and g[1] to the bias's
    failures = []
    check("vr ln constant d%d y" % d, got["y"][others], y.detach().numpy(), LN_Y, failures=failures)
    check("vr ln constant d%d dx" % d, got["dx"][others], lv[0].grad.numpy(), LN_GRAD, failures=failures)
    check("vr ln constant d%d da" % d, got["da"], lv[1].grad.numpy(), LN_GRAD, failures=failures)
    check("vr ln constant d%d db" % d, got["db"], (lv[2].grad + g[1]).numpy(), LN_GRAD, failures=failures)
    for n in ("y", "dx"):
        if not np.array_equal(got[n][others], plain[n][others]):
            failures.append("%s of the other rows depends on row 1" % n)
    _finish(failures)


_ENC_REFS = {}


def _enc_ref(d, h, regime):
    if (d, regime) not in _ENC_REFS:
        pd = {k: v.double().clone().requires_grad_() for k, v in enc_params(d, ENC_N, regime == "tiny").items()}
        x, g, mask = enc_inputs(d, regime)
        xd = x.double().requires_grad_()
        y = E.encoder_stack(pd, "", xd, mask.double(), h)
        y.backward(g.double())
        _ENC_REFS[(d, regime)] = (y.detach().numpy(), xd.grad.numpy(), {k: v.grad.numpy() for k, v in pd.items()})
    return _ENC_REFS[(d, regime)]


def enc_offset_widened(name):
    """the tensors of the offset case whose ENC_GRAD bound is widened from ENC_OFFSET_GRAD_YARD: dx, and the gradients of the attention
    projections' weights, the query bias and the first LayerNorm's gain"""
    return name == "dx" or (".self_attn.linears." in name and name.endswith(".weight")) or name.endswith("linears.0.bias") \
        or name.endswith("sublayer.0.norm.a_2")


def _enc_check(tag, run, d, h, regime):
    """test_gpu_bf16_faithful.test_encoder_stack's comparison and bounds"""
    y, dx, grads = _enc_ref(d, h, regime)
    wide = max(ENC_GRAD, 4 * VC.ENC_OFFSET_GRAD_YARD) if regime == "offset" else ENC_GRAD
    key = "enc:d%d:%s:" % (d, regime)
    failures = []
    check(tag + " y", run[key + "y"], y, ENC_OUT, ENC_OUT_ROW, failures=failures)
    check(tag + " dx", run[key + "dx"], dx, wide, ENC_ROW, failures=failures)
    flat, off = run[key + "dflat"], 0
    for name, shape in E.encoder_param_shapes(d, R.D_FF, ENC_N).items():
        size = int(np.prod(shape))
        got = flat[off: off + size].reshape(shape)
        off += size
        scale = grads[name.replace("linears.1.bias", "linears.0.bias")] if "linears.1.bias" in name else None      # analytically zero
        flips = ".w_1." in name or "sublayer.1.norm" in name
        check(tag + " " + name, got, grads[name], ENC_RELU_GRAD if flips else wide if enc_offset_widened(name) else ENC_GRAD,
              None if flips else ENC_ROW, scale_ref=scale, failures=failures)
        if len(shape) == 2:
            s = ls_scale(got, grads[name])
            if abs(s) > ENC_W_SCALE:
                failures.append("%s %s: scale %.3e > %.1e" % (tag, name, s, ENC_W_SCALE))
    assert off == flat.size
    _finish(failures)


@pytest.mark.parametrize("switch", ["default", "no_fixed_shapes", "no_chain4_boundary", "no_tail_fold"])
@pytest.mark.parametrize("d,h", ENC_TINY)
def test_encoder_stack_on_a_tiny_spread(tmp_dir, d, h, switch):
    """input spread 1e-5 and shrunk residual branches: the row chains' LayerNorm prologues and backwards, the fixed shapes at d = 128,
    and the final norm (folded into the last chains, or on its own under MMT_NO_TAIL_FOLD=1) all see sigma ~ 1e-5"""
    run = _main(tmp_dir) if switch == "default" else run_child(__name__, "enc", switch, None, tmp_dir, _SWITCHES, timeout=300)
    _enc_check("vr enc tiny d%d %s" % (d, switch), run, d, h, "tiny")


def test_encoder_stack_on_an_offset_input(tmp_dir):
    _enc_check("vr enc offset d128", _main(tmp_dir), 128, 8, "offset")


def test_stream_on_a_tiny_spread(tmp_dir):
    d, h, n, T = STREAM
    pd = {k: v.double() for k, v in enc_params(d, n, True).items()}
    x = V.layer_norm_input("tiny", 2 * T, d, tag="stream")[0].reshape(2, T, d)
    with torch.no_grad():
        ref = S.encoder_stack(pd, "", x.double(), R.prefix_mask([T, 5], T).double(), h).numpy()
    check("vr stream tiny y", _main(tmp_dir)["stream:y"], ref, ENC_OUT, ENC_OUT_ROW)


# ------------------------------------------------------------------------------------------------ scans
_SCAN_REFS = {}


def _cached(key, fn):
    if key not in _SCAN_REFS:
        _SCAN_REFS[key] = fn()
    return _SCAN_REFS[key]


def _step_check(tag, got, ref, yard, row_bound, failures):
    """the per-time-step measure under 4x its jitter yardstick, or under the tensor's per-row bound of its own tier where that is wider
    (a step's error over the rms step never exceeds the worst row's over the rms row, so that bound is implied anyway)"""
    s, bound = V.per_step(got, ref), max(4 * yard, row_bound)
    print("%-52s per-step %.2e (bound %.1e)" % (tag, s, bound))
    if not s <= bound:
        failures.append("%s: per-step maximum %.3e > %.1e" % (tag, s, bound))


def _saturated_check(tag, got, mask, failures):
    rms = float(np.sqrt((got.astype(np.float64) ** 2).mean()))
    worst = float(np.abs(got[mask]).max())
    print("%-52s at the +-200 entries %.2e of the rms" % (tag, worst / rms))
    if not worst < 1e-6 * rms:
        failures.append("%s: %.3e of the rms at a saturated entry" % (tag, worst / rms))


@pytest.mark.parametrize("regime,T", SCAN_RUNS, ids=["%s_T%d" % r for r in SCAN_RUNS])
@pytest.mark.parametrize("fam,B,H", V.LSTM_FAMILIES, ids=[f[0] for f in V.LSTM_FAMILIES])
def test_lstm_scan(tmp_dir, fam, B, H, regime, T):
    run = _main(tmp_dir)
    ref = _cached(("lstm", regime, T, fam), lambda: VC.lstm_reference(regime, T, B, H))
    yard = VC.LSTM_LONG_YARD.get((fam, T), {}) if regime == "long_memory" else {}
    tag = "vr lstm %s %s T%d" % (fam, regime, T)
    got = {n: run["lstm:%s:%d:%s:%s" % (regime, T, fam, n)] for n in ref}
    failures = []
    for n in ("h", "c"):
        check_scan("%s %s" % (tag, n), got[n], ref[n], _widen(LSTM_OUT, yard.get(n)), failures, seq=True)
    check_scan(tag + " dgx", got["dgx"], ref["dgx"], _widen(LSTM_DGX, yard.get("dgx")), failures, seq=True)
    check_scan(tag + " dW", got["dW"], ref["dW"], _widen(LSTM_DW, yard.get("dW")), failures,
               scale=max(LSTM_W_SCALE, 4 * yard.get("dW_scale", 0.0)))
    for n in ("dh0", "dc0"):
        check_scan("%s %s" % (tag, n), got[n], ref[n], _widen(LSTM_D0, yard.get(n)), failures)
    if regime == "long_memory":
        _step_check(tag + " dgx", got["dgx"], ref["dgx"], yard.get("step", 0.0), LSTM_DGX[1], failures)
    else:
        hi, lo = V.lstm(regime, T, B, H)[6:]
        _saturated_check(tag + " dgx", got["dgx"], (hi | lo).numpy(), failures)
    _finish(failures)


@pytest.mark.parametrize("regime,T", SCAN_RUNS, ids=["%s_T%d" % r for r in SCAN_RUNS])
@pytest.mark.parametrize("fam,B", V.MFN_FAMILIES, ids=[f[0] for f in V.MFN_FAMILIES])
def test_mfn_mem_scan(tmp_dir, fam, B, regime, T):
    """mem, the gradients, and per step (long_memory) or at the saturated entries (overflow).  Two cases looked wrong and are not:
    sw1 at long_memory, T = 70 moves 5.12e-2 per step: the reference has a ReLU pre-activation of 3.7e-7 there, and its float32
    evaluation flips it just as the kernels do, to the same 5.12e-2.  gen at overflow moves 9.29e-3 per row of mem: u = 200.4999936
    at t = 5, sequence 499 is a tie for bf16 that fp32 cannot resolve; the reference with that one rounding tipped agrees with the
    kernels to 1.5e-3 per row (test_value_regimes_cpu.py, MFN_OVERFLOW_YARD)."""
    run = _main(tmp_dir)
    ref = _cached(("mfn", regime, T, fam), lambda: VC.mfn_reference(regime, T, B))
    yard = VC.MFN_LONG_YARD.get((fam, T), {}) if regime == "long_memory" else VC.MFN_OVERFLOW_YARD.get(fam, {})
    bounds = MFN_SHORT if T <= 6 else MFN_LONG                  # test_gpu_bf16_scans.mfn_bounds' tiers
    tag = "vr mfn %s %s T%d" % (fam, regime, T)
    got = {n: run["mfn:%s:%d:%s:%s" % (regime, T, fam, n)] for n in ref}
    failures = []
    for n in ("mem", "dapre", "dchat"):
        check_scan("%s %s" % (tag, n), got[n], ref[n], _widen(bounds[n], yard.get(n)), failures, seq=True)
    for n in ("dWm", "dW2"):
        check_scan("%s %s" % (tag, n), got[n], ref[n], _widen(bounds[n], yard.get(n)), failures,
                   scale=max(MFN_W_SCALE, 4 * yard.get(n + "_scale", 0.0)))
    check_scan(tag + " db2", got["db2"].ravel(), ref["db2"].ravel(), _widen(bounds["db2"], yard.get("db2")), failures)
    if regime == "long_memory":
        # MFN_LONG has no per-row bound on dapre (a flipped ReLU lands in one entry); the per-step measure takes its own yardstick alone
        _step_check(tag + " dapre", got["dapre"], ref["dapre"], yard.get("step", 0.0), 0.0, failures)
    else:
        lo = V.mfn(regime, T, B)[7].numpy()
        if (got["dapre"][lo] != 0).any():
            failures.append(tag + ": a gradient through a ReLU closed by -200")
    _finish(failures)


@pytest.mark.parametrize("regime,T", SCAN_RUNS, ids=["%s_T%d" % r for r in SCAN_RUNS])
@pytest.mark.parametrize("kind", ["stack", "fb"])
def test_stacked_and_feedback_scans(tmp_dir, kind, regime, T):
    """the first case of STACK_CASES / FB_CASES under test_gpu_bf16_stack_fb's own comparison (its `long` tier at T = 70 and 130, its
    `short` tier at T = 9), plus the per-step measure and the saturated entries"""
    run = _main(tmp_dir)
    c = (V.stack_case if kind == "stack" else V.fb_case)(T)
    inp, w, sat = (V.stack_inputs if kind == "stack" else V.fb_inputs)(regime, T)
    ref = _cached((kind, regime, T), lambda: (stack_ref if kind == "stack" else fb_ref)(c, inputs=(inp, w)))
    got = {n: run["%s:%s:%d:%s" % (kind, regime, T, n)] for n in ref}
    tag = "vr %s %s T%d" % (kind, regime, T)
    failures = []
    compare(kind, tag, c, got, ref, failures)
    dg = "dgx0" if kind == "stack" else "dgxc"
    if regime == "long_memory":
        yard = (VC.STACK_STEP_YARD if kind == "stack" else VC.FB_STEP_YARD)[T]
        _step_check("%s %s" % (tag, dg), got[dg], ref[dg], yard, bound_of(kind, c, dg, "row"), failures)
    else:
        _saturated_check("%s %s" % (tag, dg), got[dg], sat.numpy(), failures)
    _finish(failures)


def test_ar_combine_with_the_gradient_at_the_last_step(tmp_dir):
    """free-running, K = 3, T = 130: dw of the last step is g times the last three p, which the walk carried across two chunk
    boundaries.  test_gpu_arlstm.test_ar_combine_against_fp64's bound: twice what the formula in fp32 on the CPU shows, or (K + 2) ulp."""
    run, inp = _main(tmp_dir), V.ar_inputs()
    ref, cpu = _fp64(inp, False), _cpu_fp32(inp, False)
    assert np.abs(ref["dw"][:, -1]).min() > 0 and not ref["dw"][:, :-1].any()
    K = V.AR_SHAPE[2]
    for n in ("p", "out", "din", "dw"):
        got = run["ar:" + n]
        e, e32 = rel_l2(got, ref[n]), rel_l2(cpu[n], ref[n])
        bound = max(2.0 * e32, (K + 2) * 2.0 ** -24)
        print("vr ar %-3s kernel %.3e  cpu fp32 %.3e  bound %.3e" % (n, e, e32, bound))
        assert np.isfinite(got).all() and e <= bound, n


# ------------------------------------------------------------------------------------------------ epilogues and glue
@pytest.mark.parametrize("act", [2, 3], ids=["tanh", "sigmoid"])
def test_linear_epilogue_beyond_the_exponent_range(tmp_dir, act):
    run = _main(tmp_dir)
    x, W, b, g = lin_inputs(act)
    ld = [t.double().requires_grad_() for t in (x, W, b)]
    ref = E.linear(*ld, act=act)
    ref.backward(g.double())
    pre = (E.bf16(x.double()) @ E.bf16(W.double()).t() + b.double()).abs()
    assert float((pre > 200).double().mean()) > 0.3
    failures = []
    for n, r in zip(("y", "dx", "dW", "db"), [ref.detach()] + [t.grad for t in ld]):
        check("vr lin act%d %s" % (act, n), run["lin:%d:%s" % (act, n)], r, LIN_REL, LIN_REL, failures=failures)
    _finish(failures)


def test_local_attention_with_peaked_logits(tmp_dir):
    run = _main(tmp_dir)
    z, h, valid, g = la_inputs()
    zd, hd = z.double().requires_grad_(), h.double().requires_grad_()
    ref = _local_attention_fp64(zd, hd, valid.double())
    ref.backward(g.double())
    for n, r in (("out", ref.detach()), ("dz", zd.grad), ("dh", hd.grad)):
        check("vr local attention " + n, run["la:" + n], r, max(LA_RTOL, 4 * VC.LA_DZ_YARD) if n == "dz" else LA_RTOL)


def test_softmax_mul_with_peaked_logits(tmp_dir):
    run = _main(tmp_dir)
    lg, v, g = (t.double() for t in sm_inputs())
    lg.requires_grad_()
    v.requires_grad_()
    att = torch.softmax(lg, dim=-1)
    out = att * v
    out.backward(g)
    assert float(att.detach().amax(dim=-1).median()) > 0.9               # most rows nearly one-hot
    for n, r in (("att", att.detach()), ("out", out.detach()), ("dlogits", lg.grad), ("dv", v.grad)):
        check("vr softmax_mul " + n, run["sm:" + n], r, SOFTMAX_REL)
