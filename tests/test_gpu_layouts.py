"""GPU: every op on strided, offset, transposed and non-fp32 arguments (tests/layout_variants.py).

The rest of the suite hands every op fresh, contiguous, 16-byte aligned fp32 tensors.  Here each op of functional.py (and
metrics.batched_ccc, optim.FlatAdam, the streams, four models end to end) is called once that way, the baseline, and then again with
the SAME VALUES in other layouts and element types; outputs and input gradients must have the baseline's bits, because the layer between
autograd and the kernels (_f32c, _f32c16, the backward methods, the raw pointers of _lib.launch) may only ever change where the numbers
lie.  The pointer contract this holds is stated in include/mmt_hip.h (conventions) and INTEGRATION.md: an argument of class (c), which a
kernel moves 16 bytes per lane, is refused by its entry when misaligned (test_c_boundary_refuses_a_misaligned_class_c_pointer) and
repaired by the binding before the call, so no kernel here ever runs on a pointer outside the contract.

ROWS is the table: one row per op and mode, at the smallest shape the op's own domain check admits with B >= 2, an odd T >= 3, prefix
lengths (T, 3) and, where the op allows it, a row length that is no multiple of 4 floats.  tests/test_layouts_cpu.py imports it and
fails on an op of functional.py without a row.
"""
import ctypes
import types

import pytest
import torch

import layout_variants as LV
import recipe as R
from conftest import rel_l2
from gpu_harness import dev, mta  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

LENGTHS = [5, 3]                 # B = 2, T = 5: one full sequence, one shorter prefix


def N(tag, *shape, s=0.5):
    return R.gen_normal("layouts:" + tag, tuple(shape), 11) * s


def MASK(B=2, T=5, lengths=None):
    return R.prefix_mask(lengths or LENGTHS, T)            # (B,T,1) float {0,1}


class Row:
    """name; covers: the names of functional.py (or "metrics.batched_ccc", ...) the row exercises; args: [(kind, CPU tensor)] with kind
    "g" a float tensor that takes a gradient, "d" float data, "f" float data whose fp32 type is part of the op's contract (layouts
    only), "m" a {0,1} mask (also given as bool and int64), "i" an int32 tensor (layouts only); call(package, *tensors) -> a tensor or
    a tuple; diff: the indices of the outputs that carry a gradient."""

    def __init__(self, name, covers, args, call, diff=(0,)):
        self.name, self.covers, self.args, self.call, self.diff = name, tuple(covers), list(args), call, tuple(diff)


def _enc_param_shapes(d, f, n):
    per = [(d, d), (d,)] * 4 + [(f, d), (f,), (d, f), (d,)] + [(d,)] * 4
    return per * n + [(d,), (d,)]


def _rows():
    rows = []

    def add(name, covers, args, call, diff=(0,)):
        rows.append(Row(name, covers, args, call, diff))

    # ---- affine maps: (M, K, N) = (5, 6, 3); K = 6 is padded to 8 inside linear (cat_cols); the pair and the prepared map refuse K % 4
    lin = [("g", N("lin:x", 5, 6)), ("g", N("lin:W", 3, 6)), ("g", N("lin:b", 3))]
    add("linear", ["linear", "_LinearFn", "cat_cols", "_CatColsFn"], lin, lambda M, x, W, b: M.functional.linear(x, W, b))
    add("linear relu rowscale", ["linear", "_LinearFn"], lin + [("d", torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0]))],
        lambda M, x, W, b, r: M.functional.linear(x, W, b, act=1, rowscale=r))
    add("linear dropout", ["linear", "_LinearFn"], lin,
        lambda M, x, W, b: M.functional.linear(x, W, b, act=1, in_dropout=0.25, out_dropout=0.5, seed=5))
    # K = 4: no padding copy stands between the caller's x and mmt_linear_forward, which moves it four floats per lane
    add("linear K4", ["linear", "_LinearFn"], [("g", N("lin4:x", 5, 4)), ("g", N("lin4:W", 3, 4)), ("g", N("lin4:b", 3))],
        lambda M, x, W, b: M.functional.linear(x, W, b, act=2))
    add("linear_pair", ["linear_pair", "_LinearPairFn"],
        [("g", N("pair:x", 5, 4)), ("g", N("pair:W1", 3, 4)), ("g", N("pair:b1", 3)), ("g", N("pair:W2", 3, 4)), ("g", N("pair:b2", 3))],
        lambda M, x, W1, b1, W2, b2: M.functional.linear_pair(x, W1, b1, W2, b2, act1=1, act2=2), diff=(0, 1))

    def prepared(M, x, W, b, r):
        with torch.no_grad():
            return M.functional.linear_prepared(x, M.functional.linear_prepare(W, b), 3, act=1, rowscale=r)
    add("linear_prepared", ["linear_prepared", "linear_prepare"],
        [("f", N("prep:x", 5, 4)), ("d", N("prep:W", 3, 4)), ("d", N("prep:b", 3)), ("d", torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0]))],
        prepared, diff=())
    hw = [("g", N("hw:x", 5, 4)), ("g", N("hw:Wp", 4, 4)), ("g", N("hw:bp", 4)), ("g", N("hw:Wg", 4, 4)), ("g", N("hw:bg", 4))]
    add("highway", ["highway", "_HighwayFn"], hw, lambda M, *t: M.functional.highway(*t))
    add("highway train relu", ["highway", "_HighwayFn"], hw, lambda M, *t: M.functional.highway(*t, dropout_p=0.3, seed=9, proj_act=1))
    add("layer_norm", ["layer_norm", "_LayerNormFn"], [("g", N("ln:x", 5, 4)), ("g", 1.0 + N("ln:a", 4)), ("g", N("ln:b", 4))],
        lambda M, x, a, b: M.functional.layer_norm(x, a, b))

    # ---- attention and the encoder stack: B = 2, T = 5, d = 16, h = 2, d_ff = 16, N = 1
    kl = ("i", torch.tensor(LENGTHS, dtype=torch.int32))
    qkv = [("g", N("att:q", 2, 5, 16)), ("g", N("att:k", 2, 5, 16)), ("g", N("att:v", 2, 5, 16)), ("m", MASK())]
    add("sdpa", ["sdpa", "_SdpaFn"], qkv, lambda M, q, k, v, m: M.functional.sdpa(q, k, v, m, 2))
    add("sdpa keys", ["sdpa", "_SdpaFn"], qkv + [kl], lambda M, q, k, v, m, l: M.functional.sdpa(q, k, v, m, 2, key_lengths=l))
    add("sdpa causal", ["sdpa", "_SdpaFn"], qkv, lambda M, q, k, v, m: M.functional.sdpa(q, k, v, m, 2, causal=True))
    add("sdpa train", ["sdpa", "_SdpaFn"], qkv, lambda M, q, k, v, m: M.functional.sdpa(q, k, v, m, 2, dropout_p=0.1, seed=7))
    qk = [("d", N("att:q", 2, 5, 16)), ("d", N("att:k", 2, 5, 16)), ("m", MASK())]
    add("attn_probs", ["attn_probs"], qk, lambda M, q, k, m: M.functional.attn_probs(q, k, m, 2), diff=())
    add("attn_probs keys", ["attn_probs"], qk + [kl], lambda M, q, k, m, l: M.functional.attn_probs(q, k, m, 2, key_lengths=l), diff=())
    add("attn_probs causal", ["attn_probs"], qk, lambda M, q, k, m: M.functional.attn_probs(q, k, m, 2, causal=True), diff=())
    add("attn_probs train", ["attn_probs"], qk, lambda M, q, k, m: M.functional.attn_probs(q, k, m, 2, dropout_p=0.1, seed=7), diff=())
    add("key_lengths", ["key_lengths"], [("m", MASK())], lambda M, m: M.functional.key_lengths(m), diff=())
    shapes = _enc_param_shapes(16, 16, 1)
    ps = [N("enc:p%d" % i, *s, s=0.25) for i, s in enumerate(shapes)]
    flat = torch.cat([p.reshape(-1) for p in ps])
    enc = [("g", N("enc:x", 2, 5, 16)), ("m", MASK()), ("g", flat)]
    add("encoder_stack", ["encoder_stack", "_EncoderStackFn"], enc, lambda M, x, m, p: M.functional.encoder_stack(x, m, p, 2, 16, 1))
    add("encoder_stack keys", ["encoder_stack", "_EncoderStackFn"], enc + [kl],
        lambda M, x, m, p, l: M.functional.encoder_stack(x, m, p, 2, 16, 1, key_lengths=l))
    add("encoder_stack causal", ["encoder_stack", "_EncoderStackFn"], enc, lambda M, x, m, p: M.functional.encoder_stack(x, m, p, 2, 16, 1, causal=True))
    add("encoder_stack train", ["encoder_stack", "_EncoderStackFn"], enc,
        lambda M, x, m, p: M.functional.encoder_stack(x, m, p, 2, 16, 1, dropout_p=0.1, seed=11))
    encp = [("g", N("enc:x", 2, 5, 16)), ("m", MASK())] + [("g", p) for p in ps]
    add("encoder_stack_params", ["encoder_stack_params", "_EncoderStackParamsFn"], encp,
        lambda M, x, m, *p: M.functional.encoder_stack_params(x, m, list(p), 2, 16, 1))
    add("encoder_stack_params keys", ["encoder_stack_params", "_EncoderStackParamsFn"], encp + [kl],
        lambda M, x, m, *p: M.functional.encoder_stack_params(x, m, list(p[:-1]), 2, 16, 1, key_lengths=p[-1]))
    add("encoder_stack_params causal", ["encoder_stack_params", "_EncoderStackParamsFn"], encp,
        lambda M, x, m, *p: M.functional.encoder_stack_params(x, m, list(p), 2, 16, 1, causal=True))
    add("encoder_stack_params train", ["encoder_stack_params", "_EncoderStackParamsFn"], encp,
        lambda M, x, m, *p: M.functional.encoder_stack_params(x, m, list(p), 2, 16, 1, dropout_p=0.1, seed=11))

    # ---- window encoder: 3 windows, W = 4, D = 8, F = 5 (the windows are data: no gradient)
    add("conv_maxpool", ["conv_maxpool", "_ConvPoolFn"], [("d", N("cv:x", 3, 4, 8)), ("g", N("cv:w", 5, 8, 2)), ("g", N("cv:b", 5))],
        lambda M, x, w, b: M.functional.conv_maxpool(x, w, b))
    add("conv_maxpool_k", ["conv_maxpool_k", "_ConvPoolFn"], [("d", N("cv:x", 3, 4, 8)), ("g", N("cv:w3", 5, 8, 3)), ("g", N("cv:b", 5))],
        lambda M, x, w, b: M.functional.conv_maxpool_k(x, w, b))

    # ---- scans: T = 3, B = 2, H = 16
    scan = [("g", N("ls:gx", 3, 2, 64)), ("g", N("ls:W", 64, 16, s=0.2))]
    init = [("g", N("ls:h0", 2, 16)), ("g", N("ls:c0", 2, 16))]
    add("lstm_scan", ["lstm_scan", "_LstmScanFn"], scan + init, lambda M, *t: M.functional.lstm_scan(*t), diff=(0, 1))
    add("lstm_scan no init", ["lstm_scan", "_LstmScanFn"], scan, lambda M, *t: M.functional.lstm_scan(*t), diff=(0, 1))
    stack = [("g", N("st:gx", 3, 2, 64)), ("g", N("st:P", 2, 64, 32, s=0.2)), ("g", N("st:b", 1, 64))]
    sinit = [("g", N("st:h0", 2, 2, 16)), ("g", N("st:c0", 2, 2, 16))]
    add("lstm_stack_scan", ["lstm_stack_scan", "_LstmStackScanFn"], stack + sinit,
        lambda M, *t: M.functional.lstm_stack_scan(*t, return_states=True))
    add("lstm_stack_scan no init", ["lstm_stack_scan", "_LstmStackScanFn"], stack,
        lambda M, *t: M.functional.lstm_stack_scan(*t, return_states=True))
    fb = [("g", N("fb:gx", 3, 2, 64)), ("g", N("fb:wp", 64)), ("g", N("fb:Whh", 64, 16, s=0.2)), ("g", N("fb:W1", 4, 16)), ("g", N("fb:b1", 4)),
          ("g", N("fb:w2", 4)), ("g", N("fb:b2", 1)), ("g", N("fb:h0", 2, 16)), ("g", N("fb:c0", 2, 16))]
    add("lstm_fb_scan", ["lstm_fb_scan", "_LstmFbScanFn"], fb,
        lambda M, *t: M.functional.lstm_fb_scan(*t, p_init=0.25, return_states=True))
    mem = [("g", N("mem:a", 3, 2, 128)), ("g", N("mem:c", 3, 2, 128)), ("g", N("mem:Wm", 128, 128, s=0.05)),
           ("g", N("mem:W2", 2, 128, 64, s=0.1)), ("g", N("mem:b2", 2, 128))]
    add("mfn_mem_scan", ["mfn_mem_scan", "_MfnMemScanFn"], mem, lambda M, *t: M.functional.mfn_mem_scan(*t))
    add("mfn_mem_scan train", ["mfn_mem_scan", "_MfnMemScanFn"], mem, lambda M, *t: M.functional.mfn_mem_scan(*t, dropout_p=0.2, seed=3))
    for H in (8, 6):
        for over in ("time", "taps"):
            add("local_attention H%d %s" % (H, over), ["local_attention", "_LocalAttnFn"],
                [("g", N("la:z", 2, 5, 3)), ("g", N("la:h%d" % H, 5, 2, H)), ("m", MASK().reshape(2, 5))],
                lambda M, z, h, v, over=over: M.functional.local_attention(z, h, v, over=over))
    ar = [("g", N("ar:c", 2, 5, 1)), ("g", N("ar:w", 2, 5, 3)), ("m", MASK())]
    add("ar_combine free", ["ar_combine", "_ArCombineFn"], ar, lambda M, c, w, m: M.functional.ar_combine(c, w, m, None, 0.5, return_p=True))
    add("ar_combine teacher", ["ar_combine", "_ArCombineFn"], ar + [("d", N("ar:t", 2, 5, 1))],
        lambda M, c, w, m, t: M.functional.ar_combine(c, w, m, t, 0.5, return_p=True))

    # ---- the MFN gate: T = 3, B = 2, three modalities of unequal H (sum 12: the gate's widths 2 sum H and sum H + 128 are multiples of 4)
    Hs, SH = (3, 5, 4), 12
    A = 2 * SH
    gshapes = [(8, A), (8,), (A, 8), (A,), (8, A), (8,), (128, 8), (128,), (64, A + 128), (64,), (128, 64), (128,),
               (64, A + 128), (64,), (128, 64), (128,), (8, SH + 128), (8,), (1, 8), (1,)]
    gate = [("g", N("gate:h%d" % i, 3, 2, H)) for i, H in enumerate(Hs)] + [("g", N("gate:c%d" % i, 3, 2, H)) for i, H in enumerate(Hs)] + \
           [("g", N("gate:p%d" % i, *s, s=0.2)) for i, s in enumerate(gshapes)]
    add("mfn_gate", ["mfn_gate", "_MfnGateFn"], gate, lambda M, *t: M.functional.mfn_gate(list(t[:3]), list(t[3:6]), list(t[6:])))
    add("mfn_gate train", ["mfn_gate", "_MfnGateFn"], gate,
        lambda M, *t: M.functional.mfn_gate(list(t[:3]), list(t[3:6]), list(t[6:]), gamma_dropout=0.2, gamma_seed=3, out_dropout=0.5, out_seed=4))

    # ---- glue, at the shapes of test_gpu_models.py::test_glue_ops_match_torch (B, T, d = 3, 7, 20)
    gm = MASK(3, 7, [7, 4, 1])
    add("time_major", ["time_major", "_TimeMajorFn", "batch_major", "_BatchMajorFn"], [("g", N("gl:x", 3, 7, 20))], lambda M, x: M.functional.time_major(x))
    add("batch_major rowscale", ["batch_major", "_BatchMajorFn"], [("g", N("gl:xt", 7, 3, 20)), ("m", gm)], lambda M, x, m: M.functional.batch_major(x, m))
    add("batch_major", ["batch_major", "_BatchMajorFn"], [("g", N("gl:xt", 7, 3, 20))], lambda M, x: M.functional.batch_major(x))
    add("add2 matrix", ["add2", "_Add2Fn"], [("g", N("gl:W", 12, 44)), ("g", N("gl:W'", 12, 44))], lambda M, a, b: M.functional.add2(a, b))
    add("add2 vector", ["add2", "_Add2Fn"], [("g", N("gl:v", 44)), ("g", N("gl:v'", 44))], lambda M, a, b: M.functional.add2(a, b))
    # add_row0 modifies a contiguous fp32 tensor in place (it raises for anything else): the variants go to the row, gx is made so
    add("add_row0", ["add_row0", "_AddRow0Fn"], [("g", N("gl:xt", 7, 3, 20)), ("g", N("gl:row", 1, 1, 20))],
        lambda M, t, r: M.functional.add_row0(t.float().contiguous() * 1.0, r))
    add("broadcast_rows", ["broadcast_rows", "_BroadcastRowsFn"], [("g", N("gl:row", 1, 1, 20))], lambda M, r: M.functional.broadcast_rows(r, 5))
    add("broadcast_layers", ["broadcast_layers", "_BroadcastLayersFn"], [("g", N("gl:rows", 2, 1, 20))], lambda M, r: M.functional.broadcast_layers(r, 3))
    # copy2d: what every glue row launches; a width of 3 floats runs its scalar form
    add("cat_cols", ["cat_cols", "_CatColsFn", "copy2d"], [("g", N("gl:p%d" % i, 7, 3, w)) for i, w in enumerate((8, 3, 20))],
        lambda M, *t: M.functional.cat_cols(list(t)))
    add("decoder_pack", ["decoder_pack", "_DecoderPackFn"],
        [("g", N("gl:Wi", 16, 8)), ("g", N("gl:Wh", 16, 4)), ("g", N("gl:bi", 16)), ("g", N("gl:bh", 16))],
        lambda M, *t: M.functional.decoder_pack(*t), diff=(0, 1, 2, 3))

    def lstm_like(names, tensors, layers):
        return types.SimpleNamespace(num_layers=layers, **dict(zip(names, tensors)))
    snames = ["%s_l%d" % (n, l) for l in range(2) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    add("decoder_stack_pack", ["decoder_stack_pack", "_DecoderStackPackFn"],
        [("g", N("gl:s%d" % i, *s)) for i, s in enumerate([(16, 8), (16, 4), (16,), (16,), (16, 4), (16, 4), (16,), (16,)])],
        lambda M, *t: M.functional.decoder_stack_pack(lstm_like(snames, t, 2)), diff=(0, 1, 2, 3))
    add("decoder_fb_pack", ["decoder_fb_pack", "_DecoderFbPackFn"], [("g", N("gl:fWi", 16, 5)), ("g", N("gl:fbi", 16)), ("g", N("gl:fbh", 16))],
        lambda M, *t: M.functional.decoder_fb_pack(lstm_like(["weight_ih_l0", "bias_ih_l0", "bias_hh_l0"], t, 1)), diff=(0, 1, 2))

    # ---- loss and metric: (2, 5, 1) and (2, 5)
    loss = [("g", N("mse:p", 2, 5, 1)), ("d", N("mse:t", 2, 5, 1))]
    add("mse_sum_loss", ["mse_sum_loss", "_MseSumLossFn"], loss, lambda M, p, t: M.functional.mse_sum_loss(p, t, 8.0))
    add("mse_sum_loss_backward", ["mse_sum_loss_backward"], loss, lambda M, p, t: M.functional.mse_sum_loss_backward(p, t, 8.0), diff=())
    add("batched_ccc", ["metrics.batched_ccc"], [("d", N("ccc:p", 2, 5)), ("d", N("ccc:t", 2, 5))],
        lambda M, p, t: M.metrics.batched_ccc(p, t, LENGTHS), diff=())
    return rows


ROWS = _rows()
# what the tests below the table exercise: name -> the test
OTHER_COVERAGE = {
    "test_streams_take_strided_windows_and_bool_masks": [
        "%s_stream_%s" % (fam, what) for fam in ("encoder", "mfn", "decoder", "lstm") for what in ("state", "prepare", "step", "step_slots")],
    "test_flat_adam_on_views_at_odd_addresses": ["optim.FlatAdam"],
}


def covered_names():
    """Every name a row of the table, or a test below it, says it exercises (tests/test_layouts_cpu.py compares with functional.py)."""
    names = set()
    for row in ROWS:
        names.update(row.covers)
    for lst in OTHER_COVERAGE.values():
        names.update(lst)
    return names


# ---------------------------------------------------------------------------------------------------------------- the runner
def _to(dev, t):
    return t.to(dev)


def _variant_args(row, dev, kind, which=None):
    """The row's arguments on the device under one variant kind: "plain"; "strided" / "transposed" / "f64" on every tensor the kind
    applies to; "offset" on argument `which` alone; "bool" / "int64" on the masks."""
    out = []
    for i, (k, t) in enumerate(row.args):
        t = LV.plain(_to(dev, t))
        if kind in ("strided", "transposed") or (kind == "offset" and i == which):
            t = LV.build(kind, t)
        elif kind == "f64" and k in ("g", "d", "m"):
            t = LV.f64(t)
        elif kind in ("bool", "int64") and k == "m":
            t = LV.build(kind, t)
        out.append(t)
    return out


def _run(row, M, tensors, gos=None, only=None):
    """One call of the row on `tensors` and, given `gos` (one gradient per output), one backward of its differentiable outputs
    (`only`: of that output alone) -> (outputs, the gradient of every argument: None where it takes or received none)."""
    leaves = [t.requires_grad_() if k == "g" else t for (k, _), t in zip(row.args, tensors)]
    outs = row.call(M, *leaves)
    outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
    diff = [i for i in row.diff if only is None or i == only]
    if gos is not None and diff:
        torch.autograd.backward([outs[i] for i in diff], [gos[i] for i in diff])
    torch.cuda.synchronize()
    return tuple(o.detach() for o in outs), tuple(t.grad if k == "g" else None for (k, _), t in zip(row.args, leaves))


def _grad_variant(kind, go):
    """(the gradient output under `kind`, what the baseline gets in its place)"""
    if kind == "expanded":
        if go.dim() == 0 or go.shape[0] < 2:
            return go, go
        e = LV.expanded(go[:1].clone(), go.shape)
        return e, e.contiguous()
    try:
        return LV.GRAD_BUILDERS[kind](go), go
    except ValueError:
        return go, go


@pytest.mark.parametrize("row", ROWS, ids=[r.name.replace(" ", "_") for r in ROWS])
def test_same_bits_in_every_layout(dev, row):
    M = mta()
    failures = []

    def attempt(tag, fn, want):
        try:
            LV.assert_same_bits("%s [%s]" % (row.name, tag), fn(), want)
        except AssertionError as e:
            failures.append(str(e))
        except Exception as e:  # noqa: BLE001 (an op that raises under a layout is a finding of this row, reported with the others)
            failures.append("%s [%s]: %s: %s" % (row.name, tag, type(e).__name__, e))

    outs0, _ = _run(row, M, _variant_args(row, dev, "plain"))
    gos = [(R.gen_normal("layouts:go:%s:%d" % (row.name, i), tuple(o.shape), 13).to(dev) if o.dtype.is_floating_point else None)
           for i, o in enumerate(outs0)]
    want = _run(row, M, _variant_args(row, dev, "plain"), gos)
    attempt("plain again", lambda: _run(row, M, _variant_args(row, dev, "plain"), gos), want)
    for kind in ("strided", "transposed", "f64"):
        attempt(kind, lambda kind=kind: _run(row, M, _variant_args(row, dev, kind), gos), want)
    for i, (k, t) in enumerate(row.args):                     # alignment is a property of one pointer: one argument at a time
        if t.element_size() == 4:
            attempt("offset arg %d" % i, lambda i=i: _run(row, M, _variant_args(row, dev, "offset", i), gos), want)
    if any(k == "m" for k, _ in row.args):
        for kind in ("bool", "int64"):
            attempt(kind, lambda kind=kind: _run(row, M, _variant_args(row, dev, kind), gos), want)
    if row.diff:
        for kind in ("strided", "offset", "expanded"):            # gradient outputs that are not plain, on the contiguous inputs
            pairs = [(_grad_variant(kind, g) if (g is not None and i in row.diff) else (g, g)) for i, g in enumerate(gos)]
            base = want if kind != "expanded" else _run(row, M, _variant_args(row, dev, "plain"), [p[1] for p in pairs])
            attempt("grad " + kind, lambda pairs=pairs: _run(row, M, _variant_args(row, dev, "plain"), [p[0] for p in pairs]), base)
    if len(row.diff) > 1:                                     # one output alone feeds the loss: the others' gradients arrive as None (or zeros)
        for i in row.diff:
            zeros = [g if j == i else (None if g is None else torch.zeros_like(g)) for j, g in enumerate(gos)]
            base = _run(row, M, _variant_args(row, dev, "plain"), zeros)
            attempt("only output %d" % i, lambda i=i: _run(row, M, _variant_args(row, dev, "plain"), gos, only=i), base)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------- streams
def _stream_family(M, dev, fam):
    """-> dict(nbytes, inputs [(B,T,d) per input], prepare(state, vary), step(state, xs_t, mask_t, t), slots(state, xs_t, mask_t, pos)) of
    one family at B = 2 and its smallest dims.  `vary`: the parameters as views 4 bytes into larger buffers (they are class (a))."""
    F = M.functional
    B, T = 2, 3

    def P(tag, *shape):
        return (N("stream:%s:%s" % (fam, tag), *shape, s=0.3)).to(dev)

    def v(t, vary):
        return LV.offset(t) if vary else t
    if fam == "encoder":
        d, h, f, n, cap = 8, 2, 4, 1, 4
        flat = torch.cat([P("p%d" % i, *s).reshape(-1) for i, s in enumerate(_enc_param_shapes(d, f, n))])
        return dict(nbytes=F.encoder_stream_bytes(B, cap, d, h, f, n), inputs=[P("x", B, T, d)], state=lambda: F.encoder_stream_state(B, cap, d, h, f, n, dev),
                    prepare=lambda st, vary: F.encoder_stream_prepare(v(flat, vary), st, B, cap, d, h, f, n),
                    step=lambda st, xs, m, t: F.encoder_stream_step(xs[0], m, flat, st, t, h, f, n, cap),
                    slots=lambda st, xs, m, pos: F.encoder_stream_step_slots(xs[0], m, flat, st, pos, h, f, n, cap))
    if fam == "mfn":
        D, H, out = [4, 8], [4, 8], 1
        SH, A = sum(H), 2 * sum(H)
        cells = [[P("l%d%d" % (i, j), *s) for j, s in enumerate([(4 * hh, dd), (4 * hh, hh), (4 * hh,), (4 * hh,)])] for i, (dd, hh) in enumerate(zip(D, H))]
        gshapes = [(128, A), (128,), (A, 128), (A,), (256, A), (256,), (128, 256), (128,), (64, A + 128), (64,), (128, 64), (128,),
                   (64, A + 128), (64,), (128, 64), (128,), (64, SH + 128), (64,), (out, 64), (out,)]
        gate = [P("g%d" % i, *s) for i, s in enumerate(gshapes)]
        return dict(nbytes=F.mfn_stream_bytes(B, D, H, out), inputs=[P("x%d" % i, B, T, dd) for i, dd in enumerate(D)],
                    state=lambda: F.mfn_stream_state(B, D, H, out, dev),
                    prepare=lambda st, vary: F.mfn_stream_prepare([[v(q, vary) for q in c] for c in cells], [v(q, vary) for q in gate], st, B, D, H, out),
                    step=lambda st, xs, m, t: F.mfn_stream_step(xs, m, st, t, D, H, out),
                    slots=lambda st, xs, m, pos: F.mfn_stream_step_slots(xs, m, st, pos, D, H, out))
    if fam == "decoder":
        d, hd, L = 4, 3, 1
        lstm = [[P("l%d" % j, *s) for j, s in enumerate([(4 * d, 2 * d), (4 * d, d), (4 * d,), (4 * d,)])]]
        h0, c0 = P("h0", L, 1, d), P("c0", L, 1, d)
        outp = [P("o%d" % j, *s) for j, s in enumerate([(hd, d), (hd,), (1, hd), (1,)])]
        return dict(nbytes=F.decoder_stream_bytes(B, d, hd, L), inputs=[P("e", B, T, d)], state=lambda: F.decoder_stream_state(B, d, hd, L, dev),
                    prepare=lambda st, vary: F.decoder_stream_prepare([[v(q, vary) for q in lstm[0]]], v(h0, vary), v(c0, vary),
                                                                      [v(q, vary) for q in outp], st, B, d, hd, L),
                    step=lambda st, xs, m, t: F.decoder_stream_step(xs[0], m, st, t, d, hd, L),
                    slots=lambda st, xs, m, pos: F.decoder_stream_step_slots(xs[0], m, st, pos, d, hd, L))
    I, E, H, NL, L = 3, 5, 3, 1, 3
    dims = (I, E, H, NL, L)
    emb = [P("e0", E, I), P("e1", E)]
    att = [P("a%d" % j, *s) for j, s in enumerate([(E, E), (E,), (L, E), (L,)])]
    lstm = [[P("l%d" % j, *s) for j, s in enumerate([(4 * H, E), (4 * H, H), (4 * H,), (4 * H,)])]]
    dec = [P("d%d" % j, *s) for j, s in enumerate([(E, H), (E,), (1, E), (1,)])]
    return dict(nbytes=F.lstm_stream_bytes(B, *dims), inputs=[P("x", B, T, I)], state=lambda: F.lstm_stream_state(B, *dims, dev),
                prepare=lambda st, vary: F.lstm_stream_prepare([v(q, vary) for q in emb], [v(q, vary) for q in att],
                                                               [[v(q, vary) for q in lstm[0]]], [v(q, vary) for q in dec], st, B, *dims),
                step=lambda st, xs, m, t: F.lstm_stream_step(xs[0], m, st, t, *dims),
                slots=lambda st, xs, m, pos: F.lstm_stream_step_slots(xs[0], m, st, pos, *dims))


@pytest.mark.parametrize("fam", ["encoder", "mfn", "decoder", "lstm"])
def test_streams_take_strided_windows_and_bool_masks(dev, fam):
    """prepare, three steps and three slot steps with x_t = x[:, t] of a (B,T,d) tensor (not contiguous), a bool mask_t and parameters at
    odd addresses: outputs, every byte of the state and the positions equal the run on contiguous fp32 windows.  A state at a
    misaligned address is refused before any launch."""
    M = mta()
    S = _stream_family(M, dev, fam)
    B, T = 2, 3
    mask = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]], device=dev)           # (B,T): the second sequence ends one window early

    def run(vary, slots):
        st = S["state"]().zero_()                   # the memory may have any contents: zeros, so that the unused bytes compare equal
        S["prepare"](st, vary)
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        ys = []
        for t in range(T):
            if vary:
                xs, m = [x[:, t] for x in S["inputs"]], mask[:, t] != 0
                assert not xs[0].is_contiguous() and m.dtype == torch.bool
            else:
                xs, m = [x[:, t].contiguous() for x in S["inputs"]], mask[:, t].contiguous()
            ys.append(S["slots"](st, xs, m, pos) if slots else S["step"](st, xs, m, t))
        torch.cuda.synchronize()
        return {"y": tuple(ys), "state": st, "positions": pos}

    for slots in (False, True):
        LV.assert_same_bits("%s stream %s" % (fam, "step_slots" if slots else "step"), run(True, slots), run(False, slots))
    big = torch.zeros(S["nbytes"] + 64, dtype=torch.uint8, device=dev)
    odd = big[4:4 + S["nbytes"]]
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    xs, pos = [x[:, 0].contiguous() for x in S["inputs"]], torch.zeros(B, dtype=torch.int32, device=dev)
    for call in (lambda: S["prepare"](odd, False), lambda: S["step"](odd, xs, None, 0), lambda: S["slots"](odd, xs, None, pos)):
        with pytest.raises(ValueError, match="16-byte aligned"):
            call()
    assert not bool(big.any()) and not bool(pos.any()), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------------------------- optimiser
def test_flat_adam_on_views_at_odd_addresses(dev):
    """Parameters and gradients that are views one float into flat buffers, with sizes that are no multiples of 4, so that the merged
    range starts and the tensors meet at odd addresses: two steps against torch.optim.Adam at the 2e-6 of
    test_gpu_training.py::test_flat_adam_matches_torch_adam, and bit-equal to FlatAdam on aligned copies."""
    from multimodal_transformer_amd.optim import FlatAdam
    shapes = [(5,), (3, 3), (2, 3, 1), (7,), (6,)]
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    vals = [N("adam:p%d" % i, *s) for i, s in enumerate(shapes)]

    def seat(lead):
        """the parameters as views of ONE flat buffer behind `lead` floats, and their gradient buffer laid out alike"""
        pbuf = torch.zeros(lead + sum(sizes), device=dev)
        gbuf = torch.zeros(lead + sum(sizes), device=dev)
        ps, off = [], lead
        for v, s, n in zip(vals, shapes, sizes):
            p = torch.nn.Parameter(pbuf[off:off + n].view(s))
            with torch.no_grad():
                p.copy_(v.to(dev))
            ps.append((p, gbuf[off:off + n].view(s)))
            off += n
        return ps
    odd, even = seat(1), seat(0)
    assert odd[0][0].data_ptr() % 16 == 4 and even[0][0].data_ptr() % 16 == 0
    ref = [torch.nn.Parameter(v.to(dev).clone()) for v in vals]
    opts = [FlatAdam([p for p, _ in odd], lr=1e-2, weight_decay=1e-2), FlatAdam([p for p, _ in even], lr=1e-2, weight_decay=1e-2),
            torch.optim.Adam(ref, lr=1e-2, weight_decay=1e-2)]
    for step in range(2):
        gs = [N("adam:g%d:%d" % (step, i), *s).to(dev) for i, s in enumerate(shapes)]
        for seated in (odd, even):
            for (p, gview), g in zip(seated, gs):
                gview.copy_(g)
                p.grad = gview
        for p, g in zip(ref, gs):
            p.grad = g.clone()
        if step == 0:
            assert len(FlatAdam._ranges([p for p, _ in odd])) == 1, "the views are neighbours: one merged range"
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    LV.assert_same_bits("FlatAdam at odd addresses against aligned copies", [p.detach() for p, _ in odd], [p.detach() for p, _ in even])
    for i, ((p, _), q) in enumerate(zip(odd, ref)):
        assert rel_l2(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 2e-6, i


# ---------------------------------------------------------------------------------------------------------------- models, end to end
def _models(M, dev):
    MT, MM = M.multiTransformer, M.models
    mods, win = ["emotient", "acoustic"], {"emotient": 8, "acoustic": 12}
    return {
        "NLPTransformer": (lambda: MT.NLPTransformer(8, embed_dim=8, h_dim=4, N=1, d_ff=8, h=2, device=dev), [8], "bt"),
        "MultiTransformer": (lambda: MT.MultiTransformer(mods, win, N=1, d_ff=8, h=2, device=dev, embed_dim={"emotient": 8, "acoustic": 8}), [8, 12], "bt"),
        "MFN": (lambda: MT.MFN(mods, win, 1, device=dev), [8, 12], "tb"),
        "MultiLSTM": (lambda: MM.MultiLSTM(8, embed_dim=8, h_dim=8, n_layers=1, attn_len=3, device=dev), [8], "bt"),
    }


@pytest.mark.parametrize("name", ["NLPTransformer", "MultiTransformer", "MFN", "MultiLSTM"])
def test_models_take_a_sliced_float64_input_and_a_bool_mask(dev, name):
    """Eval mode, smallest sizes: x = big[:, 1:T + 1] of a (B, T + 2, D) float64 tensor and a bool mask give the output and every parameter
    gradient of the plain call, bit for bit.  (The MFN takes time-major inputs and no mask: its slice is along the batch axis.)"""
    M = mta()
    make, widths, order = _models(M, dev)[name]
    torch.manual_seed(5)
    model = make().eval()
    B, T = 2, 5
    mods = ["emotient", "acoustic"]
    mask = MASK().to(dev)

    def inputs(vary):
        xs = []
        for i, D in enumerate(widths):
            x = N("model:%s:x%d" % (name, i), B, T, D).to(dev)
            if order == "tb":
                x = x.permute(1, 0, 2).contiguous()                 # (T,B,D)
            if vary:
                big = torch.full((x.shape[0], x.shape[1] + 2, D), float("nan"), dtype=torch.float64, device=dev)
                big[:, 1:x.shape[1] + 1] = x.double()
                x = big[:, 1:x.shape[1] + 1]
                assert not x.is_contiguous() and x.dtype == torch.float64
            xs.append(x)
        x = xs[0] if len(xs) == 1 else dict(zip(mods, xs))
        return (x,) if name == "MFN" else (x, (mask != 0) if vary else mask, LENGTHS)

    def run(vary):
        for p in model.parameters():
            p.grad = None
        y = model(*inputs(vary))
        y.backward(N("model:%s:go" % name, *y.shape).to(dev))
        torch.cuda.synchronize()
        return y.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    want = run(False)
    assert any(g is not None for g in want[1].values())
    LV.assert_same_bits(name, run(True), want)


# ---------------------------------------------------------------------------------------------------------------- the C boundary
def _c_cases(lib):
    """entry -> (its arguments in order, the names of its class (c) pointers).  An argument is ("p", name) for a device pointer or a
    plain value; every pointer gets its own zeroed buffer far larger than the small shapes below read or write, so a call is in bounds
    whether or not a pointer is moved by 4 bytes."""
    p = lambda name: ("p", name)  # noqa: E731
    B, T, d, h, f, n = 2, 5, 16, 2, 16, 1
    enc = [B, T, d, h, f, n]
    ews = lib.mmt_encoder_workspace_bytes_eval(*enc)
    lws = lib.mmt_linear_workspace_bytes(5, 4, 3)
    sws = lib.mmt_lstm_scan_workspace_bytes(16)
    mws = lib.mmt_mfn_mem_scan_workspace_bytes()
    cws, ckws = lib.mmt_convpool_workspace_bytes(3, 4, 8, 5), lib.mmt_convpool_k_workspace_bytes(3, 4, 8, 5, 3)
    pb = lib.mmt_linear_prepared_bytes(4, 3)
    eb = lib.mmt_encoder_stream_bytes(2, 4, 8, 2, 4, 1)
    i2 = lambda a, b: (ctypes.c_int * 2)(a, b)  # noqa: E731
    mD, mH = i2(4, 8), i2(4, 8)
    mb = lib.mmt_mfn_stream_bytes(2, 2, mD, mH, 1)
    db = lib.mmt_decoder_stream_bytes(2, 4, 3, 1)
    lb = lib.mmt_lstm_stream_bytes(2, 3, 5, 3, 1, 3)
    tab = lambda k: ("ptrs", k)  # noqa: E731 (a host array of k device pointers)
    return {
        "mmt_encoder_forward": ([p("x"), p("mask"), p("params"), p("y"), p("workspace"), ews] + enc + [1e-6, 0.0, 0], ["x", "params", "y"]),
        "mmt_encoder_backward": ([p("dy"), p("x"), p("mask"), p("params"), p("dx"), p("dparams"), p("workspace"), ews] + enc + [1e-6, 0.0, 0],
                                 ["dy", "x", "params", "dx"]),
        "mmt_layernorm_forward": ([p("x"), p("a_2"), p("b_2"), p("y"), p("stats"), 5, 4, 1e-6], ["x", "a_2", "b_2", "y"]),
        "mmt_layernorm_backward": ([p("dy"), p("x"), p("a_2"), p("stats"), p("dx"), p("da_2"), p("db_2"), p("scratch"), 5, 4, 1e-6], ["dy", "x", "a_2", "dx"]),
        "mmt_linear_forward": ([p("x"), p("Wt"), p("b"), p("rowscale"), p("y"), p("workspace"), lws, 5, 4, 3, 0], ["x", "y"]),
        "mmt_linear_backward": ([p("dy"), p("x"), p("Wt"), p("y"), p("rowscale"), p("dx"), p("dW"), p("db"), p("workspace"), lws, 5, 4, 3, 0], ["dx"]),
        "mmt_linear_prepare": ([p("Wt"), p("b"), p("prepared"), pb, 4, 3], ["prepared"]),
        "mmt_linear_forward_prepared": ([p("x"), p("prepared"), pb, p("rowscale"), p("y"), 5, 4, 3, 0], ["x", "prepared", "y"]),
        "mmt_lstm_scan_forward": ([p("gx"), p("W_rec"), p("h0"), p("c0"), p("h_all"), p("c_all"), p("acts"), p("workspace"), sws, 3, 2, 16],
                                  ["gx", "h0", "c0", "h_all", "c_all", "acts"]),
        "mmt_lstm_scan_backward": ([p("dh_all"), p("dc_all"), p("W_rec"), p("c0"), p("c_all"), p("acts"), p("dgx"), p("dh0"), p("dc0"), p("workspace"),
                                    sws, 3, 2, 16], ["dh_all", "dc_all", "c0", "c_all", "acts", "dgx", "dh0", "dc0"]),
        "mmt_mfn_mem_scan_forward": ([p("apre"), p("chat"), p("Wm"), p("W2"), p("b2"), p("mem_all"), p("u_all"), p("g_all"), p("workspace"), mws,
                                      3, 2, 128, 64, 0.0, 0], ["apre", "chat", "b2", "mem_all", "u_all", "g_all"]),
        "mmt_mfn_mem_scan_backward": ([p("dmem_all"), p("chat"), p("mem_all"), p("u_all"), p("g_all"), p("Wm"), p("W2"), p("dchat"), p("dapre"),
                                       p("dz_all"), p("workspace"), mws, 3, 2, 128, 64, 0.0],
                                      ["dmem_all", "chat", "mem_all", "u_all", "g_all", "dchat", "dapre", "dz_all"]),
        "mmt_convpool_forward": ([p("x"), p("weight"), p("bias"), p("out"), p("argmax"), p("workspace"), cws, 3, 4, 8, 5], ["x"]),
        "mmt_convpool_backward": ([p("x"), p("dout"), p("argmax"), p("dweight"), p("dbias"), p("workspace"), cws, 3, 4, 8, 5], ["x"]),
        "mmt_convpool_k_forward": ([p("x"), p("weight"), p("bias"), p("out"), p("argmax"), p("workspace"), ckws, 3, 4, 8, 5, 3], ["x"]),
        "mmt_convpool_k_backward": ([p("x"), p("dout"), p("argmax"), p("dweight"), p("dbias"), p("workspace"), ckws, 3, 4, 8, 5, 3], ["x"]),
        "mmt_mse_sum_forward": ([p("pred"), p("target"), 0.125, p("loss"), p("dpred"), p("scratch"), 10], ["pred", "target", "dpred"]),
        "mmt_encoder_stream_prepare": ([p("params"), p("state"), eb, 2, 4, 8, 2, 4, 1], ["state"]),
        "mmt_encoder_stream_step": ([p("x_t"), p("mask_t"), p("params"), p("y_t"), p("state"), eb, 0, 2, 4, 8, 2, 4, 1, 1e-6], ["state"]),
        "mmt_encoder_stream_step_slots": ([p("x_t"), p("mask_t"), p("params"), p("y_t"), p("state"), eb, p("pos"), 1, 2, 4, 8, 2, 4, 1, 1e-6], ["state"]),
        "mmt_mfn_stream_prepare": ([tab(8), tab(20), p("state"), mb, 2, 2, mD, mH, 1], ["state"]),
        "mmt_mfn_stream_step": ([tab(2), p("mask_t"), p("y_t"), p("state"), mb, 0, 2, 2, mD, mH, 1], ["state"]),
        "mmt_mfn_stream_step_slots": ([tab(2), p("mask_t"), p("y_t"), p("state"), mb, p("pos"), 0, 1, 2, 2, mD, mH, 1], ["state"]),
        "mmt_decoder_stream_prepare": ([tab(4), p("dec_h0"), p("dec_c0"), p("W1"), p("b1"), p("W2"), p("b2"), p("state"), db, 2, 4, 3, 1], ["state"]),
        "mmt_decoder_stream_step": ([p("e_t"), p("mask_t"), p("y_t"), p("state"), db, 0, 2, 4, 3, 1], ["state"]),
        "mmt_decoder_stream_step_slots": ([p("e_t"), p("mask_t"), p("y_t"), p("state"), db, p("pos"), 0, 1, 2, 4, 3, 1], ["state"]),
        "mmt_lstm_stream_prepare": ([tab(14), p("state"), lb, 2, 3, 5, 3, 1, 3], ["state"]),
        "mmt_lstm_stream_step": ([p("x_t"), p("mask_t"), p("y_t"), p("state"), lb, 0, 2, 3, 5, 3, 1, 3], ["state"]),
        "mmt_lstm_stream_step_slots": ([p("x_t"), p("mask_t"), p("y_t"), p("state"), lb, p("pos"), 0, 1, 2, 3, 5, 3, 1, 3], ["state"]),
    }


def test_c_boundary_refuses_a_misaligned_class_c_pointer(dev):
    """Every pointer the audit (include/mmt_hip.h, the pointer contract) classes as (c): the entry called with device memory of
    sufficient size that starts 4 bytes past a 16-byte boundary, every other argument valid, returns MMT_EINVAL before any launch and
    mmt_last_error() names the argument.  No kernel runs in this test."""
    lib = mta()._lib.load()
    room = 1 << 20                                  # bytes per pointer: every shape below needs a few KB, the encoder workspace less than this
    stream = torch.cuda.current_stream().cuda_stream
    keep, failures, checked = [], [], 0
    for entry, (args, cnames) in _c_cases(lib).items():
        assert max(a for a in args if isinstance(a, int)) < room - 64, entry
        for bad in cnames:
            argv = []
            for a in args:
                if isinstance(a, tuple) and a[0] == "p":
                    buf = torch.zeros(room, dtype=torch.uint8, device=dev)
                    keep.append(buf)
                    argv.append(buf.data_ptr() + (4 if a[1] == bad else 0))
                elif isinstance(a, tuple):
                    bufs = [torch.zeros(4096, dtype=torch.uint8, device=dev) for _ in range(a[1])]
                    keep.extend(bufs)
                    arr = (ctypes.c_void_p * a[1])(*[b.data_ptr() for b in bufs])
                    keep.append(arr)
                    argv.append(ctypes.cast(arr, ctypes.c_void_p))
                elif isinstance(a, ctypes.Array):
                    argv.append(ctypes.cast(a, ctypes.c_void_p))
                else:
                    argv.append(a)
            rc = getattr(lib, entry)(*argv, stream)
            msg = (lib.mmt_last_error() or b"").decode()
            checked += 1
            if rc != 1 or "must be 16-byte aligned" not in msg or (": %s must" % bad) not in msg:
                failures.append("%s with %s moved by 4 bytes: rc %d, %r" % (entry, bad, rc, msg))
    torch.cuda.synchronize()
    assert checked == 69 and not failures, "\n".join(failures)        # 69: the class (c) pointers of the contract, counted
    assert not any(bool(b.any()) for b in keep if isinstance(b, torch.Tensor)), "a refused call wrote device memory"


def test_local_attention_scalar_instantiation_at_the_c_boundary(dev):
    """Class (b): mmt_local_attn_* called with h, ctx, dctx and dh 4 bytes past a 16-byte boundary runs the scalar instantiation (the
    binding never does that: it aligns h and dctx first).  A different kernel, so not bit equality: both instantiations against the
    fp64 restatement of test_gpu_lstm_baselines.py at that file's LA_RTOL = 1e-5 (fp32 arithmetic only), at H = 8, where an aligned
    call moves four floats per lane."""
    from test_gpu_lstm_baselines import LA_RTOL, _local_attention_fp64
    M = mta()
    F, launch = M.functional, M._lib.launch
    B, T, H, L = 2, 5, 8, 3
    z, h, g = N("la:z", B, T, L), N("la:h8", T, B, H), N("la:g", B, T, H)
    valid = MASK().reshape(B, T)
    zd, hd = z.double().requires_grad_(), h.double().requires_grad_()
    ref = _local_attention_fp64(zd, hd, valid.double())
    ref.backward(g.double())
    nbytes = M._lib.load().mmt_local_attn_workspace_bytes(B, T, H, L)
    for name, place in (("aligned", LV.plain), ("4 bytes past", LV.offset)):
        z_, v_ = z.to(dev), valid.to(dev)
        h_, g_ = place(h.to(dev)), place(g.to(dev))
        out, dh = place(torch.zeros(B, T, H, device=dev)), place(torch.zeros(T, B, H, device=dev))
        a, dz = torch.zeros(B, T, L, device=dev), torch.zeros(B, T, L, device=dev)
        ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
        assert h_.data_ptr() % 16 == (0 if name == "aligned" else 4)
        launch("mmt_local_attn_forward", z_, h_, v_, out, a, B, T, H, L)
        launch("mmt_local_attn_backward", g_, a, h_, v_, dz, dh, ws, nbytes, B, T, H, L)
        torch.cuda.synchronize()
        for what, got, want in (("ctx", out, ref), ("dz", dz, zd.grad), ("dh", dh, hd.grad)):
            e = rel_l2(got.cpu().numpy(), want.detach().numpy())
            print("local attention, h / ctx / dctx / dh %s: %s rel-L2 %.2e" % (name, what, e))
            assert e < LA_RTOL, (name, what, e)
