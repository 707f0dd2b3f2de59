"""No result depends on a workspace's past (include/mmt_hip.h, the workspace paragraph; _lib.WorkspacePool).

Every other GPU test compares a call with a reference.  Here a call is compared with THE SAME CALL on a workspace that something else
has used, bit for bit (torch.equal on every output and every gradient, and every one of them finite): no tolerance, no reference.

1. Entries that take memory with any contents (lstm_scan, mfn_mem_scan, conv_maxpool / conv_maxpool_k: functional._scratch; the
   backward of local_attention: a pool buffer documented "any contents").  The memory is handed over filled with 0x00, with 0xFF (a NaN
   in fp32 and in bf16) and with the 16-bit word 0x7F80 (+Inf in bf16: a kernel that masks by multiplying with 0 makes a NaN of it); the
   three runs must agree.  Each case asserts that its forward and its backward took such memory at all.
2. Entries under "zero once, then reuse for the same shape" (encoder_stack, sdpa, linear, linear_pair, highway, mfn_gate,
   lstm_stack_scan, lstm_fb_scan).  A probe call runs on a cleared pool, and again after a dirtier with the same pool tag has used and
   returned the buffers; gpu_harness.PoolRecorder proves that the second probe was handed the dirtier's buffers, and that the dirtier
   had left other bytes in them than a clean run leaves.  Every case prints how many buffers it reused.  Dirtiers:
     other user: inputs x 1e3 with every window valid, the other attention forms (plain / keyed / causal), other weights for the
                 affine maps and the scans, another seed and another dropout probability (> 0 where the probe's is, the tag carries the train flag), at d = 128 the other seed kind;
     bad batch:  the probe's own call with NaN and +-Inf among its inputs — what one bad batch of a training run leaves behind.
   The stacked and the feedback scans' tags carry (H, L) / (H, E) only, so their dirtier has a larger B and a longer T than the probe.
   Two encoder shapes whose workspaces have the same number of bytes (WorkspacePool.get's docstring) must not be handed each other's.
Nothing here hands a zero-contract entry a workspace that breaks the contract.
"""
import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import FILLS, FilledPoolGet, FilledScratch, PoolRecorder, dev, mta, same_bits  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu
SEED = 41


def _n(tag, shape, scale=1.0):
    return scale * R.gen_normal("wsstate:" + tag, shape, SEED)


def _leaf(t, dev):
    return None if t is None else t.to(dev).requires_grad_()


def _grads(names, leaves):
    return {"d" + n: (None if t is None else t.grad) for n, t in zip(names, leaves)}


# ================================================================================================ 1. any contents
def _three_fills(monkeypatch, tag, call, make=FilledScratch, install=None):
    """call(counter) once per fill of the substituted memory -> the three results agree bit for bit"""
    F, L = mta().functional, mta()._lib
    runs = {}
    for fill in FILLS:
        L.POOL.clear()
        counter = make(fill)
        (install or (lambda c: monkeypatch.setattr(F, "_scratch", c)))(counter)
        runs[fill] = call(counter)
        F.check_device_errors()
    failures = []
    for fill in FILLS[1:]:
        same_bits("%s: %s against zeros" % (tag, fill), runs["zeros"], runs[fill], failures)
    assert not failures, "\n".join(failures)


def _took(counter, what):
    n = counter.took()
    assert n > 0, "%s took no substituted memory: the case checks nothing" % what
    return n


def lstm_family(B, H):
    """plan_lstm_scan of csrc/api.hip (tests/test_gpu_bf16_scans.py lstm_family)"""
    hp16 = -(-H // 16) * 16
    bt = 1
    while bt < 16 and -(-B // bt) > 256:
        bt *= 2
    if hp16 > 128 and B <= 32:
        return "cluster"
    if hp16 > 128 and bt == 1:
        return "scan256"
    return "units" if bt <= 2 else "general"


# (family, T, B, H); 132: scan256's ragged last tile, which reads the workspace rows behind the weights (dead results)
_LSTM = [("general", 3, 513, 40), ("units", 5, 3, 40), ("units", 5, 3, 128), ("scan256", 5, 33, 256), ("scan256", 6, 40, 132),
         ("cluster", 5, 3, 256)]


@pytest.mark.parametrize("init", [True, False], ids=["h0c0", "none"])
@pytest.mark.parametrize("fam,T,B,H", _LSTM, ids=["%s_T%d_B%d_H%d" % c for c in _LSTM])
def test_lstm_scan_any_contents(dev, monkeypatch, fam, T, B, H, init):
    F = mta().functional
    assert lstm_family(B, H) == fam
    tag = "lstm_scan %s T%d B%d H%d" % (fam, T, B, H)
    gx, W = _n(tag + "gx", (T, B, 4 * H)), _n(tag + "w", (4 * H, H)) / np.sqrt(H)
    h0, c0 = (_n(tag + "h0", (B, H), 0.5), _n(tag + "c0", (B, H), 0.5)) if init else (None, None)
    gh, gc = _n(tag + "gh", (T, B, H)).to(dev), _n(tag + "gc", (T, B, H)).to(dev)

    def call(s):
        leaves = [_leaf(t, dev) for t in (gx, W, h0, c0)]
        h, c = F.lstm_scan(*leaves)
        _took(s, tag + " forward")
        ((h * gh).sum() + (c * gc).sum()).backward()
        _took(s, tag + " backward")
        return dict(h=h.detach(), c=c.detach(), **_grads(("gx", "W", "h0", "c0"), leaves))
    _three_fills(monkeypatch, tag, call)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("T,B", [(20, 3), (6, 300)])
def test_mfn_mem_scan_any_contents(dev, monkeypatch, T, B, p):
    F = mta().functional
    tag = "mfn_mem_scan T%d B%d p%g" % (T, B, p)
    apre, chat = _n(tag + "a", (T, B, 128)), torch.tanh(_n(tag + "c", (T, B, 128)))
    Wm, W2, b2 = _n(tag + "wm", (128, 128)) / np.sqrt(128), _n(tag + "w2", (2, 128, 64)) / 8, _n(tag + "b2", (2, 128), 0.1)
    g = _n(tag + "g", (T, B, 128)).to(dev)

    def call(s):
        leaves = [_leaf(t, dev) for t in (apre, chat, Wm, W2, b2)]
        mem = F.mfn_mem_scan(*leaves, dropout_p=p, seed=4242 + T)
        _took(s, tag + " forward")
        (mem * g).sum().backward()
        _took(s, tag + " backward")
        return dict(mem=mem.detach(), **_grads(("apre", "chat", "Wm", "W2", "b2"), leaves))
    _three_fills(monkeypatch, tag, call)


@pytest.mark.parametrize("wide", [False, True], ids=["W=K+1", "W=40"])
@pytest.mark.parametrize("K", [2, 1, 3, 5])
def test_conv_maxpool_any_contents(dev, monkeypatch, K, wide):
    """K = 2: conv_maxpool (convpool.h), the others conv_maxpool_k (convk.h); W = K + 1 and W = 40 are the two instances of either
    backward; D = 36 pads DP and DPB, F = 70 ends in a remainder block of filters"""
    F = mta().functional
    N, W, D, Fo = 7, (40 if wide else K + 1), 36, 70
    tag = "conv K%d W%d" % (K, W)
    x = _n(tag + "x", (N, W, D)).to(dev)
    w, b, g = _n(tag + "w", (Fo, D, K)) / np.sqrt(D * K), _n(tag + "b", (Fo,), 0.1), _n(tag + "g", (N, Fo)).to(dev)

    def call(s):
        leaves = [_leaf(t, dev) for t in (w, b)]
        out, arg = (F.conv_maxpool if K == 2 else F.conv_maxpool_k)(x, *leaves)
        _took(s, tag + " forward")
        (out * g).sum().backward()
        _took(s, tag + " backward")
        return dict(out=out.detach(), arg=arg, **_grads(("w", "b"), leaves))
    _three_fills(monkeypatch, tag, call)


def test_local_attention_backward_any_contents(dev, monkeypatch):
    """mmt_local_attn_backward takes a POOL buffer and documents "any contents": the fill goes in at the pool"""
    F, L = mta().functional, mta()._lib
    B, T, H, Lt = 3, 37, 130, 5
    tag = "local_attention"
    z, h = _n(tag + "z", (B, T, Lt)), _n(tag + "h", (T, B, H))
    valid, g = R.prefix_mask([37, 20, 1], T).to(dev), _n(tag + "g", (B, T, H)).to(dev)

    def call(f):
        leaves = [_leaf(t, dev) for t in (z, h)]
        out = F.local_attention(*leaves, valid)
        (out * g).sum().backward()
        assert f.calls > 0, "the backward took no pool buffer tagged local_attn: the case checks nothing"
        return dict(out=out.detach(), **_grads(("z", "h"), leaves))
    real = L.POOL.get
    _three_fills(monkeypatch, tag, call, make=lambda fill: FilledPoolGet(real, fill, "local_attn"),
                 install=lambda f: monkeypatch.setattr(L.POOL, "get", f))


# ================================================================================================ 2. zero once, then reuse
def _pooled(monkeypatch, tag, probe, dirtiers, tags=None):
    """probe() on a cleared pool, then after each dirtier on the buffers that dirtier handed back: the same bits"""
    F, L = mta().functional, mta()._lib
    rec = PoolRecorder(L.POOL, monkeypatch)
    L.POOL.clear()
    rec.phase("fresh")
    fresh = probe()
    F.check_device_errors()
    rec.assert_fresh(tags=tags)
    failures = []
    for name, dirtier in dirtiers:
        L.POOL.clear()
        rec.phase("dirtier")
        dirtier()
        torch.cuda.synchronize()
        nd = rec.assert_dirtied(tags=tags)          # before the probe writes the same buffers
        rec.phase("probe")
        dirty = probe()
        F.check_device_errors()
        n = rec.assert_reused(tags=tags)
        print("%-60s after %-22s reused %d workspace(s), %d left with other bytes" % (tag, name, n, nd))
        same_bits("%s after %s" % (tag, name), fresh, dirty, failures)
    assert not failures, "\n".join(failures)


def _poison(t):
    """a few NaN and +-Inf entries, spread over the tensor (the first and the last row included)"""
    t = t.clone()
    flat = t.view(-1)
    n = flat.numel()
    for i, v in zip((0, n // 7, n // 3, n // 2 + 1, (2 * n) // 3, n - 1), (float("nan"), float("inf"), -float("inf")) * 2):
        flat[i] = v
    return t


FORMS = ("plain", "keyed", "causal")


def _form_args(form, lengths, dev):
    return dict(key_lengths=torch.tensor(lengths, dtype=torch.int32, device=dev) if form == "keyed" else None, causal=form == "causal")


# ------------------------------------------------------------------------------------------------ encoder_stack
# (d, h, n, B, T, lengths, [(p, seed kind)]): every pad at once (DP, FP, DKP, Tp, rows >= M); the fixed-shape chains, the riding generator
# and the folded final norm, with both seed kinds; the wide instance; the one-kernel backward over several tiles, where the keyed form
# skips whole 128-key workgroups
_ENC = [(40, 4, 2, 3, 70, [70, 33, 1], [(0.0, "host"), (0.25, "host")]),
        (128, 8, 2, 3, 70, [70, 33, 1], [(0.0, "host"), (0.1, "host"), (0.1, "dev")]),
        (256, 8, 1, 2, 45, [45, 1], [(0.0, "host"), (0.1, "host")]),
        (128, 8, 1, 2, 300, [300, 40], [(0.0, "host"), (0.1, "host")])]
ENC_CASES = [(c[:6], p, kind, form) for c in _ENC for p, kind in c[6] for form in FORMS]
ENC_IDS = ["d%d_n%d_T%d_p%g_%s_%s" % (c[0], c[2], c[4], p, kind, form) for c, p, kind, form in ENC_CASES]


@pytest.mark.parametrize("c,p,kind,form", ENC_CASES, ids=ENC_IDS)
def test_encoder_stack_on_a_used_workspace(dev, monkeypatch, c, p, kind, form):
    F, L = mta().functional, mta()._lib
    d, h, n, B, T, lengths = c
    tag = "encoder d%d n%d T%d" % (d, n, T)
    flat = torch.cat([t.reshape(-1) for t in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), SEED).values()])
    x, g, mask = _n(tag + "x", (B, T, d)), _n(tag + "g", (B, T, d)).to(dev), R.prefix_mask(lengths, T).to(dev)
    ones = torch.ones_like(mask)

    def run(x_, mask_, form_, lengths_, p_, seed, kind_):
        xg, fl = _leaf(x_, dev), _leaf(flat, dev)
        sd = L.DeviceSeed(dev, seed) if kind_ == "dev" else seed
        y = F.encoder_stack(xg, mask_, fl, h, R.D_FF, n, dropout_p=p_, seed=sd, **_form_args(form_, lengths_, dev))
        y.backward(g)
        return dict(y=y.detach(), dx=xg.grad, dflat=fl.grad)

    def other(form_):        # the other seed kind where the shape has both
        kind_ = kind if (d, n) != (128, 2) or p == 0 else ("dev" if kind == "host" else "host")
        return lambda: run(1e3 * x, ones, form_, [T] * B, 0.3 if p > 0 else 0.0, 90210, kind_)
    dirtiers = [("other user, " + f, other(f)) for f in FORMS if f != form]
    dirtiers.append(("bad batch", lambda: run(_poison(x), mask, form, lengths, p, 777, kind)))
    _pooled(monkeypatch, "%s p%g %s %s" % (tag, p, kind, form), lambda: run(x, mask, form, lengths, p, 777, kind), dirtiers)


# ------------------------------------------------------------------------------------------------ sdpa
# (d_k, B, T, lengths) at h = 2
_SDPA = [(10, 3, 70, [70, 33, 1]), (16, 3, 70, [70, 33, 1]), (64, 3, 70, [70, 33, 1]), (16, 2, 300, [300, 40])]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dk,B,T,lengths", _SDPA, ids=["dk%d_T%d" % (c[0], c[2]) for c in _SDPA])
def test_sdpa_on_a_used_workspace(dev, monkeypatch, dk, B, T, lengths, p, form):
    F = mta().functional
    h = 2
    tag = "sdpa dk%d T%d" % (dk, T)
    q, k, v = (_n(tag + s, (B, T, h * dk)) for s in "qkv")
    g, mask = _n(tag + "g", (B, T, h * dk)).to(dev), R.prefix_mask(lengths, T).to(dev)
    ones = torch.ones_like(mask)

    def run(qkv, mask_, form_, lengths_, p_, seed):
        leaves = [_leaf(t, dev) for t in qkv]
        out = F.sdpa(*leaves, mask_, h, p_, seed, **_form_args(form_, lengths_, dev))
        out.backward(g)
        return dict(out=out.detach(), **_grads("qkv", leaves))
    dirtiers = [("other user, " + f, lambda f=f: run([1e3 * t for t in (q, k, v)], ones, f, [T] * B, 0.3 if p > 0 else 0.0, 90210))
                for f in FORMS if f != form]
    dirtiers.append(("bad batch", lambda: run([_poison(t) for t in (q, k, v)], mask, form, lengths, p, 777)))
    _pooled(monkeypatch, "%s p%g %s" % (tag, p, form), lambda: run((q, k, v), mask, form, lengths, p, 777), dirtiers)


# ------------------------------------------------------------------------------------------------ the affine maps
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("scaled", [False, True], ids=["norowscale", "rowscale"])
@pytest.mark.parametrize("M,K,N", [(70, 300, 96), (33, 43, 129)])
def test_linear_on_a_used_workspace(dev, monkeypatch, M, K, N, scaled, drop):
    F = mta().functional
    tag = "linear %dx%dx%d" % (M, K, N)
    x, W, b = _n(tag + "x", (M, K)), _n(tag + "w", (N, K)) / np.sqrt(K), _n(tag + "b", (N,), 0.1)
    r, g = torch.rand(M, generator=torch.Generator().manual_seed(SEED)).to(dev), _n(tag + "g", (M, N)).to(dev)

    def run(x_, W_, rowscale, pin, pout, seed):
        leaves = [_leaf(t, dev) for t in (x_, W_, b)]
        y = F.linear(*leaves, act=1, rowscale=r if rowscale else None, in_dropout=pin, out_dropout=pout, seed=seed)
        y.backward(g)
        return dict(y=y.detach(), **_grads(("x", "W", "b"), leaves))
    pin, pout = (0.1, 0.2) if drop else (0.0, 0.0)
    dirtiers = [("other user", lambda: run(1e3 * x, -W, not scaled, 0.3, 0.4, 90210)),
                ("bad batch", lambda: run(_poison(x), W, scaled, pin, pout, 777))]
    _pooled(monkeypatch, "%s %s %s" % (tag, "rowscale" if scaled else "plain", "drop" if drop else "eval"),
            lambda: run(x, W, scaled, pin, pout, 777), dirtiers)


def test_linear_pair_on_a_used_workspace(dev, monkeypatch):
    F = mta().functional
    M, K, N1, N2 = 33, 44, 96, 129
    tag = "linear_pair"
    x, W1, b1, W2, b2 = (_n(tag + "x", (M, K)), _n(tag + "w1", (N1, K)) / np.sqrt(K), _n(tag + "b1", (N1,), 0.1),
                         _n(tag + "w2", (N2, K)) / np.sqrt(K), _n(tag + "b2", (N2,), 0.1))
    g1, g2 = _n(tag + "g1", (M, N1)).to(dev), _n(tag + "g2", (M, N2)).to(dev)

    def run(x_, sign=1.0):
        leaves = [_leaf(t, dev) for t in (x_, sign * W1, b1, sign * W2, b2)]
        y1, y2 = F.linear_pair(*leaves, act1=1, act2=2)
        ((y1 * g1).sum() + (y2 * g2).sum()).backward()
        return dict(y1=y1.detach(), y2=y2.detach(), **_grads(("x", "W1", "b1", "W2", "b2"), leaves))
    _pooled(monkeypatch, tag, lambda: run(x), [("other user", lambda: run(1e3 * x, -1.0)), ("bad batch", lambda: run(_poison(x)))])


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_highway_on_a_used_workspace(dev, monkeypatch, p):
    F = mta().functional
    M, K = 33, 40
    tag = "highway"
    x, Wp, bp, Wg, bg = (_n(tag + "x", (M, K)), _n(tag + "wp", (K, K)) / np.sqrt(K), _n(tag + "bp", (K,), 0.1),
                         _n(tag + "wg", (K, K)) / np.sqrt(K), _n(tag + "bg", (K,), 0.1))
    g = _n(tag + "g", (M, K)).to(dev)

    def run(x_, p_, seed, sign=1.0):
        leaves = [_leaf(t, dev) for t in (x_, sign * Wp, bp, sign * Wg, bg)]
        y = F.highway(*leaves, dropout_p=p_, seed=seed)
        y.backward(g)
        return dict(y=y.detach(), **_grads(("x", "Wp", "bp", "Wg", "bg"), leaves))
    _pooled(monkeypatch, "%s p%g" % (tag, p), lambda: run(x, p, 777),
            [("other user", lambda: run(1e3 * x, 0.5 if p > 0 else 0.0, 90210, -1.0)), ("bad batch", lambda: run(_poison(x), p, 777))])


# ------------------------------------------------------------------------------------------------ mfn_gate
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_mfn_gate_on_used_workspaces(dev, monkeypatch, train):
    """seven pooled workspaces (the gate's affine maps) held from the forward to the backward; other user only"""
    F = mta().functional
    T, B, Hs, MD, HG = 20, 3, [88, 16], 128, 64
    SH = sum(Hs)
    A = 2 * SH
    tag = "mfn_gate"
    shapes = [(128, A), (A, 128), (256, A), (MD, 256), (HG, A + MD), (MD, HG), (HG, A + MD), (MD, HG), (64, SH + MD), (1, 64)]
    params = []
    for i, (o, k) in enumerate(shapes):
        params += [_n(tag + "w%d" % i, (o, k)) / np.sqrt(k), _n(tag + "b%d" % i, (o,), 0.1)]
    hs = [torch.tanh(_n(tag + "h%d" % i, (T, B, H))) for i, H in enumerate(Hs)]
    cs = [_n(tag + "c%d" % i, (T, B, H)) for i, H in enumerate(Hs)]
    g = _n(tag + "g", (T, B, 1)).to(dev)

    def run(scale, pg, sg, po, so):
        lh, lc, lp = ([_leaf(scale * t, dev) for t in hs], [_leaf(scale * t, dev) for t in cs],
                      [_leaf(t if scale == 1.0 else -t, dev) for t in params])        # another user: other weights as well
        out = F.mfn_gate(lh, lc, lp, pg, sg, po, so)
        (out * g).sum().backward()
        names = ["h%d" % i for i in range(len(Hs))] + ["c%d" % i for i in range(len(Hs))] + ["p%d" % i for i in range(len(lp))]
        return dict(out=out.detach(), **_grads(names, lh + lc + lp))
    mine, theirs = ((0.2, 1001, 0.5, 1002), (0.3, 2001, 0.4, 2002)) if train else ((0.0, 0, 0.0, 0),) * 2
    _pooled(monkeypatch, "%s %s" % (tag, "train" if train else "eval"), lambda: run(1.0, *mine), [("other user", lambda: run(1e3, *theirs))])


# ------------------------------------------------------------------------------------------------ the stacked and the feedback scans
def test_lstm_stack_scan_after_another_shape(dev, monkeypatch):
    """the tag is (H, L): a call with another T and B uses the same buffer.  Probe: H = 40, L = 3, T = 7, B = 2 (stacked_cases.py
    model_sft_l3_d40); dirtier: T = 12, B = 5, inputs x 1e3.  Only the buffers tagged lstm_stack are held to reuse: the weight-gradient
    GEMMs behind the scan are tagged by their own shapes, which differ with T * B (test_linear_on_a_used_workspace holds those)."""
    F = mta().functional
    H, Lyr = 40, 3
    tag = "lstm_stack_scan"
    P, bias = _n(tag + "P", (Lyr, 4 * H, 2 * H)) / np.sqrt(2 * H), _n(tag + "b", (Lyr - 1, 4 * H), 0.1)

    def run(T, B, scale):
        t2 = "%s%dx%d" % (tag, T, B)
        gx0, h0, c0 = _n(t2 + "gx", (T, B, 4 * H), scale), _n(t2 + "h0", (Lyr, B, H), 0.5 * scale), _n(t2 + "c0", (Lyr, B, H), 0.5 * scale)
        leaves = [_leaf(t, dev) for t in (gx0, P if scale == 1.0 else -P, bias, h0, c0)]      # another user: other weights as well
        h_top, h_all, c_all = F.lstm_stack_scan(*leaves, return_states=True)
        (h_top * _n(t2 + "g", (T, B, H)).to(dev)).sum().backward()
        return dict(h_top=h_top.detach(), h_all=h_all, c_all=c_all, **_grads(("gx0", "P", "bias", "h0", "c0"), leaves))
    _pooled(monkeypatch, tag, lambda: run(7, 2, 1.0), [("other shape", lambda: run(12, 5, 1e3))], tags={"lstm_stack"})


def test_lstm_fb_scan_after_another_shape(dev, monkeypatch):
    """the tag is (H, E).  Probe: H = 40, E = 24, T = 7, B = 2 (edlstm_cases.py lstm_ed_h40); dirtier: T = 12, B = 5, inputs x 1e3.
    Only the buffers tagged lstm_fb are held to reuse (see test_lstm_stack_scan_after_another_shape)."""
    F = mta().functional
    H, Eo = 40, 24
    tag = "lstm_fb_scan"
    w_p, W_hh = _n(tag + "wp", (4 * H,), 0.3), _n(tag + "whh", (4 * H, H)) / np.sqrt(H)
    W1, b1, w2, b2 = _n(tag + "w1", (Eo, H)) / np.sqrt(H), _n(tag + "b1", (Eo,), 0.1), _n(tag + "w2", (Eo,)) / np.sqrt(Eo), _n(tag + "b2", (1,), 0.1)

    def run(T, B, scale):
        t2 = "%s%dx%d" % (tag, T, B)
        gxc, h0, c0 = _n(t2 + "gx", (T, B, 4 * H), scale), _n(t2 + "h0", (B, H), 0.5 * scale), _n(t2 + "c0", (B, H), 0.5 * scale)
        sign = 1.0 if scale == 1.0 else -1.0        # another user: other weights as well
        leaves = [_leaf(t, dev) for t in (gxc, w_p, sign * W_hh, sign * W1, b1, w2, b2, h0, c0)]
        p_all, h_all, c_all, u_all = F.lstm_fb_scan(*leaves, p_init=0.5, return_states=True)
        (p_all * _n(t2 + "g", (T, B)).to(dev)).sum().backward()
        return dict(p=p_all.detach(), h=h_all, c=c_all, u=u_all,
                    **_grads(("gxc", "w_p", "W_hh", "W1", "b1", "w2", "b2", "h0", "c0"), leaves))
    _pooled(monkeypatch, tag, lambda: run(7, 2, 1.0), [("other shape", lambda: run(12, 5, 1e3))], tags={"lstm_fb"})


# ------------------------------------------------------------------------------------------------ equal bytes, another layout
@pytest.mark.parametrize("n,p,first,second", [(2, 0.0, (4, 50), (2, 100)), (1, 0.1, (1, 200), (2, 100))], ids=["eval_n2", "train_n1"])
def test_encoder_shapes_with_equal_bytes_do_not_share(dev, monkeypatch, n, p, first, second):
    """WorkspacePool.get's docstring: two encoder shapes with B * T = 200 whose workspaces have the same number of bytes and another
    layout inside.  The second shape, run after the first, must be handed a buffer of its own and compute what it computes alone."""
    F, L = mta().functional, mta()._lib
    d, h = 128, 8
    nbytes = L.load().mmt_encoder_workspace_bytes if p > 0 else L.load().mmt_encoder_workspace_bytes_eval
    assert nbytes(*first, d, h, R.D_FF, n) == nbytes(*second, d, h, R.D_FF, n), "these shapes no longer collide: find another pair"
    flat = torch.cat([t.reshape(-1) for t in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), SEED).values()])

    def run(B, T, scale):
        tag = "collide%dx%d" % (B, T)
        xg, fl = _leaf(_n(tag + "x", (B, T, d), scale), dev), _leaf(flat, dev)
        mask = R.prefix_mask([T] + [1 + (7 * i) % T for i in range(1, B)], T).to(dev)
        y = F.encoder_stack(xg, mask, fl, h, R.D_FF, n, dropout_p=p, seed=777)
        y.backward(_n(tag + "g", (B, T, d)).to(dev))
        return dict(y=y.detach(), dx=xg.grad, dflat=fl.grad)
    rec = PoolRecorder(L.POOL, monkeypatch)
    L.POOL.clear()
    rec.phase("fresh")
    fresh = run(*second, 1.0)
    F.check_device_errors()
    rec.assert_fresh()
    L.POOL.clear()
    rec.phase("first")
    run(*first, 1e3)
    rec.phase("second")
    after = run(*second, 1.0)
    F.check_device_errors()
    assert rec.log["first"]["put"], "the first shape handed no workspace back"
    rec.assert_fresh(phase="second")                # handed nothing of the first shape's
    failures = []
    same_bits("encoder %s after %s" % (second, first), fresh, after, failures)
    assert not failures, "\n".join(failures)
