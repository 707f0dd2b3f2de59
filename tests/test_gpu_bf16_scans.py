"""The LSTM and MFN memory scans against the bf16-faithful fp64 reference (tests/bf16_ref.py lstm_scan / mfn_mem_scan).

test_gpu_models.py checks the scans against a plain fp64 loop with one rel-L2 over the whole tensor, 2e-2 on outputs and 4e-2 / 9e-2 on
gradients.  One wrong sequence of a few hundred, a few wrong time steps or one wrong 16-unit tile pass that.  Here the reference rounds
where the kernels round, so the bounds sit one to two orders of magnitude lower, and every tensor is measured four ways:
  * rel-L2 of the tensor;
  * the per-row maximum (gpu_harness.measures): a row is one (t, b) for h, c, dgx, mem, dapre and dchat, one sequence for
    dh0 and dc0, one output feature for the weight gradients, one entry for db2;
  * the per-sequence maximum  max_b ||got[:, b] - ref[:, b]|| / rms_b ||ref[:, b]||  of the (T, B, .) tensors;
  * the least-squares scale <got - ref, ref> / <ref, ref> of the weight gradients.

Every dispatch branch of plan_lstm_scan (one plan for mmt_lstm_scan_forward and _backward) and of mmt_mfn_mem_scan_forward / _backward
(csrc/api.hip) has cases, and each
case asserts through torch.profiler that the kernel it is labelled for ran.  The four-CU scans (scan_cluster.h) run once more under
MMT_NO_CLUSTER_SCAN=1, where the same shapes go to scan256.h; those results are checked against the reference and against the four-CU
ones.  The switch is read once per process, so all GPU work happens in child processes (gpu_harness.run_child, which calls child_main
below) that hand their arrays back through an .npz file.  The measures (check_scan over check, seq_max and ls_scale) are gpu_harness's.
"""
import json
import re

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import check_scan, device_kernel_names, run_child, tmp_dir  # noqa: F401 (tmp_dir: a fixture)

pytestmark = pytest.mark.gpu

# Bounds: about 4x the worst value measured on the MI355X over every case and switch set, which the comments give as rel-L2 / per-row
# maximum / per-sequence maximum.  None is below what fp32-level noise does to the reference itself (tests/test_bf16_ref.py
# test_scan_jitter_floor: at T = 1000, H = 256 it moves h by 1.8e-4 / 4.7e-4 / 1.8e-4, dgx by 2.9e-4 / 7.9e-4 / 3.0e-4, dW by 1.1e-3 /
# 2.6e-3).
LSTM_OUT = (7e-4, 2e-3, 1e-3)          # h and c: 1.7e-4 / 4.8e-4 / 2.5e-4
LSTM_DGX = (1.2e-3, 5e-3, 1.5e-3)      # 2.8e-4 / 1.2e-3 / 3.5e-4
# dW per output feature measured 6.8e-3 (T = 12, B = 6, H = 256): with only T B = 72 terms per entry one tipped bf16(dG) is a visible
# share of a row, and the reference moves itself by 3.4e-3 per row there under fp32-level noise.  So this row bound is only 1.6x under
# test_gpu_models' 4e-2; the least-squares scale (LSTM_W_SCALE) is what sees a wrongly scaled weight gradient.
LSTM_DW = (4e-3, 2.5e-2)               # 1.06e-3 / 6.8e-3
LSTM_D0 = (2.5e-3, 8e-3)               # dh0, dc0 (a row is a sequence): 5.9e-4 / 2.0e-3
LSTM_W_SCALE = 3e-5                    # 6.8e-6 (noise on the reference: 5.9e-6)
# The MFN memory scan in three tiers.  B = 1 and T <= 3: no rounding tips, the kernels agree to fp32 (measured 6.6e-8 on everything).
MFN_EXACT = {n: (3e-7, 3e-7, 3e-7) for n in ("mem", "dapre", "dchat", "dWm", "dW2", "db2")}
MFN_SHORT = {"mem": (4e-5, 1.6e-3, 7e-4),          # T <= 6: 1.0e-5 / 4.0e-4 / 1.8e-4
             "dapre": (1e-3, 1.1e-2, 5.5e-3),      # 2.3e-4 / 2.7e-3 / 1.4e-3
             "dchat": (1e-3, 1.1e-2, 5.5e-3),      # 5.7e-5 / 5.0e-4 / 3.0e-4
             "dWm": (1.6e-3, 1.2e-2), "dW2": (1.6e-3, 1.2e-2), "db2": (1.6e-3, 1.2e-2)}     # 4.1e-4 / 3.1e-3
# T = 300 and 1000: every bf16(mem) that fp32 noise tips moves some pre-activation near 0 across the ReLU, and the flipped unit's whole
# gradient lands in one entry of dapre.  Over hundreds of steps this is the error: the reference moves ITSELF by 2.0e-2 rel-L2 on
# dapre and dWm, 0.38 per row of dapre, 2.5e-2 per sequence and 8.7e-2 per row of dWm under noise of half an fp32 ulp
# (test_scan_jitter_floor), what the kernels measure (1.7e-2 / 0.44 / 2.7e-2 / 8.7e-2).  No per-row bound on those; their rel-L2 and
# per-sequence bounds sit at 2.5x the worst of reference-vs-itself and kernel, under test_gpu_models' 9e-2 but not 10x under: that floor
# forbids it.
MFN_LONG = {"mem": (2e-3, 6e-3, 2e-3),             # 3.6e-4 / 1.5e-3 / 5.1e-4 (the reference against itself: 4.7e-4 / 1.6e-3 / 5.1e-4)
            "dapre": (5e-2, None, 7e-2),           # 1.7e-2 / 0.44 / 2.7e-2
            "dchat": (1.2e-2, None, 2e-2),         # 2.8e-3 / 5.9e-2 / 4.7e-3
            "dWm": (5e-2, None),                   # 1.7e-2 / 8.7e-2
            "dW2": (1.4e-2, 4e-2), "db2": (1.4e-2, 4e-2)}   # 3.5e-3 / 1.0e-2
MFN_W_SCALE = 6e-4                     # 1.5e-4 (dWm at T = 300)


def mfn_bounds(c):
    return MFN_EXACT if c["B"] == 1 and c["T"] <= 3 else MFN_SHORT if c["T"] <= 6 else MFN_LONG


# ------------------------------------------------------------------------------------------------ dispatch (csrc/api.hip)
def scan_bt(B):
    """sequences per scan workgroup (api.hip scan_bt)"""
    bt = 1
    while bt < 16 and -(-B // bt) > 256:
        bt *= 2
    return bt


def lstm_family(B, H, no_cluster=False):
    """the LSTM scan variant plan_lstm_scan (csrc/api.hip: the one decision both scans dispatch from) chooses on an MI355X: cl4
    (scan_cluster.h), s256 (scan256.h), u1 / u2 (scan_units.h, one / two sequences per workgroup) or gen (scan.h)"""
    hp16 = -(-H // 16) * 16
    hpad = 64 if hp16 <= 64 else 128 if hp16 <= 128 else 256
    bt = scan_bt(B)
    if hpad == 256 and B <= 32 and not no_cluster:
        return "cl4"
    if hpad == 256 and bt == 1:
        return "s256"
    return "u1" if bt == 1 else "u2" if bt == 2 else "gen"


def mfn_family(B):
    bt = scan_bt(B)
    return "sw1" if bt == 1 else "sw2" if bt == 2 else "gen"


_KNAME = re.compile(r"(lstm_scan_(?:fwd|bwd)\w*?_kernel|mfn_mem_scan_(?:fwd|bwd)\w*?_kernel)(<[^>]*>)?")
_LABEL = {"lstm_scan_fwd_cl4_kernel": "cl4", "lstm_scan_bwd_cl4_kernel": "cl4", "lstm_scan_fwd256_kernel": "s256",
          "lstm_scan_bwd256_kernel": "s256", "lstm_scan_fwd_u_kernel": "u", "lstm_scan_bwd_u_kernel": "u",
          "lstm_scan_fwd_kernel": "gen", "lstm_scan_bwd_kernel": "gen", "mfn_mem_scan_fwd_sw_kernel": "sw",
          "mfn_mem_scan_bwd_sw_kernel": "sw", "mfn_mem_scan_fwd_kernel": "gen", "mfn_mem_scan_bwd_kernel": "gen"}


def ran(names):
    """{"fwd": label, "bwd": label} of the scan kernels in a list of device kernel names: u1 / u2 and sw1 / sw2 carry the sequences
    per workgroup (the last template argument) when the name shows it, else just u / sw"""
    out = {}
    for n in names:
        m = _KNAME.search(n)
        if not m:
            continue
        lab = _LABEL[m.group(1)]
        if lab in ("u", "sw") and m.group(2):
            lab += m.group(2)[1:-1].split(",")[-1].strip()
        out.setdefault("fwd" if "_fwd" in m.group(1) else "bwd", set()).add(lab)
    return out


def check_ran(tag, names, family):
    if names is None:
        return                              # the profiler reports no device kernels on this box: only this assertion is skipped
    got = ran(names)
    for d in ("fwd", "bwd"):
        labs = got.get(d, set())
        assert len(labs) == 1, "%s: %s scan kernels %s (%s)" % (tag, d, sorted(labs), names)
        lab = next(iter(labs))
        assert lab == family or (lab in ("u", "sw") and family.startswith(lab)), "%s: ran %s, labelled %s" % (tag, lab, family)


# ------------------------------------------------------------------------------------------------ cases
def _lstm_case(T, B, H, init, grad="hc", gs=1.0, note=""):
    cid = "l%s_T%d_B%d_H%d_%s_%s%s" % (note, T, B, H, "i" if init else "n", grad, "_x%g" % gs if gs != 1.0 else "")
    return {"id": cid, "T": T, "B": B, "H": H, "init": init, "grad": grad, "gs": gs}


_LSTM_ROWS = [
    # units, one sequence per workgroup: H = 4 (12 of 16 tile units are padding), 20 (ragged), B = 256 the last of this path
    (9, 3, 4, True), (13, 5, 20, False), (7, 64, 64, True), (6, 256, 88, False), (5, 17, 128, True),
    # units, two per workgroup: 257 ends in a one-sequence workgroup, 301 odd, 512 the last of this path; H = 132 and 256 at HPAD = 256
    (6, 257, 48, True), (5, 301, 100, False), (4, 512, 132, True), (3, 301, 256, False),
    # general kernel: 4 and 8 sequences per workgroup, HPAD = 256 (B = 700, H = 200), 16 per workgroup (B = 2100)
    (4, 513, 64, True), (3, 1100, 64, False), (4, 513, 128, False), (3, 1100, 128, True), (3, 700, 200, True), (3, 2100, 40, True),
    # four CUs per sequence
    (20, 1, 132, True), (9, 7, 252, False), (8, 32, 256, True), (1000, 2, 256, True),
    # scan256.h: B = 33 is the first past the four-CU limit
    (7, 33, 256, True), (6, 40, 132, False), (5, 256, 200, True),
    # T edges: T = 1; T around the prefetch depths (units: 6 forward, 6 / 4 backward)
    (1, 3, 48, True), (1, 5, 256, True), (1, 600, 64, True), (1, 40, 200, False),
    (5, 9, 88, True), (6, 9, 88, False), (7, 9, 88, True), (13, 9, 88, False), (5, 300, 64, True), (7, 300, 64, False),
    # long
    (1000, 3, 48, True), (1000, 2, 88, False),
]


def _lstm_cases():
    cs = [_lstm_case(*r) for r in _LSTM_ROWS]
    # saturated gates (gx x 6), one per family
    cs += [_lstm_case(20, 4, 64, True, gs=6.0), _lstm_case(5, 300, 88, True, gs=6.0), _lstm_case(4, 600, 128, False, gs=6.0),
           _lstm_case(30, 3, 200, True, gs=6.0), _lstm_case(10, 40, 256, True, gs=6.0)]
    # a backward through h_all only (dc_all arrives as None) for every family, through c_all only (dh_all None) for some
    for T, B, H in [(9, 5, 48), (5, 300, 128), (4, 700, 64), (12, 6, 256), (6, 50, 200)]:
        cs.append(_lstm_case(T, B, H, True, grad="h"))
    for T, B, H in [(9, 5, 48), (4, 700, 64), (12, 6, 256), (6, 50, 200)]:
        cs.append(_lstm_case(T, B, H, True, grad="c"))
    return cs


LSTM_CASES = _lstm_cases()
CL4_CASES = [c for c in LSTM_CASES if lstm_family(c["B"], c["H"]) == "cl4"]

_MFN_ROWS = [(1, 1, 0.0), (3, 1, 0.0), (5, 17, 0.2), (300, 33, 0.0), (300, 33, 0.2), (6, 256, 0.0), (6, 257, 0.2), (5, 400, 0.0),
             (4, 513, 0.2), (3, 2100, 0.0), (1000, 2, 0.0), (1000, 2, 0.2)]
MFN_CASES = [{"id": "m_T%d_B%d_p%g" % r, "T": r[0], "B": r[1], "p": r[2]} for r in _MFN_ROWS]


def lstm_inputs(c):
    tag = "bfscan:" + c["id"]
    T, B, H = c["T"], c["B"], c["H"]
    gx = c["gs"] * R.gen_normal(tag + "gx", (T, B, 4 * H), 23)
    W = R.gen_normal(tag + "w", (4 * H, H), 23) / np.sqrt(H)
    h0 = 0.5 * R.gen_normal(tag + "h0", (B, H), 23) if c["init"] else None
    c0 = 0.5 * R.gen_normal(tag + "c0", (B, H), 23) if c["init"] else None
    gh = R.gen_normal(tag + "gh", (T, B, H), 23) if "h" in c["grad"] else None
    gc = R.gen_normal(tag + "gc", (T, B, H), 23) if "c" in c["grad"] else None
    return gx, W, h0, c0, gh, gc


def mfn_inputs(c):
    tag = "bfscan:" + c["id"]
    T, B = c["T"], c["B"]
    apre = R.gen_normal(tag + "a", (T, B, 128), 23)
    chat = torch.tanh(R.gen_normal(tag + "c", (T, B, 128), 23))
    Wm = R.gen_normal(tag + "wm", (128, 128), 23) / np.sqrt(128)
    W2 = R.gen_normal(tag + "w2", (2, 128, 64), 23) / 8
    b2 = 0.1 * R.gen_normal(tag + "b2", (2, 128), 23)
    g = R.gen_normal(tag + "g", (T, B, 128), 23)
    return apre, chat, Wm, W2, b2, g


def mfn_seed(c):
    return 4242 + c["T"] + c["B"]


def lstm_loss(h, c, gh, gc):
    return (0 if gh is None else (h * gh).sum()) + (0 if gc is None else (c * gc).sum())


# ------------------------------------------------------------------------------------------------ child process
def child_main(kind, out_path, payload_json):
    """The GPU runs of the cases whose ids the payload lists, in a process of their own: kind "lstm" or "mfn"."""
    from multimodal_transformer_amd import functional as F
    ids = set(json.loads(payload_json))
    dev = torch.device("cuda:0")
    out = {}

    def run(fn):
        res, names = device_kernel_names(fn)
        F.check_device_errors()                 # the four-CU scans' exchange time-out word must be zero
        return res, names
    for c in (LSTM_CASES if kind == "lstm" else MFN_CASES):
        cid = c["id"]
        if cid not in ids:
            continue
        if kind == "lstm":
            gx, W, h0, c0, gh, gc = (None if t is None else t.to(dev) for t in lstm_inputs(c))
            leaves = [None if t is None else t.requires_grad_() for t in (gx, W, h0, c0)]

            def step():
                h, cc = F.lstm_scan(*leaves)
                lstm_loss(h, cc, gh, gc).backward()
                return h.detach(), cc.detach()
            (h, cc), names = run(step)
            res = {"h": h, "c": cc, "dgx": leaves[0].grad, "dW": leaves[1].grad}
            if c["init"]:
                res["dh0"], res["dc0"] = leaves[2].grad, leaves[3].grad
        else:
            apre, chat, Wm, W2, b2, g = (t.to(dev) for t in mfn_inputs(c))
            leaves = [t.requires_grad_() for t in (apre, chat, Wm, W2, b2)]
            T, B, p, seed = c["T"], c["B"], c["p"], mfn_seed(c)

            def step():
                mem = F.mfn_mem_scan(*leaves, dropout_p=p, seed=seed)
                (mem * g).sum().backward()
                return mem.detach()
            mem, names = run(step)
            res = dict(zip(("mem", "dapre", "dchat", "dWm", "dW2", "db2"), [mem] + [t.grad for t in leaves]))
            if p > 0:
                keep, sc = F.dropout_mask(p, seed, 1000, T * B * 128, dev)
                res["keep"] = keep.reshape(T, B, 128)
                out[cid + ":scale"] = np.array(sc)
        for k, v in res.items():
            out[cid + ":" + k] = v.cpu().numpy()
        out[cid + ":names"] = np.array(json.dumps(names))
    torch.cuda.synchronize()
    F.check_device_errors()
    np.savez(out_path, **out)


_SWITCHES = {"default": {}, "no_cluster": {"MMT_NO_CLUSTER_SCAN": "1"}}


def _child(kind, switch, cases, tmp_dir):
    return run_child(__name__, kind, switch, [c["id"] for c in cases], tmp_dir, _SWITCHES, timeout=600)


def _names(run, cid):
    return json.loads(str(run[cid + ":names"]))


# ------------------------------------------------------------------------------------------------ LSTM
_LSTM_REFS = {}


def lstm_ref(c):
    """the reference's h, c and gradients for case c (cached: the T = 1000 cases are the slow part of this file)"""
    if c["id"] not in _LSTM_REFS:
        gx, W, h0, c0, gh, gc = lstm_inputs(c)
        leaves = [None if t is None else t.double().requires_grad_() for t in (gx, W, h0, c0)]
        h, cc = E.lstm_scan(*leaves)
        lstm_loss(h, cc, None if gh is None else gh.double(), None if gc is None else gc.double()).backward()
        ref = {"h": h.detach().numpy(), "c": cc.detach().numpy(), "dgx": leaves[0].grad.numpy(), "dW": leaves[1].grad.numpy()}
        if c["init"]:
            ref["dh0"], ref["dc0"] = leaves[2].grad.numpy(), leaves[3].grad.numpy()
        _LSTM_REFS[c["id"]] = ref
    return _LSTM_REFS[c["id"]]


def lstm_compare(tag, run, cid, ref, failures):
    got = lambda n: run[cid + ":" + n]  # noqa: E731
    for n in ("h", "c"):
        check_scan("%s %s" % (tag, n), got(n), ref[n], LSTM_OUT, failures, seq=True)
    check_scan(tag + " dgx", got("dgx"), ref["dgx"], LSTM_DGX, failures, seq=True)
    check_scan(tag + " dW", got("dW"), ref["dW"], LSTM_DW, failures, scale=LSTM_W_SCALE)
    for n in ("dh0", "dc0"):
        if n in ref:
            check_scan("%s %s" % (tag, n), got(n), ref[n], LSTM_D0, failures)


@pytest.mark.parametrize("c", LSTM_CASES, ids=[c["id"] for c in LSTM_CASES])
def test_lstm_scan(tmp_dir, c):
    run = _child("lstm", "default", LSTM_CASES, tmp_dir)
    fam = lstm_family(c["B"], c["H"])
    tag = "bf lstm %s %s" % (fam, c["id"])
    check_ran(tag, _names(run, c["id"]), fam)
    failures = []
    lstm_compare(tag, run, c["id"], lstm_ref(c), failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", CL4_CASES, ids=[c["id"] for c in CL4_CASES])
def test_lstm_scan_without_the_four_cu_path(tmp_dir, c):
    """MMT_NO_CLUSTER_SCAN=1 sends the four-CU shapes (B <= 32, H > 128) to scan256.h: against the reference and the four-CU result"""
    run = _child("lstm", "no_cluster", CL4_CASES, tmp_dir)
    cl4 = _child("lstm", "default", LSTM_CASES, tmp_dir)
    tag = "bf lstm s256 (no cluster) %s" % c["id"]
    check_ran(tag, _names(run, c["id"]), lstm_family(c["B"], c["H"], no_cluster=True))
    failures = []
    lstm_compare(tag, run, c["id"], lstm_ref(c), failures)
    four = {k.split(":", 1)[1]: v for k, v in cl4.items() if k.startswith(c["id"] + ":") and not k.endswith(":names")}
    lstm_compare(tag + " vs cl4", run, c["id"], four, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ MFN memory scan
_MFN_REFS = {}


def mfn_ref(c, run):
    """the reference's mem and gradients for case c; in train mode with the mask the forward kernel drew (stream 1000)"""
    if c["id"] not in _MFN_REFS:
        apre, chat, Wm, W2, b2, g = mfn_inputs(c)
        drop = None
        if c["p"] > 0:
            drop = torch.from_numpy(run[c["id"] + ":keep"]).double() * float(run[c["id"] + ":scale"])
        leaves = [t.double().requires_grad_() for t in (apre, chat, Wm, W2, b2)]
        mem = E.mfn_mem_scan(*leaves, drop=drop)
        (mem * g.double()).sum().backward()
        _MFN_REFS[c["id"]] = dict(zip(("mem", "dapre", "dchat", "dWm", "dW2", "db2"),
                                      [mem.detach().numpy()] + [t.grad.numpy() for t in leaves]))
    return _MFN_REFS[c["id"]]


@pytest.mark.parametrize("c", MFN_CASES, ids=[c["id"] for c in MFN_CASES])
def test_mfn_mem_scan(tmp_dir, c):
    run = _child("mfn", "default", MFN_CASES, tmp_dir)
    fam = mfn_family(c["B"])
    tag = "bf mfn %s %s" % (fam, c["id"])
    check_ran(tag, _names(run, c["id"]), fam)
    ref = mfn_ref(c, run)
    got = lambda n: run[c["id"] + ":" + n]  # noqa: E731
    failures, bd = [], mfn_bounds(c)
    for n in ("mem", "dapre", "dchat"):
        check_scan("%s %s" % (tag, n), got(n), ref[n], bd[n], failures, seq=True)
    for n in ("dWm", "dW2"):
        check_scan("%s %s" % (tag, n), got(n), ref[n], bd[n], failures, scale=MFN_W_SCALE)
    check_scan(tag + " db2", got("db2").ravel(), ref["db2"].ravel(), bd["db2"], failures)
    assert not failures, "\n".join(failures)
