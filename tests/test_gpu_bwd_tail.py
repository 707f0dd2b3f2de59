"""The d_model = 128 fixed shape's final-norm backward as the head of the last layer's backward chain, and its fixed-shape weight
preparation, against the separate launches MMT_NO_TAIL_FOLD=1 restores, each form in a process of its own (the switch is read once per
process; gpu_harness.run_child, which calls child_main below).

With the switch unset the final LayerNorm's backward runs inside `encoder_pre_attn_bwd_head_kernel` (one body shared with
`layernorm_bwd_kernel`: rowgemm.h layernorm_bwd_rows) and the weights are prepared by `encoder_prep_shape_kernel<128>`.  Same arithmetic
in the same order, so the output, the input gradient and every parameter gradient are BIT-identical between the two forms; the separate
launches are the reference here, and the other suites keep checking the default against the oracle.

Shapes (B, T, d, h, d_ff, N): (3, 37, 128, 8, 128, 2) — 111 windows, four tiles of the head, the last of 15 rows — in eval and in
train mode (host seed: the head then drops dx on its way into the A tile), and (8, 300, 128, 8, 128, 2): 75 tiles, train mode."""
import json

import numpy as np
import pytest
import torch

import bf16_ref as E
import recipe as R
from gpu_harness import device_kernel_names, run_child, tmp_dir  # noqa: F401 (tmp_dir: a fixture)

pytestmark = pytest.mark.gpu

_SWITCHES = {"new": {}, "old": {"MMT_NO_TAIL_FOLD": "1"}}

# id: (B, T, d, h, d_ff, N, dropout p)
_FORMS = {
    "ragged_eval": (3, 37, 128, 8, 128, 2, 0.0),
    "ragged_train": (3, 37, 128, 8, 128, 2, 0.1),
    "tiles75_train": (8, 300, 128, 8, 128, 2, 0.1),
}
_NAMES = (2, 64, 128, 8, 128, 2)


def _inputs(tag, B, T, d, f, N, dev):
    p32 = R.gen_params(E.encoder_param_shapes(d, f, N), 23)
    flat = torch.cat([t.reshape(-1) for t in p32.values()]).to(dev).requires_grad_()
    x = R.gen_normal(tag + ":x", (B, T, d), 23).to(dev).requires_grad_()
    g = R.gen_normal(tag + ":g", (B, T, d), 23).to(dev)
    lengths = ([T, max(1, T // 2), max(1, T - 7)] + [T] * B)[:B]
    return flat, x, g, R.prefix_mask(lengths, T).to(dev)


# ------------------------------------------------------------------------------------------------ child process
def child_main(kind, out_path, payload_json):
    from multimodal_transformer_amd import functional as F
    payload = json.loads(payload_json)
    dev = torch.device("cuda:0")
    out = {}
    if kind == "forms":
        for cid in payload:
            B, T, d, h, f, N, p = _FORMS[cid]
            flat, x, g, mask = _inputs(cid, B, T, d, f, N, dev)
            y = F.encoder_stack(x, mask, flat, h, f, N, dropout_p=p, seed=977 + T)
            y.backward(g)
            out[cid + ":y"], out[cid + ":dx"], out[cid + ":dp"] = y.detach().cpu().numpy(), x.grad.cpu().numpy(), flat.grad.cpu().numpy()
    else:
        B, T, d, h, f, N = _NAMES
        flat, x, g, mask = _inputs(kind, B, T, d, f, N, dev)

        def step():
            x.grad, flat.grad = None, None
            y = F.encoder_stack(x, mask, flat, h, f, N, dropout_p=0.1, seed=31)
            y.backward(g)
            return y.detach()

        _, names = device_kernel_names(step, warm=True)
        out["have_names"] = np.array(names is not None)
        out["names"] = np.array(names or [""], dtype=str)
    torch.cuda.synchronize()
    F.check_device_errors()
    np.savez(out_path, **out)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("cid", sorted(_FORMS))
def test_head_and_fixed_preparation_equal_the_separate_launches(tmp_dir, cid):
    new = run_child(__name__, "forms", "new", sorted(_FORMS), tmp_dir, _SWITCHES, timeout=300)
    old = run_child(__name__, "forms", "old", sorted(_FORMS), tmp_dir, _SWITCHES, timeout=300)
    for k in ("y", "dx", "dp"):
        a, b = new["%s:%s" % (cid, k)], old["%s:%s" % (cid, k)]
        assert np.isfinite(b).all() and np.abs(b).max() > 0, "%s %s: the separate launches give nothing to compare with" % (cid, k)
        assert np.array_equal(a, b), "%s %s: %d of %d values differ between the two forms" % (cid, k, int((a != b).sum()), a.size)


def test_launch_list(tmp_dir):
    new = run_child(__name__, "names", "new", None, tmp_dir, _SWITCHES, timeout=300)
    old = run_child(__name__, "names", "old", None, tmp_dir, _SWITCHES, timeout=300)
    if not (bool(new["have_names"]) and bool(old["have_names"])):
        return                                      # the profiler reported no device activity: nothing to assert on (gpu_harness)
    count = lambda r, what: sum(what in n for n in r["names"].tolist())     # noqa: E731
    assert count(new, "layernorm_bwd_kernel") == 0 and count(new, "encoder_pre_attn_bwd_head_kernel") == 1, sorted(set(new["names"].tolist()))
    assert count(new, "encoder_prep_shape_kernel") == 1 and count(new, "encoder_prep_kernel") == 0
    assert count(old, "layernorm_bwd_kernel") == 1 and count(old, "encoder_pre_attn_bwd_head_kernel") == 0, sorted(set(old["names"].tolist()))
    assert count(old, "encoder_prep_shape_kernel") == 0 and count(old, "encoder_prep_kernel") == 1
    assert len(new["names"]) == len(old["names"]) - 1          # one launch less
