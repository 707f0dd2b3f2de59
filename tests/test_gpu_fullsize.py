"""GPU tests at BASELINE.json's full sizes (configs[3]: T=500 d=128 h=8 N=6, 32 sequences per GPU; configs[4]:
T=1000 d=256 h=8, per-modality encoder of the MFT).  The oracle cannot run a whole batch of that size in seconds,
so the checks are the size-independent properties of the path plus oracle parity on individual sequences:

  * sequences are independent: the rows of sequence b in the full-batch result equal (bit-exactly, eval mode) the
    result of a batch that holds the same sequence at another position — a row's arithmetic must not depend on which
    32-window tile or which workgroup it landed in;
  * the oracle, run on a few single sequences of the batch (fp32, seconds), matches the full-batch rows of those
    sequences to the stated bf16 tolerances, and so do the input gradients (the loss is a sum over sequences);
  * weight gradients are additive over a partition of the batch (linearity of the backward pass in the batch), and on a sub-batch
    of four sequences every weight / bias / LayerNorm gradient of all N layers matches the oracle's;
  * blanked (mask == 0) query rows: exact uniform attention, checked through the oracle rows above on ragged lengths;
  * eval mode is deterministic: two runs are bit-identical.
"""
import numpy as np
import pytest
import torch

import oracle
import recipe as R
from conftest import rel_l2
from gpu_harness import OUT_RTOL, RELU_GRAD_RTOL, CCC_MIN, dev, load_named, seeded_encoder  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

FULL = {
    "C2": dict(B=32, T=300, d=40, h=4, N=6),          # configs[1]: d_k = 10 (a padded head), T in the one-kernel-backward range
    "C4": dict(B=32, T=500, d=128, h=8, N=6),
    "C4x8": dict(B=256, T=500, d=128, h=8, N=6),      # configs[3] WHOLE batch on one GPU (bench.py's config_full_batch line)
    "C5e": dict(B=16, T=1000, d=256, h=8, N=6),       # 16 of the 64 sequences/GPU of configs[4]: same T, d, h, N
}


def _lengths(B, T):
    ls = [T] * B
    for i, frac in ((1, 0.61), (2, 0.07), (B - 1, 0.33)):
        ls[i] = max(1, int(T * frac))
    ls[3 % B] = 1                                          # a sequence with a single valid window
    return ls


def _run(enc, x, mask, g):
    for p in enc.parameters():
        p.grad = None
    xg = x.clone().requires_grad_()
    y = enc(xg, mask)
    (y * g).sum().backward()
    return y.detach(), xg.grad.detach(), torch.cat([p.grad.reshape(-1) for p in enc.parameters()]).clone()


@pytest.mark.parametrize("name", list(FULL))
def test_full_size_properties_and_oracle_rows(dev, name):
    cfg = FULL[name]
    B, T, d, h = cfg["B"], cfg["T"], cfg["d"], cfg["h"]
    enc, p32 = seeded_encoder(d, h, cfg["N"], dev, 5)
    lengths = _lengths(B, T)
    mask_c = R.prefix_mask(lengths, T)
    x_c = R.gen_normal(name + ":full:x", (B, T, d), 5)
    g_c = R.gen_normal(name + ":full:g", (B, T, d), 5) * mask_c
    x, g, mask = x_c.to(dev), g_c.to(dev), mask_c.to(dev)

    y, dx, gw = _run(enc, x, mask, g)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and torch.isfinite(gw).all()

    # determinism: two identical runs agree bit for bit (one run, one comparison: a mismatch is a failure and says what differed)
    def _describe(a_, b_):
        diff = (a_ != b_)
        rows = diff.reshape(B, T, -1).any(dim=2)
        sel = rows.reshape(-1)
        rel = float((a_.reshape(B * T, -1)[sel] - b_.reshape(B * T, -1)[sel]).norm() / a_.reshape(B * T, -1)[sel].norm())
        return "%d elements in %d rows of sequences %s, relative L2 on those rows %.2e" % (
            int(diff.sum()), int(rows.sum()), sorted(set(int(r[0]) for r in rows.nonzero()))[:8], rel)

    y2, dx2, gw2 = _run(enc, x, mask, g)
    assert torch.equal(y, y2), "forward not reproducible: " + _describe(y, y2)
    assert torch.equal(dx, dx2), "input gradient not reproducible: " + _describe(dx, dx2)
    assert torch.equal(gw, gw2), "weight gradients not reproducible: %d elements differ" % int((gw != gw2).sum())

    # independence of sequences / position in the batch: reverse the batch order
    perm = torch.arange(B - 1, -1, -1, device=dev)
    yp, dxp, gwp = _run(enc, x[perm].contiguous(), mask[perm].contiguous(), g[perm].contiguous())
    assert torch.equal(yp[perm], y), "a sequence's output depends on its position in the batch"
    assert torch.equal(dxp[perm], dx), "a sequence's input gradient depends on its position in the batch: " + _describe(dxp[perm], dx)
    assert rel_l2(gwp.cpu().numpy(), gw.cpu().numpy()) < 1e-4          # same terms, different summation order

    # additivity of the weight gradients over a partition of the batch
    half = B // 2
    _, _, g0 = _run(enc, x[:half].contiguous(), mask[:half].contiguous(), g[:half].contiguous())
    _, _, g1 = _run(enc, x[half:].contiguous(), mask[half:].contiguous(), g[half:].contiguous())
    assert rel_l2((g0 + g1).cpu().numpy(), gw.cpu().numpy()) < 1e-4

    # oracle on single sequences of the batch: full length, ragged, and a single valid window
    torch.set_num_threads(8)
    for b in (0, 1, 3 % B):
        p = {k: v.clone() for k, v in p32.items()}
        xo = x_c[b:b + 1].clone().requires_grad_()
        yo = oracle.encoder_stack(p, "", xo, mask_c[b:b + 1], h)
        (yo * g_c[b:b + 1]).sum().backward()
        L = lengths[b]
        got, ref = y[b].cpu().numpy(), yo[0].detach().numpy()
        r_valid = rel_l2(got[:L], ref[:L])
        r_all = rel_l2(got, ref)
        r_dx = rel_l2(dx[b].cpu().numpy(), xo.grad[0].numpy())
        from multimodal_transformer_amd import eval_ccc
        ccc = eval_ccc(ref.reshape(-1), got.reshape(-1))
        print("%s seq %d (len %d): out rel_l2 valid %.3e all %.3e  dx %.3e  CCC %.6f" % (name, b, L, r_valid, r_all, r_dx, ccc))
        assert r_valid < OUT_RTOL and r_all < OUT_RTOL
        assert ccc >= CCC_MIN
        assert r_dx < RELU_GRAD_RTOL

    # WEIGHT gradients against the oracle (the additivity check above compares the kernels with themselves): the full-length, the
    # ragged, the 7 %-length and the one-window sequence as one sub-batch through both — all N layers' weight, bias and LayerNorm
    # gradients, tensor by tensor (wgrad_kernel's window splits + encoder_finalize_kernel's fixed-order sums at T = 300 / 500 / 1000)
    from conftest import grad_close
    sub = sorted({0, 1, 2, 3 % B})
    names = [k for k, _ in enc.named_parameters()]
    po = {k: v.clone().requires_grad_() for k, v in p32.items()}
    yo = oracle.encoder_stack(po, "", x_c[sub], mask_c[sub], h)
    (yo * g_c[sub]).sum().backward()
    _, _, gsub = _run(enc, x[sub].contiguous(), mask[sub].contiguous(), g[sub].contiguous())
    gsub = gsub.cpu()
    off, worst = 0, (0.0, "")
    for k in names:
        ref = po[k].grad.reshape(-1)
        got = gsub[off:off + ref.numel()]
        off += ref.numel()
        rel = rel_l2(got.numpy(), ref.numpy())
        if float(ref.norm()) > 1e-3 * ref.numel() ** 0.5 and rel > worst[0]:
            worst = (rel, k)
        if k.endswith("self_attn.linears.1.bias"):
            # the key-projection bias has NO gradient analytically (a constant added to every key shifts a query's scores alike and
            # softmax ignores it): the oracle returns fp32 round-off, the kernels the column sum of bf16-rounded dK rows.  Bound it by
            # the scale of its sibling, the query-projection bias gradient of the same layer
            sib = po[k.replace("linears.1.bias", "linears.0.bias")].grad
            assert float(got.norm()) <= 3e-2 * float(sib.norm()) + 1e-5, "%s: %s should vanish, has norm %.3e (query bias %.3e)" % (
                name, k, float(got.norm()), float(sib.norm()))
            continue
        assert grad_close(got.numpy(), ref.numpy(), RELU_GRAD_RTOL, atol=2e-4), "%s: weight gradient of %s off by rel_l2 %.3e" % (name, k, rel)
    assert off == gsub.numel()
    allref = torch.cat([po[k].grad.reshape(-1) for k in names])
    r_w = rel_l2(gsub.numpy(), allref.numpy())
    print("%s weight gradients of sequences %s vs oracle: rel_l2 %.3e over all %d values; worst tensor %s %.3e" % (name, sub, r_w, off, worst[1], worst[0]))
    assert r_w < RELU_GRAD_RTOL


def test_full_size_blank_rows_are_uniform_attention(dev):
    """mask == 0 query rows at T=500: the attention output of such a row is exactly the mean of V over ALL keys
    (keys are never masked — transformer/MFT/multiTransformer.py:28-31), whatever the row's own query."""
    import multimodal_transformer_amd.functional as F
    B, T, d, h = 4, 500, 128, 8
    q = R.gen_normal("blank:q", (B, T, d), 3).to(dev)
    k = R.gen_normal("blank:k", (B, T, d), 3).to(dev)
    v = R.gen_normal("blank:v", (B, T, d), 3).to(dev)
    lengths = [500, 333, 1, 47]
    mask = R.prefix_mask(lengths, T).to(dev)
    out = F.sdpa(q, k, v, mask, h)
    vb = v.to(torch.bfloat16).float()                       # the kernel's operands are the bf16 roundings
    for b, L in enumerate(lengths):
        if L < T:
            blank = out[b, L:, :]
            mean_v = vb[b].mean(dim=0, keepdim=True)
            assert torch.equal(blank, blank[:1].expand_as(blank)), "blank rows of one sequence must be identical"
            assert (blank - mean_v).abs().max().item() < 2e-3
    # and the result does not depend on what the blanked queries contain
    q2 = q.clone()
    for b, L in enumerate(lengths):
        q2[b, L:, :] = 1e3
    assert torch.equal(F.sdpa(q2, k, v, mask, h), out)


def _check_sequences(name, model_out, oracle_fn, lengths, picks):
    """model_out: (B,T,1) valence of the full batch on the GPU; oracle_fn(b) -> (1,T,1) CPU reference of sequence b."""
    from multimodal_transformer_amd import eval_ccc
    out = model_out.detach().cpu().numpy()
    cccs = []
    for b in picks:
        with torch.no_grad():
            ref = oracle_fn(b).numpy()[0]
        got = out[b]
        L = lengths[b]
        assert (got[L:] == 0).all() and (ref[L:] == 0).all()           # exact zeros where mask == 0
        r = rel_l2(got[:L], ref[:L])
        ccc = eval_ccc(ref[:L].reshape(-1), got[:L].reshape(-1)) if L > 2 else 1.0
        print("%s seq %d (len %d): valence rel_l2 %.3e  CCC %.6f" % (name, b, L, r, ccc))
        cccs.append(ccc)
        assert r < OUT_RTOL and ccc >= CCC_MIN         # north_star: valence CCC within 1e-3 of the CPU reference, per sequence
    # the reference's metric is the MEAN of per-sequence CCCs (transformer/SFT/train.py evaluate()); a random-init model
    # has a nearly flat valence track (std ~1e-2), the least favourable case for a correlation measure
    assert float(np.mean(cccs)) >= CCC_MIN


def test_full_size_sft_model_configs3(dev):
    """configs[3] per-GPU shape through the whole SFT sequence model (transformer/SFT/multiTransformer.py:422-480):
    32 sequences, T=500, d_model=128, 8 heads — valence of single sequences vs the CPU oracle."""
    from multimodal_transformer_amd import multiTransformer as MT
    B, T = 32, 500
    model = MT.NLPTransformer(512, embed_dim=128, h=8, device=dev)
    p32 = load_named(model, 9)
    model = model.to(dev).eval()
    lengths = _lengths(B, T)
    mask_c = R.prefix_mask(lengths, T)
    x_c = torch.tanh(R.gen_normal("full:sft:x", (B, T, 512), 9))
    with torch.no_grad():
        y = model(x_c.to(dev), mask_c.to(dev), lengths)
    assert y.shape == (B, T, 1) and torch.isfinite(y).all()
    torch.set_num_threads(8)
    _check_sequences("SFT C4", y, lambda b: oracle.nlp_transformer(p32, x_c[b:b + 1], mask_c[b:b + 1], 8), lengths, (0, 1, 2))


def test_full_size_mft_model_configs2(dev):
    """configs[2]: MFT (per-modality encoders + MFN delta-memory gate), T=300, 32 sequences, three modalities
    (transformer/MFT/multiTransformer.py:250-310) — valence of single sequences vs the CPU oracle, and one
    full fwd+bwd in train mode at that size (finite gradients for every live parameter)."""
    from multimodal_transformer_amd import multiTransformer as MT
    B, T = 32, 300
    mods = R.MODS_AVL
    model = MT.MultiTransformer(mods, R.EMBED_AVL, device=dev)
    p32 = load_named(model, 13)
    model = model.to(dev).eval()
    lengths = _lengths(B, T)
    mask_c = R.prefix_mask(lengths, T)
    ins_c = {m: R.gen_normal("full:mft:" + m, (B, T, R.EMBED_AVL[m]), 13) for m in mods}
    ins = {m: v.to(dev) for m, v in ins_c.items()}
    with torch.no_grad():
        y = model(ins, mask_c.to(dev), lengths)
    assert y.shape == (B, T, 1) and torch.isfinite(y).all()
    torch.set_num_threads(8)
    _check_sequences("MFT C3", y,
                     lambda b: oracle.multi_transformer(p32, {m: v[b:b + 1] for m, v in ins_c.items()}, mask_c[b:b + 1], mods),
                     lengths, (0, 1))
    model.train()
    tgt = R.gen_uniform("full:mft:t", (B, T, 1), 13).to(dev) * mask_c.to(dev)
    loss = ((model(ins, mask_c.to(dev), lengths) - tgt) ** 2).sum() / float(sum(lengths))
    loss.backward()
    assert torch.isfinite(loss)
    live = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    assert len(live) > 100
    for n, p in live:
        assert torch.isfinite(p.grad).all(), n


def test_full_size_mft_model_configs4(dev):
    """configs[4] per-GPU slice through the WHOLE MFT model: 64 sequences, T=1000, three modalities, d_model=256, 8 heads
    (three N=6 encoder stacks, three LSTM scans and the MFN memory scan at T=1000: transformer/MFT/multiTransformer.py:181-248,
    288-313) — valence of single sequences (full length and ragged) vs the CPU oracle, exact zeros behind the mask, and one
    train-mode forward+backward at that size with finite gradients for every live parameter."""
    from multimodal_transformer_amd import multiTransformer as MT, functional as F
    B, T = 64, 1000
    mods = R.MODS_AVL
    model = MT.MultiTransformer(mods, R.EMBED_AVL, device=dev)
    p32 = load_named(model, 29)
    model = model.to(dev).eval()
    lengths = _lengths(B, T)
    mask_c = R.prefix_mask(lengths, T)
    ins_c = {m: R.gen_normal("full:mft4:" + m, (B, T, R.EMBED_AVL[m]), 29) for m in mods}
    ins = {m: v.to(dev) for m, v in ins_c.items()}
    with torch.no_grad():
        y = model(ins, mask_c.to(dev), lengths)
    assert y.shape == (B, T, 1) and torch.isfinite(y).all()
    torch.set_num_threads(8)
    _check_sequences("MFT C5", y,
                     lambda b: oracle.multi_transformer(p32, {m: v[b:b + 1] for m, v in ins_c.items()}, mask_c[b:b + 1], mods),
                     lengths, (0, 1))
    model.train()
    tgt = R.gen_uniform("full:mft4:t", (B, T, 1), 29).to(dev) * mask_c.to(dev)
    loss = ((model(ins, mask_c.to(dev), lengths) - tgt) ** 2).sum() / float(sum(lengths))
    loss.backward()
    assert torch.isfinite(loss)
    live = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    assert len(live) > 100
    for n, p in live:
        assert torch.isfinite(p.grad).all(), n
    F.check_device_errors()


def test_sub_batch_streams_match_single_stream(dev):
    """Encoder.sub_batch_streams = 2 (the batch as two halves on two HIP streams, parameter gradients of the halves summed): in eval
    mode outputs and input gradients equal the single-stream run bit for bit (a sequence's result does not depend on its batch) and the
    parameter gradients to summation order; in train mode the step runs and every gradient is finite."""
    cfg = FULL["C4"]
    B, T, d = cfg["B"], cfg["T"], cfg["d"]
    enc, _ = seeded_encoder(d, cfg["h"], cfg["N"], dev, 5)
    lengths = _lengths(B, T)
    mask = R.prefix_mask(lengths, T).to(dev)
    x = R.gen_normal("split:x", (B, T, d), 5).to(dev)
    g = (R.gen_normal("split:g", (B, T, d), 5) * R.prefix_mask(lengths, T)).to(dev)
    y1, dx1, gw1 = _run(enc, x, mask, g)
    enc.sub_batch_streams = 2
    try:
        assert enc._sub_batch_streams(x) == 2
        y2, dx2, gw2 = _run(enc, x, mask, g)
        assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
        assert rel_l2(gw2.cpu().numpy(), gw1.cpu().numpy()) < 1e-4
        assert all(p.grad.untyped_storage().data_ptr() == enc.layers[0].self_attn.linears[0].weight.grad.untyped_storage().data_ptr()
                   for p in enc.flat_parameters())                       # still views of ONE flat gradient buffer
        enc.train()
        y3, dx3, gw3 = _run(enc, x, mask, g)
        assert torch.isfinite(y3).all() and torch.isfinite(dx3).all() and torch.isfinite(gw3).all()
        assert float((y3 - y2).abs().max()) > 1e-2                        # dropout happened
    finally:
        enc.sub_batch_streams = 1
        enc.eval()
