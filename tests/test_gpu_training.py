"""Training-step semantics on the GPU (transformer/SFT/train.py:108-153, :538, :621): MSE-sum loss divided by
sum(lengths), Adam(lr=1e-4, weight_decay=1e-4), several consecutive steps.  The HIP model and the CPU oracle start from the
same weights and see the same batches; their loss trajectories and final parameters must agree (dropout off: the reference's
train-mode dropout stream is not reproducible, its masks are checked separately in test_gpu_dropout.py)."""
import numpy as np
import pytest
import torch

import oracle
import recipe as R
from conftest import rel_l2
from gpu_harness import dev  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


def _batches(n, B, T, lengths):
    for i in range(n):
        x = torch.tanh(R.gen_normal("train:x%d" % i, (B, T, 512), 31))
        tgt = R.gen_uniform("train:t%d" % i, (B, T, 1), 31) * R.prefix_mask(lengths, T)
        yield x, tgt


def test_adam_steps_follow_the_oracle(dev):
    from multimodal_transformer_amd import multiTransformer as MT
    B, T, lengths, steps, lr = 4, 24, [24, 17, 9, 3], 6, 1e-3           # a larger lr than the reference's 1e-4 so that 6 steps move
    model = MT.NLPTransformer(512, embed_dim=40, h=4, N=2, device=dev)
    p32 = R.gen_params(R.shapes_of(model.state_dict()), 31)
    model.load_state_dict(p32)
    model = model.to(dev).eval()                                         # eval(): dropout off, gradients still flow
    mask = R.prefix_mask(lengths, T)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4)
    po = {k: v.clone().requires_grad_() for k, v in p32.items()}
    opt_o = torch.optim.Adam(list(po.values()), lr=lr, weight_decay=1e-4)
    torch.set_num_threads(4)
    losses, losses_o = [], []
    for x, tgt in _batches(steps, B, T, lengths):
        opt.zero_grad(set_to_none=True)
        out = model(x.to(dev), mask.to(dev), lengths)
        loss = ((out - tgt.to(dev)) ** 2).sum() / float(sum(lengths))    # MSELoss(reduction='sum') / sum(lengths)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        opt_o.zero_grad(set_to_none=True)
        out_o = oracle.nlp_transformer(po, x, mask, 4)
        loss_o = oracle.masked_mse_sum_loss(out_o, tgt, lengths)
        loss_o.backward()
        opt_o.step()
        losses_o.append(loss_o.item())
    print("loss HIP   ", " ".join("%.5f" % v for v in losses))
    print("loss oracle", " ".join("%.5f" % v for v in losses_o))
    for a, b in zip(losses, losses_o):
        assert abs(a - b) <= 2e-2 * abs(b) + 1e-4
    # Parameters after the steps.  Adam normalises every gradient entry by its own magnitude, so entries whose gradient is
    # analytically zero (the key-projection biases: softmax is shift invariant) take sign-of-noise steps of full size in BOTH
    # runs; they are left out, and the accumulated update is compared as one vector.
    ups, ups_o = [], []
    for (n, p), (no, q) in zip(model.named_parameters(), po.items()):
        assert n == no
        if n.endswith("self_attn.linears.1.bias"):
            continue
        ups.append((p.detach().cpu() - p32[n]).reshape(-1))
        ups_o.append((q.detach() - p32[n]).reshape(-1))
    dist = rel_l2(torch.cat(ups).numpy(), torch.cat(ups_o).numpy())
    print("relative distance between the two accumulated updates: %.3e" % dist)
    assert dist < 0.18        # measured 0.138 (x1.3): Adam turns small gradient differences of small gradients into full-size steps


@pytest.mark.parametrize("lr,steps,ccc_min", [(1e-4, 10, 1 - 1e-3), (1e-3, 6, 1 - 5e-3)], ids=["reference-lr", "ten-times-lr"])
def test_trained_models_give_the_same_valence(dev, lr, steps, ccc_min):
    """What north_star cares about after training, not only before it: N Adam steps on the HIP path and N on the oracle (same batches,
    dropout off), then a FRESH batch through both models — per sequence the valence tracks must agree, although Adam turns the small
    gradient differences of small gradients into full-size steps (the accumulated updates of the six-step run at ten times the
    reference's step size differ by 14 %, test above).  With the reference's optimiser settings (Adam lr 1e-4, weight decay 1e-4:
    transformer/SFT/train.py:621) the bound is north_star's 1 - 1e-3; at ten times the step size — 10x the divergence per step — it
    is held to 1 - 5e-3 (measured 0.99895 on the least favourable sequence: a nearly flat track of a barely trained model)."""
    from multimodal_transformer_amd import multiTransformer as MT, eval_ccc
    B, T, lengths = 4, 24, [24, 17, 9, 3]
    model = MT.NLPTransformer(512, embed_dim=40, h=4, N=2, device=dev)
    p32 = R.gen_params(R.shapes_of(model.state_dict()), 31)
    model.load_state_dict(p32)
    model = model.to(dev).eval()
    mask = R.prefix_mask(lengths, T)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4)
    po = {k: v.clone().requires_grad_() for k, v in p32.items()}
    opt_o = torch.optim.Adam(list(po.values()), lr=lr, weight_decay=1e-4)
    torch.set_num_threads(4)
    for x, tgt in _batches(steps, B, T, lengths):
        opt.zero_grad(set_to_none=True)
        out = model(x.to(dev), mask.to(dev), lengths)
        (((out - tgt.to(dev)) ** 2).sum() / float(sum(lengths))).backward()
        opt.step()
        opt_o.zero_grad(set_to_none=True)
        oracle.masked_mse_sum_loss(oracle.nlp_transformer(po, x, mask, 4), tgt, lengths).backward()
        opt_o.step()
    xe = torch.tanh(R.gen_normal("adam:eval:x", (B, T, 512), 31))
    with torch.no_grad():
        ye = model(xe.to(dev), mask.to(dev), lengths).cpu().numpy()
        yo = oracle.nlp_transformer({k: v.detach() for k, v in po.items()}, xe, mask, 4).numpy()
    for b, L in enumerate(lengths):
        r = rel_l2(ye[b, :L], yo[b, :L])
        ccc = eval_ccc(yo[b, :L].reshape(-1), ye[b, :L].reshape(-1)) if L > 2 else 1.0
        print("lr %.0e, after %d Adam steps, sequence %d (len %d): valence rel_l2 %.3e  CCC %.6f" % (lr, steps, b, L, r, ccc))
        assert r < 2e-2 and ccc >= ccc_min


def test_loss_decreases_in_train_mode(dev):
    """train mode (in-kernel dropout on), reference hyper-parameters except a larger step: fitting one fixed batch"""
    from multimodal_transformer_amd import multiTransformer as MT
    torch.manual_seed(1)
    B, T, lengths = 8, 50, [50, 50, 44, 37, 30, 21, 12, 5]
    model = MT.NLPTransformer(512, embed_dim=128, h=8, N=2, device=dev).train()
    mask = R.prefix_mask(lengths, T).to(dev)
    x = torch.tanh(R.gen_normal("fit:x", (B, T, 512), 5)).to(dev)
    tgt = (R.gen_uniform("fit:t", (B, T, 1), 5)).to(dev) * mask
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    hist = []
    for _ in range(60):
        opt.zero_grad(set_to_none=True)
        loss = ((model(x, mask, lengths) - tgt) ** 2).sum() / float(sum(lengths))
        loss.backward()
        opt.step()
        hist.append(loss.item())
    print("loss: first %.4f  last %.4f" % (hist[0], hist[-1]))
    assert np.isfinite(hist).all() and np.mean(hist[-5:]) < 0.6 * np.mean(hist[:5])


def test_flat_adam_matches_torch_adam(dev):
    """optim.FlatAdam == torch.optim.Adam (L2 weight decay, bias-corrected moments; transformer/SFT/train.py:621) on the same gradients:
    the encoder's 34 tensors as ONE range (parameters and gradients are views of flat buffers), loose tensors as ranges of their own"""
    import copy
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    from multimodal_transformer_amd.optim import FlatAdam
    model = MT.NLPTransformer(512, embed_dim=64, h=4, N=2, device=dev)
    model.load_state_dict(R.gen_params(R.shapes_of(model.state_dict()), 37))
    model = model.to(dev).eval()
    ref = copy.deepcopy(model)
    lengths = [20, 13, 6]
    mask = R.prefix_mask(lengths, 20).to(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-2)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-2)
    for i in range(4):
        x = torch.tanh(R.gen_normal("fadam:x%d" % i, (3, 20, 512), 37)).to(dev)
        tgt = (R.gen_uniform("fadam:t%d" % i, (3, 20, 1), 37) * R.prefix_mask(lengths, 20)).to(dev)
        opt.zero_grad(set_to_none=True)
        F.mse_sum_loss_backward(model(x, mask, lengths), tgt, sum(lengths))
        for pm, pr in zip(model.parameters(), ref.parameters()):         # both optimisers see the SAME gradients
            pr.grad = None if pm.grad is None else pm.grad.clone()
        if i == 0:      # the whole encoder stack is one range; embed, decoder and read-out tensors are ranges of their own
            live = [q for q in model.parameters() if q.grad is not None]
            assert len(FlatAdam._ranges(live)) <= len(live) - 30
        opt.step()
        opt_ref.step()
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 2e-6, k


def test_flat_adam_state_dict_round_trip(dev):
    """optimizer.state_dict() / load_state_dict() of FlatAdam carry the moments and the per-parameter step counts, in torch.optim.Adam's
    own format: a run resumed from a checkpoint continues exactly (no lr kick from re-started bias corrections), and the two optimisers
    read each other's checkpoints.  (The reference saves only the model, transformer/SFT/train.py:342-344; resuming the optimiser is what
    torch users expect of a drop-in.)"""
    import copy
    from multimodal_transformer_amd import functional as F, multiTransformer as MT
    from multimodal_transformer_amd.optim import FlatAdam
    model = MT.NLPTransformer(512, embed_dim=64, h=4, N=2, device=dev)
    model.load_state_dict(R.gen_params(R.shapes_of(model.state_dict()), 41))
    model = model.to(dev).eval()
    lengths = [20, 13, 6]
    mask = R.prefix_mask(lengths, 20).to(dev)

    def grads(m, i):
        x = torch.tanh(R.gen_normal("fasd:x%d" % i, (3, 20, 512), 41)).to(dev)
        tgt = (R.gen_uniform("fasd:t%d" % i, (3, 20, 1), 41) * R.prefix_mask(lengths, 20)).to(dev)
        for q in m.parameters():
            q.grad = None
        F.mse_sum_loss_backward(m(x, mask, lengths), tgt, sum(lengths))

    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-2)
    for i in range(3):
        grads(model, i)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert len(sd["state"]) > 30 and all(float(v["step"]) == 3.0 for v in sd["state"].values())
    assert all(float(v["exp_avg_sq"].abs().sum()) > 0 for v in sd["state"].values())
    twin, twin_t = copy.deepcopy(model), copy.deepcopy(model)
    opt2 = FlatAdam(twin.parameters(), lr=1e-3, weight_decay=1e-2)
    opt2.load_state_dict(copy.deepcopy(sd))                              # FlatAdam -> FlatAdam (a copy each: torch keeps the CPU step tensors it is handed)
    opt_t = torch.optim.Adam(twin_t.parameters(), lr=1e-3, weight_decay=1e-2)
    opt_t.load_state_dict(copy.deepcopy(sd))                             # FlatAdam -> torch.optim.Adam
    for i in range(3, 5):
        grads(model, i)
        for m in (twin, twin_t):
            for pm, pr in zip(model.parameters(), m.parameters()):       # the same gradients for all three
                pr.grad = None if pm.grad is None else pm.grad.clone()
        opt.step(); opt2.step(); opt_t.step()
    for (k, a), (_, b), (_, c) in zip(model.state_dict().items(), twin.state_dict().items(), twin_t.state_dict().items()):
        assert torch.equal(a, b), k                                      # resumed run == uninterrupted run, bit for bit
        assert rel_l2(a.cpu().numpy(), c.cpu().numpy()) < 2e-6, k
    # torch.optim.Adam -> FlatAdam
    opt3 = FlatAdam(copy.deepcopy(twin_t).parameters(), lr=1e-3, weight_decay=1e-2)
    opt3.load_state_dict(copy.deepcopy(opt_t.state_dict()))
    assert all(float(v["step"]) == 5.0 for v in opt3.state_dict()["state"].values())


def test_packed_loader_ships_batches_through_pinned_memory(dev, tmp_path):
    """the packed file's loader assembles every batch in page-locked staging buffers and copies it on a stream of its own;
    what arrives on the device equals the host batches of generate_train_batches (the restatement of generateTrainBatch,
    transformer/SFT/train.py:74-106) bit for bit, epoch after epoch (the two staging sets are reused while copies are in flight)."""
    import numpy as np
    from multimodal_transformer_amd import batching as Bt
    rng = np.random.RandomState(9)
    lengths = [int(v) for v in rng.randint(1, 40, size=23)]
    data = {"acoustic": [rng.randn(L, 4, 8).astype(np.float32) for L in lengths],
            "image": [rng.randn(L, 3, 16).astype(np.float32) for L in lengths]}
    target = [rng.rand(L).astype(np.float32) for L in lengths]
    path = str(tmp_path / "d.mmtpack")
    Bt.pack_dataset(path, data, target, lengths)
    ds = Bt.PackedDataset(path)
    loader = Bt.PackedLoader(ds, batch_size=5, device=dev)
    assert all(v.is_pinned() for st in loader._stage for v in list(st["data"].values()) + [st["target"], st["mask"]])
    ref = list(Bt.generate_train_batches(data, target, lengths, batch_size=5))
    for epoch in range(2):
        got = []
        for d, t, m, ls in loader:
            assert t.device.type == "cuda" and all(v.device.type == "cuda" for v in d.values())
            got.append(({k: v.clone() for k, v in d.items()}, t.clone(), m.clone(), ls))      # consume on the current stream
        torch.cuda.synchronize()
        assert len(got) == len(ref) == 5
        for (d0, t0, m0, l0), (d1, t1, m1, l1) in zip(ref, got):
            assert l0 == l1 and torch.equal(t0, t1.cpu()) and torch.equal(m0, m1.cpu())
            for mod in d0:
                assert torch.equal(d0[mod], d1[mod].cpu()), (epoch, mod)
