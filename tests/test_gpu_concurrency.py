"""The multi-stream layer: on which stream a kernel runs and which workspace it is handed (_lib.StreamFork, _lib.WorkspacePool,
functional._SPLIT_STREAMS / _MOD_STREAMS, Encoder.sub_batch_streams).

The kernels are compared with references elsewhere.  Here one call is compared with THE SAME ARITHMETIC issued another way, bit for
bit: a stack run as k sub-batches against the k explicit calls on its pieces, a model with its modalities forked against the model on
one stream, a call on a user's stream against the call alone.  The only comparisons with a tolerance are those with the oracle (the
bounds of test_gpu_dropout.py) and the parameter gradients of the nested case (the 1e-4 of test_gpu_fullsize.py).

  1  sub-batch streams: encoder_stack(nsplit=k) against its explicit pieces, the oracle, its refusals, and the module path
  2  modality streams: every model and stream that forks, against itself under MMT_MODALITY_STREAMS=0
  3  every fork and join edge of StreamFork, forward and backward
  4  two streams of the user's own on one workspace (WorkspacePool)

A lost ordering edge shows only if the racing kernel wins the race, which it usually does not.  The tests of parts 3 and 4 therefore
hold one side back with a gate (gpu_harness.gate) and assert that the gate was still closed when everything was enqueued, and a test
that needs two streams to overlap checks that first (gpu_harness.runs_beside): it fails, naming the premise, if they do not.  Stale
memory hides a lost edge as well (a block the allocator hands out again still holds the previous run's result, and that is the right
result if the inputs were the same), so a gated run is always preceded by a run on OTHER values.
Wherever two users may share a buffer they use one shape and one tag, so a lost edge gives wrong numbers, never an access out of bounds.
"""
import types

import pytest
import torch

import oracle
import recipe as R
from conftest import load_golden, rel_l2
from gpu_harness import (OUT_RTOL, RELU_GRAD_RTOL, PoolRecorder, _report, assert_closed, dev, device_kernel_names, gate,  # noqa: F401
                         load_named, mta, runs_beside, same_bits)
from test_gpu_dropout import _flat_names, _masks

pytestmark = pytest.mark.gpu

N_LAYERS = 2
SHAPES = {"d128_T70": (128, 8, 70, 0.1),          # the two-kernel attention backward
          "d128_T300": (128, 8, 300, 0.1),        # the one-kernel backward, the lane-mask forward
          "d40_T33": (40, 4, 33, 0.25)}           # the generic kernels: a padded head, a ragged tile
BATCH = {2: 3, 3: 5}                              # k -> B: pieces of (2, 1) and of (2, 2, 1) sequences
FORMS = {"plain": {}, "keys": {}, "causal": dict(causal=True), "band": dict(causal=True, span=8)}
SEED = 20240607


def _encoder(d, h, n, dev, seed, p=0.1):
    """-> (an n-layer Encoder with the recipe's parameters on the device, eval mode; those parameters)"""
    MT = mta().multiTransformer
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, R.D_FF, p), p), n)
    p32 = R.gen_params(R.shapes_of(enc.state_dict()), seed)
    enc.load_state_dict(p32)
    return enc.to(dev).eval(), p32


def _lengths(B, T):
    return [T, max(1, int(0.59 * T)), 1, T - 3, int(0.13 * T) + 1][:B]


_STACK = {}


def _stack(name, k, dev):
    """The inputs of one stack case, made once: never written afterwards."""
    if (name, k) not in _STACK:
        F = mta().functional
        d, h, T, p = SHAPES[name]
        B = BATCH[k]
        enc, p32 = _encoder(d, h, N_LAYERS, dev, 71, p)
        c = types.SimpleNamespace(name=name, k=k, d=d, h=h, T=T, p=p, B=B, p32=p32, lengths=_lengths(B, T))
        c.flat = torch.cat([q.detach().reshape(-1) for q in enc.flat_parameters()])
        c.mask_c = R.prefix_mask(c.lengths, T)
        c.x_c = R.gen_normal("conc:x:" + name, (B, T, d), 71)
        c.g_c = R.gen_normal("conc:g:" + name, (B, T, d), 71)
        c.x, c.g, c.mask = c.x_c.to(dev), c.g_c.to(dev), c.mask_c.to(dev)
        c.kl = F.key_lengths(c.mask)
        c.chunks = F._row_chunks(B, k)
        assert [b1 - b0 for b0, b1 in c.chunks] == ([2, 1] if k == 2 else [2, 2, 1])
        torch.cuda.synchronize()
        _STACK[(name, k)] = c
    return _STACK[(name, k)]


def _call(c, form, b0=0, b1=None, **kw):
    """encoder_stack on the rows b0 .. b1 of the case (slices, not copies), forward and backward -> {y, dx, dflat}"""
    F = mta().functional
    b1 = c.B if b1 is None else b1
    x = c.x[b0:b1].detach().requires_grad_()
    flat = c.flat.clone().requires_grad_()
    extra = dict(FORMS[form], key_lengths=c.kl[b0:b1]) if form == "keys" else FORMS[form]
    y = F.encoder_stack(x, c.mask[b0:b1], flat, c.h, R.D_FF, N_LAYERS, **extra, **kw)
    y.backward(c.g[b0:b1])
    return {"y": y.detach(), "dx": x.grad, "dflat": flat.grad}


def _pieces(c, form, seeds=None, **kw):
    """The k explicit calls -> {y, dx} put together and dflat summed in fp32 in chunk order, (g0 + g1) + g2: what copy2d's
    accumulate forms in _encoder_bwd (dst = src * 1 + dst, one rounding per addition: csrc/glue.h)."""
    parts = [_call(c, form, b0, b1, **(kw if seeds is None else dict(kw, seed=seeds[i]))) for i, (b0, b1) in enumerate(c.chunks)]
    dflat = parts[0]["dflat"].clone()
    for q in parts[1:]:
        dflat = dflat + q["dflat"]
    return {"y": torch.cat([q["y"] for q in parts]), "dx": torch.cat([q["dx"] for q in parts]), "dflat": dflat}


def _piece_seeds(s, k):
    return [s] + [mta()._lib.mix64(s, i) for i in range(1, k)]


# ------------------------------------------------------------------------------------------------ 1. sub-batch streams
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_sub_batches_eval_equal_one_call_and_explicit_pieces(dev, name, k):
    """Eval mode, every attention form: y and dx of nsplit=k are those of nsplit=1 (a sequence does not depend on its batch) and of the
    k explicit calls on the rows, the mask and the key lengths of each piece; the parameter gradient is the fp32 sum of the pieces'
    in chunk order.  All bit for bit."""
    c = _stack(name, k, dev)
    failures = []
    for form in FORMS:
        split, one, parts = _call(c, form, nsplit=k), _call(c, form, nsplit=1), _pieces(c, form)
        same_bits("%s k=%d %s vs nsplit=1" % (name, k, form), {n: split[n] for n in ("y", "dx")}, {n: one[n] for n in ("y", "dx")},
                  failures)
        same_bits("%s k=%d %s vs pieces" % (name, k, form), split, parts, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_sub_batches_train_use_their_chunk_seeds(dev, name, k):
    """Train mode: piece i of nsplit=k with the int seed s is the explicit call on its rows with the seed s (i = 0) or mix64(s, i),
    and with a list of k int seeds the explicit call with seed[i].  Bit for bit, every attention form."""
    c = _stack(name, k, dev)
    failures = []
    for form in FORMS:
        split = _call(c, form, nsplit=k, dropout_p=c.p, seed=SEED)
        same_bits("%s k=%d %s int seed" % (name, k, form), split, _pieces(c, form, _piece_seeds(SEED, k), dropout_p=c.p), failures)
    own = [SEED + 17 * i + 5 for i in range(k)]
    for seeds in (own, tuple(own)):
        split = _call(c, "plain", nsplit=k, dropout_p=c.p, seed=seeds)
        same_bits("%s k=%d %s of seeds" % (name, k, type(seeds).__name__), split, _pieces(c, "plain", own, dropout_p=c.p), failures)
    with torch.no_grad():
        y_eval = mta().functional.encoder_stack(c.x, c.mask, c.flat, c.h, R.D_FF, N_LAYERS, nsplit=k)
    assert float((y_eval - split["y"]).abs().max()) > 1e-2, "dropout did not happen"
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("k", [2, 3])
def test_sub_batches_draw_masks_of_their_own(dev, k):
    """Every sequence of the batch is the same sequence.  In eval mode every row of y is then the same; in train mode the first rows of
    the pieces differ from each other because the pieces' seeds do, and are the same again when the caller gives every piece one seed
    (so the comparison does see the masks)."""
    F = mta().functional
    c = _stack("d128_T70", k, dev)
    x = c.x[:1].expand(c.B, c.T, c.d).contiguous()
    mask = torch.ones(c.B, c.T, 1, device=dev)
    firsts = [b0 for b0, _ in c.chunks]
    with torch.no_grad():
        y_eval = F.encoder_stack(x, mask, c.flat, c.h, R.D_FF, N_LAYERS, nsplit=k)
        y = F.encoder_stack(x, mask, c.flat, c.h, R.D_FF, N_LAYERS, dropout_p=c.p, seed=SEED, nsplit=k)
        y_one = F.encoder_stack(x, mask, c.flat, c.h, R.D_FF, N_LAYERS, dropout_p=c.p, seed=[SEED] * k, nsplit=k)
    for i in firsts[1:]:
        assert torch.equal(y_eval[i], y_eval[0])
        assert torch.equal(y_one[i], y_one[0])
    for n, i in enumerate(firsts):
        for j in firsts[n + 1:]:
            assert float((y[i] - y[j]).abs().max()) > 1e-2, "pieces starting at rows %d and %d drew the same masks" % (i, j)


@pytest.mark.parametrize("name,k", [("d128_T300", 2), ("d40_T33", 3)])
def test_sub_batches_train_against_the_oracle(dev, name, k):
    """The masks of every piece rebuilt from its chunk seed (test_gpu_dropout.py's _masks) and the oracle run piece by piece with them:
    y, dx and the summed parameter gradients under that file's bounds."""
    c = _stack(name, k, dev)
    got = _call(c, "plain", nsplit=k, dropout_p=c.p, seed=SEED)
    pd = {n: v.double().clone().requires_grad_() for n, v in c.p32.items()}
    xd = c.x_c.double().clone().requires_grad_()
    refs = []
    for (b0, b1), seed in zip(c.chunks, _piece_seeds(SEED, k)):
        drops = _masks(dev, c.p, seed, N_LAYERS, b1 - b0, c.T, c.d, c.h, R.D_FF)
        refs.append(oracle.encoder_stack(pd, "", xd[b0:b1], c.mask_c[b0:b1].double(), c.h, drops))
    ref = torch.cat(refs)
    (ref * c.g_c.double()).sum().backward()
    tag = "split train %s k=%d" % (name, k)
    assert _report(tag + " out", got["y"].cpu(), ref.detach()) < OUT_RTOL
    assert _report(tag + " dx", got["dx"].cpu(), xd.grad) < RELU_GRAD_RTOL
    ref_flat = torch.cat([pd[n].grad.reshape(-1) for n in _flat_names(N_LAYERS)])
    assert _report(tag + " dparams", got["dflat"].cpu(), ref_flat) < RELU_GRAD_RTOL


def test_sub_batch_refusals_come_before_any_launch(dev, monkeypatch):
    """One DeviceSeed for several pieces (its state word would be read and advanced from two streams) and a seed list shorter than k:
    ValueError, and nothing has happened by then: no kernel (the profiler's device activity), no workspace taken from the pool (on an
    empty pool taking one launches its zero fill, and a refusal behind it would never hand the buffer back), no stream forked."""
    F, L = mta().functional, mta()._lib
    c = _stack("d128_T70", 2, dev)
    ds = L.DeviceSeed(dev, 5)
    torch.cuda.synchronize()
    rec = PoolRecorder(L.POOL, monkeypatch)
    L.POOL.clear()
    forks = []
    begin = F._SPLIT_STREAMS.begin
    monkeypatch.setattr(F._SPLIT_STREAMS, "begin", lambda device, n: forks.append(n) or begin(device, n))

    def stack(**kw):
        return F.encoder_stack(c.x, c.mask, c.flat, c.h, R.D_FF, N_LAYERS, dropout_p=0.1, **kw)

    def refused():
        with pytest.raises(ValueError, match="need a list of 2 DeviceSeeds, got one"):
            stack(seed=ds, nsplit=2)
        with pytest.raises(ValueError, match="one seed per sub-batch stream"):
            stack(seed=[1, 2], nsplit=3)
        with pytest.raises(ValueError, match="one seed per sub-batch stream"):
            stack(seed=[ds], nsplit=2)

    rec.phase("refused")
    _, names = device_kernel_names(refused)
    assert rec.log["refused"]["got"] == [] and forks == []
    rec.phase("runs")
    _, seen = device_kernel_names(lambda: stack(seed=[ds, L.DeviceSeed(dev, 6)], nsplit=2))      # what is asked for instead runs
    assert len(rec.log["runs"]["got"]) == 2 and forks == [2]
    if seen is not None:                                        # the profiler reports device activity here: then none for the refusals
        assert names is None, names


def _sub_batch_encoder(dev):
    enc, p32 = _encoder(128, 8, N_LAYERS, dev, 47)
    enc.sub_batch_streams, enc.sub_batch_min_windows = 2, 0
    return enc, p32


def test_sub_batch_rule_of_the_module(dev, monkeypatch):
    """Encoder._sub_batch_streams: the instance's count (MMT_ENCODER_STREAMS overrides it, read at every call), at most one piece per
    sequence, and 1 for a batch of one, below sub_batch_min_windows and on a side lane (a piece of a fork does not fork again)."""
    F = mta().functional
    enc, _ = _sub_batch_encoder(dev)
    x = torch.zeros(3, 70, 128, device=dev)
    monkeypatch.delenv("MMT_ENCODER_STREAMS", raising=False)
    monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
    assert enc._sub_batch_streams(x) == 2
    assert enc._sub_batch_streams(x[:1]) == 1
    enc.sub_batch_min_windows = 3 * 70 + 1
    assert enc._sub_batch_streams(x) == 1
    enc.sub_batch_min_windows = 3 * 70
    assert enc._sub_batch_streams(x) == 2
    monkeypatch.setenv("MMT_ENCODER_STREAMS", "1")
    assert enc._sub_batch_streams(x) == 1
    monkeypatch.setenv("MMT_ENCODER_STREAMS", "8")
    assert enc._sub_batch_streams(x) == 3
    monkeypatch.delenv("MMT_ENCODER_STREAMS")
    main, streams = F._MOD_STREAMS.begin(dev, 2)
    assert streams[1] is not main
    with torch.cuda.stream(streams[1]):
        assert enc._sub_batch_streams(x) == 1
    assert enc._sub_batch_streams(x) == 2
    F._MOD_STREAMS.end(main, streams)
    user = torch.cuda.Stream(device=dev)                         # a stream of the caller's own is no side lane
    with torch.cuda.stream(user):
        assert enc._sub_batch_streams(x) == 2
    torch.cuda.synchronize()


def test_sub_batch_module_fresh_masks_per_graph_replay(dev):
    """Encoder.sub_batch_streams = 2 in train mode, captured and replayed: each piece has a DeviceSeed of its own (index 0, 1), both
    advance at every replay, the replays differ, and one replay is reproduced through the oracle from the two seeds peeked before it."""
    from multimodal_transformer_amd import graphs
    L = mta()._lib
    B, T, d, h, p = 3, 70, 128, 8, 0.1
    enc, p32 = _sub_batch_encoder(dev)
    enc.train()
    params = list(enc.parameters())
    lengths = _lengths(B, T)
    x_c, g_c, mask_c = R.gen_normal("conc:graph:x", (B, T, d), 47), R.gen_normal("conc:graph:g", (B, T, d), 47), R.prefix_mask(lengths, T)
    xg, gd, md = x_c.to(dev).requires_grad_(), g_c.to(dev), mask_c.to(dev)
    out = {}

    def step():
        for q in params:
            q.grad = None
        xg.grad = None
        y = enc(xg, md)
        (y * gd).sum().backward()
        out["y"] = y.detach()                                    # no reference to the step's autograd graph survives the step

    assert enc._sub_batch_streams(xg) == 2
    graph, _ = graphs.capture_step(step, warmup=2)
    results = []
    for _ in range(3):
        seeds = [L.device_seed(enc, 1, index=i).peek() for i in range(2)]
        graph.replay()
        torch.cuda.synchronize()
        assert all(L.device_seed(enc, 1, index=i).peek() != seeds[i] for i in range(2)), "a piece's launch did not advance its seed"
        results.append((seeds, out["y"].clone(), xg.grad.clone(), torch.cat([q.grad.reshape(-1) for q in enc.flat_parameters()]).clone()))
    assert len({s for r in results for s in r[0]}) == 6
    for i, j in ((0, 1), (1, 2), (0, 2)):
        assert float((results[i][1] - results[j][1]).abs().max()) > 1e-2, "replays %d and %d drew the same masks" % (i, j)
    seeds, y, dx, dflat = results[2]
    pd = {n: v.double().clone().requires_grad_() for n, v in p32.items()}
    xd = x_c.double().clone().requires_grad_()
    refs = []
    for (b0, b1), seed in zip(mta().functional._row_chunks(B, 2), seeds):
        drops = _masks(dev, p, seed, N_LAYERS, b1 - b0, T, d, h, R.D_FF)
        refs.append(oracle.encoder_stack(pd, "", xd[b0:b1], mask_c[b0:b1].double(), h, drops))
    ref = torch.cat(refs)
    (ref * g_c.double()).sum().backward()
    assert _report("split devseed out", y.cpu(), ref.detach()) < OUT_RTOL
    assert _report("split devseed dx", dx.cpu(), xd.grad) < RELU_GRAD_RTOL
    ref_flat = torch.cat([pd[n].grad.reshape(-1) for n in _flat_names(N_LAYERS)])
    assert _report("split devseed dparams", dflat.cpu(), ref_flat) < RELU_GRAD_RTOL


# ------------------------------------------------------------------------------------------------ models
def _model_case(kind, dev):
    """-> (model in eval mode, [two sets of inputs {name: tensor}], forward(inputs) -> the output) at the small models' shapes.  The raw
    front end's inputs are data: conv_maxpool gives no gradient for its windows, and _model_run asks for none (`model.raw`)."""
    from multimodal_transformer_amd import models as MM
    MT = mta().multiTransformer
    B, T = 3, 40
    lengths = [T, 23, 1]
    mask = R.prefix_mask(lengths, T).to(dev)
    mods = R.MODS_AVL

    def sets(shape_of, tag):
        return [{m: R.gen_normal("conc:%s:%d:%s" % (tag, i, m), shape_of(m), 83).to(dev) for m in mods} for i in range(2)]

    if kind == "mft":
        model = MT.MultiTransformer(mods, R.EMBED_AVL, N=N_LAYERS, device=dev)
        vals, fwd = sets(lambda m: (B, T, R.EMBED_AVL[m]), kind), lambda ins: model(ins, mask, lengths)
    elif kind == "b3":
        model = MT.MultiTransformerB3(mods, R.EMBED_AVL, device=dev)
        vals, fwd = sets(lambda m: (B, T, R.EMBED_AVL[m]), kind), lambda ins: model(ins, mask, lengths)
    elif kind == "mfn":
        dims = {"acoustic": 40, "image": 24, "linguistic": 56}
        model = MT.MFN(mods, dims, 1, device=dev)
        vals, fwd = sets(lambda m: (T, B, dims[m]), kind), lambda ins: model(ins)
    else:                                                        # the raw front end at its fixture's shape
        lengths = [int(v) for v in load_golden("fe_model_mft")["lengths"]]
        B, T = len(lengths), 6
        mask = R.prefix_mask(lengths, T).to(dev)
        model = MM.MultiCNNTransformerMFT(mods, R.FE_DIMS, R.FE_EMBED_MFT, device=dev)
        vals, fwd = sets(lambda m: (B, T, R.FE_WINDOW[m], R.FE_DIMS[m]), kind), lambda ins: model(ins, lengths, mask)
    load_named(model, 83)
    model.raw = kind == "frontend"
    return model.to(dev).eval(), vals, fwd


def _model_run(model, fwd, vals, g=None):
    """forward and backward on fresh leaves -> ({y, d:<input>, p:<parameter>}, the g used)"""
    for q in model.parameters():
        q.grad = None
    ins = {n: v.clone().requires_grad_(not model.raw) for n, v in vals.items()}
    y = fwd(ins)
    if g is None:
        g = R.gen_normal("conc:model:g", tuple(y.shape), 83).to(y.device)
    y.backward(g)
    torch.cuda.synchronize()
    out = {"y": y.detach()}
    out.update(("d:" + n, v.grad) for n, v in ins.items())
    out.update(("p:" + n, q.grad) for n, q in model.named_parameters())
    return out, g


def _spy_forks(fork, monkeypatch):
    """-> the list that collects, per begin() of `fork`, how many of the streams it handed out are not the caller's"""
    seen, begin = [], fork.begin

    def spy(device, n):
        main, streams = begin(device, n)
        seen.append(sum(1 for s in streams if s is not main))
        return main, streams
    monkeypatch.setattr(fork, "begin", spy)
    return seen


def _side_streams(fork):
    return [s for v in fork._side.values() for s in v]


# ------------------------------------------------------------------------------------------------ 2. modality streams on against off
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("kind", ["mft", "b3", "mfn", "frontend"])
def test_modality_streams_change_no_bit(dev, monkeypatch, kind, mode):
    """MMT_MODALITY_STREAMS=0 (what bench.py and the profiling tools measure under) against the default: the output, every input
    gradient and every parameter gradient, bit for bit, in eval mode and (the generator seeded alike, so the host-drawn dropout seeds
    come in the same order) in train mode.  The default run did fork, the other one did not.  One run comes first: a module's first
    train-mode call draws twice from the generator, once for the DeviceSeed it creates (_lib.next_dropout_seed)."""
    F = mta().functional
    model, vals, fwd = _model_case(kind, dev)
    model.train(mode == "train")
    monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
    _model_run(model, fwd, vals[1])
    forks = _spy_forks(F._MOD_STREAMS, monkeypatch)
    runs = {}
    for switch in ("0", None):
        if switch is None:
            monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
        else:
            monkeypatch.setenv("MMT_MODALITY_STREAMS", switch)
        before = len(_side_streams(F._MOD_STREAMS))
        del forks[:]
        torch.manual_seed(11)
        runs[switch], _ = _model_run(model, fwd, vals[0])
        assert forks, "the model never asked for modality streams"
        if switch == "0":
            assert set(forks) == {0} and len(_side_streams(F._MOD_STREAMS)) == before
        else:
            assert set(forks) == {len(R.MODS_AVL) - 1} and len(_side_streams(F._MOD_STREAMS)) >= len(R.MODS_AVL) - 1
    if mode == "train":
        torch.manual_seed(12)
        other, _ = _model_run(model, fwd, vals[0])
        assert not torch.equal(other["y"], runs[None]["y"]), "dropout did not happen"
    live = [n for n, v in runs[None].items() if v is not None]
    assert len(live) > (10 if kind == "mfn" else 20)
    failures = []
    same_bits("%s %s forked vs one stream" % (kind, mode), runs[None], runs["0"], failures)
    assert not failures, "\n".join(failures)


def _stream_model(dev):
    """test_gpu_mfn_stream.py's small causal MFT -> (model, {mod: width})"""
    MT = mta().multiTransformer
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    model = MT.MultiTransformer(mods, wes, N=2, h=4, device=dev, embed_dim={"acoustic": 40, "emotient": 32})
    load_named(model, 83)
    MT.causal_attention(model)
    return model.eval(), wes


def _open(model, slots, B, capacity):
    s = model.slot_stream(B, capacity) if slots else model.stream(B, capacity)
    s.reset()
    return s


@pytest.mark.parametrize("slots", [False, True], ids=["host", "slots"])
def test_modality_streams_change_no_bit_of_a_stream_step(dev, monkeypatch, slots):
    """_GateStream / _GateSlotStream of the MFT, five steps: every step's prediction with the modalities forked equals the one on one stream."""
    F = mta().functional
    model, wes = _stream_model(dev)
    B, steps = 3, 5
    xs = [{m: R.gen_normal("conc:step:%d:%s" % (t, m), (B, w), 83).to(dev) for m, w in wes.items()} for t in range(steps)]
    mask = R.prefix_mask([5, 3, 1], steps).to(dev)
    forks = _spy_forks(F._MOD_STREAMS, monkeypatch)
    runs = {}
    for switch in ("0", None):
        if switch is None:
            monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
        else:
            monkeypatch.setenv("MMT_MODALITY_STREAMS", switch)
        del forks[:]
        s = _open(model, slots, B, steps)
        assert s.modality_streams
        runs[switch] = {"t%d" % t: s.step(xs[t], mask[:, t].contiguous()).clone() for t in range(steps)}
        torch.cuda.synchronize()
        assert forks == [0 if switch == "0" else 1] * steps
    assert float((runs[None]["t0"] - runs[None]["t1"]).abs().max()) > 0
    failures = []
    same_bits("stream step forked vs one stream", runs[None], runs["0"], failures)
    assert not failures, "\n".join(failures)


def test_nested_forks_only_the_callers_modality_splits(dev, monkeypatch):
    """An MFT whose encoders have sub_batch_streams = 2: the first modality runs on the caller's stream and splits, the others run on
    side lanes and do not (Encoder._sub_batch_streams: a piece of a fork does not fork again); on one stream every modality splits.  Eval
    mode: the output and every input gradient equal the un-split model's bit for bit, the parameter gradients under the 1e-4 of
    test_gpu_fullsize.py::test_sub_batch_streams_match_single_stream (two pieces summed instead of one sum over the batch)."""
    MT = mta().multiTransformer
    model, vals, fwd = _model_case("mft", dev)
    monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
    monkeypatch.delenv("MMT_ENCODER_STREAMS", raising=False)
    plain, g = _model_run(model, fwd, vals[0])
    asked, rule = [], MT.Encoder._sub_batch_streams

    def spy(self, x):
        k = rule(self, x)
        asked.append(k)
        return k
    monkeypatch.setattr(MT.Encoder, "_sub_batch_streams", spy)
    for enc in model.transformer.values():
        enc.sub_batch_streams, enc.sub_batch_min_windows = 2, 0
    split, _ = _model_run(model, fwd, vals[0], g)
    assert asked == [2, 1, 1], asked
    del asked[:]
    monkeypatch.setenv("MMT_MODALITY_STREAMS", "0")
    serial, _ = _model_run(model, fwd, vals[0], g)
    assert asked == [2, 2, 2], asked
    failures = []
    for tag, run in (("nested", split), ("nested on one stream", serial)):
        exact = [n for n in plain if not n.startswith("p:")]
        same_bits(tag, {n: run[n] for n in exact}, {n: plain[n] for n in exact}, failures)
        for n in plain:
            if n.startswith("p:") and plain[n] is not None:
                r = rel_l2(run[n].cpu().numpy(), plain[n].cpu().numpy()) if float(plain[n].abs().max()) > 0 else float(run[n].abs().max())
                if not r < 1e-4:
                    failures.append("%s %s: rel-L2 %.3e" % (tag, n, r))
            elif n.startswith("p:") and run[n] is not None:
                failures.append("%s %s: a gradient where the un-split model has none" % (tag, n))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 3. every fork and join edge
class _StackTarget:
    """encoder_stack(nsplit=k) on B = BATCH[k] sequences at T = 70"""
    grad = True

    def __init__(self, dev, k):
        self.c, self.k, self.fork, self.n_side = _stack("d128_T70", k, dev), k, mta().functional._SPLIT_STREAMS, k - 1
        self.flat = self.c.flat.clone().requires_grad_()
        self.values = [{"x": self.c.x}, {"x": R.gen_normal("conc:edge:x", tuple(self.c.x.shape), 5).to(dev)}]
        self.g = [self.c.g, R.gen_normal("conc:edge:g", tuple(self.c.x.shape), 5).to(dev)]

    def forward(self, ins):
        return mta().functional.encoder_stack(ins["x"], self.c.mask, self.flat, self.c.h, R.D_FF, N_LAYERS, nsplit=self.k)

    def zero(self):
        self.flat.grad = None

    def param_grads(self):
        return {"p:flat": self.flat.grad}

    def sides(self):
        return _side_streams(self.fork)


class _MftTarget:
    """MultiTransformer forward and backward, three modalities"""
    grad = True

    def __init__(self, dev):
        self.model, self.values, self.fwd = _model_case("mft", dev)
        self.fork, self.n_side = mta().functional._MOD_STREAMS, 2
        self.g = [R.gen_normal("conc:edge:mft:g%d" % i, (3, 40, 1), 5).to(dev) for i in range(2)]

    def forward(self, ins):
        return self.fwd(ins)

    def zero(self):
        for q in self.model.parameters():
            q.grad = None

    def param_grads(self):
        """the per-modality encoders' and embeds' gradients: what the side streams produce"""
        return {"p:" + n: q.grad for n, q in self.model.named_parameters() if n.startswith(("transformer_", "embed_"))}

    def sides(self):
        return _side_streams(self.fork)


class _StepTarget:
    """_GateStream.step of the small causal MFT at t = 0 (the stream is reset before every step)"""
    grad = False

    def __init__(self, dev):
        self.model, wes = _stream_model(dev)
        self.fork, self.n_side = mta().functional._MOD_STREAMS, 1
        self.stream = _open(self.model, False, 3, 4)
        self.mask_t = torch.ones(3, device=dev)
        self.values = [{m: R.gen_normal("conc:edge:step:%d:%s" % (i, m), (3, w), 5).to(dev) for m, w in wes.items()} for i in range(2)]

    def forward(self, ins):
        self.stream.reset()
        return self.stream.step(ins, self.mask_t)

    def zero(self):
        pass

    def sides(self):
        return _side_streams(self.fork)


TARGETS = {"stack_k2": lambda dev: _StackTarget(dev, 2), "stack_k3": lambda dev: _StackTarget(dev, 3), "mft": _MftTarget,
           "gate_step": _StepTarget}
GRAD_TARGETS = [n for n in TARGETS if n != "gate_step"]


def _leaves(t, i):
    return {n: (v.clone().requires_grad_() if t.grad else v.clone()) for n, v in t.values[i].items()}


def _grads(t, ins):
    out = {"d:" + n: v.grad.clone() for n, v in ins.items()}
    out.update((n, None if v is None else v.clone()) for n, v in t.param_grads().items())
    return out


def _alone(t, i):
    """the target on the values i with nothing held back -> {y, and with a backward: d:<input>, p:<parameter>}"""
    t.zero()
    ins = _leaves(t, i)
    y = t.forward(ins)
    out = {"y": y.detach().clone()}
    if t.grad:
        y.backward(t.g[i])
        out.update(_grads(t, ins))
    torch.cuda.synchronize()
    return out


_SIDES = []


def _own_side_streams(fork, n, dev, monkeypatch):
    """Make the side streams of `fork` n streams that run beside the caller's stream, both ways, for the length of the test.  Which
    hardware queue a stream lands on depends on how many streams the process has made before, and a side stream that shares the
    caller's queue serialises with it: an edge test on it would pass whether or not the edge is there.  Up to eight fresh streams are
    tried, once per process; the lanes are registered as StreamFork.begin registers them."""
    L, main = mta()._lib, torch.cuda.current_stream(dev)
    for _ in range(8):
        if len(_SIDES) >= n:
            break
        s = torch.cuda.Stream(device=dev)
        if runs_beside(main, s) and runs_beside(s, main):
            _SIDES.append(s)
    assert len(_SIDES) >= n, ("premise: of eight fresh streams only %d run beside the caller's stream (hardware queues?), %d are needed"
                              % (len(_SIDES), n))
    for s in _SIDES[:n]:                                         # for good: a lane number is never given to a second stream
        L.SIDE_LANES.setdefault(int(s.cuda_stream), len(L.SIDE_LANES) + 1)
    monkeypatch.setattr(fork, "_side", {str(dev): list(_SIDES[:n])})


def _edge_case(name, dev, monkeypatch):
    """-> (the target warmed up on side streams that overlap with the caller's, its result on the values 0); the last run before the
    gated one is on the values 1, so that memory handed out again holds other numbers than the right ones"""
    monkeypatch.delenv("MMT_MODALITY_STREAMS", raising=False)
    t = TARGETS[name](dev)
    _own_side_streams(t.fork, t.n_side, dev, monkeypatch)
    _alone(t, 1)
    base = _alone(t, 0)
    _alone(t, 1)
    assert t.sides() == _SIDES[:t.n_side], "the target forked onto other side streams than the ones it was given"
    return t, base, torch.cuda.current_stream(dev)


_BESIDE = {}


def _assert_beside(a, b, what):
    key = (int(a.cuda_stream), int(b.cuda_stream))
    if key not in _BESIDE:
        _BESIDE[key] = runs_beside(a, b)
    assert _BESIDE[key], "premise: %s does not run beside the gated stream (one hardware queue?), so the edge under test cannot show" % what


def _compare(tag, got, base):
    failures = []
    same_bits(tag, got, {n: base[n] for n in got}, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(TARGETS))
def test_fork_edge_forward(dev, monkeypatch, name):
    """The inputs are NaN until a copy behind a gate on the caller's stream fills them in: a side stream that does not wait for the
    caller's stream (StreamFork.begin) reads NaN."""
    t, base, main = _edge_case(name, dev, monkeypatch)
    for s in t.sides():
        _assert_beside(main, s, "a side stream")
    bufs = {n: torch.full_like(v, float("nan")) for n, v in t.values[0].items()}
    torch.cuda.synchronize()
    ev = gate(main)
    for n, b in bufs.items():
        b.copy_(t.values[0][n])
    y = t.forward({n: (b.requires_grad_() if t.grad else b) for n, b in bufs.items()})
    assert_closed(ev)
    torch.cuda.synchronize()
    _compare(name + " forward behind a gated caller", {"y": y.detach()}, base)


@pytest.mark.parametrize("name", list(TARGETS))
def test_join_edge_forward(dev, monkeypatch, name):
    """Every side stream is held back by a gate and the output is copied on the caller's stream at once: without the caller's stream
    waiting for the side streams (StreamFork.end) the copy, or the kernel of the caller's stream that consumes the side streams'
    results, reads them before they are written."""
    t, base, main = _edge_case(name, dev, monkeypatch)
    for s in t.sides():
        _assert_beside(s, main, "the caller's stream")
    ins = _leaves(t, 0)
    poison = torch.full_like(base["y"], float("nan"))            # best effort: the allocator most likely hands this block out for y
    del poison
    torch.cuda.synchronize()
    evs = [gate(s) for s in t.sides()]
    y = t.forward(ins)
    got = y.detach().clone()
    assert_closed(*evs)
    torch.cuda.synchronize()
    _compare(name + " forward with gated side streams", {"y": got}, base)


@pytest.mark.parametrize("name", GRAD_TARGETS)
def test_fork_edge_backward(dev, monkeypatch, name):
    """The incoming gradient is NaN until a copy behind a gate on the caller's stream fills it in: a backward piece on a side stream that
    does not wait for the caller's stream reads NaN.  The stack forks its backward itself (_encoder_bwd: StreamFork.begin).  The MFT's
    backward is autograd's: the engine replays every node on the stream of its forward and orders the hand-over itself, so that case
    holds the engine to it and no edge of StreamFork can fail it."""
    t, base, main = _edge_case(name, dev, monkeypatch)
    for s in t.sides():
        _assert_beside(main, s, "a side stream")
    t.zero()
    ins = _leaves(t, 0)
    y = t.forward(ins)
    g = torch.full_like(t.g[0], float("nan"))
    torch.cuda.synchronize()
    ev = gate(main)
    g.copy_(t.g[0])
    y.backward(g)
    assert_closed(ev)
    torch.cuda.synchronize()
    _compare(name + " backward behind a gated caller", _grads(t, ins), base)


@pytest.mark.parametrize("name", GRAD_TARGETS)
def test_join_edge_backward(dev, monkeypatch, name):
    """Every side stream is held back by a gate during the backward, and the input gradients and the parameter gradients are copied on
    the caller's stream as soon as backward() returns.  The stack joins its backward itself (_encoder_bwd: StreamFork.end, then the sum
    of the pieces' parameter gradients on the caller's stream); for the MFT the engine makes the stream that called backward() wait
    for the streams its nodes ran on, as in test_fork_edge_backward."""
    t, base, main = _edge_case(name, dev, monkeypatch)
    for s in t.sides():
        _assert_beside(s, main, "the caller's stream")
    t.zero()
    ins = _leaves(t, 0)
    y = t.forward(ins)
    torch.cuda.synchronize()
    evs = [gate(s) for s in t.sides()]
    y.backward(t.g[0])
    got = _grads(t, ins)
    assert_closed(*evs)
    torch.cuda.synchronize()
    _compare(name + " backward with gated side streams", got, base)


# ------------------------------------------------------------------------------------------------ 4. two user streams
def _overlapping_pair(dev):
    """Two fresh streams of which the second runs beside the first; up to four are drawn (the runtime deals streams onto a few
    hardware queues, and two on one queue serialise)."""
    streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
    for s2 in streams[1:]:
        if runs_beside(streams[0], s2):
            return streams[0], s2
    pytest.fail("premise: none of four fresh streams ran beside the first one, so two user streams cannot overlap here")


def _user_case(kind, dev):
    """-> (run(u): the inputs of user u cloned as leaves on the CURRENT stream and the forward -> (y, leaves, g); the tag of the
    workspace).  A and B share the shape and so the tag; their values differ."""
    F = mta().functional
    B, T, d, h = 2, 70, 128, 8
    mask = R.prefix_mask([T, 41], T).to(dev)
    if kind == "sdpa":
        src = {u: [R.gen_normal("two:%s:%s" % (u, n), (B, T, d), 61).to(dev) for n in "qkvg"] for u in "AB"}

        def run(u):
            leaves = [v.clone().requires_grad_() for v in src[u][:3]]
            return F.sdpa(leaves[0], leaves[1], leaves[2], mask, h), leaves, src[u][3]
        return run, "sdpa"
    enc, _ = _encoder(d, h, N_LAYERS, dev, 61)
    flat = torch.cat([q.detach().reshape(-1) for q in enc.flat_parameters()])
    src = {u: [R.gen_normal("two:enc:%s:%s" % (u, n), (B, T, d), 61).to(dev) for n in "xg"] for u in "AB"}

    def run(u):
        leaves = [src[u][0].clone().requires_grad_(), flat.clone().requires_grad_()]
        return F.encoder_stack(leaves[0], mask, leaves[1], h, R.D_FF, N_LAYERS), leaves, src[u][1]
    return run, "encoder"


def _done(y, leaves):
    return dict([("y", y.detach())] + [("d%d" % i, v.grad) for i, v in enumerate(leaves)])


@pytest.mark.parametrize("kind", ["sdpa", "encoder"])
def test_two_user_streams_share_a_workspace_in_order(dev, monkeypatch, kind):
    """Two streams of the user's own are both lane 0 of the pool.  A runs forward and backward on s1 behind a gate, so all of it is only
    queued when its workspace goes back to the pool; B's forward on s2 is then handed that very buffer (asserted) and holds it until
    its backward.  Without an ordering edge from A's last launch to B's first, B's forward runs on a buffer whose zero fill is still
    queued, and A's kernels run over B's saved state once the gate opens: B's gradients come from A's data.  (Before the pool ordered
    the two: sdpa gave B wrong dq, dk, dv in 14194 to 17907 of 17920 entries; the encoder stack, whose forward depends on the zeroed pads,
    a wrong y as well.)  Everything equals the same call alone, bit for bit.  sdpa and the encoder stack both hold their buffer from
    forward to backward: the edge belongs to the pool, not to one Function."""
    L = mta()._lib
    run, tag0 = _user_case(kind, dev)
    ref = {}
    for u in "AB":                                               # each user alone, eagerly, on the caller's stream
        L.POOL.clear()
        y, leaves, g = run(u)
        y.backward(g)
        ref[u] = _done(y, leaves)
    torch.cuda.synchronize()
    s1, s2 = _overlapping_pair(dev)
    rec = PoolRecorder(L.POOL, monkeypatch)
    L.POOL.clear()
    torch.cuda.synchronize()

    rec.phase("A")
    ev = gate(s1)
    with torch.cuda.stream(s1):
        yA, lA, gA = run("A")
        yA.backward(gA)                                          # queued behind the gate; A's workspace is back in the pool now
    rec.phase("B")
    with torch.cuda.stream(s2):
        yB, lB, gB = run("B")
    assert_closed(ev)
    assert rec.assert_reused(dirtier="A", probe="B", tags={tag0}) == 1, "the scenario did not happen: B was not handed A's workspace"
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        yB.backward(gB)
    torch.cuda.synchronize()
    failures = []
    same_bits(kind + " A (s1, gated)", _done(yA, lA), ref["A"], failures)
    same_bits(kind + " B (s2, on A's workspace)", _done(yB, lB), ref["B"], failures)
    assert not failures, "\n".join(failures)
