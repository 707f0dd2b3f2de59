"""CPU: the LSTM baselines with the softmax over the taps, and their one-window step, without a GPU.  The reference
(tests/lstm_stream_ref.py): stepped against batch, batch against a restatement of the reference model's forward with the softmax over
the taps, and, rounded, against the composition of bf16_ref's pieces.  The surface (models.attend_over_taps, the streams, the new C
entries in the header, exported and bound), the refusals before anything touches a device, and the stand-alone host check of the limits
and the state layout (tools/lstm_step_plan_check.cpp) under ASan / UBSan."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import bf16_ref as R
import conftest
import lstm_stream_ref as LS
import recipe as G

MMT_EINVAL, MMT_EUNSUPPORTED = 1, 2

# (in, E, H, layers, taps, B, T)
CASES = [(8, 8, 4, 1, 1, 2, 3), (12, 12, 20, 1, 3, 3, 7), (20, 16, 12, 2, 5, 3, 12), (10, 8, 8, 4, 16, 2, 6), (16, 8, 8, 3, 4, 4, 9)]
IDS = ["in%d_E%d_H%d_N%d_L%d_B%d_T%d" % c for c in CASES]


def _case(c, hole=False):
    I, E, H, NL, L, B, T = c
    p = LS.params(I, E, H, NL, L, tag="lstm_stream_cpu")
    x = G.gen_normal("lstm_stream_cpu:x:%d:%d" % (I, T), (B, T, I), 7).double()
    mask = G.prefix_mask([max(1, T - (2 * b) % T) for b in range(B)], T).double().reshape(B, T)
    if hole:                                                # a blanked window in the middle of a recording: the ring must hold m_t * h_t
        mask = torch.ones(B, T, dtype=torch.float64)
        mask[0, T // 2] = 0.0
        mask[B - 1, 1] = 0.0
    return p, x, mask


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("hole", [False, True], ids=["ragged", "hole"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_stepped_is_batch(c, hole):
    """rounding off: the stepped reference, its ring written as the kernel writes it, equals the batch reference to fp64 noise, on
    ragged prefix masks and on a mask with a hole in the middle (which a ring of unmasked h_t would fail)"""
    p, x, mask = _case(c, hole)
    s, b = LS.stepped(p, x, mask, rounding=False), LS.batch(p, x, mask, rounding=False)
    err = (s - b).abs().max().item()
    print("lstm stream reference %s: stepped vs batch %.3e" % (IDS[CASES.index(c)], err))
    assert s.shape == b.shape == (c[5], c[6], 1) and err <= 1e-12 and b.abs().max() > 0
    assert (s[mask == 0] == 0).all()
    if hole and c[4] > 1 and c[6] > 2:                      # the hole matters: a ring of unmasked rows moves the windows behind it
        rows = [r for r in (0, c[5] - 1)]
        unmasked = LS.batch(p, x, torch.ones_like(mask), rounding=False)
        assert max((unmasked[r] - b[r]).abs()[mask[r] > 0].max().item() for r in rows) > 1e-6


def _restated_reference_forward(p, x, lengths, mask, NL, L):
    """The reference's MultiLSTM.forward in eval mode, restated with torch modules, its softmax moved to the taps (nn.Softmax(dim=2) on
    the (B,T,L) logits): packed nn.LSTM from zero states, outputs zero at padded steps, context[t] = sum_i a[t,i] h[t-i], read-out, mask."""
    B, T, I = x.shape
    E, H = p["embed.1.weight"].shape[0], p["lstm.weight_hh_l0"].shape[1]
    lstm = torch.nn.LSTM(E, H, NL, batch_first=True).double()
    lstm.load_state_dict({k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")})
    lin = torch.nn.functional.linear
    with torch.no_grad():
        embed = torch.relu(lin(x.reshape(-1, I), p["embed.1.weight"], p["embed.1.bias"]))
        logits = lin(torch.relu(lin(embed, p["attn.0.weight"], p["attn.0.bias"])), p["attn.2.weight"], p["attn.2.bias"])
        attn = torch.nn.Softmax(dim=2)(logits.reshape(B, T, L))
        packed = torch.nn.utils.rnn.pack_padded_sequence(embed.reshape(B, T, E), lengths, batch_first=True, enforce_sorted=False)
        h, _ = lstm(packed, (torch.zeros(NL, B, H, dtype=torch.float64), torch.zeros(NL, B, H, dtype=torch.float64)))
        h, _ = torch.nn.utils.rnn.pad_packed_sequence(h, batch_first=True, total_length=T)
        context = torch.zeros(B, T, H, dtype=torch.float64)
        for i in range(min(L, T)):
            context[:, i:] += attn[:, i:, i:i + 1] * h[:, :T - i]
        hid = torch.relu(lin(context.reshape(-1, H), p["decoder.0.weight"], p["decoder.0.bias"]))
        return lin(hid, p["decoder.2.weight"], p["decoder.2.bias"]).reshape(B, T, 1) * mask.reshape(B, T, 1)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_batch_is_the_reference_model_with_the_softmax_over_the_taps(c):
    """rounding off: ``batch`` against the restated forward of the reference's MultiLSTM with nn.Softmax(dim=2) on the reshaped logits"""
    p, x, mask = _case(c)
    lengths = [int(v) for v in mask.sum(dim=1)]
    want = _restated_reference_forward(p, x, lengths, mask, c[3], c[4])
    got = LS.batch(p, x, mask, rounding=False)
    err = (got - want).abs().max().item()
    print("lstm stream reference %s: batch vs the restated model %.3e" % (IDS[CASES.index(c)], err))
    assert got.shape == want.shape and err <= 1e-12 and want.abs().max() > 0


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_rounded_batch_is_the_composition_of_the_bf16_pieces(c):
    """rounding on: ``batch`` equals bf16_ref.linear / lstm_scan and local_attention_taps composed as _LocalAttnLSTM._front / .forward
    compose the kernels, exactly; the stepped reference stays with it to fp64 noise; and the rounding moves the result (so that the
    GPU bounds have something to stay under)"""
    I, E, H, NL, L, B, T = c
    p, x, mask = _case(c)
    embed = R.linear(x, p["embed.1.weight"], p["embed.1.bias"], act=1)
    tm = embed.transpose(0, 1)
    hid = R.linear(tm, p["attn.0.weight"], p["attn.0.bias"], act=1)
    z = R.linear(hid, p["attn.2.weight"], p["attn.2.bias"]).transpose(0, 1)
    h = tm
    for l in range(NL):
        gx = R.linear(h, p["lstm.weight_ih_l%d" % l], p["lstm.bias_ih_l%d" % l] + p["lstm.bias_hh_l%d" % l])
        h, _ = R.lstm_scan(gx, p["lstm.weight_hh_l%d" % l])
    ctx = LS.local_attention_taps(z, h, mask)
    hid = R.linear(ctx, p["decoder.0.weight"], p["decoder.0.bias"], act=1)
    want = R.linear(hid, p["decoder.2.weight"], p["decoder.2.bias"]) * mask.reshape(B, T, 1)
    got = LS.batch(p, x, mask)
    assert torch.equal(got, want)
    s = LS.stepped(p, x, mask)
    exact = LS.batch(p, x, mask, rounding=False)
    dist = ((got - exact).norm() / exact.norm()).item()
    print("lstm stream reference %s: stepped vs batch (rounded) %.3e, rounding on vs off rel-L2 %.3e"
          % (IDS[CASES.index(c)], (s - got).abs().max().item(), dist))
    assert (s - got).abs().max().item() <= 1e-12 and dist > 1e-4


def test_local_attention_taps_normalises_each_row_and_looks_back_only():
    B, T, L, H = 2, 9, 4, 5
    z = G.gen_normal("lstm_stream_cpu:z", (B, T, L), 3).double()
    h = G.gen_normal("lstm_stream_cpu:h", (T, B, H), 3).double()
    valid = torch.ones(B, T, dtype=torch.float64)
    ctx = LS.local_attention_taps(z, h, valid)
    a = torch.softmax(z, dim=2)
    want = sum(a[0, 6, i] * h[6 - i, 0] for i in range(L))
    assert (ctx[0, 6] - want).abs().max() <= 1e-14
    z2, h2 = z.clone(), h.clone()
    z2[:, 5:], h2[5:] = 7.0, -3.0                           # later steps changed: the prefix keeps its bits
    assert torch.equal(LS.local_attention_taps(z2, h2, valid)[:, :5], ctx[:, :5])


# ------------------------------------------------------------------------------------------------ 2. the plan checker
def test_lstm_step_plan_check_under_sanitizers(tmp_path):
    """tools/lstm_step_plan_check.cpp, built with -fsanitize=address,undefined, walks the limits and their refused neighbours and
    touches, on host buffers of the queried state sizes, what the preparation writes and what a step addresses"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "lstm_step_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "lstm_step_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ 3. surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def _models(cpu):
    import multimodal_transformer_amd as m
    MM = m.models
    return MM, [MM.MultiLSTM(12, embed_dim=8, h_dim=8, device=cpu), MM.MultiLSTMB1(12, embed_dim=8, h_dim=8, device=cpu),
                MM.MultiEDLSTM(12, embed_dim=8, h_dim=8, device=cpu), MM.MultiARLSTM(12, embed_dim=8, h_dim=8, device=cpu)]


def test_attend_over_taps_sets_the_flag_on_every_lstm_baseline():
    cpu = torch.device("cpu")
    MM, models = _models(cpu)
    wrap = MM.MultiCNNLSTM(["emotient"], {"emotient": 8}, device=cpu, window_embed_size={"emotient": 16}, lstm_cls=MM.MultiLSTM)
    for model in models + [wrap.LSTM]:
        assert model.over_taps is False                     # off by default
    for model in models:
        found = MM.attend_over_taps(model)
        assert list(found.values()) == [model] and model.over_taps is True
        MM.attend_over_taps(model, False)
        assert model.over_taps is False
    found = MM.attend_over_taps(wrap)
    assert found == {"LSTM": wrap.LSTM} and wrap.LSTM.over_taps is True
    assert MM.attend_over_taps(wrap, on=False) == {"LSTM": wrap.LSTM} and wrap.LSTM.over_taps is False
    assert _params(MM.attend_over_taps) == ["module", "on"]
    assert MM.attend_over_taps(torch.nn.Linear(2, 2)) == {}


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib
    F, MM, S = m.functional, m.models, m.streaming
    assert _params(F.local_attention) == ["z", "h", "valid", "over"]
    assert inspect.signature(F.local_attention).parameters["over"].default == "time"
    dims = ["in_dim", "embed_dim", "h_dim", "n_layers", "attn_len"]
    assert _params(F.lstm_stream_bytes) == ["B"] + dims
    assert _params(F.lstm_stream_state) == ["B"] + dims + ["device"]
    assert _params(F.lstm_stream_prepare) == ["embed_params", "attn_params", "lstm_params", "dec_params", "state", "B"] + dims
    assert _params(F.lstm_stream_step) == ["x_t", "mask_t", "state", "t"] + dims
    assert _params(F.lstm_stream_step_slots) == ["x_t", "mask_t", "state", "positions"] + dims + ["limit", "advance"]
    sig = inspect.signature(F.lstm_stream_step_slots).parameters
    assert sig["limit"].default is None and sig["advance"].default is True
    for cls in (MM.MultiLSTM, MM.MultiLSTMB1, MM.MultiCNNLSTM):
        assert _params(cls.slot_stream) == ["self", "batch", "limit"], cls.__name__
        assert inspect.signature(cls.slot_stream).parameters["limit"].default is None
        assert _params(cls.stream)[:2] == ["self", "batch"], cls.__name__
    assert issubclass(S.LSTMSlotStream, S._Slots) and issubclass(S.LSTMSlotStream, S.LSTMStream)
    assert S.LSTMSlotStream.slots is True and S.LSTMStream.slots is False
    for name in ("seat", "release", "reset", "full", "step", "refresh"):
        assert callable(getattr(S.LSTMSlotStream, name)), name
    for name in ("step", "reset", "refresh"):
        assert callable(getattr(S.LSTMStream, name)), name
    with pytest.raises(AttributeError, match=r"\.positions"):
        object.__new__(S.LSTMSlotStream).t
    lib = _lib.load()
    header = open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")).read()
    for name, ret, nargs in (("mmt_local_attn_forward_taps", "int", 10), ("mmt_local_attn_backward_taps", "int", 13),
                             ("mmt_lstm_stream_bytes", "size_t", 6), ("mmt_lstm_stream_prepare", "int", 10),
                             ("mmt_lstm_stream_step", "int", 13), ("mmt_lstm_stream_step_slots", "int", 15)):
        assert ("%s %s(" % (ret, name)) in header, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["mmt_local_attn_forward_taps"] == _lib.SIGNATURES["mmt_local_attn_forward"]       # the twins' signatures
    assert _lib.SIGNATURES["mmt_local_attn_backward_taps"] == _lib.SIGNATURES["mmt_local_attn_backward"]
    assert lib.mmt_abi_version() == 1


# ------------------------------------------------------------------------------------------------ 4. refusals without a device
def test_c_limits_and_their_refused_neighbours():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    size = lib.mmt_lstm_stream_bytes
    for args, limit in (((1, 1, 1, 1, 1, 1), None), ((1, 2048, 512, 512, 4, 16), None), ((33, 16, 8, 8, 2, 3), None),
                        ((2, 1556, 512, 256, 1, 5), None),
                        ((1, 2049, 8, 8, 1, 1), b"input width > 2048"), ((1, 8, 513, 8, 1, 1), b"embed_dim > 512"),
                        ((1, 8, 8, 513, 1, 1), b"h_dim > 512"), ((1, 8, 8, 8, 5, 1), b"n_layers > 4"), ((1, 8, 8, 8, 1, 17), b"attn_len > 16"),
                        ((0, 8, 8, 8, 1, 1), b"non-positive"), ((1, 0, 8, 8, 1, 1), b"non-positive"), ((1, 8, 0, 8, 1, 1), b"non-positive"),
                        ((1, 8, 8, 0, 1, 1), b"non-positive"), ((1, 8, 8, 8, 0, 1), b"non-positive"), ((1, 8, 8, 8, 1, 0), b"non-positive")):
        n = size(*args)
        if limit is None:
            assert n > 0 and n % 256 == 0, args
        else:
            assert n == 0 and limit in lib.mmt_last_error() and b"lstm stream" in lib.mmt_last_error(), (args, lib.mmt_last_error())
    # per sequence: two copies of (h, c) per layer and a ring of attn_len rows, each region rounded up to 256 bytes
    assert size(9, 16, 8, 32, 2, 4) - size(1, 16, 8, 32, 2, 4) == 8 * (2 * 2 * 2 * 32 + 4 * 32) * 4


def test_c_refusals_before_any_launch():
    """a state shorter than the size query gives MMT_EINVAL before any launch, as do null pointers and a negative position"""
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    fake, big = ctypes.c_void_p(4096), 1 << 40               # never dereferenced: each call below is refused first
    dims = (4, 12, 8, 8, 1, 3)
    step, slots, prep = lib.mmt_lstm_stream_step, lib.mmt_lstm_stream_step_slots, lib.mmt_lstm_stream_prepare
    need = lib.mmt_lstm_stream_bytes(*dims)
    assert slots(fake, None, fake, fake, big, None, 0, 1, *dims, None) == MMT_EINVAL                # the null pos
    assert b"pos" in lib.mmt_last_error()
    assert slots(None, None, None, None, 0, fake, 0, 1, *dims, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert slots(fake, None, fake, fake, need - 1, fake, 0, 1, *dims, None) == MMT_EINVAL          # a state one byte too small
    assert b"lstm stream: the state holds" in lib.mmt_last_error()
    assert slots(fake, None, fake, fake, big, fake, 0, 1, 4, 12, 8, 8, 5, 3, None) == MMT_EUNSUPPORTED
    assert b"n_layers > 4" in lib.mmt_last_error()
    assert slots(fake, None, fake, fake, big, fake, 0, 1, 0, 12, 8, 8, 1, 3, None) == MMT_EINVAL
    assert step(fake, None, fake, fake, big, -1, *dims, None) == MMT_EINVAL
    assert b"negative" in lib.mmt_last_error()
    assert step(None, None, fake, fake, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, None, fake, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, fake, None, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, fake, fake, 16, 0, *dims, None) == MMT_EINVAL
    assert b"state holds 16 bytes" in lib.mmt_last_error()
    assert step(fake, None, fake, fake, need - 1, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, fake, fake, big, 0, 4, 12, 8, 8, 1, 17, None) == MMT_EUNSUPPORTED
    table = (ctypes.c_void_p * 14)(*([4096] * 14))
    assert prep(table, None, big, *dims, None) == MMT_EINVAL
    assert prep(None, fake, big, *dims, None) == MMT_EINVAL
    assert prep((ctypes.c_void_p * 14)(*([4096] * 13 + [None])), fake, big, *dims, None) == MMT_EINVAL
    assert prep(table, fake, need - 1, *dims, None) == MMT_EINVAL
    assert prep(table, fake, big, 4, 12, 8, 513, 1, 3, None) == MMT_EUNSUPPORTED
    # the taps twins refuse as the entries they mirror
    assert lib.mmt_local_attn_forward_taps(None, fake, fake, fake, fake, 1, 1, 4, 1, None) == MMT_EINVAL
    assert lib.mmt_local_attn_forward_taps(fake, fake, fake, fake, fake, 1, 1, 4, 17, None) == MMT_EUNSUPPORTED
    assert lib.mmt_local_attn_backward_taps(fake, fake, fake, fake, fake, fake, None, 0, 1, 1, 4, 1, None) == MMT_EINVAL
    assert lib.mmt_local_attn_backward_taps(fake, fake, fake, fake, fake, fake, fake, 0, 2, 3, 4, 2, None) != 0   # a workspace too small


def test_functional_refusals():
    import multimodal_transformer_amd as m
    F = m.functional
    st = torch.zeros(4, dtype=torch.uint8)
    x = torch.zeros(2, 12)
    good = torch.zeros(2, dtype=torch.int32)
    dims = (12, 8, 8, 1, 3)
    with pytest.raises(ValueError, match='"time" or "taps"'):
        F.local_attention(torch.zeros(1, 2, 3), torch.zeros(2, 1, 4), torch.ones(1, 2), over="rows")
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.local_attention(torch.zeros(1, 2, 3), torch.zeros(2, 1, 4), torch.ones(1, 2), over="taps")
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [0, 0], None):
        with pytest.raises(ValueError, match="positions must be a contiguous int32"):
            F.lstm_stream_step_slots(x, None, st, bad, *dims)
    for op in (lambda v, mk: F.lstm_stream_step_slots(v, mk, st, good, *dims), lambda v, mk: F.lstm_stream_step(v, mk, st, 0, *dims)):
        with pytest.raises(NotImplementedError, match="autograd"):
            op(x.clone().requires_grad_(), None)
        with pytest.raises(ValueError, match="mask_t"):
            op(x, torch.ones(3))
        with pytest.raises(ValueError, match=r"float32 \(B, 12\)"):
            op(torch.zeros(2, 8), None)
        with pytest.raises(ValueError, match=r"float32 \(B, 12\)"):
            op(x.double(), None)
        with pytest.raises(RuntimeError, match="no CPU path"):
            op(x, None)
    with pytest.raises(ValueError, match="negative"):
        F.lstm_stream_step(x, None, st, -1, *dims)
    for args, limit in (((2, 2049, 8, 8, 1, 3), "input width > 2048"), ((2, 12, 513, 8, 1, 3), "embed_dim > 512"),
                        ((2, 12, 8, 513, 1, 3), "h_dim > 512"), ((2, 12, 8, 8, 5, 3), "n_layers > 4"), ((2, 12, 8, 8, 1, 17), "attn_len > 16"),
                        ((0, 12, 8, 8, 1, 3), "non-positive"), ((2, 12, 8, 8, 0, 3), "non-positive")):
        with pytest.raises(ValueError, match=limit):
            F.lstm_stream_bytes(*args)
    p = {k: v.float() for k, v in LS.params(*dims).items()}
    embed, attn = [p["embed.1.weight"], p["embed.1.bias"]], [p["attn.0.weight"], p["attn.0.bias"], p["attn.2.weight"], p["attn.2.bias"]]
    lstm = [[p["lstm.%s_l0" % n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]]
    dec = [p["decoder.0.weight"], p["decoder.0.bias"], p["decoder.2.weight"], p["decoder.2.bias"]]
    with pytest.raises(ValueError, match="shapes"):
        F.lstm_stream_prepare(embed, attn, lstm, dec, st, 2, 12, 8, 8, 2, 3)
    with pytest.raises(ValueError, match="shapes"):
        F.lstm_stream_prepare(embed, attn, lstm, dec[:2] + dec[:2], st, 2, *dims)
    with pytest.raises(NotImplementedError, match="autograd"):
        F.lstm_stream_prepare([embed[0].clone().requires_grad_(), embed[1]], attn, lstm, dec, st, 2, *dims)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.lstm_stream_prepare(embed, attn, lstm, dec, st, 2, *dims)


def test_model_refusals_on_cpu():
    """train mode and attend_over_taps not on are refused before any launch, naming the remedy; MultiEDLSTM and MultiARLSTM do not
    stream; the limits are named where the stream is opened"""
    cpu = torch.device("cpu")
    MM, (lstm, b1, ed, ar) = _models(cpu)
    wrap = MM.MultiCNNLSTM(["emotient"], {"emotient": 8}, device=cpu, window_embed_size={"emotient": 16}, lstm_cls=MM.MultiLSTM)
    for model in (lstm, b1, wrap):
        for open_ in (lambda: model.stream(2), lambda: model.slot_stream(2), lambda: model.slot_stream(2, 8)):
            with pytest.raises(ValueError, match=r"\.eval\(\)"):
                model.train()
                open_()
            with pytest.raises(ValueError, match=r"attend_over_taps\(model\)"):
                model.eval()
                open_()
        MM.attend_over_taps(model)
        with pytest.raises(RuntimeError, match="no CPU path"):  # every refusal passed: the first thing that needs a device
            model.stream(2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            model.slot_stream(2)
    with pytest.raises(ValueError, match="limit must be at least 1"):
        lstm.slot_stream(2, 0)
    with pytest.raises(ValueError, match="batch must be at least 1"):
        lstm.stream(0)
    for model in (ed, ar):
        MM.attend_over_taps(model)
        model.eval()
        for open_ in (lambda: model.stream(2), lambda: model.slot_stream(2)):
            with pytest.raises(NotImplementedError, match="state of its own"):
                open_()
    deep = MM.MultiLSTM(12, embed_dim=8, h_dim=8, n_layers=5, device=cpu).eval()
    MM.attend_over_taps(deep)
    with pytest.raises(ValueError, match="n_layers > 4"):
        deep.stream(2)
    wide = MM.MultiLSTM(12, embed_dim=8, h_dim=8, attn_len=17, device=cpu).eval()
    MM.attend_over_taps(wide)
    with pytest.raises(ValueError, match="attn_len > 16"):
        wide.slot_stream(2)
