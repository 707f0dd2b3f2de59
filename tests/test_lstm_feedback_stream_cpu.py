"""CPU: MultiEDLSTM and MultiARLSTM as free-running online predictors, without a GPU.  The reference
(tests/lstm_feedback_stream_ref.py): stepped against batch (bit for bit with the rounding on), batch against the fp64 restatements of
the two models (tests/lstm_fb_ref.py, tests/ar_ref.py) with the softmax moved to the taps, the conditions the GPU bounds lean on (the
reference rounds; the autoregressive recurrence contracts), that a row depends on the past alone, the surface (feedback_stream /
feedback_slot_stream, the C entries), every refusal before anything touches a device, and the stand-alone host check of the limits and
the state layout (tools/lstm_feedback_plan_check.cpp) under ASan / UBSan."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import ar_ref
import conftest
import lstm_fb_ref
import lstm_feedback_stream_ref as FR
import lstm_stream_ref as LS

ALL = [("ed", c) for c in FR.ED_CASES] + [("ar", c) for c in FR.AR_CASES]
ALL_IDS = FR.ED_IDS + FR.AR_IDS
_CACHE = {}


def _refs(kind, c):
    """the four references of a case, computed once: stepped / batch, rounding on / off"""
    key = (kind, c)
    if key not in _CACHE:
        p, x, mask = FR.ed_case(c) if kind == "ed" else FR.ar_case(c)
        step, batch = (FR.EdStep, FR.ed_batch) if kind == "ed" else (FR.ArStep, FR.ar_batch)
        B = c[5]
        _CACHE[key] = {"p": p, "x": x, "mask": mask,
                       "stepped": FR.stepped(lambda: step(p, B), x, mask), "batch": batch(p, x, mask),
                       "stepped_exact": FR.stepped(lambda: step(p, B, rounding=False), x, mask), "batch_exact": batch(p, x, mask, rounding=False)}
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("kind,c", ALL, ids=ALL_IDS)
def test_stepped_is_batch(kind, c):
    """rounding on: the stepped reference equals the batch composition of bf16_ref's pieces bit for bit (every affine map and cell of a
    step is the same call at T = 1); rounding off: to fp64 noise; a masked window is an exact zero"""
    r = _refs(kind, c)
    err = (r["stepped_exact"] - r["batch_exact"]).abs().max().item()
    print("feedback reference %s %s: stepped vs batch, exact %.3e" % (kind, c, err))
    assert r["stepped"].shape == r["batch"].shape == (c[5], c[6], 1)
    assert torch.equal(r["stepped"], r["batch"])
    assert err <= 1e-12 and r["batch_exact"].abs().max() > 0
    assert (r["stepped"][r["mask"] == 0] == 0).all()


@pytest.mark.parametrize("kind,c", ALL, ids=ALL_IDS)
def test_batch_is_the_restated_model_with_the_softmax_over_the_taps(kind, c, monkeypatch):
    """rounding off: against lstm_fb_ref.edlstm / ar_ref.arlstm (the fp64 restatements of the reference's models), with
    lstm_stream_ref.local_attention_taps in place of their softmax over time"""
    r = _refs(kind, c)
    B, T = c[5], c[6]
    m3 = r["mask"].reshape(B, T, 1)
    if kind == "ed":
        monkeypatch.setattr(lstm_fb_ref, "local_attention", LS.local_attention_taps)
        want = lstm_fb_ref.edlstm(r["p"], r["x"], m3, tgt_init=FR.TGT_INIT)
    else:
        monkeypatch.setattr(ar_ref, "local_attention", LS.local_attention_taps)
        want = ar_ref.arlstm(r["p"], r["x"], m3, L=c[3], target=None, tgt_init=FR.TGT_INIT)
    err = (r["batch_exact"] - want).abs().max().item()
    print("feedback reference %s %s: batch vs the restated model %.3e" % (kind, c, err))
    assert want.shape == r["batch_exact"].shape and err <= 1e-12 and want.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 2. conditions on the inputs
@pytest.mark.parametrize("kind,c", ALL, ids=ALL_IDS)
def test_the_reference_rounds(kind, c):
    """D, the distance between rounding on and off, is above 1e-4 in every case: the GPU bounds have something to stay under"""
    r = _refs(kind, c)
    D = ((r["stepped"] - r["stepped_exact"]).norm() / r["stepped_exact"].norm()).item()
    print("feedback reference %s %s: rounding on vs off rel-L2 %.3e" % (kind, c, D))
    assert D > 1e-4


@pytest.mark.parametrize("c", FR.AR_CASES, ids=FR.AR_IDS)
def test_the_autoregressive_recurrence_contracts(c):
    """max over (b, t) of sum_k |w[b,t,k]| <= 0.9 for every AR case used on the GPU: an error in a fed-back prediction (a tipped
    rounding) decays instead of growing"""
    r = _refs("ar", c)
    gain = FR.ar_weights(r["p"], r["x"], r["mask"]).abs().sum(dim=-1).max().item()
    print("feedback reference ar %s: max sum_k |w| %.3f" % (c, gain))
    assert gain <= 0.9


# ------------------------------------------------------------------------------------------------ 3. a row depends on the past alone
@pytest.mark.parametrize("kind,c", [("ed", FR.ED_CASES[1]), ("ar", FR.AR_CASES[1])], ids=["ed", "ar"])
def test_a_row_depends_only_on_the_past(kind, c):
    r = _refs(kind, c)
    p, x, mask, B, T = r["p"], r["x"], r["mask"], c[5], c[6]
    step = FR.EdStep if kind == "ed" else FR.ArStep
    cut = 4
    x2, m2 = x.clone(), mask.clone()
    x2[:, cut:] = 3.0                                       # later windows changed: the earlier rows keep their bits
    m2[:, cut:] = 1.0
    later = FR.stepped(lambda: step(p, B), x2, m2)
    assert torch.equal(later[:, :cut], r["stepped"][:, :cut]) and not torch.equal(later[:, cut:], r["stepped"][:, cut:])
    # the value fed back is the unmasked one: after a blanked window the row is an exact zero while what the step carries on is not,
    # and the next row is the one that value gives (a zero in its place gives another)
    blank = torch.ones(B, T, dtype=torch.float64)
    blank[:, 2] = 0.0
    rows = []
    for zeroed in (False, True):
        s = step(p, B)
        for t in range(3):
            y = s.step(x[:, t], blank[:, t])
        assert (y == 0).all()
        carried = s.q if kind == "ed" else s.ring[2 % (s.K + 1)]
        assert carried.abs().min() > 0
        if zeroed:
            carried.zero_()
        rows.append(s.step(x[:, 3], blank[:, 3]))
    assert torch.equal(rows[0], FR.stepped(lambda: step(p, B), x, blank)[:, 3]) and not torch.equal(rows[0], rows[1])


# ------------------------------------------------------------------------------------------------ 4. surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def _cpu_models(**kw):
    import multimodal_transformer_amd as m
    MM, cpu = m.models, torch.device("cpu")
    ed = MM.MultiEDLSTM(12, embed_dim=kw.get("E", 8), h_dim=kw.get("H", 8), n_layers=kw.get("ed_layers", 1), attn_len=kw.get("L", 3), device=cpu)
    ar = MM.MultiARLSTM(12, embed_dim=kw.get("E", 8), h_dim=kw.get("H", 8), n_layers=kw.get("ar_layers", 1), attn_len=kw.get("L", 3),
                        ar_order=kw.get("K", 2), device=cpu)
    for model in (ed, ar):
        MM.attend_over_taps(model)
        model.eval()
    return MM, ed, ar


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib
    F, MM, S = m.functional, m.models, m.streaming
    for cls in (MM.MultiEDLSTM, MM.MultiARLSTM, MM.MultiCNNLSTM):
        assert _params(cls.feedback_stream) == ["self", "batch", "tgt_init"], cls.__name__
        assert _params(cls.feedback_slot_stream) == ["self", "batch", "limit", "tgt_init"], cls.__name__
        sig = inspect.signature(cls.feedback_slot_stream).parameters
        assert sig["limit"].default is None and sig["tgt_init"].default == 0.0
        assert inspect.signature(cls.feedback_stream).parameters["tgt_init"].default == 0.0
    assert not hasattr(MM.MultiLSTM, "feedback_stream")
    assert issubclass(S.LSTMFeedbackStream, S.LSTMStream) and not issubclass(S.LSTMFeedbackStream, S._Slots)
    assert issubclass(S.LSTMFeedbackSlotStream, S.LSTMSlotStream) and issubclass(S.LSTMFeedbackSlotStream, S._Slots)
    assert S.LSTMFeedbackStream.slots is False and S.LSTMFeedbackSlotStream.slots is True and S.LSTMFeedbackStream.capacity is None
    for name in ("seat", "release", "reset", "full", "step", "refresh"):
        assert callable(getattr(S.LSTMFeedbackSlotStream, name)), name
    assert "target" not in _params(S.LSTMFeedbackStream.step) and _params(S.LSTMFeedbackSlotStream.step) == ["self", "x_t", "mask_t", "advance"]
    with pytest.raises(AttributeError, match=r"\.positions"):
        object.__new__(S.LSTMFeedbackSlotStream).t
    dims = ["in_dim", "embed_dim", "h_dim", "n_layers", "attn_len"]
    F = S                                                   # the functional layer of this family stands in streaming.py, beside encoder_ring_step
    assert _params(F.lstm_feedback_stream_bytes) == ["B", "tail", "ar_order"] + dims
    assert _params(F.lstm_feedback_stream_state) == ["B", "tail", "ar_order"] + dims + ["device"]
    assert _params(F.lstm_feedback_stream_prepare) == ["embed_params", "attn_params", "lstm_params", "dec_params", "tail_params", "state", "B",
                                                        "tail", "ar_order"] + dims
    assert _params(F.lstm_feedback_stream_step) == ["x_t", "mask_t", "state", "t", "p_init", "tail", "ar_order"] + dims
    assert _params(F.lstm_feedback_stream_step_slots) == ["x_t", "mask_t", "state", "positions", "p_init", "tail", "ar_order"] + dims + ["limit", "advance"]
    assert (F.LSTM_TAIL_FB, F.LSTM_TAIL_AR) == (1, 2)
    lib = _lib.load()
    header = open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")).read()
    for name, ret, nargs in (("mmt_lstm_feedback_stream_bytes", "size_t", 8), ("mmt_lstm_feedback_stream_prepare", "int", 12),
                             ("mmt_lstm_feedback_stream_step", "int", 16), ("mmt_lstm_feedback_stream_step_slots", "int", 18)):
        assert ("%s %s(" % (ret, name)) in header, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "models.py:268-308" in header and "models.py:354-400" in header


def test_stream_and_slot_stream_still_refuse_and_name_the_new_entry():
    MM, ed, ar = _cpu_models()
    for model in (ed, ar):
        for open_ in (lambda: model.stream(2), lambda: model.slot_stream(2), lambda: model.slot_stream(2, 8)):
            with pytest.raises(NotImplementedError, match="state of its own") as e:
                open_()
            assert "feedback_stream" in str(e.value)


def test_c_limits_and_the_state_size():
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    size, front = lib.mmt_lstm_feedback_stream_bytes, lib.mmt_lstm_stream_bytes
    for args, limit in (((1, 0, 1, 1, 1, 1, 1, 1), None), ((1, 0, 2, 2048, 512, 512, 1, 16), None), ((2, 16, 2, 2048, 512, 512, 4, 16), None),
                        ((2, 1, 33, 16, 8, 8, 2, 3), None),
                        ((1, 0, 2, 12, 8, 8, 2, 3), b"n_layers == 1"), ((2, 0, 2, 12, 8, 8, 1, 3), b"ar_order < 1"),
                        ((2, 17, 2, 12, 8, 8, 1, 3), b"ar_order > 16"), ((0, 1, 2, 12, 8, 8, 1, 3), b"tail"), ((3, 1, 2, 12, 8, 8, 1, 3), b"tail"),
                        ((1, 0, 2, 2049, 8, 8, 1, 3), b"input width > 2048"), ((2, 1, 2, 12, 513, 8, 1, 3), b"embed_dim > 512"),
                        ((1, 0, 2, 12, 8, 513, 1, 3), b"h_dim > 512"), ((2, 1, 2, 12, 8, 8, 5, 3), b"n_layers > 4"),
                        ((2, 1, 2, 12, 8, 8, 1, 17), b"attn_len > 16"), ((1, 0, 0, 12, 8, 8, 1, 3), b"non-positive")):
        n = size(*args)
        if limit is None:
            assert n > 0 and n % 256 == 0 and n > front(*args[2:]), args
        else:
            assert n == 0 and limit in lib.mmt_last_error(), (args, lib.mmt_last_error())
    # per sequence, behind the front's: two copies of (hd, cd, q) padded to 4 floats; a ring of K + 1 predictions
    assert size(1, 0, 65, 16, 8, 32, 1, 4) - size(1, 0, 1, 16, 8, 32, 1, 4) - (front(65, 16, 8, 32, 1, 4) - front(1, 16, 8, 32, 1, 4)) == 64 * 2 * 68 * 4
    assert size(2, 3, 65, 16, 8, 32, 2, 4) - size(2, 3, 1, 16, 8, 32, 2, 4) - (front(65, 16, 8, 32, 2, 4) - front(1, 16, 8, 32, 2, 4)) == 64 * 4 * 4


def test_functional_refusals():
    import multimodal_transformer_amd as m
    F = m.streaming
    st = torch.zeros(4, dtype=torch.uint8)
    x = torch.zeros(2, 12)
    good = torch.zeros(2, dtype=torch.int32)
    for tail, K in ((F.LSTM_TAIL_FB, 0), (F.LSTM_TAIL_AR, 2)):
        dims = (12, 8, 8, 1, 3)
        host = lambda v, mk, p=0.0: F.lstm_feedback_stream_step(v, mk, st, 0, p, tail, K, *dims)                     # noqa: E731
        slots = lambda v, mk, p=0.0: F.lstm_feedback_stream_step_slots(v, mk, st, good, p, tail, K, *dims)           # noqa: E731
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [0, 0], None):
            with pytest.raises(ValueError, match="positions must be a contiguous int32"):
                F.lstm_feedback_stream_step_slots(x, None, st, bad, 0.0, tail, K, *dims)
        for op in (host, slots):
            with pytest.raises(NotImplementedError, match="autograd"):
                op(x.clone().requires_grad_(), None)
            with pytest.raises(ValueError, match="mask_t"):
                op(x, torch.ones(3))
            with pytest.raises(ValueError, match=r"float32 \(B, 12\)"):
                op(torch.zeros(2, 8), None)
            with pytest.raises(ValueError, match=r"float32 \(B, 12\)"):
                op(x.double(), None)
            for p in (float("nan"), float("inf"), -float("inf")):
                with pytest.raises(ValueError, match="finite"):
                    op(x, None, p)
            with pytest.raises(RuntimeError, match="no CPU path"):
                op(x, None)
        with pytest.raises(ValueError, match="negative"):
            F.lstm_feedback_stream_step(x, None, st, -1, 0.0, tail, K, *dims)
    with pytest.raises(ValueError, match="ar_order > 16"):
        F.lstm_feedback_stream_bytes(2, F.LSTM_TAIL_AR, 17, 12, 8, 8, 1, 3)
    with pytest.raises(ValueError, match="n_layers == 1"):
        F.lstm_feedback_stream_bytes(2, F.LSTM_TAIL_FB, 0, 12, 8, 8, 2, 3)


def test_every_refusal_on_cpu_models_comes_before_the_device():
    """section 2 of the feature's refusals on CPU models; 'no CPU path', the first thing that needs a device, only when all others pass"""
    MM, ed, ar = _cpu_models()
    for model in (ed, ar):
        opens = (lambda **kw: model.feedback_stream(2, **kw), lambda **kw: model.feedback_slot_stream(2, **kw),
                 lambda **kw: model.feedback_slot_stream(2, 8, **kw))
        for open_ in opens:
            model.train()
            with pytest.raises(ValueError, match=r"\.eval\(\)"):
                open_()
            model.eval()
            MM.attend_over_taps(model, False)
            with pytest.raises(ValueError, match=r"attend_over_taps\(model\)"):
                open_()
            MM.attend_over_taps(model)
            for bad in (float("nan"), float("inf"), "0.5", None):
                with pytest.raises(ValueError, match="tgt_init"):
                    open_(tgt_init=bad)
            with pytest.raises(RuntimeError, match="no CPU path"):
                open_()
            with pytest.raises(RuntimeError, match="no CPU path"):
                open_(tgt_init=0.25)
        with pytest.raises(ValueError, match="batch must be at least 1"):
            model.feedback_stream(0)
        with pytest.raises(ValueError, match="limit must be at least 1"):
            model.feedback_slot_stream(2, 0)
    with pytest.raises(NotImplementedError, match="n_layers == 1"):
        _cpu_models(ed_layers=2)[1].feedback_stream(2)
    with pytest.raises(NotImplementedError, match="n_layers == 1"):
        _cpu_models(ed_layers=2)[1].feedback_slot_stream(2)
    for K, limit in ((0, "ar_order < 1"), (17, "ar_order > 16")):
        with pytest.raises(ValueError, match=limit):
            _cpu_models(K=K)[2].feedback_stream(2)
    with pytest.raises(ValueError, match="n_layers > 4"):
        _cpu_models(ar_layers=5)[2].feedback_slot_stream(2)
    for kw, limit in (({"E": 513}, "embed_dim > 512"), ({"H": 513}, "h_dim > 512"), ({"L": 17}, "attn_len > 16")):
        _, ed2, ar2 = _cpu_models(**kw)
        for model in (ed2, ar2):
            with pytest.raises(ValueError, match=limit):
                model.feedback_stream(2)
    cpu = torch.device("cpu")
    for cls in (MM.MultiEDLSTM, MM.MultiARLSTM):
        wide = cls(2049, embed_dim=8, h_dim=8, device=cpu).eval()
        MM.attend_over_taps(wide)
        with pytest.raises(ValueError, match="input width > 2048"):
            wide.feedback_stream(2)
    # the wrapper: the two classes pass through (their own refusals first), every other sequence model names stream / slot_stream
    plain = MM.MultiCNNLSTM(["emotient"], {"emotient": 8}, device=cpu, window_embed_size={"emotient": 16}, lstm_cls=MM.MultiLSTM).eval()
    for open_ in (lambda: plain.feedback_stream(2), lambda: plain.feedback_slot_stream(2, 4)):
        with pytest.raises(ValueError, match=r"slot_stream"):
            open_()
    for cls in (MM.MultiEDLSTM, MM.MultiARLSTM):
        wrap = MM.MultiCNNLSTM(["emotient"], {"emotient": 8}, device=cpu, window_embed_size={"emotient": 16}, lstm_cls=cls)
        wrap.LSTM = cls(16, embed_dim=8, h_dim=8, device=cpu)
        for open_ in (lambda: wrap.feedback_stream(2), lambda: wrap.feedback_slot_stream(2, 4, 0.25)):
            wrap.train()
            with pytest.raises(ValueError, match=r"\.eval\(\)"):
                open_()
            wrap.eval()
            with pytest.raises(ValueError, match=r"attend_over_taps\(model\)"):
                open_()
            MM.attend_over_taps(wrap)
            with pytest.raises(RuntimeError, match="no CPU path"):
                open_()
            MM.attend_over_taps(wrap, False)


# ------------------------------------------------------------------------------------------------ 5. the plan checker
def test_lstm_feedback_plan_check_under_sanitizers(tmp_path):
    """tools/lstm_feedback_plan_check.cpp, a stand-alone program built with -fsanitize=address,undefined, walks the limits and their
    refused neighbours and touches, on host buffers of the queried state sizes, what the preparation writes and what a step addresses"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "lstm_feedback_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "lstm_feedback_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])
