"""CPU: the one-window decoder step without a GPU.  The step reference (tests/decoder_stream_ref.py) against the oracle and against the
batch composition of bf16_ref's pieces, unrounded and rounded: one function serves the step and the batch path.  The surface
(mmt_decoder_stream_* in the header, exported and bound; functional.decoder_stream_*; the device_stream methods, with slot_stream
still refusing); the refusals of the C boundary and of the Python layer, all before anything touches a device; and the stand-alone
host check of the limits and the state layout (tools/decoder_step_plan_check.cpp) under ASan / UBSan."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import conftest
import decoder_stream_ref as D
import recipe as R
import slot_stream_ref as SL
from oracle import models_ref

MMT_EINVAL, MMT_EUNSUPPORTED, MMT_EWORKSPACE = 1, 2, 3

# (d, h_dim, L, B, T)
CASES = [(12, 20, 1, 3, 5), (40, 32, 1, 2, 12), (40, 128, 1, 3, 6), (32, 16, 2, 2, 6), (32, 16, 3, 2, 8), (16, 8, 4, 2, 5), (16, 8, 0, 2, 3)]
IDS = ["d%d_h%d_L%d_B%d_T%d" % c for c in CASES]


def _case(c):
    d, hd, L, B, T = c
    p = D.params(d, hd, L, tag="decoder_stream_cpu")
    enc = R.gen_normal("decoder_stream_cpu:enc:%d:%d" % (d, T), (B, T, d), 7).double()
    mask = R.prefix_mask([T - (2 * b) % T for b in range(B)], T).double().reshape(B, T)
    return p, enc, mask


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("c", [c for c in CASES if c[2] == 1], ids=[i for i, c in zip(IDS, CASES) if c[2] == 1])
def test_the_step_reference_is_the_oracle(c):
    """unrounded, one layer: every row of the stepped reference is the row of oracle.models_ref.lstm_decoder_head, to 1e-12"""
    p, enc, mask = _case(c)
    want = models_ref.lstm_decoder_head(p, enc) * mask.unsqueeze(-1)
    got = D.stepped(p, "", 1, enc, mask, rounding=False)
    err = (got - want).abs().max().item()
    print("decoder step reference vs oracle %s: max abs %.3e" % (IDS[CASES.index(c)], err))
    assert got.shape == want.shape == (c[3], c[4], 1) and err <= 1e-12
    assert p["dec_h0"].abs().min() > 0 and p["dec_c0"].abs().min() > 0                   # the position-0 path is not hidden by zeros


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_step_reference_is_the_batch_composition(c):
    """the stepped reference against the batch composition of bf16_ref.linear / lstm_scan / lstm_stack_scan over all T: unrounded to
    1e-12; rounded exactly at L <= 1 (the same calls on the same rows) and to 1e-12 at L >= 2 (the restated loop).  Prints what the
    rounding itself moves each case by: the room the GPU bounds have to stay under."""
    p, enc, mask = _case(c)
    L = c[2]
    exact_s, exact_b = D.stepped(p, "", L, enc, mask, rounding=False), D.batch(p, "", L, enc, mask, rounding=False)
    assert (exact_s - exact_b).abs().max().item() <= 1e-12
    round_s, round_b = D.stepped(p, "", L, enc, mask), D.batch(p, "", L, enc, mask)
    diff = (round_s - round_b).abs().max().item()
    dist = ((round_s - exact_s).norm() / exact_s.norm()).item()
    print("decoder step reference %s: stepped vs batch (rounded) %.3e, rounding on vs off rel-L2 %.3e" % (IDS[CASES.index(c)], diff, dist))
    assert diff == 0.0 if L <= 1 else diff <= 1e-12
    assert dist > 1e-4                                                                   # the reference rounds
    assert (round_s[mask == 0] == 0).all()


def test_the_slot_reference_is_the_step_reference_per_sequence():
    """sequences seated at different calls, one in a slot another recording left, one filling its slot: the rows of the stepped
    reference of each recording alone, each at its own calls; every other cell an exact zero"""
    d, hd, L, T = 12, 20, 2, 6
    p = D.params(d, hd, L, tag="decoder_stream_cpu")
    recs = {r: R.gen_normal("decoder_stream_cpu:slots:%d" % r, (T, d), 7).double() for r in range(3)}
    sched = [(0, 0, "seat", 0), (1, 1, "seat", 1), (3, 1, "release", None), (4, 1, "seat", 2)]
    table, _ = SL.timetable(sched, 8, 2, limit=T)
    got = D.decoder_slots(p, "", L, recs, None, table, rounding=False)
    assert got.shape == (8, 2, 1)
    alone = {r: D.stepped(p, "", L, recs[r].unsqueeze(0), None, rounding=False)[0] for r in recs}
    for call in range(8):
        for slot in range(2):
            cell = table[call][slot]
            if cell is None:
                assert (got[call, slot] == 0).all()
            else:
                assert torch.equal(got[call, slot], alone[cell[0]][cell[1]])
    assert table[6][0] is None and table[5][0] == (0, 5) and table[4][1] == (2, 0)


# ------------------------------------------------------------------------------------------------ 2. surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib
    F, MT, MM = m.functional, m.multiTransformer, m.models
    assert _params(F.decoder_stream_bytes) == ["B", "d", "h_dim", "n_layers"]
    assert _params(F.decoder_stream_state) == ["B", "d", "h_dim", "n_layers", "device"]
    assert _params(F.decoder_stream_prepare) == ["lstm_params", "dec_h0", "dec_c0", "out_params", "state", "B", "d", "h_dim", "n_layers"]
    assert _params(F.decoder_stream_step) == ["e_t", "mask_t", "state", "t", "d", "h_dim", "n_layers"]
    assert _params(F.decoder_stream_step_slots) == ["e_t", "mask_t", "state", "positions", "d", "h_dim", "n_layers", "limit", "advance"]
    sig = inspect.signature(F.decoder_stream_step_slots).parameters
    assert sig["limit"].default is None and sig["advance"].default is True
    for cls in (MT.NLPTransformer, MT.UniTransformer, MT.UniFullTransformer, MM.MultiCNNTransformer, MM.MultiCNNTransformerB2,
                MM.MultiCNNTransformerMFT, MM.MultiCNNTransformerB3):
        assert _params(cls.device_stream) == ["self", "batch", "capacity"], cls.__name__
        assert _params(cls.slot_stream) == ["self", "batch", "capacity"], cls.__name__   # as it was
    assert inspect.signature(MM.MultiCNNTransformerB3.device_stream).parameters["capacity"].default is None
    assert inspect.signature(MM.MultiCNNTransformerMFT.device_stream).parameters["capacity"].default is inspect.Parameter.empty
    cls = MT._SequenceSlotStream
    assert issubclass(cls, MT._Slots) and cls.slots is True and not issubclass(cls, MT._SequenceStream)
    for name in ("seat", "release", "reset", "full", "step", "refresh"):
        assert callable(getattr(cls, name)), name
    assert isinstance(inspect.getattr_static(cls, "t"), property) and isinstance(inspect.getattr_static(cls, "capacity"), property)
    assert MT._SequenceStream.__init__ is not cls.__init__ and not hasattr(MT._SequenceStream, "slots")       # stream() is what it was
    lib = _lib.load()
    header = open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")).read()
    for name, ret, nargs in (("mmt_decoder_stream_bytes", "size_t", 4), ("mmt_decoder_stream_prepare", "int", 14),
                             ("mmt_decoder_stream_step", "int", 11), ("mmt_decoder_stream_step_slots", "int", 13)):
        assert ("%s %s(" % (ret, name)) in header, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # the embed of a device stream: the affine map with its operands prepared once
    assert _params(F.linear_prepare) == ["W", "b", "prepared"] and _params(F.linear_prepared) == ["x", "prepared", "N", "act", "rowscale"]
    for name, ret, nargs in (("mmt_linear_prepared_bytes", "size_t", 2), ("mmt_linear_prepare", "int", 7), ("mmt_linear_forward_prepared", "int", 10)):
        assert ("%s %s(" % (ret, name)) in header, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.mmt_abi_version() == 1


def test_the_t_of_a_device_stream_names_positions():
    import multimodal_transformer_amd as m
    s = object.__new__(m.multiTransformer._SequenceSlotStream)         # no device needed: the member is the class's
    with pytest.raises(AttributeError, match=r"\.positions"):
        s.t


# ------------------------------------------------------------------------------------------------ 3. C ABI without a GPU
def _lib():
    from multimodal_transformer_amd import _lib
    return _lib.load()


def test_c_limits_and_their_refused_neighbours():
    lib = _lib()
    size = lib.mmt_decoder_stream_bytes
    for args, limit in (((1, 4, 1, 0), None), ((1, 512, 512, 4), None), ((33, 16, 8, 1), None), ((1, 8, 4, 1), None),
                        ((1, 516, 128, 1), b"embed_dim > 512"), ((1, 42, 128, 1), b"multiple of 4"), ((1, 2, 128, 1), b"multiple of 4"),
                        ((1, 40, 513, 1), b"h_dim > 512"), ((1, 40, 128, 5), b"n_layers > 4"),
                        ((0, 40, 128, 1), b"non-positive"), ((1, 0, 128, 1), b"non-positive"), ((1, 40, 0, 1), b"non-positive"),
                        ((1, 40, 128, -1), b"non-positive")):
        n = size(*args)
        if limit is None:
            assert n > 0 and n % 256 == 0, args
        else:
            assert n == 0 and limit in lib.mmt_last_error() and b"decoder stream" in lib.mmt_last_error(), (args, lib.mmt_last_error())
    # the stacked scan's embed_dim <= 128 limit does not apply: the weights are read from memory per step
    assert size(2, 256, 128, 4) > size(2, 128, 128, 4) > 0
    # two copies of (h, c) per layer and sequence
    assert size(3, 40, 32, 2) - size(1, 40, 32, 2) == 2 * 2 * 2 * 2 * 40 * 4


def test_c_refusals_before_any_launch():
    lib = _lib()
    fake, big = ctypes.c_void_p(4096), 1 << 40               # never dereferenced: each call below is refused first
    dims = (4, 40, 32, 1)
    step, slots, prep = lib.mmt_decoder_stream_step, lib.mmt_decoder_stream_step_slots, lib.mmt_decoder_stream_prepare
    assert slots(fake, None, fake, fake, big, None, 0, 1, *dims, None) == MMT_EINVAL                # the null pos
    assert b"pos" in lib.mmt_last_error()
    assert slots(None, None, None, None, 0, fake, 0, 1, *dims, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert slots(fake, None, fake, fake, 16, fake, 0, 1, *dims, None) == MMT_EINVAL              # a state that is too small
    assert slots(fake, None, fake, fake, big, fake, 0, 1, 4, 40, 32, 5, None) == MMT_EUNSUPPORTED
    assert b"n_layers > 4" in lib.mmt_last_error()
    assert slots(fake, None, fake, fake, big, fake, 0, 1, 4, 516, 32, 1, None) == MMT_EUNSUPPORTED
    assert slots(fake, None, fake, fake, big, fake, 0, 1, 0, 40, 32, 1, None) == MMT_EINVAL
    assert step(fake, None, fake, fake, big, -1, *dims, None) == MMT_EINVAL
    assert b"negative" in lib.mmt_last_error()
    assert step(None, None, fake, fake, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, None, fake, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, fake, None, big, 0, *dims, None) == MMT_EINVAL
    assert step(fake, None, fake, fake, 16, 0, *dims, None) == MMT_EINVAL
    assert b"state holds 16 bytes" in lib.mmt_last_error()
    assert step(fake, None, fake, fake, big, 0, 4, 42, 32, 1, None) == MMT_EUNSUPPORTED
    lp = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    assert prep(lp, fake, fake, fake, fake, fake, fake, None, big, *dims, None) == MMT_EINVAL
    assert prep(None, fake, fake, fake, fake, fake, fake, fake, big, *dims, None) == MMT_EINVAL      # one layer needs its parameters
    assert prep(lp, None, fake, fake, fake, fake, fake, fake, big, *dims, None) == MMT_EINVAL
    assert prep((ctypes.c_void_p * 4)(4096, None, 4096, 4096), fake, fake, fake, fake, fake, fake, fake, big, *dims, None) == MMT_EINVAL
    assert prep(lp, fake, fake, None, fake, fake, fake, fake, big, *dims, None) == MMT_EINVAL
    assert prep(lp, fake, fake, fake, fake, fake, fake, fake, 16, *dims, None) == MMT_EINVAL
    assert prep(lp, fake, fake, fake, fake, fake, fake, fake, big, 4, 40, 32, 5, None) == MMT_EUNSUPPORTED
    # the prepared affine map
    nbytes = lib.mmt_linear_prepared_bytes(48, 40)
    assert nbytes == 64 * 64 * 2 + 256 and lib.mmt_linear_prepared_bytes(0, 40) == 0
    assert lib.mmt_linear_prepare(None, fake, fake, big, 48, 40, None) == MMT_EINVAL
    assert lib.mmt_linear_prepare(fake, fake, fake, 16, 48, 40, None) == MMT_EWORKSPACE
    assert lib.mmt_linear_prepare(fake, fake, fake, big, 46, 40, None) == MMT_EUNSUPPORTED
    assert lib.mmt_linear_forward_prepared(fake, None, big, None, fake, 2, 48, 40, 0, None) == MMT_EINVAL
    assert lib.mmt_linear_forward_prepared(fake, fake, 16, None, fake, 2, 48, 40, 0, None) == MMT_EWORKSPACE
    assert lib.mmt_linear_forward_prepared(fake, fake, big, None, fake, 0, 48, 40, 0, None) == MMT_EINVAL


# ------------------------------------------------------------------------------------------------ 4. Python refusals without a device
def test_functional_refusals():
    import multimodal_transformer_amd as m
    F = m.functional
    st = torch.zeros(4, dtype=torch.uint8)
    e = torch.zeros(2, 40)
    good = torch.zeros(2, dtype=torch.int32)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                torch.zeros(4, dtype=torch.int32)[::2], [0, 0], None, torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="positions must be a contiguous int32"):
            F.decoder_stream_step_slots(e, None, st, bad, 40, 32, 1)
    for op in (lambda x, mk: F.decoder_stream_step_slots(x, mk, st, good, 40, 32, 1), lambda x, mk: F.decoder_stream_step(x, mk, st, 0, 40, 32, 1)):
        with pytest.raises(NotImplementedError, match="autograd"):
            op(e.clone().requires_grad_(), None)
        with pytest.raises(ValueError, match="mask_t"):
            op(e, torch.ones(3))
        with pytest.raises(ValueError, match=r"float32 \(B, 40\)"):
            op(torch.zeros(2, 32), None)
        with pytest.raises(ValueError, match=r"float32 \(B, 40\)"):
            op(e.double(), None)
        with pytest.raises(ValueError, match=r"float32 \(B, 40\)"):
            op(e.reshape(2, 1, 40), None)
        with pytest.raises(RuntimeError, match="no CPU path"):
            op(e, None)
    with pytest.raises(ValueError, match="negative"):
        F.decoder_stream_step(e, None, st, -1, 40, 32, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):                               # no host-side check of the positions' values
        F.decoder_stream_step_slots(e, None, st, torch.tensor([-5, 99], dtype=torch.int32), 40, 32, 1, limit=4, advance=False)
    for args, limit in (((2, 516, 32, 1), "embed_dim > 512"), ((2, 42, 32, 1), "multiple of 4"), ((2, 40, 513, 1), "h_dim > 512"),
                        ((2, 40, 32, 5), "n_layers > 4"), ((0, 40, 32, 1), "non-positive")):
        with pytest.raises(ValueError, match=limit):
            F.decoder_stream_bytes(*args)
    # prepare: shapes, before any device is asked for
    p = {k: v.float() for k, v in D.params(40, 32, 1).items()}
    lstm = [[p["decoder.%s_l0" % n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]]
    out = [p["out.0.weight"], p["out.0.bias"], p["out.2.weight"], p["out.2.bias"]]
    with pytest.raises(ValueError, match="LSTM's parameters"):
        F.decoder_stream_prepare(lstm, p["dec_h0"], p["dec_c0"], out, st, 2, 40, 32, 2)
    with pytest.raises(ValueError, match="dec_h0"):
        F.decoder_stream_prepare(lstm, p["dec_h0"][:, :, :8], p["dec_c0"], out, st, 2, 40, 32, 1)
    with pytest.raises(ValueError, match="read-out"):
        F.decoder_stream_prepare(lstm, p["dec_h0"], p["dec_c0"], out[:2] + out[:2], st, 2, 40, 32, 1)
    with pytest.raises(NotImplementedError, match="autograd"):
        F.decoder_stream_prepare(lstm, p["dec_h0"].clone().requires_grad_(), p["dec_c0"], out, st, 2, 40, 32, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.decoder_stream_prepare(lstm, p["dec_h0"], p["dec_c0"], out, st, 2, 40, 32, 1)


def test_model_refusals_on_cpu():
    """device_stream refuses what stream() refuses, and a decoder deeper than the kernel's limit; slot_stream refuses as it did"""
    import multimodal_transformer_amd as m
    MT, MM = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    for model in (MT.NLPTransformer(48, embed_dim=40, h=4, N=1, device=cpu), MT.UniTransformer(48, embed_dim=40, h=4, N=1, device=cpu),
                  MT.UniFullTransformer(48, embed_dim=40, h=4, N=1, device=cpu)):
        with pytest.raises(ValueError, match=r"\.eval\(\)"):
            model.train().device_stream(2, 8)
        with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
            model.eval().device_stream(2, 8)
        MT.causal_attention(model)
        with pytest.raises(ValueError, match="HIP device"):
            model.device_stream(2, 8)
        with pytest.raises(NotImplementedError, match=r"host-side state.*device_stream\("):
            model.slot_stream(2, 8)
    deep = MT.NLPTransformer(48, embed_dim=40, h=4, N=1, n_layers=5, device=cpu).eval()
    MT.causal_attention(deep)
    with pytest.raises(ValueError, match="n_layers > 4"):
        deep.device_stream(2, 8)
    odd = MT.UniTransformer(48, embed_dim=42, h=2, N=1, device=cpu).eval()
    MT.causal_attention(odd)
    with pytest.raises(ValueError, match="multiple of 4"):
        odd.device_stream(2, 8)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    for wrap in (MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=cpu), MM.MultiCNNTransformerB2(["emotient"], {"emotient": 8}, device=cpu),
                 MM.MultiCNNTransformerMFT(["emotient"], {"emotient": 8}, {"emotient": 16}, device=cpu),
                 MM.MultiCNNTransformerB3(["emotient"], {"emotient": 8}, device=cpu)):
        with pytest.raises(ValueError, match=r"\.eval\(\)"):
            wrap.train().device_stream(2, 8)
        with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
            wrap.eval().device_stream(2, 8)
        with pytest.raises(NotImplementedError, match="host-side state"):
            wrap.slot_stream(2, 8)
    with pytest.raises(ValueError, match="needs a capacity"):
        MM.MultiCNNTransformerB3(["emotient"], {"emotient": 8}, device=cpu).eval().device_stream(2)
    with pytest.raises(NotImplementedError, match=r"slot_stream\("):
        MM.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=cpu).eval().device_stream(2, 8)
    with pytest.raises(NotImplementedError, match=r"slot_stream\("):
        MM.MultiCNNTransformerB3(mods, dims, device=cpu).eval().device_stream(2)


# ------------------------------------------------------------------------------------------------ 5. the host check of the plan
def test_decoder_step_plan_check_under_sanitizers(tmp_path):
    """tools/decoder_step_plan_check.cpp, built with -fsanitize=address,undefined, walks the limits and their refused neighbours and
    touches, on host buffers of the queried state sizes, what the kernels address"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "decoder_step_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "decoder_step_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])
