"""CPU: the slots streams without a GPU.  The slot reference (tests/slot_stream_ref.py) against the existing references, sequence by
sequence; the surface (mmt_*_stream_step_slots in the header, exported and bound; functional.*_stream_step_slots; the slot_stream
methods, with every existing stream() signature as it was); the refusals of the C boundary and of the Python layer, all before
anything touches a device; and the stand-alone host check of the slot decode (tools/slot_pos_check.cpp) under ASan / UBSan."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import conftest
import mfn_stream_ref as M
import recipe as R
import slot_stream_ref as SL
import stream_ref as S
from test_mfn_stream_cpu import gate_params
from test_stream_cpu import case_inputs

MMT_EINVAL, MMT_EUNSUPPORTED, MMT_EWORKSPACE = 1, 2, 3
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_timetable():
    """seat, release, re-seat and full, call by call; the positions are what the device holds before each call"""
    sched = [(0, 0, "seat", 0), (1, 1, "seat", 1), (3, 1, "release", None), (4, 1, "seat", 2), (2, 2, "seat", 3)]
    table, pos = SL.timetable(sched, 6, 3, limit=3)
    assert [r[0] for r in table] == [(0, 0), (0, 1), (0, 2), None, None, None]           # full after 3 windows: zero rows from then on
    assert [r[1] for r in table] == [None, (1, 0), (1, 1), None, (2, 0), (2, 1)]         # released at call 3, another recording from call 4
    assert [r[2] for r in table] == [None, None, (3, 0), (3, 1), (3, 2), None]
    assert [p[0] for p in pos] == [0, 1, 2, 3, 3, 3]                                     # a full slot keeps its position
    assert [p[1] for p in pos] == [-1, 0, 1, -1, 0, 1] and [p[2] for p in pos] == [-1, -1, 0, 1, 2, 3]
    assert SL.windows_used(table) == {0: 3, 1: 2, 2: 2, 3: 3}
    free, _ = SL.timetable(sched[:1], 5, 1)                                              # no limit: never full
    assert [r[0] for r in free] == [(0, w) for w in range(5)]


def test_the_encoder_slot_reference_is_the_stream_reference_per_sequence():
    """unrounded: sequences seated at different calls, one of them in a slot that another recording left, give the rows of
    stream_ref.encoder_stack on the whole batch, each at its own calls, to 1e-12; every other cell is an exact zero"""
    c = (40, 4, 2, 45, [45, 30, 1])
    p, x, mask = case_inputs(c)                                                          # x (3, 45, 40), mask (3, 45, 1)
    want = S.encoder_stack(p, "", x, mask, c[1], rounding=False)
    recs = {r: x[r] for r in range(3)}
    masks = {r: mask[r].reshape(-1) for r in range(3)}
    sched = [(0, 0, "seat", 0), (2, 1, "seat", 2), (5, 1, "release", None), (7, 1, "seat", 1)]
    n_calls = 45
    table, _ = SL.timetable(sched, n_calls, 2, limit=45)
    got = SL.encoder_slots(p, "", c[1], recs, masks, table, rounding=False)
    assert got.shape == (n_calls, 2, 40)
    worst = 0.0
    for call in range(n_calls):
        for slot in range(2):
            cell = table[call][slot]
            if cell is None:
                assert (got[call, slot] == 0).all()
            else:
                worst = max(worst, (got[call, slot] - want[cell[0], cell[1]]).abs().max().item())
    print("encoder slot reference vs stream_ref: max abs %.3e" % worst)
    assert worst <= 1e-12
    assert table[4][1] == (2, 2) and table[5][1] is None and table[7][1] == (1, 0) and table[44][1] == (1, 37)
    inputs = SL.call_inputs(table, recs, torch.full((40,), 7.0))
    assert torch.equal(inputs[7, 1], x[1, 0]) and (inputs[5, 1] == 7.0).all()


def test_the_gate_slot_reference_is_the_stream_reference_per_sequence():
    """the same for the MFN gate against mfn_stream_ref.mfn_gate, unrounded, to 1e-12"""
    mods, widths, T, B = ["acoustic", "emotient"], [12, 16], 9, 3
    p = gate_params(mods, widths)
    x = {m: R.gen_normal("slot_cpu:%s" % m, (T, B, w), 11).double() for m, w in zip(mods, widths)}
    mask = R.prefix_mask([9, 4, 1], T).double()
    want = M.mfn_gate(p, "", x, mods, mask, rounding=False)                             # (B, T, 1)
    recs = {r: {m: x[m][:, r] for m in mods} for r in range(B)}
    masks = {r: mask[r].reshape(-1) for r in range(B)}
    sched = [(0, 0, "seat", 0), (1, 1, "seat", 1), (3, 1, "release", None), (4, 1, "seat", 2)]
    table, _ = SL.timetable(sched, T, 2)
    got = SL.mfn_slots(p, "", mods, recs, masks, table, rounding=False)
    worst = 0.0
    for call in range(T):
        for slot in range(2):
            cell = table[call][slot]
            if cell is None:
                assert (got[call, slot] == 0).all()
            else:
                worst = max(worst, (got[call, slot] - want[cell[0], cell[1]]).abs().max().item())
    print("gate slot reference vs mfn_stream_ref: max abs %.3e" % worst)
    assert worst <= 1e-12 and got[0, 0].abs().min() > 0


# ------------------------------------------------------------------------------------------------ 2. surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib, graphs
    F, MT, MM = m.functional, m.multiTransformer, m.models
    assert _params(F.encoder_stream_step_slots) == ["x_t", "mask_t", "flat_params", "state", "positions", "h", "d_ff", "n_layers", "capacity",
                                                     "eps", "advance"]
    assert _params(F.mfn_stream_step_slots) == ["xs", "mask_t", "state", "positions", "in_dims", "hidden", "output_dim", "limit", "advance"]
    sig = inspect.signature(F.mfn_stream_step_slots).parameters
    assert sig["limit"].default is None and sig["advance"].default is True
    assert inspect.signature(F.encoder_stream_step_slots).parameters["advance"].default is True
    # the defaults stay: stream() of every class is what it was and returns the host-t objects; slots are asked for by name
    assert MT.EncoderStream.slots is False and MT.MFNStream.slots is False and MT._GateStream.slots is False
    assert _params(MT.Encoder.stream) == ["self", "batch", "capacity"] and _params(MT.MFN.stream) == ["self", "batch"]
    assert _params(MT.Encoder.slot_stream) == ["self", "batch", "capacity", "positions"]
    assert _params(MT.MFN.slot_stream) == ["self", "batch", "limit", "positions"]
    assert _params(MT.MultiTransformer.slot_stream) == ["self", "batch", "capacity"]
    for cls in (MT.MultiTransformerB3, MM.MultiCNNTransformerB3):
        assert _params(cls.slot_stream) == ["self", "batch", "capacity"] and inspect.signature(cls.slot_stream).parameters["capacity"].default is None
    assert _params(MM.MultiCNNTransformerMFT.slot_stream) == ["self", "batch", "capacity"]
    for cls in (MT.NLPTransformer, MT.UniTransformer, MT.UniFullTransformer, MM.MultiCNNTransformer, MM.MultiCNNTransformerB2):
        assert callable(cls.slot_stream), cls.__name__
    for cls in (MT.EncoderSlotStream, MT.MFNSlotStream, MT._GateSlotStream):
        assert cls.slots is True
        for name in ("seat", "release", "reset", "full", "step"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        assert isinstance(inspect.getattr_static(cls, "t"), property)
    assert issubclass(MT.EncoderSlotStream, MT.EncoderStream) and issubclass(MT.MFNSlotStream, MT.MFNStream)
    # the stream classes live in a module of their own; multiTransformer's names are those objects
    for name in ("EncoderStream", "_Slots", "EncoderSlotStream", "_SequenceStream", "_SequenceSlotStream", "MFNStream", "MFNSlotStream",
                 "_GateStream", "_GateSlotStream", "_modality_rows", "_slot_positions", "_INT_MAX", "_stream_model_checks", "_no_slot_stream"):
        assert getattr(MT, name) is getattr(m.streaming, name), name
    assert MT._MOD_STREAMS is F._MOD_STREAMS
    assert _params(graphs.capture_stream) == ["stream", "inputs", "mask"]
    for name in ("inputs", "mask", "output", "replay"):
        assert name in graphs.StreamGraph.__doc__ or hasattr(graphs.StreamGraph, name)
    lib = _lib.load()
    header = open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")).read()
    for name in ("mmt_encoder_stream_step_slots", "mmt_mfn_stream_step_slots"):
        assert ("int %s(" % name) in header, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mmt_encoder_stream_step_slots"][1]) == 16 and len(_lib.SIGNATURES["mmt_mfn_stream_step_slots"][1]) == 14
    assert lib.mmt_abi_version() == 1


def test_the_t_of_a_slots_stream_names_positions():
    import multimodal_transformer_amd as m
    MT = m.multiTransformer
    s = object.__new__(MT.EncoderSlotStream)                 # no device needed: the member is the class's
    with pytest.raises(AttributeError, match=r"\.positions"):
        s.t
    s.positions, s.capacity = torch.tensor([-1, 0, 3, 4, INT_MAX], dtype=torch.int32), 4
    assert s.full().tolist() == [False, False, False, True, True]
    s.seat([0, 3])
    assert s.positions.tolist() == [0, 0, 3, 0, INT_MAX]
    s.release(torch.tensor([1]))
    assert s.positions.tolist() == [0, -1, 3, 0, INT_MAX]
    s.release(4)
    s.capacity = None                                        # a gate without a limit is never full
    assert s.full().tolist() == [False] * 5
    _Slots = MT._Slots
    _Slots.reset(s)
    assert s.positions.tolist() == [0] * 5


# ------------------------------------------------------------------------------------------------ 3. C ABI without a GPU
def _lib():
    from multimodal_transformer_amd import _lib
    return _lib.load()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_c_refusals_before_any_launch():
    lib = _lib()
    fake, big = ctypes.c_void_p(4096), 1 << 40               # never dereferenced: each call below is refused first
    dims = (4, 50, 128, 8, 128, 2)
    enc = lib.mmt_encoder_stream_step_slots
    assert enc(fake, None, fake, fake, fake, big, None, 1, *dims, 1e-6, None) == MMT_EINVAL       # the null pos
    assert b"pos" in lib.mmt_last_error()
    assert enc(None, None, None, None, None, 0, fake, 1, *dims, 1e-6, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    # every refusal of the host-t entry passes through
    assert enc(fake, None, fake, fake, fake, big, fake, 1, 4, 4097, 128, 8, 128, 2, 1e-6, None) == MMT_EUNSUPPORTED
    assert b"capacity > 4096" in lib.mmt_last_error()
    assert enc(fake, None, fake, fake, fake, big, fake, 1, 0, 50, 128, 8, 128, 2, 1e-6, None) == MMT_EINVAL
    assert enc(fake, None, fake, fake, fake, big, fake, 1, 4, 50, 130, 8, 128, 2, 1e-6, None) == MMT_EUNSUPPORTED
    assert enc(fake, None, fake, fake, fake, 16, fake, 1, *dims, 1e-6, None) == MMT_EWORKSPACE
    D, H = _ints(12, 16), _ints(48, 16)
    gdims = (4, 2, D, H, 1)
    xs = (ctypes.c_void_p * 2)(4096, 4096)
    gate = lib.mmt_mfn_stream_step_slots
    assert gate(xs, None, fake, fake, big, None, 0, 1, *gdims, None) == MMT_EINVAL                # the null pos
    assert b"pos" in lib.mmt_last_error()
    assert gate(None, None, None, None, 0, fake, 0, 1, *gdims, None) == MMT_EINVAL
    assert gate((ctypes.c_void_p * 2)(4096, None), None, fake, fake, big, fake, 0, 1, *gdims, None) == MMT_EINVAL
    assert gate(xs, None, fake, fake, big, fake, 0, 1, 4, 2, D, _ints(50, 16), 1, None) == MMT_EUNSUPPORTED
    assert gate(xs, None, fake, fake, big, fake, 0, 1, 0, 2, D, H, 1, None) == MMT_EINVAL
    assert gate(xs, None, fake, fake, 16, fake, 0, 1, *gdims, None) == MMT_EWORKSPACE
    # and the host-t entries refuse what they refused
    assert lib.mmt_encoder_stream_step(fake, None, fake, fake, fake, big, 50, *dims, 1e-6, None) == MMT_EINVAL
    assert b"outside [0, capacity" in lib.mmt_last_error()
    assert lib.mmt_mfn_stream_step(xs, None, fake, fake, big, -1, *gdims, None) == MMT_EINVAL
    assert b"negative" in lib.mmt_last_error()


# ------------------------------------------------------------------------------------------------ 4. Python refusals on CPU-built models
def test_functional_refusals():
    import multimodal_transformer_amd as m
    F = m.functional
    st = torch.zeros(4, dtype=torch.uint8)
    x = torch.zeros(2, 32)
    flat = torch.zeros(8)
    good = torch.zeros(2, dtype=torch.int32)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                torch.zeros(4, dtype=torch.int32)[::2], [0, 0], None, torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="positions must be a contiguous int32"):
            F.encoder_stream_step_slots(x, None, flat, st, bad, 2, 64, 1, 8)
        with pytest.raises(ValueError, match="positions must be a contiguous int32"):
            F.mfn_stream_step_slots([torch.zeros(2, 12), torch.zeros(2, 16)], None, st, bad, [12, 16], [48, 16], 1)
    with pytest.raises(NotImplementedError, match="autograd"):
        F.encoder_stream_step_slots(x.clone().requires_grad_(), None, flat, st, good, 2, 64, 1, 8)
    with pytest.raises(ValueError, match="mask_t"):
        F.encoder_stream_step_slots(x, torch.ones(3), flat, st, good, 2, 64, 1, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):                               # no host-side check of the positions' values
        F.encoder_stream_step_slots(x, None, flat, st, torch.tensor([-5, 99], dtype=torch.int32), 2, 64, 1, 8)
    with pytest.raises(ValueError, match="inputs for 2 modalities"):
        F.mfn_stream_step_slots([torch.zeros(2, 12)], None, st, good, [12, 16], [48, 16], 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.mfn_stream_step_slots([torch.zeros(2, 12), torch.zeros(2, 16)], None, st, good, [12, 16], [48, 16], 1, limit=4, advance=False)


def test_model_refusals_on_cpu():
    """slots on the models whose stream keeps host-side state, and every refusal of stream() passing through slot_stream()"""
    import multimodal_transformer_amd as m
    MT, MM = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    for model in (MT.NLPTransformer(48, embed_dim=40, h=4, N=1, device=cpu), MT.UniTransformer(48, embed_dim=40, h=4, N=1, device=cpu),
                  MT.UniFullTransformer(48, embed_dim=40, h=4, N=1, device=cpu)):
        MT.causal_attention(model)
        with pytest.raises(NotImplementedError, match="host-side state"):
            model.eval().slot_stream(2, 8)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    for wrap in (MM.MultiCNNTransformer(mods, dims, fuse_embed_size=48, device=cpu), MM.MultiCNNTransformerB2(["emotient"], {"emotient": 8}, device=cpu),
                 MM.MultiCNNTransformerMFT(["emotient"], {"emotient": 8}, {"emotient": 16}, device=cpu),
                 MM.MultiCNNTransformerB3(["emotient"], {"emotient": 8}, device=cpu)):
        with pytest.raises(NotImplementedError, match="host-side state"):
            wrap.eval().slot_stream(2, 8)
    enc = MT.Encoder(MT.EncoderLayer(32, MT.MultiHeadedAttention(2, 32), MT.PositionwiseFeedForward(32, 64, 0.1), 0.1), 2)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        enc.train().slot_stream(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
        enc.eval().slot_stream(2, 8)
    MT.causal_attention(enc)
    with pytest.raises(ValueError, match="HIP device"):
        enc.slot_stream(2, 8)
    wes = {"acoustic": 12, "emotient": 16}
    gate = MT.MFN(mods, wes, 1, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        gate.train().slot_stream(2)
    with pytest.raises(ValueError, match="HIP device"):
        gate.eval().slot_stream(2)
    mft = MT.MultiTransformer(mods, wes, N=1, h=2, device=cpu, embed_dim={"acoustic": 32, "emotient": 16})
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        mft.train().slot_stream(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):                  # a non-causal MFT
        mft.eval().slot_stream(2, 8)
    MT.causal_attention(mft)
    with pytest.raises(ValueError, match="capacity"):
        mft.slot_stream(2, None)
    with pytest.raises(ValueError, match="HIP device"):
        mft.slot_stream(2, 8)
    b3 = MT.MultiTransformerB3(mods, wes, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        b3.train().slot_stream(2)
    with pytest.raises(ValueError, match="HIP device"):
        b3.eval().slot_stream(2)
    wrap = MM.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        wrap.train().slot_stream(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
        wrap.eval().slot_stream(2, 8)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        MM.MultiCNNTransformerB3(mods, dims, device=cpu).train().slot_stream(2)


def test_capture_stream_refuses_a_host_position():
    from multimodal_transformer_amd import graphs

    class HostT:                                             # what stream() returns: a position on the host, no slots
        slots = False
        t = 0

    with pytest.raises(ValueError, match=r"slot_stream\("):
        graphs.capture_stream(HostT(), torch.zeros(2, 8))
    with pytest.raises(ValueError, match=r"slot_stream\("):
        graphs.capture_stream(object(), {"a": torch.zeros(2, 8)}, torch.ones(2))


# ------------------------------------------------------------------------------------------------ 5. the host check of the decode
def test_slot_pos_check_under_sanitizers(tmp_path):
    """tools/slot_pos_check.cpp, built with -fsanitize=address,undefined, walks slot_decode over the edge values of an int and
    touches, on host buffers of the queried state sizes, what a kernel would address with a position the decode let through"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "slot_pos_check")
    src = os.path.join(conftest.ROOT, "tools", "slot_pos_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])
