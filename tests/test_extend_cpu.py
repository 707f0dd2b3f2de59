"""CPU: extend, a stream moved forward by C windows from any position.  The index rule under the sanitizers
(tools/extend_plan_check.cpp), the surface of the feature and the C boundary's refusals.  No GPU: the library is loaded, nothing is
launched."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

import conftest

MMT_EINVAL, MMT_EUNSUPPORTED = 1, 2
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ 1. the rule, on the host
def test_extend_plan_check_under_sanitizers(tmp_path):
    """tools/extend_plan_check.cpp, a stand-alone program built with -fsanitize=address,undefined (nothing is preloaded), walks the
    extend rule launch by launch on a host array of exactly the state's size: plain and ring forms, spans 1, 5, 16, 17 and 33 against
    the tile of 16, calls of 1 to 70 windows from t = 0 and from inside a recording with steps between them, ragged lengths, idle and
    full slots, slots that would pass the capacity, and pairs outside their ranges"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "extend_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "extend_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ 2. the surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    F, ST, M = m.functional, m.streaming, m.models
    assert _params(ST.encoder_stream_extend)[:9] == ["x", "mask", "flat_params", "state", "t", "h", "d_ff", "n_layers", "rows"]
    assert _params(ST.encoder_stream_extend_slots)[:10] == ["x", "mask", "flat_params", "state", "positions", "table", "h", "d_ff",
                                                            "n_layers", "rows"]
    for fn in (ST.encoder_stream_extend, ST.encoder_stream_extend_slots):
        assert inspect.signature(fn).parameters["ring"].default is False
    assert F.encoder_stream_extend is ST.encoder_stream_extend and F.encoder_stream_extend_slots is ST.encoder_stream_extend_slots
    for cls in (ST.EncoderStream, ST.EncoderRingStream, ST._SequenceStream):
        assert _params(cls.extend) == ["self", "x", "mask"], cls
    for cls in (ST.EncoderSlotStream, ST.EncoderRingSlotStream):
        assert _params(cls.extend) == ["self", "indices", "x", "lengths", "mask", "advance"], cls
        assert inspect.signature(cls.extend).parameters["advance"].default is True
    assert _params(M._FrontEndStream.extend) == ["self", "inputs", "mask"]
    assert ST.EXTEND_ROWS == 16


def test_the_streams_that_only_step_say_so():
    """NotImplementedError naming step, before anything is looked at"""
    import multimodal_transformer_amd as m
    ST = m.streaming
    for cls in (ST.MFNStream, ST.MFNSlotStream, ST._GateStream, ST._GateSlotStream, ST.LSTMStream, ST.LSTMSlotStream,
                ST.LSTMFeedbackStream, ST.LSTMFeedbackSlotStream, ST._SequenceSlotStream):
        with pytest.raises(NotImplementedError, match="step"):
            cls.extend(object.__new__(cls))


# ------------------------------------------------------------------------------------------------ 3. the C boundary
def test_the_c_boundary_refuses_before_any_launch():
    """the four new symbols are declared, exported and bound; every unsupported call fails with its limit named, no pointer dereferenced"""
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    names = ["mmt_encoder_stream_extend", "mmt_encoder_stream_extend_ring", "mmt_encoder_stream_extend_slots",
             "mmt_encoder_stream_extend_ring_slots"]
    with open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and "int %s(" % name in header
    fake = ctypes.c_void_p(4096)                                                 # never dereferenced: each call below is refused first
    odd = ctypes.c_void_p(4096 + 8)
    big = 1 << 40
    err = lambda: lib.mmt_last_error()                                           # noqa: E731
    need = lib.mmt_encoder_stream_bytes(3, 8, 40, 4, 128, 2)
    assert need > 0
    for ring, ext in ((0, lib.mmt_encoder_stream_extend), (1, lib.mmt_encoder_stream_extend_ring)):
        # (x, mask, params, y, state, state_bytes, t, C, B, capacity | span, d, h, f, N, eps, stream)
        dims = (3, 8, 40, 4, 128, 2)
        call = lambda x, p, y, st, nb, t, C, dims=dims: ext(x, None, p, y, st, nb, t, C, *dims, ctypes.c_float(1e-6), None)      # noqa: E731
        assert call(None, fake, fake, fake, big, 0, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, None, fake, fake, big, 0, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, None, fake, big, 0, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, fake, None, big, 0, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, fake, fake, big, 0, 0) == MMT_EINVAL and b"C = 0" in err()
        assert call(fake, fake, fake, fake, big, -1, 4) == MMT_EINVAL and b"t = -1" in err()
        assert call(fake, fake, fake, fake, need - 1, 0, 4) == MMT_EINVAL and b"mmt_encoder_stream_bytes" in err()
        assert call(fake, fake, fake, odd, need, 0, 4) == MMT_EINVAL and b"16-byte aligned" in err()
        if ring:
            assert call(fake, fake, fake, fake, big, INT_MAX - 4, 4) == MMT_EINVAL and b"INT_MAX" in err()
            assert call(fake, fake, fake, fake, big, 0, 4, (3, 0, 40, 4, 128, 2)) == MMT_EINVAL and b"span" in err()
        else:
            assert call(fake, fake, fake, fake, big, 5, 4) == MMT_EINVAL and b"capacity = 8" in err()
            assert call(fake, fake, fake, fake, big, 8, 1) == MMT_EINVAL and b"capacity = 8" in err()
        assert call(fake, fake, fake, fake, big, 0, 4, (3, 4097, 40, 4, 128, 2)) == MMT_EUNSUPPORTED and b"capacity > 4096" in err()
        assert call(fake, fake, fake, fake, big, 0, 4, (3, 8, 260, 4, 128, 2)) == MMT_EUNSUPPORTED and b"d_k" in err()
        assert call(fake, fake, fake, fake, big, 0, 4, (3, 8, 40, 4, 128, 17)) == MMT_EUNSUPPORTED and b"n_layers" in err()
        # the plan's LDS limit: the widest row with the widest feed-forward
        assert lib.mmt_encoder_stream_bytes(1, 8, 512, 8, 2048, 1) > 0
        assert call(fake, fake, fake, fake, big, 0, 4, (1, 8, 512, 8, 2048, 1)) == MMT_EUNSUPPORTED and b"160 KB" in err()
    for ext in (lib.mmt_encoder_stream_extend_slots, lib.mmt_encoder_stream_extend_ring_slots):
        # (x, mask, params, y, state, state_bytes, pos, dst, len, advance, C, k, B_state, capacity | span, d, h, f, N, eps, stream)
        dims = (2, 3, 8, 40, 4, 128, 2)
        call = lambda x, st, nb, pos, dst, ln, C, dims=dims: ext(x, None, fake, fake, st, nb, pos, dst, ln, 1, C, *dims,      # noqa: E731
                                                                  ctypes.c_float(1e-6), None)
        assert call(fake, fake, big, None, fake, fake, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, big, fake, None, fake, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, big, fake, fake, None, 4) == MMT_EINVAL and b"null" in err()
        assert call(None, fake, big, fake, fake, fake, 4) == MMT_EINVAL and b"null" in err()
        assert call(fake, fake, big, fake, fake, fake, 0) == MMT_EINVAL and b"C = 0" in err()
        assert call(fake, fake, big, fake, fake, fake, 4, (4, 3, 8, 40, 4, 128, 2)) == MMT_EINVAL and b"B_state = 3" in err()
        assert call(fake, fake, need - 1, fake, fake, fake, 4) == MMT_EINVAL and b"mmt_encoder_stream_bytes" in err()
        assert call(fake, odd, need, fake, fake, fake, 4) == MMT_EINVAL and b"16-byte aligned" in err()
        assert call(fake, fake, big, fake, fake, fake, 4, (1, 1, 8, 512, 8, 2048, 1)) == MMT_EUNSUPPORTED and b"160 KB" in err()
