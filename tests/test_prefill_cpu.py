"""CPU: the prefill of a stream.  The index rule under the sanitizers (tools/prefill_plan_check.cpp), the reference of
a prefilled stream (tests/prefill_ref.py) against the exact function, the surface of the feature and the C boundary's refusals.
No GPU: the library is loaded, nothing is launched."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import band_ref as BD
import bf16_ref as E
import causal_ref as C
import conftest
import decoder_stream_ref as DS
import prefill_ref as PF
import recipe as R

MMT_EINVAL, MMT_EUNSUPPORTED, MMT_EWORKSPACE = 1, 2, 3
# (d, h, N): P = 7 of T = 12, lengths [7, 4, 1]
CASES = [(40, 4, 2), (64, 2, 3)]
P, T, LENGTHS = 7, 12, [7, 4, 1]
SPAN = 3


def case_inputs(d, h, n, seed=23):
    p = {k: v.double() for k, v in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), seed).items()}
    x = R.gen_normal("prefill_d%d:x" % d, (len(LENGTHS), T, d), seed).double()
    # every sequence goes on to T after its prefix, with a blanked window behind it to take the mask through the stepped part too
    mask = torch.ones(len(LENGTHS), T, 1, dtype=torch.float64)
    mask[1, 2] = 0
    mask[0, 9] = 0
    return p, x, mask


# ------------------------------------------------------------------------------------------------ 1. the rule, on the host
def test_prefill_plan_check_under_sanitizers(tmp_path):
    """tools/prefill_plan_check.cpp, a stand-alone program built with -fsanitize=address,undefined (nothing is preloaded), walks the
    prefill rule on host buffers of exactly the queried sizes: d_k in {8, 10, 16, 32, 40, 64}, P in {1, 31, 32, 33, capacity}, ragged
    lengths, rings with P <, =, > span, span 1 and P = 2 span + 3, a permuted partial dst, and pairs that must be skipped"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "prefill_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "prefill_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ 2. the reference
@pytest.mark.parametrize("span", [None, SPAN], ids=["plain", "span3"])
@pytest.mark.parametrize("c", CASES, ids=["d%d_h%d_n%d" % c for c in CASES])
def test_the_reference_is_the_exact_function(c, span):
    """rounding=False: a stream reference seeded with the batch reference's K and V of positions < len[b] gives, from t = len[b] on,
    the rows of causal_ref.encoder_stack (band_ref with the span) over all T, to 1e-12; the returned prefix rows are that function's"""
    d, h, n = c
    p, x, mask = case_inputs(d, h, n)
    with torch.no_grad():
        want = (C.encoder_stack(p, "", x, mask, h, rounding=False) if span is None
                else BD.encoder_stack(p, "", x, mask, h, span, rounding=False)).detach()
        head = (C.encoder_stack(p, "", x[:, :P], mask[:, :P], h, rounding=False) if span is None
                else BD.encoder_stack(p, "", x[:, :P], mask[:, :P], h, span, rounding=False)).detach()
    got = PF.encoder_rows(p, "", h, x, mask, LENGTHS, P, span, rounding=False)
    assert torch.isfinite(got).all()
    assert (got[:, :P] - head).abs().max().item() <= 1e-12
    worst = 0.0
    for b, n_b in enumerate(LENGTHS):
        worst = max(worst, (got[b, n_b:] - want[b, n_b:]).abs().max().item())
    print("prefill ref exact %s span %s: max abs %.3e" % (c, span, worst))
    assert worst <= 1e-12


def test_the_seed_is_what_a_stepped_reference_holds():
    """rounding=False: K and V the seeded reference holds for positions < len are those a fully stepped stream reference holds, to
    1e-12 (with rounding on they differ: the history's layers ran the batch path's attention), and t stands at len"""
    import stream_ref as S
    d, h, n = CASES[0]
    p, x, mask = case_inputs(d, h, n)
    _, streams = PF.encoder(p, "", h, x[:, :P], mask[:, :P], LENGTHS, rounding=False)
    for b, n_b in enumerate(LENGTHS):
        s = S.EncoderStream(p, "", h, rounding=False)
        for t in range(n_b):
            s.step(x[b:b + 1, t], mask[b:b + 1, t].reshape(-1))
        assert streams[b].t == n_b == s.t
        for i in range(n):
            assert len(streams[b].K[i]) == n_b == len(streams[b].V[i])
            assert (torch.cat(streams[b].K[i], 2) - torch.cat(s.K[i], 2)).abs().max().item() <= 1e-12
            assert (torch.cat(streams[b].V[i], 2) - torch.cat(s.V[i], 2)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("L", [0, 1])
def test_the_decoder_reference_is_the_stepped_one(L):
    """the decoder's composition (batch pieces up to len - 1, DecoderStep afterwards) against every window stepped: exact with
    rounding off (1e-12), and with rounding on as well, since no rounding site of the decoder depends on a tile"""
    d, hd = 12, 5
    p = DS.params(d, hd, L)
    enc = R.gen_normal("prefill_dec:e", (len(LENGTHS), T, d), 5).double()
    mask = torch.ones(len(LENGTHS), T, dtype=torch.float64)
    mask[1, 2] = 0
    for rounding in (False, True):
        got = PF.decoder(p, "", L, enc, mask, LENGTHS, P, rounding)
        want = DS.stepped(p, "", L, enc, mask, rounding)
        err = (got - want).abs().max().item()
        print("decoder prefill ref L=%d rounding=%s: max abs %.3e" % (L, rounding, err))
        assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. the surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    F, ST, M = m.functional, m.streaming, m.models
    assert _params(F.encoder_stream_prefill)[:8] == ["x", "mask", "flat_params", "state", "h", "d_ff", "n_layers", "rows"]
    assert _params(F.decoder_stream_prefill)[:8] == ["h_all", "c_all", "state", "B_state", "d", "h_dim", "n_layers", "P"]
    for cls in (ST.EncoderStream, ST.EncoderRingStream, ST._SequenceStream):
        assert _params(cls.prefill) == ["self", "x", "mask"], cls
    for cls in (ST.EncoderSlotStream, ST.EncoderRingSlotStream, ST._SequenceSlotStream):
        assert _params(cls.prefill)[:5] == ["self", "indices", "x", "lengths", "mask"], cls
    assert hasattr(M._FrontEndStream, "prefill")
    # what opens at window 0 only says so, before anything is looked at
    for cls in (ST.MFNStream, ST.MFNSlotStream, ST._GateStream, ST._GateSlotStream, ST.LSTMStream, ST.LSTMSlotStream,
                ST.LSTMFeedbackStream, ST.LSTMFeedbackSlotStream):
        with pytest.raises(NotImplementedError, match="window 0"):
            cls.prefill(object.__new__(cls))
    assert "_state" in _params(m.multiTransformer._DecoderMixin._decode)


def test_the_table_is_checked_on_the_host():
    import multimodal_transformer_amd as m
    chk = m.functional.check_prefill_table
    assert chk("op", [2, 0], [5, 1], 5, 3, 8) == ([2, 0], [5, 1])
    assert chk("op", (1,), (9,), 9, 2, None) == ([1], [9])                      # a ring: no capacity
    for bad, what in (((([0, 0], [1, 1], 4, 3, 8)), "distinct"), ((([3], [1], 4, 3, 8)), "distinct"), ((([-1], [1], 4, 3, 8)), "distinct"),
                      ((([0], [0], 4, 3, 8)), "lengths"), ((([0], [5], 4, 3, 8)), "lengths"), ((([0], [7], 9, 3, 6)), "capacity"),
                      ((([0, 1], [1], 4, 3, 8)), "one length"), ((([], [], 4, 3, 8)), "1 <= k"), ((([0, 1, 2, 0], [1] * 4, 4, 3, 8)), "1 <= k")):
        with pytest.raises(ValueError, match=what):
            chk("op", *bad)
    with pytest.raises(ValueError, match="host ints"):
        chk("op", 3, [1], 4, 3, 8)


def test_the_c_boundary_refuses_before_any_launch():
    """the two new symbols are exported and bound; every unsupported call fails with its limit named, no pointer dereferenced"""
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    assert "mmt_encoder_stream_prefill" in _lib.SIGNATURES and "mmt_decoder_stream_prefill" in _lib.SIGNATURES
    with open(os.path.join(conftest.ROOT, "include", "mmt_hip.h")) as f:
        header = f.read()
    assert "int mmt_encoder_stream_prefill(" in header and "int mmt_decoder_stream_prefill(" in header
    fake = ctypes.c_void_p(4096)                                                 # never dereferenced: each call below is refused first
    odd = ctypes.c_void_p(4096 + 8)
    big = 1 << 40
    enc = lib.mmt_encoder_stream_prefill
    # (B_src, P, B_state, rows, ring, d, h, f, N)
    ok = (2, 5, 3, 8, 0, 40, 4, 128, 2)
    err = lambda: lib.mmt_last_error()                                           # noqa: E731
    assert enc(None, big, fake, big, None, None, None, *ok, None) == MMT_EINVAL and b"null" in err()
    assert enc(fake, big, None, big, None, None, None, *ok, None) == MMT_EINVAL and b"null" in err()
    assert enc(fake, big, fake, big, fake, None, None, *ok, None) == MMT_EINVAL and b"dst and len" in err()
    assert enc(fake, big, fake, big, None, None, None, 4, 5, 3, 8, 0, 40, 4, 128, 2, None) == MMT_EINVAL and b"B_src = 4" in err()
    assert enc(fake, big, fake, big, None, None, None, 2, 9, 3, 8, 0, 40, 4, 128, 2, None) == MMT_EINVAL and b"capacity = 8" in err()
    assert enc(fake, big, fake, big, None, None, None, 2, 0, 3, 8, 0, 40, 4, 128, 2, None) == MMT_EINVAL
    assert enc(fake, big, fake, big, None, None, None, 2, 9, 3, 0, 1, 40, 4, 128, 2, None) == MMT_EINVAL and b"span" in err()
    assert enc(fake, big, fake, big, None, None, None, 2, 5, 3, 4097, 0, 40, 4, 128, 2, None) == MMT_EUNSUPPORTED and b"capacity > 4096" in err()
    assert enc(fake, big, fake, big, None, None, None, 2, 5, 3, 8, 0, 260, 4, 128, 2, None) == MMT_EUNSUPPORTED and b"d_k" in err()
    need_ws = lib.mmt_encoder_workspace_bytes_eval(2, 5, 40, 4, 128, 2)
    need_st = lib.mmt_encoder_stream_bytes(3, 8, 40, 4, 128, 2)
    assert need_ws > 0 and need_st > 0
    assert enc(fake, need_ws - 1, fake, big, None, None, None, *ok, None) == MMT_EWORKSPACE
    assert enc(fake, need_ws, fake, need_st - 1, None, None, None, *ok, None) == MMT_EINVAL and b"mmt_encoder_stream_bytes" in err()
    assert enc(fake, need_ws, odd, need_st, None, None, None, *ok, None) == MMT_EINVAL and b"16-byte aligned" in err()
    assert enc(odd, need_ws, fake, need_st, None, None, None, *ok, None) == MMT_EINVAL and b"16-byte aligned" in err()
    # a ring takes P > span
    assert enc(fake, lib.mmt_encoder_workspace_bytes_eval(2, 9, 40, 4, 128, 2) - 1, fake, big, None, None, None,
               2, 9, 3, 4, 1, 40, 4, 128, 2, None) == MMT_EWORKSPACE
    dec = lib.mmt_decoder_stream_prefill
    # (B_src, P, B_state, limit, d, h_dim, n_layers)
    okd = (2, 5, 3, 8, 40, 16, 1)
    assert dec(fake, fake, None, big, None, None, None, *okd, None) == MMT_EINVAL and b"null" in err()
    assert dec(None, fake, fake, big, None, None, None, *okd, None) == MMT_EINVAL and b"null" in err()
    assert dec(fake, fake, fake, big, None, fake, None, *okd, None) == MMT_EINVAL and b"dst and len" in err()
    assert dec(fake, fake, fake, big, None, None, None, 4, 5, 3, 8, 40, 16, 1, None) == MMT_EINVAL and b"B_src = 4" in err()
    assert dec(fake, fake, fake, big, None, None, None, 2, 9, 3, 8, 40, 16, 1, None) == MMT_EINVAL and b"limit = 8" in err()
    assert dec(fake, fake, fake, big, None, None, None, 2, 5, 3, 8, 40, 16, 2, None) == MMT_EUNSUPPORTED and b"top layer" in err()
    assert dec(fake, fake, fake, big, None, None, None, 2, 5, 3, 8, 40, 16, 5, None) == MMT_EUNSUPPORTED and b"n_layers > 4" in err()
    assert dec(None, None, fake, big, None, None, None, 2, 5, 3, 8, 40, 16, 0, None) == MMT_EINVAL and b"nothing to do" in err()
    need = lib.mmt_decoder_stream_bytes(3, 40, 16, 1)
    assert dec(fake, fake, fake, need - 1, None, None, None, *okd, None) == MMT_EINVAL and b"mmt_decoder_stream_bytes" in err()
    assert dec(fake, fake, odd, need, None, None, None, *okd, None) == MMT_EINVAL and b"16-byte aligned" in err()
