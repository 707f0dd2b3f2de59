"""CPU: the reference of the one-window MFN gate step (tests/mfn_stream_ref.py) against the exact function (oracle.mfn_gate) and against
the batch composition of the existing bf16-faithful pieces, the surface of the feature (mmt_mfn_stream_*, functional.mfn_stream_*,
MFN.stream / MFNStream and the stream methods of MultiTransformer, MultiTransformerB3 and their wrappers, with their refusals) and the
C boundary's size query and refusals.  No GPU: the library is loaded, nothing is launched."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import conftest
import mfn_stream_ref as S
import oracle
import recipe as R
from gpu_harness import measures

MMT_EINVAL, MMT_EUNSUPPORTED = 1, 2
# (modalities, input widths, T, B)
CASES = [(["acoustic", "emotient"], [12, 16], 9, 3),
         (["linguistic", "acoustic", "image"], [40, 24, 32], 40, 3),
         (["linguistic", "emotient", "acoustic", "image"], [256, 16, 256, 256], 33, 2)]       # the reference widths
IDS = ["+".join(m[:3] for m in c[0]) for c in CASES]


def gate_params(mods, widths, seed=11, output_dim=1):
    """{name: fp64} of an MFN over these modalities, from the recipe"""
    import multimodal_transformer_amd as m
    gate = m.multiTransformer.MFN(mods, dict(zip(mods, widths)), output_dim, device=torch.device("cpu"))
    return {k: v.double() for k, v in R.gen_params(R.shapes_of(gate.state_dict()), seed).items()}


def case_inputs(c, seed=11):
    mods, widths, T, B = c
    x = {m: R.gen_normal("mfn_stream:%s:%d" % (m, T), (T, B, w), seed).double() for m, w in zip(mods, widths)}
    return gate_params(mods, widths, seed), x


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_reference_is_the_exact_function(c):
    """rounding=False: T stepped windows == oracle.mfn_gate to 1e-12 (measured 2e-16)"""
    p, x = case_inputs(c)
    got = S.mfn_gate(p, "", x, c[0], rounding=False)
    with torch.no_grad():
        want = oracle.mfn_gate(p, "", x, c[0])
    err = (got - want).abs().max().item()
    print("mfn stream ref exact %s: max abs %.3e" % (IDS[CASES.index(c)], err))
    assert got.shape == want.shape == (c[3], c[2], 1) and torch.isfinite(got).all() and err <= 1e-12


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_rounded_reference_is_the_batch_composition(c):
    """rounding=True: the stepped walk == linear -> lstm_scan -> shift, concatenate -> ... -> mfn_mem_scan -> linear x2 of bf16_ref to
    1e-12 (measured exactly 0 to 2e-16): the step has the batch path's rounding sites and no others, so the GPU step can be held to
    either.  The rounding moves the function by D = 4e-3 .. 7e-3 rel-L2 (printed), the ceiling of the GPU test's bound."""
    p, x = case_inputs(c)
    got = S.mfn_gate(p, "", x, c[0])
    want = S.batch_composition(p, "", x, c[0])
    exact = S.mfn_gate(p, "", x, c[0], rounding=False)
    err = (got - want).abs().max().item()
    D = measures(got.numpy(), exact.numpy())
    print("mfn stream ref vs batch composition %s: max abs %.3e; rounding on vs off rel-L2 %.3e per-row %.3e"
          % (IDS[CASES.index(c)], err, D[0], D[1]))
    assert torch.isfinite(got).all() and err <= 1e-12
    assert 1e-4 < D[0] < 5e-2                                   # the rounding is on, and is a perturbation
    plain = S.batch_composition(p, "", x, c[0], rounding=False)
    assert (plain - exact).abs().max().item() <= 1e-12


def test_reference_step_mask_and_reset():
    """the class walks windows in order, the mask multiplies the output row only (the state advances under a blanked window), and
    reset() starts a recording anew"""
    c = CASES[0]
    p, x = case_inputs(c)
    mods, B = c[0], c[3]
    mask = R.prefix_mask([9, 4, 1], 9).double()
    s = S.MFNStream(p, "", mods)
    first = [s.step({m: x[m][t] for m in mods}, mask[:, t].reshape(-1)) for t in range(5)]
    assert s.t == 5
    s.reset()
    assert s.t == 0 and s.h is None
    again = [s.step({m: x[m][t] for m in mods}, mask[:, t].reshape(-1)) for t in range(5)]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    free = S.mfn_gate(p, "", x, mods)[:, :5]
    got = torch.stack(first, 1)
    assert torch.equal(got, free * mask[:, :5]) and (got[1, 4:] == 0).all() and (got[2, 1:] == 0).all() and got[0].abs().min() > 0


# ------------------------------------------------------------------------------------------------ surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    from multimodal_transformer_amd import _lib
    F, MT, M = m.functional, m.multiTransformer, m.models
    assert _params(F.mfn_stream_bytes) == ["B", "in_dims", "hidden", "output_dim"]
    assert _params(F.mfn_stream_state) == ["B", "in_dims", "hidden", "output_dim", "device"]
    assert _params(F.mfn_stream_prepare) == ["lstm_params", "gate_params", "state", "B", "in_dims", "hidden", "output_dim"]
    assert _params(F.mfn_stream_step) == ["xs", "mask_t", "state", "t", "in_dims", "hidden", "output_dim"]
    assert _params(MT.MFN.stream) == ["self", "batch"]
    for name in ("step", "reset", "refresh"):
        assert callable(getattr(MT.MFNStream, name))
    assert _params(MT.MFNStream.step) == ["self", "inputs", "mask_t"]
    assert "refresh()" in MT.MFNStream.__doc__ and "EncoderStream" in MT.MFNStream.__doc__      # the biases are copies: said where it differs
    assert _params(MT.MultiTransformer.stream) == ["self", "batch", "capacity"]
    assert _params(M.MultiCNNTransformerMFT.stream_modalities) == ["self", "batch", "capacity"]
    assert _params(M.MultiCNNTransformerMFT.stream) == ["self", "batch", "capacity"]
    for cls in (MT.MultiTransformerB3, M.MultiCNNTransformerB3):
        assert _params(cls.stream) == ["self", "batch", "capacity"], cls.__name__
        assert inspect.signature(cls.stream).parameters["capacity"].default is None
    lib = _lib.load()
    for name in ("mmt_mfn_stream_bytes", "mmt_mfn_stream_prepare", "mmt_mfn_stream_step"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.mmt_abi_version() == 1


def test_model_stream_refusals_on_cpu():
    """every refusal names its remedy and comes before anything touches a device"""
    import multimodal_transformer_amd as m
    MT, M = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    mods, wes = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}
    gate = MT.MFN(mods, wes, 1, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        gate.train().stream(2)
    with pytest.raises(ValueError, match="HIP device"):
        gate.eval().stream(2)
    mft = MT.MultiTransformer(mods, wes, N=1, h=2, device=cpu, embed_dim={"acoustic": 32, "emotient": 16})
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        mft.train().stream(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):                  # the encoders' own refusal passes through
        mft.eval().stream(2, 8)
    MT.causal_attention(mft)
    with pytest.raises(ValueError, match="HIP device"):
        mft.stream(2, 8)
    with pytest.raises(ValueError, match="capacity"):
        mft.stream(2, None)
    b3 = MT.MultiTransformerB3(mods, wes, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        b3.train().stream(2)
    with pytest.raises(ValueError, match="HIP device"):                                  # no causal_attention needed: the device is what is missing
        b3.eval().stream(2)
    dims = {"acoustic": 12, "emotient": 8}
    wrap = M.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        wrap.train().stream_modalities(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
        wrap.eval().stream_modalities(2, 8)
    with pytest.raises(NotImplementedError, match="MFN"):                                # stream() itself stays as it was
        wrap.stream(2, 8)
    one = M.MultiCNNTransformerMFT(["emotient"], {"emotient": 8}, {"emotient": 16}, device=cpu).eval()
    with pytest.raises(ValueError, match=r"stream\(batch, capacity\)"):
        one.stream_modalities(2, 8)
    wb3 = M.MultiCNNTransformerB3(mods, dims, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        wb3.train().stream(2)
    with pytest.raises(ValueError, match="HIP device"):
        wb3.eval().stream(2)
    with pytest.raises(ValueError, match="capacity"):
        M.MultiCNNTransformerB3(["emotient"], {"emotient": 8}, device=cpu).eval().stream(2)


def test_functional_refuses_autograd_shapes_and_cpu_tensors():
    import multimodal_transformer_amd as m
    F = m.functional
    D, H = [12, 16], [48, 16]
    st = torch.zeros(4, dtype=torch.uint8)
    x = [torch.zeros(2, 12), torch.zeros(2, 16)]
    with pytest.raises(NotImplementedError, match="autograd"):
        F.mfn_stream_step([x[0].clone().requires_grad_(), x[1]], None, st, 0, D, H, 1)
    with pytest.raises(ValueError, match="inputs for 2 modalities"):
        F.mfn_stream_step(x[:1], None, st, 0, D, H, 1)
    with pytest.raises(ValueError, match=r"float32 \(B, 16\)"):
        F.mfn_stream_step([x[0], torch.zeros(2, 12)], None, st, 0, D, H, 1)
    with pytest.raises(ValueError, match="float32"):
        F.mfn_stream_step([x[0].double(), x[1]], None, st, 0, D, H, 1)
    with pytest.raises(ValueError, match="mask_t"):
        F.mfn_stream_step(x, torch.ones(3), st, 0, D, H, 1)
    with pytest.raises(ValueError, match="negative"):
        F.mfn_stream_step(x, None, st, -1, D, H, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.mfn_stream_step(x, None, st, 0, D, H, 1)
    with pytest.raises(ValueError, match="multiples of 4"):
        F.mfn_stream_bytes(2, D, [50, 16], 1)
    with pytest.raises(ValueError, match="hidden sizes > 256"):
        F.mfn_stream_bytes(2, D, [244, 16], 1)
    gate = m.multiTransformer.MFN(["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}, 1, device=torch.device("cpu"))
    cells = [(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh) for c in (gate.lstm[k] for k in gate.mods)]
    with pytest.raises(NotImplementedError, match="autograd"):
        F.mfn_stream_prepare(cells, gate._gate_params(), st, 2, D, H, 1)
    with torch.no_grad():
        with pytest.raises(ValueError, match="LSTM cells"):
            F.mfn_stream_prepare(cells[:1], gate._gate_params(), st, 2, D, H, 1)
        bad = gate._gate_params()
        bad[0] = bad[0][:64]                                                             # att1 hidden 64: not the kernel's
        with pytest.raises(ValueError, match="sizes are fixed"):
            F.mfn_stream_prepare(cells, bad, st, 2, D, H, 1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.mfn_stream_prepare(cells, gate._gate_params(), st, 2, D, H, 1)


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
def _lib():
    from multimodal_transformer_amd import _lib
    return _lib.load()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_size_query_and_refusals():
    lib = _lib()
    D, H = _ints(12, 16), _ints(48, 16)
    base = lib.mmt_mfn_stream_bytes(4, 2, D, H, 1)
    assert base > 0 and base % 256 == 0
    # the carried state is 2 copies x B x (2 sum H + 128) floats behind the parameters: 64 more sequences cost exactly that
    assert lib.mmt_mfn_stream_bytes(68, 2, D, H, 1) - base == 2 * 64 * (2 * 64 + 128) * 4
    assert lib.mmt_mfn_stream_bytes(4, 2, _ints(20, 16), H, 1) > base                    # and the weights grow with a width
    for args, word in (((4, 5, _ints(8, 8, 8, 8, 8), _ints(16, 16, 16, 16, 16), 1), b"4 modalities"),
                       ((4, 2, _ints(14, 16), H, 1), b"input widths must be multiples of 4"),
                       ((4, 2, _ints(516, 16), H, 1), b"input width > 512"),
                       ((4, 2, D, _ints(50, 16), 1), b"hidden sizes must be multiples of 4"),
                       ((4, 2, D, _ints(244, 16), 1), b"hidden sizes > 256"),
                       ((4, 2, D, H, 257), b"output_dim > 256"),
                       ((0, 2, D, H, 1), b"non-positive"), ((4, 0, D, H, 1), b"non-positive"), ((4, 2, D, H, 0), b"non-positive"),
                       ((4, 2, _ints(0, 16), H, 1), b"non-positive"), ((4, 2, None, H, 1), b"null")):
        assert lib.mmt_mfn_stream_bytes(*args) == 0, args
        assert word in lib.mmt_last_error(), (args, lib.mmt_last_error())
    assert lib.mmt_mfn_stream_bytes(1, 1, _ints(8), _ints(16), 1) > 0
    assert lib.mmt_mfn_stream_bytes(4096, 4, _ints(512, 512, 512, 512), _ints(64, 64, 64, 64), 256) > 0      # the far corner of the domain


def test_step_refusals_before_any_launch():
    lib = _lib()
    D, H = _ints(12, 16), _ints(48, 16)
    dims = (4, 2, D, H, 1)
    assert lib.mmt_mfn_stream_step(None, None, None, None, 0, 0, *dims, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_mfn_stream_prepare(None, None, None, 0, *dims, None) == MMT_EINVAL
    fake = ctypes.c_void_p(4096)                                          # never dereferenced: each call below is refused first
    xs, big = (ctypes.c_void_p * 2)(4096, 4096), 1 << 40
    assert lib.mmt_mfn_stream_step((ctypes.c_void_p * 2)(4096, None), None, fake, fake, big, 0, *dims, None) == MMT_EINVAL
    for t in (-1, -2147483648):
        assert lib.mmt_mfn_stream_step(xs, None, fake, fake, big, t, *dims, None) == MMT_EINVAL, t
        assert b"negative" in lib.mmt_last_error()
    assert lib.mmt_mfn_stream_step(xs, None, fake, fake, big, 0, 4, 2, D, _ints(50, 16), 1, None) == MMT_EUNSUPPORTED
    assert lib.mmt_mfn_stream_step(xs, None, fake, fake, big, 0, 0, 2, D, H, 1, None) == MMT_EINVAL
    assert lib.mmt_mfn_stream_step(xs, None, fake, fake, 16, 0, *dims, None) == 3          # MMT_EWORKSPACE: state too small
    lp, gp = (ctypes.c_void_p * 8)(*[4096] * 8), (ctypes.c_void_p * 20)(*[4096] * 20)
    assert lib.mmt_mfn_stream_prepare(lp, gp, fake, 16, *dims, None) == 3
    assert lib.mmt_mfn_stream_prepare(lp, (ctypes.c_void_p * 20)(*([4096] * 19 + [None])), fake, big, *dims, None) == MMT_EINVAL


# ------------------------------------------------------------------------------------------------ the host check of the plan
def test_mfn_step_plan_check_under_sanitizers(tmp_path):
    """tools/mfn_step_plan_check.cpp, built with -fsanitize=address,undefined, walks the limits and their refused neighbours and, on
    host buffers of the queried state sizes, the job table the preparation launches and what the step kernels address"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "mfn_step_plan_check")
    src = os.path.join(conftest.ROOT, "tools", "mfn_step_plan_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("this compiler has no sanitizer runtime: %s" % build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, (run.stdout[-2000:], run.stderr[-3000:])
