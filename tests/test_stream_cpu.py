"""CPU: the reference of the one-window encoder step (tests/stream_ref.py) against the exact function and against the batch path's
reference, the surface of the feature (mmt_encoder_stream_*, functional.encoder_stream_step, Encoder.stream and the models' stream
methods with their refusals) and the C boundary's size query and refusals.  No GPU: the library is loaded, nothing is launched."""
import ctypes
import inspect

import pytest
import torch

import bf16_ref as E
import causal_ref as C
import recipe as R
import stream_ref as S
from gpu_harness import measures

MMT_EINVAL, MMT_EUNSUPPORTED = 1, 2
# (d, h, N, T, lengths)
CASES = [(128, 8, 2, 70, [70, 33, 1]), (40, 4, 2, 45, [45, 30, 1]), (64, 2, 3, 130, [130, 86, 1])]
IDS = ["d%d_h%d_n%d_T%d" % c[:4] for c in CASES]


def case_inputs(c, seed=17):
    d, h, n, T, lengths = c
    p = {k: v.double() for k, v in R.gen_params(E.encoder_param_shapes(d, R.D_FF, n), seed).items()}
    x = R.gen_normal("stream_d%d_T%d:x" % (d, T), (len(lengths), T, d), seed).double()
    return p, x, R.prefix_mask(lengths, T).double()


_REFS = {}


def refs(c):
    """(stream rounded, batch rounded, batch exact) of a case, each (B, T, d) fp64, computed once"""
    if c[:4] not in _REFS:
        p, x, mask = case_inputs(c)
        with torch.no_grad():
            _REFS[c[:4]] = (S.encoder_stack(p, "", x, mask, c[1]), C.encoder_stack(p, "", x, mask, c[1]).detach(),
                            C.encoder_stack(p, "", x, mask, c[1], rounding=False).detach())
    return _REFS[c[:4]]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_reference_is_the_exact_function(c):
    """rounding=False: row t of the window-by-window walk == row t of the batch reference, blanked rows included, to 1e-12"""
    p, x, mask = case_inputs(c)
    got = S.encoder_stack(p, "", x, mask, c[1], rounding=False)
    err = (got - refs(c)[2]).abs().max().item()
    print("stream ref exact %s: max abs %.3e" % (c[:4], err))
    assert torch.isfinite(got).all() and err <= 1e-12


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_distance_between_the_two_roundings(c):
    """rounding=True: the stream reference (row maximum exact, fp32 row sum) differs from the batch reference (lazily moved tile
    maximum) by no more than the batch reference's roundings move the batch reference itself.  Both are printed: the first is the D
    that tests/test_gpu_stream.py adds to its bound against the batch path.
    Measured with these inputs (rel-L2 / per-row maximum): d 128 9.2e-4 / 2.2e-3 against 1.9e-3 / 3.2e-3; d 40 8.0e-4 / 2.7e-3 against
    2.0e-3 / 4.8e-3; d 64 9.4e-4 / 3.5e-3 against 2.3e-3 / 5.2e-3."""
    stream, batch, exact = refs(c)
    D = measures(stream.numpy(), batch.numpy())
    floor = measures(batch.numpy(), exact.numpy())
    print("stream vs batch reference %s: rel-L2 %.3e per-row %.3e; batch rounding on vs off: %.3e / %.3e" % (c[:4], D[0], D[1], floor[0], floor[1]))
    assert D[0] > 0                          # the two roundings are not the same function
    assert D[0] <= floor[0] and D[1] <= floor[1]


def test_reference_step_and_reset():
    """the class walks windows in order, a blanked window still appends its key, and reset() starts a recording anew"""
    c = CASES[1]
    p, x, mask = case_inputs(c)
    s = S.EncoderStream(p, "", c[1])
    first = [s.step(x[:, t], mask[:, t].reshape(-1)) for t in range(5)]
    assert s.t == 5 and all(len(k) == 5 for k in s.K)
    s.reset()
    assert s.t == 0 and all(len(k) == 0 for k in s.K)
    again = [s.step(x[:, t], mask[:, t].reshape(-1)) for t in range(5)]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert torch.equal(torch.stack(first, 1), refs(c)[0][:, :5])


# ------------------------------------------------------------------------------------------------ surface
def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_surface():
    import multimodal_transformer_amd as m
    F, MT, M = m.functional, m.multiTransformer, m.models
    assert _params(F.encoder_stream_step) == ["x_t", "mask_t", "flat_params", "state", "t", "h", "d_ff", "n_layers", "capacity", "eps"]
    assert inspect.signature(F.encoder_stream_step).parameters["eps"].default == 1e-6
    assert _params(MT.Encoder.stream) == ["self", "batch", "capacity"]
    for name in ("step", "reset", "refresh"):
        assert callable(getattr(MT.EncoderStream, name))
    assert _params(MT.EncoderStream.step) == ["self", "x_t", "mask_t"]
    for cls in (MT.UniFullTransformer, MT.UniTransformer, MT.NLPTransformer, M.MultiCNNTransformer, M.MultiCNNTransformerB2,
                M.MultiCNNTransformerMFT):
        assert _params(cls.stream) == ["self", "batch", "capacity"], cls.__name__
    from multimodal_transformer_amd import _lib
    lib = _lib.load()
    for name in ("mmt_encoder_stream_bytes", "mmt_encoder_stream_prepare", "mmt_encoder_stream_step"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.mmt_abi_version() == 1


def _cpu_encoder(causal=True, n=2):
    import multimodal_transformer_amd as m
    MT = m.multiTransformer
    enc = MT.Encoder(MT.EncoderLayer(32, MT.MultiHeadedAttention(2, 32), MT.PositionwiseFeedForward(32, 64, 0.1), 0.1), n).eval()
    MT.causal_attention(enc, causal)
    return MT, enc


def test_encoder_stream_refusals_on_cpu():
    """every refusal of Encoder.stream names its remedy and comes before anything touches a device"""
    MT, enc = _cpu_encoder()
    with pytest.raises(ValueError, match=r"HIP device"):
        enc.stream(2, 8)
    enc.train()
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        enc.stream(2, 8)
    enc.eval()
    MT.causal_attention(enc, False)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
        enc.stream(2, 8)
    enc.layers[0].self_attn.causal = True                                # the layers disagree: not the fused stack
    with pytest.raises(ValueError, match="standard composition"):
        enc.stream(2, 8)
    MT.causal_attention(enc, False)
    MT.mask_padded_keys(enc)
    with pytest.raises(ValueError, match="mask_keys"):
        enc.stream(2, 8)
    MT.mask_padded_keys(enc, False)
    MT.keep_attention(enc)
    with pytest.raises(ValueError, match="standard composition"):
        enc.stream(2, 8)


def test_model_stream_refusals_on_cpu():
    import multimodal_transformer_amd as m
    MT, M = m.multiTransformer, m.models
    cpu = torch.device("cpu")
    stacked = MT.NLPTransformer(24, embed_dim=32, h=2, N=1, n_layers=2, device=cpu).eval()
    MT.causal_attention(stacked)
    with pytest.raises(NotImplementedError, match="n_layers"):
        stacked.stream(2, 8)
    for model in (MT.NLPTransformer(24, embed_dim=32, h=2, N=1, device=cpu), MT.UniTransformer(24, embed_dim=32, h=2, N=1, device=cpu),
                  MT.UniFullTransformer(24, embed_dim=32, h=2, N=1, device=cpu)):
        with pytest.raises(ValueError, match=r"\.eval\(\)"):
            model.train().stream(2, 8)
        with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
            model.eval().stream(2, 8)
        MT.causal_attention(model)
        with pytest.raises(ValueError, match="HIP device"):
            model.stream(2, 8)
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 8}
    mft = M.MultiCNNTransformerMFT(mods, dims, {"acoustic": 16, "emotient": 16}, device=cpu).eval()
    with pytest.raises(NotImplementedError, match="MFN"):
        mft.stream(2, 8)
    sft = M.MultiCNNTransformer(mods, dims, fuse_embed_size=32, device=cpu)
    with pytest.raises(ValueError, match=r"\.eval\(\)"):
        sft.train().stream(2, 8)
    with pytest.raises(ValueError, match=r"causal_attention\(model\)"):
        sft.eval().stream(2, 8)


def test_functional_refuses_autograd_and_cpu_tensors():
    import multimodal_transformer_amd as m
    F = m.functional
    x = torch.zeros(2, 32, requires_grad=True)
    with pytest.raises(NotImplementedError, match="autograd"):
        F.encoder_stream_step(x, None, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 0, 2, 64, 1, 8)
    with pytest.raises(ValueError, match="capacity"):
        F.encoder_stream_step(x.detach(), None, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 8, 2, 64, 1, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.encoder_stream_step(x.detach(), None, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 0, 2, 64, 1, 8)


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
def _lib():
    from multimodal_transformer_amd import _lib
    return _lib.load()


def test_size_query_and_refusals():
    lib = _lib()
    base = lib.mmt_encoder_stream_bytes(4, 50, 128, 8, 128, 2)
    assert base > 0
    assert lib.mmt_encoder_stream_bytes(4, 51, 128, 8, 128, 2) > base                 # grows with capacity
    assert lib.mmt_encoder_stream_bytes(5, 50, 128, 8, 128, 2) > base                 # and with B
    # the cache is N x 2 x B x capacity x h x dkp bf16 behind the weights: one more position costs exactly that many rows
    assert lib.mmt_encoder_stream_bytes(4, 4096, 128, 8, 128, 2) - lib.mmt_encoder_stream_bytes(4, 2048, 128, 8, 128, 2) \
        == 2 * 2 * 4 * 2048 * 8 * 16 * 2
    for args, word in (((4, 50, 256, 2, 128, 2), b"d_k"), ((4, 4097, 128, 8, 128, 2), b"capacity"), ((4, 50, 130, 8, 128, 2), b"divisible"),
                       ((4, 50, 516, 129, 128, 2), b"512"), ((4, 50, 128, 8, 2052, 2), b"2048"), ((4, 50, 128, 8, 128, 17), b"n_layers"),
                       ((4, 50, 126, 2, 128, 2), b"multiples of 4"), ((4, 50, 512, 512, 128, 2), b"padded to 8"),
                       ((0, 50, 128, 8, 128, 2), b"non-positive"), ((4, 0, 128, 8, 128, 2), b"non-positive")):
        assert lib.mmt_encoder_stream_bytes(*args) == 0, args
        assert word in lib.mmt_last_error(), (args, lib.mmt_last_error())
    assert lib.mmt_encoder_stream_bytes(1, 1, 32, 2, 128, 1) > 0
    assert lib.mmt_encoder_stream_bytes(4, 4096, 512, 8, 2048, 16) > 0                # the far corner of the domain


def test_step_refusals_before_any_launch():
    lib = _lib()
    dims = (4, 50, 128, 8, 128, 2)
    assert lib.mmt_encoder_stream_step(None, None, None, None, None, 0, 0, *dims, 1e-6, None) == MMT_EINVAL
    assert b"null" in lib.mmt_last_error()
    assert lib.mmt_encoder_stream_prepare(None, None, 0, *dims, None) == MMT_EINVAL
    fake = ctypes.c_void_p(4096)                                          # never dereferenced: each call below is refused first
    big = 1 << 40
    for t in (50, -1, 4096):
        assert lib.mmt_encoder_stream_step(fake, None, fake, fake, fake, big, t, *dims, 1e-6, None) == MMT_EINVAL, t
        assert b"capacity" in lib.mmt_last_error()
    assert lib.mmt_encoder_stream_step(fake, None, fake, fake, fake, big, 0, 4, 50, 256, 2, 128, 2, 1e-6, None) == MMT_EUNSUPPORTED
    assert lib.mmt_encoder_stream_step(fake, None, fake, fake, fake, 16, 0, *dims, 1e-6, None) == 3          # MMT_EWORKSPACE: state too small
    assert lib.mmt_encoder_stream_prepare(fake, fake, 16, *dims, None) == 3
