"""CPU: the layout builders and the comparator of tests/layout_variants.py do what they claim, the table of tests/test_gpu_layouts.py has
a row for every op of functional.py, and the host checks that refuse a layout raise before any launch."""
import inspect

import pytest
import torch

import layout_variants as LV
import test_gpu_layouts as G

SHAPES = [(5, 6), (2, 5, 1), (2, 5, 3), (3, 2, 64), (7,), (1, 1, 20), (4, 1)]


def _src(shape, dtype=torch.float32):
    return torch.arange(1, 1 + int(torch.Size(shape).numel()), dtype=torch.float32).reshape(shape).to(dtype)


def _back(v, t):
    return torch.equal(v.contiguous().float(), t.float()) and tuple(v.shape) == tuple(t.shape)


@pytest.mark.parametrize("shape", SHAPES + [(), (1,)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_offset_is_contiguous_four_bytes_past_a_boundary(shape, dtype):
    t = _src(shape, dtype)
    v = LV.offset(t)
    assert v.is_contiguous() and v.dtype == dtype and v.data_ptr() % 16 == 4 and _back(v, t)
    assert v.untyped_storage().nbytes() > t.numel() * t.element_size(), "a view into a larger buffer"


def test_offset_refuses_an_element_that_cannot_sit_there():
    with pytest.raises(ValueError):
        LV.offset(torch.zeros(3, dtype=torch.float64))


@pytest.mark.parametrize("shape", SHAPES)
def test_strided_is_not_contiguous_and_stays_inside_its_allocation(shape):
    t = _src(shape)
    v = LV.strided(t)
    assert not v.is_contiguous() and v.dtype == t.dtype and v.storage_offset() > 0 and _back(v, t)
    assert v.storage_offset() + v.numel() <= v.untyped_storage().nbytes() // 4, "numel() floats from its base lie in its own allocation"
    if t.dim() >= 2 and t.numel() // t.shape[-1] > 1:
        assert v.stride(-1) == 1 and v.stride(-2) == 2 * t.shape[-1], "a column slice of a buffer twice as wide"
    else:
        assert v.stride(-1) == 2, "a step-2 slice"
    flat = torch.as_strided(v, (v.numel(),), (1,), v.storage_offset())
    assert not torch.equal(flat.reshape(shape), t) or t.numel() == 1, "read without its strides it must not look right"


@pytest.mark.parametrize("shape", [s for s in SHAPES if len(s) >= 2 and sum(n > 1 for n in s) >= 2])
def test_transposed_is_a_permuted_view_of_a_transposed_allocation(shape):
    t = _src(shape)
    v = LV.transposed(t)
    assert not v.is_contiguous() and v.dtype == t.dtype and v.storage_offset() > 0 and _back(v, t)
    assert v.permute(*reversed(range(v.dim()))).is_contiguous()
    assert v.storage_offset() + v.numel() <= v.untyped_storage().nbytes() // 4


def test_builders_refuse_what_a_shape_cannot_give():
    for fn, t in ((LV.strided, torch.zeros(1)), (LV.strided, torch.zeros(())), (LV.transposed, torch.zeros(7)), (LV.transposed, torch.zeros(1, 1, 20))):
        with pytest.raises(ValueError):
            fn(t)
        assert LV.build(fn.__name__, t).is_contiguous() and LV.build(fn.__name__, t).data_ptr() % 16 == 0      # the table's fall-back: a plain clone


def test_type_builders():
    t = _src((2, 5, 3))
    v = LV.f64(t)
    assert v.dtype == torch.float64 and v.is_contiguous() and _back(v, t)
    m = torch.tensor([[1.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    b, i = LV.as_bool(m), LV.as_int64(m)
    assert b.dtype == torch.bool and i.dtype == torch.int64 and _back(b, m) and _back(i, m)
    with pytest.raises(AssertionError):
        LV.as_bool(torch.tensor([0.5]))


def test_expanded_gradient_has_stride_zero_and_a_materialised_twin():
    row = _src((1, 3, 4))
    e = LV.expanded(row, (5, 3, 4))
    assert e.stride(0) == 0 and not e.is_contiguous() and tuple(e.shape) == (5, 3, 4)
    assert torch.equal(e.contiguous(), row.repeat(5, 1, 1))
    with pytest.raises(ValueError):
        LV.expanded(_src((2, 3)), (5, 3))
    for kind, fn in LV.GRAD_BUILDERS.items():
        g = fn(_src((5, 3, 4)))
        assert _back(g, _src((5, 3, 4))) and (g.data_ptr() % 16 == 4 if kind == "offset" else not g.is_contiguous())


# ---- the comparator catches an op that reads its input as if it were plain
def _op(x):
    return x.float() * 2.0 + 1.0


def _op_ignores_strides(x):
    """reads numel() elements from the view's base, as a kernel handed data_ptr() of a tensor nobody made contiguous"""
    c = torch.empty(x.shape).stride()
    return _op(torch.as_strided(x, x.shape, c, x.storage_offset()))


def _op_ignores_offset(x):
    """reads through the strides, but from the start of the storage"""
    return _op(torch.as_strided(x, x.shape, x.stride(), 0))


@pytest.mark.parametrize("kind", ["strided", "transposed"])
def test_comparator_flags_an_op_that_ignores_strides_or_offset(kind):
    t = _src((5, 6))
    want = (_op(t), None)
    v = LV.ARG_BUILDERS[kind](t)
    LV.assert_same_bits("correct op", (_op(v), None), want)
    for wrong in (_op_ignores_strides, _op_ignores_offset):
        with pytest.raises(AssertionError):
            LV.assert_same_bits(wrong.__name__, (wrong(v), None), want)


def test_comparator_structure_none_and_types():
    a = torch.ones(3)
    LV.assert_same_bits("nested", {"y": (a, None), "g": [a.double()]}, {"y": (a.clone(), None), "g": [a]})      # fp32 against its float64
    for got, want in (((a, None), (a, a)), ((a, a), (a, None)), ((a,), (a[:2],)), ((a,), (a + 1e-6,)), ((a * float("nan"),), (a * float("nan"),))):
        with pytest.raises(AssertionError):
            LV.assert_same_bits("differs", got, want)
    with pytest.raises(AssertionError):
        LV.assert_same_bits("structure", (a,), (a, a))


# ---- coverage: every op of functional.py has a row
EXEMPT = {"check_device_errors", "poison_lds", "dropout_mask"}          # and the *_bytes size queries: helpers that take no tensor


def _ops_of_functional():
    from multimodal_transformer_amd import functional as F
    fns = {n for n, o in vars(F).items() if inspect.isfunction(o) and o.__module__ == F.__name__ and not n.startswith("_")}
    fns = {n for n in fns if n not in EXEMPT and not n.endswith("_bytes")}
    classes = {n for n, o in vars(F).items() if inspect.isclass(o) and issubclass(o, torch.autograd.Function) and o.__module__ == F.__name__}
    return fns, classes


def test_every_op_has_a_row():
    fns, classes = _ops_of_functional()
    assert len(fns) > 40 and len(classes) >= 26, "the introspection found functional.py's ops"
    assert {"linear", "copy2d", "key_lengths", "encoder_stream_step_slots"} <= fns and "_MfnGateFn" in classes
    covered = G.covered_names()
    missing = sorted((fns | classes | {"metrics.batched_ccc", "optim.FlatAdam"}) - covered)
    assert not missing, "no row of tests/test_gpu_layouts.py exercises: %s" % ", ".join(missing)
    unknown = sorted(n for n in covered if "." not in n and n not in fns | classes)
    assert not unknown, "rows name ops that functional.py does not have: %s" % ", ".join(unknown)


def test_the_exemptions_take_no_tensor():
    from multimodal_transformer_amd import functional as F
    for name in sorted(EXEMPT | {n for n in vars(F) if n.endswith("_bytes") and not n.startswith("_")}):
        params = inspect.signature(getattr(F, name)).parameters
        assert not {"x", "t", "tensor", "mask", "state", "x_t"} & set(params), (name, list(params))


def test_rows_are_well_formed():
    names = [r.name for r in G.ROWS]
    assert len(set(names)) == len(names)
    for r in G.ROWS:
        assert all(k in ("g", "d", "f", "m", "i") and isinstance(t, torch.Tensor) and t.device.type == "cpu" for k, t in r.args), r.name
        assert all(t.dtype == (torch.int32 if k == "i" else torch.float32) for k, t in r.args), r.name
        assert all(bool(((t == 0) | (t == 1)).all()) for k, t in r.args if k == "m"), r.name
    # the shapes the work asks for: B >= 2, an odd T >= 3, two prefix lengths of which one is shorter than T
    assert G.LENGTHS == [5, 3] and tuple(G.MASK().shape) == (2, 5, 1) and G.MASK().reshape(2, 5).sum(1).tolist() == [5.0, 3.0]


# ---- host checks that raise before any launch (pure host code: CPU tensors reach them)
def test_stream_state_at_an_odd_address_is_refused():
    from multimodal_transformer_amd import functional as F
    n = 4096
    big = torch.zeros(n + 64, dtype=torch.uint8)
    F._stream_state("op", big[:n], n, big.device, "maker")                                     # aligned: accepted
    odd = big[4:4 + n]
    assert odd.is_contiguous() and odd.numel() == n and odd.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        F._stream_state("op", odd, n, big.device, "maker")
    with pytest.raises(ValueError, match="state must be a contiguous uint8"):
        F._stream_state("op", big[:2 * n:2], n, big.device, "maker")


def test_stream_positions_strided_int32_is_refused():
    from multimodal_transformer_amd import functional as F
    pos = torch.zeros(4, dtype=torch.int32)
    F._stream_positions("op", pos[:2], 2, pos.device)
    with pytest.raises(ValueError, match="positions must be a contiguous int32"):
        F._stream_positions("op", pos[::2], 2, pos.device)
    with pytest.raises(ValueError, match="positions must be"):
        F._stream_positions("op", pos[:2].long(), 2, pos.device)
