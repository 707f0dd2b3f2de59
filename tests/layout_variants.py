"""The same values in another memory layout or element type: what tests/test_gpu_layouts.py hands to every op in place of the fresh,
contiguous, 16-byte aligned fp32 tensors of the rest of the suite (tests/test_layouts_cpu.py checks every builder here on the CPU).

A plain helper beside bf16_ref.py: no fixtures, no GPU at import.  Every builder takes a CPU or device tensor and returns a tensor on
the same device that is torch.equal to it after ``.contiguous()`` (and a cast back, where the builder changes the type).  A view is
always placed so that reading ``numel()`` elements from its ``data_ptr()`` stays inside its own allocation: code that ignores the
strides reads wrong values, never foreign memory.  The rest of each buffer is filled with NaN (floats) or 3 (integers, bool: True), so
such a read shows.  A builder raises ValueError where the shape admits no such view (a one-element tensor is always contiguous).
"""
import torch

from gpu_harness import same_bits


def _filler(dtype):
    return float("nan") if dtype.is_floating_point else True if dtype == torch.bool else 3


def _buffer(shape, like):
    return torch.full(tuple(shape), _filler(like.dtype), dtype=like.dtype, device=like.device)


def offset(t):
    """Contiguous, same dtype, data_ptr() % 16 == 4: a view 4 bytes (one fp32 / int32 element) into a larger buffer."""
    size = t.element_size()
    if 4 % size:
        raise ValueError("offset: a %d-byte element cannot sit 4 bytes past a 16-byte boundary" % size)
    n = t.numel()
    buf = _buffer((n + 32,), t)
    k = ((4 - buf.data_ptr()) % 16) // size            # an allocation's base is 16-byte aligned: k = 4 / size
    v = buf[k:k + n].view(t.shape)
    v.copy_(t)
    return v


def strided(t):
    """Not contiguous.  >= 2-D: the second half of the columns of a buffer twice as wide; 1-D (and where every leading dimension is 1):
    the odd elements of a buffer twice as long.  The storage offset is not 0 either."""
    if t.numel() < 2 or t.dim() == 0:
        raise ValueError("strided: a tensor of %d element(s) is always contiguous" % t.numel())
    w = t.shape[-1]
    lead = t.numel() // max(w, 1)
    buf = _buffer(tuple(t.shape[:-1]) + (2 * w,), t)
    v = buf[..., 1::2] if (t.dim() == 1 or lead == 1) else buf[..., w:]
    if v.is_contiguous():                               # e.g. (1, 1, 1, n) handled above; (n, 1): step through the rows instead
        buf = _buffer((2 * t.shape[0],) + tuple(t.shape[1:]), t)
        v = buf[1::2]
    if v.is_contiguous():
        raise ValueError("strided: no non-contiguous view of shape %s" % (tuple(t.shape),))
    v.copy_(t)
    return v


def transposed(t):
    """>= 2-D: a permuted view of an allocation that holds the dimensions in reverse order (behind one extra leading row, so that the
    storage offset is not 0)."""
    if t.dim() < 2:
        raise ValueError("transposed: needs at least two dimensions")
    rev = tuple(reversed(t.shape))
    buf = _buffer((rev[0] + 1,) + rev[1:], t)
    v = buf[1:].permute(*reversed(range(t.dim())))
    if v.is_contiguous():
        raise ValueError("transposed: shape %s has one dimension larger than 1; its transpose is contiguous" % (tuple(t.shape),))
    v.copy_(t)
    return v


def f64(t):
    """The same numbers in float64 (every fp32 value is a float64 value)."""
    return t.double()


def as_bool(t):
    """A {0, 1} mask as bool."""
    assert bool(((t == 0) | (t == 1)).all()), "as_bool: a {0, 1} mask expected"
    return t != 0


def as_int64(t):
    """A {0, 1} mask as int64."""
    assert bool(((t == 0) | (t == 1)).all()), "as_int64: a {0, 1} mask expected"
    return t.long()


def expanded(row, shape):
    """A stride-0 gradient: ``row`` (leading dimension 1) expanded to ``shape``.  The baseline gets ``.contiguous()`` of it."""
    if row.dim() == 0 or row.shape[0] != 1 or tuple(row.shape[1:]) != tuple(shape[1:]) or shape[0] < 2:
        raise ValueError("expanded: a one-row tensor (1, %s) expected for shape %s" % (tuple(shape[1:]), tuple(shape)))
    v = row.expand(*shape)
    assert v.stride(0) == 0
    return v


# kind -> builder, for the arguments and for the gradient outputs
ARG_BUILDERS = {"offset": offset, "strided": strided, "transposed": transposed, "f64": f64}
MASK_BUILDERS = {"bool": as_bool, "int64": as_int64}
GRAD_BUILDERS = {"strided": strided, "offset": offset}         # "expanded" takes the row and the shape


def plain(t):
    """What the baseline gets: a fresh, contiguous clone at an allocation's base."""
    return t.detach().clone().contiguous()


def build(kind, t):
    """ARG_BUILDERS / MASK_BUILDERS[kind](t), or a plain clone where the shape admits no such view (one element, one dimension)."""
    try:
        return {**ARG_BUILDERS, **MASK_BUILDERS}[kind](t)
    except ValueError:
        return plain(t)


def _flatten(tag, x, out):
    if x is None or isinstance(x, torch.Tensor):
        out[tag] = x
    elif isinstance(x, (tuple, list)):
        for i, y in enumerate(x):
            _flatten("%s[%d]" % (tag, i), y, out)
    elif isinstance(x, dict):
        for k, y in x.items():
            _flatten("%s[%s]" % (tag, k), y, out)
    else:
        raise TypeError("%s: %r is neither a tensor, None nor a tuple / list / dict of them" % (tag, type(x).__name__))
    return out


def _canon(t, other):
    """The values of t, laid out plainly; fp32 against float64 (a gradient of a float64 argument) is compared in float64, exactly."""
    if t is None:
        return None
    t = t.detach().contiguous()
    if other is not None and t.dtype != other.dtype and t.dtype.is_floating_point and other.dtype.is_floating_point:
        t = t.double()
    return t


def assert_same_bits(tag, got, want):
    """got, want: tensors, None, or nested tuples / lists / dicts of them, of one structure.  Every tensor of `got` has the shape of its
    twin, is finite and torch.equal to it (gpu_harness.same_bits); None matches only None.  Raises AssertionError naming every
    difference."""
    a, b = _flatten(tag, got, {}), _flatten(tag, want, {})
    assert list(a) == list(b), "%s: the two runs returned different structures: %s against %s" % (tag, list(a), list(b))
    failures = []
    ca, cb = {}, {}
    for n in a:
        if a[n] is not None and b[n] is not None and tuple(a[n].shape) != tuple(b[n].shape):
            failures.append("%s: shape %s against %s" % (n, tuple(a[n].shape), tuple(b[n].shape)))
            continue
        ca[n], cb[n] = _canon(a[n], b[n]), _canon(b[n], a[n])
    same_bits(tag, ca, cb, failures)
    assert not failures, "\n".join(failures)
