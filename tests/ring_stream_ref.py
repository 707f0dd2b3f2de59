"""The bf16-faithful fp64 reference of the one-window encoder step with a span (TEST INFRASTRUCTURE, a plain helper module beside
tests/stream_ref.py): ``stream_ref.EncoderStream`` in which, per layer, only the last ``span`` entries of the K / V lists take part, so
window t attends windows t - span + 1 .. t (csrc/step_ring.h: the ring cache holds exactly the span - 1 entries before this window's).

Every rounding site is stream_ref's: nothing but the set of keys changes, and the softmax reference point is still the row's own exact
maximum, now over the band.  ``rounding=False`` is the exact function, so row t equals
``band_ref.encoder_stack(..., span, rounding=False)[:, t]`` (tests/test_ring_stream_cpu.py, 1e-12); with ``span`` at least the number of
windows stepped nothing is ever dropped and the rows are stream_ref's, bit for bit.  The lists are TRIMMED, not masked: what left the
band cannot reach a result, as a ring row that was written over cannot.
"""
import torch

import stream_ref as S


class EncoderStream(S.EncoderStream):
    """step(x_t (B, d), mask_t (B,) or None) -> y_t (B, d); keeps the last ``span`` K and V of every layer."""

    def __init__(self, p, prefix, h, span, rounding=True):
        if isinstance(span, bool) or not isinstance(span, int) or span < 1:
            raise ValueError("span must be an int >= 1, got %r" % (span,))
        self.span = span
        super().__init__(p, prefix, h, rounding)

    def _attend(self, layer, q, k, v, keep):
        # stream_ref appends this window's K and V and attends the whole list: drop what leaves the band first, so that the list it
        # attends is positions t - span + 1 .. t
        del self.K[layer][:max(0, len(self.K[layer]) - (self.span - 1))]
        del self.V[layer][:max(0, len(self.V[layer]) - (self.span - 1))]
        return super()._attend(layer, q, k, v, keep)


def encoder_stack(p, prefix, x, mask, h, span, rounding=True):
    """band_ref.encoder_stack's arguments (eval mode: no drops) -> (B, T, d), computed one window at a time."""
    s = EncoderStream(p, prefix, h, span, rounding)
    rows = [s.step(x[:, t], None if mask is None else mask[:, t].reshape(-1)) for t in range(x.shape[1])]
    return torch.stack(rows, dim=1)
