"""The models as online predictors, one window per ``step``: the stream classes behind ``stream()``, ``slot_stream()`` and
``device_stream()`` of multiTransformer's models and of the LSTM baselines in models.  This project's own addition (the reference has no
counterpart); DESIGN 4.5 - 4.9.

A stream keeps its position in one of two places.  A host stream (``EncoderStream``, ``MFNStream``, ``LSTMStream``, ``_SequenceStream``,
``_GateStream``) has one ``t`` for the batch, a Python int passed to the step kernels by value.  A slots stream (``_Slots``:
``EncoderSlotStream``, ``MFNSlotStream``, ``LSTMSlotStream``, ``_SequenceSlotStream``, ``_GateSlotStream``) has ``positions``, one
int32 per sequence on the device, read and advanced by the positioned kernels, so its sequences are seated and released independently
and a step can be captured into a graph.  Each class decides that in its ``__init__`` and nowhere else.  The models refuse what cannot
stream (``Encoder._stream_refusals``, ``MFN._stream_refusals``, ``models._LocalAttnLSTM._stream_refusals``) before they open one of
these.  ``MultiEDLSTM`` and ``MultiARLSTM``, whose read-out feeds its own prediction back, stream free-running through entries of their
own: ``feedback_stream`` / ``feedback_slot_stream`` (``LSTMFeedbackStream``, ``LSTMFeedbackSlotStream``).

A model with a span (``causal_attention(model, span=W)``) streams from a ring K/V cache of ``span`` rows, which never fills
(``EncoderRingStream``, ``EncoderRingSlotStream``; csrc/step_ring.h): ``ring_stream(model, batch, slots=False)`` opens the
form each model has, with ring encoder streams inside."""
import ctypes
import math

import torch

from . import functional as F_hip

_INT_MAX = 2 ** 31 - 1
_RING = object()                 # in place of a composite stream's capacity: its encoders stream a span from a ring cache


def _open_encoder(encoder, batch, capacity, slots, positions=None):
    """The encoder stream of a composite stream: the encoder's own refusals pass through."""
    if capacity is _RING:
        return encoder.ring_slot_stream(batch, positions) if slots else encoder.ring_stream(batch)
    return encoder.slot_stream(batch, capacity, positions) if slots else encoder.stream(batch, capacity)


def _slot_positions(op, positions, batch, device):
    """The positions of a slots stream: a new int32 (batch) tensor, every slot idle, or the one a composite stream shares."""
    if positions is None:
        return torch.full((batch,), -1, dtype=torch.int32, device=device)
    if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or tuple(positions.shape) != (batch,) \
            or not positions.is_contiguous() or positions.device != device:
        raise ValueError("%s: positions must be a contiguous int32 (%d,) tensor on %s" % (op, batch, device))
    return positions


def _check_row(op, name, x, B, width, device, windowed=False):
    """One input of a step: float32 on ``device`` (None: not asked for, the kernel behind converts) with the shape (B, width), or
    (B, 1, width) too where ``windowed``.  Before any launch."""
    if not isinstance(x, torch.Tensor) or (device is not None and (x.dtype != torch.float32 or x.device != device)):
        raise ValueError("%s: %s must be a float32 tensor on %s, got %s on %s"
                         % (op, name, device, getattr(x, "dtype", type(x).__name__), getattr(x, "device", None)))
    if tuple(x.shape) != (B, width) and not (windowed and tuple(x.shape) == (B, 1, width)):
        raise ValueError("%s: %s must have the shape (%d,%d)%s, got %s"
                         % (op, name, B, width, " or (%d,1,%d)" % (B, width) if windowed else "", tuple(x.shape)))


def _check_mask(op, mask_t, B, device):
    if mask_t is not None and (not isinstance(mask_t, torch.Tensor) or mask_t.numel() != B or (device is not None and mask_t.device != device)):
        raise ValueError("%s: mask_t must hold one entry per sequence (%d)%s" % (op, B, "" if device is None else " on %s" % device))


def _check_history(op, x, mask, B, width, device, limit, name="x"):
    """The history of a prefill: ``x`` float32 (B, P, width) on ``device`` with 1 <= P (<= ``limit``, a plain cache's capacity; None:
    a ring), ``mask`` (B, P, 1), (B, P) or None on the same device -> P.  Before any launch."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != device:
        raise ValueError("%s: %s must be a float32 tensor on %s, got %s on %s"
                         % (op, name, device, getattr(x, "dtype", type(x).__name__), getattr(x, "device", None)))
    if x.dim() != 3 or x.shape[0] != B or x.shape[2] != width or x.shape[1] < 1:
        raise ValueError("%s: %s must have the shape (%d, P, %d) with P >= 1 windows, got %s" % (op, name, B, width, tuple(x.shape)))
    P = x.shape[1]
    if limit is not None and P > limit:
        raise ValueError("%s: P = %d windows > capacity = %d: open a stream with a larger capacity (a ring stream has no limit)"
                         % (op, P, limit))
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.device != device
                             or tuple(mask.shape) not in ((B, P), (B, P, 1))):
        raise ValueError("%s: mask must have the shape (%d, %d, 1) or (%d, %d) on %s, got %s"
                         % (op, B, P, B, P, device, tuple(getattr(mask, "shape", ()))))
    return P


def _prefill_at_zero(op, t):
    if t != 0:
        raise ValueError("%s: the stream stands at t = %d; a prefill opens a recording from its history, at t = 0 (a chunk cannot be "
                         "appended): call reset() first" % (op, t))


def _no_prefill(stream, why):
    raise NotImplementedError("%s.prefill: %s; this stream opens a recording at window 0 only: reset() / seat(), then step through "
                              "the history (DESIGN 4.13)" % (type(stream).__name__, why))


def _stream_model_checks(model, method="stream"):
    if model.training:
        raise ValueError("%s.%s: the model is in train mode; streaming is eval-mode inference (call .eval())" % (type(model).__name__, method))


class _Slots:
    """What every slots stream has instead of ``t``: ``positions``, int32 (batch) on the device, read and advanced by the step kernels
    (csrc/step_slots.h).  A slot is idle (-1, as opened), seated (0 <= position < capacity: its next window) or full (>= capacity).  A
    step gives an idle or full slot a zero row and touches nothing of it.  ``seat`` / ``release`` / ``reset`` are ordinary device
    operations on the current stream, between steps (or between the replays of a captured step); none of them synchronises."""

    slots = True

    @property
    def t(self):
        raise AttributeError("a slots stream has no single position t: every sequence has its own, see .positions (int32 on the device)")

    def _index(self, indices):
        return torch.as_tensor(indices, dtype=torch.long, device=self.positions.device).reshape(-1)

    def seat(self, indices):
        """Start a new recording in these slots: their positions become 0.  Nothing is cleared; nothing needs to be."""
        self.positions.index_fill_(0, self._index(indices), 0)

    def release(self, indices):
        """Make these slots idle: their positions become -1."""
        self.positions.index_fill_(0, self._index(indices), -1)

    def reset(self):
        """Seat every slot."""
        self.positions.zero_()

    def full(self):
        """bool (batch) on the device: the slots whose recording has used the whole capacity (no synchronisation)."""
        return self.positions >= (_INT_MAX if self.capacity is None else self.capacity)


class EncoderStream:
    """A causal ``Encoder`` run one window at a time (``Encoder.stream``): ``step(x_t)`` returns the row that the encoder's batch
    forward gives at position ``t`` of the windows stepped so far, in ONE kernel launch (csrc/encoder_step.h), and advances ``t``.
    The state is the bf16 copy of the weight matrices and the bf16 K / V of every layer for ``batch`` x ``capacity`` windows.

    ``reset()`` starts a new recording: it sets ``t`` back to 0 and neither clears nor re-reads anything.  ``refresh()`` converts the
    weights again: call it after the encoder's parameters changed (biases and LayerNorm weights are read live).  Rows agree with the
    batch forward to the distance between two roundings of the same arithmetic (about 1.5e-3 rel-L2), not bit for bit."""

    slots = False                    # True in EncoderSlotStream: positions on the device instead of ``t``

    def __init__(self, encoder, batch, capacity):
        self._shape(encoder, batch, capacity)
        self.t = 0
        self._allocate()

    def _shape(self, encoder, batch, capacity):
        """The members that describe the stream, and the refusals of its shape: nothing is allocated or launched."""
        l0 = encoder.layers[0]
        self.encoder = encoder
        self.batch, self.capacity = int(batch), int(capacity)
        self.d, self.h, self.d_ff, self.n_layers = l0.size, l0.self_attn.h, l0.feed_forward.w_1.weight.shape[0], len(encoder.layers)
        self.eps = encoder.norm.eps
        self.device = encoder.norm.a_2.device
        if self.batch < 1 or self.capacity < 1:
            raise ValueError("Encoder.stream: batch and capacity must be at least 1, got %d and %d" % (self.batch, self.capacity))
        self._dims = (self.batch, self.capacity, self.d, self.h, self.d_ff, self.n_layers)
        F_hip.encoder_stream_bytes(*self._dims)                                   # ValueError naming the limit for an unsupported shape

    def _allocate(self):
        self.state = F_hip.encoder_stream_state(*self._dims, self.device)
        self.refresh()

    def refresh(self):
        """Convert the encoder's current weight matrices into the state (one launch); the cache and ``t`` stay."""
        ps = self.encoder.flat_parameters()
        flat = self.encoder._flat_storage(ps)
        if flat is None:
            flat = torch.cat([q.detach().reshape(-1) for q in ps]).float()
        self._flat = flat.detach()
        F_hip.encoder_stream_prepare(self._flat, self.state, *self._dims)

    def reset(self):
        self.t = 0

    def step(self, x_t, mask_t=None):
        """x_t (B,d) or (B,1,d) float32 on the encoder's device, mask_t (B), (B,1) or (B,1,1) or None -> the same shape as x_t."""
        if self.t >= self.capacity:
            raise ValueError("EncoderStream.step: the stream is full (t = capacity = %d): reset() starts a new recording, "
                             "Encoder.stream(batch, capacity) opens a longer one" % self.capacity)
        self._check_step(x_t, mask_t)
        y = F_hip.encoder_stream_step(x_t.reshape(self.batch, self.d), mask_t, self._flat, self.state, self.t, self.h, self.d_ff,
                                      self.n_layers, self.capacity, self.eps)
        self.t += 1
        return y.view(x_t.shape)

    def _check_step(self, x_t, mask_t):
        _check_row("EncoderStream.step", "x_t", x_t, self.batch, self.d, self.device, windowed=True)
        _check_mask("EncoderStream.step", mask_t, self.batch, self.device)

    _ring = False                    # True in EncoderRingStream: the cache is a ring of ``span`` rows

    def _fill(self, x, mask, table=None, positions=None):
        """The batch forward over a history and the fill of the cache behind it (functional.encoder_stream_prefill) -> its rows."""
        return encoder_stream_prefill(x, mask, self._flat, self.state, self.h, self.d_ff, self.n_layers,
                                            self.span if self._ring else self.capacity, self.eps, ring=self._ring, batch=self.batch,
                                            table=table, positions=positions)

    def prefill(self, x, mask=None):
        """Open the recording from its history in ONE forward: x (B, P, d), mask (B, P, 1), (B, P) or None -> (B, P, d), the rows of
        ``Encoder.forward(x, mask)`` bit for bit; afterwards ``t == P`` and ``step`` continues as if the P windows had been stepped
        (to the distance between the batch path's rounding and the step's).  Requires ``t == 0`` and, for a plain cache,
        1 <= P <= capacity.  One fused forward plus ONE launch of encoder_prefill_kernel (csrc/step_prefill.h)."""
        op = "%s.prefill" % type(self).__name__
        _prefill_at_zero(op, self.t)
        P = _check_history(op, x, mask, self.batch, self.d, self.device, self.capacity)
        y = self._fill(x, mask)
        self.t = P
        return y

    def _slots_prefill(self, indices, x, lengths, mask, set_positions):
        op = "%s.prefill" % type(self).__name__
        k = len(indices) if hasattr(indices, "__len__") else -1
        if not 1 <= k <= self.batch:
            raise ValueError("%s: indices must name 1 .. batch = %d slots, got %r" % (op, self.batch, indices))
        P = _check_history(op, x, mask, k, self.d, self.device, self.capacity)
        table, _, prefix = prefill_table(op, indices, lengths, P, self.batch, self.capacity, self.device)
        return self._fill(x, prefix if mask is None else mask, table, self.positions if set_positions else None)

    def extend(self, x, mask=None):
        """Move the stream forward by C windows from ANY ``t``: x (B, C, d), mask (B, C, 1), (B, C) or None -> (B, C, d), the rows
        that C calls of ``step`` give, to fp32 summation order (the same rounding sites); afterwards ``t += C`` and
        ``step``, ``extend`` and the cache go on as if the windows had been stepped.  A plain cache: t + C <= capacity; a ring stream
        has no limit.  ceil(C / 16) launches of encoder_extend_kernel (csrc/encoder_extend.h), sixteen windows sharing one pass over
        the weights.  Measured: from four windows on it is faster than stepping them; for ONE window ``step`` is the
        better call, and at ``t == 0`` ``prefill`` is."""
        op = "%s.extend" % type(self).__name__
        _extend_eval(op, self.encoder)
        C = _check_chunk(op, x, mask, self.batch, self.d, self.device, self.t, self.capacity)
        y = encoder_stream_extend(x, mask, self._flat, self.state, self.t, self.h, self.d_ff, self.n_layers,
                                  self.span if self._ring else self.capacity, self.eps, ring=self._ring)
        self.t += C
        return y

    def _slots_extend(self, indices, x, lengths, mask, advance):
        op = "%s.extend" % type(self).__name__
        _extend_eval(op, self.encoder)
        k = len(indices) if hasattr(indices, "__len__") else -1
        if not 1 <= k <= self.batch:
            raise ValueError("%s: indices must name 1 .. batch = %d slots, got %r" % (op, self.batch, indices))
        C = _check_history(op, x, mask, k, self.d, self.device, None)
        table, _, _ = prefill_table(op, indices, lengths, C, self.batch, self.capacity, self.device)
        return encoder_stream_extend_slots(x, mask, self._flat, self.state, self.positions, table, self.h, self.d_ff, self.n_layers,
                                           self.span if self._ring else self.capacity, self.eps, ring=self._ring, advance=advance)


class EncoderSlotStream(_Slots, EncoderStream):
    """``EncoderStream`` with slots (``Encoder.slot_stream``; members: ``_Slots``).  ``step(x_t, mask_t)`` is ONE launch of
    encoder_step_slots_kernel: row b is what an ``EncoderStream`` of that recording alone gives at window ``positions[b]``, bit for bit
    (the same kernel body, one workgroup per sequence), and the kernel advances the positions of the slots it ran.  No position crosses
    the host, so there is no "full" error: a full slot gets a zero row, and ``full()`` shows it."""

    def __init__(self, encoder, batch, capacity, positions=None):
        self._shape(encoder, batch, capacity)
        self.positions = _slot_positions("Encoder.slot_stream", positions, self.batch, self.device)
        self._allocate()

    def step(self, x_t, mask_t=None, advance=True):
        """As ``EncoderStream.step``.  ``advance=False`` leaves the positions (a composite stream advances them once, in its last launch)."""
        self._check_step(x_t, mask_t)
        y = F_hip.encoder_stream_step_slots(x_t.reshape(self.batch, self.d), mask_t, self._flat, self.state, self.positions, self.h,
                                            self.d_ff, self.n_layers, self.capacity, self.eps, advance=advance)
        return y.view(x_t.shape)

    def prefill(self, indices, x, lengths, mask=None, advance=True):
        """Open recordings in the slots ``indices`` (k distinct ints, k <= batch) from their histories in ONE forward: x (k, P, d),
        ``lengths`` k host ints with 1 <= len <= P (<= capacity), mask (k, P[, 1]) or None: the prefix mask of the lengths -> (k, P, d),
        the rows of ``Encoder.forward(x, mask)``.  The slots may be idle, seated or full; afterwards ``positions[indices[b]] ==
        lengths[b]``, and not a byte of any other slot has changed.  One host-to-device copy (the table), no synchronisation; one fused
        forward plus ONE launch of encoder_prefill_kernel.  ``advance=False`` leaves the positions (a composite stream sets them in its
        last launch)."""
        return self._slots_prefill(indices, x, lengths, mask, bool(advance))

    def extend(self, indices, x, lengths, mask=None, advance=True):
        """Move the slots ``indices`` (k distinct ints, k <= batch) forward by their next windows: x (k, C, d), ``lengths`` k host ints
        with 1 <= len <= C, mask (k, C[, 1]) or None -> (k, C, d); row b holds the ``lengths[b]`` rows that ``EncoderStream.extend`` of
        that recording alone gives from window ``positions[indices[b]]``, bit for bit, and zeros behind them.  All or nothing, decided
        on the device: an idle slot, and one whose position plus length exceeds the capacity, gets zero rows and nothing of it
        changes; a slot that runs advances by its length (``advance=False`` leaves the positions).  Not a byte of any other slot
        changes.  One host-to-device copy (the table), no synchronisation; ceil(C / 16) launches of encoder_extend_slots_kernel."""
        return self._slots_extend(indices, x, lengths, mask, bool(advance))


def encoder_ring_step(x_t, mask_t, flat_params, state, t, h, d_ff, n_layers, span, eps=1e-6):
    """Row t of a causal encoder stack with a span: x_t (B,d), mask_t (B) or None -> y_t (B,d) = Encoder.forward(x, mask)[:, t] with
    ``causal_attention(model, span=span)`` on, from a RING cache of ``span`` rows in ``state`` (``functional.encoder_stream_state`` and
    ``encoder_stream_prepare`` with capacity := span; csrc/step_ring.h).  Position j lives in row j mod span, so any 0 <= t < INT_MAX is
    served; while t < span the row is that of ``functional.encoder_stream_step``, bit for bit.  Steps of a recording run in order; t is
    passed by value.  One launch (encoder_step_ring_kernel).  Forward only."""
    return F_hip._encoder_step("encoder_ring_step", x_t, mask_t, flat_params, state, h, d_ff, n_layers, span, eps, t=int(t), _ring=True)


def encoder_ring_step_slots(x_t, mask_t, flat_params, state, positions, h, d_ff, n_layers, span, eps=1e-6, advance=True):
    """``encoder_ring_step`` with the position of every sequence in device memory (csrc/step_slots.h): ``positions`` int32 (B), read by
    the kernel.  Row b is the row of ``encoder_ring_step`` at t = positions[b], bit for bit, and zeros, with nothing else written, where
    the slot is idle (negative) or stands at INT_MAX.  There is no limit, so no slot becomes full.  ``advance``: the kernel adds 1 to the
    position of every slot it ran.  One launch (encoder_step_ring_slots_kernel), which can be captured into a graph."""
    return F_hip._encoder_step("encoder_ring_step_slots", x_t, mask_t, flat_params, state, h, d_ff, n_layers, span, eps,
                               positions=positions, advance=advance, _ring=True)


# Prefill: a stream state filled from ONE batch forward over a recording's history (include/mmt_hip.h mmt_*_stream_prefill; the index
# rule: csrc/step_prefill_plan.h).  Eval mode, forward only.  The functional layer stands here, beside encoder_ring_step, and
# functional.py resolves these names here.
def prefill_table(op, indices, lengths, P, batch, limit, device):
    """The (dst, len) table of a slots prefill: ``indices`` k distinct ints in [0, batch), ``lengths`` k ints in [1, P] (and at most
    ``limit``, a plain cache's capacity; None: a ring) -> (an int32 (2, k) tensor on ``device``: ONE host-to-device copy and no
    synchronisation, the lengths as a list, the prefix mask of the lengths (k, P) float32 from the same copy).  ValueError before any
    launch for anything else."""
    idx, lens = check_prefill_table(op, indices, lengths, P, batch, limit)
    # the table and the prefix mask of the lengths travel as ONE buffer: int32 [dst (k) | len (k)] and then k x P floats
    k = len(idx)
    host = torch.empty(2 * k + k * P, dtype=torch.int32)
    host[:2 * k] = torch.tensor(idx + lens, dtype=torch.int32)
    host[2 * k:].view(torch.float32).view(k, P).copy_(torch.arange(P).unsqueeze(0) < torch.tensor(lens).unsqueeze(1))
    buf = host.to(device, non_blocking=True)
    return buf[:2 * k].view(2, k), lens, buf[2 * k:].view(torch.float32).view(k, P)


def check_prefill_table(op, indices, lengths, P, batch, limit):
    """The host-side refusals of ``prefill_table`` alone -> (indices, lengths) as lists of ints.  Nothing is copied or launched."""
    try:
        idx, lens = [int(i) for i in indices], [int(n) for n in lengths]
    except (TypeError, ValueError):
        raise ValueError("%s: indices and lengths must be sequences of host ints (a device tensor would synchronise)" % op)
    if not 1 <= len(idx) <= batch or len(lens) != len(idx):
        raise ValueError("%s: %d indices and %d lengths for a stream of %d slots: 1 <= k <= batch, one length per index"
                         % (op, len(idx), len(lens), batch))
    if len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= batch:
        raise ValueError("%s: indices must be distinct and in [0, batch = %d), got %s" % (op, batch, idx))
    top = P if limit is None else min(P, limit)
    if min(lens) < 1 or max(lens) > top:
        raise ValueError("%s: lengths must lie in [1, %d] (P = %d windows%s), got %s; a recording without a window is seated with seat()"
                         % (op, top, P, "" if limit is None else ", capacity = %d" % limit, lens))
    return idx, lens


def _ones_mask(B, P, device):
    """An all-ones (B, P) mask made on the host: a copy, not a launch."""
    return torch.ones(B, P, dtype=torch.float32).to(device, non_blocking=True)


def _prefill_where(op, table, positions, B_src, B_state, device):
    """(dst, len, pos) of a prefill entry: null pointers for the host's form, the rows of ``table`` and ``positions`` for the slots form."""
    if table is None:
        if positions is not None:
            F_hip._stream_positions(op, positions, B_state, device)
        return None, None, positions
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (2, B_src) or not table.is_contiguous() \
            or table.device != device:
        raise ValueError("%s: table must be a contiguous int32 (2, %d) tensor on %s (prefill_table)" % (op, B_src, device))
    if positions is not None:
        F_hip._stream_positions(op, positions, B_state, device)
    return table[0], table[1], positions


def encoder_stream_prefill(x, mask, flat_params, state, h, d_ff, n_layers, rows, eps=1e-6, ring=False, batch=None, table=None,
                           positions=None):
    """Fill the K/V cache of an encoder stream from ONE batch forward over a history: x (B_src, P, d), mask (B_src, P[, 1]) or None ->
    y (B_src, P, d), the rows of ``encoder_stack(x, mask, ..., causal=True)`` (``ring``: with ``span=rows``), bit for bit: the fused
    stack's eval forward runs as one piece into a pool workspace, ``mmt_encoder_stream_prefill`` moves K and V of every layer from that
    workspace into ``state`` on the same stream (one launch), and the workspace goes back to the pool.  ``rows``: the stream's capacity,
    or its span with ``ring``; ``batch``: the state's sequences (default B_src).  ``table`` None: sequence b fills sequence b with all P
    windows (a host stream then continues at t = P; plain form: P <= capacity).  ``table`` (``prefill_table``): row b fills sequence
    table[0, b] with its first table[1, b] windows.  ``positions``: the stream's int32 positions, which the launch sets to the lengths.
    Replaces P calls of ``encoder_stream_step`` / ``encoder_ring_step``.  Forward only."""
    op = "encoder_stream_prefill"
    F_hip._forward_only(op, (x, mask, flat_params), "an input or a parameter requires grad: call it under torch.no_grad() with detached inputs")
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("%s: x must be a float32 (B, P, d) tensor, got %s %s"
                         % (op, getattr(x, "dtype", type(x).__name__), tuple(getattr(x, "shape", ()))))
    B, P, d = x.shape
    rows, B_state = int(rows), B if batch is None else int(batch)
    if B < 1 or P < 1:
        raise ValueError("%s: x has no windows (shape %s): a recording without a history opens with reset() / seat()" % (op, tuple(x.shape)))
    if not ring and P > rows:
        raise ValueError("%s: P = %d windows > capacity = %d: open a stream with a larger capacity" % (op, P, rows))
    if B > B_state:
        raise ValueError("%s: %d sequences do not fit a stream of %d" % (op, B, B_state))
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.numel() != B * P or mask.device != x.device):
        raise ValueError("%s: mask must have B*P = %d elements (shape (B,P,1) or (B,P)) on %s" % (op, B * P, x.device))
    lib = F_hip._lib.load()
    F_hip._lib.require_hip(x, flat_params, state)
    dst, length, pos = _prefill_where(op, table, positions, B, B_state, x.device)
    nstate = F_hip.encoder_stream_bytes(B_state, rows, d, h, d_ff, n_layers)
    p_ = F_hip._f32c16(F_hip._stream_params(op, flat_params, d, d_ff, n_layers))
    F_hip._stream_state(op, state, nstate, x.device, "encoder_stream_state")
    x_ = F_hip._f32c16(x)
    m_ = _ones_mask(B, P, x.device) if mask is None else F_hip._f32c(mask).view(B, P)
    dims = (B, P, d, int(h), int(d_ff), int(n_layers))
    nbytes = lib.mmt_encoder_workspace_bytes_eval(*dims)
    if nbytes == 0:
        F_hip._lib.launch("mmt_encoder_forward", None, None, None, None, None, 0, *dims, eps, 0.0, 0)      # raises with the library's reason
    y = torch.empty_like(x_)
    ws = F_hip._lib.POOL.get(nbytes, x.device, tag=("encoder",) + dims + (False,))       # the eval forward's own workspaces: one shape, one layout
    try:
        F_hip._lib.launch("mmt_encoder_forward", x_, m_, p_, y, ws, nbytes, *dims, float(eps), 0.0, 0, causal=True, span=rows if ring else None)
        F_hip._lib.launch("mmt_encoder_stream_prefill", ws, nbytes, state, state.numel(), dst, length, pos, B, P, B_state, rows, int(bool(ring)),
                    d, int(h), int(d_ff), int(n_layers))
    finally:
        F_hip._lib.POOL.put(ws)
    return y


def decoder_stream_prefill(h_all, c_all, state, B_state, d, h_dim, n_layers, P, limit=None, table=None, positions=None):
    """Seed the carried state of a decoder stream (``decoder_stream_state``) from the decoder's scan over a history: h_all, c_all
    (P, B_src, d), what ``lstm_scan`` returned (None with ``n_layers == 0``, which carries nothing); row len - 1 of sequence b goes to the
    copy of the carried state that step len reads.  ``table`` / ``positions`` as ``encoder_stream_prefill``; in a composite stream this
    is the last launch, and it sets the positions, as the decoder's step advances them.  One launch.  Replaces P calls of
    ``decoder_stream_step``.  ``n_layers > 1``: NotImplementedError (``lstm_stack_scan`` returns the top layer only)."""
    op = "decoder_stream_prefill"
    L, d, P, B_state = int(n_layers), int(d), int(P), int(B_state)
    if L > 1:
        raise NotImplementedError("%s: a decoder of n_layers = %d: lstm_stack_scan returns the top layer's states only, so a stacked "
                                  "decoder opens at window 0: step through the history" % (op, L))
    F_hip._forward_only(op, (h_all, c_all))
    if L == 1:
        for name, a in (("h_all", h_all), ("c_all", c_all)):
            if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 3 or a.shape[0] != P or a.shape[2] != d \
                    or not a.is_contiguous():
                raise ValueError("%s: %s must be a contiguous float32 (P = %d, B, d = %d) tensor, got %s %s"
                                 % (op, name, P, d, getattr(a, "dtype", type(a).__name__), tuple(getattr(a, "shape", ()))))
        if h_all.shape != c_all.shape:
            raise ValueError("%s: h_all %s and c_all %s differ" % (op, tuple(h_all.shape), tuple(c_all.shape)))
        B = h_all.shape[1]
    else:
        h_all = c_all = None
        B = B_state if table is None else int(table.shape[1])
    F_hip._lib.require_hip(state, h_all, c_all)
    dst, length, pos = _prefill_where(op, table, positions, B, B_state, state.device)
    F_hip._stream_state(op, state, F_hip.decoder_stream_bytes(B_state, d, h_dim, L), state.device, "decoder_stream_state")
    F_hip._lib.launch("mmt_decoder_stream_prefill", h_all, c_all, state, state.numel(), dst, length, pos, B, P, B_state,
                0 if limit is None else int(limit), d, int(h_dim), L)


# Extend: a stream moved forward by C windows from ANY position, sixteen windows per launch (include/mmt_hip.h mmt_encoder_stream_extend*;
# csrc/encoder_extend.h).  Eval mode, forward only.
EXTEND_ROWS = 16                 # windows per launch (csrc/encoder_extend_plan.h MMT_EXTEND_ROWS)


def _extend_operands(op, x, mask, flat_params, state, B_state, h, d_ff, n_layers, rows):
    """The checks both forms of ``encoder_stream_extend`` share, before any launch -> (x, mask, params) as the entry takes them.
    ``B_state``: the state's sequences (None: those of x, the host form)."""
    F_hip._forward_only(op, (x, mask, flat_params), "an input or a parameter requires grad: call it under torch.no_grad() with detached inputs")
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("%s: x must be a float32 (B, C, d) tensor, got %s %s"
                         % (op, getattr(x, "dtype", type(x).__name__), tuple(getattr(x, "shape", ()))))
    B, C, d = x.shape
    if B < 1 or C < 1:
        raise ValueError("%s: x has no windows (shape %s): C must be at least 1" % (op, tuple(x.shape)))
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.numel() != B * C or mask.device != x.device):
        raise ValueError("%s: mask must have B*C = %d elements (shape (B,C,1) or (B,C)) on %s" % (op, B * C, x.device))
    F_hip._lib.require_hip(x, flat_params, state)
    nstate = F_hip.encoder_stream_bytes(B if B_state is None else B_state, rows, d, h, d_ff, n_layers)
    p_ = F_hip._stream_params(op, flat_params, d, d_ff, n_layers)
    F_hip._stream_state(op, state, nstate, x.device, "encoder_stream_state")
    return F_hip._f32c(x), None if mask is None else F_hip._f32c(mask).view(B, C), p_


def encoder_stream_extend(x, mask, flat_params, state, t, h, d_ff, n_layers, rows, eps=1e-6, ring=False):
    """Rows t .. t + C - 1 of a causal encoder stack from the K/V cache in ``state``: x (B, C, d), mask (B, C[, 1]) or None -> y (B, C, d),
    what C calls of ``encoder_stream_step`` (``ring``: ``encoder_ring_step``, with ``rows`` the span) give at t, t + 1, ..., to fp32
    summation order (the same rounding sites; every product on the matrix cores), and the cache afterwards holds the C windows as
    those calls leave it.  ``rows``: the stream's capacity, t + C <= rows; with ``ring`` its span, and no limit below INT_MAX.  t is
    passed by value.  ceil(C / 16) launches of encoder_extend_kernel and nothing else.  Forward only."""
    op = "encoder_stream_extend"
    t, rows = int(t), int(rows)
    x_, m_, p_ = _extend_operands(op, x, mask, flat_params, state, None, h, d_ff, n_layers, rows)
    B, C, d = x_.shape
    if t < 0 or (ring and t + C >= _INT_MAX):
        raise ValueError("%s: position t = %d with C = %d windows: t must lie in [0, INT_MAX - C)" % (op, t, C))
    if not ring and t + C > rows:
        raise ValueError("%s: t + C = %d + %d > capacity = %d: open a stream with a larger capacity (a ring stream has no limit)"
                         % (op, t, C, rows))
    y = torch.empty_like(x_)
    F_hip._lib.launch("mmt_encoder_stream_extend" + ("_ring" if ring else ""), x_, m_, p_, y, state, state.numel(), t, C, B, rows,
                      d, int(h), int(d_ff), int(n_layers), float(eps))
    return y


def encoder_stream_extend_slots(x, mask, flat_params, state, positions, table, h, d_ff, n_layers, rows, eps=1e-6, ring=False, advance=True):
    """``encoder_stream_extend`` with the position of every sequence in device memory (csrc/step_slots.h): x (k, C, d), ``positions`` int32
    (B_state) and ``table`` int32 (2, k) on the device (``prefill_table``): row b goes to slot table[0, b] with its first table[1, b]
    windows, from positions[table[0, b]].  All or nothing: an idle slot, and one whose position plus length exceeds the capacity
    (``ring``: reaches INT_MAX), gets zero rows and not a byte of it changes; a slot that runs has zeros in its rows behind its length and,
    with ``advance``, its position moved on by its length.  A slot the table does not name is not touched.  No position crosses the
    host.  ceil(C / 16) launches of encoder_extend_slots_kernel and nothing else."""
    op = "encoder_stream_extend_slots"
    if not isinstance(positions, torch.Tensor) or positions.dim() != 1 or positions.shape[0] < 1:
        raise ValueError("%s: positions must be the stream's int32 (B_state,) tensor" % op)
    B_state = positions.shape[0]
    x_, m_, p_ = _extend_operands(op, x, mask, flat_params, state, B_state, h, d_ff, n_layers, int(rows))
    k, C, d = x_.shape
    dst, length, pos = _prefill_where(op, table, positions, k, B_state, x_.device)
    if dst is None or pos is None:
        raise ValueError("%s: the table (prefill_table) and the positions are both needed" % op)
    y = torch.empty_like(x_)
    F_hip._lib.launch("mmt_encoder_stream_extend" + ("_ring_slots" if ring else "_slots"), x_, m_, p_, y, state, state.numel(), pos, dst, length,
                      int(bool(advance)), C, k, B_state, int(rows), d, int(h), int(d_ff), int(n_layers), float(eps))
    return y


def _check_chunk(op, x, mask, B, width, device, t, limit, name="x"):
    """The windows of an ``extend``: ``_check_history``'s checks, then t + C against a plain cache's capacity (None: a ring) -> C."""
    C = _check_history(op, x, mask, B, width, device, None, name)
    if limit is not None and t + C > limit:
        raise ValueError("%s: t + C = %d + %d windows > capacity = %d: open a stream with a larger capacity (a ring stream, "
                         "ring_stream(model, batch), has no limit)" % (op, t, C, limit))
    if limit is None and t + C >= _INT_MAX:
        raise ValueError("%s: t + C = %d + %d reaches INT_MAX, which is no position: reset() starts a new recording" % (op, t, C))
    return C


def _extend_eval(op, module):
    if module.training:
        raise ValueError("%s: the model is in train mode; streaming is eval-mode inference (call .eval())" % op)


def _no_extend(stream, why):
    raise NotImplementedError("%s.extend: %s; this stream moves one window at a time: call step once per window (DESIGN 4.14, 10)"
                              % (type(stream).__name__, why))


class EncoderRingStream(EncoderStream):
    """A causal ``Encoder`` with a span run one window at a time (``Encoder.ring_stream``): ``EncoderStream`` against a ring cache of
    ``span`` rows (csrc/step_ring.h).  ``step(x_t)`` returns the row that the batch forward with the span gives at position ``t``, in ONE
    launch of encoder_step_ring_kernel, at a cost that stops growing at t = span - 1.  ``capacity`` is None: the stream never fills
    (a host ``t`` of INT_MAX, which is no position, raises ValueError).  ``reset()`` / ``refresh()`` as ``EncoderStream``: nothing is
    cleared.  The first ``span`` rows are those of ``Encoder.stream(batch, span)`` of the same stack without the span, bit for bit, and
    a row's bits depend on the last windows only, not on ``t``."""

    def __init__(self, encoder, batch):
        self._shape(encoder, batch)
        self.t = 0
        self._allocate()

    _ring = True

    def _shape(self, encoder, batch):
        """As ``EncoderStream._shape`` with capacity := span: the state, its size query and its preparation are those of a plain
        stream of ``span`` windows, so a span above 4096 is refused with that limit's message."""
        super()._shape(encoder, batch, encoder.layers[0].self_attn.span)
        self.span, self.capacity = self.capacity, None

    def step(self, x_t, mask_t=None):
        """x_t (B,d) or (B,1,d) float32 on the encoder's device, mask_t (B), (B,1) or (B,1,1) or None -> the same shape as x_t."""
        if self.t >= _INT_MAX:
            raise ValueError("EncoderRingStream.step: t = %d is INT_MAX, which is no position: reset() starts a new recording" % self.t)
        self._check_step(x_t, mask_t)
        y = encoder_ring_step(x_t.reshape(self.batch, self.d), mask_t, self._flat, self.state, self.t, self.h, self.d_ff, self.n_layers,
                              self.span, self.eps)
        self.t += 1
        return y.view(x_t.shape)


class EncoderRingSlotStream(_Slots, EncoderRingStream):
    """``EncoderRingStream`` with slots (``Encoder.ring_slot_stream``; members: ``_Slots``).  ``step(x_t, mask_t)`` is ONE launch of
    encoder_step_ring_slots_kernel: row b is what an ``EncoderRingStream`` of that recording alone gives at window ``positions[b]``, bit
    for bit, and the kernel advances the positions of the slots it ran.  No slot becomes full: ``full()`` shows INT_MAX only."""

    def __init__(self, encoder, batch, positions=None):
        self._shape(encoder, batch)
        self.positions = _slot_positions("Encoder.ring_slot_stream", positions, self.batch, self.device)
        self._allocate()

    def step(self, x_t, mask_t=None, advance=True):
        """As ``EncoderRingStream.step``.  ``advance=False`` leaves the positions (a composite stream advances them once, in its last launch)."""
        self._check_step(x_t, mask_t)
        y = encoder_ring_step_slots(x_t.reshape(self.batch, self.d), mask_t, self._flat, self.state, self.positions, self.h, self.d_ff,
                                    self.n_layers, self.span, self.eps, advance=advance)
        return y.view(x_t.shape)

    def prefill(self, indices, x, lengths, mask=None, advance=True):
        """As ``EncoderSlotStream.prefill``, into the ring: the last min(len, span) windows of each history, with no limit on P."""
        return self._slots_prefill(indices, x, lengths, mask, bool(advance))

    def extend(self, indices, x, lengths, mask=None, advance=True):
        """As ``EncoderSlotStream.extend``, into the ring: no capacity, so only idle slots (and a position that would reach INT_MAX)
        are skipped."""
        return self._slots_extend(indices, x, lengths, mask, bool(advance))


def _no_slot_stream(model):
    raise NotImplementedError("%s.slot_stream: this model's stream keeps host-side state per recording (one position t for the batch; "
                              "with an LSTM decoder also the carried (h, c) and the first row h0 W_hh, chosen on the host at t == 0), so "
                              "its sequences cannot be seated independently; slots serve Encoder, MFN, MultiTransformer and MultiTransformerB3 "
                              "(and their wrappers).  Use stream(batch, capacity), or device_stream(batch, capacity), which keeps that "
                              "state on the device and seats sequences independently" % type(model).__name__)


def _embed_of(model):
    """(the embed's Linear, its activation) of a sequence model.  NLPTransformer: Dropout (identity in eval) -> Linear -> ReLU."""
    embed = model.embed
    return (embed[1], 1) if isinstance(embed, torch.nn.Sequential) else (embed, 0)


class _SequenceStream:
    """``stream()`` of UniFullTransformer, UniTransformer and NLPTransformer: ``step(x_t (B, window_embed_size), mask_t)`` -> the (B,1)
    prediction of that window, what the model's eval forward gives at [:, t] with causal attention on.  Around the encoder step it runs
    the kernels the batch forward runs: the embed affine map and the two read-out maps, and for the LSTM decoder one scan of T = 1
    with the carried (h, c).  ``reset()`` starts a new recording."""

    def __init__(self, model, batch, capacity):
        _stream_model_checks(model)
        self.model, self.batch = model, int(batch)
        dec = getattr(model, "decoder", None)
        if dec is not None and dec.num_layers != 1:
            raise NotImplementedError("%s.stream: a decoder with n_layers = %d; the stepping state of the stacked scan is not implemented "
                                      "(n_layers == 1 streams)" % (type(model).__name__, dec.num_layers))
        self.enc = _open_encoder(model.encoder, batch, capacity, False)
        self._embed, self._embed_act = _embed_of(model)
        self._dec = None
        if dec is not None:
            with torch.no_grad():
                Wx, W_rec, Whh, bias = F_hip.decoder_pack(dec.weight_ih_l0, dec.weight_hh_l0, dec.bias_ih_l0, dec.bias_hh_l0)
                self._dec = tuple(z.detach() for z in (Wx, W_rec, bias, F_hip.linear(model.dec_h0, Whh),
                                                       F_hip.broadcast_rows(model.dec_c0, self.batch)))
        self._h = self._c = None

    t = property(lambda self: self.enc.t)
    capacity = property(lambda self: self.enc.capacity)

    def reset(self):
        self.enc.reset()
        self._h = self._c = None

    @staticmethod
    def _affine(x, layer, act=0, rowscale=None):
        # detached views of the live parameters: an autograd node that sees a tensor requiring grad keeps its pool workspace for a
        # backward that never comes, and the next call would get a new one (an allocation and a zero fill per step)
        return F_hip.linear(x, layer.weight.detach(), layer.bias.detach(), act=act, rowscale=rowscale)

    def step(self, x_t, mask_t=None):
        m, B = self.model, self.batch
        op = "%s stream step" % type(m).__name__
        _check_row(op, "x_t", x_t, B, self._embed.in_features, None)         # the embed is ``linear``, which converts what it is given
        _check_mask(op, mask_t, B, None)
        if self.enc.capacity is not None and self.enc.t >= self.enc.capacity:          # None: a ring cache, which never fills
            raise ValueError("%s: the stream is full (t = capacity = %d)" % (op, self.enc.capacity))
        with torch.no_grad():
            first = self.enc.t == 0
            r = None if mask_t is None else mask_t.float().reshape(B)
            e = self.enc.step(self._affine(x_t, self._embed, act=self._embed_act), r)
            if self._dec is not None:
                Wx, W_rec, bias, row0, c0 = self._dec
                gx = F_hip.linear(e.view(1, B, -1), Wx, bias)                    # (1,B,4d)
                if first:
                    gx = F_hip.add_row0(gx, row0)                                # step 0 sees h0 W_hh^T, as _decode
                h_all, c_all = F_hip.lstm_scan(gx, W_rec, None if first else self._h, c0 if first else self._c)
                self._h, self._c = h_all[0], c_all[0]
                e = self._h
            return self._affine(self._affine(e, m.out[0], act=1), m.out[2], rowscale=r)

    def prefill(self, x, mask=None):
        """Open the recording from its history in ONE forward: x (B, P, window_embed_size), mask (B, P, 1), (B, P) or None -> the
        (B, P, 1) predictions of the model's eval forward over these windows, bit for bit; afterwards ``t == P``, the encoder's cache
        holds the P windows and the decoder's carried (h, c) is the scan's state behind window P - 1.  Requires ``t == 0``."""
        m, B = self.model, self.batch
        op = "%s stream prefill" % type(m).__name__
        _prefill_at_zero(op, self.enc.t)
        P = _check_history(op, x, mask, B, self._embed.in_features, self.enc.device, self.enc.capacity)
        with torch.no_grad():
            y, state = _sequence_forward(m, self._embed, self._embed_act, x, mask, lambda e, mk: self.enc.prefill(e, mk))
            if state is not None:
                self._h, self._c = state[0][P - 1], state[1][P - 1]
        return y

    def extend(self, x, mask=None):
        """Move the recording forward by C windows from ANY ``t``: x (B, C, window_embed_size), mask (B, C, 1), (B, C) or None -> the
        (B, C, 1) predictions that C calls of ``step`` give, to fp32 summation order; afterwards ``t += C`` and the decoder's carried
        (h, c) is the scan's state behind the last window.  The embed affine map over the C rows, ``enc.extend`` (ceil(C / 16)
        launches), ONE scan of T = C seeded with the carried (h, c) for the LSTM decoder, and the two read-out maps.  A plain cache:
        t + C <= capacity.  For ONE window ``step`` is the better call."""
        m, B = self.model, self.batch
        op = "%s stream extend" % type(m).__name__
        _extend_eval(op, m)
        C = _check_chunk(op, x, mask, B, self._embed.in_features, self.enc.device, self.enc.t, self.enc.capacity)
        with torch.no_grad():
            first = self.enc.t == 0
            mk = None if mask is None else mask.float().reshape(B, C)
            enc = self.enc.extend(self._affine(x, self._embed, act=self._embed_act), mk)
            if self._dec is None:
                hid = self._affine(enc, m.out[0], act=1)
                return self._affine(hid, m.out[2], rowscale=None if mk is None else mk.reshape(-1))
            Wx, W_rec, bias, row0, c0 = self._dec
            gx = F_hip.linear(F_hip.time_major(enc), Wx, bias)                   # (C,B,4d)
            if first:
                gx = F_hip.add_row0(gx, row0)                                    # window 0 sees h0 W_hh^T, as _decode
            h_all, c_all = F_hip.lstm_scan(gx, W_rec, None if first else self._h, c0 if first else self._c)
            self._h, self._c = h_all[C - 1], c_all[C - 1]
            hid = self._affine(h_all, m.out[0], act=1)                           # rows stay time-major ...
            return F_hip.batch_major(self._affine(hid, m.out[2]), None if mk is None else mk.reshape(B, C, 1))     # ... until the mask pass


def _sequence_forward(model, embed, embed_act, x, mask, encode):
    """The eval forward of UniFullTransformer, UniTransformer and NLPTransformer over x (B, P, width) with ``encode(e, mask)`` in the
    encoder's place: the launches of the model's own ``forward``, in its order -> (the (B, P, 1) predictions, (h_all, c_all) of the
    decoder's scan or None).  ``mask`` None: every window counts."""
    B, P = x.shape[0], x.shape[1]
    mk = _ones_mask(B, P, x.device).view(B, P, 1) if mask is None else mask.float().reshape(B, P, 1)
    e = _SequenceStream._affine(x, embed, act=embed_act)
    enc = encode(e, mk)
    if getattr(model, "decoder", None) is None:
        hid = _SequenceStream._affine(enc, model.out[0], act=1)
        return _SequenceStream._affine(hid, model.out[2], rowscale=mk.reshape(-1)), None
    state = []
    return model._decode(enc, mk, _state=state), state[0]


class _SequenceSlotStream(_Slots):
    """``device_stream()`` of UniFullTransformer, UniTransformer and NLPTransformer: a stream whose whole per-recording state lives on the
    device (members: ``_Slots``).  ``step(x_t (B, window_embed_size), mask_t)`` -> the (B,1) prediction of that window, in THREE launches:
    the embed affine map, the encoder's positioned step (``EncoderSlotStream``, advance off) and ONE launch of decoder_step_slots_kernel
    (csrc/decoder_step.h) for the LSTM decoder and the read-out, which advances the positions.  The decoder's carried (h, c) of every
    layer sits in ``state`` beside the bf16 copy of its weights; at position 0 the kernel takes dec_h0 / dec_c0 instead of it, so
    ``seat`` is all a new recording needs, and decoders of up to 4 layers are served (0: the read-out alone).  It owns ONE ``positions``
    tensor, which its encoder stream shares.  Row b is what this stream opened for that recording alone gives at window
    ``positions[b]``, bit for bit; no position crosses the host, so a step can be captured (``graphs.capture_stream``).

    ``refresh()`` converts the parameters again: call it after any of them changed (the decoder step reads every one from ``state``)."""

    def __init__(self, model, batch, capacity):
        _stream_model_checks(model, "device_stream")
        self.model, self.batch = model, int(batch)
        dec = getattr(model, "decoder", None)
        self.n_layers = 0 if dec is None else dec.num_layers
        self.d, self.h_dim = model.out[0].in_features, model.out[0].out_features
        self._dims = (self.batch, self.d, self.h_dim, self.n_layers)
        if self.batch >= 1:
            F_hip.decoder_stream_bytes(*self._dims)                              # ValueError naming the limit, before anything is opened
        self.enc = _open_encoder(model.encoder, batch, capacity, True)           # the encoder's refusals pass through; it makes the positions
        self.device, self.positions = self.enc.device, self.enc.positions
        self.state = F_hip.decoder_stream_state(*self._dims, self.device)
        self._embed, self._embed_act = _embed_of(model)
        self._embed_prep = None          # the embed's padded bf16 weight and bias, laid out once: its step is the row GEMM alone
        self.refresh()

    capacity = property(lambda self: self.enc.capacity)

    def refresh(self):
        """Convert the model's current parameters into the states (the encoder's and the decoder's preparation launch and the embed's
        two); the carried state, the cache and the positions stay."""
        m, dec = self.model, getattr(self.model, "decoder", None)
        self.enc.refresh()
        self._embed_prep = F_hip.linear_prepare(self._embed.weight.detach(), self._embed.bias.detach(), self._embed_prep)
        lstm = [[getattr(dec, "%s_l%d" % (n, l)).detach() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                for l in range(self.n_layers)]
        h0, c0 = (m.dec_h0.detach(), m.dec_c0.detach()) if self.n_layers else (None, None)
        out = [q.detach() for q in (m.out[0].weight, m.out[0].bias, m.out[2].weight, m.out[2].bias)]
        F_hip.decoder_stream_prepare(lstm, h0, c0, out, self.state, *self._dims)

    def step(self, x_t, mask_t=None, advance=True):
        """``advance=False``: the decoder's launch leaves the positions, so the same windows can be stepped again (a measurement at a
        fixed position; a recording advances)."""
        B, op = self.batch, "%s device_stream step" % type(self.model).__name__
        _check_row(op, "x_t", x_t, B, self._embed.in_features, self.device)
        _check_mask(op, mask_t, B, self.device)
        with torch.no_grad():
            r = None if mask_t is None else mask_t.float().reshape(B)
            e = self.enc.step(F_hip.linear_prepared(x_t, self._embed_prep, self.d, act=self._embed_act), r, advance=False)
            return F_hip.decoder_stream_step_slots(e, r, self.state, self.positions, self.d, self.h_dim, self.n_layers,
                                                   limit=self.capacity, advance=advance)

    def prefill(self, indices, x, lengths, mask=None):
        """Open recordings in the slots ``indices`` (k distinct ints, k <= batch) from their histories in ONE forward: x (k, P,
        window_embed_size), ``lengths`` k host ints with 1 <= len <= P (<= capacity), mask (k, P[, 1]) or None: the prefix mask of the
        lengths -> the (k, P, 1) predictions of the model's eval forward.  The slots may be idle, seated or full; afterwards
        ``positions[indices[b]] == lengths[b]`` and no byte of another slot has changed.  The model's forward with ONE launch of
        encoder_prefill_kernel behind the encoder and ONE of decoder_prefill_kernel behind the decoder's scan, which sets the
        positions (a model without a decoder layer carries nothing: the encoder's fill sets them); one host-to-device copy (the table), no synchronisation.  A stacked decoder: NotImplementedError."""
        m, op = self.model, "%s device_stream prefill" % type(self.model).__name__
        if self.n_layers > 1:
            _no_prefill(self, "a decoder of n_layers = %d: lstm_stack_scan returns the top layer's states only" % self.n_layers)
        k = len(indices) if hasattr(indices, "__len__") else -1
        if not 1 <= k <= self.batch:
            raise ValueError("%s: indices must name 1 .. batch = %d slots, got %r" % (op, self.batch, indices))
        P = _check_history(op, x, mask, k, self._embed.in_features, self.device, self.capacity)
        table, _, prefix = prefill_table(op, indices, lengths, P, self.batch, self.capacity, self.device)
        with torch.no_grad():
            y, state = _sequence_forward(m, self._embed, self._embed_act, x, prefix if mask is None else mask,
                                         lambda e, mk: self.enc._fill(e, mk, table, None if self.n_layers else self.positions))
            if self.n_layers:                # else: the read-out alone carries nothing, and the encoder's fill has set the positions
                decoder_stream_prefill(state[0], state[1], self.state, self.batch, self.d, self.h_dim, self.n_layers, P,
                                             limit=self.capacity, table=table, positions=self.positions)
        return y

    def extend(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_extend(self, "the decoder's carried state lives on the device and its step kernel has no chunked form (stream(), whose "
                         "decoder state lives on the host, has extend)")


class MFNStream:
    """An ``MFN`` gate run one window at a time (``MFN.stream``): ``step({mod: (B, dims[mod])}, mask_t)`` returns the (B, output_dim)
    row that the gate's eval forward gives at position ``t`` of the windows stepped so far (times ``mask_t``), in ONE kernel launch
    (csrc/mfn_step.h), and advances ``t``.  The state holds the bf16 copy of every weight matrix, the fp32 biases and two copies of
    the carried (h, c, mem) of ``batch`` sequences.

    ``reset()`` starts a new recording: it sets ``t`` back to 0 and neither clears nor re-reads anything.  ``refresh()`` converts
    and copies the parameters again: call it after ANY parameter of the gate changed.  Unlike ``EncoderStream``, which reads biases
    and LayerNorm weights live, the biases here are copies made at ``refresh()`` (``b_ih + b_hh`` already summed): the step kernel
    reads nothing but its inputs and the state.  Rows have the batch path's rounding sites exactly and agree with it to fp32
    summation order."""

    slots = False                    # True in MFNSlotStream: positions on the device instead of ``t``

    def __init__(self, mfn, batch):
        self._shape(mfn, batch)
        self.t = 0
        self._allocate()

    def _shape(self, mfn, batch):
        """The members that describe the stream, and the refusals of its shape: nothing is allocated or launched."""
        self.mfn, self.batch = mfn, int(batch)
        self.mods = list(mfn.mods)
        self.in_dims = [mfn.lstm[m].input_size for m in self.mods]
        self.hidden = [mfn.lstm[m].hidden_size for m in self.mods]
        self.output_dim = mfn.out_fc2.out_features
        self.device = mfn.out_fc2.weight.device
        if self.batch < 1:
            raise ValueError("MFN.stream: batch must be at least 1, got %d" % self.batch)
        F_hip.mfn_stream_bytes(self.batch, self.in_dims, self.hidden, self.output_dim)        # ValueError naming the limit

    def _allocate(self):
        self.state = F_hip.mfn_stream_state(self.batch, self.in_dims, self.hidden, self.output_dim, self.device)
        self.refresh()

    def refresh(self):
        """Convert and copy the gate's current parameters, biases included, into the state (one launch); (h, c, mem) and ``t`` stay."""
        cells = [tuple(q.detach() for q in (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)) for c in (self.mfn.lstm[m] for m in self.mods)]
        F_hip.mfn_stream_prepare(cells, [q.detach() for q in self.mfn._gate_params()], self.state, self.batch, self.in_dims, self.hidden,
                                 self.output_dim)

    def reset(self):
        self.t = 0

    def step(self, inputs, mask_t=None):
        """inputs {mod: (B, dims[mod]) float32 on the gate's device}, mask_t (B), (B,1) or (B,1,1) or None -> (B, output_dim)."""
        xs = _modality_rows("MFNStream.step", inputs, self.mods, self.in_dims, self.batch, self.device, mask_t)
        y = F_hip.mfn_stream_step(xs, mask_t, self.state, self.t, self.in_dims, self.hidden, self.output_dim)
        self.t += 1
        return y

    def prefill(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_prefill(self, "the MFN gate's carried (h, c, mem) is not seeded from its batch scan yet")

    def extend(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_extend(self, "the MFN gate's recurrence has no chunked form")


class MFNSlotStream(_Slots, MFNStream):
    """``MFNStream`` with slots (``MFN.slot_stream``; members: ``_Slots``, ``capacity`` is the ``limit``).  ``step(inputs, mask_t)`` is
    ONE launch of mfn_step_slots_kernel: row b is what an ``MFNStream`` of that recording alone gives at window ``positions[b]``, bit
    for bit (copy ``positions[b] & 1`` of the carried state is read and the other written, per sequence), and the kernel advances the
    positions of the slots it ran."""

    def __init__(self, mfn, batch, limit=None, positions=None):
        self._shape(mfn, batch)
        self.capacity = None if limit is None else int(limit)
        if self.capacity is not None and self.capacity < 1:
            raise ValueError("MFN.slot_stream: limit must be at least 1 (or None), got %d" % self.capacity)
        self.positions = _slot_positions("MFN.slot_stream", positions, self.batch, self.device)
        self._allocate()

    def step(self, inputs, mask_t=None, advance=True):
        xs = _modality_rows("MFNStream.step", inputs, self.mods, self.in_dims, self.batch, self.device, mask_t)
        return F_hip.mfn_stream_step_slots(xs, mask_t, self.state, self.positions, self.in_dims, self.hidden, self.output_dim,
                                           limit=self.capacity, advance=advance)


class LSTMStream:
    """An LSTM baseline (``MultiLSTM`` / ``MultiLSTMB1`` with ``models.attend_over_taps`` on) run one window at a time
    (``MultiLSTM.stream``): ``step(x_t (B, window_embed_size), mask_t)`` returns the (B,1) row that the model's eval forward gives at
    position ``t`` of the windows stepped so far, in ONE kernel launch (csrc/lstm_step.h), and advances ``t``.  The state holds the
    bf16 copy of every weight matrix, the fp32 biases, two copies of the carried (h, c) of every layer and, per sequence, a ring of
    the last attn_len masked outputs of the top layer.  There is no cache, so no capacity: a recording may be of any length.

    ``reset()`` starts a new recording: it sets ``t`` back to 0 and neither clears nor re-reads anything.  ``refresh()`` converts and
    copies the parameters again: call it after ANY parameter of the model changed (the step reads nothing but its inputs and the
    state).  Rows have the batch path's rounding sites exactly."""

    slots = False                    # True in LSTMSlotStream: positions on the device instead of ``t``
    capacity = None

    def __init__(self, model, batch):
        self._shape(model, batch)
        self.t = 0
        self._allocate()

    def _shape(self, model, batch):
        """The members that describe the stream, and the refusals of its shape: nothing is allocated or launched."""
        self.model, self.batch = model, int(batch)
        self.device = model.embed[1].weight.device
        self._dims = (model.embed[1].in_features, model.embed_dim, model.h_dim, model.n_layers, model.attn_len)
        if self.batch < 1:
            raise ValueError("%s.stream: batch must be at least 1, got %d" % (type(model).__name__, self.batch))
        self._nbytes = F_hip.lstm_stream_bytes(self.batch, *self._dims)         # ValueError naming the limit

    def _allocate(self):
        self.state = F_hip._scratch(self._nbytes, self.device)                  # any contents (functional.lstm_stream_state)
        self.refresh()

    def refresh(self):
        """Convert and copy the model's current parameters, biases included, into the state (one launch); (h, c), the ring and the
        position(s) stay."""
        m = self.model
        lin = lambda layer: [layer.weight.detach(), layer.bias.detach()]            # noqa: E731
        lstm = [[getattr(m.lstm, "%s_l%d" % (n, l)).detach() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                for l in range(m.n_layers)]
        F_hip.lstm_stream_prepare(lin(m.embed[1]), lin(m.attn[0]) + lin(m.attn[2]), lstm, lin(m.decoder[0]) + lin(m.decoder[-1]),
                                  self.state, self.batch, *self._dims)

    def reset(self):
        self.t = 0

    def _check_step(self, x_t, mask_t):
        op = "%s stream step" % type(self.model).__name__
        _check_row(op, "x_t", x_t, self.batch, self._dims[0], self.device)
        _check_mask(op, mask_t, self.batch, self.device)

    def step(self, x_t, mask_t=None):
        """x_t (B, window_embed_size) float32 on the model's device, mask_t (B), (B,1) or (B,1,1) or None -> (B,1)."""
        self._check_step(x_t, mask_t)
        y = self._host_step(x_t, mask_t)
        self.t += 1
        return y

    def _host_step(self, x_t, mask_t):
        return F_hip.lstm_stream_step(x_t, mask_t, self.state, self.t, *self._dims)

    def _slots_step(self, x_t, mask_t, advance):
        return F_hip.lstm_stream_step_slots(x_t, mask_t, self.state, self.positions, *self._dims, limit=self.capacity, advance=advance)

    def prefill(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_prefill(self, "the LSTM baselines' carried state, their ring of taps and a fed-back prediction are not seeded from the "
                          "batch scans yet")

    def extend(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_extend(self, "the LSTM baselines' recurrence, their ring of taps and a fed-back prediction have no chunked form")


class LSTMSlotStream(_Slots, LSTMStream):
    """``LSTMStream`` with slots (``MultiLSTM.slot_stream``; members: ``_Slots``, ``capacity`` is the ``limit``).  ``step(x_t, mask_t)`` is
    ONE launch of lstm_step_slots_kernel: row b is what an ``LSTMStream`` of that recording alone gives at window ``positions[b]``, bit
    for bit (copy ``positions[b] & 1`` of the carried state is read and the other written, per sequence), and the kernel advances the
    positions of the slots it ran."""

    def __init__(self, model, batch, limit=None, positions=None):
        self._shape(model, batch)
        self.capacity = None if limit is None else int(limit)
        if self.capacity is not None and self.capacity < 1:
            raise ValueError("%s.slot_stream: limit must be at least 1 (or None), got %d" % (type(model).__name__, self.capacity))
        self.positions = _slot_positions("%s.slot_stream" % type(model).__name__, positions, self.batch, self.device)
        self._allocate()

    def step(self, x_t, mask_t=None, advance=True):
        """As ``LSTMStream.step``.  ``advance=False`` leaves the positions, so the same windows can be stepped again."""
        self._check_step(x_t, mask_t)
        return self._slots_step(x_t, mask_t, advance)


# The functional layer of the two LSTM baselines whose read-out feeds its own prediction back, one window per call (include/mmt_hip.h
# mmt_lstm_feedback_stream_*): the LSTM step with a tail, on the helpers of functional.lstm_stream_*.  It stands here, beside
# encoder_ring_step, and not in functional.py.  tail: LSTM_TAIL_FB (MultiEDLSTM, the read-out in the decoder's recurrence) or
# LSTM_TAIL_AR (MultiARLSTM, ar_order taps on its own predictions).  The state is the LSTM stream's with the tail's pieces behind it;
# any contents: F_hip._scratch.  dims = (in, E, H, n_layers, attn_len), as above.
LSTM_TAIL_FB, LSTM_TAIL_AR = 1, 2


def lstm_feedback_stream_bytes(B, tail, ar_order, in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Bytes of the feedback stream state for ``B`` sequences; ValueError, naming the limit, for a shape outside the step kernel's domain."""
    return F_hip._stream_bytes("mmt_lstm_feedback_stream_bytes", "%s", b"lstm feedback stream: ?", int(tail), int(ar_order), int(B), int(in_dim),
                         int(embed_dim), int(h_dim), int(n_layers), int(attn_len))


def lstm_feedback_stream_state(B, tail, ar_order, in_dim, embed_dim, h_dim, n_layers, attn_len, device):
    """An unprepared feedback stream state on ``device`` (uint8; any contents)."""
    return F_hip._scratch(lstm_feedback_stream_bytes(B, tail, ar_order, in_dim, embed_dim, h_dim, n_layers, attn_len), device)


def lstm_feedback_stream_prepare(embed_params, attn_params, lstm_params, dec_params, tail_params, state, B, tail, ar_order,
                                 in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Convert and copy every parameter into ``state`` (one launch; no carried block or ring is touched).  The first four groups are
    those of ``lstm_stream_prepare`` (``lstm_params`` of the LSTM that reads the embedding, ``dec_params`` the read-out's W0 (E, H), b0,
    W2 (1, E), b2).  ``tail_params``, LSTM_TAIL_FB: the decoder's weight_ih (4H, 1 + H), weight_hh (4H, H), bias_ih, bias_hh and the rows
    enc_h0, enc_c0, dec_h0, dec_c0 (H elements each); LSTM_TAIL_AR: autoreg's weight (ar_order, H) and bias."""
    op = "lstm_feedback_stream_prepare"
    tail, K = int(tail), int(ar_order)
    I, E, H, NL, L = int(in_dim), int(embed_dim), int(h_dim), int(n_layers), int(attn_len)
    nbytes = lstm_feedback_stream_bytes(B, tail, K, I, E, H, NL, L)
    front = list(embed_params) + list(attn_params) + [q for layer in lstm_params for q in layer] + list(dec_params)
    tp = list(tail_params)
    F_hip._forward_only(op, front + tp, F_hip._PARAMS_GRAD)
    want = [(E, I), (E,), (E, E), (E,), (L, E), (L,)]
    want += [s for l in range(NL) for s in ((4 * H, E if l == 0 else H), (4 * H, H), (4 * H,), (4 * H,))]
    want += [(E, H), (E,), (1, E), (1,)]
    if tail == LSTM_TAIL_FB:
        want += [(4 * H, 1 + H), (4 * H, H), (4 * H,), (4 * H,)] + [(H,)] * 4
        tp = tp[:4] + [q.reshape(-1) if isinstance(q, torch.Tensor) and q.numel() == H else q for q in tp[4:]]      # (n_layers, 1, H) rows
    else:
        want += [(K, H), (K,)]
    if [tuple(q.shape) for q in front + tp] != want:
        raise ValueError("%s: the parameters have the shapes %s, expected %s" % (op, [tuple(q.shape) for q in front + tp], want))
    F_hip._lib.require_hip(state, *front, *tp)
    F_hip._stream_state(op, state, nbytes, front[0].device, "lstm_feedback_stream_state")
    if tail == LSTM_TAIL_FB:                                                # a vector job copies contiguous floats: column 0 on its own
        tp = [tp[0], tp[0][:, 0].contiguous()] + tp[1:]
    keep = [F_hip._f32c(q) for q in front + tp]                                   # alive until the launch is enqueued
    table = (ctypes.c_void_p * len(keep))(*[q.data_ptr() for q in keep])
    F_hip._lib.launch("mmt_lstm_feedback_stream_prepare", table, state, state.numel(), tail, K, int(B), I, E, H, NL, L)


def _lstm_feedback_step(op, x_t, mask_t, state, p_init, tail, ar_order, dims, t=None, positions=None, limit=None, advance=True):
    """Both forms of the step with a tail: the position is ``t``, by value, or ``positions`` on the device with their ``limit``."""
    dims = tuple(int(v) for v in dims)
    tail, K, p_init = int(tail), int(ar_order), float(p_init)
    F_hip._forward_only(op, (x_t, mask_t))
    if not isinstance(x_t, torch.Tensor) or x_t.dim() != 2 or x_t.dtype != torch.float32 or x_t.shape[1] != dims[0]:
        raise ValueError("%s: x_t must be a float32 (B, %d) tensor, got %s %s"
                         % (op, dims[0], getattr(x_t, "dtype", type(x_t).__name__), tuple(getattr(x_t, "shape", ()))))
    if not math.isfinite(p_init):
        raise ValueError("%s: p_init must be a finite float, got %r" % (op, p_init))
    B, dev = x_t.shape[0], x_t.device
    m_ = F_hip._step_mask(op, mask_t, B, dev)
    where = F_hip._step_where(op, t, positions, limit, advance, B, dev) + (p_init, tail, K)
    return F_hip._run_step(op, "mmt_" + op, x_t, m_, (B, 1), state, lambda: lstm_feedback_stream_bytes(B, tail, K, *dims),
                     "lstm_feedback_stream_state", where, dims)


def lstm_feedback_stream_step(x_t, mask_t, state, t, p_init, tail, ar_order, in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Window t of ``MultiEDLSTM`` (LSTM_TAIL_FB) or ``MultiARLSTM`` (LSTM_TAIL_AR), free-running: x_t (B, in); mask_t (B) or None ->
    y_t (B, 1) = what the model's eval ``forward(..., target=None, tgt_init=p_init)`` gives at [:, t] with ``attend_over_taps`` on.  The
    front's carried state, and the tail's (the decoder's (h, c) and its last unmasked prediction; the last ar_order unmasked
    predictions), live in ``state`` (lstm_feedback_stream_state, prepared by lstm_feedback_stream_prepare), which this call advances.
    Steps of a recording run in order t = 0, 1, ...; t and p_init are passed by value.  One launch.  Forward only."""
    return _lstm_feedback_step("lstm_feedback_stream_step", x_t, mask_t, state, p_init, tail, ar_order,
                               (in_dim, embed_dim, h_dim, n_layers, attn_len), t=int(t))


def lstm_feedback_stream_step_slots(x_t, mask_t, state, positions, p_init, tail, ar_order, in_dim, embed_dim, h_dim, n_layers, attn_len,
                                    limit=None, advance=True):
    """``lstm_feedback_stream_step`` with the position of every sequence in device memory (csrc/step_slots.h): row b is its row at
    t = positions[b], bit for bit, where the slot is seated, and zero, with nothing else written, where it is idle or full.  With
    ``advance=False`` the call can be repeated: no word it reads is one it writes.  One launch; it can be captured into a graph."""
    return _lstm_feedback_step("lstm_feedback_stream_step_slots", x_t, mask_t, state, p_init, tail, ar_order,
                               (in_dim, embed_dim, h_dim, n_layers, attn_len), positions=positions, limit=limit, advance=advance)


class _LSTMFeedback:
    """What the streams of the two models whose read-out feeds its own prediction back put in place of ``LSTMStream``'s: the shape
    (the tail, ``tgt_init``), the preparation and the call inside ``step``.  ``MultiEDLSTM``: the LSTM that reads the embedding is
    ``encoder``, started from enc_h0 / enc_c0, and the decoder cell with the read-out ``out`` in its recurrence is the tail;
    ``MultiARLSTM``: ``lstm`` from zero states, ``decoder`` and ``autoreg`` with the ring of the last ar_order predictions."""

    def _shape(self, model, batch):
        name = type(model).__name__
        self.model, self.batch = model, int(batch)
        self.device = model.embed[1].weight.device
        self._dims = (model.embed[1].in_features, model.embed_dim, model.h_dim, model.n_layers, model.attn_len)
        fb = hasattr(model, "encoder")                          # MultiEDLSTM; else MultiARLSTM
        self._tail = (LSTM_TAIL_FB, 0) if fb else (LSTM_TAIL_AR, int(model.ar_order))
        if self.batch < 1:
            raise ValueError("%s.feedback_stream: batch must be at least 1, got %d" % (name, self.batch))
        self._nbytes = lstm_feedback_stream_bytes(self.batch, *self._tail, *self._dims)     # ValueError naming the limit
        if isinstance(self.tgt_init, bool) or not isinstance(self.tgt_init, (int, float)) or not math.isfinite(self.tgt_init):
            raise ValueError("%s.feedback_stream: tgt_init must be a finite float, got %r" % (name, self.tgt_init))
        self.tgt_init = float(self.tgt_init)

    def refresh(self):
        """Convert and copy the model's current parameters, the initial rows included, into the state (one launch); every carried
        block, the rings and the position(s) stay."""
        m = self.model
        lin = lambda layer: [layer.weight.detach(), layer.bias.detach()]            # noqa: E731
        names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
        if self._tail[0] == LSTM_TAIL_FB:
            lstm, readout = m.encoder, lin(m.out[0]) + lin(m.out[2])
            tail = [getattr(m.decoder, n + "_l0").detach() for n in names] + [r.detach() for r in (m.enc_h0, m.enc_c0, m.dec_h0, m.dec_c0)]
        else:
            lstm, readout, tail = m.lstm, lin(m.decoder[0]) + lin(m.decoder[2]), lin(m.autoreg)
        layers = [[getattr(lstm, "%s_l%d" % (n, l)).detach() for n in names] for l in range(m.n_layers)]
        lstm_feedback_stream_prepare(lin(m.embed[1]), lin(m.attn[0]) + lin(m.attn[2]), layers, readout, tail, self.state, self.batch,
                                           *self._tail, *self._dims)

    def _host_step(self, x_t, mask_t):
        return lstm_feedback_stream_step(x_t, mask_t, self.state, self.t, self.tgt_init, *self._tail, *self._dims)

    def _slots_step(self, x_t, mask_t, advance):
        return lstm_feedback_stream_step_slots(x_t, mask_t, self.state, self.positions, self.tgt_init, *self._tail, *self._dims,
                                                     limit=self.capacity, advance=advance)


class LSTMFeedbackStream(_LSTMFeedback, LSTMStream):
    """``MultiEDLSTM`` / ``MultiARLSTM`` (``models.attend_over_taps`` on) run one window at a time, free-running
    (``feedback_stream``): ``step(x_t (B, window_embed_size), mask_t)`` returns the (B,1) row that the model's eval
    ``forward(inputs, mask, lengths, target=None, tgt_init=tgt_init)`` gives at position ``t``, in ONE kernel launch (csrc/lstm_step.h
    with a tail), and advances ``t``.  The prediction that is fed back is one more carried value; ``tgt_init`` is fixed when the
    stream is opened.  No cache and no capacity; ``reset()`` and ``refresh()`` as ``LSTMStream``'s."""

    def __init__(self, model, batch, tgt_init=0.0):
        self.tgt_init = tgt_init
        LSTMStream.__init__(self, model, batch)


class LSTMFeedbackSlotStream(_LSTMFeedback, LSTMSlotStream):
    """``LSTMFeedbackStream`` with slots (``feedback_slot_stream``; members: ``_Slots``, ``capacity`` is the ``limit``): row b is what
    a ``LSTMFeedbackStream`` of that recording alone gives at window ``positions[b]``, bit for bit.  ``step(..., advance=False)`` can be
    repeated: no word it reads is one it writes (two copies of every carried block; the history ring has ar_order + 1 slots)."""

    def __init__(self, model, batch, limit=None, tgt_init=0.0, positions=None):
        self.tgt_init = tgt_init
        LSTMSlotStream.__init__(self, model, batch, limit, positions)


def _modality_rows(op, inputs, mods, widths, B, device, mask_t):
    """The checks of a per-modality step, all before any launch -> the rows in the order of ``mods``."""
    if not isinstance(inputs, dict) or any(m not in inputs for m in mods):
        raise ValueError("%s: inputs must be a dict with a row for every modality %s, got %s"
                         % (op, mods, sorted(inputs) if isinstance(inputs, dict) else type(inputs).__name__))
    for m, d in zip(mods, widths):
        _check_row(op, "inputs[%r]" % m, inputs[m], B, d, device)
    _check_mask(op, mask_t, B, device)
    return [inputs[m] for m in mods]


class _GateStream:
    """``stream()`` of MultiTransformer (the MFT) and MultiTransformerB3: ``step({mod: (B, window_embed_size[mod])}, mask_t)`` -> the
    (B,1) prediction of that window, what the model's eval forward gives at [:, t] (the MFT: with causal attention on).  Per modality
    the embed affine map and, in the MFT, the encoder's step; then ONE launch for the whole MFN gate (``MFNStream``).  ``reset()``
    starts a new recording.

    ``modality_streams`` (an attribute; on for the MFT, off for B3-MFN): the per-modality launches run on ``_MOD_STREAMS`` as in the
    batch forward, joined in front of the gate's launch.  Kept where it measured faster at B = 32 on the AVL models at the reference
    sizes.  The MFT: 311 us forked against 560 us on one stream at t = 0, 574 us against 1225 us at t = 499: an encoder
    step at d = 256, N = 6 is long enough for the fork and join to pay.  B3-MFN, whose modalities only run their embed: 181 us forked
    against 126 us on one stream.  ``MMT_MODALITY_STREAMS=0`` serialises the MFT's step too."""

    takes_modalities = True          # models._FrontEndStream hands such a stream the per-modality dict
    slots = False                    # True in _GateSlotStream

    def __init__(self, model, batch, capacity):
        stacks = self._shape(model, batch, capacity)
        self.encs = None if stacks is None else {m: _open_encoder(stacks[m], batch, capacity, False) for m in self.mods}      # their refusals pass through
        self.gate = model.mfn.stream(batch)
        self.device = self.gate.device

    def _shape(self, model, batch, capacity):
        """The members that describe the stream, and its own refusals -> the model's encoder stacks, or None (B3-MFN)."""
        _stream_model_checks(model)
        self.model, self.batch = model, int(batch)
        self.mods = list(model.mods)
        self.widths = [model.embed[m].in_features for m in self.mods]
        stacks = getattr(model, "transformer", None)
        if stacks is not None and capacity is None:
            raise ValueError("%s.stream: the encoders' K/V cache needs a capacity (windows per recording)" % type(model).__name__)
        self.modality_streams = stacks is not None
        return stacks

    t = property(lambda self: self.gate.t)
    capacity = property(lambda self: None if self.encs is None else self.encs[self.mods[0]].capacity)

    def reset(self):
        self.gate.reset()
        for e in (self.encs or {}).values():
            e.reset()

    def refresh(self):
        self.gate.refresh()
        for e in (self.encs or {}).values():
            e.refresh()

    def step(self, inputs, mask_t=None):
        op = "%s stream step" % type(self.model).__name__
        xs = _modality_rows(op, inputs, self.mods, self.widths, self.batch, self.device, mask_t)
        if self.encs is not None and self.capacity is not None and self.t >= self.capacity:       # None: ring caches, which never fill
            raise ValueError("%s: the stream is full (t = capacity = %d)" % (op, self.capacity))
        return self._step(xs, mask_t, True)

    def _encoder_step(self, enc, e, r):
        return enc.step(e, r)

    def _gate_step(self, rows, r, advance):
        return self.gate.step(rows, r)           # a host stream always advances: its t is the recording's

    def _step(self, xs, mask_t, advance):
        """The step of both forms behind their checks: the per-modality launches, forked where that pays, then the gate's."""
        m, B = self.model, self.batch
        with torch.no_grad():
            r = None if mask_t is None else mask_t.float().reshape(B)
            rows = {}
            fork = self.modality_streams and len(self.mods) > 1
            main, streams = F_hip._MOD_STREAMS.begin(self.device, len(self.mods)) if fork else (None, [None] * len(self.mods))
            for mod, x, st in zip(self.mods, xs, streams):
                with torch.cuda.stream(st):                                # None: the caller's stream
                    e = _SequenceStream._affine(x, m.embed[mod])
                    rows[mod] = e if self.encs is None else self._encoder_step(self.encs[mod], e, r)
            if fork:
                F_hip._MOD_STREAMS.end(main, streams, list(rows.values()))
            return self._gate_step(rows, r, advance)

    def prefill(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_prefill(self, "the MFN gate behind the modalities is not seeded from its batch scan yet")

    def extend(self, *args, **kwargs):
        """Not implemented: NotImplementedError before any launch."""
        _no_extend(self, "the MFN gate behind the modalities has no chunked form")


class _GateSlotStream(_Slots, _GateStream):
    """``slot_stream()`` of MultiTransformer and MultiTransformerB3: ``_GateStream`` with slots (members: ``_Slots``).  It owns ONE
    ``positions`` tensor, which its encoder streams and its gate share: the encoders' launches read it, the gate's launch, the last of
    the step, advances it.  A step launches what the ``_GateStream`` step launches, with the positioned kernels in place of the two step
    kernels, and row b is what a ``_GateStream`` of that recording alone gives at window ``positions[b]``."""

    def __init__(self, model, batch, capacity):
        stacks = self._shape(model, batch, capacity)
        # ONE positions tensor: the first stream opened makes it and the others are handed it.  The encoders read it (advance off, on the
        # modality streams as before), the gate's launch, which runs behind the join, advances it.  The gate's limit is the encoders'
        # capacity, so a full slot is skipped by every launch.
        self.positions = self.encs = None
        if stacks is not None:
            self.encs = {}
            for mod in self.mods:
                self.encs[mod] = _open_encoder(stacks[mod], batch, capacity, True, self.positions)             # their refusals pass through
                self.positions = self.encs[mod].positions
        self.gate = model.mfn.slot_stream(batch, capacity if stacks is not None and capacity is not _RING else None, self.positions)
        self.device, self.positions = self.gate.device, self.gate.positions

    def step(self, inputs, mask_t=None, advance=True):
        """As ``_GateStream.step``.  ``advance=False``: the gate's launch leaves the positions, so the same windows can be stepped again
        (a measurement at a fixed position; a recording advances)."""
        xs = _modality_rows("%s stream step" % type(self.model).__name__, inputs, self.mods, self.widths, self.batch, self.device, mask_t)
        return self._step(xs, mask_t, bool(advance))

    def _encoder_step(self, enc, e, r):
        return enc.step(e, r, advance=False)

    def _gate_step(self, rows, r, advance):
        return self.gate.step(rows, r, advance=advance)


def ring_stream(model, batch, slots=False):
    """Open ``model`` as an online predictor WITHOUT a length limit: a model with a span (``causal_attention(model, span=W)``) streams
    from ring K/V caches of ``span`` rows (``EncoderRingStream``), at a cost per window that stops growing at window
    span - 1.  Serves ``Encoder``, ``NLPTransformer``, ``UniTransformer``, ``UniFullTransformer``, ``MultiTransformer`` and the
    ``MultiCNNTransformer`` / ``B2`` / ``MFT`` wrappers, and returns the form each has, with ring encoder streams inside:

      * ``slots=False``: what ``stream`` gives, one host ``t`` for the batch (``_SequenceStream``, ``_GateStream``, ``_FrontEndStream``);
      * ``slots=True``: the model's own slots form, positions on the device, independent seats, capturable
        (``graphs.capture_stream``): ``_GateSlotStream`` for the MFT, ``_SequenceSlotStream`` (``device_stream``'s) for the three
        sequence models, the same behind the window encoder for the wrappers.

    ``.capacity`` is None and ``step`` never raises "full".  Before any launch or allocation: the refusals of ``stream`` (train mode, a
    stack that is not the standard composition, ``mask_keys``, layers that are not causal, a model that is not on a HIP device;
    NotImplementedError for ``slots=False`` with a decoder of n_layers > 1), ValueError naming ``causal_attention(model, span=W)`` for a
    model without a span, and ValueError naming ``stream(batch)`` for a model without attention (B3-MFN, the LSTM baselines), which
    needs no cache to run without a limit."""
    from . import models, multiTransformer as M

    slots = bool(slots)
    if isinstance(model, M.Encoder):
        return model.ring_slot_stream(batch) if slots else model.ring_stream(batch)
    seq = getattr(model, "Transformer", None) if isinstance(model, models._FrontEnd) else model
    if isinstance(seq, M.MultiTransformer):
        form = _GateSlotStream if slots else _GateStream
    elif isinstance(seq, (M.NLPTransformer, M.UniTransformer, M.UniFullTransformer)):
        form = _SequenceSlotStream if slots else _SequenceStream
    else:
        raise ValueError("ring_stream: %s has no attention, so no K/V cache and no length limit to lift: stream(batch) already runs for "
                         "as long as the recording does" % type(model).__name__)
    if seq is model:
        return form(model, batch, _RING)
    _stream_model_checks(model, "ring_stream")
    return models._FrontEndStream(model, batch, None, seq=form(seq, batch, _RING))
