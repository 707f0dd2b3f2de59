"""Drop-in module surface for the reference's ``multiTransformer.py`` on MI355X.

Same class names, constructor keywords, ``forward`` signatures and ``state_dict`` keys as
transformer/{SFT,MFT,B2-Trans}/multiTransformer.py, so a reference checkpoint
loads and the reference ``models.py`` / ``train.py`` can import this module in its place.
All arithmetic runs in hand-written HIP kernels through ``libmmt_hip.so``; calling a module
on CPU tensors raises (there is no CPU path).

Deviations, all documented in DESIGN.md:
  * ``MultiHeadedAttention.attn`` stays ``None`` unless asked for: the attention core never materialises the
    (B,h,T,T) probability tensor (the reference writes it at :59 and never reads it).  ``keep_attention(model)``
    / ``MultiHeadedAttention.keep_attn = True`` / ``attention_with_map(...)`` have a kernel of its own
    write it beside the core, with the core's rounding and dropout decisions.
  * ``mask_padded_keys(model)`` / ``MultiHeadedAttention.mask_keys = True`` (off by default, no counterpart in the reference):
    the padding mask then masks KEYS too, so a sequence attends only its own windows and its output no longer depends on the
    batch it is padded into.  Results then differ from the reference's by design.
  * ``causal_attention(model)`` / ``MultiHeadedAttention.causal = True`` (off by default, no counterpart in the reference): window t
    attends windows 0 .. t only, so the model can be run and trained as an online predictor.  Results then differ from the
    reference's by design.
  * train-mode dropout draws from a counter-based generator inside the kernels, not from torch's
    global generator: training-mode parity with the reference is statistical, eval-mode is numerical.
"""
import copy
import os

import torch
import torch.nn as nn

from . import _lib
from . import functional as F_hip


def clones(module, N):
    """N independent deep copies (all start from the same initial values, as in the reference :78-79)."""
    return nn.ModuleList(copy.deepcopy(module) for _ in range(N))


def _hip_device(device):
    return device if torch.cuda.is_available() else torch.device("cpu")


class LayerNorm(nn.Module):
    """Reference LayerNorm (:81-91): unbiased std, eps added to the std."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps

    def forward(self, x):
        return F_hip.layer_norm(x, self.a_2, self.b_2, self.eps)


class PositionwiseFeedForward(nn.Module):
    """w_2(dropout(relu(w_1(x))))  (:9-20)."""

    def __init__(self, d_model, d_ff, dropout=0.1):
        super().__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.w_2 = nn.Linear(d_ff, d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        hidden = F_hip.linear(x, self.w_1.weight, self.w_1.bias, act=1)
        return F_hip.linear(self.dropout(hidden), self.w_2.weight, self.w_2.bias)


def _attention(query, key, value, mask, dropout, need_attn):
    p = float(dropout.p) if dropout is not None and getattr(dropout, "training", False) else 0.0     # nn.Dropout: identity in eval
    B, h, T, dk = query.shape

    def merge(z):
        return z.transpose(1, 2).reshape(B, T, h * dk)

    m = None
    if mask is not None:
        if mask.numel() != B * T:
            raise NotImplementedError("attention(): only the query-row mask (B,1,T,1)/(B,T,1) of the reference is supported")
        m = mask.reshape(B, T, 1)
    seed = _lib.next_dropout_seed(query.device, 3) if p > 0.0 else 0
    q, k = merge(query), merge(key)
    ctx = F_hip.sdpa(q, k, merge(value), m, h, dropout_p=p, seed=seed)
    p_attn = F_hip.attn_probs(q, k, m, h, dropout_p=p, seed=seed) if need_attn else None       # one seed serves both kernels
    return ctx.reshape(B, T, h, dk).transpose(1, 2), p_attn


def attention(query, key, value, mask=None, dropout=None):
    """Scaled dot-product attention on (B,h,T,d_k) tensors (:22-34).

    ``mask`` is the reference's (B,1,T,1) (or (B,T,1)) float mask: rows where it is 0 are blanked.
    Returns (context (B,h,T,d_k), None): the probabilities are not materialised (``attention_with_map`` returns them).
    """
    return _attention(query, key, value, mask, dropout, False)


def attention_with_map(query, key, value, mask=None, dropout=None):
    """``attention`` with the reference's second return value: (context (B,h,T,d_k), p_attn (B,h,T,T)).  The map is the one the context
    was formed with (post-dropout in train mode, the same seed serves both kernels), detached.  ``attention`` itself keeps the
    reference's five parameters (:22), so the request is a function of its own and not a sixth keyword."""
    return _attention(query, key, value, mask, dropout, True)


class MultiHeadedAttention(nn.Module):
    """(:36-65).  ``linears`` = [query, key, value, output] projections.

    ``keep_attn`` (a class attribute, off; ``keep_attention`` sets it per instance): ``forward`` leaves the detached (B,h,T,T)
    probabilities of its call in ``self.attn`` as the reference does (:59), written by one extra kernel.  A diagnostic: an Encoder
    holding such a layer runs layer by layer instead of as the fused stack.

    ``mask_keys`` (a class attribute, off; ``mask_padded_keys`` sets it per instance): with a mask given, sequence b attends only the
    keys in front of its key length, ``1 +`` the index of the last non-zero mask entry of its row (``functional.key_lengths``): the
    padded windows behind a sequence get probability exactly 0 and no gradient as keys or values.  The reference (:29-31) blanks
    query rows only, so every window also attends its batch's padding; this flag removes that dependence on the batch.  Holes
    inside the prefix stay attended.  ``keep_attn`` then shows the zeros.

    ``causal`` (a class attribute, off; ``causal_attention`` sets it per instance): window t attends windows 0 .. t of its sequence only;
    later windows get probability exactly 0 and no gradient from that query (the reference, :27-31, lets every window attend the whole
    batch row).  ``keep_attn`` then shows the zeros above the diagonal.  Not combined with ``mask_keys`` (ValueError at the call): a valid
    window t < len sees keys <= t < len only, so causal attention already keeps it from the padding behind its sequence."""

    keep_attn = False
    mask_keys = False
    causal = False

    def __init__(self, h, d_model, dropout=0.1):
        super().__init__()
        assert d_model % h == 0
        self.d_k = d_model // h
        self.h = h
        self.linears = clones(nn.Linear(d_model, d_model), 4)
        self.attn = None
        self.dropout = nn.Dropout(p=dropout)

    def attention_mode(self):
        """(mask_keys, causal) of this layer; both set raises ValueError, before any launch."""
        if self.mask_keys and self.causal:
            raise ValueError("MultiHeadedAttention: mask_keys and causal are both set and cannot be combined: a valid window t < len of a "
                             "prefix-masked batch sees keys <= t < len only, so causal attention already keeps it from the padding "
                             "behind its sequence (mask_padded_keys(model, False))")
        return self.mask_keys, self.causal

    def forward(self, query, key, value, mask=None):
        mask_keys, causal = self.attention_mode()
        p = float(self.dropout.p) if self.training else 0.0
        B = query.size(0)
        q, k, v = (F_hip.linear(x, l.weight, l.bias) for l, x in zip(self.linears, (query, key, value)))
        m = None
        if mask is not None:
            if mask.numel() != B * query.size(1):
                raise NotImplementedError("only the reference's query-row mask of shape (B,T,1) is supported")
            m = mask.reshape(B, -1, 1)
        seed = _lib.next_dropout_seed(q.device, 3) if p > 0.0 else 0
        kl = F_hip.key_lengths(m) if mask_keys and m is not None else None      # derived once, serves both kernels
        ctx = F_hip.sdpa(q, k, v, m, self.h, dropout_p=p, seed=seed, key_lengths=kl, causal=causal)
        self.attn = F_hip.attn_probs(q, k, m, self.h, dropout_p=p, seed=seed, key_lengths=kl, causal=causal) if self.keep_attn else None
        return F_hip.linear(ctx, self.linears[3].weight, self.linears[3].bias)


def keep_attention(module, on=True):
    """Set ``keep_attn`` on every MultiHeadedAttention below ``module`` (the SFT / MFT / B2 models, the per-modality encoders of
    MultiTransformer) -> {qualified name: module}.  After the next forward each holds its (B,h,T,T) map in ``.attn``.

    While the flag is set an Encoder runs layer by layer, not as the fused stack: same arithmetic in eval mode within the kernels'
    rounding, but in train mode the layer-by-layer path draws other dropout seeds than the fused stack does.  The flag is a
    diagnostic, not a training mode; ``keep_attention(module, False)`` restores the fused path."""
    found = {}
    for name, m in module.named_modules():
        if isinstance(m, MultiHeadedAttention):
            m.keep_attn = bool(on)
            if not on:
                m.attn = None
            found[name] = m
    return found


def mask_padded_keys(module, on=True):
    """Set ``mask_keys`` on every MultiHeadedAttention below ``module`` (the SFT / MFT / B2 models, every modality's stack of
    MultiTransformer, the MultiCNNTransformer wrappers) -> {qualified name: module}.  From the next forward on a sequence attends only
    its own windows: keys behind its length (``functional.key_lengths`` of the mask) are masked in every layer, forward and backward.

    An Encoder keeps running as the fused stack (it derives the lengths once per call); only layers that disagree about the flag make
    it run layer by layer.  Outputs then differ from the reference's, which lets padded windows be attended — by design: they no
    longer depend on the batch a sequence sits in.  ``mask_padded_keys(module, False)`` restores the reference's semantics and the
    plain kernels."""
    found = {}
    for name, m in module.named_modules():
        if isinstance(m, MultiHeadedAttention):
            m.mask_keys = bool(on)
            found[name] = m
    return found


def causal_attention(module, on=True):
    """Set ``causal`` on every MultiHeadedAttention below ``module`` (the SFT / MFT / B2 models, every modality's stack of
    MultiTransformer, the MultiCNNTransformer wrappers) -> {qualified name: module}.  From the next forward on window t attends
    windows 0 .. t of its sequence only, in every layer, forward and backward: every other part of these models already runs forward in
    time (window encoder, LayerNorm, FFN and residuals are per window), so the model's output at window t no longer depends on later
    windows.

    An Encoder keeps running as the fused stack; only layers that disagree about the flag make it run layer by layer.  Outputs then
    differ from the reference's, whose windows attend the whole recording — by design.  Not combined with ``mask_padded_keys`` (the
    next forward raises ValueError; causal attention already keeps a valid window from its batch's padding).
    ``causal_attention(module, False)`` restores the reference's semantics and the plain kernels."""
    found = {}
    for name, m in module.named_modules():
        if isinstance(m, MultiHeadedAttention):
            m.causal = bool(on)
            found[name] = m
    return found


class SublayerConnection(nn.Module):
    """x + dropout(sublayer(norm(x)))  (:93-104)."""

    def __init__(self, size, dropout):
        super().__init__()
        self.norm = LayerNorm(size)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, sublayer):
        return x + self.dropout(sublayer(self.norm(x)))


class EncoderLayer(nn.Module):
    """(:106-116)."""

    def __init__(self, size, self_attn, feed_forward, dropout):
        super().__init__()
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.sublayer = clones(SublayerConnection(size, dropout), 2)
        self.size = size

    def forward(self, x, mask):
        x = self.sublayer[0](x, lambda z: self.self_attn(z, z, z, mask))
        return self.sublayer[1](x, self.feed_forward)

    def _is_standard(self):
        a, f = self.self_attn, self.feed_forward
        return (type(a) is MultiHeadedAttention and type(f) is PositionwiseFeedForward
                and a.linears[0].weight.shape == (self.size, self.size)
                and f.w_1.weight.shape[1] == self.size and f.w_2.weight.shape[0] == self.size)

    def _flat_order(self):
        """Parameters in the order the fused stack expects (= registration order of the reference)."""
        a, f, s = self.self_attn, self.feed_forward, self.sublayer
        out = []
        for l in a.linears:
            out += [l.weight, l.bias]
        out += [f.w_1.weight, f.w_1.bias, f.w_2.weight, f.w_2.bias,
                s[0].norm.a_2, s[0].norm.b_2, s[1].norm.a_2, s[1].norm.b_2]
        return out


class Encoder(nn.Module):
    """N layers and a final LayerNorm (:67-76), executed as one fused HIP stack (one forward and one
    backward library call for the whole stack) when the layers are the standard composition."""

    def __init__(self, layer, N):
        super().__init__()
        self.layers = clones(layer, N)
        self.norm = LayerNorm(layer.size)
        self._flat = None        # one buffer holding every parameter of the stack in the library's order; the Parameters are views of it
        self._flat_sig = None    # data pointers of the 16 N + 2 parameters while they are such views

    def _apply(self, fn, *args, **kwargs):        # .to() / .cuda() / .float() replace the parameters' storage
        self._flat = None
        return super()._apply(fn, *args, **kwargs)

    def _flat_storage(self, ps):
        """The fused stack reads its 16 N + 2 parameter tensors as ONE flat fp32 buffer.  Concatenating them costs a kernel per step, so the
        Parameters are re-seated once as views of such a buffer (like ``nn.LSTM.flatten_parameters``): optimizers and ``load_state_dict``
        update them in place and the buffer follows.  Anything that replaces the storage of ANY parameter (``w.data = ...``, pruning or
        re-initialisation utilities, ``load_state_dict(assign=True)``) is detected by the signature of all 16 N + 2 pointers, the same
        check ``optim.FlatAdam`` makes, and the buffer is rebuilt."""
        flat = self._flat
        if flat is not None and tuple(q.data_ptr() for q in ps) == self._flat_sig:
            return flat
        dev = ps[0].device
        if torch.cuda.is_current_stream_capturing() or any(q.device != dev or q.dtype != torch.float32 or not q.is_contiguous() for q in ps):
            return None
        flat = torch.empty(sum(q.numel() for q in ps), dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for q in ps:
                view = flat[off:off + q.numel()].view(q.shape)
                view.copy_(q.data)
                q.data = view
                off += q.numel()
        self._flat = flat
        self._flat_sig = tuple(q.data_ptr() for q in ps)
        return flat

    def _fusable(self):
        if len(self.layers) == 0:
            return False
        l0 = self.layers[0]
        if not all(type(l) is EncoderLayer and l._is_standard() for l in self.layers):
            return False
        if any(l.self_attn.keep_attn for l in self.layers):       # the fused stack never forms the map: run layer by layer
            return False
        if any(l.self_attn.mask_keys != l0.self_attn.mask_keys for l in self.layers):      # one set of key lengths serves the whole stack
            return False
        if any(l.self_attn.causal != l0.self_attn.causal for l in self.layers):            # and one attention mode
            return False
        h, f = l0.self_attn.h, l0.feed_forward.w_1.weight.shape[0]
        p = l0.sublayer[0].dropout.p
        for l in self.layers:
            if l.self_attn.h != h or l.feed_forward.w_1.weight.shape[0] != f or l.size != l0.size:
                return False
            if any(abs(q - p) > 0 for q in (l.sublayer[0].dropout.p, l.sublayer[1].dropout.p,
                                            l.self_attn.dropout.p, l.feed_forward.dropout.p)):
                return False
        return True

    def flat_parameters(self):
        ps = []
        for l in self.layers:
            ps += l._flat_order()
        return ps + [self.norm.a_2, self.norm.b_2]

    def forward(self, x, mask):
        if not self._fusable():
            for layer in self.layers:
                x = layer(x, mask)
            return self.norm(x)
        l0 = self.layers[0]
        mask_keys, causal = l0.self_attn.attention_mode()      # the layers agree (_fusable); both set: ValueError before any launch
        for l in self.layers:                    # the fused stack forms no map: one kept by an earlier layer-by-layer call is stale
            if l.self_attn.attn is not None:
                l.self_attn.attn = None
        p = l0.sublayer[0].dropout.p if self.training else 0.0
        k = self._sub_batch_streams(x)
        seed = [_lib.next_dropout_seed(x.device, 1, holder=self, index=i) for i in range(k)] if p > 0.0 else 0
        ps = self.flat_parameters()
        kl = F_hip.key_lengths(mask) if mask_keys else None                    # mask_padded_keys: derived once per call, for every layer
        return F_hip.encoder_stack_params(x, mask, ps, l0.self_attn.h, l0.feed_forward.w_1.weight.shape[0],
                                          len(self.layers), eps=self.norm.eps, dropout_p=p, seed=seed,
                                          flat=self._flat_storage(ps) if x.is_cuda else None, nsplit=k, key_lengths=kl,
                                          causal=causal)

    def stream(self, batch, capacity):
        """Open an ``EncoderStream``: this stack as an online predictor for ``batch`` recordings of up to ``capacity`` windows, one
        window per ``step`` against a K/V cache instead of a forward over the whole prefix.  Eval mode, forward only; every layer must
        attend causally (``causal_attention(model)``).  Raises ValueError, before any launch, for anything else."""
        name = type(self).__name__
        if self.training:
            raise ValueError("%s.stream: the encoder is in train mode; streaming is eval-mode inference (call .eval())" % name)
        if not self._fusable():
            raise ValueError("%s.stream: the stack is not the standard composition the fused kernels run (EncoderLayer of "
                             "MultiHeadedAttention and PositionwiseFeedForward with one width, h, d_ff and attention mode in every "
                             "layer, keep_attention off): use such a stack" % name)
        l0 = self.layers[0].self_attn
        if l0.mask_keys:
            raise ValueError("%s.stream: mask_keys is set; a stream attends its own past only, which already keeps it from any padding "
                             "(mask_padded_keys(model, False))" % name)
        if not l0.causal:
            raise ValueError("%s.stream: the layers do not attend causally, so window t depends on later windows and cannot be "
                             "predicted online: call causal_attention(model) (and train the model that way)" % name)
        if self.norm.a_2.device.type != "cuda":
            raise ValueError("%s.stream: the encoder is on %s; move it to a HIP device (there is no CPU path)" % (name, self.norm.a_2.device))
        return EncoderStream(self, batch, capacity)

    def slot_stream(self, batch, capacity, positions=None):
        """``stream(batch, capacity)`` with slots (``EncoderSlotStream``): the position of every sequence lives on the device, so the
        sequences are seated and released independently and a step can be captured into a graph (``graphs.capture_stream``).  The same
        refusals, before any launch."""
        return EncoderSlotStream(self.stream(batch, capacity), positions)

    sub_batch_streams = 1        # set to 2: the batch runs as two halves on two HIP streams (functional._SPLIT_STREAMS); opt-in
    sub_batch_min_windows = 8192

    def _sub_batch_streams(self, x):
        """``sub_batch_streams`` sub-batches on streams of their own when the call is large enough for it to pay (>= 8192 windows:
        every BASELINE configuration) and is not itself one of several concurrent pieces (a modality of the MFT).  Off by default:
        -3.5 % step time at configs[3]'s 32 sequences, -11 % at 64, but the halves draw dropout masks of their own and per-kernel
        timings (bench.py's roofline) are no longer those of a kernel that has the GPU to itself."""
        k = int(os.environ.get("MMT_ENCODER_STREAMS", self.sub_batch_streams))
        if not x.is_cuda or k < 2 or x.shape[0] < 2 or x.shape[0] * x.shape[1] < self.sub_batch_min_windows or _lib.on_side_lane(x.device):
            return 1
        return min(k, x.shape[0])


class EncoderStream:
    """A causal ``Encoder`` run one window at a time (``Encoder.stream``): ``step(x_t)`` returns the row that the encoder's batch
    forward gives at position ``t`` of the windows stepped so far, in ONE kernel launch (csrc/encoder_step.h), and advances ``t``.
    The state is the bf16 copy of the weight matrices and the bf16 K / V of every layer for ``batch`` x ``capacity`` windows.

    ``reset()`` starts a new recording: it sets ``t`` back to 0 and neither clears nor re-reads anything.  ``refresh()`` converts the
    weights again: call it after the encoder's parameters changed (biases and LayerNorm weights are read live).  Rows agree with the
    batch forward to the distance between two roundings of the same arithmetic (about 1.5e-3 rel-L2), not bit for bit."""

    slots = False                    # True in EncoderSlotStream: positions on the device instead of ``t``

    def __init__(self, encoder, batch, capacity):
        l0 = encoder.layers[0]
        self.encoder = encoder
        self.batch, self.capacity = int(batch), int(capacity)
        if not self.slots:
            self.t = 0
        self.d, self.h, self.d_ff, self.n_layers = l0.size, l0.self_attn.h, l0.feed_forward.w_1.weight.shape[0], len(encoder.layers)
        self.eps = encoder.norm.eps
        self.device = encoder.norm.a_2.device
        if self.batch < 1 or self.capacity < 1:
            raise ValueError("Encoder.stream: batch and capacity must be at least 1, got %d and %d" % (self.batch, self.capacity))
        self._dims = (self.batch, self.capacity, self.d, self.h, self.d_ff, self.n_layers)
        self.state = F_hip.encoder_stream_state(*self._dims, self.device)        # ValueError naming the limit for an unsupported shape
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
        if not isinstance(x_t, torch.Tensor) or x_t.dtype != torch.float32 or x_t.device != self.device:
            raise ValueError("EncoderStream.step: x_t must be a float32 tensor on %s, got %s on %s"
                             % (self.device, getattr(x_t, "dtype", type(x_t).__name__), getattr(x_t, "device", None)))
        if tuple(x_t.shape) not in ((self.batch, self.d), (self.batch, 1, self.d)):
            raise ValueError("EncoderStream.step: x_t must have the shape (%d,%d) or (%d,1,%d), got %s"
                             % (self.batch, self.d, self.batch, self.d, tuple(x_t.shape)))
        if mask_t is not None and (not isinstance(mask_t, torch.Tensor) or mask_t.numel() != self.batch or mask_t.device != self.device):
            raise ValueError("EncoderStream.step: mask_t must hold one entry per sequence (%d) on %s" % (self.batch, self.device))


_INT_MAX = 2 ** 31 - 1


def _slot_positions(op, positions, batch, device):
    """The positions of a slots stream: a new int32 (batch) tensor, every slot idle, or the one a composite stream shares."""
    if positions is None:
        return torch.full((batch,), -1, dtype=torch.int32, device=device)
    if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or tuple(positions.shape) != (batch,) \
            or not positions.is_contiguous() or positions.device != device:
        raise ValueError("%s: positions must be a contiguous int32 (%d,) tensor on %s" % (op, batch, device))
    return positions


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


class EncoderSlotStream(_Slots, EncoderStream):
    """``EncoderStream`` with slots (``Encoder.slot_stream``; members: ``_Slots``).  ``step(x_t, mask_t)`` is ONE launch of
    encoder_step_slots_kernel: row b is what an ``EncoderStream`` of that recording alone gives at window ``positions[b]``, bit for bit
    (the same kernel body, one workgroup per sequence), and the kernel advances the positions of the slots it ran.  No position crosses
    the host, so there is no "full" error: a full slot gets a zero row, and ``full()`` shows it."""

    def __init__(self, opened, positions=None):
        self.__dict__.update({k: v for k, v in opened.__dict__.items() if k != "t"})     # the state and the weights of the stream just opened
        self.positions = _slot_positions("Encoder.slot_stream", positions, self.batch, self.device)

    def step(self, x_t, mask_t=None, advance=True):
        """As ``EncoderStream.step``.  ``advance=False`` leaves the positions (a composite stream advances them once, in its last launch)."""
        self._check_step(x_t, mask_t)
        y = F_hip.encoder_stream_step_slots(x_t.reshape(self.batch, self.d), mask_t, self._flat, self.state, self.positions, self.h,
                                            self.d_ff, self.n_layers, self.capacity, self.eps, advance=advance)
        return y.view(x_t.shape)


def _stream_model_checks(model):
    if model.training:
        raise ValueError("%s.stream: the model is in train mode; streaming is eval-mode inference (call .eval())" % type(model).__name__)


def _no_slot_stream(model):
    raise NotImplementedError("%s.slot_stream: this model's stream keeps host-side state per recording (one position t for the batch; "
                              "with an LSTM decoder also the carried (h, c) and the first row h0 W_hh, chosen on the host at t == 0), so "
                              "its sequences cannot be seated independently; slots serve Encoder, MFN, MultiTransformer and MultiTransformerB3 "
                              "(and their wrappers).  Use stream(batch, capacity), or device_stream(batch, capacity), which keeps that "
                              "state on the device and seats sequences independently" % type(model).__name__)


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
        self.enc = model.encoder.stream(batch, capacity)
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

    def _embed(self, x_t):
        m = self.model
        if isinstance(m.embed, nn.Sequential):                    # NLPTransformer: Dropout (identity in eval) -> Linear -> ReLU
            return self._affine(x_t, m.embed[1], act=1)
        return self._affine(x_t, m.embed)

    def step(self, x_t, mask_t=None):
        m, B = self.model, self.batch
        if not isinstance(x_t, torch.Tensor) or x_t.dim() != 2 or x_t.shape[0] != B:
            raise ValueError("%s stream step: x_t must have the shape (%d, window_embed_size), got %s"
                             % (type(m).__name__, B, tuple(getattr(x_t, "shape", ()))))
        if self.enc.t >= self.enc.capacity:
            raise ValueError("%s stream step: the stream is full (t = capacity = %d)" % (type(m).__name__, self.enc.capacity))
        if mask_t is not None and (not isinstance(mask_t, torch.Tensor) or mask_t.numel() != B):
            raise ValueError("%s stream step: mask_t must hold one entry per sequence (%d)" % (type(m).__name__, B))
        with torch.no_grad():
            first = self.enc.t == 0
            r = None if mask_t is None else mask_t.float().reshape(B)
            e = self.enc.step(self._embed(x_t), r)
            if self._dec is not None:
                Wx, W_rec, bias, row0, c0 = self._dec
                gx = F_hip.linear(e.view(1, B, -1), Wx, bias)                    # (1,B,4d)
                if first:
                    gx = F_hip.add_row0(gx, row0)                                # step 0 sees h0 W_hh^T, as _decode
                h_all, c_all = F_hip.lstm_scan(gx, W_rec, None if first else self._h, c0 if first else self._c)
                self._h, self._c = h_all[0], c_all[0]
                e = self._h
            return self._affine(self._affine(e, m.out[0], act=1), m.out[2], rowscale=r)


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
        name = type(model).__name__
        if model.training:
            raise ValueError("%s.device_stream: the model is in train mode; streaming is eval-mode inference (call .eval())" % name)
        self.model, self.batch = model, int(batch)
        dec = getattr(model, "decoder", None)
        self.n_layers = 0 if dec is None else dec.num_layers
        self.d, self.h_dim = model.out[0].in_features, model.out[0].out_features
        self._dims = (self.batch, self.d, self.h_dim, self.n_layers)
        if self.batch >= 1:
            F_hip.decoder_stream_bytes(*self._dims)                              # ValueError naming the limit, before anything is opened
        opened = model.encoder.stream(batch, capacity)                           # the encoder's refusals pass through
        self.device = opened.device
        self.positions = _slot_positions("%s.device_stream" % name, None, self.batch, self.device)
        self.enc = EncoderSlotStream(opened, self.positions)
        self.state = F_hip.decoder_stream_state(*self._dims, self.device)
        embed = model.embed
        self._embed, self._embed_act = (embed[1], 1) if isinstance(embed, nn.Sequential) else (embed, 0)     # NLPTransformer: Dropout -> Linear -> ReLU
        self._embed_prep = None          # the embed's padded bf16 weight and bias, laid out once: its step is the row GEMM alone
        self.refresh()

    capacity = property(lambda self: self.enc.capacity)

    def refresh(self):
        """Convert the model's current parameters into the states (the encoder's and the decoder's preparation launch and the embed's
        two); the carried state, the cache and the positions stay."""
        m, dec = self.model, getattr(self.model, "decoder", None)
        self.enc.refresh()
        self._embed_prep = F_hip.linear_prepare(self._embed.weight.detach(), self._embed.bias.detach(), self._embed_prep)
        lstm =[[getattr(dec, "%s_l%d" % (n, l)).detach() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                for l in range(self.n_layers)]
        h0, c0 = (m.dec_h0.detach(), m.dec_c0.detach()) if self.n_layers else (None, None)
        out = [q.detach() for q in (m.out[0].weight, m.out[0].bias, m.out[2].weight, m.out[2].bias)]
        F_hip.decoder_stream_prepare(lstm, h0, c0, out, self.state, *self._dims)

    def step(self, x_t, mask_t=None, advance=True):
        """``advance=False``: the decoder's launch leaves the positions, so the same windows can be stepped again (a measurement at a
        fixed position; a recording advances)."""
        m, B = self.model, self.batch
        op = "%s device_stream step" % type(m).__name__
        if not isinstance(x_t, torch.Tensor) or x_t.dtype != torch.float32 or x_t.device != self.device:
            raise ValueError("%s: x_t must be a float32 tensor on %s, got %s on %s"
                             % (op, self.device, getattr(x_t, "dtype", type(x_t).__name__), getattr(x_t, "device", None)))
        if tuple(x_t.shape) != (B, self._embed.in_features):
            raise ValueError("%s: x_t must have the shape (%d,%d), got %s" % (op, B, self._embed.in_features, tuple(x_t.shape)))
        if mask_t is not None and (not isinstance(mask_t, torch.Tensor) or mask_t.numel() != B or mask_t.device != self.device):
            raise ValueError("%s: mask_t must hold one entry per sequence (%d) on %s" % (op, B, self.device))
        with torch.no_grad():
            r = None if mask_t is None else mask_t.float().reshape(B)
            e = self.enc.step(F_hip.linear_prepared(x_t, self._embed_prep, self.d, act=self._embed_act), r, advance=False)
            return F_hip.decoder_stream_step_slots(e, r, self.state, self.positions, self.d, self.h_dim, self.n_layers,
                                                   limit=self.capacity, advance=advance)


def _encoder(embed_dim, h, d_ff, dropout, N):
    return Encoder(EncoderLayer(embed_dim, MultiHeadedAttention(h, embed_dim), PositionwiseFeedForward(embed_dim, d_ff, dropout),
                                dropout), N)


# The modalities of the MFT are independent until the MFN gate: their embeds, encoder stacks and LSTM scans run on one HIP stream each
# (the first on the caller's stream): one stack at the reference sizes fills only part of the 256 CUs, so concurrency, not a faster
# kernel, is what is missing.  ``MMT_MODALITY_STREAMS=0`` serialises everything on one stream.
_MOD_STREAMS = _lib.StreamFork("MMT_MODALITY_STREAMS")


class MFN(nn.Module):
    """Memory Fusion Network gate (transformer/MFT/multiTransformer.py:118-248).

    inputs: {mod: (T,B,dims[mod])} -> (B,T,output_dim).  The reference walks T steps of ~40 small ops; here
    only the two true recurrences run as scans (per-modality LSTM state, and the memory update) and
    everything that depends only on the inputs or on the LSTM cell states is batched over all T windows
    through the row GEMM:
        A  gx_mod = x W_ih^T + b              -> LSTM scan             (:207-208)
        B  att1 / att2 MLPs on cStar, and the `attended` part of both gamma fc1 layers   (:218-223)
        C  memory scan                        (:221-224)
        D  read-out MLP                       (:238-247)
    """
    hidden_dim = {"linguistic": 88, "emotient": 16, "acoustic": 48, "image": 88}

    def __init__(self, mods, dims, output_dim, device=torch.device("cuda:0")):
        super().__init__()
        self.mods = list(mods)
        self.dims = dims
        total_h = sum(self.hidden_dim[m] for m in self.mods)
        self.mem_dim = 128
        att_in = 2 * total_h
        gamma_in = att_in + self.mem_dim
        self.lstm = {}
        for mod in self.mods:
            self.lstm[mod] = nn.LSTMCell(dims[mod], self.hidden_dim[mod])
            self.add_module("lstm_%s" % mod, self.lstm[mod])
        self.att1_fc1 = nn.Linear(att_in, 128)
        self.att1_fc2 = nn.Linear(128, att_in)
        self.att1_dropout = nn.Dropout(0.0)
        self.att2_fc1 = nn.Linear(att_in, 256)
        self.att2_fc2 = nn.Linear(256, self.mem_dim)
        self.att2_dropout = nn.Dropout(0.0)
        self.gamma1_fc1 = nn.Linear(gamma_in, 64)
        self.gamma1_fc2 = nn.Linear(64, self.mem_dim)
        self.gamma1_dropout = nn.Dropout(0.2)
        self.gamma2_fc1 = nn.Linear(gamma_in, 64)
        self.gamma2_fc2 = nn.Linear(64, self.mem_dim)
        self.gamma2_dropout = nn.Dropout(0.2)
        self.out_fc1 = nn.Linear(total_h + self.mem_dim, 64)
        self.out_fc2 = nn.Linear(64, output_dim)
        self.out_dropout = nn.Dropout(0.5)
        self.device = _hip_device(device)
        self.to(self.device)

    def _gate_params(self):
        out = []
        for l in (self.att1_fc1, self.att1_fc2, self.att2_fc1, self.att2_fc2, self.gamma1_fc1, self.gamma1_fc2,
                  self.gamma2_fc1, self.gamma2_fc2, self.out_fc1, self.out_fc2):
            out += [l.weight, l.bias]
        return out

    def forward(self, inputs):
        return self._gate(inputs, None)

    def _gate(self, inputs, mask):
        """inputs: {mod: (T,B,d)} -> (B,T,output_dim).  ``mask`` (B,T,1) or None: multiplied onto the output while it is brought
        back to batch-major (MultiTransformer's ``* mask.float()``, :310, in the same pass)."""
        pg = self.gamma1_dropout.p if self.training else 0.0        # gamma dropout runs inside the memory scan
        if self.training and self.gamma2_dropout.p != self.gamma1_dropout.p:
            raise NotImplementedError("MFN: gamma1_dropout and gamma2_dropout must share one probability")
        if self.training and (self.att1_dropout.p or self.att2_dropout.p):
            raise NotImplementedError("MFN: att1_dropout / att2_dropout are 0 in the reference (:161,165); other values are not implemented")
        po = self.out_dropout.p if self.training else 0.0           # out_dropout rides in the read-out kernel's epilogue
        seed_g = _lib.next_dropout_seed(self.device, 2, holder=self) if pg > 0.0 else 0
        seed_o = _lib.next_dropout_seed(self.device, 4, holder=self) if po > 0.0 else 0
        hs, cs = [], []
        main, streams = _MOD_STREAMS.begin(self.device, len(self.mods))
        for mod, st in zip(self.mods, streams):
            with torch.cuda.stream(st):
                cell = self.lstm[mod]
                gx = F_hip.linear(inputs[mod], cell.weight_ih, F_hip.add2(cell.bias_ih, cell.bias_hh))     # (T,B,4H)
                h_all, c_all = F_hip.lstm_scan(gx, cell.weight_hh)
                hs.append(h_all)
                cs.append(c_all)
        _MOD_STREAMS.end(main, streams, hs + cs)
        out = F_hip.mfn_gate(hs, cs, self._gate_params(), pg, seed_g, po, seed_o)          # (T,B,output_dim)
        return F_hip.batch_major(out, mask)

    def stream(self, batch):
        """Open an ``MFNStream``: this gate as an online predictor for ``batch`` recordings, one window per ``step`` with the carried
        (h, c, mem) instead of a forward over the whole prefix.  Eval mode, forward only; no attention, so no length limit.  Raises
        ValueError, before any launch, for anything else."""
        if self.training:
            raise ValueError("MFN.stream: the gate is in train mode; streaming is eval-mode inference (call .eval())")
        dev = self.out_fc2.weight.device
        if dev.type != "cuda":
            raise ValueError("MFN.stream: the gate is on %s; move it to a HIP device (there is no CPU path)" % dev)
        return MFNStream(self, batch)

    def slot_stream(self, batch, limit=None, positions=None):
        """``stream(batch)`` with slots (``MFNSlotStream``): the position of every sequence lives on the device, so the sequences are
        seated and released independently and a step can be captured into a graph (``graphs.capture_stream``).  ``limit``: windows per
        recording after which a slot is full (None: none, a gate has no cache).  The same refusals, before any launch."""
        return MFNSlotStream(self.stream(batch), limit, positions)


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
        self.mfn, self.batch = mfn, int(batch)
        if not self.slots:
            self.t = 0
        self.mods = list(mfn.mods)
        self.in_dims = [mfn.lstm[m].input_size for m in self.mods]
        self.hidden = [mfn.lstm[m].hidden_size for m in self.mods]
        self.output_dim = mfn.out_fc2.out_features
        self.device = mfn.out_fc2.weight.device
        if self.batch < 1:
            raise ValueError("MFN.stream: batch must be at least 1, got %d" % self.batch)
        self.state = F_hip.mfn_stream_state(self.batch, self.in_dims, self.hidden, self.output_dim, self.device)   # ValueError naming the limit
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


class MFNSlotStream(_Slots, MFNStream):
    """``MFNStream`` with slots (``MFN.slot_stream``; members: ``_Slots``, ``capacity`` is the ``limit``).  ``step(inputs, mask_t)`` is
    ONE launch of mfn_step_slots_kernel: row b is what an ``MFNStream`` of that recording alone gives at window ``positions[b]``, bit
    for bit (copy ``positions[b] & 1`` of the carried state is read and the other written, per sequence), and the kernel advances the
    positions of the slots it ran."""

    def __init__(self, opened, limit=None, positions=None):
        self.__dict__.update({k: v for k, v in opened.__dict__.items() if k != "t"})     # the state of the stream just opened
        self.capacity = None if limit is None else int(limit)
        if self.capacity is not None and self.capacity < 1:
            raise ValueError("MFN.slot_stream: limit must be at least 1 (or None), got %d" % self.capacity)
        self.positions = _slot_positions("MFN.slot_stream", positions, self.batch, self.device)

    def step(self, inputs, mask_t=None, advance=True):
        xs = _modality_rows("MFNStream.step", inputs, self.mods, self.in_dims, self.batch, self.device, mask_t)
        return F_hip.mfn_stream_step_slots(xs, mask_t, self.state, self.positions, self.in_dims, self.hidden, self.output_dim,
                                           limit=self.capacity, advance=advance)


def _modality_rows(op, inputs, mods, widths, B, device, mask_t):
    """The checks of a per-modality step, all before any launch -> the rows in the order of ``mods``."""
    if not isinstance(inputs, dict) or any(m not in inputs for m in mods):
        raise ValueError("%s: inputs must be a dict with a row for every modality %s, got %s"
                         % (op, mods, sorted(inputs) if isinstance(inputs, dict) else type(inputs).__name__))
    for m, d in zip(mods, widths):
        x = inputs[m]
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != device:
            raise ValueError("%s: inputs[%r] must be a float32 tensor on %s, got %s on %s"
                             % (op, m, device, getattr(x, "dtype", type(x).__name__), getattr(x, "device", None)))
        if tuple(x.shape) != (B, d):
            raise ValueError("%s: inputs[%r] must have the shape (%d,%d), got %s" % (op, m, B, d, tuple(x.shape)))
    if mask_t is not None and (not isinstance(mask_t, torch.Tensor) or mask_t.numel() != B or mask_t.device != device):
        raise ValueError("%s: mask_t must hold one entry per sequence (%d) on %s" % (op, B, device))
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
        _stream_model_checks(model)
        self.model, self.batch = model, int(batch)
        self.mods = list(model.mods)
        self.widths = [model.embed[m].in_features for m in self.mods]
        stacks = getattr(model, "transformer", None)
        if stacks is not None and capacity is None:
            raise ValueError("%s.stream: the encoders' K/V cache needs a capacity (windows per recording)" % type(model).__name__)
        self.encs = None if stacks is None else {m: stacks[m].stream(batch, capacity) for m in self.mods}      # their refusals pass through
        self.gate = model.mfn.stream(batch)
        self.device = self.gate.device
        self.modality_streams = self.encs is not None
        if self.slots:
            # ONE positions tensor: the encoders read it (advance off, on the modality streams as before), the gate's launch, which runs
            # behind the join, advances it.  The gate's limit is the encoders' capacity, so a full slot is skipped by every launch.
            self.positions = _slot_positions("%s.slot_stream" % type(model).__name__, None, self.batch, self.device)
            if self.encs is not None:
                self.encs = {m: EncoderSlotStream(e, self.positions) for m, e in self.encs.items()}
            self.gate = MFNSlotStream(self.gate, self.capacity, self.positions)

    t = property(lambda self: self.gate.t)
    capacity = property(lambda self: None if self.encs is None else self.encs[self.mods[0]].capacity)

    def reset(self):
        self.gate.reset()
        for e in (self.encs or {}).values():
            e.reset()                # a slots stream: the one shared tensor, zeroed again (idempotent)

    def refresh(self):
        self.gate.refresh()
        for e in (self.encs or {}).values():
            e.refresh()

    def step(self, inputs, mask_t=None):
        m, B = self.model, self.batch
        op = "%s stream step" % type(m).__name__
        xs = _modality_rows(op, inputs, self.mods, self.widths, B, self.device, mask_t)
        if not self.slots and self.encs is not None and self.t >= self.capacity:
            raise ValueError("%s: the stream is full (t = capacity = %d)" % (op, self.capacity))
        with torch.no_grad():
            r = None if mask_t is None else mask_t.float().reshape(B)
            rows = {}
            fork = self.modality_streams and len(self.mods) > 1
            main, streams = _MOD_STREAMS.begin(self.device, len(self.mods)) if fork else (None, [None] * len(self.mods))
            for mod, x, st in zip(self.mods, xs, streams):
                with torch.cuda.stream(st):                                # None: the caller's stream
                    e = _SequenceStream._affine(x, m.embed[mod])
                    if self.encs is None:
                        rows[mod] = e
                    elif self.slots:
                        rows[mod] = self.encs[mod].step(e, r, advance=False)
                    else:
                        rows[mod] = self.encs[mod].step(e, r)
            if fork:
                _MOD_STREAMS.end(main, streams, list(rows.values()))
            return self.gate.step(rows, r, advance=self._advance) if self.slots else self.gate.step(rows, r)


class _GateSlotStream(_Slots, _GateStream):
    """``slot_stream()`` of MultiTransformer and MultiTransformerB3: ``_GateStream`` with slots (members: ``_Slots``).  It owns ONE
    ``positions`` tensor, which its encoder streams and its gate share: the encoders' launches read it, the gate's launch, the last of
    the step, advances it.  A step launches what the ``_GateStream`` step launches, with the positioned kernels in place of the two step
    kernels, and row b is what a ``_GateStream`` of that recording alone gives at window ``positions[b]``."""

    _advance = True

    def reset(self):
        _Slots.reset(self)

    def step(self, inputs, mask_t=None, advance=True):
        """As ``_GateStream.step``.  ``advance=False``: the gate's launch leaves the positions, so the same windows can be stepped again
        (a measurement at a fixed position; a recording advances)."""
        self._advance = bool(advance)
        try:
            return _GateStream.step(self, inputs, mask_t)
        finally:
            self._advance = True


class MultiTransformer(nn.Module):
    """MFT sequence model (transformer/MFT/multiTransformer.py:250-313): per-modality Linear embed ->
    own Encoder stack -> MFN gate -> mask.  ``attn{mod}`` / ``ff{mod}`` are registered as in the reference
    (:273-276) although only deep copies of them are used (:277): they are dead parameters kept so that
    reference checkpoints load with identical keys."""

    def __init__(self, mods, window_embed_size, N=6, d_ff=128, h=8, dropout=0.1, n_layers=1, device=torch.device("cuda:0"),
                 embed_dim=None):
        super().__init__()
        self.mods = list(mods)
        self.window_embed_size = window_embed_size
        self.embed_dim = embed_dim or {"linguistic": 256, "emotient": 16, "acoustic": 256, "image": 256}
        self.embed, self.transformer, self.attn, self.ff = {}, {}, {}, {}
        for mod in self.mods:
            e = self.embed_dim[mod]
            self.embed[mod] = nn.Linear(window_embed_size[mod], e)
            self.add_module("embed_%s" % mod, self.embed[mod])
            self.attn[mod] = MultiHeadedAttention(h, e)
            self.ff[mod] = PositionwiseFeedForward(e, d_ff, dropout)
            self.add_module("attn%s" % mod, self.attn[mod])
            self.add_module("ff%s" % mod, self.ff[mod])
            self.transformer[mod] = Encoder(EncoderLayer(e, copy.deepcopy(self.attn[mod]), copy.deepcopy(self.ff[mod]), dropout), N)
            self.add_module("transformer_%s" % mod, self.transformer[mod])
        self.mfn = MFN(self.mods, self.embed_dim, 1, device=device)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, mask, lengths, tgt_init=0.5, target=None):
        gate_in = {}
        main, streams = _MOD_STREAMS.begin(self.device, len(self.mods))
        for mod, st in zip(self.mods, streams):
            with torch.cuda.stream(st):
                e = F_hip.linear(inputs[mod], self.embed[mod].weight, self.embed[mod].bias)
                e = self.transformer[mod](e, mask)
                gate_in[mod] = F_hip.time_major(e)                    # (T,B,d): the reference's permute(1,0,2), :300
        _MOD_STREAMS.end(main, streams, list(gate_in.values()))
        return self.mfn._gate(gate_in, mask)                         # ... * mask (:310) in the gate's last pass

    def stream(self, batch, capacity):
        """The MFT as an online predictor: ``.step({mod: (B, window_embed_size[mod])}, mask_t)`` -> the (B,1) prediction of window t
        (``_GateStream``).  Eval mode, ``causal_attention(model)`` on; the encoders' own refusals pass through, before any launch."""
        return _GateStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """``stream(batch, capacity)`` with slots (``_GateSlotStream``): sequences are seated and released independently, and a step can
        be captured into a graph (``graphs.capture_stream``).  The same refusals, before any launch."""
        return _GateSlotStream(self, batch, capacity)


class MultiTransformerB3(nn.Module):
    """B3-MFN sequence model (transformer/B3-MFN/multiTransformer.py:250-307): the MFT model without its encoder stacks — per-modality
    Linear embed -> MFN gate -> mask.  Keys ``embed_{mod}.*`` and ``mfn.*`` only."""

    def __init__(self, mods, window_embed_size, N=6, d_ff=128, h=8, dropout=0.1, n_layers=1, device=torch.device("cuda:0")):
        super().__init__()
        self.mods = list(mods)
        self.window_embed_size = window_embed_size
        self.embed_dim = {"linguistic": 256, "emotient": 16, "acoustic": 256, "image": 256}
        self.embed = {}
        for mod in self.mods:
            self.embed[mod] = nn.Linear(window_embed_size[mod], self.embed_dim[mod])
            self.add_module("embed_%s" % mod, self.embed[mod])
        self.mfn = MFN(self.mods, self.embed_dim, 1, device=device)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, mask, lengths, tgt_init=0.5, target=None):
        gate_in = {}
        main, streams = _MOD_STREAMS.begin(self.device, len(self.mods))
        for mod, st in zip(self.mods, streams):
            with torch.cuda.stream(st):
                e = F_hip.linear(inputs[mod], self.embed[mod].weight, self.embed[mod].bias)
                gate_in[mod] = F_hip.time_major(e)                    # the reference's permute(1,0,2), :294
        _MOD_STREAMS.end(main, streams, list(gate_in.values()))
        return self.mfn._gate(gate_in, mask)                         # ... * mask (:304) in the gate's last pass

    def stream(self, batch, capacity=None):
        """B3-MFN as an online predictor: ``.step({mod: (B, window_embed_size[mod])}, mask_t)`` -> the (B,1) prediction of window t
        (``_GateStream``).  Eval mode.  No attention, so no cache: ``capacity`` is accepted and ignored, a recording has no length
        limit, and ``causal_attention`` is not needed."""
        return _GateStream(self, batch, capacity)

    def slot_stream(self, batch, capacity=None):
        """``stream(batch)`` with slots (``_GateSlotStream``); ``capacity`` is accepted and ignored, a slot is never full."""
        return _GateSlotStream(self, batch, None)


class _DeviceStreamMixin:
    """``device_stream`` of UniTransformer, UniFullTransformer and NLPTransformer."""

    def device_stream(self, batch, capacity):
        """This model as an online predictor whose whole per-recording state lives on the device (``_SequenceSlotStream``): sequences
        are seated and released independently (``.positions``, ``.seat``, ``.release``, ``.full``), a step is three launches and can be
        captured into a graph (``graphs.capture_stream``).  Eval mode, ``causal_attention(model)`` on, a decoder of at most 4 layers;
        ValueError before any launch."""
        return _SequenceSlotStream(self, batch, capacity)


class _DecoderMixin:
    """Autoregressive LSTM decoder + MLP shared by UniTransformer and NLPTransformer
    (transformer/SFT/multiTransformer.py:463-483).  One layer: step t feeds [o_{t-1}; enc_t] with o = h, so
        gates_t = enc_t W_ih[:, d:]^T + b  +  h_{t-1} (W_ih[:, :d] + W_hh)^T          for t >= 1
        gates_0 = enc_0 W_ih[:, d:]^T + b  +  h0 W_hh^T                               (o_{-1} = 0, h_{-1} = dec_h0)
    i.e. one batched input projection plus one LSTM scan with W_rec = W_ih[:, :d] + W_hh.  More layers: _decode_stacked."""

    def _decode(self, enc, mask):
        B, T, d = enc.shape
        if self.decoder.num_layers != 1:
            return self._decode_stacked(enc, mask)
        Wx, W_rec, Whh, bias = F_hip.decoder_pack(self.decoder.weight_ih_l0, self.decoder.weight_hh_l0,
                                                  self.decoder.bias_ih_l0, self.decoder.bias_hh_l0)
        gx = F_hip.linear(F_hip.time_major(enc), Wx, bias)                                  # (T,B,4d)
        gx = F_hip.add_row0(gx, F_hip.linear(self.dec_h0, Whh))                             # step 0 sees h0 W_hh^T (in place, no concat)
        h_all, _ = F_hip.lstm_scan(gx, W_rec, None, F_hip.broadcast_rows(self.dec_c0, B))
        hid = F_hip.linear(h_all, self.out[0].weight, self.out[0].bias, act=1)              # rows stay time-major ...
        return F_hip.batch_major(F_hip.linear(hid, self.out[2].weight, self.out[2].bias), mask)   # ... until the mask pass


    def _decode_stacked(self, enc, mask):
        """n_layers = L > 1: o is the TOP layer's output and every layer has its own state, so the layers are coupled inside each step
        (functional.lstm_stack_scan, csrc/scan_stack.h):
            gates^0_t = enc_t W_ih_l0[:, d:]^T + b_0  +  [o_{t-1} ; h^0_{t-1}] [W_ih_l0[:, :d] | W_hh_l0]^T         o_{-1} = 0
            gates^l_t = b_l  +  [h^{l-1}_t ; h^l_{t-1}] [W_ih_l | W_hh_l]^T                                          h^l_{-1} = dec_h0[l]
        The enc term is one batched projection as above.  2 <= L <= 4, embed_dim % 4 == 0 and <= 128, batch <= 512."""
        B, T, d = enc.shape
        L = self.decoder.num_layers
        if not 2 <= L <= 4 or d % 4 or d > 128 or B > 512:
            raise NotImplementedError("%s: a decoder with n_layers > 1 runs on the stacked scan, which takes 2 <= n_layers <= 4, embed_dim a "
                                      "multiple of 4 up to 128 and batches up to 512 (got n_layers=%d, embed_dim=%d, batch=%d)"
                                      % (type(self).__name__, L, d, B))
        Wx, bias0, P, bias = F_hip.decoder_stack_pack(self.decoder)
        gx = F_hip.linear(F_hip.time_major(enc), Wx, bias0)                                 # (T,B,4d)
        h_top = F_hip.lstm_stack_scan(gx, P, bias, F_hip.broadcast_layers(self.dec_h0, B), F_hip.broadcast_layers(self.dec_c0, B))
        hid = F_hip.linear(h_top, self.out[0].weight, self.out[0].bias, act=1)
        return F_hip.batch_major(F_hip.linear(hid, self.out[2].weight, self.out[2].bias), mask)


class UniTransformer(nn.Module, _DecoderMixin, _DeviceStreamMixin):
    """Single-modality model (transformer/MFT/multiTransformer.py:315-376): Linear embed -> Encoder -> LSTM decoder -> MLP."""

    def __init__(self, window_embed_size, embed_dim=256, h_dim=128, N=6, d_ff=128, h=8, dropout=0.1, n_layers=1,
                 device=torch.device("cuda:0")):
        super().__init__()
        self.embed_dim, self.h_dim = embed_dim, h_dim
        self.embed = nn.Linear(window_embed_size, embed_dim)
        self.encoder = _encoder(embed_dim, h, d_ff, dropout, N)
        self.decoder = nn.LSTM(2 * embed_dim, embed_dim, n_layers, batch_first=True)
        self.dec_h0 = nn.Parameter(torch.zeros(n_layers, 1, embed_dim))
        self.dec_c0 = nn.Parameter(torch.zeros(n_layers, 1, embed_dim))
        self.out = nn.Sequential(nn.Linear(embed_dim, h_dim), nn.ReLU(), nn.Linear(h_dim, 1))
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, mask, lengths, tgt_init=0.5, target=None):
        e = F_hip.linear(inputs, self.embed.weight, self.embed.bias)
        return self._decode(self.encoder(e, mask), mask)

    def stream(self, batch, capacity):
        """This model as an online predictor: ``.step(x_t (B, window_embed_size), mask_t)`` -> the (B,1) prediction of window t
        (``_SequenceStream``).  Eval mode, ``causal_attention(model)`` on; ValueError / NotImplementedError before any launch."""
        return _SequenceStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """Not implemented for this model (``_no_slot_stream`` says why): ``device_stream`` is the stream with slots."""
        _no_slot_stream(self)


class UniFullTransformer(nn.Module, _DeviceStreamMixin):
    """B2-Trans model (transformer/B2-Trans/multiTransformer.py:378-420): Linear embed -> Encoder -> MLP -> mask."""

    def __init__(self, window_embed_size, embed_dim=256, h_dim=128, N=6, d_ff=128, h=8, dropout=0.1, n_layers=1,
                 device=torch.device("cuda:0")):
        super().__init__()
        self.embed_dim, self.h_dim = embed_dim, h_dim
        self.embed = nn.Linear(window_embed_size, embed_dim)
        self.encoder = _encoder(embed_dim, h, d_ff, dropout, N)
        self.out = nn.Sequential(nn.Linear(embed_dim, h_dim), nn.ReLU(), nn.Linear(h_dim, 1))
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, mask, lengths, tgt_init=0.5, target=None):
        enc = self.encoder(F_hip.linear(inputs, self.embed.weight, self.embed.bias), mask)
        hid = F_hip.linear(enc, self.out[0].weight, self.out[0].bias, act=1)
        return F_hip.linear(hid, self.out[2].weight, self.out[2].bias, rowscale=mask.float().reshape(-1))

    def stream(self, batch, capacity):
        """This model as an online predictor: ``.step(x_t (B, window_embed_size), mask_t)`` -> the (B,1) prediction of window t
        (``_SequenceStream``).  Eval mode, ``causal_attention(model)`` on; ValueError / NotImplementedError before any launch."""
        return _SequenceStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """Not implemented for this model (``_no_slot_stream`` says why): ``device_stream`` is the stream with slots."""
        _no_slot_stream(self)


class NLPTransformer(nn.Module, _DecoderMixin, _DeviceStreamMixin):
    """SFT model (transformer/SFT/multiTransformer.py:422-484): Dropout(0.1) -> Linear -> ReLU embed,
    Encoder, LSTM decoder, MLP, mask."""

    def __init__(self, window_embed_size, embed_dim=256, h_dim=128, N=6, d_ff=128, h=8, dropout=0.1, n_layers=1,
                 device=torch.device("cuda:0")):
        super().__init__()
        self.embed_dim, self.h_dim = embed_dim, h_dim
        self.embed = nn.Sequential(nn.Dropout(0.1), nn.Linear(window_embed_size, embed_dim), nn.ReLU())
        self.encoder = _encoder(embed_dim, h, d_ff, dropout, N)
        self.decoder = nn.LSTM(2 * embed_dim, embed_dim, n_layers, batch_first=True)
        self.dec_h0 = nn.Parameter(torch.zeros(n_layers, 1, embed_dim))
        self.dec_c0 = nn.Parameter(torch.zeros(n_layers, 1, embed_dim))
        self.out = nn.Sequential(nn.Linear(embed_dim, h_dim), nn.ReLU(), nn.Linear(h_dim, 1))
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, mask, lengths, tgt_init=0.5, target=None):
        p_in = float(self.embed[0].p) if self.training else 0.0      # Dropout(0.1) on the input rides in the embed kernel's A-tile staging
        seed = _lib.next_dropout_seed(inputs.device, 5, holder=self) if p_in > 0.0 else 0
        e = F_hip.linear(inputs, self.embed[1].weight, self.embed[1].bias, act=1, in_dropout=p_in, seed=seed)
        return self._decode(self.encoder(e, mask), mask)

    def stream(self, batch, capacity):
        """This model as an online predictor: ``.step(x_t (B, window_embed_size), mask_t)`` -> the (B,1) prediction of window t
        (``_SequenceStream``).  Eval mode, ``causal_attention(model)`` on; ValueError / NotImplementedError before any launch."""
        return _SequenceStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """Not implemented for this model (``_no_slot_stream`` says why): ``device_stream`` is the stream with slots."""
        _no_slot_stream(self)
