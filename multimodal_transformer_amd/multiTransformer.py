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
  * ``causal_attention(model, span=W)`` / ``MultiHeadedAttention.span = W`` (None by default, needs ``causal``): window t attends its
    last W windows only, t - W + 1 .. t (banded / sliding-window causal attention; the ``*_band_kernel`` entries of csrc/attn.h).
  * train-mode dropout draws from a counter-based generator inside the kernels, not from torch's
    global generator: training-mode parity with the reference is statistical, eval-mode is numerical.
"""
import copy
import os

import torch
import torch.nn as nn

from . import _lib
from . import functional as F_hip
from .functional import _MOD_STREAMS            # the one object, shared with streaming; models imports it from here
# the models as online predictors: what stream() / slot_stream() / device_stream() below open
from .streaming import (_INT_MAX, EncoderRingSlotStream, EncoderRingStream, EncoderSlotStream, EncoderStream, MFNSlotStream, MFNStream,
                        _GateSlotStream, _GateStream, _modality_rows, _no_slot_stream, _SequenceSlotStream, _SequenceStream,
                        _slot_positions, _Slots, _stream_model_checks, ring_stream)


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
    window t < len sees keys <= t < len only, so causal attention already keeps it from the padding behind its sequence.

    ``span`` (a class attribute, None; ``causal_attention(model, span=W)`` sets it per instance): with ``causal``, window t attends
    its last ``span`` windows only, t - span + 1 .. t, its own included — a fixed receptive field per layer.  ``keep_attn`` then
    shows the zeros on both sides of the band.  ValueError at the call without ``causal``, with ``mask_keys``, for span < 1 and
    for a bool or a non-integer."""

    keep_attn = False
    mask_keys = False
    causal = False
    span = None

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

    def attention_span(self):
        """``span`` of this layer, None or an int >= 1, checked against (mask_keys, causal): ValueError, before any launch, otherwise."""
        mask_keys, causal = self.attention_mode()
        return F_hip._check_span("MultiHeadedAttention", None, causal, self.span, mask_keys=mask_keys)

    def forward(self, query, key, value, mask=None):
        mask_keys, causal = self.attention_mode()
        span = self.attention_span()
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
        ctx = F_hip.sdpa(q, k, v, m, self.h, dropout_p=p, seed=seed, key_lengths=kl, causal=causal, span=span)
        self.attn = (F_hip.attn_probs(q, k, m, self.h, dropout_p=p, seed=seed, key_lengths=kl, causal=causal, span=span)
                     if self.keep_attn else None)
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


def causal_attention(module, on=True, span=None):
    """Set ``causal`` and ``span`` on every MultiHeadedAttention below ``module`` (the SFT / MFT / B2 models, every modality's stack of
    MultiTransformer, the MultiCNNTransformer wrappers) -> {qualified name: module}.  From the next forward on window t attends
    windows 0 .. t of its sequence only, in every layer, forward and backward: every other part of these models already runs forward in
    time (window encoder, LayerNorm, FFN and residuals are per window), so the model's output at window t no longer depends on later
    windows.

    An Encoder keeps running as the fused stack; only layers that disagree about the flag make it run layer by layer.  Outputs then
    differ from the reference's, whose windows attend the whole recording — by design.  Not combined with ``mask_padded_keys`` (the
    next forward raises ValueError; causal attention already keeps a valid window from its batch's padding).
    ``span`` (an int >= 1; None: no lower edge): window t attends its last ``span`` windows only, t - span + 1 .. t, so every layer has
    a fixed receptive field and the model conditions on a context of bounded length, in training and in evaluation; the band kernels
    also sweep about span/32 + 1 key tiles per query tile instead of all tiles up to the diagonal.  ValueError here for span < 1, a
    bool or a non-integer, and for a span with ``on=False``.  A span streams through ``ring_stream(model, batch)`` (``stream`` refuses it at open).
    ``causal_attention(module, False)`` restores the reference's semantics and the plain kernels, and clears ``span``."""
    span = F_hip._check_span("causal_attention", None, bool(on), span)
    found = {}
    for name, m in module.named_modules():
        if isinstance(m, MultiHeadedAttention):
            m.causal = bool(on)
            m.span = span
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
        if any(l.self_attn.span != l0.self_attn.span for l in self.layers):                # with one span
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
        span = l0.self_attn.attention_span()
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
                                          causal=causal, span=span)

    def _stream_refusals(self, ring=False):
        """What ``stream`` and ``slot_stream`` refuse, before anything is allocated or launched.  ``ring`` (``ring_stream``,
        ``ring_slot_stream``): the same, but the span must be there."""
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
        if ring and l0.span is None:
            raise ValueError("%s.ring_stream: the layers have no span, so a window attends its whole past and no ring of rows can hold "
                             "it: call causal_attention(model, span=W) (and train the model that way), or open stream(batch, capacity)" % name)
        if not ring and l0.span is not None:
            raise ValueError("%s.stream: the layers attend a band of span = %r windows, but this step kernel attends every cached key "
                             "and would be wrong from window t = span on; a span streams from a ring cache of span rows, which never "
                             "fills: Encoder.ring_stream(batch) / ring_stream(model, batch) (DESIGN.md 4.11)" % (name, l0.span))
        if self.norm.a_2.device.type != "cuda":
            raise ValueError("%s.stream: the encoder is on %s; move it to a HIP device (there is no CPU path)" % (name, self.norm.a_2.device))

    def stream(self, batch, capacity):
        """Open an ``EncoderStream``: this stack as an online predictor for ``batch`` recordings of up to ``capacity`` windows, one
        window per ``step`` against a K/V cache instead of a forward over the whole prefix.  Eval mode, forward only; every layer must
        attend causally (``causal_attention(model)``).  Raises ValueError, before any launch, for anything else."""
        self._stream_refusals()
        return EncoderStream(self, batch, capacity)

    def slot_stream(self, batch, capacity, positions=None):
        """``stream(batch, capacity)`` with slots (``EncoderSlotStream``): the position of every sequence lives on the device, so the
        sequences are seated and released independently and a step can be captured into a graph (``graphs.capture_stream``).  The same
        refusals, before any launch."""
        self._stream_refusals()
        return EncoderSlotStream(self, batch, capacity, positions)

    def ring_stream(self, batch):
        """Open an ``EncoderRingStream``: this stack, with a span (``causal_attention(model, span=W)``), as an online predictor for
        ``batch`` recordings of ANY length, one window per ``step`` against a ring K/V cache of ``span`` rows.  The
        refusals of ``stream``, and ValueError for a stack without a span, before any launch."""
        self._stream_refusals(ring=True)
        return EncoderRingStream(self, batch)

    def ring_slot_stream(self, batch, positions=None):
        """``ring_stream(batch)`` with slots (``EncoderRingSlotStream``): positions on the device, independent seats, a step that can
        be captured into a graph, and no slot ever full.  The same refusals, before any launch."""
        self._stream_refusals(ring=True)
        return EncoderRingSlotStream(self, batch, positions)

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


def _encoder(embed_dim, h, d_ff, dropout, N):
    return Encoder(EncoderLayer(embed_dim, MultiHeadedAttention(h, embed_dim), PositionwiseFeedForward(embed_dim, d_ff, dropout),
                                dropout), N)


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

    def _stream_refusals(self):
        """What ``stream`` and ``slot_stream`` refuse, before anything is allocated or launched."""
        if self.training:
            raise ValueError("MFN.stream: the gate is in train mode; streaming is eval-mode inference (call .eval())")
        dev = self.out_fc2.weight.device
        if dev.type != "cuda":
            raise ValueError("MFN.stream: the gate is on %s; move it to a HIP device (there is no CPU path)" % dev)

    def stream(self, batch):
        """Open an ``MFNStream``: this gate as an online predictor for ``batch`` recordings, one window per ``step`` with the carried
        (h, c, mem) instead of a forward over the whole prefix.  Eval mode, forward only; no attention, so no length limit.  Raises
        ValueError, before any launch, for anything else."""
        self._stream_refusals()
        return MFNStream(self, batch)

    def slot_stream(self, batch, limit=None, positions=None):
        """``stream(batch)`` with slots (``MFNSlotStream``): the position of every sequence lives on the device, so the sequences are
        seated and released independently and a step can be captured into a graph (``graphs.capture_stream``).  ``limit``: windows per
        recording after which a slot is full (None: none, a gate has no cache).  The same refusals, before any launch."""
        self._stream_refusals()
        return MFNSlotStream(self, batch, limit, positions)


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

    def _decode(self, enc, mask, _state=None):
        """``_state`` (internal; a list): the one-layer scan's (h_all, c_all), (T, B, d) each, are appended to it (a stream's prefill
        keeps the last row as its carried state).  What is returned does not change."""
        B, T, d = enc.shape
        if self.decoder.num_layers != 1:
            return self._decode_stacked(enc, mask)
        # a prefill is inference: detached views, or an autograd node that sees a tensor requiring grad keeps its pool workspace for a
        # backward that never comes (streaming._SequenceStream._affine says the same of a step)
        p = (lambda q: q.detach()) if _state is not None else (lambda q: q)
        dec, out = self.decoder, self.out
        Wx, W_rec, Whh, bias = F_hip.decoder_pack(p(dec.weight_ih_l0), p(dec.weight_hh_l0), p(dec.bias_ih_l0), p(dec.bias_hh_l0))
        gx = F_hip.linear(F_hip.time_major(enc), Wx, bias)                                  # (T,B,4d)
        gx = F_hip.add_row0(gx, F_hip.linear(p(self.dec_h0), Whh))                          # step 0 sees h0 W_hh^T (in place, no concat)
        h_all, c_all = F_hip.lstm_scan(gx, W_rec, None, F_hip.broadcast_rows(p(self.dec_c0), B))
        if _state is not None:
            _state.append((h_all, c_all))
        hid = F_hip.linear(h_all, p(out[0].weight), p(out[0].bias), act=1)                  # rows stay time-major ...
        return F_hip.batch_major(F_hip.linear(hid, p(out[2].weight), p(out[2].bias)), mask)   # ... until the mask pass


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
