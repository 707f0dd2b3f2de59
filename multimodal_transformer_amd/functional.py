"""torch.autograd bindings of the HIP entry points (include/mmt_hip.h).

Each Function is the forward/backward pair of one reference class:
  encoder_stack  <- Encoder.forward                  transformer/MFT/multiTransformer.py:73-76
  layer_norm     <- LayerNorm.forward                :88-91
  sdpa           <- attention()                      :22-34
  attn_probs     <- p_attn / MultiHeadedAttention.attn :22-34,59
  linear         <- nn.Linear (+ReLU) call sites     :15-20,43,55,65
  local_attention <- softmax(dim=1) + convolve of the LSTM baselines   transformer/B1-LSTM/models.py:10-25,186-207
  ar_combine     <- the autoregressive read-out of MultiARLSTM        transformer/MFT/models.py:381-399
All tensors must live on a HIP device; there is no CPU path.  Every C call goes through ``_lib.launch``.
"""
import ctypes
import math

import torch

from . import _lib


def _f32c(t):
    return t.detach().contiguous().float() if t is not None else None


def _f32c16(t):
    """contiguous fp32 AND 16-byte aligned (a contiguous view at an odd storage offset is not): for the arguments that an entry's kernels
    move four floats per lane (include/mmt_hip.h, pointer contract, class (c): the entry refuses any other address).  An aligned
    argument is passed as it is: no copy, no launch."""
    t = _f32c(t)
    return t.clone() if t is not None and t.data_ptr() % 16 else t


# Dropout seeds: a python int (by value) or a ``_lib.DeviceSeed`` (device-resident: fresh masks at every hipGraph replay).
def _seed_arg(seed):
    """The one normalisation of a seed argument: a DeviceSeed stays one, anything else becomes a python int (a list: item by item)."""
    if isinstance(seed, (list, tuple)):
        return [_seed_arg(v) for v in seed]
    return seed if isinstance(seed, _lib.DeviceSeed) else int(seed)


def _seed_pair(seed):
    """(value, state word) of the entry points that take a seed either way: (seed, None) by value, (0, state) for a DeviceSeed."""
    return (0, seed.state) if isinstance(seed, _lib.DeviceSeed) else (int(seed), None)


def _launch_seeded(name, seed, *args, state_arg=True, key_lengths=None, causal=False, span=None):
    """``name`` with the seed by value behind ``args``, or its twin ``name``_devseed with the DeviceSeed's state word there, which the
    launch reads and advances.  ``state_arg=False``: the twin takes no seed (the encoder backward finds it in its forward's workspace).
    ``key_lengths`` / ``causal`` / ``span``: the ``_keys`` / ``_causal`` / ``_band`` form of either (_lib.launch)."""
    devseed = isinstance(seed, _lib.DeviceSeed)
    tail = (seed,) if not devseed else (seed.state,) if state_arg else ()
    _lib.launch(name, *args, *tail, key_lengths=key_lengths, causal=causal, devseed=devseed, span=span)


# Key lengths: a padding mask that masks KEYS (opt-in; the reference blanks query rows only, transformer/MFT/multiTransformer.py:29-31).
def key_lengths(mask):
    """(B,T,1) or (B,T) mask -> int32 (B,) on the mask's device: ``1 +`` the index of the last non-zero entry of each row, 1 for an
    all-zero row.  For the prefix masks that padding produces this is the sequence length.  Holes INSIDE the prefix stay attended as
    keys (their query rows are still blanked by the mask itself).  One kernel launch, no host synchronisation: safe under hipGraph capture."""
    _lib.require_hip(mask)
    _lib.load()
    m_ = _f32c(mask)
    if m_.dim() < 2 or m_.numel() == 0 or m_.numel() != m_.shape[0] * max(m_.shape[1:]):
        raise ValueError("key_lengths: mask must have the shape (B,T,1), (B,1,T,1) or (B,T), got %s" % (tuple(mask.shape),))
    m_ = m_.view(m_.shape[0], -1)
    B, T = m_.shape
    out = torch.empty(B, dtype=torch.int32, device=m_.device)
    _lib.launch("mmt_key_lengths", m_, out, B, T)
    return out


def _check_key_lengths(op, key_lengths, B, device):
    """A ``key_lengths`` argument is None or a contiguous int32 (B,) tensor on ``device``: anything else raises before any launch."""
    if key_lengths is None:
        return None
    if not isinstance(key_lengths, torch.Tensor) or key_lengths.dtype != torch.int32:
        raise ValueError("%s: key_lengths must be an int32 tensor (functional.key_lengths(mask)), got %s"
                         % (op, getattr(key_lengths, "dtype", type(key_lengths).__name__)))
    if tuple(key_lengths.shape) != (B,):
        raise ValueError("%s: key_lengths must have the shape (B,) = (%d,), got %s" % (op, B, tuple(key_lengths.shape)))
    if key_lengths.device != device:
        raise ValueError("%s: key_lengths is on %s, the operands on %s" % (op, key_lengths.device, device))
    return key_lengths.detach().contiguous()


# Causal self-attention (opt-in; the reference lets window t attend every window of its batch row, transformer/MFT/multiTransformer.py:27-31).
def _check_causal(op, key_lengths, causal):
    """``causal`` as a bool.  It is never combined with ``key_lengths``: raises before any launch."""
    if causal and key_lengths is not None:
        raise ValueError("%s: key_lengths and causal=True cannot be combined: a valid window t < len of a prefix-masked batch sees keys "
                         "<= t < len only, so causal attention already keeps it from the padding behind its sequence "
                         "(pass causal=True alone)" % op)
    return bool(causal)


# Banded causal self-attention (opt-in): window t attends windows max(0, t - span + 1) .. t.
def _check_span(op, key_lengths, causal, span, mask_keys=False):
    """``span`` as None or an int >= 1.  It needs ``causal`` and is never combined with ``key_lengths`` (or, on a module, with
    ``mask_keys``, which derives them): raises before any launch."""
    if span is None:
        return None
    if isinstance(span, bool) or not isinstance(span, int):
        raise ValueError("%s: span must be an int >= 1 (the number of windows a query attends, its own included) or None, got %r"
                         % (op, span))
    if span < 1:
        raise ValueError("%s: span = %d, but a query attends at least its own window: span must be >= 1" % (op, span))
    if key_lengths is not None or mask_keys:
        raise ValueError("%s: key_lengths and span cannot be combined: span needs causal=True, and causal attention already keeps a "
                         "valid window t < len of a prefix-masked batch from the padding behind its sequence" % op)
    if not causal:
        raise ValueError("%s: span = %d without causal=True: the span is the lower edge of causal attention (window t attends "
                         "windows t - span + 1 .. t); pass causal=True with it" % (op, span))
    return span


# Workspaces of the entries that take memory with any contents (include/mmt_hip.h: mmt_lstm_scan_*, mmt_mfn_mem_scan_*, mmt_convpool_*,
# mmt_convpool_k_*): every word their kernels read is written first by a kernel of the same call, so they come from the caching
# allocator as they are, neither pooled nor cleared.  One function, so that a test can hand those entries memory it has filled.
def _scratch(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# Pool workspaces held from forward to backward (_lib.WorkspacePool): the Functions that keep one use these two.
def _hold(ctx, *ws):
    """Forward: keep the workspaces for the backward if an input needs a gradient (-> True), else hand them back to the pool at once."""
    if any(ctx.needs_input_grad):
        ctx.ws = ws
        return True
    for w in ws:
        _lib.POOL.put(w)
    return False


def _take_ws(ctx, op):
    """Backward: the workspaces the forward kept, exactly once; a second backward of the same forward raises before any launch."""
    ws, ctx.ws = getattr(ctx, "ws", None), None
    if ws is None:
        raise RuntimeError("%s: backward called twice on the same forward (its workspace went back to the pool)" % op)
    return ws


# Sub-batch streams.  Sequences are independent, so one stack call may run as k sub-batches on k HIP streams (forked and joined by event,
# inside one hipGraph too).  Every kernel of a stack launches all its workgroups in ONE round at the BASELINE sizes, i.e. a step is a
# chain of ~34 kernel latencies; with two half-batches in flight the attention kernels (bound by vector issue) of one run beside the row
# chains (bound by latency) of the other, and one half's tail overlaps the other's head.  Measured at configs[3]: 32 sequences as 2 x 16:
# -3.5 % step time, 64 as 2 x 32: -11 %; 4 streams were no better than 2.  The pieces use seeds of their own (different dropout masks).
_SPLIT_STREAMS = _lib.StreamFork()

# Modality streams.  The modalities of the MFT are independent until the MFN gate: their embeds, encoder stacks and LSTM scans run on one HIP
# stream each (the first on the caller's stream): one stack at the reference sizes fills only part of the 256 CUs, so concurrency, not a
# faster kernel, is what is missing.  ``MMT_MODALITY_STREAMS=0`` serialises everything on one stream.  Here, not beside the models, so that
# multiTransformer and streaming share the one object.
_MOD_STREAMS = _lib.StreamFork("MMT_MODALITY_STREAMS")


def _row_chunks(B, k):
    k = max(1, min(int(k), B))
    base, rem = divmod(B, k)
    out, lo = [], 0
    for i in range(k):
        hi = lo + base + (1 if i < rem else 0)
        out.append((lo, hi))
        lo = hi
    return out


def _chunk_seed(seed, i, nsplit=1):
    if isinstance(seed, (list, tuple)):
        return seed[i]
    if isinstance(seed, _lib.DeviceSeed):
        if nsplit > 1:          # seed_advance_kernel reads and writes the state word: sub-batches on concurrent streams need one each
            raise ValueError("encoder_stack: %d sub-batch streams need a list of %d DeviceSeeds, got one" % (nsplit, nsplit))
        return seed
    return seed if i == 0 else _lib.mix64(seed, i)


def _encoder_fwd(ctx, x, mask, flat_params, h, d_ff, n_layers, eps, dropout_p, seed, nsplit, key_lengths=None, causal=False, span=None):
    """The fused stack's forward, one launch per sub-batch on a stream of its own; keeps on ``ctx`` what _encoder_bwd needs."""
    span = _check_span("encoder_stack", key_lengths, causal, span)
    causal = _check_causal("encoder_stack", key_lengths, causal)
    lib = _lib.load()
    _lib.require_hip(x, mask, flat_params)
    x_, m_, p_ = _f32c16(x), _f32c(mask), _f32c16(flat_params)
    B, T, d = x_.shape
    kl_ = _check_key_lengths("encoder_stack", key_lengths, B, x_.device)
    if m_.numel() != B * T:
        raise ValueError("mask must have B*T = %d elements (shape (B,T,1)), got %s" % (B * T, tuple(mask.shape)))
    m_ = m_.view(B, T)
    need = lib.mmt_encoder_param_count(d, d_ff, n_layers)
    if p_.numel() != need:
        raise ValueError("flat parameter buffer has %d elements, expected %d" % (p_.numel(), need))
    train = dropout_p > 0.0                    # eval-mode workspaces carry no dropout bit masks
    if isinstance(seed, (list, tuple)) and len(seed) < nsplit:
        raise ValueError("encoder_stack: one seed per sub-batch stream")
    chunks = _row_chunks(B, nsplit)
    seeds = [_chunk_seed(seed, i, len(chunks)) for i in range(len(chunks))]      # one DeviceSeed for several pieces: refused here, before
    y = torch.empty_like(x_)                                                     # a workspace is taken or a stream forked
    main, streams = _SPLIT_STREAMS.begin(x_.device, len(chunks))
    parts = []
    for i, ((b0, b1), st) in enumerate(zip(chunks, streams)):
        with torch.cuda.stream(st):
            dims = (b1 - b0, T, d, h, d_ff, n_layers)
            nbytes = (lib.mmt_encoder_workspace_bytes if train else lib.mmt_encoder_workspace_bytes_eval)(*dims)
            if nbytes == 0:
                _lib.launch("mmt_encoder_forward", None, None, None, None, None, 0, *dims, eps, 0.0, 0)
            ws = _lib.POOL.get(nbytes, x_.device, tag=("encoder",) + dims + (train,))
            sd = seeds[i]
            _launch_seeded("mmt_encoder_forward", sd, x_[b0:b1], m_[b0:b1], p_, y[b0:b1], ws, nbytes, *dims, eps, dropout_p,
                           key_lengths=None if kl_ is None else kl_[b0:b1], causal=causal, span=span)
            parts.append((b0, b1, ws, sd))
    _SPLIT_STREAMS.end(main, streams)
    if _hold(ctx, *[ws for _, _, ws, _ in parts]):
        ctx.save_for_backward(x_, m_, p_)
        ctx.parts = [(b0, b1, sd) for b0, b1, _, sd in parts]
        ctx.cfg = (T, d, h, d_ff, n_layers, eps, dropout_p)
        ctx.key_lengths, ctx.causal, ctx.span = kl_, causal, span
    return y


def _encoder_bwd(ctx, dy):
    """-> (dx, gradient of the flat parameter buffer) of _encoder_fwd's call."""
    wss = _take_ws(ctx, "encoder_stack")
    x_, m_, p_ = ctx.saved_tensors
    T, d, h, d_ff, n_layers, eps, dropout_p = ctx.cfg
    kl_ = ctx.key_lengths
    dy_ = _f32c16(dy)
    dx = torch.empty_like(x_)
    dps = [torch.empty_like(p_) for _ in wss]       # fresh buffers per call: returned gradient views never alias later calls
    main, streams = _SPLIT_STREAMS.begin(x_.device, len(wss))
    for (b0, b1, sd), ws, dp, st in zip(ctx.parts, wss, dps, streams):
        with torch.cuda.stream(st):
            _launch_seeded("mmt_encoder_backward", sd, dy_[b0:b1], x_[b0:b1], m_[b0:b1], p_, dx[b0:b1], dp, ws, ws.numel(),
                           b1 - b0, T, d, h, d_ff, n_layers, eps, dropout_p, state_arg=False,
                           key_lengths=None if kl_ is None else kl_[b0:b1], causal=ctx.causal, span=ctx.span)
            _lib.POOL.put(ws)
    _SPLIT_STREAMS.end(main, streams)
    if len(dps) > 1:                                # the sub-batches' parameter gradients, summed into the first buffer
        n = p_.numel()
        for other in dps[1:]:
            copy2d([_seg(dps[0], n, 1, n, src=other, src_ld=n, acc=True)])
    return dx, dps[0]


class _EncoderStackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, flat_params, h, d_ff, n_layers, eps, dropout_p, seed, nsplit, key_lengths=None, causal=False, span=None):
        return _encoder_fwd(ctx, x, mask, flat_params, h, d_ff, n_layers, eps, dropout_p, seed, nsplit, key_lengths, causal, span)

    @staticmethod
    def backward(ctx, dy):
        dx, dflat = _encoder_bwd(ctx, dy)
        return dx, None, dflat, None, None, None, None, None, None, None, None, None, None


def encoder_stack(x, mask, flat_params, h, d_ff, n_layers, eps=1e-6, dropout_p=0.0, seed=0, nsplit=1, key_lengths=None, causal=False,
                  span=None):
    """``seed``: a python int (by value) or a ``_lib.DeviceSeed`` (device-resident: fresh masks at every hipGraph replay), or one
    of either per sub-batch stream; ``nsplit``: run the batch as that many sub-batches on HIP streams of their own (see _SPLIT_STREAMS).
    ``key_lengths``: int32 (B,) (``key_lengths(mask)``): sequence b attends keys < key_lengths[b] in every layer; None: the
    reference's semantics, every key is attended.  Sub-batches take their slice of the lengths.
    ``causal``: window t attends windows 0 .. t in every layer (see ``sdpa``); never together with ``key_lengths`` (ValueError).
    ``span`` (with ``causal``): window t attends windows t - span + 1 .. t in every layer (see ``sdpa``)."""
    return _EncoderStackFn.apply(x, mask, flat_params, int(h), int(d_ff), int(n_layers), float(eps), float(dropout_p), _seed_arg(seed),
                                 int(nsplit), key_lengths, causal, span)


class _EncoderStackParamsFn(torch.autograd.Function):
    """Same stack, taking the individual parameter tensors (in the reference's registration order).  The flat buffer is
    assembled inside ``forward`` and — the point of this variant — ``backward`` hands every parameter a VIEW of ONE flat
    gradient buffer, so ``p.grad`` of all parameters alias a single allocation: data-parallel training all-reduces that
    buffer in place with one collective and no staging copies (``parallel.allreduce_gradients``)."""

    @staticmethod
    def forward(ctx, x, mask, h, d_ff, n_layers, eps, dropout_p, seed, flat, nsplit, key_lengths, causal, span, *params):
        # `flat`: the parameters' own storage when they are views of one buffer (multiTransformer.Encoder keeps them that way), else
        # None and the buffer is assembled here (one concatenation kernel per step)
        if flat is None:
            flat = torch.cat([q.detach().reshape(-1) for q in params]).float()
        ctx.shapes = [tuple(q.shape) for q in params]
        return _encoder_fwd(ctx, x, mask, flat, h, d_ff, n_layers, eps, dropout_p, seed, nsplit, key_lengths, causal, span)

    @staticmethod
    def backward(ctx, dy):
        dx, dflat = _encoder_bwd(ctx, dy)
        grads = [g.view(shp) for g, shp in zip(dflat.split([math.prod(shp) for shp in ctx.shapes]), ctx.shapes)]
        return (dx, None, None, None, None, None, None, None, None, None, None, None, None) + tuple(grads)


def encoder_stack_params(x, mask, params, h, d_ff, n_layers, eps=1e-6, dropout_p=0.0, seed=0, flat=None, nsplit=1, key_lengths=None,
                         causal=False, span=None):
    return _EncoderStackParamsFn.apply(x, mask, int(h), int(d_ff), int(n_layers), float(eps), float(dropout_p), _seed_arg(seed), flat,
                                       int(nsplit), key_lengths, causal, span, *params)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a_2, b_2, eps):
        _lib.require_hip(x, a_2, b_2)
        x_, a_, b_ = _f32c16(x), _f32c16(a_2), _f32c16(b_2)
        d = x_.shape[-1]
        M = x_.numel() // d
        y = torch.empty_like(x_)
        stats = torch.empty(M, 2, dtype=torch.float32, device=x_.device)
        _lib.launch("mmt_layernorm_forward", x_, a_, b_, y, stats, M, d, eps)
        ctx.save_for_backward(x_, a_, stats)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x_, a_, stats = ctx.saved_tensors
        d = x_.shape[-1]
        M = x_.numel() // d
        dy_ = _f32c16(dy)
        dx, da, db = torch.empty_like(x_), torch.empty_like(a_), torch.empty_like(a_)
        scratch = torch.empty(_lib.load().mmt_layernorm_scratch_floats(M, d), dtype=torch.float32, device=x_.device)
        _lib.launch("mmt_layernorm_backward", dy_, x_, a_, stats, dx, da, db, scratch, M, d, ctx.eps)
        return dx, da, db, None


def layer_norm(x, a_2, b_2, eps=1e-6):
    return _LayerNormFn.apply(x, a_2, b_2, float(eps))


class _SdpaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, h, dropout_p, seed, key_lengths=None, causal=False, span=None):
        span = _check_span("sdpa", key_lengths, causal, span)
        causal = _check_causal("sdpa", key_lengths, causal)
        lib = _lib.load()
        _lib.require_hip(q, k, v, mask)
        q_, k_, v_, m_ = _f32c(q), _f32c(k), _f32c(v), _f32c(mask)
        B, T, d = q_.shape
        kl_ = _check_key_lengths("sdpa", key_lengths, B, q_.device)
        if k_.shape != q_.shape or v_.shape != q_.shape:
            raise NotImplementedError("sdpa: query, key and value must share the shape (B,T,d)")
        if m_ is not None and m_.numel() != B * T:
            raise NotImplementedError("sdpa: only the reference's query-row mask of shape (B,T,1) is supported")
        train = dropout_p > 0.0
        nbytes = (lib.mmt_sdpa_workspace_bytes if train else lib.mmt_sdpa_workspace_bytes_eval)(B, T, d, h)
        if nbytes == 0:
            _lib.launch("mmt_sdpa_forward", None, None, None, None, None, None, 0, B, T, d, h, 0.0, 0)
        ws = _lib.POOL.get(nbytes, q_.device, tag=("sdpa", B, T, d, h, train))
        out = torch.empty_like(q_)
        _lib.launch("mmt_sdpa_forward", q_, k_, v_, m_, out, ws, nbytes, B, T, d, h, dropout_p, seed, key_lengths=kl_, causal=causal,
                    span=span)
        if _hold(ctx, ws):
            ctx.cfg, ctx.mask, ctx.key_lengths, ctx.causal, ctx.span = (B, T, d, h, dropout_p, seed), m_, kl_, causal, span
        return out

    @staticmethod
    def backward(ctx, dctx):
        (ws,) = _take_ws(ctx, "sdpa")
        B, T, d, h, dropout_p, seed = ctx.cfg
        g = _f32c(dctx)
        dq, dk, dv = (torch.empty_like(g) for _ in range(3))
        _lib.launch("mmt_sdpa_backward", g, ctx.mask, dq, dk, dv, ws, ws.numel(), B, T, d, h, dropout_p, seed, key_lengths=ctx.key_lengths,
                    causal=ctx.causal, span=ctx.span)
        _lib.POOL.put(ws)
        return dq, dk, dv, None, None, None, None, None, None, None


def sdpa(q, k, v, mask, h, dropout_p=0.0, seed=0, key_lengths=None, causal=False, span=None):
    """q,k,v: (B,T,d) with head i in columns [i*d/h,(i+1)*d/h); mask (B,T,1) blanks query rows; -> (B,T,d).
    dropout_p / seed: train-mode dropout on the probabilities (transformer/MFT/multiTransformer.py:32-33).
    key_lengths: int32 (B,) (``key_lengths(mask)``): sequence b attends keys < key_lengths[b] only — later keys get probability 0 and
    dk = dv = 0, a blanked query row is uniform over the visible keys; values outside [1, T] are clamped.  None: every key is attended.
    causal: query window t attends keys 0 .. t of its sequence only — later keys get probability exactly 0 and no dk, dv from that query,
    a blanked query row t is uniform over its t + 1 visible keys, row 0 attends one key.  Dropout bits are drawn as without the flag.
    Not combined with key_lengths (ValueError before any launch): causal attention already keeps a valid window of a prefix-masked
    batch from the padding behind its sequence, since t < len means every visible key is < len.
    span (an int >= 1, with causal=True only; None: off): query window t attends keys max(0, t - span + 1) .. t — the last ``span``
    windows, its own included.  Every other key gets probability exactly 0 and no dk, dv from that query; a blanked query row t is
    uniform over its min(t + 1, span) visible keys; span = 1 gives ctx[b, t] = bf16(v[b, t]) in eval mode; span >= T is causal
    attention as a function, computed by the band kernels (within tolerance of causal=True alone, not bit for bit).  ValueError before
    any launch without causal=True, with key_lengths, for span < 1 and for a bool or a non-integer."""
    return _SdpaFn.apply(q, k, v, mask, int(h), float(dropout_p), int(seed), key_lengths, causal, span)


def attn_probs(q, k, mask, h, dropout_p=0.0, seed=0, key_lengths=None, causal=False, span=None):
    """The probabilities ``sdpa(q, k, v, mask, h, dropout_p, seed)`` uses, materialised: (B,h,T,T) fp32, [b][head][query][key]
    (transformer/MFT/multiTransformer.py:22-34, the reference's ``self.attn`` of :59).  Same operand rounding as the attention core; in
    train mode the same keep decisions for the same seed, dropped = 0 and kept = P/(1-p).  A blanked query row is exactly 1/T.
    key_lengths: as for ``sdpa``; columns >= key_lengths[b] are exact zeros and a blanked query row is 1/key_lengths[b] on the others.
    causal: as for ``sdpa``; entries above the diagonal are exact zeros and a blanked query row t is 1/(t+1) on columns 0 .. t.
    span: as for ``sdpa``; entries outside columns max(0, t - span + 1) .. t of row t are exact zeros and a blanked query row t is
    1/min(t + 1, span) on those columns.
    No autograd graph: the reference never differentiates the map."""
    span = _check_span("attn_probs", key_lengths, causal, span)
    causal = _check_causal("attn_probs", key_lengths, causal)
    _lib.require_hip(q, k, mask)
    _lib.load()
    q_, k_, m_ = _f32c(q), _f32c(k), _f32c(mask)
    B, T, d = q_.shape
    if k_.shape != q_.shape:
        raise NotImplementedError("attn_probs: query and key must share the shape (B,T,d)")
    if m_ is not None and m_.numel() != B * T:
        raise NotImplementedError("attn_probs: only the reference's query-row mask of shape (B,T,1) is supported")
    kl_ = _check_key_lengths("attn_probs", key_lengths, B, q_.device)
    h = int(h)
    if h <= 0 or d % h or d // h > 64 or T > 4096:         # refused by the library before anything as large as the map is allocated
        _lib.launch("mmt_attn_probs_forward", None, None, None, None, B, T, d, h, 0.0, 0)
    out = torch.empty((B, h, T, T), dtype=torch.float32, device=q_.device)
    _lib.launch("mmt_attn_probs_forward", q_, k_, m_, out, B, T, d, h, float(dropout_p), int(seed), key_lengths=kl_, causal=causal,
                span=span)
    return out


def _linear_ws(x_, N):
    """The pool workspace of an affine map of x_ to N features (zero pads survive reuse: the kernels never write them)."""
    K = x_.shape[-1]
    M = x_.numel() // K
    return _lib.POOL.get(_lib.load().mmt_linear_workspace_bytes(M, K, N), x_.device, tag=("linear", M, K, N))


def _raw_linear_fwd(x_, W_, b_, act=0, r_=None, in_p=0.0, out_p=0.0, seed=0):
    """y = rowscale * drop_out(act(drop_in(x) W^T + b)) on contiguous fp32 device tensors, outside autograd -> (y, workspace)."""
    K, N = x_.shape[-1], W_.shape[0]
    M = x_.numel() // K
    if W_.shape[1] != K:
        raise ValueError("linear: weight %s does not match input features %d" % (tuple(W_.shape), K))
    ws = _linear_ws(x_, N)
    y = torch.empty(x_.shape[:-1] + (N,), dtype=torch.float32, device=x_.device)
    if in_p > 0.0 or out_p > 0.0:
        _lib.launch("mmt_linear_dropout_forward", x_, W_, b_, r_, y, ws, ws.numel(), M, K, N, act, in_p, out_p, *_seed_pair(seed))
    else:
        _lib.launch("mmt_linear_forward", x_, W_, b_, r_, y, ws, ws.numel(), M, K, N, act)
    return y, ws


def _raw_linear_bwd(g, x_, W_, y_, r_, ws, need_x, need_w, need_b, act=0, in_p=0.0, out_p=0.0, seed=0, dW=None, db=None):
    """-> (dx, dW, db) of the affine map above, each None unless asked for (or, for dW and db, handed in to be written); hands the
    workspace back to the pool."""
    K, N = x_.shape[-1], W_.shape[0]
    M = x_.numel() // K
    dx = torch.empty_like(x_) if need_x else None
    dW = torch.empty_like(W_) if need_w else dW
    db = torch.empty(N, dtype=torch.float32, device=x_.device) if need_b else db
    if in_p > 0.0 or out_p > 0.0:
        value, state = _seed_pair(seed)
        _lib.launch("mmt_linear_dropout_backward", g, x_, W_, y_, r_, dx, dW, db, ws, ws.numel(), M, K, N, act, in_p, out_p, value,
                    int(state is not None))
    else:
        _lib.launch("mmt_linear_backward", g, x_, W_, y_, r_, dx, dW, db, ws, ws.numel(), M, K, N, act)
    _lib.POOL.put(ws)
    return dx, dW, db


def _wgrad(g, x, W, dW, db=None):
    """dW = g^T x (and db = the column sums of g) into the given tensors: the weight-gradient half of the affine map's backward, used
    for the window contractions of the scans."""
    _raw_linear_bwd(g, x, W, None, None, _linear_ws(x, W.shape[0]), False, False, False, dW=dW, db=db)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, rowscale, act, in_p, out_p, seed):
        _lib.require_hip(x, W, b, rowscale)
        x_, W_, b_, r_ = _f32c16(x), _f32c(W), _f32c(b), _f32c(rowscale)
        if r_ is not None and r_.numel() != x_.numel() // x_.shape[-1]:
            raise ValueError("linear: rowscale must have one entry per row")
        y, ws = _raw_linear_fwd(x_, W_, b_, act, r_, in_p, out_p, seed)
        ctx.cfg = (act, b is not None, in_p, out_p, seed)
        if _hold(ctx, ws):
            ctx.save_for_backward(x_, W_, y if act != 0 else None, r_)
        return y

    @staticmethod
    def backward(ctx, dy):
        (ws,) = _take_ws(ctx, "linear")
        x_, W_, y_, r_ = ctx.saved_tensors
        act, has_b, in_p, out_p, seed = ctx.cfg
        need = ctx.needs_input_grad
        dx, dW, db = _raw_linear_bwd(_f32c(dy), x_, W_, y_, r_, ws, need[0], need[1], has_b and need[2], act, in_p, out_p, seed)
        return dx, dW, db, None, None, None, None, None


def linear(x, weight, bias=None, act=0, rowscale=None, in_dropout=0.0, out_dropout=0.0, seed=0):
    """y = rowscale * drop_out(act(drop_in(x) W^T + b)); act: 0 none, 1 ReLU, 2 tanh, 3 sigmoid.  in_dropout / out_dropout: train-mode
    dropout probabilities fused into the kernel (out_dropout behind ReLU only); seed: python int or ``_lib.DeviceSeed``."""
    K = x.shape[-1]
    if K % 4:
        # the row kernels stage their A tile in 16-byte pieces of fp32: an input width that is no multiple of 4 (none occurs in the reference's
        # models) is brought to the next one with zero columns on x and on W — the product is unchanged, the gradients of the pads are dropped
        # by cat_cols' backward (an input-dropout mask then indexes the padded width, like every mask indexes padded leading dimensions)
        pad = 4 - K % 4
        x = cat_cols([x, torch.zeros(*x.shape[:-1], pad, dtype=x.dtype, device=x.device)])
        weight = cat_cols([weight, torch.zeros(weight.shape[0], pad, dtype=weight.dtype, device=weight.device)])
    return _LinearFn.apply(x, weight, bias, rowscale, int(act), float(in_dropout), float(out_dropout), _seed_arg(seed))


class _LinearPairFn(torch.autograd.Function):
    """(act1(x W1^T + b1), act2(x W2^T + b2)): two affine maps of ONE input as one autograd node, so that the two gradients into x are
    summed by a copy2d launch instead of by autograd's library add (the LSTM baselines feed their time-major embedding to the attention
    MLP and to the LSTM's input projection)."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, act1, act2):
        _lib.require_hip(x, W1, b1, W2, b2)
        x_, W1_, b1_, W2_, b2_ = _f32c16(x), _f32c(W1), _f32c(b1), _f32c(W2), _f32c(b2)
        y1, ws1 = _raw_linear_fwd(x_, W1_, b1_, act1)
        y2, ws2 = _raw_linear_fwd(x_, W2_, b2_, act2)
        ctx.cfg = (act1, act2, b1 is not None, b2 is not None)
        if _hold(ctx, ws1, ws2):
            ctx.save_for_backward(x_, W1_, W2_, y1 if act1 else None, y2 if act2 else None)
        return y1, y2

    @staticmethod
    def backward(ctx, dy1, dy2):
        ws1, ws2 = _take_ws(ctx, "linear_pair")
        x_, W1_, W2_, y1, y2 = ctx.saved_tensors
        act1, act2, has_b1, has_b2 = ctx.cfg
        need_x, g = ctx.needs_input_grad[0], ctx.needs_input_grad
        dy1 = _f32c(dy1) if dy1 is not None else torch.zeros(x_.shape[:-1] + (W1_.shape[0],), dtype=torch.float32, device=x_.device)
        dy2 = _f32c(dy2) if dy2 is not None else torch.zeros(x_.shape[:-1] + (W2_.shape[0],), dtype=torch.float32, device=x_.device)
        dx1, dW1, db1 = _raw_linear_bwd(dy1, x_, W1_, y1, None, ws1, need_x, g[1], has_b1 and g[2], act1)
        dx2, dW2, db2 = _raw_linear_bwd(dy2, x_, W2_, y2, None, ws2, need_x, g[3], has_b2 and g[4], act2)
        dx = torch.empty_like(x_) if need_x else None
        if need_x:
            K = x_.shape[-1]
            copy2d([_seg(dx, K, x_.numel() // K, K, src=dx1, src_ld=K, src2=dx2, src2_ld=K)])        # dx = dx1 + dx2
        return dx, dW1, db1, dW2, db2, None, None


def linear_pair(x, W1, b1, W2, b2, act1=0, act2=0):
    """(act1(x W1^T + b1), act2(x W2^T + b2)) with one gradient node for x; x's width must be a multiple of 4."""
    if x.shape[-1] % 4:
        raise ValueError("linear_pair: input width %d is no multiple of 4" % x.shape[-1])
    return _LinearPairFn.apply(x, W1, b1, W2, b2, int(act1), int(act2))


class _HighwayFn(torch.autograd.Function):
    """The Highway layer of the window encoder with the front-end's Dropout(0.3) behind it, as ONE autograd node:
        out = drop(gate * proj + (1 - gate) * x),  proj = x Wp^T + bp,  gate = sigmoid(x Wg^T + bg)
    (transformer/SFT/models.py:27-55,132-134).  One node, so that the three gradient paths into x (direct, through proj, through gate) are
    summed by a copy2d launch instead of by autograd's library adds."""

    @staticmethod
    def forward(ctx, x, Wp, bp, Wg, bg, p, seed, proj_act):
        _lib.require_hip(x, Wp, bp, Wg, bg)
        x_, Wp_, bp_, Wg_, bg_ = _f32c16(x), _f32c(Wp), _f32c(bp), _f32c(Wg), _f32c(bg)
        proj, wsp = _raw_linear_fwd(x_, Wp_, bp_, act=proj_act)
        gate, wsg = _raw_linear_fwd(x_, Wg_, bg_, act=3)
        out = torch.empty_like(x_)
        value, state = _seed_pair(seed)
        block = None if state is None else torch.empty(2, dtype=torch.int64, device=x_.device)     # this call's seed + stream keys
        _lib.launch("mmt_highway_forward", x_, proj, gate, out, x_.numel(), p, value, state, block)
        if _hold(ctx, wsp, wsg):
            ctx.save_for_backward(x_, Wp_, Wg_, proj, gate, block)
        ctx.cfg = (p, value, proj_act)
        return out

    @staticmethod
    def backward(ctx, dout):
        wsp, wsg = _take_ws(ctx, "highway")
        x_, Wp_, Wg_, proj, gate, block = ctx.saved_tensors
        p, seed, proj_act = ctx.cfg
        d_ = _f32c(dout)
        dx, dproj, dgate = torch.empty_like(x_), torch.empty_like(x_), torch.empty_like(x_)
        _lib.launch("mmt_highway_backward", d_, x_, proj, gate, dx, dproj, dgate, x_.numel(), p, seed, block)
        need_x, g = ctx.needs_input_grad[0], ctx.needs_input_grad
        dx1, dWp, dbp = _raw_linear_bwd(dproj, x_, Wp_, proj if proj_act else None, None, wsp, need_x, g[1], g[2], act=proj_act)
        dx2, dWg, dbg = _raw_linear_bwd(dgate, x_, Wg_, gate, None, wsg, need_x, g[3], g[4], act=3)
        if need_x:
            K = x_.shape[-1]
            copy2d([_seg(dx, K, x_.numel() // K, K, src=dx1, src_ld=K, src2=dx2, src2_ld=K, acc=True)])        # dx += dx1 + dx2
        return (dx if need_x else None), dWp, dbp, dWg, dbg, None, None, None


def highway(x, Wp, bp, Wg, bg, dropout_p=0.0, seed=0, proj_act=0):
    """drop(gate * proj + (1 - gate) * x) with proj = x Wp^T + bp, gate = sigmoid(x Wg^T + bg); seed: python int or ``_lib.DeviceSeed``
    (train-mode dropout: stream 3000 of dropout_mask, index = element).  proj_act = 1: proj = ReLU(x Wp^T + bp), the Highway of the
    B1-LSTM variant (transformer/B1-LSTM/models.py:52), the ReLU riding in the projection GEMM's epilogue."""
    return _HighwayFn.apply(x, Wp, bp, Wg, bg, float(dropout_p), _seed_arg(seed), int(proj_act))


class _LocalAttnFn(torch.autograd.Function):
    """ctx = convolve(h * valid, softmax(z)): the local attention of the LSTM baselines (transformer/B1-LSTM/models.py:10-25,186-207).
    z (B,T,L) logits, h (T,B,H) LSTM outputs (time-major, as lstm_scan returns them), valid (B,T[,1]) prefix mask -> ctx (B,T,H).
    ``taps`` False: the softmax runs over the TIME axis, padded steps included (the reference's nn.Softmax(dim=1) on 3-D logits).
    ``taps`` True (``models.attend_over_taps``): over the L taps of each row, so that row t depends on steps <= t alone.  Steps with
    valid == 0 contribute no h (pad_packed_sequence's zeros).  Gradients flow to z and h."""

    @staticmethod
    def forward(ctx, z, h, valid, taps):
        _lib.require_hip(z, h, valid)
        z_, h_, v_ = _f32c(z), _f32c16(h), _f32c(valid)
        B, T, L = z_.shape
        if h_.dim() != 3 or h_.shape[0] != T or h_.shape[1] != B:
            raise ValueError("local_attention: h must be (T,B,H) = (%d,%d,H), got %s" % (T, B, tuple(h_.shape)))
        if v_.numel() != B * T:
            raise ValueError("local_attention: valid must have B*T = %d entries, got %d" % (B * T, v_.numel()))
        H = h_.shape[2]
        out = torch.empty(B, T, H, dtype=torch.float32, device=z_.device)
        a = torch.empty(B, T, L, dtype=torch.float32, device=z_.device)
        _lib.launch("mmt_local_attn_forward_taps" if taps else "mmt_local_attn_forward", z_, h_, v_, out, a, B, T, H, L)
        ctx.save_for_backward(a, h_, v_)
        ctx.taps = taps
        return out

    @staticmethod
    def backward(ctx, dout):
        a, h_, v_ = ctx.saved_tensors
        B, T, L = a.shape
        H = h_.shape[2]
        g = _f32c16(dout)
        nbytes = _lib.load().mmt_local_attn_workspace_bytes(B, T, H, L)
        ws = _lib.POOL.get(nbytes, g.device, tag=("local_attn", B, T, H, L))
        dz, dh = torch.empty_like(a), torch.empty_like(h_)
        _lib.launch("mmt_local_attn_backward_taps" if ctx.taps else "mmt_local_attn_backward", g, a, h_, v_, dz, dh, ws, nbytes, B, T, H, L)
        _lib.POOL.put(ws)
        return dz, dh, None, None


def local_attention(z, h, valid, over="time"):
    """(B,T,L) logits, (T,B,H) LSTM outputs, (B,T[,1]) mask -> (B,T,H) context; see _LocalAttnFn.  ``over``: what the softmax
    normalises over, "time" (the reference's) or "taps" (``models.attend_over_taps``)."""
    if over not in ("time", "taps"):
        raise ValueError("local_attention: over must be \"time\" or \"taps\", got %r" % (over,))
    return _LocalAttnFn.apply(z, h, valid, over == "taps")


class _LstmScanFn(torch.autograd.Function):
    """h_all, c_all = scan(gx, W_rec, h0, c0): the recurrent half of an LSTM layer.

    gx (T,B,4H) already holds x_t W_ih^T + b_ih + b_hh.  Replaces the nn.LSTMCell loop of MFN
    (transformer/MFT/multiTransformer.py:200-208) and the nn.LSTM step loop of the SFT decoder
    (transformer/SFT/multiTransformer.py:471-476)."""

    @staticmethod
    def forward(ctx, gx, W_rec, h0, c0):
        ctx.set_materialize_grads(False)            # an unused output (the decoder never reads c_all) arrives as None, not as a zero fill
        _lib.require_hip(gx, W_rec, h0, c0)
        gx_, W_, h0_, c0_ = _f32c16(gx), _f32c(W_rec), _f32c16(h0), _f32c16(c0)
        T, B, H4 = gx_.shape
        H = H4 // 4
        if W_.shape != (4 * H, H):
            raise ValueError("lstm_scan: W_rec must be (4H,H) = (%d,%d), got %s" % (4 * H, H, tuple(W_.shape)))
        nbytes = _lib.load().mmt_lstm_scan_workspace_bytes(H)
        ws = _scratch(nbytes, gx_.device)
        h_all = torch.empty(T, B, H, dtype=torch.float32, device=gx_.device)
        c_all = torch.empty_like(h_all)
        acts = torch.empty(T, B, 4 * H, dtype=torch.float32, device=gx_.device)
        _lib.launch("mmt_lstm_scan_forward", gx_, W_, h0_, c0_, h_all, c_all, acts, ws, nbytes, T, B, H)
        if H > 128:                                 # four-CU scan: its exchange waits are bounded and report through this word
            _lib.ERRORS.watch(ws[:4].view(torch.int32), "lstm_scan forward (T=%d, B=%d, H=%d)" % (T, B, H))
        ctx.save_for_backward(W_, h0_, c0_, h_all, c_all, acts)
        ctx.dims = (T, B, H, nbytes)
        return h_all, c_all

    @staticmethod
    def backward(ctx, dh_all, dc_all):
        W_, h0_, c0_, h_all, c_all, acts = ctx.saved_tensors
        T, B, H, nbytes = ctx.dims
        dev = h_all.device
        dh_, dc_ = _f32c16(dh_all), _f32c16(dc_all)
        ws = _scratch(nbytes, dev)
        dgx = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
        dh0, dc0 = (torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(2))
        _lib.launch("mmt_lstm_scan_backward", dh_, dc_, W_, c0_, c_all, acts, dgx, dh0, dc0, ws, nbytes, T, B, H)
        if H > 128:
            _lib.ERRORS.watch(ws[:4].view(torch.int32), "lstm_scan backward (T=%d, B=%d, H=%d)" % (T, B, H))
        dW = None
        if ctx.needs_input_grad[1]:
            # dW_rec = sum_{t,b} dG[t,b,:]^T h_{t-1}[b,:]  — a window-contraction: the weight-gradient GEMM
            hprev = torch.empty_like(h_all)          # h_{t-1}: h0 (or zeros), then h_all shifted by one step
            copy2d([_seg(hprev, H, B, H, src=h0_, src_ld=H), _seg(hprev, H, (T - 1) * B, H, src=h_all, src_ld=H, dst_off=B * H)])
            dW = torch.empty_like(W_)
            _wgrad(dgx, hprev, W_, dW)
        return (dgx, dW, dh0 if (h0_ is not None and ctx.needs_input_grad[2]) else None,
                dc0 if (c0_ is not None and ctx.needs_input_grad[3]) else None)


def lstm_scan(gx, W_rec, h0=None, c0=None):
    return _LstmScanFn.apply(gx, W_rec, h0, c0)


def _stack_limits(T, B, H, L):
    """The limits of the stacked scan (csrc/scan_stack_plan.h), refused before any launch with the limit named."""
    if not 2 <= L <= 4:
        raise NotImplementedError("lstm_stack_scan: %d layers; the stacked scan takes 2 <= n_layers <= 4 (one layer: lstm_scan)" % L)
    if H % 4 or not 0 < H <= 128:
        raise NotImplementedError("lstm_stack_scan: hidden size %d; the stacked scan takes multiples of 4 up to 128 "
                                  "(its contraction is 2H <= 256 wide)" % H)
    if B > 512:
        raise NotImplementedError("lstm_stack_scan: batch %d; the stacked scan takes at most 512 sequences" % B)
    if T < 1 or B < 1:
        raise ValueError("lstm_stack_scan: empty input (T=%d, B=%d)" % (T, B))


def _stack_ws(H, L, device):
    return _lib.POOL.get(_lib.load().mmt_lstm_stack_workspace_bytes(H, L), device, tag=("lstm_stack", H, L))


class _LstmStackScanFn(torch.autograd.Function):
    """h_top, h_all, c_all = stacked scan(gx0, P, bias, h0, c0): L coupled LSTM layers whose top output feeds back into layer 0 — the
    decoder of transformer/SFT/multiTransformer.py:463-483 with n_layers = L > 1 (csrc/scan_stack.h, include/mmt_hip.h
    mmt_lstm_stack_scan_*).  gx0 (T,B,4H) holds enc_t W_ih_l0[:, d:]^T + b_0; P (L,4H,2H) the packed weights, bias (L-1,4H) the biases
    of layers >= 1, h0 / c0 (L,B,H) or None.  Only h_top = h_all[L-1] (T,B,H) carries a gradient; h_all / c_all (L,T,B,H) are returned
    for inspection.  The weight and bias gradients are batched after the scan: dP_l = dG_l^T [x_a ; x_b] and the column sums of dG_l."""

    @staticmethod
    def forward(ctx, gx0, P, bias, h0, c0):
        ctx.set_materialize_grads(False)
        _lib.require_hip(gx0, P, bias, h0, c0)
        gx_, P_, b_, h0_, c0_ = _f32c(gx0), _f32c(P), _f32c(bias), _f32c(h0), _f32c(c0)
        T, B, H4 = gx_.shape
        H, L = H4 // 4, P_.shape[0]
        _stack_limits(T, B, H, L)
        if P_.shape != (L, 4 * H, 2 * H) or b_.shape != (L - 1, 4 * H):
            raise ValueError("lstm_stack_scan: P must be (L,4H,2H) and bias (L-1,4H) for gx0 %s, got %s and %s"
                             % (tuple(gx_.shape), tuple(P_.shape), tuple(b_.shape)))
        for name, t in (("h0", h0_), ("c0", c0_)):
            if t is not None and t.shape != (L, B, H):
                raise ValueError("lstm_stack_scan: %s must be (L,B,H) = (%d,%d,%d), got %s" % (name, L, B, H, tuple(t.shape)))
        dev = gx_.device
        ws = _stack_ws(H, L, dev)
        h_all = torch.empty(L, T, B, H, dtype=torch.float32, device=dev)
        c_all = torch.empty_like(h_all)
        acts = torch.empty(L, T, B, 4 * H, dtype=torch.float32, device=dev)
        _lib.launch("mmt_lstm_stack_scan_forward", gx_, P_, b_, h0_, c0_, h_all, c_all, acts, ws, ws.numel(), T, B, H, L)
        _lib.POOL.put(ws)                           # the backward prepares its own fragments: nothing is kept in the workspace
        ctx.save_for_backward(P_, h0_, c0_, h_all, c_all, acts)
        ctx.dims = (T, B, H, L)
        h_top = h_all[L - 1]
        ctx.mark_non_differentiable(h_all, c_all)
        return h_top, h_all, c_all

    @staticmethod
    def backward(ctx, dh_top, _dh_all, _dc_all):
        P_, h0_, c0_, h_all, c_all, acts = ctx.saved_tensors
        T, B, H, L = ctx.dims
        dev = h_all.device
        need = ctx.needs_input_grad
        dG = torch.empty(L, T, B, 4 * H, dtype=torch.float32, device=dev)
        dh0, dc0 = (torch.empty(L, B, H, dtype=torch.float32, device=dev) for _ in range(2))
        ws = _stack_ws(H, L, dev)
        _lib.launch("mmt_lstm_stack_scan_backward", _f32c(dh_top), P_, c0_, c_all, acts, dG, dh0, dc0, ws, ws.numel(), T, B, H, L)
        _lib.POOL.put(ws)
        dP = dbias = None
        if need[1] or need[2]:
            # dP_l = sum_{t,b} dG_l[t,b,:]^T [x_a ; x_b][t,b,:]: the operand rows are h_all shifted by one step (h0 / zeros in step 0)
            n, S = T * B, T * B * H
            X = torch.empty(L, n, 2 * H, dtype=torch.float32, device=dev)
            segs = []
            for l in range(L):
                xo = l * n * 2 * H
                if l == 0:                          # x_a = o_{t-1}: zeros, then the top layer's outputs
                    segs += [_seg(X, 2 * H, B, H, dst_off=xo),
                             _seg(X, 2 * H, n - B, H, src=h_all, src_ld=H, src_off=(L - 1) * S, dst_off=xo + B * 2 * H)]
                else:                               # x_a = h^{l-1}_t
                    segs.append(_seg(X, 2 * H, n, H, src=h_all, src_ld=H, src_off=(l - 1) * S, dst_off=xo))
                segs += [_seg(X, 2 * H, B, H, src=h0_, src_ld=H, src_off=l * B * H, dst_off=xo + H),          # x_b = h^l_{t-1}
                         _seg(X, 2 * H, n - B, H, src=h_all, src_ld=H, src_off=l * S, dst_off=xo + B * 2 * H + H)]
            copy2d(segs)
            dP = torch.empty_like(P_)
            dbias = torch.empty(L - 1, 4 * H, dtype=torch.float32, device=dev)
            for l in range(L):
                _wgrad(dG[l].view(n, 4 * H), X[l], P_[l], dP[l], dbias[l - 1] if l else None)
        return (dG[0] if need[0] else None, dP if need[1] else None, dbias if need[2] else None,
                dh0 if (h0_ is not None and need[3]) else None, dc0 if (c0_ is not None and need[4]) else None)


def lstm_stack_scan(gx0, P, bias, h0=None, c0=None, return_states=False):
    """The top layer's outputs (T,B,H) of the stacked scan; return_states: also h_all, c_all (L,T,B,H), which carry no gradient."""
    h_top, h_all, c_all = _LstmStackScanFn.apply(gx0, P, bias, h0, c0)
    return (h_top, h_all, c_all) if return_states else h_top


def _fb_limits(T, B, H, E):
    """The limits of the feedback scan (csrc/scan_fb_plan.h), refused before any launch with the limit named."""
    if H % 4 or not 4 <= H <= 128:
        raise NotImplementedError("lstm_fb_scan: hidden size %d; the scan with the read-out in its recurrence takes h_dim in multiples of 4 "
                                  "from 4 to 128 (W_hh and the read-out stay in registers)" % H)
    if E % 4 or not 4 <= E <= 128:
        raise NotImplementedError("lstm_fb_scan: read-out width %d; the scan takes embed_dim in multiples of 4 from 4 to 128" % E)
    if B > 512:
        raise NotImplementedError("lstm_fb_scan: batch %d; the scan takes at most 512 sequences" % B)
    if T < 1 or B < 1:
        raise ValueError("lstm_fb_scan: empty input (T=%d, B=%d)" % (T, B))


def _fb_ws(H, E, device):
    return _lib.POOL.get(_lib.load().mmt_lstm_fb_scan_workspace_bytes(H, E), device, tag=("lstm_fb", H, E))


class _LstmFbScanFn(torch.autograd.Function):
    """p_all, h_all, c_all, u_all = feedback scan(gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0; p_init): an LSTM whose input at step t holds
    p_{t-1} = out(h_{t-1}), the read-out MLP of the previous state — the decoder loop of MultiEDLSTM, transformer/MFT/models.py:290-305
    (csrc/scan_fb.h, include/mmt_hip.h mmt_lstm_fb_scan_*).  gxc (T,B,4H) holds ctx_t W_ih[:, 1:]^T + b_ih + b_hh, w_p (4H) = W_ih[:, 0],
    W1 (E,H) / b1 (E) and w2 (E or (1,E)) / b2 (1) the read-out, h0 / c0 (B,H) or None, p_init a python float (no gradient).
    Only p_all (T,B) carries a gradient.  The parameter gradients are batched after the scan from its dG, du and dp:
    [dW_hh | dw_p] = dG^T [h_prev | p_prev], dW1 = du^T h, db1 = colsum du, dw2 = dp^T u, db2 = sum dp."""

    @staticmethod
    def forward(ctx, gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0, p_init):
        ctx.set_materialize_grads(False)
        _lib.require_hip(gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0)
        gx_, wp_, Wh_, W1_, b1_, w2_, b2_, h0_, c0_ = (_f32c(t) for t in (gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0))
        if gx_.dim() != 3 or gx_.shape[2] % 4:
            raise ValueError("lstm_fb_scan: gxc must be (T,B,4H), got %s" % (tuple(gx_.shape),))
        T, B, H4 = gx_.shape
        H, E = H4 // 4, W1_.shape[0]
        _fb_limits(T, B, H, E)
        if wp_.numel() != 4 * H or Wh_.shape != (4 * H, H) or W1_.shape != (E, H) or b1_.numel() != E or w2_.numel() != E or b2_.numel() != 1:
            raise ValueError("lstm_fb_scan: for gxc %s and W1 %s: w_p (4H), W_hh (4H,H), b1 (E), w2 (E), b2 (1) expected"
                             % (tuple(gx_.shape), tuple(W1_.shape)))
        for name, t in (("h0", h0_), ("c0", c0_)):
            if t is not None and t.shape != (B, H):
                raise ValueError("lstm_fb_scan: %s must be (B,H) = (%d,%d), got %s" % (name, B, H, tuple(t.shape)))
        dev = gx_.device
        ws = _fb_ws(H, E, dev)
        h_all = torch.empty(T, B, H, dtype=torch.float32, device=dev)
        c_all = torch.empty_like(h_all)
        acts = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
        u_all = torch.empty(T, B, E, dtype=torch.float32, device=dev)
        pfull = torch.empty(T + 1, B, dtype=torch.float32, device=dev)          # row 0: p_init, row t + 1: p_t
        _lib.launch("mmt_lstm_fb_scan_forward", gx_, wp_, Wh_, W1_, b1_, w2_, b2_, h0_, c0_, float(p_init), h_all, c_all, acts, u_all, pfull,
                    ws, ws.numel(), T, B, H, E)
        _lib.POOL.put(ws)                           # the backward prepares its own fragments: nothing is kept in the workspace
        ctx.save_for_backward(wp_, Wh_, W1_, w2_, h0_, c0_, h_all, c_all, acts, u_all, pfull)
        ctx.dims = (T, B, H, E)
        ctx.shapes = (tuple(w_p.shape), tuple(w2.shape), tuple(b2.shape))
        p_all = pfull[1:]
        ctx.mark_non_differentiable(h_all, c_all, u_all)
        return p_all, h_all, c_all, u_all

    @staticmethod
    def backward(ctx, dp_all, _dh_all, _dc_all, _du_all):
        wp_, Wh_, W1_, w2_, h0_, c0_, h_all, c_all, acts, u_all, pfull = ctx.saved_tensors
        T, B, H, E = ctx.dims
        dev = h_all.device
        need = ctx.needs_input_grad
        n = T * B
        g = _f32c(dp_all)
        if g is None:
            g = _new(T, B, like=h_all)
            copy2d([_seg(g, B, T, B)])
        dG = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
        du = torch.empty(T, B, E, dtype=torch.float32, device=dev)
        dp = torch.empty(T, B, dtype=torch.float32, device=dev)
        dh0, dc0 = (torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(2))
        ws = _fb_ws(H, E, dev)
        _lib.launch("mmt_lstm_fb_scan_backward", g, wp_, Wh_, W1_, w2_, c0_, c_all, acts, u_all, dG, du, dp, dh0, dc0, ws, ws.numel(), T, B, H, E)
        _lib.POOL.put(ws)
        dwp = dWhh = dW1 = db1 = dw2 = db2 = None
        K = H + 4                                   # p_{t-1} and three zero columns: the row kernels take widths in multiples of 4
        segs, X, dp4 = [], None, None
        if need[1] or need[2]:
            # [dW_hh | dw_p] = sum_{t,b} dG[t,b,:]^T [h_{t-1} | p_{t-1}][b,:]: the operand rows are h_all / p shifted by one step
            X = torch.empty(n, K, dtype=torch.float32, device=dev)
            segs += [_seg(X, K, B, H, src=h0_, src_ld=H), _seg(X, K, n - B, H, src=h_all, src_ld=H, dst_off=B * K),
                     _seg(X, K, n, 1, src=pfull, src_ld=1, dst_off=H), _seg(X, K, n, 3, dst_off=H + 1)]
        if need[5] or need[6]:
            # dw2 = sum dp_t u_t, db2 = sum dp_t: dp as the first of four columns of a gradient operand
            dp4 = torch.empty(n, 4, dtype=torch.float32, device=dev)
            segs += [_seg(dp4, 4, n, 1, src=dp, src_ld=1), _seg(dp4, 4, n, 3, dst_off=1)]
        copy2d(segs)
        if X is not None:
            dWX = torch.empty(4 * H, K, dtype=torch.float32, device=dev)
            _wgrad(dG.view(n, 4 * H), X, dWX, dWX)
            dWhh, dwp = torch.empty_like(Wh_), torch.empty(4 * H, dtype=torch.float32, device=dev)
            copy2d([_seg(dWhh, H, 4 * H, H, src=dWX, src_ld=K), _seg(dwp, 1, 4 * H, 1, src=dWX, src_ld=K, src_off=H)])
        if need[3] or need[4]:
            dW1, db1 = torch.empty_like(W1_), torch.empty(E, dtype=torch.float32, device=dev)
            _wgrad(du.view(n, E), h_all.view(n, H), W1_, dW1, db1)
        if dp4 is not None:
            dW2x, db2x = torch.empty(4, E, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.float32, device=dev)
            _wgrad(dp4, u_all.view(n, E), dW2x, dW2x, db2x)
            dw2, db2 = dW2x[0], db2x[:1]
        wp_shape, w2_shape, b2_shape = ctx.shapes
        return (dG if need[0] else None, dwp.view(wp_shape) if need[1] else None, dWhh if need[2] else None, dW1 if need[3] else None,
                db1 if need[4] else None, dw2.view(w2_shape) if need[5] else None, db2.view(b2_shape) if need[6] else None,
                dh0 if (h0_ is not None and need[7]) else None, dc0 if (c0_ is not None and need[8]) else None, None)


def lstm_fb_scan(gxc, w_p, W_hh, W1, b1, w2, b2, h0=None, c0=None, p_init=0.0, return_states=False):
    """p_all (T,B) of the scan with the read-out MLP in its recurrence (see _LstmFbScanFn); return_states: also h_all, c_all (T,B,H) and
    u_all (T,B,E), which carry no gradient."""
    p_all, h_all, c_all, u_all = _LstmFbScanFn.apply(gxc, w_p, W_hh, W1, b1, w2, b2, h0, c0, float(p_init))
    return (p_all, h_all, c_all, u_all) if return_states else p_all


AR_ORDER_MAX = 16   # csrc/ar_combine.h MMT_AR_MAXK (the tap cap of local_attn.h)


def _ar_limits(K):
    """The limit of the autoregressive read-out (csrc/ar_combine.h), refused before any launch with the limit named."""
    if not 1 <= K <= AR_ORDER_MAX:
        raise NotImplementedError("ar_combine: ar_order %d; the autoregressive read-out takes 1 <= ar_order <= %d" % (K, AR_ORDER_MAX))


def _scan_limits(H, who="lstm_scan"):
    """The hidden sizes mmt_lstm_scan_* takes, for callers that must refuse a size before any launch."""
    if H % 4 or not 4 <= H <= 256:
        raise NotImplementedError("%s: hidden size %d; lstm_scan takes h_dim in multiples of 4 from 4 to 256" % (who, H))


class _ArCombineFn(torch.autograd.Function):
    """out, p = the autoregressive read-out of MultiARLSTM (transformer/MFT/models.py:381-399; csrc/ar_combine.h, mmt_ar_combine_*).
    in_part (B,T[,1]) and ar_w (B,T,K) carry gradients; mask (B,T[,1]) and target (B,T[,1]) or None are data; p_init a python float.
      target given: p[b,t] = in_part[b,t] + sum_i ar_w[b,t,i] target[b,t-i], zeros before step 0 (tap 0 reads the current target);
      target None:  p[b,t] = in_part[b,t] + sum_k ar_w[b,t,k] p[b,t-K+k], p_init before step 0 — the step loop as ONE launch.
    out = p * mask.  The reference detaches the fed-back predictions, so the backward is one element-wise launch in both branches:
    d in_part = dout * mask, d ar_w[b,t,k] = d in_part[b,t] * (the value tap k read).  p (unmasked) carries no gradient."""

    @staticmethod
    def forward(ctx, in_part, ar_w, mask, target, p_init):
        ctx.set_materialize_grads(False)
        _lib.require_hip(in_part, ar_w, mask, target)
        if target is not None and target.requires_grad:
            raise NotImplementedError("ar_combine: the target is input data; a gradient w.r.t. it is not implemented "
                                      "(the reference never asks for one)")
        if ar_w.dim() != 3:
            raise ValueError("ar_combine: ar_w must be (B,T,ar_order), got %s" % (tuple(ar_w.shape),))
        B, T, K = ar_w.shape
        _ar_limits(K)
        if T < 1 or B < 1:
            raise ValueError("ar_combine: empty input (B=%d, T=%d)" % (B, T))
        for name, t in (("in_part", in_part), ("mask", mask), ("target", target)):
            if t is not None and (t.numel() != B * T or tuple(t.shape[:2]) != (B, T)):
                raise ValueError("ar_combine: %s must be (B,T[,1]) = (%d,%d[,1]), got %s" % (name, B, T, tuple(t.shape)))
        c_, w_, m_, t_ = _f32c(in_part), _f32c(ar_w), _f32c(mask), _f32c(target)
        p = _new(B, T, 1, like=w_)
        out = _new(B, T, 1, like=w_)
        _lib.launch("mmt_ar_combine_forward", c_, w_, m_, t_, float(p_init), p, out, B, T, K)
        ctx.save_for_backward(m_, p if t_ is None else t_)
        ctx.cfg = (B, T, K, t_ is not None, float(p_init), tuple(in_part.shape))
        ctx.mark_non_differentiable(p)
        return out, p

    @staticmethod
    def backward(ctx, dout, _dp):
        if dout is None:
            return None, None, None, None, None
        m_, hist = ctx.saved_tensors
        B, T, K, teacher, p_init, in_shape = ctx.cfg
        g = _f32c(dout)
        din, dw = _new(*in_shape, like=g), _new(B, T, K, like=g)
        _lib.launch("mmt_ar_combine_backward", g, m_, hist, int(teacher), p_init, din, dw, B, T, K)
        return din, dw, None, None, None


def ar_combine(in_part, ar_w, mask, target=None, p_init=0.0, return_p=False):
    """(B,T,1) masked predictions of the autoregressive read-out (see _ArCombineFn): teacher-forced on ``target``, free-running from
    ``p_init`` (a python number, passed by value: capturable in a hipGraph) without one.  return_p: also the unmasked p (B,T,1), which
    carries no gradient."""
    out, p = _ArCombineFn.apply(in_part, ar_w, mask, target, float(p_init))
    return (out, p) if return_p else out


class _ConvPoolFn(torch.autograd.Function):
    """out = max over positions of Conv1d(D -> F, kernel K)(window) + bias — the reference's CNN.forward
    (transformer/SFT/models.py:57-79).  x (N,W,D) is input data: no gradient flows to it.  K = weight.shape[2]: 2 (the reference's
    constant) runs the 2-tap kernels (mmt_convpool_*), every other 1 <= K <= 5 the K-tap kernels (csrc/convk.h, mmt_convpool_k_*).
    ``op``: the public function called, for the messages; "conv_maxpool" takes K = 2 only."""

    @staticmethod
    def forward(ctx, x, weight, bias, op):
        _lib.require_hip(x, weight, bias)
        if x.requires_grad:
            raise NotImplementedError("%s: the windows are input data; a gradient w.r.t. them is not implemented "
                                      "(the reference never asks for one)" % op)
        x_, w_, b_ = _f32c16(x), _f32c(weight), _f32c(bias)
        N, W, D = x_.shape
        k = "2" if op == "conv_maxpool" else "K"
        if w_.dim() != 3 or w_.shape[1] != D or (k == "2" and w_.shape[2] != 2):
            raise NotImplementedError("%s: weight must be (F, D, %s) = nn.Conv1d(D, F, kernel_size=%s).weight, got %s"
                                      % (op, k, k, tuple(w_.shape)))
        F_, K = w_.shape[0], w_.shape[2]
        entry, dims = ("mmt_convpool", (N, W, D, F_)) if K == 2 else ("mmt_convpool_k", (N, W, D, F_, K))
        nbytes = getattr(_lib.load(), entry + "_workspace_bytes")(*dims)
        if nbytes == 0:             # refused: the launch with nothing to run raises the library's own message
            _lib.launch(entry + "_forward", None, None, None, None, None, None, 0, *dims)
        ws = _scratch(nbytes, x_.device)
        out = torch.empty(N, F_, dtype=torch.float32, device=x_.device)
        arg = torch.empty(N, F_, dtype=torch.int32, device=x_.device)
        _lib.launch(entry + "_forward", x_, w_, b_, out, arg, ws, nbytes, *dims)
        ctx.save_for_backward(x_, arg)
        ctx.call = (entry, dims, tuple(w_.shape), nbytes)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)        # no zeros tensor for the index output's "gradient" (that would be a library fill kernel)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        x_, arg = ctx.saved_tensors
        entry, dims, wshape, nbytes = ctx.call
        if dout is None:
            return None, None, None, None
        g = _f32c(dout)
        ws = _scratch(nbytes, g.device)
        dw, db = torch.empty(wshape, dtype=torch.float32, device=g.device), torch.empty(wshape[0], dtype=torch.float32, device=g.device)
        _lib.launch(entry + "_backward", x_, g, arg, dw, db, ws, nbytes, *dims)
        return None, dw, db, None


def conv_maxpool(x, weight, bias):
    """x (N,W,D) windows, weight (F,D,2), bias (F) -> (out (N,F), argmax positions (N,F) int32)."""
    return _ConvPoolFn.apply(x, weight, bias, "conv_maxpool")


CONV_K_MAX = 5      # csrc/convk.h CK_MAXK


def conv_maxpool_k(x, weight, bias):
    """x (N,W,D) windows, weight (F,D,K) with 1 <= K <= 5, bias (F) -> (out (N,F), argmax positions (N,F) int32 in [0, W-K]).
    K = 2 is ``conv_maxpool`` itself (the product has one 2-tap path); the other sizes run the K-tap kernels."""
    return _ConvPoolFn.apply(x, weight, bias, "conv_maxpool_k")


def _mem_scan_fwd(apre, chat, Wm, W2, b2, T, B, dropout_p, seed):
    """The MFN memory recurrence on contiguous fp32 tensors with rows t*B + b -> (mem_all, u_all, g_all), shaped like apre's rows."""
    MD, HG = W2.shape[1], W2.shape[2]
    nbytes = _lib.load().mmt_mfn_mem_scan_workspace_bytes()
    ws = _scratch(nbytes, apre.device)
    rows = apre.shape[:-1]
    mem_all, u_all, g_all = _new(*rows, MD, like=apre), _new(*rows, 2 * HG, like=apre), _new(*rows, 2 * MD, like=apre)
    _launch_seeded("mmt_mfn_mem_scan_forward", seed, apre, chat, Wm, W2, b2, mem_all, u_all, g_all, ws, nbytes, T, B, MD, HG, dropout_p)
    return mem_all, u_all, g_all


def _mem_scan_bwd(dmem, chat, Wm, W2, mem_all, u_all, g_all, T, B, dropout_p):
    """-> (dapre, dchat, dWm, dW2, db2) of _mem_scan_fwd: the scan backward, then its batched weight gradients (window contractions)
    dWm = dapre^T mem_prev, dW2_g = dz_g^T u_g, db2_g = sum dz_g."""
    MD, HG = W2.shape[1], W2.shape[2]
    M = T * B
    nbytes = _lib.load().mmt_mfn_mem_scan_workspace_bytes()
    ws = _scratch(nbytes, dmem.device)
    dchat, dapre, dz = torch.empty_like(chat), torch.empty_like(u_all), torch.empty_like(g_all)
    _lib.launch("mmt_mfn_mem_scan_backward", dmem, chat, mem_all, u_all, g_all, Wm, W2, dchat, dapre, dz, ws, nbytes, T, B, MD, HG,
                dropout_p)
    mem_prev = torch.empty_like(mem_all)
    dzs, us = [_new(M, MD, like=dz) for _ in range(2)], [_new(M, HG, like=dz) for _ in range(2)]
    segs = [_seg(mem_prev, MD, B, MD), _seg(mem_prev, MD, M - B, MD, src=mem_all, src_ld=MD, dst_off=B * MD)]
    for g in range(2):
        segs += [_seg(dzs[g], MD, M, MD, src=dz, src_ld=2 * MD, src_off=g * MD),
                 _seg(us[g], HG, M, HG, src=u_all, src_ld=2 * HG, src_off=g * HG)]
    copy2d(segs)
    dWm, dW2, db2 = torch.empty_like(Wm), torch.empty_like(W2), _new(2, MD, like=dz)
    _wgrad(dapre, mem_prev, Wm, dWm)
    for g in range(2):
        _wgrad(dzs[g], us[g], W2[g], dW2[g], db2[g])
    return dapre, dchat, dWm, dW2, db2


class _MfnMemScanFn(torch.autograd.Function):
    """mem_all = scan(apre, chat, Wm, W2, b2): the MFN memory recurrence
    (transformer/MFT/multiTransformer.py:221-224) with everything that does not depend on mem batched before."""

    @staticmethod
    def forward(ctx, apre, chat, Wm, W2, b2, dropout_p, seed):
        _lib.require_hip(apre, chat, Wm, W2, b2)
        a_, c_, Wm_, W2_, b2_ = _f32c16(apre), _f32c16(chat), _f32c(Wm), _f32c(W2), _f32c16(b2)
        T, B, U = a_.shape
        MD, HG = c_.shape[-1], W2_.shape[-1]
        if U != 2 * HG or Wm_.shape != (U, MD) or W2_.shape != (2, MD, HG) or b2_.shape != (2, MD):
            raise ValueError("mfn_mem_scan: inconsistent shapes")
        mem_all, u_all, g_all = _mem_scan_fwd(a_, c_, Wm_, W2_, b2_, T, B, dropout_p, seed)
        ctx.save_for_backward(c_, Wm_, W2_, mem_all, u_all, g_all)
        ctx.dropout_p = dropout_p
        return mem_all

    @staticmethod
    def backward(ctx, dmem):
        c_, Wm_, W2_, mem_all, u_all, g_all = ctx.saved_tensors
        T, B = mem_all.shape[:2]
        dapre, dchat, dWm, dW2, db2 = _mem_scan_bwd(_f32c16(dmem), c_, Wm_, W2_, mem_all, u_all, g_all, T, B, ctx.dropout_p)
        return dapre, dchat, dWm, dW2, db2, None, None


def mfn_mem_scan(apre, chat, Wm, W2, b2, dropout_p=0.0, seed=0):
    return _MfnMemScanFn.apply(apre, chat, Wm, W2, b2, float(dropout_p), _seed_arg(seed))


def _mse_sum(pred, target, denom):
    """-> (loss, dpred): sum((pred - target)^2) / denom and its gradient 2 (pred - target) / denom, in one launch."""
    _lib.require_hip(pred, target)
    p_, t_ = _f32c16(pred), _f32c16(target)
    if p_.shape != t_.shape:
        raise ValueError("mse_sum_loss: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    n = p_.numel()
    loss = torch.empty((), dtype=torch.float32, device=p_.device)
    dpred = torch.empty_like(p_)
    scratch = torch.empty(_lib.load().mmt_mse_sum_scratch_doubles(n), dtype=torch.float64, device=p_.device)
    _lib.launch("mmt_mse_sum_forward", p_, t_, 1.0 / float(denom), loss, dpred, scratch, n)
    return loss, dpred


class _MseSumLossFn(torch.autograd.Function):
    """loss = sum((pred - target)^2) / denom and its gradient in one pass — the reference's per-batch loss
    (transformer/SFT/train.py:133-137: MSELoss(reduction='sum') divided by sum(lengths))."""

    @staticmethod
    def forward(ctx, pred, target, denom):
        loss, dpred = _mse_sum(pred, target, denom)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None


def mse_sum_loss(pred, target, denom):
    """sum((pred - target)^2) / denom with the gradient produced in the same pass (train-step semantics of the reference)."""
    return _MseSumLossFn.apply(pred, target, float(denom))


def mse_sum_loss_backward(pred, target, denom):
    """``loss = mse_sum_loss(pred, target, denom); loss.backward()`` (transformer/SFT/train.py:133-139) without the two kernels autograd
    spends on the seed gradient (a fill with 1.0 and a multiplication by it): the loss kernel's gradient 2 (pred - target) / denom is
    handed straight to ``pred.backward``.  Returns the detached loss."""
    loss, dpred = _mse_sum(pred, target, denom)
    pred.backward(dpred.view(pred.shape))
    return loss


# ---------------------------------------------------------------------------------------------------------------------------
# Data movement between the kernels (csrc/glue.h, mmt_copy2d): everything the reference does with torch.cat / stack / permute /
# slicing / broadcasting around the MFN gate and the SFT decoder, and the autograd twins of those ops, as strided 2-D copies in
# hand-written kernels — several per launch.
def _seg(dst, dst_ld, rows, cols, src=None, src_ld=0, src2=None, src2_ld=0, rowscale=None, perm=0, B=0, T=0, acc=False,
         dst_off=0, src_off=0, src2_off=0):
    """One copy segment on fp32 device tensors; *_off are ELEMENT offsets into the tensors' storage views."""
    def at(t, off):
        return None if t is None else t.data_ptr() + 4 * int(off)
    return _lib.CopySeg(at(src, src_off), at(src2, src2_off), at(dst, dst_off), at(rowscale, 0), int(rows), int(cols), int(src_ld),
                        int(src2_ld), int(dst_ld), int(perm), int(B), int(T), 1 if acc else 0)


def copy2d(segs):
    """Run a list of ``_seg`` copies (destinations must not overlap) — 24 per kernel launch."""
    segs = [g for g in segs if g.rows > 0 and g.cols > 0]
    if not segs:
        return
    arr = (_lib.CopySeg * len(segs))(*segs)
    _lib.launch("mmt_copy2d", ctypes.cast(arr, ctypes.c_void_p), len(segs))


def _new(*shape, like):
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


class _TimeMajorFn(torch.autograd.Function):
    """(B,T,d) -> (T,B,d) contiguous (the reference's ``permute(1,0,2)``, transformer/MFT/multiTransformer.py:300) as ONE copy."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_hip(x)
        x_ = _f32c(x)
        B, T, d = x_.shape
        y = _new(T, B, d, like=x_)
        copy2d([_seg(y, d, B * T, d, src=x_, src_ld=d, perm=1, B=B, T=T)])
        return y

    @staticmethod
    def backward(ctx, dy):
        return batch_major(dy)


class _BatchMajorFn(torch.autograd.Function):
    """(T,B,d) -> (B,T,d) contiguous, optionally times a per-window scale (the reference's ``* mask.float()``, :310)."""

    @staticmethod
    def forward(ctx, x, rowscale):
        _lib.require_hip(x, rowscale)
        x_, r_ = _f32c(x), _f32c(rowscale)
        T, B, d = x_.shape
        y = _new(B, T, d, like=x_)
        copy2d([_seg(y, d, B * T, d, src=x_, src_ld=d, perm=2, B=B, T=T, rowscale=r_)])
        ctx.r = r_
        return y

    @staticmethod
    def backward(ctx, dy):
        g = _f32c(dy)
        B, T, d = g.shape
        dx = _new(T, B, d, like=g)
        copy2d([_seg(dx, d, B * T, d, src=g, src_ld=d, perm=1, B=B, T=T, rowscale=ctx.r)])
        return dx, None


def time_major(x):
    return _TimeMajorFn.apply(x)


def batch_major(x, rowscale=None):
    """(T,B,d) -> (B,T,d); rowscale: (B,T[,1]) factors per window of the OUTPUT (e.g. the mask)."""
    return _BatchMajorFn.apply(x, rowscale)


class _DecoderPackFn(torch.autograd.Function):
    """Operands of the SFT decoder's recurrence from nn.LSTM's parameters (transformer/SFT/multiTransformer.py:463-476; step t feeds
    [o_{t-1}; enc_t] with o = h):  Wx = W_ih[:, d:] (multiplies enc_t, batched over T),  W_rec = W_ih[:, :d] + W_hh (multiplies h_{t-1}),
    a copy of W_hh (multiplies h0 in step 0, where o_{-1} = 0) and bias = b_ih + b_hh.  ONE node, so that the gradients of the several
    uses of W_ih and W_hh are combined here by the copy kernel and not by autograd's accumulation."""

    @staticmethod
    def forward(ctx, W_ih, W_hh, b_ih, b_hh):
        _lib.require_hip(W_ih, W_hh, b_ih, b_hh)
        Wi, Wh, bi, bh = _f32c(W_ih), _f32c(W_hh), _f32c(b_ih), _f32c(b_hh)
        G, d = Wh.shape
        if Wi.shape != (G, 2 * d):
            raise ValueError("decoder_pack: weight_ih must be (4d, 2d)")
        Wx, Wrec, Whh, bias = _new(G, d, like=Wi), _new(G, d, like=Wi), _new(G, d, like=Wi), _new(G, like=Wi)
        copy2d([_seg(Wx, d, G, d, src=Wi, src_ld=2 * d, src_off=d),
                _seg(Wrec, d, G, d, src=Wi, src_ld=2 * d, src2=Wh, src2_ld=d),
                _seg(Whh, d, G, d, src=Wh, src_ld=d),
                _seg(bias, G, 1, G, src=bi, src_ld=G, src2=bh, src2_ld=G)])
        ctx.dims = (G, d)
        return Wx, Wrec, Whh, bias

    @staticmethod
    def backward(ctx, dWx, dWrec, dWhh, dbias):
        G, d = ctx.dims
        like = next(t for t in (dWx, dWrec, dWhh, dbias) if t is not None)

        def z(t, *shape):
            return _f32c(t) if t is not None else torch.zeros(*shape, dtype=torch.float32, device=like.device)
        dWx, dWrec, dWhh, dbias = z(dWx, G, d), z(dWrec, G, d), z(dWhh, G, d), z(dbias, G)
        dWi, dWh = _new(G, 2 * d, like=like), _new(G, d, like=like)
        copy2d([_seg(dWi, 2 * d, G, d, src=dWrec, src_ld=d), _seg(dWi, 2 * d, G, d, src=dWx, src_ld=d, dst_off=d),
                _seg(dWh, d, G, d, src=dWrec, src_ld=d, src2=dWhh, src2_ld=d)])
        return dWi, dWh, dbias, dbias


def decoder_pack(W_ih, W_hh, b_ih, b_hh):
    return _DecoderPackFn.apply(W_ih, W_hh, b_ih, b_hh)


class _DecoderStackPackFn(torch.autograd.Function):
    """Operands of the stacked decoder scan from a multi-layer nn.LSTM's parameters (lstm_stack_scan; transformer/SFT/multiTransformer.py
    :444-446,463-476 with n_layers = L > 1): Wx = W_ih_l0[:, d:] (multiplies enc_t, batched over T), bias0 = b_ih_l0 + b_hh_l0,
    P (L,4d,2d) with P_0 = [W_ih_l0[:, :d] | W_hh_l0] and P_l = [W_ih_l | W_hh_l], bias (L-1,4d) = b_ih_l + b_hh_l.  Arguments: the four
    parameters of every layer, layer by layer.  ONE node: the gradients go back to weight_ih_l*, weight_hh_l*, bias_* by one copy launch."""

    @staticmethod
    def forward(ctx, *params):
        _lib.require_hip(*params)
        ps = [_f32c(t) for t in params]
        L = len(ps) // 4
        G, d = ps[1].shape
        if len(ps) != 4 * L or L < 2 or ps[0].shape != (G, 2 * d) or any(ps[4 * l].shape != (G, d) for l in range(1, L)):
            raise ValueError("decoder_stack_pack: nn.LSTM(2d, d, L >= 2) parameters expected")
        like = ps[0]
        Wx, bias0, P, bias = _new(G, d, like=like), _new(G, like=like), _new(L, G, 2 * d, like=like), _new(L - 1, G, like=like)
        segs = [_seg(Wx, d, G, d, src=ps[0], src_ld=2 * d, src_off=d), _seg(bias0, G, 1, G, src=ps[2], src_ld=G, src2=ps[3], src2_ld=G),
                _seg(P, 2 * d, G, d, src=ps[0], src_ld=2 * d), _seg(P, 2 * d, G, d, src=ps[1], src_ld=d, dst_off=d)]
        for l in range(1, L):
            Wi, Wh, bi, bh = ps[4 * l:4 * l + 4]
            po = l * G * 2 * d
            segs += [_seg(P, 2 * d, G, d, src=Wi, src_ld=d, dst_off=po), _seg(P, 2 * d, G, d, src=Wh, src_ld=d, dst_off=po + d),
                     _seg(bias, G, 1, G, src=bi, src_ld=G, src2=bh, src2_ld=G, dst_off=(l - 1) * G)]
        copy2d(segs)
        ctx.dims = (L, G, d)
        return Wx, bias0, P, bias

    @staticmethod
    def backward(ctx, dWx, dbias0, dP, dbias):
        L, G, d = ctx.dims
        like = next(t for t in (dWx, dbias0, dP, dbias) if t is not None)
        dWx, dbias0, dP, dbias = _f32c(dWx), _f32c(dbias0), _f32c(dP), _f32c(dbias)         # an absent gradient: zeros (src None)
        dWi0, dWh0, db0 = _new(G, 2 * d, like=like), _new(G, d, like=like), _new(G, like=like)
        segs = [_seg(dWi0, 2 * d, G, d, src=dP, src_ld=2 * d), _seg(dWi0, 2 * d, G, d, src=dWx, src_ld=d, dst_off=d),
                _seg(dWh0, d, G, d, src=dP, src_ld=2 * d, src_off=d), _seg(db0, G, 1, G, src=dbias0, src_ld=G)]
        outs = [dWi0, dWh0, db0, db0]
        for l in range(1, L):
            dWi, dWh, db = _new(G, d, like=like), _new(G, d, like=like), _new(G, like=like)
            po = l * G * 2 * d
            segs += [_seg(dWi, d, G, d, src=dP, src_ld=2 * d, src_off=po), _seg(dWh, d, G, d, src=dP, src_ld=2 * d, src_off=po + d),
                     _seg(db, G, 1, G, src=dbias, src_ld=G, src_off=(l - 1) * G)]
            outs += [dWi, dWh, db, db]
        copy2d(segs)
        return tuple(outs)


def decoder_stack_pack(lstm):
    """(Wx, bias0, P, bias) of a multi-layer decoder ``nn.LSTM(2d, d, L)`` for ``lstm_stack_scan``."""
    params = []
    for l in range(lstm.num_layers):
        params += [getattr(lstm, "%s_l%d" % (n, l)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return _DecoderStackPackFn.apply(*params)


class _DecoderFbPackFn(torch.autograd.Function):
    """Operands of the feedback scan from the parameters of MultiEDLSTM's decoder nn.LSTM(1 + H, H) (transformer/MFT/models.py:256,299-301;
    step t feeds [p_{t-1} ; ctx_t]): w_p = W_ih[:, 0] (multiplies the fed-back prediction), W_c = W_ih[:, 1:] (multiplies ctx_t, batched
    over T) and bias = b_ih + b_hh.  ONE node: the gradients go back to weight_ih_l0 and both biases by one copy launch."""

    @staticmethod
    def forward(ctx, W_ih, b_ih, b_hh):
        _lib.require_hip(W_ih, b_ih, b_hh)
        Wi, bi, bh = _f32c(W_ih), _f32c(b_ih), _f32c(b_hh)
        G, K = Wi.shape
        if G % 4 or K != G // 4 + 1 or bi.shape != (G,) or bh.shape != (G,):
            raise ValueError("decoder_fb_pack: nn.LSTM(1 + H, H) parameters expected, got weight_ih %s" % (tuple(Wi.shape),))
        H = K - 1
        wp, Wc, bias = _new(G, like=Wi), _new(G, H, like=Wi), _new(G, like=Wi)
        copy2d([_seg(wp, 1, G, 1, src=Wi, src_ld=K), _seg(Wc, H, G, H, src=Wi, src_ld=K, src_off=1),
                _seg(bias, G, 1, G, src=bi, src_ld=G, src2=bh, src2_ld=G)])
        ctx.dims = (G, H)
        return wp, Wc, bias

    @staticmethod
    def backward(ctx, dwp, dWc, dbias):
        G, H = ctx.dims
        like = next(t for t in (dwp, dWc, dbias) if t is not None)
        dwp, dWc, dbias = _f32c(dwp), _f32c(dWc), _f32c(dbias)                  # an absent gradient: zeros (src None)
        dWi, db = _new(G, H + 1, like=like), _new(G, like=like)
        copy2d([_seg(dWi, H + 1, G, 1, src=dwp, src_ld=1), _seg(dWi, H + 1, G, H, src=dWc, src_ld=H, dst_off=1),
                _seg(db, G, 1, G, src=dbias, src_ld=G)])
        return dWi, db, db


def decoder_fb_pack(lstm):
    """(w_p, W_c, bias) of a one-layer decoder ``nn.LSTM(1 + H, H)`` for ``lstm_fb_scan``."""
    return _DecoderFbPackFn.apply(lstm.weight_ih_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)


class _BroadcastLayersFn(torch.autograd.Function):
    """(L,1,n) parameter -> (L,B,n) contiguous (``dec_h0.repeat(1, B, 1)``, transformer/SFT/multiTransformer.py:465-466) as ONE copy;
    backward: the column sums per layer."""

    @staticmethod
    def forward(ctx, rows, B):
        _lib.require_hip(rows)
        r_ = _f32c(rows)
        L, n = r_.shape[0], r_.shape[-1]
        y = _new(L, B, n, like=r_)
        copy2d([_seg(y, n, B, n, src=r_, src_ld=0, src_off=l * n, dst_off=l * B * n) for l in range(L)])
        ctx.dims = (L, B, n, tuple(rows.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        L, B, n, shape = ctx.dims
        g = _f32c(dy)
        drows = _new(L, n, like=g)
        for l in range(L):
            _lib.launch("mmt_colsum", g[l], drows[l], B, n, n)
        return drows.view(shape), None


def broadcast_layers(rows, B):
    return _BroadcastLayersFn.apply(rows, int(B))


class _Add2Fn(torch.autograd.Function):
    """a + b for two tensors of one shape (bias_ih + bias_hh, W_ih[:, :d] + W_hh); the gradient passes to both unchanged."""

    @staticmethod
    def forward(ctx, a, b):
        _lib.require_hip(a, b)
        a_, b_ = _f32c(a), _f32c(b)
        if a_.shape != b_.shape:
            raise ValueError("add2: shapes differ")
        y = torch.empty_like(a_)
        n = a_.shape[-1] if a_.dim() > 1 else a_.numel()
        copy2d([_seg(y, n, a_.numel() // n, n, src=a_, src_ld=n, src2=b_, src2_ld=n)])
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add2(a, b):
    return _Add2Fn.apply(a, b)


class _AddRow0Fn(torch.autograd.Function):
    """gx[0] += row for a (T,B,n) tensor and a (1,n) row broadcast over the batch, IN PLACE (the reference's first decoder step sees
    h0 W_hh^T, transformer/SFT/multiTransformer.py:466-471); backward: the row's gradient is the column sum of dgx[0]."""

    @staticmethod
    def forward(ctx, gx, row):
        _lib.require_hip(gx, row)
        T, B, n = gx.shape
        if not gx.is_contiguous() or gx.dtype != torch.float32:
            raise ValueError("add_row0: a contiguous fp32 (T,B,n) tensor is modified in place")
        r_ = _f32c(row).reshape(-1)
        copy2d([_seg(gx, n, B, n, src=r_, src_ld=0, acc=True)])
        ctx.mark_dirty(gx)
        ctx.dims = (B, n, tuple(row.shape))
        return gx

    @staticmethod
    def backward(ctx, dy):
        B, n, rshape = ctx.dims
        g = _f32c(dy)
        drow = _new(n, like=g)
        _lib.launch("mmt_colsum", g, drow, B, n, n)
        return dy, drow.view(rshape)


def add_row0(gx, row):
    return _AddRow0Fn.apply(gx, row)


class _BroadcastRowsFn(torch.autograd.Function):
    """(1,n) parameter row -> (B,n) contiguous (``dec_c0[0].expand(B, d)``); backward: column sum."""

    @staticmethod
    def forward(ctx, row, B):
        _lib.require_hip(row)
        r_ = _f32c(row).reshape(-1)
        n = r_.numel()
        y = _new(B, n, like=r_)
        copy2d([_seg(y, n, B, n, src=r_, src_ld=0)])
        ctx.dims = (B, n, tuple(row.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, n, rshape = ctx.dims
        g = _f32c(dy)
        drow = _new(n, like=g)
        _lib.launch("mmt_colsum", g, drow, B, n, n)
        return drow.view(rshape), None


def broadcast_rows(row, B):
    return _BroadcastRowsFn.apply(row, int(B))


class _CatColsFn(torch.autograd.Function):
    """torch.cat(tensors, dim=-1) of tensors that share their leading dimensions; backward: the column split."""

    @staticmethod
    def forward(ctx, *ts):
        _lib.require_hip(*ts)
        ts_ = [_f32c(t) for t in ts]
        widths = [t.shape[-1] for t in ts_]
        rows = ts_[0].numel() // widths[0]
        W = sum(widths)
        y = _new(*ts_[0].shape[:-1], W, like=ts_[0])
        segs, col = [], 0
        for t, w in zip(ts_, widths):
            if t.numel() // w != rows:
                raise ValueError("cat_cols: leading dimensions differ")
            segs.append(_seg(y, W, rows, w, src=t, src_ld=w, dst_off=col))
            col += w
        copy2d(segs)
        ctx.widths, ctx.shapes = widths, [tuple(t.shape) for t in ts_]
        return y

    @staticmethod
    def backward(ctx, dy):
        g = _f32c(dy)
        W = sum(ctx.widths)
        rows = g.numel() // W
        outs, segs, col = [], [], 0
        for w, shp in zip(ctx.widths, ctx.shapes):
            o = _new(*shp, like=g)
            segs.append(_seg(o, w, rows, w, src=g, src_ld=W, src_off=col))
            outs.append(o)
            col += w
        copy2d(segs)
        return tuple(outs)


def cat_cols(tensors):
    return _CatColsFn.apply(*tensors)


class _MfnGateFn(torch.autograd.Function):
    """Everything of MFN.forward behind the per-modality LSTM scans (transformer/MFT/multiTransformer.py:212-247) as ONE autograd node:
    cStar assembly (one-step shift of c + concatenation), att1 MLP, softmax * cStar, att2 MLP, the `attended` part of both gamma fc1
    layers, the memory scan, [h ; mem] and the read-out MLP with its dropout.  Forward and backward call the C entry points in
    sequence: no library kernel runs, nothing is concatenated or sliced by torch, and gradients that meet (cStar and `attended` feed two
    consumers each) are added by the copy kernel instead of by autograd."""
    NP = 20     # parameter tensors, in this order: att1_fc1.{w,b} att1_fc2 att2_fc1 att2_fc2 gamma1_fc1 gamma1_fc2 gamma2_fc1 gamma2_fc2 out_fc1 out_fc2

    @staticmethod
    def forward(ctx, nm, pg, seed_g, p_out, seed_out, *ts):
        _lib.require_hip(*ts)
        hs = [_f32c(t) for t in ts[:nm]]
        cs = [_f32c(t) for t in ts[nm:2 * nm]]
        P = [_f32c(t) for t in ts[2 * nm:]]
        (a11w, a11b, a12w, a12b, a21w, a21b, a22w, a22b, g11w, g11b, g12w, g12b, g21w, g21b, g22w, g22b, o1w, o1b, o2w, o2b) = P
        T, B = hs[0].shape[0], hs[0].shape[1]
        M = T * B
        Hs = [h.shape[2] for h in hs]
        SH, MD, HG = sum(Hs), g12w.shape[0], g12w.shape[1]
        A = 2 * SH
        like = hs[0]
        # cStar = [c_{t-1} of every modality ; c_t of every modality]   (:212-217)
        c_star = _new(M, A, like=like)
        segs, col = [], 0
        for c, H in zip(cs, Hs):
            segs += [_seg(c_star, A, B, H, dst_off=col), _seg(c_star, A, M - B, H, src=c, src_ld=H, dst_off=B * A + col)]
            col += H
        for c, H in zip(cs, Hs):
            segs.append(_seg(c_star, A, M, H, src=c, src_ld=H, dst_off=col))
            col += H
        copy2d(segs)
        a1, ws_a11 = _raw_linear_fwd(c_star, a11w, a11b, 1)
        logits, ws_a12 = _raw_linear_fwd(a1, a12w, a12b, 0)
        att, attended = torch.empty_like(logits), torch.empty_like(logits)
        _lib.launch("mmt_softmax_mul_forward", logits, c_star, att, attended, M, A)
        a2, ws_a21 = _raw_linear_fwd(attended, a21w, a21b, 1)
        c_hat, ws_a22 = _raw_linear_fwd(a2, a22w, a22b, 2)
        # gamma fc1 = [attended part | memory part] of `both` (:221-223), gamma1 rows above gamma2 rows
        Wa, Wm, b1 = _new(2 * HG, A, like=like), _new(2 * HG, MD, like=like), _new(2 * HG, like=like)
        W2, b2 = _new(2, MD, HG, like=like), _new(2, MD, like=like)
        segs = []
        for i, (w, b, w2, bb2) in enumerate(((g11w, g11b, g12w, g12b), (g21w, g21b, g22w, g22b))):
            segs += [_seg(Wa, A, HG, A, src=w, src_ld=A + MD, dst_off=i * HG * A),
                     _seg(Wm, MD, HG, MD, src=w, src_ld=A + MD, src_off=A, dst_off=i * HG * MD),
                     _seg(b1, HG, 1, HG, src=b, src_ld=HG, dst_off=i * HG),
                     _seg(W2, HG, MD, HG, src=w2, src_ld=HG, dst_off=i * MD * HG),
                     _seg(b2, MD, 1, MD, src=bb2, src_ld=MD, dst_off=i * MD)]
        copy2d(segs)
        apre, ws_ap = _raw_linear_fwd(attended, Wa, b1, 0)
        mem_all, u_all, g_all = _mem_scan_fwd(apre, c_hat, Wm, W2, b2, T, B, pg, seed_g)
        # [h of every modality ; mem]  (:241-243) and the read-out MLP (:244-246)
        last = _new(M, SH + MD, like=like)
        segs, col = [], 0
        for h, H in zip(hs, Hs):
            segs.append(_seg(last, SH + MD, M, H, src=h, src_ld=H, dst_off=col))
            col += H
        segs.append(_seg(last, SH + MD, M, MD, src=mem_all, src_ld=MD, dst_off=col))
        copy2d(segs)
        hid, ws_o1 = _raw_linear_fwd(last, o1w, o1b, 1, None, 0.0, p_out, seed_out)
        out, ws_o2 = _raw_linear_fwd(hid, o2w, o2b, 0)
        if _hold(ctx, ws_a11, ws_a12, ws_a21, ws_a22, ws_ap, ws_o1, ws_o2):        # inference keeps nothing
            ctx.k = dict(nm=nm, T=T, B=B, Hs=Hs, SH=SH, MD=MD, HG=HG, A=A, pg=pg, p_out=p_out, seed_out=seed_out,
                         P=P, c_star=c_star, a1=a1, att=att, attended=attended, a2=a2, c_hat=c_hat, Wa=Wa, Wm=Wm, W2=W2,
                         mem_all=mem_all, u_all=u_all, g_all=g_all, last=last, hid=hid)
        return out.view(T, B, o2w.shape[0])

    @staticmethod
    def backward(ctx, dout):
        ws_a11, ws_a12, ws_a21, ws_a22, ws_ap, ws_o1, ws_o2 = _take_ws(ctx, "mfn_gate")
        k, ctx.k = ctx.k, None
        nm, T, B, Hs, SH, MD, HG, A = k["nm"], k["T"], k["B"], k["Hs"], k["SH"], k["MD"], k["HG"], k["A"]
        (a11w, a11b, a12w, a12b, a21w, a21b, a22w, a22b, g11w, g11b, g12w, g12b, g21w, g21b, g22w, g22b, o1w, o1b, o2w, o2b) = k["P"]
        M = T * B
        g = _f32c(dout).reshape(M, -1)
        like = g
        d_hid, dWo2, dbo2 = _raw_linear_bwd(g, k["hid"], o2w, None, None, ws_o2, True, True, True)
        d_last, dWo1, dbo1 = _raw_linear_bwd(d_hid, k["last"], o1w, k["hid"], None, ws_o1, True, True, True, 1, 0.0, k["p_out"],
                                             k["seed_out"])
        d_hs = [_new(T, B, H, like=like) for H in Hs]
        d_mem = _new(M, MD, like=like)
        segs, col = [], 0
        for o, H in zip(d_hs, Hs):
            segs.append(_seg(o, H, M, H, src=d_last, src_ld=SH + MD, src_off=col))
            col += H
        segs.append(_seg(d_mem, MD, M, MD, src=d_last, src_ld=SH + MD, src_off=col))
        copy2d(segs)
        d_apre, d_chat, dWm, dW2, db2s = _mem_scan_bwd(d_mem, k["c_hat"], k["Wm"], k["W2"], k["mem_all"], k["u_all"], k["g_all"], T, B,
                                                      k["pg"])
        d_att, dWa, db1 = _raw_linear_bwd(d_apre, k["attended"], k["Wa"], None, None, ws_ap, True, True, True)
        d_a2, dWa22, dba22 = _raw_linear_bwd(d_chat, k["a2"], a22w, k["c_hat"], None, ws_a22, True, True, True, 2)
        d_att2, dWa21, dba21 = _raw_linear_bwd(d_a2, k["attended"], a21w, k["a2"], None, ws_a21, True, True, True, 1)
        copy2d([_seg(d_att, A, M, A, src=d_att2, src_ld=A, acc=True)])                 # `attended` feeds att2_fc1 and both gamma fc1
        d_logits, d_cstar = torch.empty_like(d_att), torch.empty_like(d_att)
        _lib.launch("mmt_softmax_mul_backward", d_att, k["att"], k["c_star"], d_logits, d_cstar, M, A)
        d_a1, dWa12, dba12 = _raw_linear_bwd(d_logits, k["a1"], a12w, None, None, ws_a12, True, True, True)
        d_cs2, dWa11, dba11 = _raw_linear_bwd(d_a1, k["c_star"], a11w, k["a1"], None, ws_a11, True, True, True, 1)
        # dc_t = d cStar[new part]_t + d cStar[prev part]_{t+1}; both cStar paths (att1 MLP input, the product) summed on the way
        d_cs = [_new(T, B, H, like=like) for H in Hs]
        segs, col = [], 0
        for o, H in zip(d_cs, Hs):
            pc, nc = col, SH + col
            segs += [_seg(o, H, M, H, src=d_cstar, src_ld=A, src_off=nc, src2=d_cs2, src2_ld=A, src2_off=nc)]
            col += H
        copy2d(segs)
        segs, col = [], 0
        for o, H in zip(d_cs, Hs):
            segs += [_seg(o, H, M - B, H, src=d_cstar, src_ld=A, src_off=B * A + col, src2=d_cs2, src2_ld=A, src2_off=B * A + col, acc=True)]
            col += H
        copy2d(segs)
        # gradients of the gamma parameters back into the reference's tensors
        dg = [(_new(HG, A + MD, like=like), _new(HG, like=like), _new(MD, HG, like=like), _new(MD, like=like)) for _ in range(2)]
        segs = []
        for i, (dw, db, dw2, db2) in enumerate(dg):
            segs += [_seg(dw, A + MD, HG, A, src=dWa, src_ld=A, src_off=i * HG * A),
                     _seg(dw, A + MD, HG, MD, src=dWm, src_ld=MD, src_off=i * HG * MD, dst_off=A),
                     _seg(db, HG, 1, HG, src=db1, src_ld=HG, src_off=i * HG),
                     _seg(dw2, HG, MD, HG, src=dW2[i], src_ld=HG),
                     _seg(db2, MD, 1, MD, src=db2s[i], src_ld=MD)]
        copy2d(segs)
        gp = (dWa11, dba11, dWa12, dba12, dWa21, dba21, dWa22, dba22, dg[0][0], dg[0][1], dg[0][2], dg[0][3],
              dg[1][0], dg[1][1], dg[1][2], dg[1][3], dWo1, dbo1, dWo2, dbo2)
        return (None, None, None, None, None) + tuple(d_hs) + tuple(d_cs) + gp


def mfn_gate(hs, cs, params, gamma_dropout=0.0, gamma_seed=0, out_dropout=0.0, out_seed=0):
    """hs, cs: per-modality (T,B,H_m) LSTM states; params: the 20 gate tensors (see _MfnGateFn.NP) -> (T,B,output_dim)."""
    return _MfnGateFn.apply(len(hs), float(gamma_dropout), _seed_arg(gamma_seed), float(out_dropout), _seed_arg(out_seed),
                            *hs, *cs, *params)


# A causal encoder stack, one window per call (include/mmt_hip.h mmt_encoder_stream_*): eval mode, forward only.  The state (prepared
# bf16 weights, then the K/V cache) takes memory with any contents, so it comes from _scratch.
def _stream_bytes(entry, message, unknown, *dims):
    """The size query ``entry`` of a stream family; where it returns 0 a ValueError with the library's reason."""
    lib = _lib.load()
    nbytes = getattr(lib, entry)(*dims)
    if nbytes == 0:
        raise ValueError(message % (lib.mmt_last_error() or unknown).decode())
    return nbytes


def _forward_only(op, tensors, why="an input requires grad"):
    """The streams are inference: nothing that requires grad while grad is enabled."""
    if torch.is_grad_enabled() and any(isinstance(a, torch.Tensor) and a.requires_grad for a in tensors):
        raise NotImplementedError("%s: forward only, no autograd (%s)" % (op, why))


_PARAMS_GRAD = "parameters that require grad: pass detached tensors or call it under torch.no_grad()"


def _step_mask(op, mask_t, B, device):
    """``mask_t`` of a step: one entry per sequence on the inputs' device -> the (B) float32 argument, or None."""
    if mask_t is None:
        return None
    if not isinstance(mask_t, torch.Tensor) or mask_t.numel() != B or mask_t.device != device:
        raise ValueError("%s: mask_t must hold one entry per sequence (B = %d) on %s" % (op, B, device))
    return _f32c(mask_t).reshape(B)


def _stream_state(op, state, nbytes, device, maker):
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < nbytes:
        raise ValueError("%s: state must be a contiguous uint8 tensor of at least %d bytes (%s)" % (op, nbytes, maker))
    if state.device != device:
        raise ValueError("%s: state is on %s, the operands on %s" % (op, state.device, device))
    if state.data_ptr() % 16:           # a step reads the prepared weights (and the K/V cache) eight bf16 per lane, from pieces laid out from the base
        raise ValueError("%s: state must start at a 16-byte aligned address (%s gives one; a view at an odd offset does not), got "
                         "an address that is %d modulo 16" % (op, maker, state.data_ptr() % 16))


def _stream_positions(op, positions, B, device):
    """``positions`` of a slots step: the int32 (B) tensor the kernel reads and advances in place, so nothing may stand in for it."""
    if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or tuple(positions.shape) != (B,) \
            or not positions.is_contiguous() or positions.device != device:
        raise ValueError("%s: positions must be a contiguous int32 (%d,) tensor on %s (the kernel advances it in place), got %s %s on %s"
                         % (op, B, device, getattr(positions, "dtype", type(positions).__name__),
                            tuple(getattr(positions, "shape", ())), getattr(positions, "device", None)))


def _step_where(op, t, positions, limit, advance, B, device):
    """Where a step runs, as the entry's arguments: ``(t,)`` for a position by value (a negative one is refused), else ``positions`` on
    the device with their ``limit`` (None: none) and ``advance``."""
    if t is not None:
        if int(t) < 0:
            raise ValueError("%s: position t = %d is negative" % (op, int(t)))
        return (int(t),)
    _stream_positions(op, positions, B, device)
    return (positions, 0 if limit is None else int(limit), int(bool(advance)))


def _run_step(op, entry, rows, mask, out_shape, state, nbytes, maker, where, dims):
    """The launch of a carried-state step: ``rows`` the checked input (a tensor, or a list of them that goes as a table of pointers),
    ``mask`` from _step_mask, ``where`` from _step_where, ``nbytes`` the family's size query for these ``dims`` (called after
    require_hip, as its ValueError comes second) and ``maker`` the name of what allocates such a state -> y_t of ``out_shape``."""
    many = not isinstance(rows, torch.Tensor)
    rows = list(rows) if many else [rows]
    dev = rows[0].device
    _lib.require_hip(*rows, state)
    _stream_state(op, state, nbytes(), dev, maker)
    keep = [_f32c(x) for x in rows]                                        # alive until the launch is enqueued
    first = (ctypes.c_void_p * len(keep))(*[x.data_ptr() for x in keep]) if many else keep[0]
    y = torch.empty(*out_shape, dtype=torch.float32, device=dev)
    _lib.launch(entry, first, mask, y, state, state.numel(), *where, out_shape[0], *dims)
    return y


def encoder_stream_bytes(B, capacity, d, h, d_ff, n_layers):
    """Bytes of the stream state of this shape; ValueError, naming the limit, for a shape outside the step kernel's domain."""
    return _stream_bytes("mmt_encoder_stream_bytes", "encoder stream: %s", b"?", int(B), int(capacity), int(d), int(h), int(d_ff), int(n_layers))


def encoder_stream_state(B, capacity, d, h, d_ff, n_layers, device):
    """An unprepared stream state on ``device`` (uint8; any contents)."""
    return _scratch(encoder_stream_bytes(B, capacity, d, h, d_ff, n_layers), device)


def _stream_params(op, flat_params, d, d_ff, n_layers):
    _forward_only(op, (flat_params,), "parameters that require grad: call it under torch.no_grad()")
    p_ = _f32c(flat_params)
    need = _lib.load().mmt_encoder_param_count(d, d_ff, n_layers)
    if p_.numel() != need:
        raise ValueError("%s: flat parameter buffer has %d elements, expected %d" % (op, p_.numel(), need))
    return p_


def encoder_stream_prepare(flat_params, state, B, capacity, d, h, d_ff, n_layers):
    """Write the bf16 weights of ``flat_params`` into the front of ``state`` (one launch; the cache is not touched).  Again after the
    parameters change."""
    _lib.require_hip(flat_params, state)
    nbytes = encoder_stream_bytes(B, capacity, d, h, d_ff, n_layers)
    p_ = _stream_params("encoder_stream_prepare", flat_params, d, d_ff, n_layers)
    _stream_state("encoder_stream_prepare", state, nbytes, p_.device, "encoder_stream_state")
    _lib.launch("mmt_encoder_stream_prepare", p_, state, state.numel(), int(B), int(capacity), int(d), int(h), int(d_ff), int(n_layers))


def _encoder_step(op, x_t, mask_t, flat_params, state, h, d_ff, n_layers, capacity, eps, t=None, positions=None, advance=True, _ring=False):
    """Both forms of the encoder step: the position is ``t``, by value, or ``positions`` on the device (the capacity is its limit).
    ``_ring`` (streaming.encoder_ring_step*): ``capacity`` is the span of a ring cache, which no position below INT_MAX is outside."""
    _forward_only(op, (x_t, mask_t))
    if not isinstance(x_t, torch.Tensor) or x_t.dim() != 2 or x_t.dtype != torch.float32:
        raise ValueError("%s: x_t must be a float32 (B,d) tensor, got %s %s"
                         % (op, getattr(x_t, "dtype", type(x_t).__name__), tuple(getattr(x_t, "shape", ()))))
    B, d = x_t.shape
    m_ = _step_mask(op, mask_t, B, x_t.device)
    capacity = int(capacity)
    if t is not None:
        where = (int(t),)
        if _ring:
            if capacity < 1 or not 0 <= where[0] < 2 ** 31 - 1:
                raise ValueError("%s: span = %d and position t = %d: the span must be at least 1 and t in [0, INT_MAX)" % (op, capacity, where[0]))
        elif not 0 <= where[0] < capacity:
            raise ValueError("%s: position t = %d outside [0, capacity = %d): open a stream with a larger capacity" % (op, where[0], capacity))
    else:
        where = _step_where(op, None, positions, None, advance, B, x_t.device)
        where = (where[0], where[2])                                       # the capacity is the limit: the entry takes none
    _lib.require_hip(x_t, flat_params, state)
    nbytes = encoder_stream_bytes(B, capacity, d, h, d_ff, n_layers)
    p_ = _stream_params(op, flat_params, d, d_ff, n_layers)
    _stream_state(op, state, nbytes, x_t.device, "encoder_stream_state")
    x_ = _f32c(x_t)
    y = torch.empty_like(x_)
    entry = "mmt_" + op if not _ring else "mmt_encoder_stream_step_ring" + ("" if t is not None else "_slots")
    _lib.launch(entry, x_, m_, p_, y, state, state.numel(), *where, B, capacity, d, int(h), int(d_ff), int(n_layers), float(eps))
    return y


def encoder_stream_step(x_t, mask_t, flat_params, state, t, h, d_ff, n_layers, capacity, eps=1e-6):
    """Row t of a causal encoder stack: x_t (B,d), mask_t (B) or None -> y_t (B,d) = Encoder.forward(x, mask)[:, t] with causal attention
    on (transformer/MFT/multiTransformer.py:73-76; departs from :27-31), from the K/V cache in ``state`` (encoder_stream_state, prepared
    by encoder_stream_prepare), to which this window's keys and values are appended.  Steps of a recording run in order t = 0, 1, ...;
    t is passed by value.  One launch.  Forward only: an input that requires grad raises NotImplementedError."""
    return _encoder_step("encoder_stream_step", x_t, mask_t, flat_params, state, h, d_ff, n_layers, capacity, eps, t=int(t))


def encoder_stream_step_slots(x_t, mask_t, flat_params, state, positions, h, d_ff, n_layers, capacity, eps=1e-6, advance=True):
    """``encoder_stream_step`` with the position of every sequence in device memory (csrc/step_slots.h): ``positions`` int32 (B), read by
    the kernel.  Row b is the row of ``encoder_stream_step`` at t = positions[b], bit for bit, where 0 <= positions[b] < capacity, and
    zeros, with nothing else written, where the slot is idle (negative) or full (>= capacity).  ``advance``: the kernel adds 1 to the
    position of every slot it ran.  No position crosses the host, so the call can be captured into a graph; the capacity check is the
    kernel's.  One launch."""
    return _encoder_step("encoder_stream_step_slots", x_t, mask_t, flat_params, state, h, d_ff, n_layers, capacity, eps,
                         positions=positions, advance=advance)


# The MFN gate, one window per call (include/mmt_hip.h mmt_mfn_stream_*): eval mode, forward only.  The state (prepared bf16 weights,
# fp32 biases, two copies of the carried (h, c, mem)) takes memory with any contents, so it comes from _scratch.
_MFN_GATE_SHAPES = "att1_fc1 (128, A), att1_fc2 (A, 128), att2_fc1 (256, A), att2_fc2 (128, 256), gamma{1,2}_fc1 (64, A + 128), " \
                   "gamma{1,2}_fc2 (128, 64), out_fc1 (64, sum H + 128), out_fc2 (output_dim, 64), A = 2 sum H"


def _mfn_dims(in_dims, hidden):
    in_dims, hidden = [int(v) for v in in_dims], [int(v) for v in hidden]
    if len(in_dims) != len(hidden):
        raise ValueError("mfn stream: %d input widths for %d hidden sizes" % (len(in_dims), len(hidden)))
    n = len(in_dims)
    return n, (ctypes.c_int * max(n, 1))(*in_dims), (ctypes.c_int * max(n, 1))(*hidden), in_dims, hidden


def mfn_stream_bytes(B, in_dims, hidden, output_dim):
    """Bytes of the MFN stream state for ``B`` sequences, modalities of input widths ``in_dims`` and LSTM hidden sizes ``hidden``;
    ValueError, naming the limit, for a shape outside the step kernel's domain."""
    n, cd, ch, _, _ = _mfn_dims(in_dims, hidden)
    return _stream_bytes("mmt_mfn_stream_bytes", "%s", b"mfn stream: ?", int(B), n, cd, ch, int(output_dim))


def mfn_stream_state(B, in_dims, hidden, output_dim, device):
    """An unprepared MFN stream state on ``device`` (uint8; any contents)."""
    return _scratch(mfn_stream_bytes(B, in_dims, hidden, output_dim), device)


def mfn_stream_prepare(lstm_params, gate_params, state, B, in_dims, hidden, output_dim):
    """Convert and copy every parameter of an MFN into ``state`` (one launch; the carried state is not touched): ``lstm_params`` per
    modality (weight_ih, weight_hh, bias_ih, bias_hh) of its LSTMCell, ``gate_params`` the 20 gate tensors in ``_MfnGateFn``'s order.
    Again after any parameter changes: a step reads the biases from the state too."""
    op = "mfn_stream_prepare"
    lstm = [q for cell in lstm_params for q in cell]
    gate = list(gate_params)
    _forward_only(op, lstm + gate, _PARAMS_GRAD)
    n, cd, ch, D, H = _mfn_dims(in_dims, hidden)
    nbytes = mfn_stream_bytes(B, D, H, output_dim)
    SH, MD, HG = sum(H), 128, 64
    A = 2 * SH
    want = [s for d, h in zip(D, H) for s in ((4 * h, d), (4 * h, h), (4 * h,), (4 * h,))]
    if len(lstm) != 4 * n or [tuple(q.shape) for q in lstm] != want:
        raise ValueError("%s: the LSTM cells' parameters have the shapes %s, expected %s" % (op, [tuple(q.shape) for q in lstm], want))
    want = [(128, A), (128,), (A, 128), (A,), (256, A), (256,), (MD, 256), (MD,), (HG, A + MD), (HG,), (MD, HG), (MD,),
            (HG, A + MD), (HG,), (MD, HG), (MD,), (64, SH + MD), (64,), (int(output_dim), 64), (int(output_dim),)]
    if [tuple(q.shape) for q in gate] != want:
        raise ValueError("%s: the gate's sizes are fixed in the step kernel (%s); got %s"
                         % (op, _MFN_GATE_SHAPES, [tuple(q.shape) for q in gate]))
    _lib.require_hip(state, *lstm, *gate)
    _stream_state(op, state, nbytes, lstm[0].device, "mfn_stream_state")
    keep = [_f32c(q) for q in lstm + gate]                                 # alive until the launch is enqueued
    pl = (ctypes.c_void_p * len(lstm))(*[q.data_ptr() for q in keep[:len(lstm)]])
    pg = (ctypes.c_void_p * 20)(*[q.data_ptr() for q in keep[len(lstm):]])
    _lib.launch("mmt_mfn_stream_prepare", pl, pg, state, state.numel(), int(B), n, cd, ch, int(output_dim))


def _mfn_step(op, xs, mask_t, state, in_dims, hidden, output_dim, t=None, positions=None, limit=None, advance=True):
    """Both forms of the gate step: the position is ``t``, by value, or ``positions`` on the device with their ``limit``."""
    xs = list(xs)
    _forward_only(op, xs + [mask_t])
    n, cd, ch, D, H = _mfn_dims(in_dims, hidden)
    if len(xs) != n:
        raise ValueError("%s: %d inputs for %d modalities" % (op, len(xs), n))
    for x, d in zip(xs, D):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] != d or x.shape[0] != xs[0].shape[0] \
                or x.device != xs[0].device:
            raise ValueError("%s: every x_t must be a float32 (B, %d) tensor on one device, got %s %s on %s"
                             % (op, d, getattr(x, "dtype", type(x).__name__), tuple(getattr(x, "shape", ())), getattr(x, "device", None)))
    B, dev = xs[0].shape[0], xs[0].device
    m_ = _step_mask(op, mask_t, B, dev)
    where = _step_where(op, t, positions, limit, advance, B, dev)
    return _run_step(op, "mmt_" + op, xs, m_, (B, int(output_dim)), state, lambda: mfn_stream_bytes(B, D, H, output_dim), "mfn_stream_state",
                     where, (n, cd, ch, int(output_dim)))


def mfn_stream_step(xs, mask_t, state, t, in_dims, hidden, output_dim):
    """Window t of an MFN gate: xs, per modality x_t (B, in_dims[m]); mask_t (B) or None -> y_t (B, output_dim) = MFN.forward(...)[:, t]
    in eval mode, times mask_t (transformer/MFT/multiTransformer.py:200-247, :310), from the (h, c, mem) carried in ``state``
    (mfn_stream_state, prepared by mfn_stream_prepare), which this call advances.  Steps of a recording run in order t = 0, 1, ...;
    t is passed by value.  One launch.  Forward only: an input that requires grad raises NotImplementedError."""
    return _mfn_step("mfn_stream_step", xs, mask_t, state, in_dims, hidden, output_dim, t=int(t))


def mfn_stream_step_slots(xs, mask_t, state, positions, in_dims, hidden, output_dim, limit=None, advance=True):
    """``mfn_stream_step`` with the position of every sequence in device memory (csrc/step_slots.h): ``positions`` int32 (B), read by the
    kernel.  Row b is the row of ``mfn_stream_step`` at t = positions[b], bit for bit (copy positions[b] & 1 of the carried state read,
    the other written), where the slot is seated, and zeros, with nothing else written, where it is idle (negative) or full
    (>= ``limit``; None: no limit).  ``advance``: the kernel adds 1 to the position of every slot it ran.  No position crosses the host,
    so the call can be captured into a graph.  One launch."""
    return _mfn_step("mfn_stream_step_slots", xs, mask_t, state, in_dims, hidden, output_dim, positions=positions, limit=limit, advance=advance)


# The affine map with its operands prepared once (include/mmt_hip.h mmt_linear_prepare / mmt_linear_forward_prepared): forward only.
def linear_prepare(W, b, prepared=None):
    """The padded bf16 copy of ``W`` (N, K) and the padded bias ``b`` (N) or None, as ``linear`` lays them into its workspace at every
    call -> a uint8 tensor for ``linear_prepared`` (``prepared``: one of this shape to write again), which carries its (K, N): the
    padded layout alone does not tell two shapes of one padded size apart.  Two launches."""
    _forward_only("linear_prepare", (W, b), "pass detached tensors or call it under torch.no_grad()")
    if not isinstance(W, torch.Tensor) or W.dim() != 2 or (b is not None and tuple(b.shape) != (W.shape[0],)):
        raise ValueError("linear_prepare: W must be (N, K) and b (N) or None")
    N, K = W.shape
    if K % 4:
        raise ValueError("linear_prepare: in_features %d must be a multiple of 4" % K)
    _lib.require_hip(W, b, prepared)
    nbytes = _lib.load().mmt_linear_prepared_bytes(K, N)
    if prepared is None:
        prepared = _scratch(nbytes, W.device)
    elif prepared.dtype != torch.uint8 or not prepared.is_contiguous() or prepared.numel() < nbytes or prepared.device != W.device \
            or prepared.data_ptr() % 16:
        raise ValueError("linear_prepare: prepared must be a contiguous, 16-byte aligned uint8 tensor of at least %d bytes on %s"
                         % (nbytes, W.device))
    W_, b_ = _f32c(W), _f32c(b)
    prepared._mmt_linear_kn = None                                         # not valid for any shape while it is rewritten
    _lib.launch("mmt_linear_prepare", W_, b_, prepared, prepared.numel(), K, N)
    prepared._mmt_linear_kn = (K, N)
    return prepared


def linear_prepared(x, prepared, N, act=0, rowscale=None):
    """``linear(x, W, b, act, rowscale)`` of x (M, K) with (W, b) given as ``linear_prepare(W, b)``: ONE launch, the row GEMM alone on
    the same operands, so the same bits.  Forward only."""
    _forward_only("linear_prepared", (x, rowscale))
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("linear_prepared: x must be a float32 (M, K) tensor")
    M, K = x.shape
    N = int(N)
    if rowscale is not None and rowscale.numel() != M:
        raise ValueError("linear_prepared: rowscale must hold one entry per row (%d)" % M)
    _lib.require_hip(x, prepared, rowscale)
    nbytes = _lib.load().mmt_linear_prepared_bytes(K, N)
    if not isinstance(prepared, torch.Tensor) or prepared.dtype != torch.uint8 or prepared.numel() < nbytes or prepared.device != x.device:
        raise ValueError("linear_prepared: prepared must be linear_prepare's tensor for (N, K) = (%d, %d) on %s" % (N, K, x.device))
    if getattr(prepared, "_mmt_linear_kn", None) != (K, N):
        raise ValueError("linear_prepared: prepared was laid out for (K, N) = %s, the call is for (%d, %d) (the tensor linear_prepare "
                         "returned carries its shape; a view or a copy of it does not)" % (getattr(prepared, "_mmt_linear_kn", None), K, N))
    x_, r_ = _f32c16(x), _f32c(rowscale)
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    _lib.launch("mmt_linear_forward_prepared", x_, prepared, prepared.numel(), r_, y, M, K, N, int(act))
    return y


# The LSTM decoder and the read-out, one window per call (include/mmt_hip.h mmt_decoder_stream_*): eval mode, forward only.  The state
# (prepared bf16 weights, fp32 vectors, two copies of the carried (h, c) of every layer) takes memory with any contents: _scratch.
def decoder_stream_bytes(B, d, h_dim, n_layers):
    """Bytes of the decoder stream state for ``B`` sequences, embed_dim ``d``, read-out width ``h_dim`` and ``n_layers`` LSTM layers
    (0: the read-out alone); ValueError, naming the limit, for a shape outside the step kernel's domain."""
    return _stream_bytes("mmt_decoder_stream_bytes", "%s", b"decoder stream: ?", int(B), int(d), int(h_dim), int(n_layers))


def decoder_stream_state(B, d, h_dim, n_layers, device):
    """An unprepared decoder stream state on ``device`` (uint8; any contents)."""
    return _scratch(decoder_stream_bytes(B, d, h_dim, n_layers), device)


def decoder_stream_prepare(lstm_params, dec_h0, dec_c0, out_params, state, B, d, h_dim, n_layers):
    """Convert and copy every parameter of a decoder into ``state`` (one launch; the carried state is not touched): ``lstm_params`` per
    layer (weight_ih, weight_hh, bias_ih, bias_hh) of its nn.LSTM(2d, d, n_layers), ``dec_h0`` / ``dec_c0`` (n_layers, 1, d) or
    (n_layers, d) (all three empty / None when n_layers == 0), ``out_params`` (W1 (h_dim, d), b1, W2 (1, h_dim), b2) of the read-out.
    Again after any parameter changes: a step reads every one of them from the state."""
    op = "decoder_stream_prepare"
    L, d, h_dim = int(n_layers), int(d), int(h_dim)
    lstm = [q for layer in (lstm_params or []) for q in layer]
    out = list(out_params)
    init = [dec_h0, dec_c0] if L else []
    _forward_only(op, lstm + out + init, _PARAMS_GRAD)
    nbytes = decoder_stream_bytes(B, d, h_dim, L)
    want = [s for l in range(L) for s in ((4 * d, 2 * d if l == 0 else d), (4 * d, d), (4 * d,), (4 * d,))]
    if [tuple(q.shape) for q in lstm] != want:
        raise ValueError("%s: the LSTM's parameters have the shapes %s, expected %s (nn.LSTM(2d, d, n_layers))"
                         % (op, [tuple(q.shape) for q in lstm], want))
    if any(q is None or q.numel() != L * d for q in init):
        raise ValueError("%s: dec_h0 and dec_c0 must hold n_layers x d = %d values each" % (op, L * d))
    want = [(h_dim, d), (h_dim,), (1, h_dim), (1,)]
    if [tuple(q.shape) for q in out] != want:
        raise ValueError("%s: the read-out's parameters have the shapes %s, expected %s" % (op, [tuple(q.shape) for q in out], want))
    _lib.require_hip(state, *lstm, *out, *init)
    _stream_state(op, state, nbytes, out[0].device, "decoder_stream_state")
    keep = [_f32c(q) for q in lstm + init + out]                           # alive until the launch is enqueued
    pl = (ctypes.c_void_p * max(len(lstm), 1))(*[q.data_ptr() for q in keep[:len(lstm)]]) if L else None
    h0, c0 = (keep[len(lstm)], keep[len(lstm) + 1]) if L else (None, None)
    W1, b1, W2, b2 = keep[len(lstm) + len(init):]
    _lib.launch("mmt_decoder_stream_prepare", pl, h0, c0, W1, b1, W2, b2, state, state.numel(), int(B), d, h_dim, L)


def _decoder_step(op, e_t, mask_t, state, d, h_dim, n_layers, t=None, positions=None, limit=None, advance=True):
    """Both forms of the decoder step: the position is ``t``, by value, or ``positions`` on the device with their ``limit``."""
    _forward_only(op, (e_t, mask_t))
    if not isinstance(e_t, torch.Tensor) or e_t.dim() != 2 or e_t.dtype != torch.float32 or e_t.shape[1] != int(d):
        raise ValueError("%s: e_t must be a float32 (B, %d) tensor, got %s %s"
                         % (op, int(d), getattr(e_t, "dtype", type(e_t).__name__), tuple(getattr(e_t, "shape", ()))))
    B, dev = e_t.shape[0], e_t.device
    m_ = _step_mask(op, mask_t, B, dev)
    where = _step_where(op, t, positions, limit, advance, B, dev)
    return _run_step(op, "mmt_" + op, e_t, m_, (B, 1), state, lambda: decoder_stream_bytes(B, d, h_dim, n_layers), "decoder_stream_state",
                     where, (int(d), int(h_dim), int(n_layers)))


def decoder_stream_step(e_t, mask_t, state, t, d, h_dim, n_layers):
    """Window t of the LSTM decoder and the read-out: e_t (B, d), the encoder's row of this window; mask_t (B) or None -> y_t (B, 1) =
    what ``_DecoderMixin._decode`` gives at [:, t] in eval mode, times mask_t (transformer/SFT/multiTransformer.py:463-483), from the
    (h, c) of every layer carried in ``state`` (decoder_stream_state, prepared by decoder_stream_prepare), which this call advances.
    Steps of a recording run in order t = 0, 1, ...; t is passed by value.  One launch.  Forward only."""
    return _decoder_step("decoder_stream_step", e_t, mask_t, state, d, h_dim, n_layers, t=int(t))


def decoder_stream_step_slots(e_t, mask_t, state, positions, d, h_dim, n_layers, limit=None, advance=True):
    """``decoder_stream_step`` with the position of every sequence in device memory (csrc/step_slots.h): ``positions`` int32 (B), read
    by the kernel.  Row b is the row of ``decoder_stream_step`` at t = positions[b], bit for bit (copy positions[b] & 1 of the carried
    state read, the other written), where the slot is seated, and zero, with nothing else written, where it is idle (negative) or full
    (>= ``limit``; None: no limit).  ``advance``: the kernel adds 1 to the position of every slot it ran.  No position crosses the host,
    so the call can be captured into a graph.  One launch."""
    return _decoder_step("decoder_stream_step_slots", e_t, mask_t, state, d, h_dim, n_layers, positions=positions, limit=limit, advance=advance)


# Prefill of a stream state (include/mmt_hip.h mmt_*_stream_prefill): its functional layer stands in streaming.py, beside
# encoder_ring_step, and these names resolve there.
_IN_STREAMING = ("encoder_stream_prefill", "decoder_stream_prefill", "prefill_table", "check_prefill_table",
                 "encoder_stream_extend", "encoder_stream_extend_slots")


def __getattr__(name):
    if name in _IN_STREAMING:
        from . import streaming
        return getattr(streaming, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


# The LSTM baseline, one window per call (include/mmt_hip.h mmt_lstm_stream_*): eval mode, forward only.  The state (prepared bf16
# weights, fp32 vectors, two copies of the carried (h, c) of every layer, the ring of the local attention) takes memory with any
# contents: _scratch.  dims = (in, E, H, n_layers, attn_len).
def lstm_stream_bytes(B, in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Bytes of the LSTM stream state for ``B`` sequences; ValueError, naming the limit, for a shape outside the step kernel's domain."""
    return _stream_bytes("mmt_lstm_stream_bytes", "%s", b"lstm stream: ?", int(B), int(in_dim), int(embed_dim), int(h_dim), int(n_layers),
                         int(attn_len))


def lstm_stream_state(B, in_dim, embed_dim, h_dim, n_layers, attn_len, device):
    """An unprepared LSTM stream state on ``device`` (uint8; any contents)."""
    return _scratch(lstm_stream_bytes(B, in_dim, embed_dim, h_dim, n_layers, attn_len), device)


def lstm_stream_prepare(embed_params, attn_params, lstm_params, dec_params, state, B, in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Convert and copy every parameter of an LSTM baseline into ``state`` (one launch; the carried state and the ring are not touched):
    ``embed_params`` (W (E, in), b), ``attn_params`` (W0 (E, E), b0, W2 (L, E), b2), ``lstm_params`` per layer (weight_ih, weight_hh,
    bias_ih, bias_hh) of its nn.LSTM(E, H, n_layers), ``dec_params`` (W0 (E, H), b0, W2 (1, E), b2) of the read-out.  Again after any
    parameter changes: a step reads every one of them from the state."""
    op = "lstm_stream_prepare"
    I, E, H, NL, L = int(in_dim), int(embed_dim), int(h_dim), int(n_layers), int(attn_len)
    nbytes = lstm_stream_bytes(B, I, E, H, NL, L)
    ps = list(embed_params) + list(attn_params) + [q for layer in lstm_params for q in layer] + list(dec_params)
    _forward_only(op, ps, _PARAMS_GRAD)
    want = [(E, I), (E,), (E, E), (E,), (L, E), (L,)]
    want += [s for l in range(NL) for s in ((4 * H, E if l == 0 else H), (4 * H, H), (4 * H,), (4 * H,))]
    want += [(E, H), (E,), (1, E), (1,)]
    if [tuple(q.shape) for q in ps] != want:
        raise ValueError("%s: the parameters have the shapes %s, expected %s" % (op, [tuple(q.shape) for q in ps], want))
    _lib.require_hip(state, *ps)
    _stream_state(op, state, nbytes, ps[0].device, "lstm_stream_state")
    keep = [_f32c(q) for q in ps]                                          # alive until the launch is enqueued
    table = (ctypes.c_void_p * len(keep))(*[q.data_ptr() for q in keep])
    _lib.launch("mmt_lstm_stream_prepare", table, state, state.numel(), int(B), I, E, H, NL, L)


def _lstm_step(op, x_t, mask_t, state, dims, t=None, positions=None, limit=None, advance=True):
    """Both forms of the LSTM step: the position is ``t``, by value, or ``positions`` on the device with their ``limit``."""
    dims = tuple(int(v) for v in dims)
    _forward_only(op, (x_t, mask_t))
    if not isinstance(x_t, torch.Tensor) or x_t.dim() != 2 or x_t.dtype != torch.float32 or x_t.shape[1] != dims[0]:
        raise ValueError("%s: x_t must be a float32 (B, %d) tensor, got %s %s"
                         % (op, dims[0], getattr(x_t, "dtype", type(x_t).__name__), tuple(getattr(x_t, "shape", ()))))
    B, dev = x_t.shape[0], x_t.device
    m_ = _step_mask(op, mask_t, B, dev)
    where = _step_where(op, t, positions, limit, advance, B, dev)
    return _run_step(op, "mmt_" + op, x_t, m_, (B, 1), state, lambda: lstm_stream_bytes(B, *dims), "lstm_stream_state", where, dims)


def lstm_stream_step(x_t, mask_t, state, t, in_dim, embed_dim, h_dim, n_layers, attn_len):
    """Window t of the LSTM baseline: x_t (B, in); mask_t (B) or None -> y_t (B, 1) = what ``_LocalAttnLSTM.forward`` gives at [:, t] in
    eval mode with ``attend_over_taps`` on, from the (h, c) of every layer and the ring of the last attn_len outputs carried in ``state``
    (lstm_stream_state, prepared by lstm_stream_prepare), which this call advances.  Steps of a recording run in order t = 0, 1, ...; t
    is passed by value.  One launch.  Forward only."""
    return _lstm_step("lstm_stream_step", x_t, mask_t, state, (in_dim, embed_dim, h_dim, n_layers, attn_len), t=int(t))


def lstm_stream_step_slots(x_t, mask_t, state, positions, in_dim, embed_dim, h_dim, n_layers, attn_len, limit=None, advance=True):
    """``lstm_stream_step`` with the position of every sequence in device memory (csrc/step_slots.h): ``positions`` int32 (B), read by
    the kernel.  Row b is the row of ``lstm_stream_step`` at t = positions[b], bit for bit, where the slot is seated, and zero, with
    nothing else written, where it is idle (negative) or full (>= ``limit``; None: no limit).  ``advance``: the kernel adds 1 to the
    position of every slot it ran.  No position crosses the host, so the call can be captured into a graph.  One launch."""
    return _lstm_step("lstm_stream_step_slots", x_t, mask_t, state, (in_dim, embed_dim, h_dim, n_layers, attn_len), positions=positions,
                      limit=limit, advance=advance)


def check_device_errors():
    """Synchronise and raise if an asynchronous kernel reported an error through its device error word (mmt_hip.h)."""
    _lib.ERRORS.check()


def poison_lds(device, pattern=0x7FC00000):
    """Test hook: leave `pattern` in every LDS word of every CU (see include/mmt_hip.h)."""
    sink = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.launch("mmt_debug_poison_lds", int(pattern), sink)


def _attn_mask_words(p, seed, stream_id, nbh, nt, device, lanes=False):
    """Test hook: the attention-dropout generator's stored words (lq, lk), each a (nbh * nt * nt, 64) int16 tensor of raw uint16 words:
    lq in the lane-word form, or with `lanes` in the lane-mask form the plain d_k = 16 forward reads; lk in the lane-word form."""
    lq = torch.empty(nbh * nt * nt, 64, dtype=torch.int16, device=device)
    lk = torch.empty_like(lq)
    _lib.launch("mmt_debug_attn_mask_words", float(p), int(seed), int(stream_id), int(nbh), int(nt), int(bool(lanes)), lq, lk)
    return lq, lk


def dropout_mask(p, seed, stream_id, n, device, attn_Tp=0):
    """Test hook: (keep mask as a bool tensor of n entries, scale of kept values) of one dropout stream."""
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    sc = ctypes.c_float(0.0)
    _lib.launch("mmt_debug_dropout_mask", float(p), int(seed), int(stream_id), int(n), int(attn_Tp), keep,
                ctypes.cast(ctypes.pointer(sc), ctypes.c_void_p))
    return keep.bool(), float(sc.value)
