"""Drop-in for the reference's ``models.py`` window-encoder front-end: ``CNN``, ``Highway`` and the
``MultiCNNTransformer`` wrappers of the three Transformer variants — same class names, constructor arguments,
``forward(inputs, length, mask)`` contract and ``state_dict`` keys (so reference checkpoints load unchanged):

    transformer/SFT/models.py:27-142      early fusion: concat -> tanh(fusionLayer) -> NLPTransformer   (``MultiCNNTransformer``)
    transformer/MFT/models.py:27-138      per-modality dict -> MultiTransformer (MFN gate)               (``MultiCNNTransformerMFT``)
    transformer/B2-Trans/models.py:27-134 single modality -> UniFullTransformer                           (``MultiCNNTransformerB2``)
    transformer/B3-MFN/models.py:81-138   per-modality dict -> MultiTransformerB3 (Linear embed, MFN gate) (``MultiCNNTransformerB3``)
    transformer/B1-LSTM/models.py:79-133  ReLU Highway, concat -> MultiLSTM with local attention           (``MultiCNNLSTM``)

and the two copies of the LSTM baseline's sequence model: ``MultiLSTM`` (transformer/SFT/models.py:144-225, byte-identical in MFT,
B2-Trans, B3-MFN and Performance-Eval) and ``MultiLSTMB1`` (transformer/B1-LSTM/models.py:135-216), and the encoder-decoder LSTM
``MultiEDLSTM`` (transformer/MFT/models.py:222-308) and the LSTM baseline with an autoregressive read-out ``MultiARLSTM``
(transformer/MFT/models.py:310-400).

The reference walks the batch in a Python loop (SFT/models.py:123) and runs Conv1d + MaxPool1d per sequence; windows are
independent, so here all B*T windows of a modality go through ONE fused conv-GEMM + max-pool HIP kernel
(``csrc/convpool.h``), the Highway layer through the row GEMM, and the modalities on concurrent streams.
There is no CPU path.
"""
import torch
import torch.nn as nn

from . import _lib, functional as F_hip
from .streaming import (LSTMFeedbackSlotStream, LSTMFeedbackStream, LSTMSlotStream, LSTMStream, _SequenceSlotStream, _SequenceStream,
                        _prefill_at_zero, check_prefill_table)
from .multiTransformer import (MultiTransformer, MultiTransformerB3, NLPTransformer, UniFullTransformer, UniTransformer, _MOD_STREAMS,
                               _hip_device, _stream_model_checks)


class Highway(nn.Module):
    """x_gate * proj(x) + (1 - x_gate) * x with a LINEAR projection (the reference applies no ReLU) — SFT/models.py:27-55."""

    def __init__(self, word_embed_size):
        super().__init__()
        self.word_embed_size = word_embed_size
        self.linear_projection = nn.Linear(word_embed_size, word_embed_size, bias=True)
        self.linear_gate = nn.Linear(word_embed_size, word_embed_size, bias=True)

    def forward(self, x_conv_out, dropout_p=0.0, seed=0):
        """``dropout_p`` / ``seed``: the front-end's Dropout(0.3) on the Highway output (SFT/models.py:132-134), fused into the combine"""
        return F_hip.highway(x_conv_out, self.linear_projection.weight, self.linear_projection.bias,
                             self.linear_gate.weight, self.linear_gate.bias, dropout_p, seed)       # drop(gate*proj + (1-gate)*x)


class HighwayB1(Highway):
    """The B1-LSTM variant's Highway: x_gate * ReLU(proj(x)) + (1 - x_gate) * x — transformer/B1-LSTM/models.py:27-55 (:52 applies the
    ReLU the other variants' Highway omits).  Same keys as ``Highway``; the ReLU rides in the projection GEMM's epilogue."""

    def forward(self, x_conv_out, dropout_p=0.0, seed=0):
        return F_hip.highway(x_conv_out, self.linear_projection.weight, self.linear_projection.bias,
                             self.linear_gate.weight, self.linear_gate.bias, dropout_p, seed, proj_act=1)


class CNN(nn.Module):
    """Conv1d(word_embed_size -> window_embed_size, k) + max over all positions — SFT/models.py:57-79.
    ``forward`` takes the reference's (batch, word_embed_size, window_length) layout; ``forward_windows`` takes the
    natural (N, window_length, word_embed_size) rows that the kernel reads (no permute copy)."""

    def __init__(self, word_embed_size=300, window_embed_size=128, k=2):
        super().__init__()
        self.k = k
        self.f = window_embed_size
        self.word_embed_size = word_embed_size
        self.window_embed_size = window_embed_size
        self.conv1d = nn.Conv1d(word_embed_size, window_embed_size, k, bias=True)

    def forward_windows(self, x):
        if self.k == 2:
            out, _ = F_hip.conv_maxpool(x, self.conv1d.weight, self.conv1d.bias)
            return out
        if not 1 <= self.k <= F_hip.CONV_K_MAX:
            raise NotImplementedError("CNN: kernel sizes 1..%d are implemented on the HIP path, got k=%d" % (F_hip.CONV_K_MAX, self.k))
        out, _ = F_hip.conv_maxpool_k(x, self.conv1d.weight, self.conv1d.bias)
        return out

    def forward(self, x_reshape):
        return self.forward_windows(x_reshape.permute(0, 2, 1).contiguous())


class _FrontEnd(nn.Module):
    window_embed_size = {"linguistic": 300, "emotient": 20, "acoustic": 256, "image": 256}     # SFT/models.py:90
    _highway_cls = Highway

    def _build(self, mods, dims, k):
        self.mods = mods
        self.dims = dims
        self.CNN, self.Highway = {}, {}
        total = 0
        for mod in mods:
            self.CNN[mod] = CNN(dims[mod], self.window_embed_size[mod], k)
            self.Highway[mod] = self._highway_cls(self.window_embed_size[mod])
            self.add_module("cnn_{}".format(mod), self.CNN[mod])
            self.add_module("highway_{}".format(mod), self.Highway[mod])
            total += self.window_embed_size[mod]
        return total

    def _encode(self, inputs):
        """{mod: (B,T,W,D)} -> {mod: (B,T,F_mod)}: conv+pool, Highway, Dropout(0.3), one stream per modality."""
        outs = {}
        p = float(self.dropout.p) if self.training else 0.0
        main, streams = _MOD_STREAMS.begin(self.device, len(self.mods))
        for i, (mod, st) in enumerate(zip(self.mods, streams)):
            with torch.cuda.stream(st):
                x = inputs[mod]
                B, T, W, D = x.shape
                e = self.CNN[mod].forward_windows(x.reshape(B * T, W, D))
                seed = _lib.next_dropout_seed(x.device, 6, holder=self, index=i) if p > 0.0 else 0      # one seed state per modality stream
                e = self.Highway[mod](e, p, seed)
                outs[mod] = e.reshape(B, T, -1)
        _MOD_STREAMS.end(main, streams, list(outs.values()))
        return outs


class _FrontEndStream:
    """``stream()`` of the MultiCNNTransformer wrappers: ``step({mod: (B, W, d_raw)}, mask_t)`` -> the (B,1) prediction of that window.
    The window encoder runs on a T = 1 batch (``_encode``), then the fusion layer where the model has one, then the sequence model's
    own step (``streaming._SequenceStream``; the MFT and B3-MFN take the per-modality rows as a dict: ``streaming._GateStream``).  ``reset()`` starts a new recording."""

    def __init__(self, model, batch, capacity, method="stream", seq=None):
        """``method``: the sequence model's method that opens its stream, "stream", "slot_stream" or "device_stream".  ``seq``: the
        sequence model's stream, already open (``streaming.ring_stream``)."""
        _stream_model_checks(model)
        self.model, self.batch = model, int(batch)
        seq_model = getattr(model, "Transformer", None)
        if seq is not None:
            self.seq = seq
        elif seq_model is None:                                 # MultiCNNLSTM: the sequence model is .LSTM, which has no cache, so no capacity
            self.seq = getattr(model.LSTM, method)(batch, capacity)
        else:
            self.seq = getattr(seq_model, method)(batch, capacity)

    t = property(lambda self: self.seq.t)                   # a slots stream: AttributeError naming .positions
    capacity = property(lambda self: self.seq.capacity)
    # with slots (``slot_stream``): the members of streaming._Slots, those of the sequence model's stream
    slots = property(lambda self: self.seq.slots)
    positions = property(lambda self: self.seq.positions)

    def seat(self, indices):
        self.seq.seat(indices)

    def release(self, indices):
        self.seq.release(indices)

    def full(self):
        return self.seq.full()

    def reset(self):
        self.seq.reset()

    def refresh(self):
        """Convert the sequence model's current parameters again, where its stream keeps converted copies (the MFT, the B3-MFN and every
        ``device_stream``; the window encoder itself reads the live parameters)."""
        if not hasattr(self.seq, "refresh"):                 # streaming._SequenceStream packs the decoder's weights when it is opened
            raise NotImplementedError("%s.stream: the stream of %s has no refresh() (it packs the decoder's weights once, when it is "
                                      "opened): open a new stream after a parameter changed, or use device_stream, whose refresh() "
                                      "follows it" % (type(self.model).__name__, type(self.seq).__name__))
        self.seq.refresh()

    def step(self, inputs, mask_t=None):
        m, B = self.model, self.batch
        for mod in m.mods:
            x = inputs[mod]
            if x.dim() != 3 or x.shape[0] != B:
                raise ValueError("%s stream step: inputs[%r] must have the shape (%d, W, d_raw), got %s"
                                 % (type(m).__name__, mod, B, tuple(x.shape)))
        with torch.no_grad():
            outs = m._encode({mod: inputs[mod].unsqueeze(1) for mod in m.mods})           # {mod: (B,1,F_mod)}
            if getattr(self.seq, "takes_modalities", False):                              # the MFT and B3-MFN: no fusion, one row per modality
                return self.seq.step({mod: outs[mod].reshape(B, -1) for mod in m.mods}, mask_t)
            if len(m.mods) > 1:
                x = F_hip.cat_cols([outs[mod] for mod in m.mods])
                if getattr(m, "fusionLayer", None) is not None:
                    x = F_hip.linear(x, m.fusionLayer.weight.detach(), m.fusionLayer.bias.detach(), act=2)   # tanh, SFT/models.py:138
            else:
                x = outs[m.mods[0]]
            return self.seq.step(x.reshape(B, -1), mask_t)

    def prefill(self, *args, mask=None):
        """Open recordings from their histories in ONE forward (``streaming._SequenceStream.prefill`` behind the window encoder and the
        fusion, run as ``forward`` runs them).  A host stream: ``prefill({mod: (B, P, W, d_raw)}, mask=None)`` -> (B, P, 1), requires
        ``t == 0``.  With slots (``device_stream``): ``prefill(indices, {mod: (k, P, W, d_raw)}, lengths, mask=None)`` -> (k, P, 1).
        The MFT, B3-MFN and the LSTM baselines behind the window encoder: NotImplementedError (their streams say why)."""
        m, seq = self.model, self.seq
        if not isinstance(seq, (_SequenceStream, _SequenceSlotStream)):
            return seq.prefill()                                 # NotImplementedError, before any launch
        op = "%s stream prefill" % type(m).__name__
        slots = isinstance(seq, _SequenceSlotStream)
        if len(args) != (3 if slots else 1):
            raise ValueError("%s: %s" % (op, "a stream with slots takes (indices, inputs, lengths)" if slots else "a host stream takes (inputs)"))
        inputs = args[1] if slots else args[0]
        k = len(args[0]) if slots and hasattr(args[0], "__len__") else self.batch
        if not isinstance(inputs, dict) or any(mod not in inputs for mod in m.mods):
            raise ValueError("%s: inputs must be a dict with an entry for every modality %s" % (op, list(m.mods)))
        P = None
        for mod in m.mods:
            x = inputs[mod]
            if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[0] != k or x.shape[1] < 1 or (P is not None and x.shape[1] != P):
                raise ValueError("%s: inputs[%r] must have the shape (%d, P, W, d_raw) with one P >= 1 for every modality, got %s"
                                 % (op, mod, k, tuple(getattr(x, "shape", ()))))
            P = x.shape[1]
        if seq.capacity is not None and P > seq.capacity:
            raise ValueError("%s: P = %d windows > capacity = %d: open a stream with a larger capacity" % (op, P, seq.capacity))
        if slots:
            check_prefill_table(op, args[0], args[2], P, self.batch, seq.capacity)
        else:
            _prefill_at_zero(op, seq.t)
        with torch.no_grad():
            outs = m._encode({mod: inputs[mod] for mod in m.mods})                          # {mod: (k,P,F_mod)}
            if len(m.mods) > 1:
                x = F_hip.cat_cols([outs[mod] for mod in m.mods])
                if getattr(m, "fusionLayer", None) is not None:
                    x = F_hip.linear(x, m.fusionLayer.weight.detach(), m.fusionLayer.bias.detach(), act=2)
            else:
                x = outs[m.mods[0]]
            return seq.prefill(args[0], x, args[2], mask) if slots else seq.prefill(x, mask)

    def extend(self, inputs, mask=None):
        """Move the recording forward by C windows from ANY ``t`` (``streaming._SequenceStream.extend`` behind the window encoder and
        the fusion, run as ``forward`` runs them): ``extend({mod: (B, C, W, d_raw)}, mask=None)`` -> (B, C, 1); afterwards ``t += C``.
        Every other sequence stream behind the window encoder (the MFT, B3-MFN, the LSTM baselines, ``device_stream``):
        NotImplementedError naming ``step`` (their streams say why)."""
        m, seq = self.model, self.seq
        if not isinstance(seq, _SequenceStream):
            return seq.extend()                                  # NotImplementedError, before any launch
        op = "%s stream extend" % type(m).__name__
        _stream_model_checks(m, "stream extend")
        if not isinstance(inputs, dict) or any(mod not in inputs for mod in m.mods):
            raise ValueError("%s: inputs must be a dict with an entry for every modality %s" % (op, list(m.mods)))
        C = None
        for mod in m.mods:
            x = inputs[mod]
            if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[0] != self.batch or x.shape[1] < 1 or (C is not None and x.shape[1] != C):
                raise ValueError("%s: inputs[%r] must have the shape (%d, C, W, d_raw) with one C >= 1 for every modality, got %s"
                                 % (op, mod, self.batch, tuple(getattr(x, "shape", ()))))
            C = x.shape[1]
        if seq.capacity is not None and seq.t + C > seq.capacity:
            raise ValueError("%s: t + C = %d + %d windows > capacity = %d: open a stream with a larger capacity (a ring stream has no limit)"
                             % (op, seq.t, C, seq.capacity))
        with torch.no_grad():
            outs = m._encode({mod: inputs[mod] for mod in m.mods})                          # {mod: (B,C,F_mod)}
            if len(m.mods) > 1:
                x = F_hip.cat_cols([outs[mod] for mod in m.mods])
                if getattr(m, "fusionLayer", None) is not None:
                    x = F_hip.linear(x, m.fusionLayer.weight.detach(), m.fusionLayer.bias.detach(), act=2)
            else:
                x = outs[m.mods[0]]
            return seq.extend(x, mask)


class MultiCNNTransformer(_FrontEnd):
    """SFT: transformer/SFT/models.py:81-142."""

    def __init__(self, mods, dims, fuse_embed_size=512, k=2, device=torch.device("cuda:0")):
        super().__init__()
        total = self._build(mods, dims, k)
        self.fusionLayer = nn.Linear(total, fuse_embed_size)
        if len(mods) > 1:
            self.Transformer = NLPTransformer(fuse_embed_size, device=device)
        else:
            self.Transformer = UniTransformer(total, device=device)
        self.dropout = nn.Dropout(p=0.3)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, length, mask=None):
        outs = self._encode(inputs)
        if len(self.mods) > 1:
            cat = F_hip.cat_cols([outs[m] for m in self.mods])
            fused = F_hip.linear(cat, self.fusionLayer.weight, self.fusionLayer.bias, act=2)      # tanh, :138
            return self.Transformer(fused, mask, length)
        return self.Transformer(outs[self.mods[0]], mask, length)

    def stream(self, batch, capacity):
        """This model as an online predictor (``_FrontEndStream``): eval mode, ``causal_attention(model)`` on."""
        return _FrontEndStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """Not implemented: the sequence model keeps host-side state per recording (its own ``slot_stream`` says why)."""
        return self.Transformer.slot_stream(batch, capacity)

    def device_stream(self, batch, capacity):
        """``stream(batch, capacity)`` with the sequence model's whole per-recording state on the device (its ``device_stream``): sequences
        are seated and released independently, and a step can be captured into a graph (``graphs.capture_stream``)."""
        return _FrontEndStream(self, batch, capacity, "device_stream")


class MultiCNNTransformerMFT(_FrontEnd):
    """MFT: transformer/MFT/models.py:81-138 (``embed_dims`` replaces the fixed window embed sizes; no fusion layer)."""

    def __init__(self, mods, dims, embed_dims, fuse_embed_size=256, k=2, device=torch.device("cuda:0")):
        super().__init__()
        self.window_embed_size = embed_dims
        total = self._build(mods, dims, k)
        if len(mods) > 1:
            self.Transformer = MultiTransformer(mods=mods, window_embed_size=self.window_embed_size, device=device)
        else:
            self.Transformer = UniTransformer(total, device=device)
        self.dropout = nn.Dropout(p=0.3)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, length, mask=None):
        outs = self._encode(inputs)
        if len(self.mods) > 1:
            return self.Transformer(outs, mask, length)
        return self.Transformer(outs[self.mods[0]], mask, length)

    def stream(self, batch, capacity):
        """One modality: the UniTransformer's stream behind the window encoder.  More: NotImplementedError (the MFN gate)."""
        if len(self.mods) > 1:
            raise NotImplementedError("MultiCNNTransformerMFT.stream: with more than one modality the sequence model is the MFT, whose "
                                      "MFN gate (per-modality LSTM cells and the delta-memory) needs a stepping state of its own; not "
                                      "implemented (a single-modality model streams)")
        return _FrontEndStream(self, batch, capacity)

    def stream_modalities(self, batch, capacity):
        """More than one modality: the MFT's stream (``MultiTransformer.stream``) behind the window encoder, ``step({mod: (B, W, d_raw)},
        mask_t)`` -> (B,1).  Eval mode, ``causal_attention(model)`` on.  One modality: ValueError, ``stream`` serves that model."""
        if len(self.mods) < 2:
            raise ValueError("MultiCNNTransformerMFT.stream_modalities: with one modality the sequence model is the UniTransformer, not "
                             "the MFT: call stream(batch, capacity)")
        return _FrontEndStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """``stream_modalities(batch, capacity)`` with slots: sequences are seated and released independently (``.positions``,
        ``.seat``, ``.release``, ``.full``: streaming._Slots), and a step can be captured into a graph
        (``graphs.capture_stream``).  One modality: NotImplementedError, the UniTransformer keeps host-side state per recording."""
        return _FrontEndStream(self, batch, capacity, "slot_stream")

    def device_stream(self, batch, capacity):
        """One modality: the UniTransformer's ``device_stream`` behind the window encoder (its whole per-recording state on the device:
        sequences are seated and released independently, a step can be captured).  More: NotImplementedError, ``slot_stream`` serves
        the MFT."""
        if len(self.mods) > 1:
            raise NotImplementedError("MultiCNNTransformerMFT.device_stream: with more than one modality the sequence model is the MFT, whose slots "
                                      "stream is slot_stream(batch, capacity)")
        return _FrontEndStream(self, batch, capacity, "device_stream")


class MultiCNNTransformerB2(_FrontEnd):
    """B2-Trans: transformer/B2-Trans/models.py:81-134 (single modality; the fusion layer is commented out there)."""

    def __init__(self, mods, dims, fuse_embed_size=512, k=2, device=torch.device("cuda:0")):
        super().__init__()
        total = self._build(mods, dims, k)
        self.Transformer = UniFullTransformer(total, device=device)
        self.dropout = nn.Dropout(p=0.3)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, length, mask=None):
        outs = self._encode(inputs)
        if len(outs) > 1:
            return self.Transformer(F_hip.cat_cols([outs[m] for m in self.mods]), mask, length)
        return self.Transformer(outs[self.mods[0]], mask, length)

    def stream(self, batch, capacity):
        """This model as an online predictor (``_FrontEndStream``): eval mode, ``causal_attention(model)`` on."""
        return _FrontEndStream(self, batch, capacity)

    def slot_stream(self, batch, capacity):
        """Not implemented: the sequence model keeps host-side state per recording (its own ``slot_stream`` says why)."""
        return self.Transformer.slot_stream(batch, capacity)

    def device_stream(self, batch, capacity):
        """``stream(batch, capacity)`` with the sequence model's whole per-recording state on the device (its ``device_stream``): sequences
        are seated and released independently, and a step can be captured into a graph (``graphs.capture_stream``)."""
        return _FrontEndStream(self, batch, capacity, "device_stream")


class MultiCNNTransformerB3(_FrontEnd):
    """B3-MFN: transformer/B3-MFN/models.py:81-138 — the MFT front-end with the fixed window embed sizes of SFT and the B3 sequence model
    (Linear embed -> MFN gate, no encoder stacks)."""

    def __init__(self, mods, dims, fuse_embed_size=256, k=2, device=torch.device("cuda:0")):
        super().__init__()
        total = self._build(mods, dims, k)
        if len(mods) > 1:
            self.Transformer = MultiTransformerB3(mods=mods, window_embed_size=self.window_embed_size, device=device)
        else:
            self.Transformer = UniTransformer(total, device=device)
        self.dropout = nn.Dropout(p=0.3)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, length, mask=None):
        outs = self._encode(inputs)
        if len(self.mods) > 1:
            return self.Transformer(outs, mask, length)
        return self.Transformer(outs[self.mods[0]], mask, length)

    def stream(self, batch, capacity=None):
        """This model as an online predictor (``_FrontEndStream``): eval mode.  More than one modality: B3-MFN has no attention, so no
        cache, no length limit and no need for ``causal_attention``.  One modality: the UniTransformer's stream, which needs both."""
        if len(self.mods) < 2 and capacity is None:
            raise ValueError("MultiCNNTransformerB3.stream: with one modality the sequence model is the UniTransformer, whose K/V cache "
                             "needs a capacity (windows per recording)")
        return _FrontEndStream(self, batch, capacity)

    def slot_stream(self, batch, capacity=None):
        """``stream(batch)`` with slots: sequences are seated and released independently (``.positions``, ``.seat``, ``.release``,
        ``.full``: streaming._Slots), and a step can be captured into a graph (``graphs.capture_stream``).  One modality:
        NotImplementedError, the UniTransformer keeps host-side state per recording."""
        return _FrontEndStream(self, batch, capacity, "slot_stream")

    def device_stream(self, batch, capacity=None):
        """One modality: the UniTransformer's ``device_stream`` behind the window encoder (its whole per-recording state on the device:
        sequences are seated and released independently, a step can be captured).  More: NotImplementedError, ``slot_stream`` serves
        the B3-MFN."""
        if len(self.mods) > 1:
            raise NotImplementedError("MultiCNNTransformerB3.device_stream: with more than one modality the sequence model is the B3-MFN, whose slots "
                                      "stream is slot_stream(batch)")
        if capacity is None:
            raise ValueError("MultiCNNTransformerB3.device_stream: with one modality the sequence model is the UniTransformer, whose K/V "
                             "cache needs a capacity (windows per recording)")
        return _FrontEndStream(self, batch, capacity, "device_stream")


def attend_over_taps(module, on=True):
    """Set ``over_taps`` on every LSTM baseline (``_LocalAttnLSTM``: MultiLSTM, MultiLSTMB1, MultiEDLSTM, MultiARLSTM, and MultiCNNLSTM
    through its ``.LSTM``) at or below ``module`` -> {qualified name: module}.  From the next forward on the local attention's softmax
    normalises the L taps of each step (``functional.local_attention(..., over="taps")``), forward and backward, what the reference's
    own comment describes, instead of each tap's column over all T steps of the padded batch (what its ``nn.Softmax(dim=1)`` computes).
    The output at step t then depends on steps <= t alone and no longer on the padded length, which is what lets these models run as
    online predictors (``stream`` / ``slot_stream``).  Outputs then differ from the reference's, by design; a model is trained with
    the flag it is used with.  Off by default; ``attend_over_taps(module, False)`` restores the reference's semantics."""
    found = {}
    for name, m in module.named_modules():
        if isinstance(m, _LocalAttnLSTM):
            m.over_taps = bool(on)
            found[name] = m
    return found


class _LocalAttnLSTM(nn.Module):
    """The LSTM baseline's sequence model, shared by both copies:

        embed   = ReLU(Linear(Dropout(p_in)(x)))                                  (B,T,E)    one row-GEMM, input dropout in its staging
        z       = Linear(E->L)(ReLU(Linear(E->E)(embed)))                         (B,T,L)    the attention MLP  } one node on the
        gx      = embed W_ih^T + (b_ih + b_hh)                                    (T,B,4H)   time-major for the scan } time-major embed
        h       = LSTM scan of gx with zero h0 / c0                               (T,B,H)
                  n_layers > 1: layer l scans h^{l-1} W_ih_l^T + (b_ih_l + b_hh_l); the top layer is h
        context = convolve(h * mask, softmax over TIME of z)                      (B,T,H)    functional.local_attention
        out     = Linear(E->1)(ReLU(Linear(H->E)(context)) [Dropout]) * mask      (B,T,1)

    pack_padded_sequence / pad_packed_sequence are not needed: the LSTM is causal, so the scan over all T steps gives the same h at
    real steps, and local_attention zeroes it at padded ones (outputs and gradients are those of the packed run).  The attention
    softmax normalises each of the L columns over all T steps of the padded batch (nn.Softmax(dim=1) on (B,T,L) logits), so outputs
    at real steps depend on the padded length, as in the reference.  With ``attend_over_taps(model)`` on (``over_taps``) the softmax
    normalises the L taps of each step instead, and the model can be stepped one window at a time (``stream`` / ``slot_stream``)."""

    _embed_p = 0.1
    _dec_dropout = None
    over_taps = False                  # set by attend_over_taps(): the softmax over the taps of a step, not over time

    def __init__(self, window_embed_size, embed_dim, h_dim=256, n_layers=1, attn_len=5, device=torch.device("cuda:0")):
        super().__init__()
        self.embed_dim = embed_dim
        self.h_dim = h_dim
        self.n_layers = n_layers
        self.attn_len = attn_len
        self.embed = nn.Sequential(nn.Dropout(self._embed_p), nn.Linear(window_embed_size, embed_dim), nn.ReLU())
        self.attn = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, attn_len), nn.Softmax(dim=1))
        self.lstm = nn.LSTM(embed_dim, h_dim, n_layers, batch_first=True)
        if self._dec_dropout is None:
            self.decoder = nn.Sequential(nn.Linear(h_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, 1))
        else:
            self.decoder = nn.Sequential(nn.Linear(h_dim, embed_dim), nn.ReLU(), nn.Dropout(self._dec_dropout), nn.Linear(embed_dim, 1))
        self.device = _hip_device(device)
        self.to(self.device)

    def _front(self, inputs, mask, lengths, lstm, h0=None, c0=None):
        """embed -> attention logits and LSTM scan -> local attention: (B,T,H) context.  ``lstm``: the nn.LSTM that reads the embedding;
        h0 / c0: its initial state rows (n_layers,1,H) broadcast over the batch, or None for zeros (then nothing is launched for them)."""
        B, T = inputs.shape[0], inputs.shape[1]
        if len(lengths) != B or int(max(lengths)) != T:
            raise ValueError("%s: the input's time axis (%d) must equal max(lengths) and len(lengths) the batch (%d); got lengths %s"
                             % (type(self).__name__, T, B, list(lengths)))
        if mask is None:
            raise ValueError("%s: the (B,T,1) mask is required (the reference multiplies the output by it)" % type(self).__name__)
        p_in = float(self.embed[0].p) if self.training else 0.0
        seed = _lib.next_dropout_seed(inputs.device, 7, holder=self) if p_in > 0.0 else 0
        embed = F_hip.linear(inputs, self.embed[1].weight, self.embed[1].bias, act=1, in_dropout=p_in, seed=seed)
        # both consumers of the embedding read it time-major (one gradient node for it: no library add in the backward); the attention
        # MLP's (T,B,L) logits go back to batch-major, a copy of B*T*L floats
        hid, gx = F_hip.linear_pair(F_hip.time_major(embed), self.attn[0].weight, self.attn[0].bias,
                                    lstm.weight_ih_l0, F_hip.add2(lstm.bias_ih_l0, lstm.bias_hh_l0), act1=1)
        z = F_hip.batch_major(F_hip.linear(hid, self.attn[2].weight, self.attn[2].bias))

        hb, cb = (None if rows is None else F_hip.broadcast_layers(rows, B) for rows in (h0, c0))      # (n_layers,B,H)

        def init(t, l):                                 # one layer: a view (indexing a layer would put a library kernel into the backward)
            return None if t is None else (t.view(B, -1) if self.n_layers == 1 else t[l])
        h_all, _ = F_hip.lstm_scan(gx, lstm.weight_hh_l0, init(hb, 0), init(cb, 0))
        for l in range(1, self.n_layers):               # nn.LSTM's upper layers read the layer below: independent scans, rows stay time-major
            gx = F_hip.linear(h_all, getattr(lstm, "weight_ih_l%d" % l),
                              F_hip.add2(getattr(lstm, "bias_ih_l%d" % l), getattr(lstm, "bias_hh_l%d" % l)))
            h_all, _ = F_hip.lstm_scan(gx, getattr(lstm, "weight_hh_l%d" % l), init(hb, l), init(cb, l))
        return F_hip.local_attention(z, h_all, mask, over="taps" if self.over_taps else "time")

    def forward(self, inputs, mask, lengths, target=None, output_feats=False):
        context = self._front(inputs, mask, lengths, self.lstm)
        dec0, last = self.decoder[0], self.decoder[-1]
        p_dec = float(self.decoder[2].p) if (self.training and self._dec_dropout is not None) else 0.0
        seed_dec = _lib.next_dropout_seed(inputs.device, 8, holder=self) if p_dec > 0.0 else 0
        hid = F_hip.linear(context, dec0.weight, dec0.bias, act=1, out_dropout=p_dec, seed=seed_dec)
        return F_hip.linear(hid, last.weight, last.bias, rowscale=mask.float().reshape(-1))

    def _stream_refusals(self, method):
        """What cannot stream, before anything is opened or launched."""
        _stream_model_checks(self, method)
        if not self.over_taps:
            raise ValueError("%s.%s: the local attention's softmax runs over time, so a step's output depends on every later window and "
                             "on the padded length; streaming needs attend_over_taps(model) (models.attend_over_taps), which normalises "
                             "the taps of each step instead" % (type(self).__name__, method))

    def stream(self, batch, capacity=None):
        """This model as an online predictor (``streaming.LSTMStream``): ``step(x_t (B, window_embed_size), mask_t)`` -> the (B,1)
        prediction of that window in ONE launch (csrc/lstm_step.h).  Eval mode, ``attend_over_taps(model)`` on.  There is no cache, so
        no capacity (the argument is accepted and ignored, for the wrappers' common call)."""
        self._stream_refusals("stream")
        return LSTMStream(self, batch)

    def slot_stream(self, batch, limit=None):
        """``stream(batch)`` with slots (``streaming.LSTMSlotStream``): sequences are seated and released independently (``.positions``,
        ``.seat``, ``.release``, ``.full``: streaming._Slots), and a step can be captured into a graph (``graphs.capture_stream``).
        ``limit``: windows per recording after which a slot counts as full (None: none)."""
        self._stream_refusals("slot_stream")
        return LSTMSlotStream(self, batch, limit)


class _FeedbackStreams:
    """``feedback_stream`` / ``feedback_slot_stream`` of the two baselines whose read-out feeds its own prediction back (MultiEDLSTM,
    MultiARLSTM): the model as a free-running online predictor.  ``stream`` / ``slot_stream`` keep refusing (the fed-back prediction is
    carried state that ``LSTMStream`` does not have); these entries carry it (csrc/lstm_step.h with a tail).  There is no
    teacher-forced stream: that branch reads the current target, so it predicts nothing online."""

    def _feedback_refusals(self, method):
        self._stream_refusals(method)

    def feedback_stream(self, batch, tgt_init=0.0):
        """This model as an online predictor (``streaming.LSTMFeedbackStream``): ``step(x_t (B, window_embed_size), mask_t)`` -> the
        (B,1) row that the eval ``forward(inputs, mask, lengths, target=None, tgt_init=tgt_init)`` gives at that window, in ONE launch.
        Eval mode, ``attend_over_taps(model)`` on.  h_dim and embed_dim up to 512: the default h_dim = 512, which ``forward`` refuses,
        streams."""
        self._feedback_refusals("feedback_stream")
        return LSTMFeedbackStream(self, batch, tgt_init)

    def feedback_slot_stream(self, batch, limit=None, tgt_init=0.0):
        """``feedback_stream(batch, tgt_init)`` with slots (``streaming.LSTMFeedbackSlotStream``): ``.positions``, ``.seat``,
        ``.release``, ``.full`` (streaming._Slots); a step can be captured into a graph (``graphs.capture_stream``).  ``limit``: windows
        per recording after which a slot counts as full (None: none)."""
        self._feedback_refusals("feedback_slot_stream")
        return LSTMFeedbackSlotStream(self, batch, limit, tgt_init)


class MultiLSTM(_LocalAttnLSTM):
    """The shared copy: transformer/SFT/models.py:144-225 (MFT, B2-Trans, B3-MFN, Performance-Eval identical) — embed dropout 0.1,
    decoder Linear, ReLU, Linear (keys decoder.0 / decoder.2).  The configuration of the shipped B1-LSTM-L.pth checkpoint."""

    def __init__(self, window_embed_size, embed_dim=128, h_dim=256, n_layers=1, attn_len=5, device=torch.device("cuda:0")):
        super().__init__(window_embed_size, embed_dim, h_dim, n_layers, attn_len, device)


class MultiLSTMB1(_LocalAttnLSTM):
    """The B1-LSTM copy: transformer/B1-LSTM/models.py:135-216 — embed_dim 512, embed dropout 0.4, decoder Linear, ReLU,
    Dropout(0.4), Linear (keys decoder.0 / decoder.3).  The reference calls this class ``MultiLSTM`` too."""
    _embed_p = 0.4
    _dec_dropout = 0.4

    def __init__(self, window_embed_size, embed_dim=512, h_dim=256, n_layers=1, attn_len=5, device=torch.device("cuda:0")):
        super().__init__(window_embed_size, embed_dim, h_dim, n_layers, attn_len, device)


class MultiEDLSTM(_FeedbackStreams, _LocalAttnLSTM):
    """The encoder-decoder LSTM: transformer/MFT/models.py:222-308 (the SFT, B2-Trans, B3-MFN and Performance-Eval copies are the same).

        context = the front of the LSTM baseline (``_front``) with ``encoder`` as its LSTM, started from enc_h0 / enc_c0       (B,T,H)
        gxc     = context W_c^T + (b_ih + b_hh),  W_c = decoder.weight_ih_l0[:, 1:]                                          (T,B,4H)
        p       = functional.lstm_fb_scan: decoder LSTM steps on [p_{t-1} ; context_t] from dec_h0 / dec_c0, p_{-1} = tgt_init,
                  p_t = out(h_t) — the read-out MLP runs inside the recurrence (csrc/scan_fb.h)                               (T,B)
        out     = p * mask                                                                                                   (B,T,1)

    The decoder runs all T steps of the padded batch, as the reference does; it is causal and masked outputs carry no gradient.
    ``target`` is accepted and ignored, as in the reference.  Limits (raised as NotImplementedError at the first forward): n_layers == 1,
    and h_dim and embed_dim multiples of 4 in [4,128] — the reference's default h_dim = 512 is outside them."""

    def __init__(self, window_embed_size, embed_dim=128, h_dim=512, n_layers=1, attn_len=3, device=torch.device("cuda:0")):
        nn.Module.__init__(self)
        self.embed_dim = embed_dim
        self.h_dim = h_dim
        self.n_layers = n_layers
        self.attn_len = attn_len
        self.embed = nn.Sequential(nn.Dropout(self._embed_p), nn.Linear(window_embed_size, embed_dim), nn.ReLU())
        self.attn = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, attn_len), nn.Softmax(dim=1))
        self.encoder = nn.LSTM(embed_dim, h_dim, n_layers, batch_first=True)
        self.enc_h0 = nn.Parameter(torch.zeros(n_layers, 1, h_dim))
        self.enc_c0 = nn.Parameter(torch.zeros(n_layers, 1, h_dim))
        self.decoder = nn.LSTM(1 + h_dim, h_dim, n_layers, batch_first=True)
        self.dec_h0 = nn.Parameter(torch.zeros(n_layers, 1, h_dim))
        self.dec_c0 = nn.Parameter(torch.zeros(n_layers, 1, h_dim))
        self.out = nn.Sequential(nn.Linear(h_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, 1))
        self.device = _hip_device(device)
        self.to(self.device)

    def stream(self, batch, capacity=None):
        raise NotImplementedError("MultiEDLSTM.stream: the decoder LSTM with the read-out in its recurrence carries state of its own "
                                  "(its (h, c) and the fed-back prediction), which this stream does not have: open "
                                  "feedback_stream(batch, tgt_init) / feedback_slot_stream(batch, limit, tgt_init) instead")

    slot_stream = stream

    def _feedback_refusals(self, method):
        self._stream_refusals(method)
        if self.n_layers != 1:
            raise NotImplementedError("MultiEDLSTM.%s: n_layers = %d; the decoder step with the read-out in its recurrence takes "
                                      "n_layers == 1, as forward" % (method, self.n_layers))

    def forward(self, inputs, mask, lengths, target=None, tgt_init=0.0):
        if self.n_layers != 1:
            raise NotImplementedError("MultiEDLSTM: n_layers = %d; the decoder scan with the read-out in its recurrence takes n_layers == 1"
                                      % self.n_layers)
        B, T = inputs.shape[0], inputs.shape[1]
        F_hip._fb_limits(max(T, 1), max(B, 1), self.h_dim, self.embed_dim)      # before any launch, with the limit named
        context = self._front(inputs, mask, lengths, self.encoder, self.enc_h0, self.enc_c0)
        w_p, W_c, bias = F_hip.decoder_fb_pack(self.decoder)
        gxc = F_hip.linear(F_hip.time_major(context), W_c, bias)
        p = F_hip.lstm_fb_scan(gxc, w_p, self.decoder.weight_hh_l0, self.out[0].weight, self.out[0].bias, self.out[2].weight,
                               self.out[2].bias, F_hip.broadcast_layers(self.dec_h0, B).view(B, -1),
                               F_hip.broadcast_layers(self.dec_c0, B).view(B, -1), p_init=float(tgt_init))
        return F_hip.batch_major(p.reshape(T, B, 1), mask.float())


class MultiARLSTM(_FeedbackStreams, _LocalAttnLSTM):
    """The LSTM baseline with an autoregressive read-out: transformer/MFT/models.py:310-400 (the SFT, B2-Trans, B3-MFN, Performance-Eval
    and B1-LSTM copies are the same).

        context = the front of the LSTM baseline (``_front``), zero initial states, n_layers as MultiLSTM takes them           (B,T,H)
        in_part = decoder(context) = Linear(E->1)(ReLU(Linear(H->E)(context)))                                                 (B,T,1)
        w       = autoreg(context) = Linear(H->ar_order)                                                                       (B,T,K)
        out     = functional.ar_combine(in_part, w, mask, target, tgt_init)                                                    (B,T,1)

    With a ``target`` the read-out is teacher-forced: in_part + sum_i w[:,t,i] target[:,t-i], zeros before step 0, tap 0 on the current
    target (:381-386).  Without one it runs on its own predictions from ``tgt_init``, tap K-1 on the newest (:388-397): the reference's
    step loop, here one kernel launch (csrc/ar_combine.h); as there, the fed-back predictions carry no gradient.  decoder[0] and autoreg
    read the context through one autograd node (``linear_pair``), so its two gradients are summed by a hand-written kernel.
    Limits (raised as NotImplementedError at the first forward, before any launch): 1 <= ar_order <= 16, and h_dim a multiple of 4 in
    [4,256], what ``lstm_scan`` takes — the reference's default h_dim = 512 is outside them."""

    def __init__(self, window_embed_size, embed_dim=128, h_dim=512, n_layers=1, attn_len=7, ar_order=1, device=torch.device("cuda:0")):
        nn.Module.__init__(self)
        self.embed_dim = embed_dim
        self.h_dim = h_dim
        self.n_layers = n_layers
        self.attn_len = attn_len
        self.ar_order = ar_order
        self.embed = nn.Sequential(nn.Dropout(self._embed_p), nn.Linear(window_embed_size, embed_dim), nn.ReLU())
        self.attn = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, attn_len), nn.Softmax(dim=1))
        self.lstm = nn.LSTM(embed_dim, h_dim, n_layers, batch_first=True)
        self.decoder = nn.Sequential(nn.Linear(h_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, 1))
        self.autoreg = nn.Linear(h_dim, ar_order)
        self.device = _hip_device(device)
        self.to(self.device)

    def stream(self, batch, capacity=None):
        raise NotImplementedError("MultiARLSTM.stream: the autoregressive read-out carries state of its own (its last ar_order "
                                  "predictions), which this stream does not have: open feedback_stream(batch, tgt_init) / "
                                  "feedback_slot_stream(batch, limit, tgt_init) instead")

    slot_stream = stream

    def forward(self, inputs, mask, lengths, target=None, tgt_init=0.0):
        F_hip._ar_limits(self.ar_order)                 # both before any launch, with the limit named
        F_hip._scan_limits(self.h_dim, "MultiARLSTM")
        context = self._front(inputs, mask, lengths, self.lstm)
        dec0, last = self.decoder[0], self.decoder[2]
        hid, w = F_hip.linear_pair(context, dec0.weight, dec0.bias, self.autoreg.weight, self.autoreg.bias, act1=1)
        in_part = F_hip.linear(hid, last.weight, last.bias)
        return F_hip.ar_combine(in_part, w, mask, target, p_init=float(tgt_init))


class MultiCNNLSTM(_FrontEnd):
    """B1-LSTM: transformer/B1-LSTM/models.py:79-133 — per modality CNN(k=2) + max-pool -> ReLU Highway (``HighwayB1``) -> Dropout(0.3),
    modalities concatenated (no fusion layer), then the LSTM baseline's sequence model.

    Keyword-only extensions (the reference's positional signature is kept): ``window_embed_size`` replaces B1's fixed window embed sizes
    (linguistic 1024, :91) and ``lstm_cls`` chooses the copy of the sequence model (B1's own by default).  The shipped checkpoint
    transformer/ModelSave/B1-LSTM/B1-LSTM-L.pth was saved from an older models.py: linguistic window_embed_size 300 and the shared
    MultiLSTM (E = 128, H = 256, L = 5, decoder keys .0 / .2), i.e.
        MultiCNNLSTM(["linguistic"], {"linguistic": 300}, window_embed_size={"linguistic": 300}, lstm_cls=MultiLSTM).
    Whether that file's Highway had the ReLU cannot be read from its weights; ``MultiCNNLSTM`` exists only in B1, so B1's Highway is used."""
    _highway_cls = HighwayB1

    def __init__(self, mods, dims, fuse_embed_size=256, k=2, device=torch.device("cuda:0"), *, window_embed_size=None,
                 lstm_cls=MultiLSTMB1):
        super().__init__()
        self.window_embed_size = dict(window_embed_size) if window_embed_size is not None else \
            {"linguistic": 1024, "emotient": 20, "acoustic": 256, "image": 256}          # B1-LSTM/models.py:91
        total = self._build(mods, dims, k)
        self.LSTM = lstm_cls(total, device=device)
        self.dropout = nn.Dropout(p=0.3)
        self.device = _hip_device(device)
        self.to(self.device)

    def forward(self, inputs, length, mask=None):
        outs = self._encode(inputs)
        x = F_hip.cat_cols([outs[m] for m in self.mods]) if len(self.mods) > 1 else outs[self.mods[0]]
        return self.LSTM(x, mask, length)

    def stream(self, batch, capacity=None):
        """This model as an online predictor (``_FrontEndStream``): the window encoder at T = 1, then the LSTM baseline's one-launch step.
        Eval mode, ``attend_over_taps(model)`` on.  No cache, so no capacity."""
        return _FrontEndStream(self, batch, None)

    def slot_stream(self, batch, limit=None):
        """``stream(batch)`` with slots: sequences are seated and released independently (``.positions``, ``.seat``, ``.release``,
        ``.full``: streaming._Slots), and a step can be captured into a graph (``graphs.capture_stream``)."""
        return _FrontEndStream(self, batch, limit, "slot_stream")

    def _feedback_seq(self, method, *args):
        if not isinstance(self.LSTM, _FeedbackStreams):
            raise ValueError("MultiCNNLSTM.%s: the sequence model %s feeds no prediction back; open stream(batch) / "
                             "slot_stream(batch, limit)" % (method, type(self.LSTM).__name__))
        _stream_model_checks(self, method)
        return _FrontEndStream(self, args[0], None, seq=getattr(self.LSTM, method)(*args))

    def feedback_stream(self, batch, tgt_init=0.0):
        """With ``lstm_cls`` MultiEDLSTM or MultiARLSTM: the window encoder at T = 1, then the sequence model's ``feedback_stream``."""
        return self._feedback_seq("feedback_stream", batch, tgt_init)

    def feedback_slot_stream(self, batch, limit=None, tgt_init=0.0):
        """``feedback_stream(batch, tgt_init)`` with slots: the sequence model's ``feedback_slot_stream``."""
        return self._feedback_seq("feedback_slot_stream", batch, limit, tgt_init)
