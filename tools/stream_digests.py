"""Developer tool: digests of what the one-window streams compute, to compare two builds bit for bit.

    python tools/stream_digests.py [--out FILE]

Prints the first 32 hex digits of the SHA-256 of every prepared state, every y_t, the state after the steps and the positions, one
line each (the format of profiles/r09_stream_digests.txt), for the functional host (t by value) and slots (positions on the device)
forms and the stream classes of the families: encoder (plain and ring cache), MFN gate, decoder, LSTM baseline and, after those, the LSTM
baselines that feed their prediction back (MultiEDLSTM, MultiARLSTM; a build without them stops there).  Two runs of it
on two builds of the library agree line for line exactly when the builds compute the same bits on these shapes.

Everything is fixed: parameters and inputs come from seeded CPU generators, every state is zero-filled before it is prepared.  The
shapes are the smallest at which the shared pieces of the step kernels can go wrong: B = 3 with slot 1 idle in the positioned forms
and row 2 masked out at windows 1 and 3, 5 windows (position 0 and both copies of the carried state), decoders of 0, 1 and 2 layers,
LSTM baselines of 1 and 2 layers with 3 taps (the ring wraps), an MFN of two modalities with hidden sizes 48 and 16, a 2-layer encoder
at d = 128, a ring of span 3.  A few seconds on one GPU."""
import argparse
import hashlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimodal_transformer_amd as m  # noqa: E402

B, T, IDLE = 3, 5, 1
LINES = []


def emit(label, tensor):
    digest = hashlib.sha256(tensor.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]
    LINES.append("%-44s %s" % (label, digest))
    print(LINES[-1], flush=True)


def seeded(module, seed, dev):
    """every parameter of ``module`` from a CPU generator (no dependence on how a build or a device initialises), eval mode"""
    g = torch.Generator().manual_seed(seed)
    module.to(dev)
    with torch.no_grad():
        for p in module.parameters():
            scale = 0.5 / math.sqrt(p.shape[-1]) if p.dim() > 1 else 0.1
            p.copy_((torch.randn(p.shape, generator=g) * scale).to(dev))
    return module.eval()


def rows(seed, width, dev):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, width, generator=g).to(dev) for _ in range(T)]


def masks(dev):
    out = [torch.ones(B, device=dev) for _ in range(T)]
    out[1][2] = 0.0
    out[3][2] = 0.0
    return out


def seats(dev):
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    pos[IDLE] = -1
    return pos


def fresh(stream):
    """the stream with a zero-filled state, prepared again (its allocation has any contents)"""
    stream.state.zero_()
    stream.refresh()
    if stream.slots:
        stream.seat([b for b in range(B) if b != IDLE])
    return stream


def record(label, state, step, positions=None):
    emit(label + " state after prepare", state)
    for t in range(T):
        emit("%s y[%d]" % (label, t), step(t))
    emit(label + " state after steps", state)
    if positions is not None:
        emit(label + " positions", positions)


def family(label, names, open_host, open_slots, host_step, slots_step, class_step):
    """the four routes of one family: the functional entries on the state of a stream opened for that, and the two stream classes.
    ``host_step(stream, t)`` / ``slots_step(stream, positions, t)`` call the functional layer, ``class_step(stream, t)`` the class."""
    s = fresh(open_host())
    record(label + " host", s.state, lambda t: host_step(s, t))
    z = fresh(open_host())
    pos = seats(z.state.device)
    record(label + " slots", z.state, lambda t: slots_step(z, pos, t), pos)
    s = fresh(open_host())
    record(names[0], s.state, lambda t: class_step(s, t))
    z = fresh(open_slots())
    record(names[1], z.state, lambda t: class_step(z, t), z.positions)


def encoders(dev):
    MT, F, S = m.multiTransformer, m.functional, m.streaming
    d, h, f, n, cap, span = 128, 4, 128, 2, 6, 3

    def make(seed, **causal):
        enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, f, 0.1), 0.1), n)
        MT.causal_attention(seeded(enc, seed, dev), True, **causal)
        return enc

    x, mk = rows(101, d, dev), masks(dev)
    enc = make(1)
    family("encoder", ("Encoder.stream", "Encoder.slot_stream"), lambda: enc.stream(B, cap), lambda: enc.slot_stream(B, cap),
           lambda s, t: F.encoder_stream_step(x[t], mk[t], s._flat, s.state, t, h, f, n, cap, s.eps),
           lambda s, pos, t: F.encoder_stream_step_slots(x[t], mk[t], s._flat, s.state, pos, h, f, n, cap, s.eps),
           lambda s, t: s.step(x[t], mk[t]))
    ring = make(2, span=span)
    family("encoder ring", ("Encoder.ring_stream", "Encoder.ring_slot_stream"), lambda: ring.ring_stream(B), lambda: ring.ring_slot_stream(B),
           lambda s, t: S.encoder_ring_step(x[t], mk[t], s._flat, s.state, t, h, f, n, span, s.eps),
           lambda s, pos, t: S.encoder_ring_step_slots(x[t], mk[t], s._flat, s.state, pos, h, f, n, span, s.eps),
           lambda s, t: s.step(x[t], mk[t]))


def mfn(dev):
    F = m.functional
    mods, dims = ["acoustic", "emotient"], {"acoustic": 12, "emotient": 16}          # hidden sizes 48 and 16
    gate = seeded(m.multiTransformer.MFN(mods, dims, 2, device=dev), 3, dev)
    x = {mod: rows(110 + i, dims[mod], dev) for i, mod in enumerate(mods)}
    mk = masks(dev)
    family("mfn", ("MFN.stream", "MFN.slot_stream"), lambda: gate.stream(B), lambda: gate.slot_stream(B),
           lambda s, t: F.mfn_stream_step([x[mod][t] for mod in mods], mk[t], s.state, t, s.in_dims, s.hidden, s.output_dim),
           lambda s, pos, t: F.mfn_stream_step_slots([x[mod][t] for mod in mods], mk[t], s.state, pos, s.in_dims, s.hidden, s.output_dim),
           lambda s, t: s.step({mod: x[mod][t] for mod in mods}, mk[t]))


def decoders(dev):
    MT, F = m.multiTransformer, m.functional
    width, d, cap = 48, 40, 6
    x, e, mk = rows(120, width, dev), rows(121, d, dev), masks(dev)
    for L in (0, 1, 2):
        if L == 0:
            model = MT.UniFullTransformer(width, embed_dim=d, h_dim=128, h=4, N=1, device=dev)
        else:
            model = MT.NLPTransformer(width, embed_dim=d, h_dim=128, h=4, N=1, n_layers=L, device=dev)
        MT.causal_attention(seeded(model, 4 + L, dev))
        label, name = "decoder L%d" % L, type(model).__name__ + ".device_stream"

        def opened():
            z = model.device_stream(B, cap)
            z.state.zero_()
            z.enc.state.zero_()
            z.refresh()
            return z

        s = opened()                                                     # the functional entries on the decoder's state alone
        record(label + " host", s.state, lambda t: F.decoder_stream_step(e[t], mk[t], s.state, t, s.d, s.h_dim, L))
        z, pos = opened(), seats(dev)
        record(label + " slots", z.state, lambda t: F.decoder_stream_step_slots(e[t], mk[t], z.state, pos, z.d, z.h_dim, L, limit=cap), pos)
        c = opened()                                                     # the class: embed, encoder step and decoder step
        c.seat([b for b in range(B) if b != IDLE])
        record(name + " L%d" % L, c.state, lambda t: c.step(x[t], mk[t]), c.positions)
        emit(name + " L%d encoder state after steps" % L, c.enc.state)


def lstms(dev):
    F = m.functional
    width = 20
    x, mk = rows(130, width, dev), masks(dev)
    for NL in (1, 2):
        model = seeded(m.models.MultiLSTM(width, embed_dim=32, h_dim=24, n_layers=NL, attn_len=3, device=dev), 7 + NL, dev)
        m.models.attend_over_taps(model)
        family("lstm NL%d" % NL, ("MultiLSTM.stream NL%d" % NL, "MultiLSTM.slot_stream NL%d" % NL),
               lambda: model.stream(B), lambda: model.slot_stream(B),
               lambda s, t: F.lstm_stream_step(x[t], mk[t], s.state, t, *s._dims),
               lambda s, pos, t: F.lstm_stream_step_slots(x[t], mk[t], s.state, pos, *s._dims),
               lambda s, t: s.step(x[t], mk[t]))


def feedback_lstms(dev):
    """MultiEDLSTM and MultiARLSTM (two layers, ar_order 2: the history ring of 3 slots wraps), free-running from tgt_init 0.25"""
    F, MM = m.streaming, m.models
    width, p0 = 20, 0.25
    x, mk = rows(140, width, dev), masks(dev)
    ed = seeded(MM.MultiEDLSTM(width, embed_dim=32, h_dim=24, attn_len=3, device=dev), 11, dev)
    ar = seeded(MM.MultiARLSTM(width, embed_dim=32, h_dim=24, n_layers=2, attn_len=3, ar_order=2, device=dev), 12, dev)
    for label, model in (("lstm fb", ed), ("lstm ar", ar)):
        MM.attend_over_taps(model)
        name = type(model).__name__
        family(label, (name + ".feedback_stream", name + ".feedback_slot_stream"),
               lambda: model.feedback_stream(B, p0), lambda: model.feedback_slot_stream(B, tgt_init=p0),
               lambda s, t: F.lstm_feedback_stream_step(x[t], mk[t], s.state, t, p0, *s._tail, *s._dims),
               lambda s, pos, t: F.lstm_feedback_stream_step_slots(x[t], mk[t], s.state, pos, p0, *s._tail, *s._dims),
               lambda s, t: s.step(x[t], mk[t]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_digests: no HIP device (the digests are of what the kernels compute; there is no CPU path)")
    dev = torch.device("cuda:0")
    print("# SHA-256 (first 32 hex digits) of stream states and outputs: zero-filled states, fixed shapes and seeds", flush=True)
    with torch.no_grad():
        for run in (encoders, mfn, decoders, lstms, feedback_lstms):
            run(dev)
    torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
