"""The bf16-faithful fp64 reference of a PREFILLED stream (TEST INFRASTRUCTURE, a plain helper module beside tests/stream_ref.py): the
batch path's reference over a history, then the step's reference from there on.  It composes the existing modules unchanged.

The encoder.  ``encoder`` walks ``causal_ref.encoder_layer`` (``band_ref.encoder_layer`` with a span) layer by layer over the prefix
x (B, P, d).  At each layer it forms K = bf16(affine(n0)) and V likewise by that file's own lines (n0 = rf(LN1(x)); k = _affine(...);
K = rf(rb(k))), which are also stream_ref's (K_t = rf(_affine(...))): both paths round K and V at the same site, so the cache a
prefill fills holds the batch path's K and V, and these are what the seeded stream reference is given.  Per sequence b it seeds a
``stream_ref.EncoderStream`` (``ring_stream_ref.EncoderStream`` with a span) of batch 1 with the entries of positions < len[b], sets
``t = len[b]``, and the stream reference steps on.  What differs from a fully stepped stream reference is only that the history's
K / V came out of layers whose inputs went through the batch path's attention (lazily moved tile maximum) and not the step's (exact
row maximum).  With ``rounding=False`` both are the exact function, so a row stepped after the seed equals
``causal_ref.encoder_stack(..., rounding=False)[:, t]`` to 1e-12 (tests/test_prefill_cpu.py).

The decoder.  ``decoder`` composes ``decoder_stream_ref.batch``'s pieces over windows < len and hands (h, c) of window len - 1 to a
``decoder_stream_ref.DecoderStep`` standing at t = len.
"""
import torch

import band_ref as BD
import bf16_ref as E
import causal_ref as C
import decoder_stream_ref as DS
import oracle
import ring_stream_ref as RS
import stream_ref as S


def encoder(p, prefix, h, x, mask, lengths, span=None, rounding=True):
    """x (B, P, d) fp64, mask (B, P, 1) or None, lengths: B ints in [1, P] -> (the batch reference's rows (B, P, d), a list of B stream
    references of batch 1, sequence b seeded with its first lengths[b] windows and standing at t = lengths[b])."""
    rf, rb = E._sites(rounding)
    B, P, d = x.shape
    n, dk = oracle.count_layers(p, prefix), d // h
    Ks, Vs = [], []
    with torch.no_grad():
        cur = x
        for i in range(n):
            L = "%slayers.%d." % (prefix, i)
            n0 = rf(oracle.layer_norm(cur, p[L + "sublayer.0.norm.a_2"], p[L + "sublayer.0.norm.b_2"]))
            a = L + "self_attn.linears."
            Ks.append(rf(rb(E._affine(p, a + "1", n0, rf))).detach())                    # (B, P, d): K carries no scale
            Vs.append(rf(rb(E._affine(p, a + "2", n0, rf))).detach())
            cur = (C.encoder_layer(p, L, cur, mask, h, None, rounding) if span is None
                   else BD.encoder_layer(p, L, cur, mask, h, span, None, rounding)).detach()
        rows = oracle.layer_norm(cur, p[prefix + "norm.a_2"], p[prefix + "norm.b_2"])
    streams = []
    for b in range(B):
        s = S.EncoderStream(p, prefix, h, rounding) if span is None else RS.EncoderStream(p, prefix, h, span, rounding)
        for i in range(n):
            s.K[i] = [Ks[i][b, t].reshape(1, h, 1, dk) for t in range(lengths[b])]
            s.V[i] = [Vs[i][b, t].reshape(1, h, 1, dk) for t in range(lengths[b])]
        s.t = lengths[b]
        streams.append(s)
    return rows, streams


def encoder_rows(p, prefix, h, x, mask, lengths, P, span=None, rounding=True):
    """x (B, T, d), mask (B, T, 1) or None: prefill with the first P windows (sequence b with min(lengths[b], P) of them), then step
    every sequence from its own position to T -> (B, T, d): rows < P are the batch reference's, rows t >= min(lengths[b], P) of
    sequence b the seeded stream reference's (rows in between: the batch reference's, which a real stream never returns)."""
    B, T, d = x.shape
    lens = [min(int(n), P) for n in lengths]
    rows, streams = encoder(p, prefix, h, x[:, :P], None if mask is None else mask[:, :P], lens, span, rounding)
    out = torch.zeros(B, T, d, dtype=x.dtype)
    out[:, :P] = rows
    for b, s in enumerate(streams):
        for t in range(lens[b], T):
            out[b, t] = s.step(x[b:b + 1, t], None if mask is None else mask[b:b + 1, t].reshape(-1))[0]
    return out


def decoder(p, prefix, n_layers, enc, mask, lengths, P, rounding=True):
    """enc (B, T, d), mask (B, T) or None: ``decoder_stream_ref.batch``'s composition over the first P windows, sequence b carried on
    from (h, c) of window min(lengths[b], P) - 1 by a ``DecoderStep`` -> (B, T, 1), rows as in ``encoder_rows``."""
    B, T, d = enc.shape
    L = int(n_layers)
    assert L in (0, 1), "a stacked decoder has no prefill: lstm_stack_scan returns the top layer only"
    lens = [min(int(n), P) for n in lengths]
    out = torch.zeros(B, T, 1, dtype=enc.dtype)
    out[:, :P] = DS.batch(p, prefix, L, enc[:, :P], None if mask is None else mask[:, :P], rounding)
    h_all = c_all = None
    if L == 1:
        Wi, Wh, bi, bh = DS._lstm(p, prefix, 0)
        gx = E.linear(enc[:, :P].transpose(0, 1), Wi[:, d:], bi + bh, rounding=rounding)
        gx = torch.cat([gx[:1] + E.linear(p[prefix + "dec_h0"][0], Wh, rounding=rounding), gx[1:]], dim=0)
        h_all, c_all = E.lstm_scan(gx, Wi[:, :d] + Wh, None, p[prefix + "dec_c0"][0].expand(B, d), rounding=rounding)
    for b in range(B):
        s = DS.DecoderStep(p, prefix, L, 1, rounding)
        s.t = lens[b]
        if L == 1:
            s.h, s.c = [h_all[lens[b] - 1, b:b + 1]], [c_all[lens[b] - 1, b:b + 1]]
        for t in range(lens[b], T):
            out[b, t] = s.step(enc[b:b + 1, t], None if mask is None else mask[b:b + 1, t])[0]
    return out
