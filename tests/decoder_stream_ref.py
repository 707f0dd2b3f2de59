"""The reference of the one-window decoder step (TEST INFRASTRUCTURE, a plain helper module beside tests/mfn_stream_ref.py): the LSTM
decoder of UniTransformer / NLPTransformer and the read-out MLP, ONE window per call, in fp64 with the ``rounding`` switch of
tests/bf16_ref.py.

``DecoderStep`` carries, per layer, (h, c) and, for a stacked decoder, the top layer's previous output o.  One layer: a step is composed
of ``bf16_ref.linear`` and ``bf16_ref.lstm_scan`` at T = 1, exactly the pieces ``_DecoderMixin._decode`` runs over all T.  More layers:
one window of ``bf16_ref.lstm_stack_scan``'s loop restated with a carried o (that function always starts from o = 0).  ``batch`` is the
batch composition over all T, from the same pieces, what the step is held against in tests/test_decoder_stream_cpu.py.

Parameters: a dict of fp64 tensors under the model's own names, "decoder.weight_ih_l0", ..., "dec_h0" (L, 1, d), "dec_c0", "out.0.weight",
"out.0.bias", "out.2.weight", "out.2.bias".  L = 0: the read-out alone.
"""
import torch

import bf16_ref as R
import slot_stream_ref as SL

# device_stream against the existing stream() on the GPU, in lockstep (rel-L2 / per-row maximum): the ONE place these bounds live, for
# tests/test_gpu_decoder_stream.py (where they are measured and explained) and tools/decoder_stream_bench.py (which asserts them).
DEC_STEP_VS_STREAM, DEC_STEP_VS_STREAM_ROW = 1.4e-4, 1.8e-3


def _lstm(p, prefix, l):
    return [p["%sdecoder.%s_l%d" % (prefix, n, l)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _readout(p, prefix, h, mask_row, rounding):
    hid = R.linear(h, p[prefix + "out.0.weight"], p[prefix + "out.0.bias"], act=1, rounding=rounding)
    return R.linear(hid, p[prefix + "out.2.weight"], p[prefix + "out.2.bias"], rowscale=mask_row, rounding=rounding)


class DecoderStep:
    """step(e_t (B, d), mask_t (B) or None) -> y_t (B, 1), window by window from position 0"""

    def __init__(self, p, prefix, n_layers, batch, rounding=True):
        self.p, self.prefix, self.L, self.B, self.rounding = p, prefix, int(n_layers), int(batch), rounding
        self.t = 0
        self.h = self.c = self.o = None

    def step(self, e, mask_t=None):
        p, pre, L, B, rd = self.p, self.prefix, self.L, self.B, self.rounding
        d = e.shape[1]
        if L == 0:
            top = e
        elif L == 1:
            Wi, Wh, bi, bh = _lstm(p, pre, 0)
            gx = R.linear(e.reshape(1, B, d), Wi[:, d:], bi + bh, rounding=rd)                       # (1, B, 4d)
            if self.t == 0:
                gx = gx + R.linear(p[pre + "dec_h0"][0], Wh, rounding=rd)                             # h0 W_hh^T: o_{-1} = 0
                h_all, c_all = R.lstm_scan(gx, Wi[:, :d] + Wh, None, p[pre + "dec_c0"][0].expand(B, d), rounding=rd)
            else:
                h_all, c_all = R.lstm_scan(gx, Wi[:, :d] + Wh, self.h[0], self.c[0], rounding=rd)
            self.h, self.c = [h_all[0]], [c_all[0]]
            top = h_all[0]
        else:
            rf, rb = R._sites(rd)
            if self.t == 0:
                self.h = [p[pre + "dec_h0"][l].expand(B, d) for l in range(L)]
                self.c = [p[pre + "dec_c0"][l].expand(B, d) for l in range(L)]
                self.o = e.new_zeros(B, d)
            Wi0, Wh0, bi0, bh0 = _lstm(p, pre, 0)
            gx0 = R.linear(e, Wi0[:, d:], bi0 + bh0, rounding=rd)
            h, c = list(self.h), list(self.c)
            for l in range(L):
                Wi, Wh, bi, bh = _lstm(p, pre, l)
                Pl = torch.cat([Wi[:, :d], Wh], dim=1)                                               # [x_a columns | x_b columns]
                xa = self.o if l == 0 else h[l - 1]
                prod = rf(torch.cat([xa, h[l]], dim=1)) @ rf(Pl).t()
                g = gx0 + rb(prod) if l == 0 else rb(prod + (bi + bh))
                h[l], c[l], _ = R._cell(g, c[l], d)
            self.h, self.c, self.o = h, c, h[L - 1]
            top = h[L - 1]
        self.t += 1
        return _readout(p, pre, top, mask_t, rd)


def stepped(p, prefix, n_layers, enc, mask=None, rounding=True):
    """enc (B, T, d), mask (B, T) or None -> (B, T, 1): every window through DecoderStep, in order"""
    B, T, _ = enc.shape
    s = DecoderStep(p, prefix, n_layers, B, rounding)
    return torch.stack([s.step(enc[:, t], None if mask is None else mask[:, t]) for t in range(T)], dim=1)


def batch(p, prefix, n_layers, enc, mask=None, rounding=True):
    """the batch composition over all T of the same pieces (``_decode`` / ``_decode_stacked``) -> (B, T, 1)"""
    B, T, d = enc.shape
    L = int(n_layers)
    tm = enc.transpose(0, 1)                                                                        # (T, B, d)
    if L == 0:
        top = tm
    else:
        Wi0, Wh0, bi0, bh0 = _lstm(p, prefix, 0)
        gx = R.linear(tm, Wi0[:, d:], bi0 + bh0, rounding=rounding)
        if L == 1:
            row0 = R.linear(p[prefix + "dec_h0"][0], Wh0, rounding=rounding)
            gx = torch.cat([gx[:1] + row0, gx[1:]], dim=0)
            top, _ = R.lstm_scan(gx, Wi0[:, :d] + Wh0, None, p[prefix + "dec_c0"][0].expand(B, d), rounding=rounding)
        else:
            P, bias = [torch.cat([Wi0[:, :d], Wh0], dim=1)], []
            for l in range(1, L):
                Wi, Wh, bi, bh = _lstm(p, prefix, l)
                P.append(torch.cat([Wi, Wh], dim=1))
                bias.append(bi + bh)
            h0 = torch.stack([p[prefix + "dec_h0"][l].expand(B, d) for l in range(L)])
            c0 = torch.stack([p[prefix + "dec_c0"][l].expand(B, d) for l in range(L)])
            top, _, _ = R.lstm_stack_scan(gx, torch.stack(P), torch.stack(bias), h0, c0, rounding=rounding)
    y = _readout(p, prefix, top, None, rounding)                                                    # (T, B, 1)
    y = y.transpose(0, 1)
    return y if mask is None else y * mask.reshape(B, T, 1)


def decoder_slots(p, prefix, n_layers, enc, mask, table, rounding=True):
    """enc {recording: (T, d)}, mask {recording: (T,)} or None -> (calls, slots, 1): every recording alone through ``stepped``, put
    where the timetable (slot_stream_ref.timetable) says; idle and full cells are zeros"""
    alone = {}
    for rec, n in SL.windows_used(table).items():
        m = None if mask is None else mask[rec][:n].reshape(1, n)
        alone[rec] = stepped(p, prefix, n_layers, enc[rec][:n].unsqueeze(0), m, rounding)[0]
    return SL.assemble(table, alone, 1)


def params(d, h_dim, n_layers, seed=11, tag="decoder_stream", scale=None):
    """fp64 parameters of a decoder under the model's names; dec_h0 / dec_c0 random and non-zero everywhere (zeros, the model's own
    initial values, would hide the position-0 path)"""
    import recipe as G
    p = {}
    s = scale if scale is not None else 1.0 / d ** 0.5

    def draw(name, shape, k):
        p[name] = (G.gen_normal("%s:%s" % (tag, name), shape, seed) * k).double()

    for l in range(n_layers):
        draw("decoder.weight_ih_l%d" % l, (4 * d, 2 * d if l == 0 else d), s)
        draw("decoder.weight_hh_l%d" % l, (4 * d, d), s)
        draw("decoder.bias_ih_l%d" % l, (4 * d,), 0.1)
        draw("decoder.bias_hh_l%d" % l, (4 * d,), 0.1)
    if n_layers:
        draw("dec_h0", (n_layers, 1, d), 0.5)
        draw("dec_c0", (n_layers, 1, d), 0.5)
    draw("out.0.weight", (h_dim, d), s)
    draw("out.0.bias", (h_dim,), 0.1)
    draw("out.2.weight", (1, h_dim), 1.0 / h_dim ** 0.5)
    draw("out.2.bias", (1,), 0.1)
    return p
