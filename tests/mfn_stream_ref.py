"""A bf16-faithful fp64 reference of the one-window MFN gate step (TEST INFRASTRUCTURE, a plain helper module).

``MFNStream`` walks transformer/MFT/multiTransformer.py:200-247 one window at a time and carries (h_m, c_m, mem) itself, as
csrc/mfn_step.h does.  With ``rounding=True`` it rounds (``bf16_ref.bf16``) where the step kernel forms a bf16 operand, the batch
path's sites (bf16_ref.py: the affine map's x and W, the scans' h_{t-1}, mem_{t-1}, u and their weights): every weight and the left
operand of every product; sums, biases, activations, the softmax, the carried state and the output stay fp64.  No site depends on a
tile, so the stepped walk and the batch composition of the existing pieces are the SAME function (tests/test_mfn_stream_cpu.py holds
them to 1e-12), and with ``rounding=False`` it is ``oracle.mfn_gate``.  ``bf16_ref.mfn_mem_scan`` has no initial memory and is not used.

The batch composition (``lstm_states``, ``gate_from_states``, ``batch_composition``) is also the reference of the gate's TRAINING path
(tests/test_gpu_bf16_mfn_gate.py): it runs under autograd, bf16_ref's pieces place ``round_fwd`` / ``round_bwd``, and it takes the two
dropout multipliers and the window mask.  Sites of functional._MfnGateFn and MFN._gate beyond those of the pieces, read from the sources:
  * b_ih + b_hh is one fp32 sum (functional.add2: glue.h copy2d_kernel, src + src2) in front of the affine map, whose bias stays
    fp32: no bf16 site.  The reference sums the two fp32 values in fp64, 2^-25 of the bias away; both biases receive the SAME
    gradient tensor (_Add2Fn.backward returns dy twice), db = colsum(bf16(dgx));
  * cStar, [h ; mem] and the gamma operands Wa, Wm, b1, W2, b2 are fp32 copies (copy2d): the bf16 roundings of cStar, `attended`, `last`
    and of the weights happen inside the affine maps that read them, one rounding of the same fp32 value per reader;
  * softmax_mul (glue.h softmax_mul_fwd_kernel / _bwd_kernel) is fp32 throughout, forward and backward: nothing is rounded, att is kept;
  * gradients that meet are summed in fp32 by copy2d: d attended = (d apre) Wa + (d a2') W_att2_fc1 (accumulate), and
    dc_t = (d cStar + d cStar')[new part]_t + (d cStar + d cStar')[prev part]_{t+1} with d cStar from the product and d cStar' from
    att1_fc1's dx; autograd's fp64 sums stand for them.  Each summand is the fp32 dx of an affine map: g W with g = bf16(.);
  * d apre leaves the memory scan in fp32 and is rounded once in each of its two readers, the affine backward (dWa, db1, d attended:
    grad_prep_kernel) and _wgrad (dWm): the same bf16 value, as ``round_bwd`` in bf16_ref.linear and in mfn_mem_scan place it;
  * the out-dropout multiplier sits behind out_fc1's ReLU in the forward and inside g = bf16(dy * act' * 1/(1-p)) in the backward
    (bf16_ref.linear's out_drop); the mask multiplies the fp32 output (copy2d rowscale) and its gradient before out_fc2's g is rounded.
None of these differs from what ``batch_composition`` assumed before it ran under autograd; the fp32 bias sum is the one site it
does not emulate (below the fp32 noise the jitter floor measures).
"""
import torch

import bf16_ref as E
from oracle.mfn_ref import HIDDEN, MEM_DIM


class MFNStream:
    """p: {prefix + name: fp64 tensor} under MFN's state_dict names; ``step({mod: (B, d_mod)}, mask_t (B) or None) -> (B, output_dim)``."""

    def __init__(self, p, prefix, mods, rounding=True, hidden=None):
        self.mods, self.rounding = list(mods), rounding
        self.hidden = dict(hidden or HIDDEN)
        self.rf = E.bf16 if rounding else (lambda t: t)
        g = lambda n: p[prefix + n]                                                      # noqa: E731
        self.cells = {m: (self.rf(g("lstm_%s.weight_ih" % m)), self.rf(g("lstm_%s.weight_hh" % m)),
                          g("lstm_%s.bias_ih" % m) + g("lstm_%s.bias_hh" % m)) for m in self.mods}
        self.fc = {n: (self.rf(g(n + ".weight")), g(n + ".bias")) for n in
                   ("att1_fc1", "att1_fc2", "att2_fc1", "att2_fc2", "gamma1_fc1", "gamma1_fc2", "gamma2_fc1", "gamma2_fc2", "out_fc1", "out_fc2")}
        self.reset()

    def reset(self):
        self.t, self.h, self.c, self.mem = 0, None, None, None

    def _lin(self, name, x):
        W, b = self.fc[name]
        return self.rf(x) @ W.t() + b

    def step(self, inputs, mask_t=None):
        rf = self.rf
        first = inputs[self.mods[0]]
        B = first.shape[0]
        if self.h is None:
            kw = dict(dtype=first.dtype)
            self.h = {m: torch.zeros(B, self.hidden[m], **kw) for m in self.mods}
            self.c = {m: torch.zeros(B, self.hidden[m], **kw) for m in self.mods}
            self.mem = torch.zeros(B, MEM_DIM, **kw)
        c_prev, c_new, h_new = [], [], []
        for m in self.mods:                                                              # :207-208
            Wih, Whh, bias = self.cells[m]
            H = self.hidden[m]
            pre = (rf(inputs[m]) @ Wih.t() + bias) + rf(self.h[m]) @ Whh.t()
            i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
            g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            c = f * self.c[m] + i * g
            h = o * torch.tanh(c)
            c_prev.append(self.c[m]); c_new.append(c); h_new.append(h)
            self.c[m], self.h[m] = c, h
        c_star = torch.cat(c_prev + c_new, dim=1)                                        # :212-217
        att = torch.softmax(self._lin("att1_fc2", torch.relu(self._lin("att1_fc1", c_star))), dim=1)
        attended = att * c_star                                                          # :218-219
        c_hat = torch.tanh(self._lin("att2_fc2", torch.relu(self._lin("att2_fc1", attended))))      # :220
        A = c_star.shape[1]
        z = []
        for name in ("gamma1", "gamma2"):                                                # :221-223; fc1 = [attended part | memory part]
            W1, b1 = self.fc[name + "_fc1"]
            u = torch.relu((rf(attended) @ W1[:, :A].t() + b1) + rf(self.mem) @ W1[:, A:].t())
            z.append(self._lin(name + "_fc2", u))
        self.mem = torch.sigmoid(z[0]) * self.mem + torch.sigmoid(z[1]) * c_hat          # :224
        last = torch.cat(h_new + [self.mem], dim=1)                                      # :241-243
        out = self._lin("out_fc2", torch.relu(self._lin("out_fc1", last)))              # :244-246
        self.t += 1
        return out if mask_t is None else out * mask_t.reshape(B, 1).to(out.dtype)


def mfn_gate(p, prefix, inputs, mods, mask=None, rounding=True, hidden=None):
    """inputs {mod: (T, B, d_mod)} fp64, mask (B, T, 1) or None -> (B, T, output_dim): every window through MFNStream.step, in order."""
    s = MFNStream(p, prefix, mods, rounding, hidden)
    T = inputs[mods[0]].shape[0]
    with torch.no_grad():
        rows = [s.step({m: inputs[m][t] for m in mods}, None if mask is None else mask[:, t].reshape(-1)) for t in range(T)]
    return torch.stack(rows, dim=1)


def lstm_states(p, prefix, inputs, mods, rounding=True):
    """Phase A of the batch path (MFN._gate): per modality gx = linear(x, W_ih, b_ih + b_hh) -> bf16_ref.lstm_scan.
    inputs {mod: (T, B, d_mod)} -> (hs, cs), lists of (T, B, H_m).  Autograd runs through it when an argument requires grad."""
    g = lambda n: p[prefix + n]                                                          # noqa: E731
    hs, cs = [], []
    for m in mods:
        gx = E.linear(inputs[m], g("lstm_%s.weight_ih" % m), g("lstm_%s.bias_ih" % m) + g("lstm_%s.bias_hh" % m), rounding=rounding)
        h_all, c_all = E.lstm_scan(gx, g("lstm_%s.weight_hh" % m), rounding=rounding)
        hs.append(h_all); cs.append(c_all)
    return hs, cs


def gate_from_states(p, prefix, hs, cs, gamma_drop=None, out_drop=None, rounding=True):
    """functional.mfn_gate(hs, cs, params, ...) from bf16_ref's pieces: hs, cs lists of (T, B, H_m) (leaves of their own or the scans'
    outputs), gamma_drop (T, B, 128) the multiplier inside the memory scan (gamma1's 64 units first), out_drop (T, B, 64) the multiplier
    behind out_fc1's ReLU -> (T, B, output_dim), time-major as the kernel path returns it."""
    g = lambda n: p[prefix + n]                                                          # noqa: E731
    lin = lambda name, x, act=0, **kw: E.linear(x, g(name + ".weight"), g(name + ".bias"), act=act, rounding=rounding, **kw)   # noqa: E731
    prev = [torch.cat([torch.zeros_like(c[:1]), c[:-1]], dim=0) for c in cs]
    c_star = torch.cat(prev + list(cs), dim=-1)
    att = torch.softmax(lin("att1_fc2", lin("att1_fc1", c_star, 1)), dim=-1)
    attended = att * c_star
    c_hat = lin("att2_fc2", lin("att2_fc1", attended, 1), 2)
    A = c_star.shape[-1]
    w1, w2 = g("gamma1_fc1.weight"), g("gamma2_fc1.weight")
    Wa, Wm = torch.cat([w1[:, :A], w2[:, :A]]), torch.cat([w1[:, A:], w2[:, A:]])
    b1 = torch.cat([g("gamma1_fc1.bias"), g("gamma2_fc1.bias")])
    apre = E.linear(attended, Wa, b1, rounding=rounding)
    W2 = torch.stack([g("gamma1_fc2.weight"), g("gamma2_fc2.weight")])
    b2 = torch.stack([g("gamma1_fc2.bias"), g("gamma2_fc2.bias")])
    mem_all = E.mfn_mem_scan(apre, c_hat, Wm, W2, b2, drop=gamma_drop, rounding=rounding)
    last = torch.cat(list(hs) + [mem_all], dim=-1)
    return lin("out_fc2", lin("out_fc1", last, 1, out_drop=out_drop))


def batch_composition(p, prefix, inputs, mods, rounding=True, hidden=None, gamma_drop=None, out_drop=None, mask=None, states=None):
    """The same gate from the batch path's pieces, as MFN._gate and functional._MfnGateFn compose their kernels: bf16_ref.linear ->
    bf16_ref.lstm_scan (lstm_states) -> shift and concatenate -> linear x2 -> softmax * cStar -> linear x2 -> linear (apre) ->
    bf16_ref.mfn_mem_scan -> linear x2 (gate_from_states) -> batch-major, times the window mask (B, T, 1) as F.batch_major(out, mask).
    inputs {mod: (T, B, d_mod)} -> (B, T, output_dim), with autograd wherever an argument requires grad.  ``hidden`` is kept for the
    callers that pass it: the hidden sizes are read from the weights.  states: a dict that receives "hs" and "cs"."""
    hs, cs = lstm_states(p, prefix, inputs, mods, rounding)
    if states is not None:
        states["hs"], states["cs"] = hs, cs
    out = gate_from_states(p, prefix, hs, cs, gamma_drop, out_drop, rounding).permute(1, 0, 2)
    return out if mask is None else out * mask.to(out.dtype)
