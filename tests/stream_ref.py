"""The bf16-faithful fp64 reference of the one-window encoder step (TEST INFRASTRUCTURE, a plain helper module beside
tests/causal_ref.py): a causal encoder stack walked window by window against a K / V list per layer, forward only.

Built from bf16_ref's pieces (bf16, the affine map, LOG2E) and oracle.layer_norm, with the same ``rounding`` switch: ``rounding=False``
is the exact function, so row t equals ``causal_ref.encoder_stack(..., rounding=False)[:, t]`` (tests/test_stream_cpu.py, 1e-12).

Sites, read from csrc/encoder_step.h (encoder_step_kernel).  Every line of a layer is causal_ref.encoder_layer's, on one row:
  * n0 = bf16(LN1(x_t)); Q' = bf16((n0 Wq^T + bq) log2(e) / sqrt(d_k)), Q' = 0 where mask_t == 0; K_t = bf16(.), V_t = bf16(.), both
    appended to the layer's lists whatever the mask says (the cache holds exactly these bf16 values);
  * attention of the one query over keys 0 .. t, per head, scores S_j = Q' . K_j in the log2 domain.  THE SOFTMAX REFERENCE POINT IS
    THE ROW'S OWN EXACT MAXIMUM m = max_j S_j: the batch kernel's lazily moved per-32-query-tile maximum (causal_ref._forward_value)
    looks at later queries of the tile, which a step cannot see.  P_j = bf16(2^(S_j - m)), the normaliser l = sum_j 2^(S_j - m) sums
    the UNROUNDED values (at every d_k: there is no ones-row form here), ctx = bf16((sum_j P_j V_j) / l);
  * x1 = x + ctx Wo^T + bo; n1 = bf16(LN2(x1)); hid = bf16(relu(n1 W1^T + b1)); x2 = x1 + hid W2^T + b2; LayerNorm statistics, biases,
    residuals and the final LayerNorm unrounded.
Not emulated, as in bf16_ref: fp32 accumulation order and the hardware exp2.
"""
import math

import torch

import bf16_ref as E
import oracle


class EncoderStream:
    """step(x_t (B, d), mask_t (B,) or None) -> y_t (B, d); keeps K and V of every layer for the windows seen so far."""

    def __init__(self, p, prefix, h, rounding=True):
        self.p, self.prefix, self.h, self.rounding = p, prefix, h, rounding
        self.n = oracle.count_layers(p, prefix)
        self.reset()

    def reset(self):
        self.K = [[] for _ in range(self.n)]
        self.V = [[] for _ in range(self.n)]
        self.t = 0

    def _attend(self, layer, q, k, v, keep):
        """q, k, v: (B, d) affine outputs of this window -> merged context (B, d)"""
        rf = E.bf16 if self.rounding else (lambda z: z)
        B, d = q.shape
        h = self.h
        dk = d // h
        Qs = q * (E.LOG2E / math.sqrt(dk))
        if keep is not None:
            Qs = Qs * keep.reshape(B, 1)
        Qp = rf(Qs).reshape(B, h, 1, dk)
        self.K[layer].append(rf(k).reshape(B, h, 1, dk))
        self.V[layer].append(rf(v).reshape(B, h, 1, dk))
        K, V = torch.cat(self.K[layer], dim=2), torch.cat(self.V[layer], dim=2)          # (B, h, t + 1, d_k)
        S = Qp @ K.transpose(-2, -1)                                                      # (B, h, 1, t + 1), log2 domain
        if not self.rounding:
            return (torch.softmax(S * E.LN2, dim=-1) @ V).reshape(B, d)
        m = S.amax(dim=-1, keepdim=True)                                                  # the row's own exact maximum
        P = torch.exp2(S - m)
        l = P.sum(dim=-1, keepdim=True)                                                   # the unrounded values
        return E.bf16((E.bf16(P) @ V) / l).reshape(B, d)

    def step(self, x_t, mask_t=None):
        with torch.no_grad():
            p = self.p
            rf = E.bf16 if self.rounding else (lambda z: z)
            keep = None if mask_t is None else (mask_t.reshape(-1) != 0).to(x_t.dtype)
            x = x_t
            for i in range(self.n):
                L = "%slayers.%d." % (self.prefix, i)
                n0 = rf(oracle.layer_norm(x, p[L + "sublayer.0.norm.a_2"], p[L + "sublayer.0.norm.b_2"]))
                a = L + "self_attn.linears."
                q, k, v = (E._affine(p, a + str(j), n0, rf) for j in range(3))
                x = x + E._affine(p, a + "3", self._attend(i, q, k, v, keep), rf)
                n1 = rf(oracle.layer_norm(x, p[L + "sublayer.1.norm.a_2"], p[L + "sublayer.1.norm.b_2"]))
                f = L + "feed_forward."
                hid = torch.relu(E._affine(p, f + "w_1", n1, rf))
                x = x + E._affine(p, f + "w_2", rf(hid), rf)
            self.t += 1
            return oracle.layer_norm(x, p[self.prefix + "norm.a_2"], p[self.prefix + "norm.b_2"])


def encoder_stack(p, prefix, x, mask, h, rounding=True):
    """causal_ref.encoder_stack's arguments (eval mode: no drops) -> (B, T, d), computed one window at a time."""
    s = EncoderStream(p, prefix, h, rounding)
    rows = [s.step(x[:, t], None if mask is None else mask[:, t].reshape(-1)) for t in range(x.shape[1])]
    return torch.stack(rows, dim=1)
