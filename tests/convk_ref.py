"""The bf16-faithful fp64 reference of the K-tap window encoder (csrc/convk.h), 1 <= K (TEST INFRASTRUCTURE, a plain helper module).

bf16_ref.conv_sums / conv_maxpool / conv_plan with the kernel size taken from w.shape[2], built on bf16_ref's primitives and rounding
at the same sites: x and w are INPUTS, rounded to bf16 without jitter (convk_prep_kernel; the staging of convk_fwd_kernel and
convk_bwd_kernel), the sums S[n, p, f] = sum_j bf16(x)[n, p + j] . bf16(w)[f, :, j] over the W - K + 1 positions are fp64 here and fp32
in the kernel, the pool takes the FIRST maximum, the bias is added after the pool, dW sums bf16(dy) and db the unrounded dy.
With rounding=False it is oracle.frontend_ref.cnn_maxpool; at K = 2 with rounding it is bf16_ref.conv_maxpool (tests/test_convk_cpu.py).
"""
import math

import torch

import bf16_ref as E

K_MAX = 5                   # csrc/convk.h CK_MAXK
CT_BULK = 2                 # csrc/convk.h CK_CT: 128 channels per forward workgroup


def _taps(xr, wr, fx=lambda t: t, fw=lambda t: t):
    K, L = wr.shape[2], xr.shape[1] - wr.shape[2] + 1
    S = 0
    for j in range(K):
        S = S + fx(xr[:, j:j + L]) @ fw(wr[:, :, j]).t()
    return S


def conv_sums(x, w, rounding=True):
    """S (N, W-K+1, F) without the bias, and per (n, p, f) the sum of |terms| (for the fp32 dot-product bound), no autograd"""
    with torch.no_grad():
        xr, wr = (E._exact_bf16(x), E._exact_bf16(w)) if rounding else (x, w)
        return _taps(xr, wr), _taps(xr, wr, torch.abs, torch.abs)


def conv_maxpool(x, w, b, arg=None, rounding=True):
    """Same arguments as functional.conv_maxpool_k (x (N, W, D), w (F, D, K), b (F,)) -> (out (N, F), arg (N, F), S (N, W-K+1, F)
    without the bias).  arg given: the pool gathers at those positions, so autograd yields the exact gradient for that choice.  Under
    bf16_ref.jitter the operands are not perturbed (inputs); the sums are, by eps * sqrt(K D) * sqrt(sum of the squared terms)."""
    rin = E._RoundInput.apply if rounding else (lambda t: t)
    xr, wr = rin(x), rin(w)
    S = _taps(xr, wr)
    if E._JITTER is not None:
        g, eps = E._JITTER
        with torch.no_grad():
            sq = _taps(xr, wr, torch.square, torch.square)
            noise = eps * math.sqrt(w.shape[2] * x.shape[2]) * sq.sqrt() * torch.randn(sq.shape, generator=g, dtype=sq.dtype)
        S = S + noise
    if arg is None:
        arg = S.detach().argmax(dim=1)                          # argmax: the first position of the maximum
    pooled = S.gather(1, arg.long().unsqueeze(1)).squeeze(1)
    if rounding:
        pooled = E.round_bwd(pooled)                            # dW from bf16(dy), db from dy
    return pooled + b, arg, S.detach()


def conv_plan(N, W, D, F, K):
    """What mmt_convpool_k_forward / _backward launch for (N, W, D, F, K): a mirror of carve_conv with ktap = true and of the forward's
    channel dispatch (csrc/api.hip).  The backward's grid carries the tap, so `blocks` counts it; fwd lists the forward launches as (K, CT, channel
    blocks, c_first); one_rt is the backward instance (at most 32 conv positions)."""
    up = lambda a, m: -(-a // m) * m  # noqa: E731
    FPAD, DPB = up(F, 256), up(D, 128)
    blocks = K * (DPB // 128) * (FPAD // 256)
    ns = max(1, min(-(-512 // blocks), (N + 1) // 2))
    wins = up(-(-N // ns), 2)
    nsplit = -(-N // wins)
    cfb = 64 * CT_BULK
    nmain, rem = F // cfb, F % cfb
    fwd = [(K, CT_BULK, nmain, 0)] if nmain else []
    if rem > 64:
        fwd.append((K, CT_BULK, 1, nmain * cfb))
    elif rem > 0:
        fwd.append((K, 1, 1, nmain * cfb))
    npos = W - K + 1
    return {"nsplit": nsplit, "wins": wins, "last": N - (nsplit - 1) * wins, "npairs": (min(wins, N) + 1) // 2, "nrt": -(-npos // 32),
            "one_rt": npos <= 32, "fwd": fwd, "fwd_wgs": -(-N // 8), "bwd_grid": (K * (DPB // 128), nsplit, FPAD // 256)}
