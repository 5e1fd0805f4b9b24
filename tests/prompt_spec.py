"""fp64 numpy restatement of ``act.prefix_concat_dropout`` (csrc/prefix_cat.hip, vlpet_prefix_concat_dropout_{fwd,bwd}):

    x[b] = dropout(cat([pre, a[b], v[b]], dim = 0), p)            pre [P, d] the same for every b, a [B, La, d], v [B, Lv, d]

The mask is the Philox site of tests/dropout_spec.py over the row-major x: ``keep_mask(B * (P + La + Lv), d, seed, p, ctr)``; kept
elements are scaled by ``keep_scale(p)`` (float arithmetic, as the kernels compute it).  Backward: da / dv are the masked, scaled slices
of dx; dpre[j, c] = sum over b of keep * scale * dx[b, j, c]."""
import numpy as np

import dropout_spec as DS

MAX_CHUNKS = 32          # csrc/kernels.h PREFIX_CAT_MAX_CHUNKS


def chunks(B: int):
    """csrc/prefix_cat.hip prefix_cat_split: (batch items per chunk, number of chunks) -- a function of B alone."""
    cs = (B + MAX_CHUNKS - 1) // MAX_CHUNKS
    return cs, (B + cs - 1) // cs


def scale(p: float) -> np.float32:
    """1 / (1 - p) in float arithmetic; 1 where the threshold rounds to no dropout at all"""
    return DS.keep_scale(p) if DS.tail_thr(p) else np.float32(1.0)


def keep(B, P, La, Lv, d, seed, p, ctr=None) -> np.ndarray:
    """[B, P + La + Lv, d] bool"""
    L = P + La + Lv
    return DS.keep_mask(B * L, d, seed, p, ctr).reshape(B, L, d)


def source(pre, a, v) -> np.ndarray:
    """cat([pre expanded, a, v], 1), fp64"""
    pre, a, v = (np.asarray(t, dtype=np.float64) for t in (pre, a, v))
    return np.concatenate([np.broadcast_to(pre[None], (a.shape[0],) + pre.shape), a, v], axis=1)


def forward(pre, a, v, seed, p, ctr=None):
    """(x in fp64 before the rounding to the IO dtype, keep mask)"""
    src = source(pre, a, v)
    B, L, d = src.shape
    k = keep(B, pre.shape[0], a.shape[1], v.shape[1], d, seed, p, ctr)
    return np.where(k, src * np.float64(scale(p)), 0.0), k


def backward(dx, P, La, Lv, seed, p, ctr=None):
    """(dpre [P, d] fp64, da, dv, sum over b of |term| [P, d]: the magnitude the accumulation bound of dpre is stated in)"""
    dx = np.asarray(dx, dtype=np.float64)
    B, L, d = dx.shape
    assert L == P + La + Lv
    k = keep(B, P, La, Lv, d, seed, p, ctr)
    g = np.where(k, dx * np.float64(scale(p)), 0.0)
    return g[:, :P].sum(0), g[:, P:P + La], g[:, P + La:], np.abs(g[:, :P]).sum(0)
