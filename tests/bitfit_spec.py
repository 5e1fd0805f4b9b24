"""fp64 statements of the two entry points of csrc/biasgrad.hip (include/vlpet_hip.h: vlpet_colsum_seg, vlpet_act_dropout_bwd_cols),
each with the bound an fp32 evaluation in the kernels' order must meet, in the manner of tests/tail_spec.py / tests/rowgate_spec.py.

The bound of a sum.  Both kernels add fp32 numbers in a fixed tree.  For ANY tree, the computed sum s^ of terms t_i satisfies
|s^ - sum t_i| <= gamma_h sum |t_i| with gamma_h = h u / (1 - h u), u = 2^-24, h = the largest number of additions any one term passes
through (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2: each term is multiplied by at most h factors
(1 + delta), |delta| <= u).  h is counted from the code, nothing is added to it:

    first pass    a wave adds its rows one by one                       rows per wave   = ceil(M / (4 nb))
                  wave 0 adds the four waves' sums to 0                 4
    reduce        a thread adds every 16th partial row: groups of four as (a0 + a1) + (a2 + a3), then into v (3 additions for
                  a term, later groups add 1 each), single rows after that; at most ceil(nb / 16) additions into v, + 2
                  16 threads' values are added to 0                     16

nb = partial rows: tail_blocks(M) for the segmented sum (csrc/tail.hip), act_cols_partials(M, n_cols) for the activation backward.
The terms are what the kernel reads / stores, already rounded to the IO dtype, so they carry no error of their own: the activation
backward sums dx AS STORED -- that rounding is part of the OPERATION, not of the error model (mutation "unrounded")."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import dropout_spec as DS

U = 2.0 ** -24
WAVES = 4
CAPS = ((2500, 256), (8500, 512), (None, 1024))       # csrc/tail.hip tail_blocks: rows up to -> workgroups at most
ACT_COLS_CAP = 2048                                   # csrc/biasgrad.hip: workgroups of the activation backward's grid at most
MAX_SEGS = 16
ACTS = {"gelu": 0, "gelu_new": 1, "relu": 2}
MUTATIONS = ("seg_shift", "unrounded", "mask_shift")


def tail_blocks(M: int) -> int:
    cap = next(c for top, c in CAPS if top is None or M <= top)
    return min((M + WAVES - 1) // WAVES, cap)


def act_cols_partials(M: int, n_cols: int) -> int:
    gx = (n_cols // 8 + 63) // 64
    return min((M + WAVES - 1) // WAVES, max(ACT_COLS_CAP // gx, 1))


def grid_edges():
    """Row counts on both sides of every change of tail_blocks' rule: where the grid stops growing under the first cap, and the two
    thresholds at which the cap steps up."""
    return [CAPS[0][1] * WAVES, CAPS[0][1] * WAVES + 1, 2500, 2501, 8500, 8501]


def depth(M: int, nb: int) -> int:
    return math.ceil(M / (WAVES * nb)) + WAVES + math.ceil(nb / 16) + 2 + 16


def gamma(h: int) -> float:
    return h * U / (1.0 - h * U)


def _c(t, ct):
    return torch.as_tensor(t).detach().cpu().to(ct)


def round_io(t: torch.Tensor, dtype) -> torch.Tensor:
    return t.to(torch.float32).to(dtype).to(t.dtype)


# ------------------------------------------------------------------------------------------------------------------ segmented sums
def colsum_seg(x, S: int, w: int, ct=torch.float64, mut=()):
    """x [M, ld] (IO dtype; columns >= S w are guard columns that do not belong to the matrix).  -> out [S, w] = column sums of
    segment s = columns [s w, (s + 1) w), e_out = gamma_h sum |x| per column."""
    M = x.shape[0]
    n = S * w
    xc = _c(x, ct)
    lo = 1 if "seg_shift" in mut else 0                  # mutation: every segment starts one column late
    body = xc[:, lo:lo + n]
    h = depth(M, tail_blocks(M))
    return SimpleNamespace(out=body.sum(0).reshape(S, w), e_out=(gamma(h) * xc[:, :n].abs().sum(0)).reshape(S, w), h=h)


def kernel_order_sum(t: torch.Tensor, nb: int) -> torch.Tensor:
    """Column sums of t [M, n] in t's own dtype in the kernels' order (see the module docstring): the restatement whose error the
    bound is derived for."""
    M, n = t.shape
    rpw = math.ceil(M / (WAVES * nb))
    pad = torch.zeros(rpw * WAVES * nb - M, n, dtype=t.dtype)
    g = torch.cat([t, pad]).reshape(rpw, nb, WAVES, n)   # row = 4 b + w + 4 nb k  ->  [k, b, w]
    s = torch.zeros(nb, WAVES, n, dtype=t.dtype)
    for k in range(rpw):
        s = s + g[k]
    part = torch.zeros(nb, n, dtype=t.dtype)
    for wv in range(WAVES):
        part = part + s[:, wv]
    tot = torch.zeros(n, dtype=t.dtype)
    for th in range(16):
        v = torch.zeros(n, dtype=t.dtype)
        r = th
        while r + 48 < nb:
            v = v + ((part[r] + part[r + 16]) + (part[r + 32] + part[r + 48]))
            r += 64
        while r < nb:
            v = v + part[r]
            r += 16
        tot = tot + v
    return tot


# --------------------------------------------------------------------------------------------------- activation backward + column sums
_C = math.sqrt(2.0 / math.pi)


def act_df(act: str, x: torch.Tensor) -> torch.Tensor:
    """act'(x) in x's dtype: F.gelu (erf form), HF NewGELUActivation (tanh form), relu -- the forms that keep their accuracy in the tails
    (Phi = erfc(-x / sqrt 2) / 2; 1 - tanh^2 u = 4 s (1 - s) with s = sigmoid(2 u), 1 - s = sigmoid(-2 u))."""
    if act == "relu":
        return (x > 0).to(x.dtype)
    if act == "gelu":
        cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
        return cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    v = 2.0 * _C * (x + 0.044715 * x ** 3)
    s = torch.sigmoid(v)
    return s + x * 2.0 * s * torch.sigmoid(-v) * _C * (1.0 + 3 * 0.044715 * x * x)      # 1 - s as sigmoid(-v): no cancellation in fp32


def e_act_df(act: str, x: torch.Tensor, df: torch.Tensor) -> torch.Tensor:
    """What the device derivative may miss (tests/test_gpu_act.py test_activation_value_sweep holds the kernel's act'(x) to these): relu
    exact; the gelu forms 4e-7 min(|x|, 1) + 2^-22 |df| (Abramowitz & Stegun 7.1.26 on Phi, one ulp each of the hardware reciprocal
    and exponential)."""
    if act == "relu":
        return torch.zeros_like(df)
    return 4e-7 * x.abs().clamp_max(1.0) + 2.0 ** -22 * df.abs()


def keep_mask(M, n_cols, seed, p, ctr=None, mut=()) -> torch.Tensor:
    """group of element (row, col) = (row * n_cols + col) / 8: the flat index of vlpet_act_dropout_bwd"""
    k = torch.from_numpy(np.ascontiguousarray(DS.keep_mask(M, n_cols, seed, p, ctr)))
    if "mask_shift" in mut:
        k = torch.roll(k.reshape(-1, 8), 1, 0).reshape(k.shape)
    return k


def act_dropout_bwd_cols(dy, x, act: str, p: float, seed: int, ctr=None, ct=torch.float64, mut=()):
    """dy, x [M, n_cols] (IO dtype).  dx = dy * keep / (1 - p) * act'(x); sums [n_cols] = column sums of dx ROUNDED TO THE IO DTYPE.
    e_dx: bound before the rounding to the IO dtype (two products, the derivative's own error); e_sums = gamma_h sum |round(dx)|."""
    dtype = x.dtype
    M, n_cols = x.shape
    thr = DS.tail_thr(p)
    k = keep_mask(M, n_cols, seed, p, ctr, mut).to(ct) * float(DS.keep_scale(p)) if thr else torch.ones(M, n_cols, dtype=ct)
    xc, dyc = _c(x, ct), _c(dy, ct)
    df = act_df(act, xc)
    dx = dyc * k * df
    e_dx = (dyc * k).abs() * e_act_df(act, xc, df) + 3 * U * dx.abs()
    stored = dx if "unrounded" in mut else round_io(dx, dtype)
    r = SimpleNamespace(dx=dx, e_dx=e_dx, stored=stored)
    r.sums, r.e_sums, r.h = colsums_of_stored(stored, n_cols)
    return r


def colsums_of_stored(dx_stored, n_cols: int):
    """-> (fp64 column sums of the given stored dx [M, n_cols], their bound, h): what the GPU test holds the kernel's sums to, from the dx
    the kernel itself stored."""
    d = _c(dx_stored, torch.float64)
    M = d.shape[0]
    h = depth(M, act_cols_partials(M, n_cols))
    return d.sum(0), gamma(h) * d.abs().sum(0), h


def hold_io(e, ref, dtype):
    """e plus, for a bf16 result, the one rounding to bf16 at the magnitude of the result (tail_spec.hold_bound)"""
    if dtype != torch.bfloat16:
        return e
    mag = (ref.abs() + e).clamp_min(2.0 ** -126)
    return e + torch.exp2(torch.floor(torch.log2(mag)) - 8)


def worst(got, ref, bound) -> float:
    """largest err / bound (NaN -- an unwritten element -- counts as infinite)"""
    err = (got.detach().double().cpu() - ref.double()).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.double().clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
