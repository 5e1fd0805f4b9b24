"""fp64 statements of the entry points of csrc/tail.hip (include/vlpet_hip.h: the K5 sublayer tail, the RMS forms, the LayerNorm
backward forms that ride on its backward kernel, the partial reduce and the column sum), one function per entry point, taking that
entry point's inputs.

Row tensors arrive already rounded to the IO dtype (bf16 or fp32 torch tensors; the IO dtype is read from them), parameters and
saved statistics are fp32.  Everything is evaluated in ``ct`` = fp64.  The same functions evaluated with ``ct = torch.float32`` are
"the reference alone, in fp32": tests/test_tail_spec.py holds that restatement to every bound the GPU test uses.

The keep mask is always ``dropout_spec.keep_mask(M, d, seed, p, ctr)`` -- a function of (seed, step counter, element index), never
something a kernel exported.  ``keep=`` replaces it and ``mut=`` names a deliberate mis-statement; both exist only for the tests
that show the bounds can be missed.

Beside each value ``v`` a function returns ``e_v``: the bound on |kernel - v| BEFORE the final rounding to the IO dtype, built from
the sums of absolute terms as derived in tests/test_gpu_tail_edges.py (``hold_bound`` adds that rounding).  Two integers enter it:
``n`` = additions of a row statistic (ceil(d / 64) per lane + 6 shuffle steps) and, for the partials, the rows a wave walks.

One rounding is part of the OPERATION, not of the error model: vlpet_sublayer_tail_rms_fwd normalises the sum ROUNDED TO THE IO
DTYPE (the statistic and the normed rows read the sum as a second launch would have read it from memory)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import dropout_spec as DS

U = 2.0 ** -24
TAIL_WAVES = 4
# Relative error allowed to the device rsqrtf.  It is not stated in the ROCm headers or documents shipped with the toolchain, so it is
# 4 x the worst relative error of the fp32 CPU restatement's rsqrt against fp64 on the suite's inputs (1 / sqrt, two correctly rounded steps: 1.31 u, measured by
# tests/test_tail_spec.py::test_rsqrt_allowance_is_four_times_the_cpu_figure, which also holds the figure): a different
# summation tree in front of it plus an approximate instruction.  profiles/tail_edges_tests.md records the measurement.
RSQRT_CPU_WORST_U = 1.31
R_RSQRT = 4 * RSQRT_CPU_WORST_U * U

MUTATIONS = ("padded_width", "last_piece", "uncentred", "c1_in_rms", "mask_shift", "mask_swap", "no_beta", "partial_missing",
             "rms2_unrounded")


def n_stat(d: int) -> int:
    return math.ceil(d / 64) + 6


def form(dtype, d: int):
    """Host restatement of tail_pieces8 / launch_io / launch_np (csrc/tail.hip): -> (piece bytes, pieces per lane, FULL with
    16-byte-aligned parameters), or None where launch_io refuses the width."""
    if d <= 0 or d % 8:
        return None
    if dtype == torch.bfloat16:
        np16, np8 = (d // 8 + 63) // 64, (d // 4 + 63) // 64
        if np8 <= 4 and np8 * 4 < np16 * 8:
            return 8, np8, d == np8 * 64 * 4
        if np16 > 8:
            return None
        np_ = next(k for k in (1, 2, 3, 4, 8) if np16 <= k)
        return 16, np_, np_ <= 4 and d == np_ * 64 * 8
    np16 = (d // 4 + 63) // 64
    if np16 > 8:
        return None
    return 16, next(k for k in (1, 2, 3, 4, 8) if np16 <= k), False


def padded_width(dtype, d: int) -> int:
    pb, np_, _ = form(dtype, d)
    return np_ * 64 * (pb // (2 if dtype == torch.bfloat16 else 4))


def piece_elems(dtype, d: int) -> int:
    return form(dtype, d)[0] // (2 if dtype == torch.bfloat16 else 4)


def keep_mask(M, d, seed, p, ctr=None) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(DS.keep_mask(M, d, seed, p, ctr)))


def shifted_mask(k: torch.Tensor) -> torch.Tensor:
    """mutation: every 8-element group takes the bits of the group before it"""
    return torch.roll(k.reshape(-1, 8), 1, 0).reshape(k.shape)


def swapped_mask(k: torch.Tensor) -> torch.Tensor:
    """mutation: the two 4-element halves of a group (lanes 2j / 2j + 1 of the 8-byte and fp32 forms) exchanged"""
    return k.reshape(-1, 2, 4).flip(1).reshape(k.shape)


def _c(t, ct):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(ct)


def round_io(t: torch.Tensor, dtype) -> torch.Tensor:
    """Round to the IO dtype (nearest even) and return in t's dtype."""
    return t.to(torch.float32).to(dtype).to(t.dtype)


def hold_bound(e, ref, dtype):
    """e, plus for a bf16 output the one rounding: half a unit in the last of bf16's 8 significant bits at the magnitude of the
    result (the form of test_gpu_rowgate._el_bound); an fp32 output's rounding is inside the 4 u terms."""
    if dtype != torch.bfloat16:
        return e
    mag = (ref.abs() + e).clamp_min(2.0 ** -126)
    return e + torch.exp2(torch.floor(torch.log2(mag)) - 8)


def _scale(p, ct):
    return float(DS.keep_scale(p)) if DS.tail_thr(p) else 1.0


def _dropped_sum(y, x1, p, seed, ctr, keep, ct):
    """h = x1 + keep * y * scale with its absolute terms; e_h = 2 u h_abs (the product, then the sum; the two may be fused).  Without
    dropout the sum is ONE correctly rounded fp32 addition, whose error is known exactly (0 for almost every pair of bf16 numbers)."""
    M, d = x1.shape
    k = keep if keep is not None else keep_mask(M, d, seed, p, ctr)
    x = _c(x1, ct)
    t = torch.zeros_like(x) if y is None else _c(y, ct) * _scale(p, ct) * k.to(ct)
    h, h_abs = x + t, x.abs() + t.abs()
    if y is None:
        e_h = torch.zeros_like(h)
    elif DS.tail_thr(p):
        e_h = 2 * U * h_abs * k.to(ct)          # (a dropped element is x1 itself)
    else:
        e_h = (h.to(torch.float32).to(ct) - h).abs()
    return h, h_abs, e_h, k


def _stats(h, h_abs, e_h, d, eps, rms, dtype, mut=()):
    """mean (0 in RMS mode) and rstd = (var + eps)^-1/2 of each row, the variance CENTRED (second pass over h - mean)."""
    n = n_stat(d)
    M = h.shape[0]
    dd, hs = d, h
    if "padded_width" in mut:
        dd = padded_width(dtype, d)
    if "last_piece" in mut:
        hs = h[:, :d - piece_elems(dtype, d)]
    if rms:
        mean, e_mean = torch.zeros(M, dtype=h.dtype), torch.zeros(M, dtype=h.dtype)
    else:
        mean = hs.sum(1) / dd
        e_mean = (n + 8) * U * h_abs.mean(1)
    c = h - mean[:, None]
    e_c = e_h + e_mean[:, None] + U * c.abs()
    cs = c if "last_piece" not in mut else c[:, :hs.shape[1]]
    var = ((hs * hs) if "uncentred" in mut else (cs * cs)).sum(1) / dd
    e_var = (n + 8) * U * var + (2 * c.abs() * e_c + e_c * e_c).mean(1)
    v = var + eps
    rel = (e_var + U * v) / v
    rstd = 1.0 / torch.sqrt(v)           # (both correctly rounded in any IEEE arithmetic: the fp32 restatement is the same everywhere)
    e_rstd = rstd * (0.5 * rel * (1 + rel) + R_RSQRT)
    return mean, e_mean, rstd, e_rstd, c, e_c


# ---------------------------------------------------------------------------------------------------------------- forward
def sublayer_tail_fwd(y, x1, gamma, beta, eps, p, seed, norm_mode, ctr=None, ct=torch.float64, keep=None, mut=(), post=False,
                      rms=False):
    """norm_mode 1: out = LayerNorm(x1 + dropout(y)) * gamma + beta, h_save = the pre-norm sum, mean / rstd [M];
    norm_mode 0: out = x1 + dropout(y).  keep_out = the mask.  (post / rms: the two forms below.)"""
    dtype = x1.dtype
    M, d = x1.shape
    if post:            # statistics of y alone; the residual joins after the norm
        h, h_abs, e_h, k = _dropped_sum(None, y, 0.0, 0, None, None, ct)
        h_abs, e_h = h.abs(), torch.zeros_like(h)
    else:
        h, h_abs, e_h, k = _dropped_sum(y, x1, p, seed, ctr, keep, ct)
    r = SimpleNamespace(keep=k, h=h, e_h=e_h)
    if not norm_mode:
        r.out, r.e_out = h, e_h
        return r
    mean, e_mean, rstd, e_rstd, c, e_c = _stats(h, h_abs, e_h, d, eps, rms, dtype, mut)
    g = _c(gamma, ct)
    b = _c(beta, ct) if beta is not None else torch.zeros_like(g)
    xg = c * rstd[:, None] * g
    out = xg + b
    e_out = g.abs() * (e_c * rstd[:, None] + c.abs() * e_rstd[:, None]) + 4 * U * (xg.abs() + b.abs())
    if post:
        res = _c(x1, ct)
        out, e_out = out + res, e_out + 4 * U * res.abs()
    r.mean, r.e_mean, r.rstd, r.e_rstd, r.out, r.e_out = mean, e_mean, rstd, e_rstd, out, e_out
    return r


def norm_residual_fwd(y, r, gamma, beta, eps, ct=torch.float64, mut=()):
    """out = LayerNorm(y) * gamma + beta + r: the statistics are those of y alone."""
    return sublayer_tail_fwd(y, r, gamma, beta, eps, 0.0, 0, 1, ct=ct, mut=mut, post=True)


def rmsnorm_fwd(x, gamma, eps, ct=torch.float64, mut=()):
    """out = x * rsqrt(mean(x^2) + eps) * gamma; rstd [M] (no mean is written)."""
    return sublayer_tail_fwd(None, x, gamma, None, eps, 0.0, 0, 1, ct=ct, mut=mut, rms=True)


def sublayer_tail_rms_fwd(y, x1, gamma_next, eps, p, seed, ctr=None, ct=torch.float64, keep=None, mut=()):
    """sum = x1 + dropout(y);  normed = rmsnorm(round_io(sum)) * gamma_next -- the norm reads the sum ROUNDED TO THE IO DTYPE.
    e_hr: how far the kernel's rounded sum may lie from the spec's (0 unless the sum is within e_h of a rounding boundary, then one
    unit in the last place)."""
    dtype = x1.dtype
    M, d = x1.shape
    h, h_abs, e_h, k = _dropped_sum(y, x1, p, seed, ctr, keep, ct)
    if dtype == torch.bfloat16 and "rms2_unrounded" not in mut:
        hr = round_io(h, dtype)
        e_hr = torch.maximum((round_io(h - e_h, dtype) - hr).abs(), (round_io(h + e_h, dtype) - hr).abs())
    else:
        hr, e_hr = h, e_h
    _, _, rstd, e_rstd, c, e_c = _stats(hr, hr.abs(), e_hr, d, eps, True, dtype, mut)
    g = _c(gamma_next, ct)
    normed = hr * rstd[:, None] * g
    e_normed = g.abs() * (e_c * rstd[:, None] + hr.abs() * e_rstd[:, None]) + 4 * U * normed.abs()
    return SimpleNamespace(keep=k, sum=h, e_sum=e_h, rstd=rstd, e_rstd=e_rstd, normed=normed, e_normed=e_normed)


# ---------------------------------------------------------------------------------------------------------------- backward
def block_rows(M: int, nb: int) -> torch.Tensor:
    """workgroup of each row: wave w of workgroup b walks rows 4 b + w, + 4 nb, ..."""
    return (torch.arange(M) // TAIL_WAVES) % nb


def block_partials(terms: torch.Tensor, nb: int) -> torch.Tensor:
    """[nb, d]: the sum, per workgroup, of its rows of ``terms`` [M, d]"""
    out = torch.zeros(nb, terms.shape[1], dtype=terms.dtype)
    return out.index_add_(0, block_rows(terms.shape[0], nb), terms)


def partial_bound(terms_abs, e_terms, M: int, nb: int):
    """a partial = rows-per-wave additions + the 4-wave combine, (+ 8) u on the absolute terms, plus what the terms carry"""
    rpw = math.ceil(M / (nb * TAIL_WAVES))
    return (rpw + 4 + 8) * U * block_partials(terms_abs, nb) + block_partials(e_terms, nb)


def _norm_bwd(dout, x, e_x, rstd, gamma, d, rms, dres, p, seed, ctr, keep, ct, mut=()):
    """dx = (g - mean(g) - x mean(g x)) rstd with g = dout gamma (no mean(g) in RMS mode) [+ dres]; dy = dx keep / (1 - p);
    dgamma rows = dout x, dbeta rows = dout."""
    n = n_stat(d)
    M = dout.shape[0]
    do, g_ = _c(dout, ct), _c(gamma, ct)
    rs = _c(rstd, ct)[:, None]
    g = do * g_
    gx = g * x
    c1 = torch.zeros(M, 1, dtype=ct) if (rms and "c1_in_rms" not in mut) else g.mean(1, keepdim=True)
    e_c1 = torch.zeros(M, 1, dtype=ct) if rms else (n + 8) * U * g.abs().mean(1, keepdim=True)
    c2 = gx.mean(1, keepdim=True)
    e_c2 = (n + 8) * U * gx.abs().mean(1, keepdim=True) + (g.abs() * e_x).mean(1, keepdim=True)
    t = g - c1 - x * c2
    e_t = e_c1 + x.abs() * e_c2 + c2.abs() * e_x + 4 * U * (g.abs() + c1.abs() + (x * c2).abs())
    dx = t * rs
    e_dx = rs * e_t + U * dx.abs()
    if dres is not None:
        dr = _c(dres, ct)
        e_dx = e_dx + U * (dx.abs() + dr.abs())
        dx = dx + dr
    r = SimpleNamespace(dx1=dx, e_dx1=e_dx, dg_rows=do * x, db_rows=do)
    r.e_dg_rows = do.abs() * e_x + U * r.dg_rows.abs()
    r.e_db_rows = torch.zeros_like(do)
    _dy(r, dx, e_dx, p, seed, ctr, keep, ct)
    return r


def _dy(r, dx, e_dx, p, seed, ctr, keep, ct):
    if DS.tail_thr(p):
        M, d = dx.shape
        k = keep if keep is not None else keep_mask(M, d, seed, p, ctr)
        s = _scale(p, ct)
        r.keep, r.dy = k, dx * s * k.to(ct)
        r.e_dy = (s * e_dx + U * r.dy.abs()) * k.to(ct)
    else:
        r.keep, r.dy, r.e_dy = None, dx, e_dx             # p = 0: dy IS dx1 (the caller aliases)


def sublayer_tail_bwd(dout, h_save, mean, rstd, gamma, p, seed, norm_mode, ctr=None, ct=torch.float64, keep=None, mut=()):
    """norm_mode 1: the LayerNorm backward from the saved pre-norm sum and statistics.  norm_mode 0: dx1 = dout (NULL in the aliased
    form: the caller hands dout on), dy = dout keep / (1 - p)."""
    d = dout.shape[1]
    if not norm_mode:
        do = _c(dout, ct)
        r = SimpleNamespace(dx1=do, e_dx1=torch.zeros_like(do))
        _dy(r, do, r.e_dx1, p, seed, ctr, keep, ct)
        return r
    x = (_c(h_save, ct) - _c(mean, ct)[:, None]) * _c(rstd, ct)[:, None]
    return _norm_bwd(dout, x, 2 * U * x.abs(), rstd, gamma, d, False, None, p, seed, ctr, keep, ct, mut)


def sublayer_tail_bwd_out(dout, out_save, rstd, gamma, beta, p, seed, ctr=None, ct=torch.float64, keep=None, mut=()):
    """The same from the LayerNorm OUTPUT rows: xhat = (out_save - beta) / gamma, 0 where gamma == 0.  out_save is an input: xhat
    is recovered from the rows as given (what the rounding of `out` cost the forward is not this entry point's error)."""
    g = _c(gamma, ct)
    gi = torch.where(g != 0, 1.0 / torch.where(g != 0, g, torch.ones_like(g)), torch.zeros_like(g))
    b = _c(beta, ct) if (beta is not None and "no_beta" not in mut) else torch.zeros_like(g)
    a1, a2 = _c(out_save, ct) * gi, b * gi
    x = a1 - a2
    e_x = 4 * U * (a1.abs() + a2.abs())
    return _norm_bwd(dout, x, e_x, rstd, gamma, dout.shape[1], False, None, p, seed, ctr, keep, ct, mut)


def layernorm_bwd_xhat(dout, xhat, rstd, gamma, ct=torch.float64, mut=()):
    x = _c(xhat, ct)
    return _norm_bwd(dout, x, torch.zeros_like(x), rstd, gamma, dout.shape[1], False, None, 0.0, 0, None, None, ct, mut)


def rmsnorm_bwd(dout, x, rstd, gamma, dx_in=None, ct=torch.float64, mut=()):
    """dx = rmsnorm'(dout) [+ dx_in]; the dgamma rows (no dbeta is meaningful: the partials' second half holds sum dout)."""
    xh = _c(x, ct) * _c(rstd, ct)[:, None]
    return _norm_bwd(dout, xh, U * xh.abs(), rstd, gamma, dout.shape[1], True, dx_in, 0.0, 0, None, None, ct, mut)


def rmsnorm_tail_bwd(d_normed, sum_, rstd, gamma_next, dsum_in, p, seed, ctr=None, ct=torch.float64, keep=None, mut=()):
    """d_sum = rmsnorm'(d_normed) [+ dsum_in]; dx1 = d_sum; dy = d_sum keep / (1 - p)."""
    xh = _c(sum_, ct) * _c(rstd, ct)[:, None]
    return _norm_bwd(d_normed, xh, U * xh.abs(), rstd, gamma_next, d_normed.shape[1], True, dsum_in, p, seed, ctr, keep, ct, mut)


# ---------------------------------------------------------------------------------------------------------------- reductions
def sublayer_tail_reduce(partials, d, ct=torch.float64, mut=()):
    """partials [nb, 2, d] -> dgamma [d], dbeta [d]: plain sums.  A thread of the kernel adds ceil(nb / 16) values, 16 are combined."""
    pt = _c(partials, ct).reshape(-1, 2, d)
    nb = pt.shape[0]
    ps = pt[1:] if "partial_missing" in mut else pt
    s, a = ps.sum(0), pt.abs().sum(0)
    e = (math.ceil(nb / 16) + 16 + 8) * U * a
    return SimpleNamespace(dgamma=s[0], dbeta=s[1], e_dgamma=e[0], e_dbeta=e[1])


def colsum(x, nb, ct=torch.float64):
    """out [n] = column sums of x [M, n]: per-workgroup partials (rows per wave + 4 waves), then the reduce above."""
    xc = _c(x, ct)
    M = xc.shape[0]
    rpw = math.ceil(M / (nb * TAIL_WAVES))
    e = (rpw + 4 + math.ceil(nb / 16) + 16 + 8) * U * xc.abs().sum(0)
    return SimpleNamespace(out=xc.sum(0), e_out=e)


# ------------------------------------------------------------------------------------------- the suite's inputs and its operations
P0, SEED, EPS = 0.1, 0x1234_5678_9ABC_DEF1, 1e-5
CAPS = ((2500, 256), (8500, 512), (None, 1024))       # csrc/tail.hip tail_blocks: rows up to -> workgroups at most


def tail_blocks(M: int) -> int:
    cap = next(c for top, c in CAPS if top is None or M <= top)
    return min((M + TAIL_WAVES - 1) // TAIL_WAVES, cap)


def _rn(i, d, *shape):
    """Seeded normal numbers whose first rows do not depend on the row count (numpy's legacy generator fills in order)."""
    return torch.from_numpy(np.random.RandomState(1000 * d + i).standard_normal(shape)).float()


def _nonzero(t, floor=2.0 ** -6):
    """no element closer to zero than ``floor``: a dropped element (exactly 0) cannot be mistaken for a kept one"""
    return torch.where(t.abs() < floor, torch.where(t < 0, -floor, floor).to(t.dtype), t)


def make_inputs(dtype, M: int, d: int) -> dict:
    """Inputs of one shape, chosen so that the listed mis-statements show: every row of x1 carries its own common offset (a wrong
    divisor or an uncentred variance moves mean / rstd), gamma is not constant and beta not small, dout has a nonzero row mean
    (c1 matters), no dout / y element is zero.  The saved tensors of the backward forms are the fp64 forward rounded as the forward
    entry points store them (rows to the IO dtype, statistics to fp32)."""
    off = 2.0 * _rn(10, d, M, 1)
    I = dict(y=_nonzero(_rn(0, d, M, d)).to(dtype), x1=(_rn(1, d, M, d) + off).to(dtype),
             dout=_nonzero(_rn(2, d, M, d) + 0.5).to(dtype), dres=_rn(3, d, M, d).to(dtype))
    g = 1.0 + 0.3 * _rn(4, d, d)
    I["gamma"] = torch.where(g.abs() < 0.25, torch.full_like(g, 0.25), g)
    I["beta"] = 0.5 * _rn(5, d, d)
    g2 = 1.0 + 0.3 * _rn(6, d, d)
    I["gamma2"] = torch.where(g2.abs() < 0.25, torch.full_like(g2, 0.25), g2)
    return derive_saved(I, dtype)


def derive_saved(I: dict, dtype) -> dict:
    """The saved tensors the backward forms read, from the fp64 forward of the same inputs."""
    f = sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], I["beta"], EPS, P0, SEED, 1)
    I["h"], I["out"] = f.h.float().to(dtype), f.out.float().to(dtype)
    I["mean"], I["rstd"] = f.mean.float(), f.rstd.float()
    I["xhat"] = ((f.h - f.mean[:, None]) * f.rstd[:, None]).float().to(dtype)
    s = sublayer_tail_rms_fwd(I["y"], I["x1"], I["gamma2"], EPS, P0, SEED)
    I["sum"], I["rstd2"] = s.sum.float().to(dtype), s.rstd.float()
    return I


OPS = ["fwd_ln", "fwd_ln_p0", "fwd_res", "post", "rms_fwd", "rms2_fwd", "rms2_fwd_p0", "bwd_ln", "bwd_ln_p0", "bwd_res", "bwd_res_p0", "bwd_out",
       "bwd_xhat", "rms_bwd", "rms_bwd_plain", "rms_tail_bwd", "rms_tail_bwd_plain", "colsum"]


def _bwd_items(r, M, nb, dy, part):
    o = {"dx1": (r.dx1, r.e_dx1, "row")}
    if dy:
        o["dy"] = (r.dy, r.e_dy, "row")
    if part:
        v = torch.stack([block_partials(r.dg_rows, nb), block_partials(r.db_rows, nb)], 1)
        e = torch.stack([partial_bound(r.dg_rows.abs(), r.e_dg_rows, M, nb), partial_bound(r.db_rows.abs(), r.e_db_rows, M, nb)], 1)
        o["partials"] = (v, e, "f32")
    return o


def spec_op(op: str, I: dict, ct=torch.float64, ctr=None, mut=(), keep=None, p=None):
    """name -> (value, bound before the output rounding, "row" (IO-dtype rows) / "f32" / "mask") for every output of one operation
    of the suite; tests/test_gpu_tail_edges.py makes the matching call (its _CALLS), tests/test_tail_spec.py evaluates this with
    ct = fp32.  ``p`` replaces the operation's dropout rate (only for operations that have one)."""
    M, d = I["x1"].shape
    nb = tail_blocks(M)
    kw = dict(ct=ct, mut=mut)
    dk = dict(ctr=ctr, keep=keep, **kw)
    pp = lambda default: default if p is None else p
    if op == "fwd_ln":
        r = sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], I["beta"], EPS, pp(P0), SEED, 1, **dk)
        return {"out": (r.out, r.e_out, "row"), "h": (r.h, r.e_h, "row"), "mean": (r.mean, r.e_mean, "f32"),
                "rstd": (r.rstd, r.e_rstd, "f32"), "keep": (r.keep, None, "mask")}
    if op == "fwd_ln_p0":       # beta NULL, h_save NULL, no dropout
        r = sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], None, EPS, 0.0, SEED, 1, **kw)
        return {"out": (r.out, r.e_out, "row"), "mean": (r.mean, r.e_mean, "f32"), "rstd": (r.rstd, r.e_rstd, "f32")}
    if op == "fwd_res":
        r = sublayer_tail_fwd(I["y"], I["x1"], None, None, EPS, pp(0.5), SEED + 1, 0, **dk)
        return {"out": (r.out, r.e_out, "row"), "keep": (r.keep, None, "mask")}
    if op == "post":
        r = norm_residual_fwd(I["y"], I["x1"], I["gamma"], I["beta"], EPS, **kw)
        return {"out": (r.out, r.e_out, "row"), "mean": (r.mean, r.e_mean, "f32"), "rstd": (r.rstd, r.e_rstd, "f32")}
    if op == "rms_fwd":
        r = rmsnorm_fwd(I["x1"], I["gamma"], EPS, **kw)
        return {"out": (r.out, r.e_out, "row"), "rstd": (r.rstd, r.e_rstd, "f32")}
    if op in ("rms2_fwd", "rms2_fwd_p0"):   # (without dropout the sum is exact in fp32: no element near a rounding boundary, e_hr = 0)
        r = sublayer_tail_rms_fwd(I["y"], I["x1"], I["gamma2"], EPS, pp(P0) if op == "rms2_fwd" else 0.0, SEED, **dk)
        return {"sum": (r.sum, r.e_sum, "row"), "normed": (r.normed, r.e_normed, "row"), "rstd": (r.rstd, r.e_rstd, "f32")}
    if op == "bwd_ln":
        r = sublayer_tail_bwd(I["dout"], I["h"], I["mean"], I["rstd"], I["gamma"], pp(P0), SEED, 1, **dk)
        return _bwd_items(r, M, nb, True, True)
    if op == "bwd_ln_p0":       # dy NULL, dgb_partials NULL
        r = sublayer_tail_bwd(I["dout"], I["h"], I["mean"], I["rstd"], I["gamma"], 0.0, SEED, 1, **kw)
        return _bwd_items(r, M, nb, False, False)
    if op == "bwd_res":         # the aliased residual form: dx1 NULL, only dy is written
        r = sublayer_tail_bwd(I["dout"], None, None, None, None, pp(0.5), SEED + 1, 0, **dk)
        return {"dy": (r.dy, r.e_dy, "row")}
    if op == "bwd_res_p0":
        r = sublayer_tail_bwd(I["dout"], None, None, None, None, 0.0, SEED, 0, **kw)
        return {"dx1": (r.dx1, r.e_dx1, "row")}
    if op == "bwd_out":
        r = sublayer_tail_bwd_out(I["dout"], I["out"], I["rstd"], I["gamma"], I["beta"], pp(P0), SEED, **dk)
        return _bwd_items(r, M, nb, True, True)
    if op == "bwd_xhat":
        return _bwd_items(layernorm_bwd_xhat(I["dout"], I["xhat"], I["rstd"], I["gamma"], **kw), M, nb, False, True)
    if op == "rms_bwd":
        return _bwd_items(rmsnorm_bwd(I["dout"], I["sum"], I["rstd2"], I["gamma2"], I["dres"], **kw), M, nb, False, True)
    if op == "rms_bwd_plain":
        return _bwd_items(rmsnorm_bwd(I["dout"], I["sum"], I["rstd2"], I["gamma2"], None, **kw), M, nb, False, False)
    if op == "rms_tail_bwd":
        r = rmsnorm_tail_bwd(I["dout"], I["sum"], I["rstd2"], I["gamma2"], I["dres"], pp(P0), SEED, **dk)
        return _bwd_items(r, M, nb, True, True)
    if op == "rms_tail_bwd_plain":
        r = rmsnorm_tail_bwd(I["dout"], I["sum"], I["rstd2"], I["gamma2"], None, 0.0, SEED, **kw)
        return _bwd_items(r, M, nb, False, False)
    if op == "colsum":
        r = colsum(I["dout"], nb, ct=ct)
        return {"out": (r.out, r.e_out, "f32")}
    raise KeyError(op)


def check(name, got, ref, e, kind, dtype, log):
    """Every element within its own bound (a NaN -- an unwritten element -- fails); the worst err / bound goes to ``log``.
    -> number of elements over their bound."""
    got = got.detach().double().cpu()
    ref = ref.double()
    bound = hold_bound(e.double(), ref, dtype if kind == "row" else torch.float32)
    err = (got - ref).abs()
    ok = err <= bound
    worst = float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    log.append(f"{name} {worst:.3f}")
    return int((~ok).sum())
