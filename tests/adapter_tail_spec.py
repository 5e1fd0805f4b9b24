"""Host statement of vlpet_adapter_tail_fwd (csrc/adapter_tail.hip):

    out = N(res + h + s * (up(gelu_new(down(h) + b_d)) + b_u)),      N = LayerNorm(gamma, beta, eps) | identity

twice: ``reference`` in fp64 from the formula, and ``kernel_model``, which walks the kernel's documented steps -- the down product's K
split over eight waves and summed in wave order, the operand roundings (bf16 IO: h, both weights and z as bf16; fp32 IO: each as
a bf16 hi + lo pair with the lo * lo product dropped), fp32 everywhere else, two-pass LayerNorm statistics, one rounding of the result.
With ``exact=True`` every rounding is the identity and the walk must agree with the formula to fp64 precision; with the roundings on it
bounds what the kernel may differ from ``reference`` by.  Pure torch, CPU."""
import math

import torch

WAVES = 8


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def reference(h, res, wd, bd, wu, bu, gamma=None, beta=None, eps=1e-5, scale=1.0, norm=True):
    """fp64, straight from the formula"""
    h, res, wd, bd, wu, bu = (t.double() for t in (h, res, wd, bd, wu, bu))
    v = res + h + scale * (gelu_new(h @ wd.t() + bd) @ wu.t() + bu)
    if not norm:
        return v
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    out = (v - mean) / torch.sqrt(var + eps) * gamma.double()
    return out if beta is None else out + beta.double()


def _bf16(x):
    return x.float().bfloat16().double()


def _planes(x, io_dtype, exact):
    """the MFMA operand planes of ``x``: [x] (exact), [bf16(x)] (bf16 IO) or [hi, lo] (fp32 IO)"""
    if exact:
        return [x.double()]
    hi = _bf16(x)
    if io_dtype == torch.bfloat16:
        return [hi]
    return [hi, _bf16(x.double() - hi)]


def _product(a, b):
    """sum of the plane products the kernel issues: hi*hi (+ hi*lo + lo*hi with two planes)"""
    out = a[0] @ b[0]
    if len(a) == 2:
        out = out + a[1] @ b[0] + a[0] @ b[1]
    return out


def kernel_model(h, res, wd, bd, wu, bu, gamma=None, beta=None, eps=1e-5, scale=1.0, norm=True, io_dtype=torch.bfloat16, exact=False):
    """the kernel's steps; accumulations are carried in fp64 (the kernel's fp32 sums are not restated, their error is part of the
    tolerance), roundings of operands and of the result are"""
    acc = (lambda t: t.double()) if exact else (lambda t: t.float().double())          # values the kernel holds in fp32
    d = h.shape[-1]
    k_steps = d // 32
    per_wave = -(-k_steps // WAVES)
    hp, wdp = _planes(h, io_dtype, exact), _planes(wd, io_dtype, exact)
    parts = []
    for w in range(WAVES):
        lo, hi = 32 * per_wave * w, min(d, 32 * per_wave * (w + 1))
        if lo >= d:
            parts.append(torch.zeros(h.shape[0], wd.shape[0], dtype=torch.float64))
            continue
        parts.append(acc(_product([p[:, lo:hi] for p in hp], [p[:, lo:hi].t() for p in wdp])))
    pre = parts[0]
    for part in parts[1:]:
        pre = acc(pre + part)
    z = acc(gelu_new(acc(pre + bd.double())))
    u = acc(_product(_planes(z, io_dtype, exact), [p.t() for p in _planes(wu, io_dtype, exact)]))
    x = acc(scale * acc(u + bu.double()))
    v = acc(acc(res.double() + h.double()) + x)
    if norm:
        mean = acc(v.mean(-1, keepdim=True))
        var = acc(((v - mean) ** 2).mean(-1, keepdim=True))
        v = acc((v - mean) / torch.sqrt(var + eps) * gamma.double())
        if beta is not None:
            v = acc(v + beta.double())
    if exact:
        return v
    return _bf16(v) if io_dtype == torch.bfloat16 else v.float().double()


def make_case(M, d, r, seed, dtype=torch.float32, big_row=None, const_row=None):
    """inputs at the sizes the models see: h, res ~ N(0, 1) (``big_row``: that row of h times 300), adapter weights ~ N(0, 0.05)
    (the fixtures' scale) rounded to ``dtype``, LayerNorm parameters around (1, 0).  ``const_row``: a row whose pre-norm sum is the
    same in every column, whatever the adapter adds -- the caller zeroes the up projection for it."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    h, res = rnd(M, d), rnd(M, d)
    if big_row is not None and big_row < M:
        h[big_row] *= 300.0
    t = dict(h=h, res=res, wd=rnd(r, d, std=0.05), bd=rnd(r, std=0.05), wu=rnd(d, r, std=0.05), bu=rnd(d, std=0.05),
             gamma=1.0 + rnd(d, std=0.1), beta=rnd(d, std=0.1))
    return {k: v.to(dtype).float() if k in ("h", "res") else v for k, v in t.items()}
