"""fp64 statements of the five row operations of csrc/rowgate.hip, exactly as its header comment gives them:

    ROW_DOT    : s[row] = sum_j a[row,j]*va[j] + c[row,j]*vc[j]      (va == null: s[row] = sum_j a[row,j]*c[row,j])
    ROW_AFFINE : o1[row,:] = a[row,:]*ra[row] + rb[row]
    ROW_BWD    : o1 = ra[row]*a + rb[row]*vc  (dh);  o2 = rb[row]*va  (dx1);  partials: sum_rows rb*c (dwa), rb*e (dwc)
                 (a = dy, c = x1, e = h)
    VEC_FWD    : o1[row,:] = a[row,:]*va[:] + vc[:]
    VEC_BWD    : o1 = a*va (dh, a = dy);  partials: sum_rows a*c (c = h), sum_rows a

Every function takes tensors of any float dtype, computes in fp64 and returns, beside each value, the sum of the absolute values
of the products that form it (``*_abs``): the quantity a floating-point error bound of the kernel is stated in
(tests/test_gpu_rowgate.py).  tests/test_rowgate_spec.py chains these as vlpet_amd/gates.py chains the kernels and holds the result
to oracle.vlpet_oracle.encoder_adapter_gate, so the ABI-level statements and the module-level oracle are one definition."""
from __future__ import annotations

from types import SimpleNamespace

import torch


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to(torch.float64)


def row_dot(a, c=None, wa=None, wc=None):
    """The three modes of vlpet_row_dot: weighted pair (a, c, wa, wc), weighted single (c None), plain pair product (wa None).
    -> s [M], s_abs [M]"""
    a, c, wa, wc = _d(a), _d(c), _d(wa), _d(wc)
    if wa is None:
        t = a * c
        return SimpleNamespace(s=t.sum(1), s_abs=t.abs().sum(1))
    t = a * wa
    s, s_abs = t.sum(1), t.abs().sum(1)
    if c is not None:
        t = c * wc
        s, s_abs = s + t.sum(1), s_abs + t.abs().sum(1)
    return SimpleNamespace(s=s, s_abs=s_abs)


def row_affine(a, ra, rb=None):
    """o1[row, :] = a[row, :] * ra[row] + rb[row]  (rb None: no additive term)"""
    a, ra, rb = _d(a), _d(ra), _d(rb)
    o = a * ra[:, None]
    o_abs = o.abs()
    if rb is not None:
        o, o_abs = o + rb[:, None], o_abs + rb.abs()[:, None]
    return SimpleNamespace(o1=o, o1_abs=o_abs)


def row_bwd(dy, x1, h, ra, rb, va, vc):
    """dh = ra[row]*dy + rb[row]*vc;  dx1 = rb[row]*va;  p0 = sum_rows rb*x1;  p1 = sum_rows rb*h"""
    dy, x1, h, ra, rb, va, vc = _d(dy), _d(x1), _d(h), _d(ra), _d(rb), _d(va), _d(vc)
    t0, t1 = ra[:, None] * dy, rb[:, None] * vc[None, :]
    dx1 = rb[:, None] * va[None, :]
    q0, q1 = rb[:, None] * x1, rb[:, None] * h
    return SimpleNamespace(dh=t0 + t1, dh_abs=t0.abs() + t1.abs(), dx1=dx1, dx1_abs=dx1.abs(),
                           p0=q0.sum(0), p0_abs=q0.abs().sum(0), p1=q1.sum(0), p1_abs=q1.abs().sum(0))


def vec_fwd(a, va, vc=None):
    """o1[row, :] = a[row, :] * va[:] + vc[:]  (vc None: no additive term)"""
    a, va, vc = _d(a), _d(va), _d(vc)
    o = a * va[None, :]
    o_abs = o.abs()
    if vc is not None:
        o, o_abs = o + vc[None, :], o_abs + vc.abs()[None, :]
    return SimpleNamespace(o1=o, o1_abs=o_abs)


def vec_bwd(dy, h, va):
    """dh = dy*va;  p0 = sum_rows dy*h;  p1 = sum_rows dy"""
    dy, h, va = _d(dy), _d(h), _d(va)
    dh = dy * va[None, :]
    q = dy * h
    return SimpleNamespace(dh=dh, dh_abs=dh.abs(), p0=q.sum(0), p0_abs=q.abs().sum(0), p1=dy.sum(0), p1_abs=dy.abs().sum(0))


# ------------------------------------------------------------------------------------------------ the chains of vlpet_amd/gates.py
def row_gate_chain(x1, h, w, b, dy, small, gating_add, gs):
    """_RowGateFn forward + backward stated with the operations above (x1, h, dy [B, S, d]; w [1, 2d] (small) or [1, d]; b [1]).
    -> y, dx1, dh [B, S, d], dw like w, db [1]"""
    B, S, d = h.shape
    x1f, hf, dyf = (_d(t).reshape(-1, d) for t in (x1, h, dy))
    w64, b64 = _d(w).reshape(-1), _d(b).reshape(())
    wa = w64[:d]
    wc = w64[d:] if small else wa
    s = row_dot(x1f, hf, wa, wc).s
    g_row = torch.sigmoid(s + b64)
    g_exp = g_row.view(-1, S).mean(1).repeat_interleave(S) if small else g_row
    if gating_add:
        alpha, gamma = torch.full_like(g_exp, gs), gs * g_exp
    else:
        alpha, gamma = gs * g_exp, None
    y = row_affine(hf, alpha, gamma).o1
    if gating_add:
        t = row_dot(dyf, None, torch.ones(d, dtype=torch.float64), None).s
    else:
        t = row_dot(dyf, hf, None, None).s
    dg = gs * t
    if small:
        dg = (dg.view(-1, S).sum(1) / S).repeat_interleave(S)
    beta = dg * g_row * (1.0 - g_row)
    r = row_bwd(dyf, x1f, hf, alpha, beta, wa, wc)
    dw = torch.cat([r.p0, r.p1]) if small else r.p0 + r.p1
    return SimpleNamespace(y=y.view(B, S, d), dx1=r.dx1.view(B, S, d), dh=r.dh.view(B, S, d), dw=dw.view(w.shape),
                           db=beta.sum().view(1))


def vec_gate_chain(h, z, dy, gating_add, gs):
    """_VecGateFn forward + backward stated with the operations above.  -> y, dh [B, S, d], dz [d]"""
    B, S, d = h.shape
    hf, dyf, z64 = _d(h).reshape(-1, d), _d(dy).reshape(-1, d), _d(z)
    if gating_add:
        v, u = torch.full_like(z64, gs), gs * (1.0 + z64)
    else:
        v, u = gs * (1.0 + z64), None
    y = vec_fwd(hf, v, u).o1
    r = vec_bwd(dyf, hf, v)
    dz = gs * (r.p1 if gating_add else r.p0)
    return SimpleNamespace(y=y.view(B, S, d), dh=r.dh.view(B, S, d), dz=dz)
