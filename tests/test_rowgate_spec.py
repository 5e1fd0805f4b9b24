"""CPU: the fp64 statements of the row operations (tests/rowgate_spec.py), chained as vlpet_amd/gates.py chains the kernels
(dot -> sigmoid (-> sequence mean) -> affine, and the backward likewise), are oracle.vlpet_oracle.encoder_adapter_gate and its
autograd.  tests/test_gpu_rowgate.py holds the kernels to these statements through the C ABI; this test ties the statements to the
oracle that the module tests (tests/test_gpu_gates.py) use, so the two levels check one definition.

The oracle builds h = x2 + up(gelu_new(down(x2))) itself; with a zero up projection h is x2 and dL/dx2 is dL/dh."""
import pytest
import torch

import rowgate_spec as RS
from oracle import vlpet_oracle as O

RTOL = 1e-12


def _close(a, ref):
    """max |a - ref| <= RTOL * max |ref|"""
    return float((a - ref).abs().max()) <= RTOL * float(ref.abs().max())


def _oracle(x1, h, gate, mode, add, gs, dy):
    d = h.shape[-1]
    x1r, hr = x1.clone().requires_grad_(True), h.clone().requires_grad_(True)
    gate = {k: v.clone().requires_grad_(True) for k, v in gate.items()}
    g = torch.Generator().manual_seed(5)
    dw, db = [torch.randn(4, d, generator=g, dtype=torch.float64)], [torch.randn(4, generator=g, dtype=torch.float64)]
    uw, ub = torch.zeros(d, 4, dtype=torch.float64), torch.zeros(d, dtype=torch.float64)      # delta = 0: h = x2
    y = O.encoder_adapter_gate(x1r, hr, dw, db, uw, ub, gate, mode, add, 1.0, 1.0, gs)
    y.backward(dy)
    return y.detach(), x1r.grad, hr.grad, {k: v.grad for k, v in gate.items()}


@pytest.mark.parametrize("add,gs", [(False, 1.0), (True, 1.0), (False, 0.3), (True, 0.3)])
@pytest.mark.parametrize("mode", [O.GATE_SMALL, O.GATE_MIDDLE_X, O.GATE_MIDDLE_Y])
def test_the_chained_statements_are_the_oracle(mode, add, gs):
    g = torch.Generator().manual_seed(17 + mode)
    B, S, d = 3, 5, 24
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x1, h, dy = r(B, S, d), r(B, S, d), r(B, S, d)
    if mode == O.GATE_MIDDLE_Y:
        z = r(d) * 0.5
        y, _, dh, gg = _oracle(x1, h, dict(z=z), mode, add, gs, dy)
        c = RS.vec_gate_chain(h, z, dy, add, gs)
        assert _close(c.y, y) and _close(c.dh, dh) and _close(c.dz, gg["z"])
        return
    small = mode == O.GATE_SMALL
    w, b = r(1, 2 * d if small else d) * 0.2, r(1) * 0.2
    y, dx1, dh, gg = _oracle(x1, h, dict(w=w, b=b), mode, add, gs, dy)
    c = RS.row_gate_chain(x1, h, w, b, dy, small, add, gs)
    assert _close(c.y, y) and _close(c.dx1, dx1) and _close(c.dh, dh)
    assert _close(c.dw, gg["w"]) and _close(c.db, gg["b"])


def test_row_dot_modes_and_the_term_sums():
    """The three argument modes of ROW_DOT, and every ``*_abs`` is the sum of |product| of the same operation."""
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a, c, wa, wc = r(6, 16), r(6, 16), r(16), r(16)
    assert _close(RS.row_dot(a, c, wa, wc).s, a @ wa + c @ wc)
    assert _close(RS.row_dot(a, None, wa, None).s, a @ wa)
    assert _close(RS.row_dot(a, c).s, (a * c).sum(1))
    assert _close(RS.row_dot(a, c, wa, wc).s_abs, a.abs() @ wa.abs() + c.abs() @ wc.abs())
    assert _close(RS.row_dot(a, c).s_abs, (a * c).abs().sum(1))
    ra, rb = r(6), r(6)
    assert _close(RS.row_affine(a, ra).o1, a * ra[:, None])
    assert _close(RS.row_affine(a, ra, rb).o1_abs, (a * ra[:, None]).abs() + rb.abs()[:, None])
    assert _close(RS.vec_fwd(a, wa).o1, a * wa)
    assert _close(RS.vec_fwd(a, wa, wc).o1_abs, (a * wa).abs() + wc.abs())
    q = RS.row_bwd(a, c, a + c, ra, rb, wa, wc)
    assert _close(q.p0, rb @ c) and _close(q.p1, rb @ (a + c)) and _close(q.p0_abs, rb.abs() @ c.abs())
    v = RS.vec_bwd(a, c, wa)
    assert _close(v.p0, (a * c).sum(0)) and _close(v.p1, a.sum(0)) and _close(v.p1_abs, a.abs().sum(0))
    # inputs of any float dtype are taken at their own (already rounded) values
    ab = a.to(torch.bfloat16)
    assert torch.equal(RS.row_dot(ab, None, wa.float(), None).s, (ab.double() * wa.float().double()).sum(1))
