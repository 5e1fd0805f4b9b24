"""tests/attn_spec.py on its own (CPU): the hand-written backward of the reference against autograd, and the restatement of the
kernels' rounding against the reference under the project's tensor-wide bound, on the cases the GPU suite runs."""
import pytest
import torch

import attn_spec as S


def _autograd(q, k, v, do, key_mask, causal, keep, p, bias, scale, heads):
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    out = S.eager(qd, kd, vd, key_mask, causal, keep, p, None if bias is None else bias.double(), scale, heads)
    out.backward(do.double())
    return [S.heads_first(t, heads) for t in (out.detach(), qd.grad, kd.grad, vd.grad)]


# a plain shape; a causal one whose first queries see nothing; dead rows (a dead item, a bias row of -inf), -inf bias columns and dropout
@pytest.mark.parametrize("name", ["3x5x63x65-random-p0.1", "3x3x56x20-causal-p0.1", "3x1x65x33-random-p0.1-bias_row5", "dead+bias+dropout"])
def test_hand_written_backward_equals_autograd_in_fp64(name):
    if name in S.BY_NAME:
        case = S.BY_NAME[name]
    else:
        case = S.make_case(3, 3, 40, 33, True, "dead1", 0.1, bias="col7")
    q, k, v, do, km, bias, scale = S.inputs(case)
    if name not in S.BY_NAME:
        bias[:, 37, :] = float("-inf")                         # a dead row in the middle of live ones, past the causal dead rows
    keep = S.host_keep(case)
    got = S.chain(q, k, v, do, km, case.causal, keep, case.p, bias, scale, case.H, torch.float64, False)
    ref = _autograd(q, k, v, do, km, case.causal, keep, case.p, bias, scale, case.H)
    dead = S.dead_rows(q, k, km, case.causal, bias, case.H)
    if name != "3x5x63x65-random-p0.1":
        assert bool(dead.any()) and not bool(dead.all())
    for n, a, r in zip(S.NAMES, got, ref):
        assert a.dtype == torch.float64 and torch.isfinite(a).all() and float(r.abs().max()) > 0.1
        assert float((a - r).abs().max()) <= 1e-12, n
    assert float(got[0][dead].abs().max() if dead.any() else 0.0) == 0.0
    assert float(got[1][dead].abs().max() if dead.any() else 0.0) == 0.0


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_restated_rounding_meets_the_tensor_wide_bound(case):
    q, k, v, do, km, bias, scale = S.inputs(case)
    keep = S.host_keep(case)
    ref = S.chain(q, k, v, do, km, case.causal, keep, case.p, bias, scale, case.H, torch.float64, False)
    got = S.chain(q, k, v, do, km, case.causal, keep, case.p, bias, scale, case.H, torch.float32, True)
    errs = {n: S.wide_error(n, a, r) for n, a, r in zip(S.NAMES, got, ref)}
    print(case.name, "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, a, r in zip(S.NAMES, got, ref):
        assert a.dtype == torch.float32 and torch.isfinite(a).all()
        if n in case.zero:
            assert float(r.abs().max()) <= 1e-12               # zero in the reference (to fp64 rounding): only delta's rounding is left
            continue
        assert errs[n] <= S.TOL, (n, errs)
        # and the restatement sits inside its own per-tile budget trivially; the tiles' shapes are the kernels'
        e, m = S.tile_errors(a, r)
        assert e.shape == m.shape == (case.B, case.H, (r.shape[2] + 31) // 32)


def test_tile_errors_sees_a_small_tile_behind_a_large_one():
    r = torch.zeros(1, 1, 70, 64, dtype=torch.float64)
    r[0, 0, :32] = 100.0
    r[0, 0, 64:] = 0.01
    a = r.clone()
    a[0, 0, 69, 3] += 0.005                                    # half of the ragged last tile's magnitude, 5e-5 of the tensor's
    assert S.wide_error("dq", a, r) < 1e-4
    e, m = S.tile_errors(a, r)
    assert e.shape == (1, 1, 3) and torch.allclose(m[0, 0], torch.tensor([100.0, 0.0, 0.01], dtype=torch.float64))
    assert float(e[0, 0, 2]) == pytest.approx(0.005) and float(e[0, 0, :2].max()) == 0.0
    assert bool((e > S.tile_budget(torch.zeros_like(e), m)).any())
