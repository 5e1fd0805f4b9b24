"""vlpet_phm_expand_pair_fwd / _bwd (csrc/phm.hip) on the GPU against tests/phm_spec.py under its derived error budget, fp32 and bf16
parameters: the full-size and tiny adapter shapes at every division, shapes with partial 32 x 32 tiles and k or p of 1 or 2, zero and
one-hot rules, run-to-run bits of the backward, guard elements behind every output and around the workspace, a rule shared by both
layers, and autograd through functional.phm_expand_pair + K2 against the eager composition."""
import functools

import numpy as np
import pytest
import torch

import phm_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (d, r, n): both adapter geometries at every division the scripts and defaults use; (12, 6, 3), (40, 10, 5), (7, 7, 7): partial tiles,
# k or p of 1 or 2; n = 1: a scaled transpose
SHAPES = [(64, 8, 2), (64, 8, 4), (768, 96, 2), (768, 96, 4), (768, 96, 8), (12, 6, 3), (40, 10, 5), (7, 7, 7), (64, 8, 1)]
DTYPES = [torch.float32, torch.bfloat16]
PAD = 64            # guard elements on either side of every output (a multiple of 16 bytes in both dtypes)
GUARD = 7.25        # exactly representable in bf16


@functools.lru_cache(maxsize=None)
def inputs(d, r, n, dtype, rule="randn"):
    """parameters (rounded to ``dtype``, so that the fp64 spec sees the values the kernel reads) and upstream gradients, on the CPU"""
    g = torch.Generator().manual_seed(1000 * d + 10 * r + n)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)
    p = dict(rule_d=mk(n, n, n), W_d=mk(n, d // n, r // n), rule_u=mk(n, n, n), W_u=mk(n, r // n, d // n))
    if rule == "zero":
        p["rule_d"], p["rule_u"] = torch.zeros_like(p["rule_d"]), torch.zeros_like(p["rule_u"])
    elif rule == "one_hot":
        for k, idx in (("rule_d", (n - 1, 0, n - 1)), ("rule_u", (0, n - 1, 0))):
            p[k] = torch.zeros_like(p[k])
            p[k][idx] = 2.0
    p["g_d"], p["g_u"] = torch.randn(r, d, generator=g), torch.randn(d, r, generator=g)
    return p


def guarded(numel, dtype):
    """(whole buffer filled with GUARD, the view of ``numel`` elements in its middle)"""
    buf = torch.full((numel + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + numel]


def guards_intact(buf, numel):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + numel:] == GUARD).all())


def run_fwd(p, d, r, n, dtype):
    from vlpet_amd import _lib
    lib = _lib.load()
    dev = {k: v.to(DEV).contiguous() for k, v in p.items()}
    (b0, wt_d), (b1, wt_u) = guarded(r * d, dtype), guarded(d * r, dtype)
    pdt = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    rc = lib.vlpet_phm_expand_pair_fwd(dev["rule_d"].data_ptr(), dev["W_d"].data_ptr(), dev["rule_u"].data_ptr(), dev["W_u"].data_ptr(),
                                       wt_d.data_ptr(), wt_u.data_ptr(), d, r, n, pdt, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(b0, r * d) and guards_intact(b1, d * r)
    return wt_d.view(r, d).float().cpu().numpy().astype(np.float64), wt_u.view(d, r).float().cpu().numpy().astype(np.float64)


def run_bwd(p, d, r, n, dtype):
    """-> (drule_d, dW_d, drule_u, dW_u) as CPU fp32 tensors; guards behind every output and around the workspace checked"""
    from vlpet_amd import _lib
    lib = _lib.load()
    dev = {k: v.to(DEV).contiguous() for k, v in p.items()}
    n3, nw = n * n * n, d * r // n
    outs = [guarded(n3, torch.float32), guarded(nw, torch.float32), guarded(n3, torch.float32), guarded(nw, torch.float32)]
    nws = lib.vlpet_phm_workspace_bytes(d, r, n)
    assert nws > 0 and nws % 4 == 0
    wbuf, ws = guarded(nws // 4, torch.float32)
    pdt = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    rc = lib.vlpet_phm_expand_pair_bwd(dev["g_d"].data_ptr(), dev["g_u"].data_ptr(), dev["rule_d"].data_ptr(), dev["W_d"].data_ptr(),
                                       dev["rule_u"].data_ptr(), dev["W_u"].data_ptr(), outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                                       outs[2][1].data_ptr(), outs[3][1].data_ptr(), ws.data_ptr(), nws, d, r, n, pdt,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for (buf, view) in outs:
        assert guards_intact(buf, view.numel())
    assert guards_intact(wbuf, nws // 4)
    return [v.cpu().clone() for _, v in outs]


def f64(t):
    return t.float().numpy().astype(np.float64)


def within(got, exact, budget, what):
    err = np.abs(np.asarray(got, np.float64).reshape(exact.shape) - exact)
    worst = float((err - budget).max())
    print(f"{what}: worst error {float(err.max()):.3e}, worst error / budget {float((err / np.maximum(budget, 1e-300)).max()):.3f}")
    assert worst <= 0, (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,r,n", SHAPES)
def test_forward_within_the_budget(d, r, n, dtype):
    p = inputs(d, r, n, dtype)
    wt_d, wt_u = run_fwd(p, d, r, n, dtype)
    bf = dtype == torch.bfloat16
    for got, rule, W, tag in ((wt_d, p["rule_d"], p["W_d"], "wt_d"), (wt_u, p["rule_u"], p["W_u"], "wt_u")):
        ht, mag = S.weight(f64(rule), f64(W))
        assert got.shape == ht.shape
        within(got, ht, S.budget(mag, n, ht, bf), f"{tag} {(d, r, n)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,r,n", SHAPES)
def test_backward_within_the_budget_and_bitwise_repeatable(d, r, n, dtype):
    p = inputs(d, r, n, dtype)
    first = run_bwd(p, d, r, n, dtype)
    again = run_bwd(p, d, r, n, dtype)
    for a, b in zip(first, again):
        assert torch.equal(a, b)                                   # no atomics, a fixed order: the same bits
    for (drule, dW), rule, W, G, (k, pp), tag in (((first[0], first[1]), p["rule_d"], p["W_d"], p["g_d"], (d // n, r // n), "down"),
                                                  ((first[2], first[3]), p["rule_u"], p["W_u"], p["g_u"], (r // n, d // n), "up")):
        dA, dWx, mA, mW = S.weight_grads(f64(rule), f64(W), f64(G))
        within(f64(drule), dA, S.budget(mA, k * pp), f"d rule {tag} {(d, r, n)}")
        within(f64(dW), dWx, S.budget(mW, n * n), f"dW {tag} {(d, r, n)}")


def test_n1_is_a_scaled_transpose():
    d, r = 64, 8
    p = inputs(d, r, 1, torch.float32)
    wt_d, wt_u = run_fwd(p, d, r, 1, torch.float32)
    assert np.array_equal(wt_d, f64(p["rule_d"].reshape(()) * p["W_d"][0].t()))          # one product: one rounding, the same in torch
    assert np.array_equal(wt_u, f64(p["rule_u"].reshape(()) * p["W_u"][0].t()))


@pytest.mark.parametrize("d,r,n", [(64, 8, 4), (12, 6, 3), (768, 96, 2)])
def test_zero_rule_and_single_rule_entry(d, r, n):
    p = inputs(d, r, n, torch.float32, "zero")
    wt_d, wt_u = run_fwd(p, d, r, n, torch.float32)
    assert not wt_d.any() and not wt_u.any()
    p = inputs(d, r, n, torch.float32, "one_hot")
    wt_d, wt_u = run_fwd(p, d, r, n, torch.float32)
    # rule_d[i = n - 1, a = 0, c = n - 1] = 2: H^T rows (c p ..), columns (a k ..) hold 2 W[i]^T, nothing anywhere else
    for wt, (i, a, c), W, k, pp in ((wt_d, (n - 1, 0, n - 1), p["W_d"], d // n, r // n), (wt_u, (0, n - 1, 0), p["W_u"], r // n, d // n)):
        assert int(np.count_nonzero(wt)) == k * pp
        block = wt[c * pp:(c + 1) * pp, a * k:(a + 1) * k]
        assert np.array_equal(block, f64(2.0 * W[i].t()))


def test_shared_rule_gets_the_sum_of_both_gradients():
    import vlpet_amd.functional as VF
    d, r, n = 64, 8, 4
    p = inputs(d, r, n, torch.float32)
    sep = run_bwd(dict(p, rule_u=p["rule_d"]), d, r, n, torch.float32)
    rule = p["rule_d"].to(DEV).requires_grad_(True)
    W_d, W_u = p["W_d"].to(DEV).requires_grad_(True), p["W_u"].to(DEV).requires_grad_(True)
    n0 = VF.PHM_CALLS
    wt_d, wt_u = VF.phm_expand_pair(rule, W_d, rule, W_u, n)
    assert VF.PHM_CALLS == n0 + 1
    torch.autograd.backward([wt_d, wt_u], [p["g_d"].to(DEV), p["g_u"].to(DEV)])
    assert torch.equal(rule.grad.cpu().reshape(-1), sep[0] + sep[2])
    assert torch.equal(W_d.grad.cpu().reshape(-1), sep[1]) and torch.equal(W_u.grad.cpu().reshape(-1), sep[3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,r,n", [(64, 8, 2), (768, 96, 4)])
def test_autograd_through_expansion_and_k2_matches_the_eager_composition(d, r, n, dtype):
    """M = 48 rows; tolerances: K2's in tests/test_gpu_kernels.py (1e-3 fp32 IO, 1e-2 bf16 IO; gpu_cases.rel_err)"""
    import math
    import vlpet_amd.functional as VF
    from vlpet_amd import eager
    from vlpet_amd.adapters.adapter_utils import Activations
    from gpu_cases import rel_err
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    M = 48
    g = torch.Generator().manual_seed(5)
    x, y, dy = (torch.randn(M, d, generator=g).to(dtype) for _ in range(3))
    k, pp = d // n, r // n
    P = dict(rule_d=torch.randn(n, n, n, generator=g), W_d=torch.randn(n, k, pp, generator=g) / math.sqrt(d * n),
             rule_u=torch.randn(n, n, n, generator=g), W_u=torch.randn(n, pp, k, generator=g) / math.sqrt(r * n),
             b_d=torch.randn(r, generator=g) * 0.1, b_u=torch.randn(d, generator=g) * 0.1)
    ref = {k_: v.double().requires_grad_(True) for k_, v in P.items()}
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    out_ref = yr + eager.phm_adapter(xr, ref["rule_d"], ref["W_d"], ref["b_d"], ref["rule_u"], ref["W_u"], ref["b_u"], Activations("gelu_new"))
    out_ref.backward(dy.double())
    Q = {k_: v.to(DEV).requires_grad_(True) for k_, v in P.items()}
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    wt_d, wt_u = VF.phm_expand_pair(Q["rule_d"], Q["W_d"], Q["rule_u"], Q["W_u"], n)
    pk = VF.pack_pair([wt_d], [Q["b_d"]], wt_u, Q["b_u"], VF._io_dtype(xg))
    out = VF.parallel_adapter(xg, yg, wt_d, Q["b_d"], wt_u, Q["b_u"], pk, 1.0)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    errs = dict(out=rel_err(out, out_ref), dx=rel_err(xg.grad, xr.grad), dy=rel_err(yg.grad, yr.grad))
    for k_ in P:
        errs["d" + k_] = rel_err(Q[k_].grad, ref[k_].grad)
    print(errs)
    assert max(errs.values()) <= tol, errs
