"""tests/phm_spec.py against the reference's own PHMLinear (tests/golden/phm_linear_*.npz, make_compacter_goldens.golden_phm_linear):
forward and every gradient to 1e-6 relative, the factorized chain included; the index convention pinned by a case small enough to
write out by hand; the package's plain-torch restatement (vl-pet_amd/eager.py) and ``PHMLinear`` against the same fixtures."""
import os

import numpy as np
import pytest
import torch

import phm_spec as S

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["phm_linear_64x8_n2", "phm_linear_8x64_n4", "phm_linear_12x6_n3"]


def _load(name):
    z = np.load(os.path.join(G, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _close(a, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(a, np.float64) - ref).max()
    assert err <= 1e-6 * max(1.0, np.abs(ref).max()), (what, err)


@pytest.mark.parametrize("name", FIXTURES)
def test_spec_reproduces_the_reference_layer(name):
    z = _load(name)
    fac = int(z["rank"]) > 0
    W = S.factors(z["W_left"], z["W_right"]) if fac else z["W"]
    assert W.shape[0] == int(z["n"]) and z["phm_rule"].shape == (int(z["n"]),) * 3
    _close(S.linear(z["x"], z["phm_rule"], W, z["b"]), z["y"], "y")
    dx, dA, dW, db = S.linear_grads(z["x"], z["phm_rule"], W, z["dy"])
    _close(dx, z["d_x"], "dx")
    _close(dA, z["d_phm_rule"], "d rule")
    _close(db, z["d_b"], "db")
    if fac:
        dL, dR = S.factor_grads(z["W_left"], z["W_right"], dW)
        _close(dL, z["d_W_left"], "dW_left")
        _close(dR, z["d_W_right"], "dW_right")
    else:
        _close(dW, z["d_W"], "dW")


def test_index_convention_by_hand():
    # n = 2, k = p = 1: H[a, c] = A[0, a, c] W[0] + A[1, a, c] W[1]
    A = np.array([[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0]]])
    W = np.array([[[10.0]], [[100.0]]])
    H = np.array([[1 * 10 + 5 * 100, 2 * 10 + 6 * 100], [3 * 10 + 7 * 100, 4 * 10 + 8 * 100]], dtype=np.float64)
    ht, mag = S.weight(A, W)
    assert np.array_equal(ht, H.T) and np.array_equal(mag, H.T) and np.array_equal(S.weight_loops(A, W), H)
    # a gradient that is 1 at H[a = 1, c = 0] only, i.e. at H^T[0, 1]
    Gt = np.zeros((2, 2))
    Gt[0, 1] = 1.0
    dA, dW, _, _ = S.weight_grads(A, W, Gt)
    want = np.zeros((2, 2, 2))
    want[0, 1, 0], want[1, 1, 0] = 10.0, 100.0
    assert np.array_equal(dA, want)
    assert np.array_equal(dW.reshape(-1), [3.0, 7.0])             # A[i, 1, 0]


def test_vectorised_form_equals_the_loops_and_blocks_are_kronecker_products():
    rng = np.random.default_rng(0)
    for n, k, p in ((3, 4, 2), (2, 1, 5), (4, 2, 2)):
        A, W = rng.standard_normal((n, n, n)), rng.standard_normal((n, k, p))
        ht, mag = S.weight(A, W)
        H = S.weight_loops(A, W)
        np.testing.assert_allclose(ht.T, H, rtol=0, atol=1e-13)
        np.testing.assert_allclose(H, sum(np.kron(A[i], W[i]) for i in range(n)), rtol=0, atol=1e-13)
        assert (mag >= np.abs(ht) - 1e-15).all()
        # gradients against finite differences of <G, H^T>
        Gt = rng.standard_normal(ht.shape)
        dA, dW, _, _ = S.weight_grads(A, W, Gt)
        f = lambda A_, W_: float((S.weight(A_, W_)[0] * Gt).sum())
        e = np.zeros_like(A); e[1, 0, n - 1] = 1e-6
        assert abs((f(A + e, W) - f(A - e, W)) / 2e-6 - dA[1, 0, n - 1]) <= 1e-6 * max(1.0, abs(dA[1, 0, n - 1]))
        e = np.zeros_like(W); e[n - 1, k - 1, 0] = 1e-6
        assert abs((f(A, W + e) - f(A, W - e)) / 2e-6 - dW[n - 1, k - 1, 0]) <= 1e-6 * max(1.0, abs(dW[n - 1, k - 1, 0]))


def test_budget_counts_products_and_adds_the_bf16_rounding():
    mag = np.array([1.0, 4.0])
    assert np.array_equal(S.budget(mag, 2), 4 * 2.0 ** -24 * mag)
    assert np.array_equal(S.budget(mag, 2, value=np.array([-2.0, 0.0]), bf16=True), 4 * 2.0 ** -24 * mag + np.array([2.0 ** -7, 0.0]))


@pytest.mark.parametrize("name", FIXTURES)
def test_package_layer_and_eager_restatement_match_the_reference(name):
    from vlpet_amd import eager
    from vlpet_amd.adapters import PHMLinear
    z = _load(name)
    n, rank = int(z["n"]), int(z["rank"])
    in_f, out_f = z["x"].shape[1], z["y"].shape[1]
    layer = PHMLinear(in_f, out_f, n, factorized_phm=rank > 0, phm_rank=max(rank, 1))
    keys = [k for k, _ in layer.named_parameters()]
    assert sorted(keys) == sorted(k for k in z if not k.startswith("d_") and k not in ("x", "y", "dy", "n", "rank"))
    layer.load_state_dict({k: torch.from_numpy(z[k]) for k in keys})
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    y = layer(x)
    (y * torch.from_numpy(z["dy"])).sum().backward()
    _close(y.detach().numpy(), z["y"], "y")
    _close(x.grad.numpy(), z["d_x"], "dx")
    for k, p in layer.named_parameters():
        _close(p.grad.numpy(), z["d_" + k], k)
    H = eager.phm_weight(layer.phm_rule, layer.slices()).detach().numpy()
    _close(H.T, S.weight(z["phm_rule"], layer.slices().detach().numpy())[0], "H")
