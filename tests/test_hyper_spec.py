"""tests/hyper_spec.py (the fp64 specification of Hyperformer's weight generator, csrc/hyper.hip) pinned without a GPU: an index-convention
case by hand, the loops against the vectorised forms, torch's autograd of the plain composition, the budget's terms, and the package's
eager path (eager.hyper_generate) against the specification."""
import numpy as np
import pytest
import torch

import hyper_spec as S


def _case(n=(12, 3, 1, 7), E=3, P=5, seed=0, holes=True):
    rng = np.random.default_rng(seed)
    maps = [(rng.standard_normal((k, P)), rng.standard_normal(k)) for k in n]
    e = rng.standard_normal((E, P))
    dout = [[None if holes and (s + l) % 3 == 2 else rng.standard_normal(k) for l in range(E)] for s, k in enumerate(n)]
    return maps, e, dout


def test_index_convention_by_hand():
    """G [n, P] is nn.Linear's [out, in]; row l of out belongs to row l of e; a weight row viewed [r, d] is row-major"""
    G = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0], [11.0, 12.0]])          # n = 6, P = 2
    g = np.array([0.5, -0.5, 0.25, -0.25, 0.125, -0.125])
    e = np.array([[1.0, 0.0], [0.0, 1.0], [2.0, -1.0]])
    (out, mag), = S.generate([(G, g)], e)
    assert out.shape == (3, 6)
    assert np.array_equal(out[0], G[:, 0] + g) and np.array_equal(out[1], G[:, 1] + g)
    assert np.array_equal(out[2], 2 * G[:, 0] - G[:, 1] + g)
    assert np.array_equal(mag[2], 2 * G[:, 0] + G[:, 1] + np.abs(g))
    # layer 2's down weight for (r, d) = (2, 3): W[a, b] = out[2, a * 3 + b], i.e. F.linear(x, W) maps d = 3 inputs to r = 2 outputs
    W = out[2].reshape(2, 3)
    assert W[1, 0] == out[2, 3] and W[0, 2] == out[2, 2]
    dout = [[None, np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0]), None]]
    r = S.grads([(G, g)], e, dout)
    assert np.array_equal(r["dg"][0], dout[0][1])
    want = np.zeros((6, 2))
    want[3] = e[1]
    assert np.array_equal(r["dG"][0], want)
    want = np.zeros((3, 2))
    want[1] = G[3]
    assert np.array_equal(r["de"], want)


@pytest.mark.parametrize("n,E,P", [((12, 3, 1, 7), 3, 5), ((8,), 1, 1), ((4, 4), 6, 8)])
def test_loops_equal_the_vectorised_forms(n, E, P):
    maps, e, dout = _case(n, E, P, seed=E + P)
    for (out, mag), ref in zip(S.generate(maps, e), S.generate_loops(maps, e)):
        assert np.allclose(out, ref, rtol=1e-13, atol=1e-13)
        assert (mag >= np.abs(out) - 1e-12).all()
    r = S.grads(maps, e, dout)
    dGs, dgs, de = S.grads_loops(maps, e, dout)
    for a, b in zip(r["dG"] + r["dg"] + [r["de"]], dGs + dgs + [de]):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)
    for v, m in zip(r["dG"] + r["dg"] + [r["de"]], r["mG"] + r["mg"] + [r["me"]]):
        assert (m >= np.abs(v) - 1e-12).all()


def test_missing_rows_are_zero_rows():
    maps, e, dout = _case()
    dense = [[np.zeros(G.shape[0]) if t is None else t for t in d_s] for d_s, (G, _) in zip(dout, maps)]
    a, b = S.grads(maps, e, dout), S.grads(maps, e, dense)
    for k in ("dG", "dg", "mG", "mg"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    assert np.array_equal(a["de"], b["de"])


def test_gradients_are_torchs_autograd_of_the_composition():
    maps, e, dout = _case(seed=3)
    tm = [(torch.tensor(G, requires_grad=True), torch.tensor(g, requires_grad=True)) for G, g in maps]
    te = torch.tensor(e, requires_grad=True)
    loss = 0
    for (G, g), d_s in zip(tm, dout):
        out = torch.nn.functional.linear(te, G, g)
        for l, t in enumerate(d_s):
            if t is not None:
                loss = loss + (out[l] * torch.tensor(t)).sum()
    loss.backward()
    r = S.grads(maps, e, dout)
    for (G, g), dG, dg in zip(tm, r["dG"], r["dg"]):
        assert np.allclose(G.grad.numpy(), dG, rtol=1e-12, atol=1e-12) and np.allclose(g.grad.numpy(), dg, rtol=1e-12, atol=1e-12)
    assert np.allclose(te.grad.numpy(), r["de"], rtol=1e-12, atol=1e-12)


def test_budget_terms():
    mag = np.array([1.0, 4.0])
    assert np.array_equal(S.budget(mag, 9), 9 * 2.0 ** -24 * mag)
    assert np.array_equal(S.budget(mag, 9, np.array([-2.0, 0.5]), bf16=True), 9 * 2.0 ** -24 * mag + 2.0 ** -8 * np.array([2.0, 0.5]))
    # an fp32 evaluation of the forward in the kernel's order stays inside it
    maps, e, _ = _case((64, 5), 4, 8, seed=5)
    for (G, g), (out, m) in zip(maps, S.generate(maps, e)):
        G32, g32, e32 = G.astype(np.float32), g.astype(np.float32), e.astype(np.float32)
        (x, m32), = S.generate([(G32, g32)], e32)
        acc = np.zeros((4, G.shape[0]), np.float32)
        for p in range(8):
            acc = (acc.astype(np.float64) + e32[:, p:p + 1].astype(np.float64) * G32[:, p][None, :]).astype(np.float32)      # one rounding: fused
        got = acc + g32[None, :]
        assert (np.abs(got.astype(np.float64) - x) <= S.budget(m32, 9)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_eager_path_matches_the_spec(dtype):
    from vlpet_amd import eager
    maps, e, dout = _case((40, 6, 40, 9), 4, 8, seed=9, holes=False)
    tm = [(torch.tensor(G, dtype=dtype, requires_grad=True), torch.tensor(g, dtype=dtype, requires_grad=True)) for G, g in maps]
    te = torch.tensor(e, dtype=dtype, requires_grad=True)
    rows = eager.hyper_generate(tm, te)
    assert len(rows) == 4 and all(len(r) == 4 for r in rows) and rows[0][2].shape == (40,)
    spec_in = [(G.detach().numpy(), g.detach().numpy()) for G, g in tm]
    ref = S.generate(spec_in, te.detach().numpy())
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=0, atol=0)
    for s in range(4):
        got = torch.stack(rows[s]).detach().numpy().astype(np.float64)
        if dtype == torch.float64:
            assert np.allclose(got, ref[s][0], **tol)
        else:
            assert (np.abs(got - ref[s][0]) <= S.budget(ref[s][1], 9)).all()
    torch.autograd.backward([rows[s][l] for s in range(4) for l in range(4)], [torch.tensor(dout[s][l], dtype=dtype) for s in range(4) for l in range(4)])
    r = S.grads(spec_in, te.detach().numpy(), dout)
    for s, (G, g) in enumerate(tm):
        for got, want, m, nt in ((G.grad, r["dG"][s], r["mG"][s], 4), (g.grad, r["dg"][s], r["mg"][s], 4)):
            err = np.abs(got.numpy().astype(np.float64) - want)
            assert (err <= (1e-12 if dtype == torch.float64 else S.budget(m, nt) + 1e-30)).all()
    err = np.abs(te.grad.numpy().astype(np.float64) - r["de"])
    assert (err <= (1e-11 if dtype == torch.float64 else S.budget(r["me"], 95))).all()
