"""Specification of Compacter's PHM weight expansion (csrc/phm.hip, functional.phm_expand_pair) in fp64, written from the definition:

    PHMLinear(in, out, n):  rule A [n, n, n],  W [n, k, p]   (k = in / n, p = out / n)
    H[a k + kk, c p + pp] = sum_i A[i, a, c] W[i, kk, pp]           y = x H + b

and, for a gradient G of H^T (the nn.Linear layout [out, in] the kernels write and K2's backward returns):

    dW[i, kk, pp] = sum_{a, c} A[i, a, c] G[c p + pp, a k + kk]      dA[i, a, c] = sum_{kk, pp} G[c p + pp, a k + kk] W[i, kk, pp]

Loops over the definition's indices only where that is the clearest statement (``weight_loops``, used to pin the vectorised form).  Each
function also returns the sum of the absolute values of the terms of every element, from which the error budget follows:

    |computed - exact| <= (N + 2) * 2^-24 * sum |terms|         N products summed: n (forward), n^2 (dW), k p (dA)

which is derived, not measured: fp32 products summed in fp32 in ANY order err by at most gamma_N = N u / (1 - N u) times the sum of
absolute values (u = 2^-24: each product one rounding, each element passes through at most N - 1 rounded additions); the + 2 covers the
second-order part N^2 u^2 up to N = 5,792 and one more rounding of the result.  At the largest N of the GPU tests (k p = 18,432 for dA
at (768, 96, n = 2)) the rigorous constant is 0.1 % above (N + 2) u -- for a sum in which every element passes through all N - 1
additions; the kernels add in trees (4 per thread, 6 butterfly steps, 4 waves, the tiles), far inside either.
bf16 outputs add one rounding of the value: 2^-8 |value| (round to nearest: half of bf16's 2^-7 spacing)."""
import numpy as np

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def weight(A, W):
    """(H^T [n p, n k], sum |terms| of each element) in fp64"""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    n, k, p = W.shape
    assert A.shape == (n, n, n)
    # [c, pp, a, kk] = sum_i A[i, a, c] W[i, kk, pp]
    ht = np.einsum("iac,ikp->cpak", A, W).reshape(n * p, n * k)
    mag = np.einsum("iac,ikp->cpak", np.abs(A), np.abs(W)).reshape(n * p, n * k)
    return ht, mag


def weight_loops(A, W):
    """H [n k, n p] by the definition's loops (small shapes)"""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    n, k, p = W.shape
    H = np.zeros((n * k, n * p))
    for i in range(n):
        for a in range(n):
            for c in range(n):
                for kk in range(k):
                    for pp in range(p):
                        H[a * k + kk, c * p + pp] += A[i, a, c] * W[i, kk, pp]
    return H


def weight_grads(A, W, G):
    """G: gradient of H^T [n p, n k] -> (dA, dW, sum |terms| of dA, sum |terms| of dW)"""
    A, W, G = np.asarray(A, np.float64), np.asarray(W, np.float64), np.asarray(G, np.float64)
    n, k, p = W.shape
    g = G.reshape(n, p, n, k)                                  # [c, pp, a, kk]
    dA = np.einsum("cpak,ikp->iac", g, W)
    dW = np.einsum("iac,cpak->ikp", A, g)
    mA = np.einsum("cpak,ikp->iac", np.abs(g), np.abs(W))
    mW = np.einsum("iac,cpak->ikp", np.abs(A), np.abs(g))
    return dA, dW, mA, mW


def factors(W_left, W_right):
    """the n slices of a factorized W: W[i] = W_left[i] @ W_right[i]"""
    return np.einsum("ikr,irp->ikp", np.asarray(W_left, np.float64), np.asarray(W_right, np.float64))


def factor_grads(W_left, W_right, dW):
    L, R, dW = np.asarray(W_left, np.float64), np.asarray(W_right, np.float64), np.asarray(dW, np.float64)
    return np.einsum("ikp,irp->ikr", dW, R), np.einsum("ikr,ikp->irp", L, dW)


def linear(x, A, W, b):
    """y = x H + b and the pieces a backward needs"""
    ht, _ = weight(A, W)
    return np.asarray(x, np.float64) @ ht.T + (0.0 if b is None else np.asarray(b, np.float64))


def linear_grads(x, A, W, dy):
    """(dx, dA, dW, db) of y = x H + b under the upstream gradient dy"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    ht, _ = weight(A, W)
    G = dy.T @ x                                               # d/dH^T [out, in]
    dA, dW, _, _ = weight_grads(A, W, G)
    return dy @ ht, dA, dW, dy.sum(0)


def budget(mag, n_products, value=None, bf16=False):
    """the per-element error budget (module docstring); ``value``: the exact result, needed for bf16 outputs"""
    b = (n_products + 2) * U32 * np.asarray(mag, np.float64)
    if bf16:
        b = b + U_BF16 * np.abs(np.asarray(value, np.float64))
    return b
