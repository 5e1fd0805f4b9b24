"""Specification of Hyperformer's weight generator (csrc/hyper.hip, functional.hyper_generate) in fp64, written from the definition.
One stack's hyper-network is S linear maps applied to the same E embedding rows:

    map s: G_s [n_s, P], g_s [n_s] (nn.Linear layout)        e [E, P]
    out_s[l, i] = g_s[i] + sum_p G_s[i, p] e[l, p]           out_s [E, n_s]

and, for upstream gradients dout[s][l] [n_s] (``None``: zeros):

    dG_s[i, p] = sum_l dout[s][l][i] e[l, p]     dg_s[i] = sum_l dout[s][l][i]     de[l, p] = sum_s sum_i dout[s][l][i] G_s[i, p]

``generate_loops`` / ``grads_loops`` walk the definition's indices (small shapes; they pin the vectorised forms).  Each function also
returns the sum of the absolute values of the terms of every element, from which the error budget follows:

    |computed - exact| <= N * 2^-24 * sum |terms|        N terms added: P + 1 (forward), E (dG, dg), sum_s n_s (de)

which is derived, not measured: N terms summed in fp32 in any order, each product fused into its addition, pass through at most N
roundings of relative size u = 2^-24 each (the forward's first product is rounded once, then P - 1 fused additions and the bias).  The
kernels add de in trees (6 butterfly steps, 4 waves, the slabs in 16 runs), far inside N roundings per term.  bf16 outputs add one
rounding of the value: 2^-8 |value| (round to nearest: half of bf16's 2^-7 spacing)."""
import numpy as np

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def _f64(x):
    return np.asarray(x, np.float64)


def generate(maps, e):
    """maps: [(G_s, g_s)] -> [(out_s [E, n_s], sum |terms| of each element)] in fp64"""
    e = _f64(e)
    res = []
    for G, g in maps:
        G, g = _f64(G), _f64(g)
        assert G.ndim == 2 and g.shape == (G.shape[0],) and G.shape[1] == e.shape[1]
        res.append((e @ G.T + g[None, :], np.abs(e) @ np.abs(G).T + np.abs(g)[None, :]))
    return res


def generate_loops(maps, e):
    """[out_s] by the definition's loops"""
    e = _f64(e)
    E, P = e.shape
    res = []
    for G, g in maps:
        G, g = _f64(G), _f64(g)
        out = np.zeros((E, G.shape[0]))
        for l in range(E):
            for i in range(G.shape[0]):
                acc = g[i]
                for p in range(P):
                    acc += G[i, p] * e[l, p]
                out[l, i] = acc
        res.append(out)
    return res


def _dense(dout_s, E, n):
    """the rows of one map stacked [E, n], zeros where a row is None"""
    d = np.zeros((E, n))
    for l in range(E):
        if dout_s[l] is not None:
            d[l] = _f64(dout_s[l]).reshape(n)
    return d


def grads(maps, e, dout):
    """dout[s][l]: [n_s] or None -> dict(dG=[..], dg=[..], de=[E, P], mG=[..], mg=[..], me=[E, P]) (m*: sum |terms|)"""
    e = _f64(e)
    E, P = e.shape
    r = dict(dG=[], dg=[], mG=[], mg=[], de=np.zeros((E, P)), me=np.zeros((E, P)))
    for (G, _), d_s in zip(maps, dout):
        G = _f64(G)
        d = _dense(d_s, E, G.shape[0])
        r["dG"].append(d.T @ e)
        r["mG"].append(np.abs(d).T @ np.abs(e))
        r["dg"].append(d.sum(0))
        r["mg"].append(np.abs(d).sum(0))
        r["de"] += d @ G
        r["me"] += np.abs(d) @ np.abs(G)
    return r


def grads_loops(maps, e, dout):
    """(dG list, dg list, de) by the definition's loops"""
    e = _f64(e)
    E, P = e.shape
    dGs, dgs, de = [], [], np.zeros((E, P))
    for (G, _), d_s in zip(maps, dout):
        G = _f64(G)
        n = G.shape[0]
        dG, dg = np.zeros((n, P)), np.zeros(n)
        for l in range(E):
            if d_s[l] is None:
                continue
            row = _f64(d_s[l])
            for i in range(n):
                dg[i] += row[i]
                for p in range(P):
                    dG[i, p] += row[i] * e[l, p]
                    de[l, p] += row[i] * G[i, p]
        dGs.append(dG)
        dgs.append(dg)
    return dGs, dgs, de


def budget(mag, n_terms, value=None, bf16=False):
    """the per-element error budget (module docstring); ``value``: the exact result, needed for bf16 outputs"""
    b = n_terms * U32 * _f64(mag)
    if bf16:
        b = b + U_BF16 * np.abs(_f64(value))
    return b
