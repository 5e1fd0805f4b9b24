"""vlpet_hyper_gen_fwd / _bwd (csrc/hyper.hip) on the GPU against tests/hyper_spec.py under its derived error budget, fp32 and bf16
parameters: the fixtures' geometry, the launch script's (BART-base, one stack with cross-attention), the one-hypernet form, odd sizes
(fewer rows than a wave, P no multiple of 4), the limits of E, P and of the row-pointer table; NULL rows of dout, run-to-run bits of
the backward, guard elements around every output and the workspace, NaN-filled outputs fully overwritten, and autograd through
functional.hyper_generate + pack + K2 against the eager composition."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hyper_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK = lambda d, r: [r * d, r, d * r, d]          # one adapter's generators: down weight, down bias, up weight, up bias
# name -> (n of every map, E, P)
SHAPES = {
    "fixture": (BLOCK(64, 8) * 3, 2, 8),
    "script": (BLOCK(768, 96) * 3, 6, 8),
    "one_hypernet": (BLOCK(768, 96), 18, 64),
    "odd": ([192, 3, 1], 1, 5),
    "limits_E_P": ([300], 64, 64),
    "limits_rows": ([40, 7] * 8, 16, 16),             # S = 16, S * E = 256 row pointers
    "p12_p24": ([257, 31], 3, 12),                    # P between the instantiated widths, a slab edge
    "p24": ([513], 5, 24),
}
DTYPES = [torch.float32, torch.bfloat16]
PAD = 64            # guard elements on either side of every output (a multiple of 16 bytes in both dtypes)
GUARD = 7.25        # exactly representable in bf16


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """parameters (rounded to ``dtype``, so that the fp64 spec sees the values the kernel reads), embeddings and upstream gradients,
    on the CPU; every fifth row of dout is missing (None), and the whole of the last map's when it has more than one row"""
    n, E, P = SHAPES[name]
    g = torch.Generator().manual_seed(len(n) * 1000 + E * 10 + P)
    maps = [(torch.randn(k, P, generator=g).to(dtype), torch.randn(k, generator=g).to(dtype)) for k in n]
    e = torch.randn(E, P, generator=g)
    dout = [[None if (s * E + l) % 5 == 4 else torch.randn(k, generator=g) for l in range(E)] for s, k in enumerate(n)]
    if E > 1 and len(n) > 1:
        dout[-1] = [None] * E
    return maps, e, dout


def guarded(numel, dtype):
    """(whole buffer: GUARD on either side of ``numel`` NaNs, the view of those)"""
    buf = torch.full((numel + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
    buf[PAD:PAD + numel] = float("nan")
    return buf, buf[PAD:PAD + numel]


def guards_intact(buf, numel):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + numel:] == GUARD).all())


def tab(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def f64(t):
    return t.float().numpy().astype(np.float64)


def spec_maps(maps):
    return [(f64(G), f64(g)) for G, g in maps]


def run_fwd(name, dtype):
    from vlpet_amd import _lib
    lib = _lib.load()
    maps, e, _ = inputs(name, dtype)
    n, E, P = SHAPES[name]
    Gd, gd, ed = [G.to(DEV) for G, _ in maps], [g.to(DEV) for _, g in maps], e.to(DEV)
    outs = [guarded(E * k, dtype) for k in n]
    pdt = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    rc = lib.vlpet_hyper_gen_fwd(len(n), tab([t.data_ptr() for t in Gd]), tab([t.data_ptr() for t in gd]), (ctypes.c_int * len(n))(*n),
                                 ed.data_ptr(), E, P, tab([v.data_ptr() for _, v in outs]), pdt, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for (buf, v), k in zip(outs, n):
        assert guards_intact(buf, E * k)
        assert not bool(torch.isnan(v).any())                      # every element written
    return [f64(v.cpu()).reshape(E, k) for (_, v), k in zip(outs, n)]


def run_bwd(name, dtype, dout=None):
    """-> (dG list, dg list, de) as CPU fp32 tensors; guards around every output and the workspace checked"""
    from vlpet_amd import _lib
    lib = _lib.load()
    maps, e, dflt = inputs(name, dtype)
    dout = dflt if dout is None else dout
    n, E, P = SHAPES[name]
    Gd, ed = [G.to(DEV) for G, _ in maps], e.to(DEV)
    rows = [None if t is None else t.to(DEV) for d_s in dout for t in d_s]
    dG, dg, de = [guarded(k * P, torch.float32) for k in n], [guarded(k, torch.float32) for k in n], guarded(E * P, torch.float32)
    n_tab = (ctypes.c_int * len(n))(*n)
    nws = lib.vlpet_hyper_gen_workspace_bytes(len(n), n_tab, E, P)
    assert nws > 0 and nws % 4 == 0
    wbuf, ws = guarded(nws // 4, torch.float32)
    pdt = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    rc = lib.vlpet_hyper_gen_bwd(len(n), tab([None if t is None else t.data_ptr() for t in rows]), tab([t.data_ptr() for t in Gd]), n_tab,
                                 ed.data_ptr(), E, P, tab([v.data_ptr() for _, v in dG]), tab([v.data_ptr() for _, v in dg]),
                                 de[1].data_ptr(), ws.data_ptr(), nws, pdt, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf, v in dG + dg + [de]:
        assert guards_intact(buf, v.numel())
        assert not bool(torch.isnan(v).any())
    assert guards_intact(wbuf, nws // 4)
    return [v.cpu().clone() for _, v in dG], [v.cpu().clone() for _, v in dg], de[1].cpu().clone()


def within(got, exact, budget, what):
    err = np.abs(np.asarray(got, np.float64).reshape(exact.shape) - exact)
    worst = float((err - budget).max())
    print(f"{what}: worst error {float(err.max()):.3e}, worst error / budget {float((err / np.maximum(budget, 1e-300)).max()):.3f}")
    assert worst <= 0, (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_within_the_budget(name, dtype):
    maps, e, _ = inputs(name, dtype)
    n, E, P = SHAPES[name]
    got = run_fwd(name, dtype)
    for s, ((out, mag), o) in enumerate(zip(S.generate(spec_maps(maps), f64(e)), got)):
        assert o.shape == out.shape == (E, n[s])
        within(o, out, S.budget(mag, P + 1, out, dtype == torch.bfloat16), f"out[{s}] {name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_within_the_budget_and_bitwise_repeatable(name, dtype):
    maps, e, dout = inputs(name, dtype)
    n, E, P = SHAPES[name]
    first, again = run_bwd(name, dtype), run_bwd(name, dtype)
    for a, b in zip(first[0] + first[1] + [first[2]], again[0] + again[1] + [again[2]]):
        assert torch.equal(a, b)                                   # no atomics, a fixed order: the same bits
    ref = S.grads(spec_maps(maps), f64(e), dout)
    for s in range(len(n)):
        within(f64(first[0][s]), ref["dG"][s], S.budget(ref["mG"][s], E), f"dG[{s}] {name}")
        within(f64(first[1][s]), ref["dg"][s], S.budget(ref["mg"][s], E), f"dg[{s}] {name}")
    within(f64(first[2]), ref["de"], S.budget(ref["me"], sum(n)), f"de {name}")


@pytest.mark.parametrize("name", ["fixture", "odd", "p12_p24"])
def test_null_rows_of_dout_equal_zero_rows(name):
    maps, e, dout = inputs(name, torch.float32)
    dense = [[torch.zeros(k) if t is None else t for t in d_s] for d_s, k in zip(dout, SHAPES[name][0])]
    a, b = run_bwd(name, torch.float32), run_bwd(name, torch.float32, dense)
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        assert torch.equal(x, y)
    n, E, P = SHAPES[name]
    none = run_bwd(name, torch.float32, [[None] * E for _ in n])
    assert all(not bool(t.any()) for t in none[0] + none[1] + [none[2]])


def test_a_single_row_reaches_only_its_own_results():
    """one nonzero element of one row of dout: dG / dg of that map's row i and de's row l, nothing else (the index convention)"""
    name = "fixture"
    maps, e, _ = inputs(name, torch.float32)
    n, E, P = SHAPES[name]
    s0, l0, i0 = 2, 1, 300
    dout = [[None] * E for _ in n]
    row = torch.zeros(n[s0])
    row[i0] = 2.0
    dout[s0][l0] = row
    dG, dg, de = run_bwd(name, torch.float32, dout)
    for s in range(len(n)):
        if s != s0:
            assert not bool(dG[s].any()) and not bool(dg[s].any())
    assert torch.equal(dG[s0].view(n[s0], P)[i0], 2.0 * e[l0]) and int(torch.count_nonzero(dG[s0])) == int(torch.count_nonzero(e[l0]))
    assert float(dg[s0][i0]) == 2.0 and int(torch.count_nonzero(dg[s0])) == 1
    assert torch.equal(de.view(E, P)[l0], 2.0 * maps[s0][0][i0]) and not bool(de.view(E, P)[1 - l0].any())


def test_python_entry_counts_one_launch_and_refreshes_in_place():
    import vlpet_amd.functional as VF
    maps, e, _ = inputs("fixture", torch.float32)
    dev = [(G.to(DEV), g.to(DEV)) for G, g in maps]
    n0 = VF.HYPER_CALLS
    outs = VF.hyper_generate_into(dev, e.to(DEV))
    assert VF.HYPER_CALLS == n0 + 1
    ptrs = [o.data_ptr() for o in outs]
    dev2 = [(2 * G, g) for G, g in dev]
    again = VF.hyper_generate_into(dev2, e.to(DEV), out=outs)
    assert [o.data_ptr() for o in again] == ptrs and VF.HYPER_CALLS == n0 + 2
    ref = S.generate([(2 * G, g) for G, g in spec_maps(maps)], f64(e))
    for o, (x, mag) in zip(again, ref):
        within(f64(o.cpu()), x, S.budget(mag, 9), "refreshed")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_autograd_through_generator_and_k2_matches_the_eager_composition(d, r, dtype):
    """two layers, M = 48 rows each; tolerances: K2's in tests/test_gpu_kernels.py (1e-3 fp32 IO, 1e-2 bf16 IO; gpu_cases.rel_err)"""
    import math
    import vlpet_amd.functional as VF
    from vlpet_amd import eager
    from vlpet_amd.adapters.adapter_utils import Activations
    from gpu_cases import rel_err
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    M, E, P = 48, 2, 8
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(M, d, generator=g).to(dtype) for _ in range(E)]
    ys = [torch.randn(M, d, generator=g).to(dtype) for _ in range(E)]
    dys = [torch.randn(M, d, generator=g).to(dtype) for _ in range(E)]
    sc = 1.0 / math.sqrt(P)
    prm = [(torch.randn(r * d, P, generator=g) * sc / math.sqrt(d), torch.randn(r * d, generator=g) * 0.01),
           (torch.randn(r, P, generator=g) * sc * 0.1, torch.randn(r, generator=g) * 0.1),
           (torch.randn(d * r, P, generator=g) * sc / math.sqrt(r), torch.randn(d * r, generator=g) * 0.01),
           (torch.randn(d, P, generator=g) * sc * 0.1, torch.randn(d, generator=g) * 0.1)]
    e = torch.randn(E, P, generator=g)
    act = Activations("gelu_new")

    ref_p = [(G.double().requires_grad_(True), b.double().requires_grad_(True)) for G, b in prm]
    ref_e = e.double().requires_grad_(True)
    ref_x, ref_y = [x.double().requires_grad_(True) for x in xs], [y.double().requires_grad_(True) for y in ys]
    rows = eager.hyper_generate(ref_p, ref_e)
    ref_out = [ref_y[l] + eager.adapter(ref_x[l], rows[0][l].view(r, d), rows[1][l], rows[2][l].view(d, r), rows[3][l], act) for l in range(E)]
    torch.autograd.backward(ref_out, [t.double() for t in dys])

    gpu_p = [(G.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) for G, b in prm]
    gpu_e = e.to(DEV).requires_grad_(True)
    gx, gy = [x.to(DEV).requires_grad_(True) for x in xs], [y.to(DEV).requires_grad_(True) for y in ys]
    n0 = VF.HYPER_CALLS
    rows = VF.hyper_generate(gpu_p, gpu_e)
    assert VF.HYPER_CALLS == n0 + 1
    outs = []
    for l in range(E):
        wd, bd, wu, bu = rows[0][l].view(r, d), rows[1][l], rows[2][l].view(d, r), rows[3][l]
        pk = VF.pack_pair([wd], [bd], wu, bu, VF._io_dtype(gx[l]))
        outs.append(VF.parallel_adapter(gx[l], gy[l], wd, bd, wu, bu, pk, 1.0))
    torch.autograd.backward(outs, [t.to(DEV) for t in dys])
    torch.cuda.synchronize()
    errs = {"de": rel_err(gpu_e.grad, ref_e.grad)}
    for l in range(E):
        errs.update({f"out{l}": rel_err(outs[l], ref_out[l]), f"dx{l}": rel_err(gx[l].grad, ref_x[l].grad),
                     f"dy{l}": rel_err(gy[l].grad, ref_y[l].grad)})
    for s, ((G, b), (Gr, br)) in enumerate(zip(gpu_p, ref_p)):
        errs[f"dG{s}"], errs[f"dg{s}"] = rel_err(G.grad, Gr.grad), rel_err(b.grad, br.grad)
    print(errs)
    assert max(errs.values()) <= tol, errs
