"""vlpet_adapter_tail_fwd (csrc/adapter_tail.hip) on the GPU against the fp64 statement of tests/adapter_tail_spec.py: row counts around
the kernel's 16-row tile and the decode batch (1, T - 1, T, T + 1, 2T + 1, 250), both geometries, both norm modes, two scales, both IO
dtypes at the project's parity tolerances (bf16 1e-2, fp32 1e-3: max |error| over max(1, max |reference|)), fp32 and bf16 parameters; a
constant row (zero variance -> beta), a row with |h| in the hundreds; bitwise: run to run, independent of M, nothing written past row M.
The composed K2 -> K5 path's error on the same inputs is printed beside the fused one (recorded in profiles/r14_single_adapter.md), not
asserted."""
import functools

import pytest
import torch

import adapter_tail_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 16
MS = (1, T - 1, T, T + 1, 2 * T + 1, 250)
TOL = {torch.bfloat16: 1e-2, torch.float32: 1e-3}
BIG_ROW, CONST_ROW = 0, 3            # (present at every M >= 4; M = 1 has the big row only)


@functools.lru_cache(maxsize=None)
def case(d, r, dtype):
    """250 rows of inputs and the four fp64 references (norm x scale), computed once and shared: a call at M rows uses the first M"""
    t = S.make_case(250, d, r, seed=d + r, dtype=dtype, big_row=BIG_ROW)
    refs = {(norm, s): S.reference(**t, eps=1e-5, scale=s, norm=norm) for norm in (True, False) for s in (1.0, 0.5)}
    return t, refs


def run(t, M, dtype, norm, scale, pdtype=torch.float32, pad_rows=0):
    import vlpet_amd.adapter_tail as AT
    h, res = (t[k][:M].to(DEV, dtype).contiguous() for k in ("h", "res"))
    p = [t[k].to(DEV, pdtype).contiguous() for k in ("wd", "bd", "wu", "bu")]
    ln = None
    if norm:
        ln = torch.nn.LayerNorm(h.shape[-1], eps=1e-5).to(DEV)
        with torch.no_grad():
            ln.weight.copy_(t["gamma"])
            ln.bias.copy_(t["beta"])
    return AT.adapter_tail(h, res, *p, ln, scale)


def err(out, ref):
    return float((out.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_against_the_fp64_statement_at_every_row_count(d, r, dtype):
    t, refs = case(d, r, dtype)
    with torch.no_grad():
        for (norm, scale), ref in refs.items():
            for M in MS:
                e = err(run(t, M, dtype, norm, scale), ref[:M])
                print(f"adapter_tail d={d} r={r} {str(dtype)[6:]} norm={int(norm)} s={scale} M={M}: fused err {e:.3e}")
                assert e <= TOL[dtype], (M, norm, scale, e)


@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_bf16_parameters_next_to_both_io_dtypes(d, r):
    """(a model whose adapters were cast with the backbone: the parameters are read in their own dtype)"""
    t, _ = case(d, r, torch.bfloat16)
    tb = dict(t, **{k: t[k].bfloat16().float() for k in ("wd", "bd", "wu", "bu")})
    ref = S.reference(**tb)
    with torch.no_grad():
        for dtype in (torch.bfloat16, torch.float32):
            assert err(run(tb, 33, dtype, True, 1.0, pdtype=torch.bfloat16), ref[:33]) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_constant_row_gives_beta_and_a_large_row_stays_in_tolerance(d, r, dtype):
    t, _ = case(d, r, dtype)
    t = {k: v.clone() for k, v in t.items()}
    t["wu"].zero_()                               # the adapter adds s * b_u: constant per row when b_u is
    t["bu"].fill_(0.25)
    t["h"][CONST_ROW] = 1.5
    t["res"][CONST_ROW] = -0.75
    ref = S.reference(**t)
    assert float((ref[CONST_ROW] - t["beta"].double()).abs().max()) < 1e-9
    with torch.no_grad():
        out = run(t, 20, dtype, True, 1.0).double().cpu()
    assert float((out[CONST_ROW] - t["beta"].double()).abs().max()) <= TOL[dtype]
    assert float(t["h"][BIG_ROW].abs().max()) > 300
    assert float((out[BIG_ROW] - ref[BIG_ROW]).abs().max()) <= TOL[dtype] * max(1.0, float(ref[BIG_ROW].abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_bits_repeat_do_not_depend_on_m_and_stop_at_row_m(d, r, norm, dtype):
    from vlpet_amd import _lib
    t, _ = case(d, r, dtype)
    with torch.no_grad():
        a, b = run(t, 250, dtype, norm, 1.0), run(t, 250, dtype, norm, 1.0)
        small = run(t, T + 1, dtype, norm, 1.0)
    assert torch.equal(a, b)                                             # two calls, equal bits
    assert torch.equal(a[:T + 1], small)                                 # a row's bits: not a function of M or of its workgroup
    # sentinel rows behind row M (a tile's unused rows and one more tile) stay as they were
    lib = _lib.load()
    M = T + 1
    h, res = (t[k][:M].to(DEV, dtype).contiguous() for k in ("h", "res"))
    p = [t[k].to(DEV).contiguous() for k in ("wd", "bd", "wu", "bu")]
    g, be = t["gamma"].to(DEV), t["beta"].to(DEV)
    out = torch.full((M + 2 * T, d), 777.0, device=DEV, dtype=dtype)
    rc = lib.vlpet_adapter_tail_fwd(h.data_ptr(), res.data_ptr(), *[x.data_ptr() for x in p], g.data_ptr(), be.data_ptr(), out.data_ptr(),
                                    M, d, r, 1.0, 1e-5, int(norm), _lib.VLPET_F32, _lib.VLPET_BF16 if dtype == torch.bfloat16 else _lib.VLPET_F32,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:M], small) and bool((out[M:] == 777.0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_composed_k2_then_k5_error_is_printed_beside_the_fused_one(dtype):
    """K2 (x = residual = h) then K5 on the same inputs: the figure recorded in the profile; only the fused path is held to the bound"""
    from vlpet_amd.adapters import AdapterConfig, AdapterController
    from vlpet_amd.tail import sublayer_tail
    for d, r in ((64, 8), (768, 96)):
        t, refs = case(d, r, dtype)
        ctl = AdapterController(AdapterConfig(tasks=["vqa"], input_dim=d, d_model=d, use_single_adapter=True, reduction_factor=d // r)).to(DEV)
        ad = ctl.adapters["vqa"]
        ln = torch.nn.LayerNorm(d, eps=1e-5).to(DEV)
        with torch.no_grad():
            for dst, k in ((ad.down_sampler.weight, "wd"), (ad.down_sampler.bias, "bd"), (ad.up_sampler.weight, "wu"), (ad.up_sampler.bias, "bu"),
                           (ln.weight, "gamma"), (ln.bias, "beta")):
                dst.copy_(t[k])
            h, res = (t[k].to(DEV, dtype) for k in ("h", "res"))
            for norm in (True, False):
                comp = sublayer_tail(res, ctl(h, "vqa"), ln if norm else None, 0.0, False)
                fused = run(t, 250, dtype, norm, 1.0)
                ref = refs[(norm, 1.0)]
                print(f"adapter_tail d={d} r={r} {str(dtype)[6:]} norm={int(norm)} M=250: fused err {err(fused, ref):.3e}   composed K2+K5 err {err(comp, ref):.3e}")
                assert err(fused, ref) <= TOL[dtype]
