"""tests/adapter_tail_spec.py against the project's own eager pieces in fp64: ``eager.adapter`` (the plain-torch adapter) followed by the
residual adds and ``F.layer_norm`` -- both statements of the fused operation (the formula, and the walk through the kernel's steps with its
roundings switched off) to 1e-12; with the roundings on, the walk stays within the IO dtype's parity tolerance of the formula."""
import pytest
import torch
import torch.nn.functional as F

import adapter_tail_spec as S


def _eager(t, scale, norm, eps):
    from vlpet_amd import eager
    from vlpet_amd.adapters.adapter_utils import Activations
    dd = {k: v.double() for k, v in t.items()}
    out = eager.adapter(dd["h"], dd["wd"], dd["bd"], dd["wu"], dd["bu"], Activations("gelu_new"), lambda z: None)
    v = dd["res"] + (dd["h"] + scale * out)
    return F.layer_norm(v, (v.shape[-1],), dd["gamma"], dd["beta"], eps) if norm else v


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_both_statements_equal_the_eager_composition_in_fp64(d, r, scale, norm):
    t = S.make_case(19, d, r, seed=d + r, big_row=3)
    want = _eager(t, scale, norm, 1e-5)
    kw = dict(eps=1e-5, scale=scale, norm=norm)
    lim = 1e-12 * max(1.0, float(want.abs().max()))
    assert float((S.reference(**t, **kw) - want).abs().max()) <= lim
    assert float((S.kernel_model(**t, **kw, exact=True) - want).abs().max()) <= lim


@pytest.mark.parametrize("io,tol", [(torch.bfloat16, 1e-2), (torch.float32, 1e-3)])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("d,r", [(64, 8), (768, 96)])
def test_the_kernels_roundings_stay_within_the_parity_tolerance(d, r, norm, io, tol):
    t = S.make_case(33, d, r, seed=7, dtype=io, big_row=5)
    ref = S.reference(**t, norm=norm)
    got = S.kernel_model(**t, norm=norm, io_dtype=io)
    assert float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))


def test_a_constant_row_normalises_to_beta():
    t = S.make_case(4, 64, 8, seed=1)
    t["wu"].zero_()
    t["bu"].fill_(0.25)
    t["h"][2] = 1.5
    t["res"][2] = -0.5
    for fn in (S.reference, S.kernel_model):
        out = fn(**t)
        assert float((out[2] - t["beta"].double()).abs().max()) <= 1e-3
