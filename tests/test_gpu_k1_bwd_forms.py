"""One case per row of the K1 / K2 backward's plan (csrc/api.hip bwd_plan; the table of DESIGN.md section 4), each at the smallest
shape that reaches the row, against the CPU oracle through the product path (gpu_cases.run_k1 / run_k2).

A case first asserts that its shape IS on the intended row: with the form queries of the ABI (vlpet_adapter_gate_bwd_form: 2 = the
column-parallel pass 2 of pet_cols.hip / pet_cols6y.hip, 1 = both passes of pet_gate_bwd3.hip, 0 = row kernel + wgrad.hip;
vlpet_adapter_gate_bwd_finalize_launch) and, for what the ABI does not show (which pass 1, how many feature blocks, whether their
partial sums fit), with the row's definition written out below from the predicates.  Bounds: BASELINE.json's per-tensor 1e-2 (bf16) /
1e-3 (fp32); for bf16 the element-wise 0.1 on a 6 % floor and the bias gradients' per-column 5e-2 of tests/test_gpu_cols.py (where
they are argued); for fp32 the per-column 5e-3 of tests/test_gpu_kernels.py."""
import pytest
import torch

import gpu_cases as C

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
TOL = {F32: 1e-3, BF16: 1e-2}
EL_TOL = 0.1            # tests/test_gpu_cols.py (floor: gpu_cases.K1_EL_FLOOR)


def _align256(v):
    return (v + 255) // 256 * 256


def dz2_blocks(M, d):       # k1_dz2_feature_blocks
    return 4 if M <= 8192 and (d // 64) % 4 == 0 else 1


def dz6_blocks(M, d):       # k1_dz6_feature_blocks
    if M <= 8192 and (d // 64) % 6 == 0 and ((M + 127) // 128) * 6 <= 256:
        return 6
    return dz2_blocks(M, d)


def dz2_split_fits(M, d, tiles):     # the fp32 partial dz, [nfb][M][2][32 tiles], against the dh / dq area of a bf16 call
    return dz2_blocks(M, d) * M * 2 * 32 * tiles * 4 <= 2 * _align256(M * d * 2)


def dz6_runs(M, d):         # k1_dz6_applies by shape: above 16,384 rows, and where its feature split applies up to 8,192
    return M > 16384 or (M <= 8192 and dz6_blocks(M, d) > 1)


def _queries(M, d, r, dtype):
    import vlpet_amd.functional as F
    from vlpet_amd import _lib
    lib, tiles, io = _lib.load(), F.rank_tiles(r), (_lib.VLPET_F32 if dtype == F32 else _lib.VLPET_BF16)
    return lib.vlpet_adapter_gate_bwd_form(M, d, tiles, io), lib.vlpet_adapter_gate_bwd_finalize_launch(M, d, tiles, io), tiles


def _check_k1(dtype, **kw):
    ce, ee = {}, {}
    errs = C.run_k1(dtype, col_errs=ce, el_errs=ee, **kw)
    print("per tensor:", {k: f"{v:.2e}" for k, v in errs.items()})
    print("element-wise:", {k: f"{v:.3f}" for k, v in ee.items()}, "bias columns:", {k: f"{v:.3f}" for k, v in ce.items()})
    assert max(errs.values()) <= TOL[dtype], errs
    assert max(ce.values()) <= 5 * TOL[dtype], ce
    assert max(ee.values()) <= EL_TOL, ee


# (id, M, d, r, what the row's definition says of the shape: (form, finalize launch, pass 1, feature blocks or None))
GATED_BF16 = [
    ("dz2-split-on", 129, 256, 32, (2, 1, "dz2", 4)),
    ("dz2-split-off-room-short", 129, 256, 96, (2, 1, "dz2", 0)),
    ("dz2-unsplit-finalize", 33, 128, 96, (2, 1, "dz2", 1)),
    ("cols-finalize-launch", 8191, 128, 96, (2, 1, "dz2", 1)),
    ("cols-in-launch-reduce", 8192, 128, 96, (2, 0, "dz2", 1)),
    ("dz6-six-blocks", 129, 384, 192, (2, 1, "dz6", 6)),
    ("dz6-four-blocks", 129, 256, 192, (2, 1, "dz6", 4)),
    ("six-tiles-chain-split-pass1-past-six-blocks", 5377, 384, 192, (2, 1, "gate_dz", None)),
    ("six-tiles-chain-split-pass1-8193", 8193, 128, 192, (2, 1, "gate_dz", None)),
    ("dz6-unsplit", 16385, 128, 192, (2, 1, "dz6", 1)),
    ("bwd3-4096", 4096, 64, 96, (1, 0, "dz2", 1)),
    ("bwd2-4097", 4097, 64, 96, (0, 0, "gate_bwd2", None)),
]


@pytest.mark.parametrize("name,M,d,r,row", GATED_BF16, ids=[c[0] for c in GATED_BF16])
def test_gated_bf16_rows(name, M, d, r, row):
    form, fin, pass1, blocks = row
    got_form, got_fin, tiles = _queries(M, d, r, BF16)
    assert (got_form, got_fin) == (form, fin)
    # the row's definition: column-parallel pass 2 needs d % 128 = 0; up to three tiles pass 1 is k1_dz2_kernel, at six tiles
    # k1_dz6_kernel where dz6_runs; the older two-pass form takes M <= 4,096 (or six tiles), the chain-split row kernel the rest
    assert (form == 2) == (d % 128 == 0)
    if pass1 == "dz2":
        assert tiles <= 3 and (form == 2 or M <= 4096)
        nfb = dz2_blocks(M, d)
        assert (nfb if nfb == 1 or dz2_split_fits(M, d, tiles) else 0) == blocks       # (0: split wanted, silently off)
    elif pass1 == "dz6":
        assert tiles == 6 and dz6_runs(M, d) and dz6_blocks(M, d) == blocks
    elif pass1 == "gate_dz":
        assert tiles == 6 and not dz6_runs(M, d)
    else:
        assert tiles <= 3 and form == 0 and M > 4096
    if form == 2 and tiles <= 3:
        assert fin == (0 if M >= 8192 else 1)       # k1_in_launch_reduce
    # r = 192: the T5 script's scales, and its y (functional.K1_BWD_FROM_OUTPUT, the default) puts six tiles on pet_cols6y.hip
    kw = dict(delta_scale=4.0, x2_scale=0.5, gate_scale=0.3) if r == 192 else {}
    _check_k1(BF16, M=M, d=d, r=r, rg=r, nh=4, **kw)


def test_fp32_six_tiles_gate_cols_with_the_add_pass():
    """fp32 at r = 192: both passes of pet_gate_bwd3.hip (form 1); dx1_in takes the add_inplace launch after pass 2."""
    assert _queries(33, 64, 192, F32)[:2] == (1, 0)
    _check_k1(F32, M=33, d=64, r=192, rg=192, nh=4, dx1_in=True)


def test_previous_split_phases(monkeypatch):
    """`phases` 1|4 then 2|4 (functional.K1_BWD_PREVIOUS_SPLIT): bit 2 takes a shape of the column-parallel row off every two-pass
    form -- chain-split row kernel (which adds dx1_in itself), then wgrad.hip."""
    import vlpet_amd.functional as F
    assert _queries(129, 256, 96, BF16)[0] == 2
    monkeypatch.setattr(F, "K1_BWD_PREVIOUS_SPLIT", True)
    _check_k1(BF16, M=129, d=256, r=96, rg=96, nh=4, dx1_in=True)


def test_no_saved_block(monkeypatch):
    """Without the forward's block (functional.SAVE_ACTIVATIONS off) every predicate fails: pet_bwd_kernel<GATE> + wgrad.hip."""
    import vlpet_amd.functional as F
    monkeypatch.setattr(F, "SAVE_ACTIVATIONS", False)
    _check_k1(BF16, M=129, d=256, r=96, rg=96, nh=4)


@pytest.mark.parametrize("d,two_pass", [(128, True), (64, False)], ids=["saved-two-pass", "row-kernel"])
def test_ungated_bf16_rows(d, two_pass):
    """K2, bf16, saved block: both passes of pet_cols_ng.hip where d % 128 = 0 (ng_two_pass_applies), else pet_bwd_kernel + wgrad.hip."""
    assert (d % 128 == 0) == two_pass
    errs = C.run_k2(BF16, M=33, d=d, r=96)
    print("per tensor:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[BF16], errs
