"""CPU: tests/bitfit_spec.py tied down.

* It IS the operation: the segmented sums are x[:, s w : (s + 1) w].sum(0); the activation backward is fp64 autograd of
  dropout(act(x)) with the spec's mask, and its sums are those of the rounded result.
* The bounds can be met: an fp32 restatement IN THE KERNELS' ORDER (bitfit_spec.kernel_order_sum) stays inside them at the shapes
  tests/test_gpu_biasgrad.py uses, on both sides of every change of the grid rule.
* The bounds can be missed: a segment one column off, the sum of the unrounded values at bf16, a shifted mask."""
import math

import pytest
import torch
import torch.nn.functional as F

import bitfit_spec as B

BF, F32 = torch.bfloat16, torch.float32
SEG_SHAPES = [(1, 16), (3, 64), (3, 768), (6, 768), (16, 16)]
SEED = 0x0BADC0FFEE123457


def _x(M, ld, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * M + ld)
    return (torch.randn(M, ld, generator=g) + 0.25).to(dtype)


def test_depth_counts_the_additions_of_the_code():
    # M = 28,000 rows: 1,024 workgroups of 4 waves, 7 rows per wave; the reduce: 64 partial rows per thread
    assert B.tail_blocks(28000) == 1024 and B.depth(28000, 1024) == 7 + 4 + 64 + 2 + 16
    assert B.tail_blocks(1) == 1 and B.depth(1, 1) == 1 + 4 + 1 + 2 + 16
    assert B.act_cols_partials(28000, 3072) == 2048 // 6 and B.act_cols_partials(9, 64) == 3
    assert B.grid_edges() == [1024, 1025, 2500, 2501, 8500, 8501]
    assert [B.tail_blocks(m) for m in B.grid_edges()] == [256, 256, 256, 512, 512, 1024]
    assert B.gamma(93) == pytest.approx(93 * 2.0 ** -24, rel=1e-5)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_segmented_sums_are_the_slices_summed(dtype):
    S, w, M = 3, 64, 33
    x = _x(M, S * w + 64, dtype)
    r = B.colsum_seg(x, S, w)
    for s in range(S):
        torch.testing.assert_close(r.out[s], x[:, s * w:(s + 1) * w].double().sum(0), rtol=1e-13, atol=1e-13)
    assert r.out.shape == (S, w) and bool((r.e_out > 0).all())


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("M", [1, 3, 33] + B.grid_edges())
def test_fp32_restatement_of_the_segmented_sums_is_inside_the_bound(dtype, M):
    for S, w in SEG_SHAPES if M <= 33 else [(3, 64), (16, 16)]:
        n = S * w
        x = _x(M, n + 64, dtype)
        r = B.colsum_seg(x, S, w)
        got = B.kernel_order_sum(x[:, :n].float(), B.tail_blocks(M)).reshape(S, w)
        assert B.worst(got, r.out, r.e_out) <= 1.0, (S, w)


def test_a_segment_one_column_off_is_outside_the_bound():
    S, w, M = 3, 64, 33
    x = _x(M, S * w + 64, F32)
    r = B.colsum_seg(x, S, w)
    off = B.colsum_seg(x, S, w, mut=("seg_shift",))
    assert B.worst(off.out, r.out, r.e_out) > 100.0
    # ... and so are the guard columns mistaken for the last segment's
    assert B.worst(x[:, 64:64 + S * w].double().sum(0).reshape(S, w), r.out, r.e_out) > 100.0


def _act_inputs(M, n, dtype):
    g = torch.Generator().manual_seed(5 + M + n)
    x = (torch.randn(M, n, generator=g) * 2.0).to(dtype)
    dy = torch.randn(M, n, generator=g)
    dy = (torch.where(dy < 0, -1.0, 1.0) * (dy.abs() + 0.25)).to(dtype)
    return dy, x


@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_activation_backward_is_autograd_of_the_eager_pair(act, p):
    M, n = 9, 64
    dy, x = _act_inputs(M, n, F32)
    k = B.keep_mask(M, n, SEED, p).double() * (float(B.DS.keep_scale(p)) if p else 1.0)
    xd = x.double().requires_grad_(True)
    fn = {"gelu": F.gelu, "relu": F.relu, "gelu_new": lambda t: F.gelu(t, approximate="tanh")}[act]
    (fn(xd) * k).backward(dy.double())
    r = B.act_dropout_bwd_cols(dy, x, act, p, SEED)
    torch.testing.assert_close(r.dx, xd.grad, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(r.sums, r.dx.float().double().sum(0), rtol=1e-13, atol=1e-13)
    if p:
        assert 0 < float((k == 0).double().mean()) < 0.5 and bool((r.dx[k == 0] == 0).all())
        assert not torch.equal(B.keep_mask(M, n, SEED, p), B.keep_mask(M, n, SEED, p, ctr=3))


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
@pytest.mark.parametrize("M,n", [(1, 8), (9, 64), (130, 256), (1031, 512), (8200, 64)])
def test_fp32_restatement_of_the_activation_backward_is_inside_the_bounds(dtype, act, M, n):
    p = 0.1
    dy, x = _act_inputs(M, n, dtype)
    r = B.act_dropout_bwd_cols(dy, x, act, p, SEED)
    k = B.keep_mask(M, n, SEED, p).float() * float(B.DS.keep_scale(p))
    dx32 = dy.float() * k * B.act_df(act, x.float())                       # the reference alone, in fp32
    assert B.worst(dx32, r.dx, r.e_dx) <= 1.0
    stored = dx32.to(dtype)
    assert B.worst(stored, r.dx, B.hold_io(r.e_dx, r.dx, dtype)) <= 1.0
    sums, e_sums, h = B.colsums_of_stored(stored, n)
    assert h == B.depth(M, B.act_cols_partials(M, n))
    got = B.kernel_order_sum(stored.float(), B.act_cols_partials(M, n))
    assert B.worst(got, sums, e_sums) <= 1.0


def test_sums_of_the_unrounded_values_are_outside_the_bound_at_bf16():
    M, n = 1031, 512
    dy, x = _act_inputs(M, n, BF)
    r = B.act_dropout_bwd_cols(dy, x, "gelu", 0.1, SEED)
    bad = B.act_dropout_bwd_cols(dy, x, "gelu", 0.1, SEED, mut=("unrounded",))
    assert B.worst(bad.sums, r.sums, r.e_sums) > 10.0
    # at fp32 the stored value is the fp32 product either way: the mutation is a bf16 one
    r32 = B.act_dropout_bwd_cols(dy.float(), x.float(), "gelu", 0.1, SEED)
    assert math.isfinite(B.worst(r32.stored.sum(0), r32.sums, r32.e_sums))


def test_a_shifted_mask_is_outside_the_bounds():
    M, n = 9, 64
    dy, x = _act_inputs(M, n, F32)
    r = B.act_dropout_bwd_cols(dy, x, "relu", 0.1, SEED)
    bad = B.act_dropout_bwd_cols(dy, x, "relu", 0.1, SEED, mut=("mask_shift",))
    assert B.worst(bad.dx, r.dx, r.e_dx) > 100.0
    assert B.worst(bad.sums, r.sums, r.e_sums) > 100.0
