"""Downsample HIP kernel (csrc/downsample.hip) against the reference-generated fixture and the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import vlpet_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

# ---- launch geometry (csrc/downsample.hip) ------------------------------------------------------------------------------------
GATHER_CAP_ITEMS = 4096 * 256       # downsample.hip:113 (blocks capped at 256 * 16) x 256 threads: work items (8 channels of one output
                                    # token) per grid pass of downsample_kernel, the gather form
SLAB_LDS_BYTES = 64 * 1024          # downsample.hip:105: the slab form takes fp32 input whose s_in * s_in * 256 * 4 bytes fit in this


def test_downsample_fixture_bit_exact():
    from vlpet_amd.visual import Downsample
    g = np.load(os.path.join(G, "downsample_7to6_d64.npz"))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    ds = Downsample((6, 6))
    y, yb = ds((t("x"), t("boxes")))
    assert torch.equal(y.cpu(), torch.from_numpy(g["y"])) and torch.equal(yb.cpu(), torch.from_numpy(g["yb"]))
    y2, b2, i2, o2 = ds((t("x2"), t("boxes2"), t("img_ids"), t("obj_ids")))
    assert torch.equal(y2.cpu(), torch.from_numpy(g["y2"])) and torch.equal(b2.cpu(), torch.from_numpy(g["yb2"]))
    assert torch.equal(i2.cpu(), torch.from_numpy(g["yi2"])) and torch.equal(o2.cpu(), torch.from_numpy(g["yo2"]))


@pytest.mark.parametrize("B,L,dim,out", [(3, 49, 2048, 6), (1, 49, 8, 6), (2, 64, 512, 4), (2, 49, 2048, 7), (5, 100, 72, 3)])
def test_downsample_matches_oracle(B, L, dim, out):
    from vlpet_amd.visual import Downsample
    gen = torch.Generator().manual_seed(B * 1000 + L)
    x = torch.randn(B, L, dim, generator=gen)
    ds = Downsample((out, out))
    ref = O.downsample(x, (out, out))
    assert torch.equal(ds.downsample_inputs(x.cuda()).cpu(), ref)                       # fp32 -> fp32: bit exact
    yb = ds.downsample_inputs(x.cuda(), out_dtype=torch.bfloat16).cpu()                 # fused cast == cast of the pool
    assert torch.equal(yb, ref.to(torch.bfloat16))
    yb2 = ds.downsample_inputs(x.cuda().bfloat16()).cpu()                               # bf16 in
    assert torch.equal(yb2, O.downsample(x.bfloat16().float(), (out, out)).to(torch.bfloat16))


def test_downsample_bench_shape_nlvr():
    """BASELINE configs[1] NLVR shape: [166, 98, 2048] fp32 -> [166, 72, 2048] bf16."""
    from vlpet_amd.visual import Downsample
    gen = torch.Generator().manual_seed(3)
    B = 166
    x = torch.randn(B, 98, 2048, generator=gen)
    boxes = torch.zeros(B, 98, 4)
    img = torch.cat([torch.zeros(B, 49), torch.ones(B, 49)], 1).long()
    obj = torch.cat([torch.arange(49), torch.arange(49)]).unsqueeze(0).expand(B, -1).contiguous()
    y, b, i, o = Downsample((6, 6))((x.cuda(), boxes.cuda(), img.cuda(), obj.cuda()), out_dtype=torch.bfloat16)
    yr, br, ir, orr = O.downsample_nlvr(x, boxes, img, obj)
    assert torch.equal(y.cpu(), yr.to(torch.bfloat16)) and torch.equal(i.cpu(), ir) and torch.equal(o.cpu(), orr)
    assert y.shape == (B, 72, 2048) and b.shape == (B, 72, 4)


def _abi_downsample(x, s_out, out_dtype):
    """vlpet_downsample_fwd on x [B, L, dim] into a NaN-filled output with sentinel rows behind it."""
    from sentinel import pad_intact, padded_rows
    from vlpet_amd import _lib
    lib = _lib.load()
    B, L, dim = x.shape
    s_in = int(L ** 0.5)
    io = lambda dt: _lib.VLPET_F32 if dt == torch.float32 else _lib.VLPET_BF16
    xg = x.cuda()
    buf, out = padded_rows(B * s_out * s_out, dim, out_dtype)
    assert lib.vlpet_downsample_fwd(xg.data_ptr(), out.data_ptr(), B, s_in, s_out, dim, io(x.dtype), io(out_dtype),
                                    torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert pad_intact(buf, out)
    return out.cpu().view(B, s_out * s_out, dim)


@pytest.mark.parametrize("dtype,B,L,dim,out", [(torch.bfloat16, 360, 49, 2048, 6), (torch.float32, 64, 81, 2048, 4)])
def test_downsample_gather_form_past_the_grid_cap(dtype, B, L, dim, out):
    """The gather form (bf16 input; fp32 input whose 9 x 9 grid exceeds the slab form's LDS) against the oracle, bit for bit.  The
    bf16 case is 3.3 M work items: every thread walks three and some a fourth."""
    items = B * out * out * dim // 8
    if dtype == torch.bfloat16:
        assert items >= 3 * GATHER_CAP_ITEMS and items % GATHER_CAP_ITEMS != 0
    else:
        assert L * 256 * 4 > SLAB_LDS_BYTES
    x = torch.randn(B, L, dim, generator=torch.Generator().manual_seed(B + L)).to(dtype)
    ref = O.downsample(x.float(), (out, out)).to(dtype)
    assert torch.equal(_abi_downsample(x, out, dtype), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["slab", "gather"])
def test_downsample_nan_and_infinities_propagate_like_torch(dtype):
    """NaN in some windows, -inf filling one whole window, +inf in one: the output equals O.downsample of the same input, NaN
    positions included.  fp32 [3, 49, 2048] takes the slab form, the same in bf16 the gather form."""
    B, L, dim, out = 3, 49, 2048, 6
    assert L * 256 * 4 <= SLAB_LDS_BYTES and dim % 256 == 0
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(B, L, dim, generator=gen)
    x[torch.rand(B, L, dim, generator=gen) < 0.01] = float("nan")
    g = x.view(B, 7, 7, dim)
    g[0, 0:2, 0:2] = float("-inf")          # 7 -> 6: window (0, 0) is rows 0..1 x columns 0..1
    g[1, 3, 3, ::2] = float("inf")
    x = x.to(dtype)
    ref = O.downsample(x.float(), (out, out)).to(dtype)
    assert bool(ref.isnan().any()) and bool((ref[0, 0] == float("-inf")).all()) and bool((ref == float("inf")).any())
    got = _abi_downsample(x, out, dtype)
    assert torch.equal(got.isnan(), ref.isnan())
    assert torch.equal(got.nan_to_num(nan=0.0), ref.nan_to_num(nan=0.0))
