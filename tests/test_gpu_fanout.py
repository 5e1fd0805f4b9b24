"""GPU: vlpet_sum_n and functional.fanout -- the gradient of a tensor that several consumers read (the encoder output under every
decoder layer's cross-attention, my_transformers/modeling_bart.py:2300-2330) summed in ONE launch instead of autograd's pairwise adds."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 6, 8, 9, 12, 17])
def test_sum_n_through_the_abi(n, dtype):
    from vlpet_amd import _lib
    lib = _lib.load()
    torch.manual_seed(n)
    L = 8 * 12345                       # not a multiple of the block size
    srcs = [torch.randn(L, device="cuda").to(dtype) for _ in range(n)]
    ref = torch.stack([s.float() for s in srcs]).sum(0)
    out = torch.empty(L, dtype=dtype, device="cuda")
    arr = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    io = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vlpet_sum_n(arr, n, out.data_ptr(), L, io, st) == 0
    torch.cuda.synchronize()
    # one rounding per launch of eight sources: n <= 8 is the exactly rounded fp32 sum; beyond, a rounding per extra launch
    tol = (2.0 ** -8 if dtype == torch.bfloat16 else 1e-6) * (1 + (n - 1) // 7)
    assert float((out.float() - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
    if n <= 8 and dtype == torch.bfloat16:
        assert torch.equal(out, ref.to(dtype))
    # in place over the first source
    assert lib.vlpet_sum_n(arr, n, srcs[0].data_ptr(), L, io, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(srcs[0], out)
    assert lib.vlpet_sum_n(arr, n, out.data_ptr(), L + 4, io, st) == -1        # VLPET_E_SHAPE: len % 8


# ---- launch geometry (csrc/optim.hip) -----------------------------------------------------------------------------------------
SUM_N_CAP_GROUPS = 4096 * 256       # optim.hip:179 (blocks capped at 4096) x OPT_THREADS = 256: 8-element groups per grid pass
                                    # (8,388,608 elements; the encoder-output gradient the kernel exists for is 21.5 M)


@pytest.mark.parametrize("n,dtype", [(2, torch.bfloat16), (8, torch.bfloat16), (3, torch.float32)])
def test_sum_n_past_the_grid_cap(n, dtype):
    """L = 8 (3 G + 5): every thread walks three groups, the first five a fourth.  Against the fp64 sum of the same sources: bf16
    exactly rounded (the fp32 sum in source order, rounded once -- and between round(exact - e) and round(exact + e), e the fp32
    accumulation error), fp32 within the present tolerance; then in place over the first source.  Outputs are NaN-filled with sentinel elements
    behind."""
    from sentinel import pad_intact, padded_flat
    from vlpet_amd import _lib
    lib = _lib.load()
    L = 8 * (3 * SUM_N_CAP_GROUPS + 5)
    assert L >= 3 * 8 * SUM_N_CAP_GROUPS
    torch.manual_seed(100 + n)
    s0buf, s0 = padded_flat(L, dtype)
    s0.copy_(torch.randn(L, device="cuda").to(dtype))
    srcs = [s0] + [torch.randn(L, device="cuda").to(dtype) for _ in range(n - 1)]
    host = [s.cpu() for s in srcs]
    ref64 = torch.zeros(L, dtype=torch.float64)
    abs64 = torch.zeros(L, dtype=torch.float64)
    ref32 = torch.zeros(L, dtype=torch.float32)
    for h in host:
        ref64 += h.double(); abs64 += h.double().abs(); ref32 += h.float()
    obuf, out = padded_flat(L, dtype)
    arr = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    io = _lib.VLPET_F32 if dtype == torch.float32 else _lib.VLPET_BF16
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vlpet_sum_n(arr, n, out.data_ptr(), L, io, st) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert pad_intact(obuf, out)
    eps = n * 2.0 ** -24 * abs64                     # running fp32 sum of n terms
    if dtype == torch.bfloat16:
        assert torch.equal(got, ref32.to(dtype))
        lo, hi = (ref64 - eps).to(dtype).double(), (ref64 + eps).to(dtype).double()     # rounding is monotone
        assert bool(((got.double() >= lo) & (got.double() <= hi)).all())
    else:
        assert float((got.double() - ref64).abs().max()) <= 1e-6 * max(1.0, float(ref64.abs().max()))
        assert bool(((got.double() - ref64).abs() <= eps).all())
    assert lib.vlpet_sum_n(arr, n, s0.data_ptr(), L, io, st) == 0        # in place over the first source
    torch.cuda.synchronize()
    assert torch.equal(s0, out) and pad_intact(s0buf, s0)


def test_fanout_sums_the_consumers_gradients_in_one_launch(monkeypatch):
    import vlpet_amd.functional as VF
    torch.manual_seed(0)
    x = torch.randn(7, 33, 768, device="cuda").bfloat16().requires_grad_(True)
    ws = [torch.randn(768, 768, device="cuda").bfloat16() * 0.05 for _ in range(6)]
    calls = []
    orig = VF._FanoutFn.backward
    monkeypatch.setattr(VF._FanoutFn, "backward", staticmethod(lambda ctx, *gs: (calls.append(len(gs)), orig(ctx, *gs))[1]))
    ys = VF.fanout(x, 6)
    assert all(y.data_ptr() == x.data_ptr() for y in ys)
    sum((y @ w).float().square().sum() for y, w in zip(ys, ws)).backward()
    g_fan, x.grad = x.grad, None
    assert calls == [6]
    sum((x @ w).float().square().sum() for w in ws).backward()        # autograd's pairwise accumulation
    ref64 = sum(((2 * (x.detach().double() @ w.double())) @ w.double().t()) for w in ws)
    e_fan = float((g_fan.double() - ref64).abs().max()); e_auto = float((x.grad.double() - ref64).abs().max())
    assert e_fan <= 2.0 ** -7 * float(ref64.abs().max()) and e_fan <= 1.5 * e_auto + 1e-6       # one rounding instead of five
    # off the GPU path (no gradient wanted / switch off): plain references
    with torch.no_grad():
        assert all(y is x for y in VF.fanout(x, 3))
    monkeypatch.setattr(VF, "FANOUT_SUM", False)
    assert all(y is x for y in VF.fanout(x, 3))
