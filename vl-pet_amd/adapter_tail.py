"""Host glue of the fused "sequential adapter, then sublayer tail" launch (csrc/adapter_tail.hip, vlpet_adapter_tail_fwd):

    out = N(res + h + s * adapter(h)),     N = LayerNorm (BART) | identity (T5)

Inference form only (no dropout, nothing saved): the cached decode step of a Single-Adapter model runs it three times per decoder
layer at M = batch (x beams) rows, where K2 + K5 are two fixed-latency launches.  ``host.bart._adapter_then_tail`` /
``host.t5._adapter_then_tail`` decide when it is taken; everything else composes ``AdapterController`` (K2) and ``sublayer_tail`` (K5).
No CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .functional import _flat, _io_dtype, _need_cuda, _param_dtype, _ptr, _stream, _timed
from .tail import _f32_frozen

# Largest row count at which the fused launch was not slower than K2 + K5 through the C ABI (profiles/r14_single_adapter.md: bf16,
# d = 768, r = 96, calls alternating in one process); above it the helpers compose.
ADAPTER_TAIL_MAX_ROWS = 3500
CALLS = 0          # fused launches issued (tests assert on it; a replayed graph does not count)


def row_tile() -> int:
    return int(_lib.load().vlpet_adapter_tail_rows())


def applies(M: int, d: int, r: int, dtype: torch.dtype) -> bool:
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    io = _lib.VLPET_BF16 if dtype == torch.bfloat16 else _lib.VLPET_F32
    return bool(_lib.load().vlpet_adapter_tail_applies(int(M), int(d), int(r), io))


def adapter_tail(h: torch.Tensor, res: torch.Tensor, down_w, down_b, up_w, up_b, norm: Optional[torch.nn.Module],
                 scale: float = 1.0) -> torch.Tensor:
    """``norm(res + h + scale * (up(gelu_new(down(h) + down_b)) + up_b))`` for ``h``, ``res`` [..., d] (bf16 or fp32, CUDA);
    ``norm``: an ``nn.LayerNorm`` or None (plain residual sum).  The four parameters are read in place (one dtype among them)."""
    global CALLS
    lib = _lib.load()
    _need_cuda(h, res, down_w, down_b, up_w, up_b)
    d = h.shape[-1]
    r = down_w.shape[0]
    io = _io_dtype(h)
    if res.dtype != h.dtype:
        res = res.to(h.dtype)
    ps = [p.detach() for p in (down_w, down_b, up_w, up_b)]
    if len({p.dtype for p in ps}) != 1 or not all(p.is_contiguous() for p in ps):
        raise RuntimeError("vl-pet_amd: adapter_tail needs the adapter's parameters contiguous and in one dtype")
    if tuple(up_w.shape) != (d, r) or tuple(down_w.shape) != (r, d):
        raise RuntimeError(f"vl-pet_amd: adapter weights {tuple(down_w.shape)} / {tuple(up_w.shape)} do not match d = {d}")
    hf, rf = _flat(h, d), _flat(res, d)
    M = hf.shape[0]
    out = torch.empty_like(hf)
    g32 = b32 = None
    eps = 0.0
    if norm is not None:
        g32, b32, eps = _f32_frozen(norm.weight), _f32_frozen(norm.bias), float(norm.eps)
    rc = _timed("adapter_tail", M, lambda: lib.vlpet_adapter_tail_fwd(
        hf.data_ptr(), rf.data_ptr(), ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(), ps[3].data_ptr(), _ptr(g32), _ptr(b32),
        out.data_ptr(), M, d, r, float(scale), eps, 0 if norm is None else 1, _param_dtype(ps[0]), io, _stream()))
    _lib.check(rc, "vlpet_adapter_tail_fwd")
    CALLS += 1
    return out.view(h.shape)
