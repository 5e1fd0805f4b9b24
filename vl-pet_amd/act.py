"""Host glue of the FFN activation + dropout pass (csrc/actdrop.hip): ``dropout(act(x), p)`` between fc1 and fc2 of the
backbone's feed-forward sublayer as one HIP pass forward and one backward.

Reference op chains replaced: my_transformers/modeling_bart.py:1264-1265 (encoder), :1750-1756 (decoder);
my_transformers/modeling_t5.py:262-265 (T5DenseReluDense).  Only the pre-activation is kept for the backward (the
reference keeps x, act(x) and a byte mask); the mask is a function of (seed, element index) and is regenerated.
One 64-bit seed per call from torch's CPU generator, as the sublayer tail does.  No CPU fallback."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .functional import _io_dtype, _need_cuda, _ptr, _stream, _timed
from .tail import _draw_seed

ACTS = {"gelu": 0, "gelu_new": 1, "relu": 2}


class _ActDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, p, seed, want_mask):
        lib = _lib.load()
        _need_cuda(x)
        xc = x.contiguous()
        n = xc.numel()
        io = _io_dtype(xc)
        out = torch.empty_like(xc)
        mask = torch.empty(xc.shape, dtype=torch.uint8, device=x.device) if want_mask else None
        rc = _timed("ffn_act_fwd", n // xc.shape[-1], lambda: lib.vlpet_act_dropout_fwd(
            xc.data_ptr(), out.data_ptr(), _ptr(mask), n, act, float(p), seed, io, _stream()))
        _lib.check(rc, "vlpet_act_dropout_fwd")
        ctx.save_for_backward(xc)
        ctx.cfg = (act, float(p), seed, io)
        if want_mask:
            ctx.mark_non_differentiable(mask)
            return out, mask
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        lib = _lib.load()
        (xc,) = ctx.saved_tensors
        act, p, seed, io = ctx.cfg
        dy = dout.contiguous()
        if dy.dtype != xc.dtype:
            dy = dy.to(xc.dtype)
        dx = torch.empty_like(xc)
        n = xc.numel()
        rc = _timed("ffn_act_bwd", n // xc.shape[-1], lambda: lib.vlpet_act_dropout_bwd(
            dy.data_ptr(), xc.data_ptr(), dx.data_ptr(), n, act, p, seed, io, _stream()))
        _lib.check(rc, "vlpet_act_dropout_bwd")
        return dx, None, None, None, None


def act_dropout(x: torch.Tensor, act: str = "gelu", p: float = 0.0, training: bool = False, seed=None,
                return_mask: bool = False):
    """``F.dropout(act(x), p, training)`` in one pass; ``act`` in {"gelu", "gelu_new", "relu"}.  The last dimension
    must be a multiple of 8 (every FFN width is)."""
    if act not in ACTS:
        raise RuntimeError(f"vl-pet_amd: unsupported FFN activation {act!r} (expected one of {sorted(ACTS)})")
    if x.shape[-1] % 8 != 0:
        raise RuntimeError("vl-pet_amd: act_dropout needs a last dimension that is a multiple of 8")
    pe = float(p) if training else 0.0
    if seed is None:
        seed = _draw_seed() if pe > 0.0 else 0
    return _ActDropFn.apply(x, ACTS[act], pe, int(seed), bool(return_mask))


# ------------------------------------------------------------------------------------------------ fc1 + activation, trainable fc1 bias
class _LinearActDropFn(torch.autograd.Function):
    """``dropout(act(x W^T + b), p)`` with a FROZEN weight and a TRAINABLE bias (BitFit): the backward runs the activation backward that
    also leaves the column partials of its result (vlpet_act_dropout_bwd_cols), reduces them into the bias's slot, then runs the dgrad
    GEMM onto whatever the sublayer's tail parked (the hand-over of functional._LinearAccFn) -- the [M, ffn] gradient is not read a
    second time for the bias."""

    @staticmethod
    def forward(ctx, x, w, b, link, act, p, seed):
        from . import functional as VF
        lib = _lib.load()
        _need_cuda(x)
        ctx.link = link.arm() if (link is not None and ctx.needs_input_grad[0]) else None
        pre = torch.nn.functional.linear(x, w, VF.io_view(b, x.dtype).detach()).contiguous()
        out = torch.empty_like(pre)
        n, io = pre.numel(), _io_dtype(pre)
        rc = _timed("ffn_act_fwd", n // pre.shape[-1], lambda: lib.vlpet_act_dropout_fwd(
            pre.data_ptr(), out.data_ptr(), None, n, act, float(p), seed, io, _stream()))
        _lib.check(rc, "vlpet_act_dropout_fwd")
        ctx.save_for_backward(pre, w, b)
        ctx.cfg = (act, float(p), seed, io)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import functional as VF
        lib = _lib.load()
        pre, w, b = ctx.saved_tensors
        act, p, seed, io = ctx.cfg
        link, ctx.link = ctx.link, None
        dy = dout.contiguous()
        if dy.dtype != pre.dtype:
            dy = dy.to(pre.dtype)
        n = pre.shape[-1]
        M = pre.numel() // n
        slot = VF.grad_slot(b, (n,))
        dpre = act_bwd_cols_into(dy, pre, act, p, seed, io, slot)
        db = slot.finish()
        dx = None
        if ctx.needs_input_grad[0]:
            xshape = (*pre.shape[:-1], w.shape[1])
            d2 = dpre.view(-1, n)
            base = link.take(xshape, w.dtype, writable=True) if link is not None else None
            dx = (d2 @ w if base is None else base.view(-1, w.shape[1]).addmm_(d2, w)).view(xshape)
        return dx, None, db, None, None, None, None


def act_bwd_cols_into(dy: torch.Tensor, pre: torch.Tensor, act: int, p: float, seed: int, io: int, slot) -> torch.Tensor:
    """-> dpre = dy * mask / (1 - p) * act'(pre) (bit for bit vlpet_act_dropout_bwd's), its column sums into ``slot.t`` [n]: now, or --
    for a slot of the trainer's flat buffer under DEFER_REDUCES -- with the step's other reductions (functional.flush_reduces)."""
    from . import functional as VF
    lib = _lib.load()
    n = pre.shape[-1]
    M = pre.numel() // n
    dpre = torch.empty_like(pre)
    nb = min((M + 3) // 4, 2048)                    # an upper bound of the partial rows (include/vlpet_hip.h); the call reports the count
    ws = torch.empty(nb * n, dtype=torch.float32, device=pre.device)
    got = ctypes.c_int(0)
    defer = VF.DEFER_REDUCES and slot.sunk
    rc = _timed("ffn_act_bwd_cols", M, lambda: lib.vlpet_act_dropout_bwd_cols(
        dy.data_ptr(), pre.data_ptr(), dpre.data_ptr(), M, n, act, p, seed, ws.data_ptr(), ws.numel() * 4,
        None if defer else slot.ptr, ctypes.addressof(got), io, _stream()))
    _lib.check(rc, "vlpet_act_dropout_bwd_cols")
    if defer:
        tf = slot.t.reshape(-1)
        VF.reduce_partials(ws, got.value, n // 2, tf[:n // 2], tf[n // 2:], True)
    VF.BITFIT_CALLS["act"] += 1
    return dpre


def linear_act_dropout_ok(x: torch.Tensor, fc1, act: str) -> bool:
    from . import functional as VF
    w, b = fc1.weight, fc1.bias
    return (VF.FUSE_BIAS_GRAD_SITES and act in ACTS and b is not None and b.requires_grad and not w.requires_grad and x.is_cuda
            and x.dtype in (torch.bfloat16, torch.float32) and w.shape[0] % 8 == 0 and w.shape[0] % 2 == 0 and x.numel() > 0
            and torch.is_grad_enabled())


def linear_act_dropout(x: torch.Tensor, fc1, act: str = "gelu", p: float = 0.0, training: bool = False, link=None, seed=None):
    """``dropout(act(fc1(x)), p)`` for an ``nn.Linear`` with a frozen weight and a trainable bias (see _LinearActDropFn); ``link``: the
    sublayer's hand-over, as for host.bart._first_linear."""
    pe = float(p) if training else 0.0
    if seed is None:
        seed = _draw_seed() if pe > 0.0 else 0
    w = fc1.weight if fc1.weight.dtype == x.dtype else fc1.weight.to(x.dtype)
    return _LinearActDropFn.apply(x, w, fc1.bias, link, ACTS[act], pe, int(seed))


# ------------------------------------------------------------------------------------------------ joint-encoder input assembly
FUSE_CONCAT_DROPOUT = True      # A/B switch (tools/ab_switches.py: VLPET_NO_CONCAT_DROPOUT=1): torch.cat + F.dropout instead


class _ConcatDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, v, p, seed):
        lib = _lib.load()
        _need_cuda(a, v)
        ac, vc = a.contiguous(), v.contiguous()
        B, La, d = ac.shape
        Lv = vc.shape[1]
        io = _io_dtype(ac)
        x = torch.empty(B, La + Lv, d, dtype=ac.dtype, device=ac.device)
        rc = _timed("concat_drop_fwd", B * (La + Lv), lambda: lib.vlpet_concat_dropout_fwd(
            ac.data_ptr(), vc.data_ptr(), x.data_ptr(), B, La, Lv, d, float(p), seed, io, _stream()))
        _lib.check(rc, "vlpet_concat_dropout_fwd")
        ctx.cfg = (B, La, Lv, d, float(p), seed, io, ac.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        lib = _lib.load()
        B, La, Lv, d, p, seed, io, dtype = ctx.cfg
        dxc = dx.contiguous()
        if dxc.dtype != dtype:
            dxc = dxc.to(dtype)
        da = torch.empty(B, La, d, dtype=dtype, device=dx.device) if ctx.needs_input_grad[0] else None
        dv = torch.empty(B, Lv, d, dtype=dtype, device=dx.device) if ctx.needs_input_grad[1] else None
        if da is None and dv is None:
            return None, None, None, None
        rc = _timed("concat_drop_bwd", B * (La + Lv), lambda: lib.vlpet_concat_dropout_bwd(
            dxc.data_ptr(), _ptr(da), _ptr(dv), B, La, Lv, d, p, seed, io, _stream()))
        _lib.check(rc, "vlpet_concat_dropout_bwd")
        return da, dv, None, None


def concat_dropout(a: torch.Tensor, v: torch.Tensor, p: float = 0.0, training: bool = False, seed=None) -> torch.Tensor:
    """``F.dropout(torch.cat([a, v], dim=1), p, training)`` for ``a [B, La, d]``, ``v [B, Lv, d]`` in one HIP pass each way
    (src/modeling_bart.py:804-820: the joint encoder's text | visual concatenation and the dropout behind it); plain torch ops where
    the kernel does not apply (CPU tensors, other dtypes, widths not a multiple of 8)."""
    pe = float(p) if training else 0.0
    ok = (FUSE_CONCAT_DROPOUT and a.is_cuda and v.is_cuda and a.dim() == 3 and v.dim() == 3 and a.dtype == v.dtype
          and a.dtype in (torch.bfloat16, torch.float32) and a.shape[0] == v.shape[0] and a.shape[2] == v.shape[2] and a.shape[2] % 8 == 0
          and a.shape[0] > 0 and a.shape[1] > 0 and v.shape[1] > 0)
    if not ok:
        return torch.nn.functional.dropout(torch.cat([a, v], dim=1), p=p, training=training)
    if seed is None:
        seed = _draw_seed() if pe > 0.0 else 0
    return _ConcatDropFn.apply(a, v, pe, int(seed))


# ------------------------------------------------------------------------------------------------ ... with a prompt in front
FUSE_PREFIX_CONCAT = True       # A/B switch (tools/ab_switches.py: VLPET_NO_PREFIX_CONCAT=1): expand + torch.cat + F.dropout instead


class _PrefixConcatDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, a, v, p, seed):
        lib = _lib.load()
        _need_cuda(pre, a, v)
        pc, ac, vc = pre.contiguous(), a.contiguous(), v.contiguous()
        B, La, d = ac.shape
        P, Lv = pc.shape[0], vc.shape[1]
        io = _io_dtype(ac)
        x = torch.empty(B, P + La + Lv, d, dtype=ac.dtype, device=ac.device)
        rc = _timed("prefix_concat_drop_fwd", B * (P + La + Lv), lambda: lib.vlpet_prefix_concat_dropout_fwd(
            pc.data_ptr(), ac.data_ptr(), vc.data_ptr(), x.data_ptr(), B, P, La, Lv, d, float(p), seed, io, _stream()))
        _lib.check(rc, "vlpet_prefix_concat_dropout_fwd")
        ctx.cfg = (B, P, La, Lv, d, float(p), seed, io, ac.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        lib = _lib.load()
        B, P, La, Lv, d, p, seed, io, dtype = ctx.cfg
        dxc = dx.contiguous()
        if dxc.dtype != dtype:
            dxc = dxc.to(dtype)
        dev = dx.device
        dpre = torch.empty(P, d, dtype=dtype, device=dev) if ctx.needs_input_grad[0] else None
        da = torch.empty(B, La, d, dtype=dtype, device=dev) if ctx.needs_input_grad[1] else None
        dv = torch.empty(B, Lv, d, dtype=dtype, device=dev) if ctx.needs_input_grad[2] else None
        if dpre is None and da is None and dv is None:
            return None, None, None, None, None
        # fp32 partials of dpre, one [P, d] slab per batch chunk (the chunk count is a function of B alone)
        ws = torch.empty(lib.vlpet_prefix_concat_ws_bytes(B, P, d) // 4, dtype=torch.float32, device=dev) if dpre is not None else None
        rc = _timed("prefix_concat_drop_bwd", B * (P + La + Lv), lambda: lib.vlpet_prefix_concat_dropout_bwd(
            dxc.data_ptr(), _ptr(dpre), _ptr(da), _ptr(dv), _ptr(ws), B, P, La, Lv, d, p, seed, io, _stream()))
        _lib.check(rc, "vlpet_prefix_concat_dropout_bwd")
        return dpre, da, dv, None, None


def prefix_concat_dropout(pre: torch.Tensor, a: torch.Tensor, v: torch.Tensor, p: float = 0.0, training: bool = False,
                          seed=None) -> torch.Tensor:
    """``F.dropout(torch.cat([pre.expand(B, -1, -1), a, v], dim=1), p, training)`` for ``pre [P, d]`` (the encoder prompt: the same
    rows for every batch item), ``a [B, La, d]``, ``v [B, Lv, d]`` in one HIP pass forward; backward one pass for ``da`` / ``dv`` and
    the batch sum ``dpre`` (fp32 partials per batch chunk, added in chunk order: no atomics, bitwise repeatable) -- the joint encoder's
    input assembly under prompt tuning (src/modeling_bart.py:776-820, src/modeling_t5.py:236-300).  Plain torch ops where the kernel
    does not apply (CPU tensors, other dtypes, widths not a multiple of 8)."""
    pe = float(p) if training else 0.0
    ok = (FUSE_PREFIX_CONCAT and pre.is_cuda and a.is_cuda and v.is_cuda and pre.dim() == 2 and a.dim() == 3 and v.dim() == 3
          and pre.dtype == a.dtype == v.dtype and a.dtype in (torch.bfloat16, torch.float32) and a.shape[0] == v.shape[0]
          and pre.shape[1] == a.shape[2] == v.shape[2] and a.shape[2] % 8 == 0 and a.shape[0] > 0 and pre.shape[0] > 0
          and a.shape[1] > 0 and v.shape[1] > 0)
    if not ok:
        return torch.nn.functional.dropout(torch.cat([pre.expand(a.shape[0], -1, -1), a, v], dim=1), p=p, training=training)
    if seed is None:
        seed = _draw_seed() if pe > 0.0 else 0
    return _PrefixConcatDropFn.apply(pre, a, v, pe, int(seed))
