"""Host glue of the attention kernels: ``dropout(softmax(scale * q k^T + mask), p) v`` on bf16 tensors of head dim 64 that stay in the
``[B, L, H * 64]`` layout the projections produce (no head transpose / re-pack in either direction).  No CPU fallback.

Reference op chain replaced: BartAttention.forward (my_transformers/modeling_bart.py:283-566): bmm, mask add, softmax,
F.dropout(p=attention_dropout), bmm, head transposes.  A bias shared by the batch -- T5's relative position bias
(my_transformers/modeling_t5.py:520-560, 640-660) -- is taken as ``AttnBias`` (round 4).

Three kernel families, each with a separate-q/k/v and a fused-``qkv`` wrapper:
  ``short``       ``short_attention`` / ``short_self_attention`` (csrc/attn.hip): at most 128 keys / queries -- the lengths VL-PET
                  trains on -- forward and backward on chip, one workgroup per (batch, head);
  ``long``        ``long_attention`` / ``long_self_attention`` (csrc/attn_long.hip): the forward alone for up to 1,024 keys / queries --
                  the video configuration's 664-token encoder under ``no_grad`` -- with a fixed summation order: no dropout, no autograd;
  ``long_train``  ``long_attention_train`` / ``long_self_attention_train`` (csrc/attn_long.hip with dropout + csrc/attn_long_bwd.hip):
                  the training form at those lengths, dropout by the short kernels' mask rule, a backward with a fixed order as well.

Structure: ONE launch layer (``_launch_fwd`` / ``_launch_bwd`` take the family and the full argument set; the forward-only
``_launch_long`` beside them), ONE autograd pair for both training families (``_AttnFn``: separate q, k, v; ``_AttnQkvFn``: one
``[B, L, 3E]`` tensor; the family is a non-tensor argument), ONE preamble for the four training wrappers (``_train_args``).
``route`` is the rule that picks a family for a call (or none: the library path -- fp32 parity runs, longer sequences, per-sample
additive biases), ``attend`` / ``attend_qkv`` call the wrapper of a family: the host models (host/bart.py, host/t5.py) hold no ladder
of their own."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .functional import _need_cuda, _ptr, _stream, _timed
from .tail import _draw_seed

MAX_LEN = 128
MAX_LONG = 1024      # the forward-only kernel of csrc/attn_long.hip (long_attention below)
HEAD_DIM = 64
LONG_CALLS = 0       # launches of the long kernel so far (tests tell by it which path ran)
LONG_TRAIN_CALLS = 0  # forward calls of long_attention_train / long_self_attention_train so far


class AttnBias:
    """An additive score bias ``[1 or none, H, Lq, Lk]`` shared by every sample, in the layout the kernels read: fp32, both
    sequence axes zero-padded to multiples of 32, plus its transpose for the key-major phase of the backward.  Built once per
    forward (it is the same for every layer of a T5 stack) and passed to ``short_attention(..., bias=...)``.  No gradient.
    ``transposed=False`` leaves the transpose to its first reader: a forward-only user (``long_attention`` at [12, 672, 672]: 21.7 MB
    per table) never builds it."""

    def __init__(self, bias: torch.Tensor, transposed: bool = True):
        b = bias.detach()
        if b.dim() == 4:
            if b.shape[0] != 1:
                raise RuntimeError("vl-pet_amd: AttnBias is shared by the batch ([1, H, Lq, Lk] or [H, Lq, Lk])")
            b = b[0]
        H, Lq, Lk = b.shape
        Lqp, Lkp = (Lq + 31) // 32 * 32, (Lk + 31) // 32 * 32
        self.H, self.Lq, self.Lk = H, Lq, Lk
        self.b = torch.zeros(H, Lqp, Lkp, dtype=torch.float32, device=b.device)
        self.b[:, :Lq, :Lk] = b.float()
        self._bt = self.b.transpose(1, 2).contiguous() if transposed else None

    @property
    def bt(self) -> torch.Tensor:
        if self._bt is None:
            self._bt = self.b.transpose(1, 2).contiguous()
        return self._bt


def supported(q: torch.Tensor, k: torch.Tensor, num_heads: int) -> bool:
    return (q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and q.shape[-1] == num_heads * HEAD_DIM
            and q.shape[1] <= MAX_LEN and k.shape[1] <= MAX_LEN)


class KeyGradSlot:
    """Where the key gradients of n attention calls go when their keys are the column blocks of ONE ``[B, Lk, n * E]`` buffer (the
    decoder layers' fused key projection of the encoder output, functional.cross_key_blocks): every call's backward writes its dk into
    block ``index`` of one gradient buffer of the same geometry, allocated by the first call that gets there, and the projection's
    backward consumes the whole buffer with a single GEMM."""

    def __init__(self, n: int, E: int):
        self.n, self.E, self.buf = n, E, None

    def block(self, k: torch.Tensor, index: int) -> torch.Tensor:
        if self.buf is None:
            self.buf = torch.empty(k.shape[0], k.shape[1], self.n * self.E, dtype=k.dtype, device=k.device)
        return self.buf[..., index * self.E:(index + 1) * self.E]


def _is_row_block(t: torch.Tensor) -> bool:
    """a [B, L, E] column block of a wider contiguous [B, L, ld] buffer that the kernels can read in place"""
    return (t.dim() == 3 and t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and t.stride(1) % 8 == 0
            and t.data_ptr() % 16 == 0)


# ---- the launch layer: per training family the (timer, C entry point, name in its error message) of the forward and of the backward.
# The short family's _kv entry points serve the separate and the qkv form alike (vlpet_attn_*_bias only forwards to them with ld_kv
# passed twice); ``what`` keeps the qkv form's name in an error message.
_FAMILY = {"short": (("attn_fwd", "vlpet_attn_fwd_kv", "vlpet_attn_fwd"), ("attn_bwd", "vlpet_attn_bwd_kv", "vlpet_attn_bwd")),
           "long_train": (("attn_long_fwd_train", "vlpet_attn_long_fwd_train", "vlpet_attn_long_fwd_train"),
                          ("attn_long_bwd", "vlpet_attn_long_bwd", "vlpet_attn_long_bwd"))}


def _check_bias(bias, H, Lq, Lk) -> None:
    if bias is not None and (bias.H, bias.Lq, bias.Lk) != (H, Lq, Lk):
        raise RuntimeError(f"vl-pet_amd: attention bias [{bias.H}, {bias.Lq}, {bias.Lk}] does not match [{H}, {Lq}, {Lk}]")


def _launch_fwd(family, q_ptr, k_ptr, v_ptr, key_mask, bias, o, lse, keep, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed, what=None):
    global LONG_TRAIN_CALLS
    timer, entry, name = _FAMILY[family][0]
    if family == "long_train" and scale == 0.0:
        raise RuntimeError("vl-pet_amd: long_attention_train needs a nonzero scale")
    _check_bias(bias, H, Lq, Lk)
    fn = getattr(_lib.load(), entry)
    if family == "long_train":
        LONG_TRAIN_CALLS += 1
    rc = _timed(timer, B * Lq, lambda: fn(
        q_ptr, k_ptr, v_ptr, _ptr(key_mask), bias.b.data_ptr() if bias is not None else None, o.data_ptr(), lse.data_ptr(), _ptr(keep),
        B, H, Lq, Lk, ld_q, ld_k, ld_v, int(causal), float(scale), float(p), seed, _stream()))
    _lib.check(rc, what or name)


def _launch_bwd(family, q_ptr, k_ptr, v_ptr, o, do, lse, key_mask, bias, dq_ptr, dk_ptr, dv_ptr, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale,
                p, seed, what=None):
    timer, entry, name = _FAMILY[family][1]
    fn = getattr(_lib.load(), entry)
    bias_t, scratch = None, ()
    if family == "long_train":
        # (the kernel reads the bias along keys in both passes: the transposed table, bias.bt, is never built for it)
        delta = torch.empty(B, H, Lq, dtype=torch.float32, device=o.device)        # the kernels' scratch: sum_d dO O per row
        scratch = (delta.data_ptr(),)
    elif bias is not None:
        bias_t = bias.bt.data_ptr()
    rc = _timed(timer, B * Lq, lambda: fn(
        q_ptr, k_ptr, v_ptr, o.data_ptr(), do.data_ptr(), lse.data_ptr(), _ptr(key_mask), bias.b.data_ptr() if bias is not None else None,
        bias_t, dq_ptr, dk_ptr, dv_ptr, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed, *scratch, _stream()))
    _lib.check(rc, what or name)


def _launch_long(q_ptr, k_ptr, v_ptr, key_mask, bias, o, lse, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale):
    global LONG_CALLS
    if scale == 0.0:
        raise RuntimeError("vl-pet_amd: long_attention needs a nonzero scale")
    _check_bias(bias, H, Lq, Lk)
    lib = _lib.load()
    LONG_CALLS += 1
    rc = _timed("attn_long_fwd", B * Lq, lambda: lib.vlpet_attn_long_fwd(
        q_ptr, k_ptr, v_ptr, _ptr(key_mask), bias.b.data_ptr() if bias is not None else None, o.data_ptr(), lse.data_ptr(),
        B, H, Lq, Lk, ld_q, ld_k, ld_v, int(causal), float(scale), _stream()))
    _lib.check(rc, "vlpet_attn_long_fwd")


def _grad_out(dout, like):
    do = dout.contiguous()
    return do if do.dtype == like.dtype else do.to(like.dtype)


# ---- the autograd pair of both training families (``family``: "short" | "long_train")
class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_mask, H, causal, scale, p, seed, want_mask, bias=None, k_slot=None, family="short"):
        _need_cuda(q, k, v)
        # (k_slot = (KeyGradSlot, index): k is a column block of the fused key projection's output and is read in place, row stride n * E)
        if k_slot is not None and not _is_row_block(k):
            k_slot = None
        q, v = q.contiguous(), v.contiguous()
        if k_slot is None:
            k = k.contiguous()
        B, Lq, E = q.shape
        Lk = k.shape[1]
        o = torch.empty_like(q)
        lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
        # (the kernel writes the mask only when it drops something: without dropout every element is kept)
        keep = torch.ones(B, H, Lq, Lk, dtype=torch.uint8, device=q.device) if want_mask else None
        _launch_fwd(family, q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask, bias, o, lse, keep, B, H, Lq, Lk, E, k.stride(1), E,
                    causal, scale, p, seed)
        ctx.save_for_backward(q, k, v, o, lse, key_mask)
        ctx.bias = bias
        ctx.k_slot = k_slot
        ctx.cfg = (family, H, int(causal), float(scale), float(p), seed)
        if want_mask:
            ctx.mark_non_differentiable(keep)
            return o, keep
        return o

    @staticmethod
    def backward(ctx, dout, *unused):
        q, k, v, o, lse, key_mask = ctx.saved_tensors
        family, H, causal, scale, p, seed = ctx.cfg
        B, Lq, E = q.shape
        Lk = k.shape[1]
        do = _grad_out(dout, q)
        dq, dv = torch.empty_like(q), torch.empty_like(v)
        k_slot, ctx.k_slot = ctx.k_slot, None
        # (the slot's block has k's strides; without a slot -- a second backward over a column block included -- so does a fresh tensor)
        dk = (torch.empty_strided(k.shape, k.stride(), dtype=k.dtype, device=k.device) if k_slot is None
              else k_slot[0].block(k, k_slot[1]))
        assert dk.stride() == k.stride()
        _launch_bwd(family, q.data_ptr(), k.data_ptr(), v.data_ptr(), o, do, lse, key_mask, ctx.bias, dq.data_ptr(), dk.data_ptr(),
                    dv.data_ptr(), B, H, Lq, Lk, E, k.stride(1), E, causal, scale, p, seed)
        ctx.bias = None
        return dq, dk, dv, None, None, None, None, None, None, None, None, None, None


class _AttnQkvFn(torch.autograd.Function):
    """Self-attention on a fused projection output ``qkv [B, L, 3*E]`` (columns q | k | v): the kernels read the three column
    blocks in place (row stride 3E) and the backward writes dq | dk | dv into ONE ``[B, L, 3E]`` gradient, which the fused
    projection's dgrad GEMM consumes directly."""

    @staticmethod
    def forward(ctx, qkv, key_mask, H, causal, scale, p, seed, bias=None, family="short"):
        _need_cuda(qkv)
        qkv = qkv.contiguous()
        B, L, E3 = qkv.shape
        E = E3 // 3
        o = torch.empty(B, L, E, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, H, L, dtype=torch.float32, device=qkv.device)
        base, esz = qkv.data_ptr(), qkv.element_size()
        _launch_fwd(family, base, base + E * esz, base + 2 * E * esz, key_mask, bias, o, lse, None, B, H, L, L, E3, E3, E3, causal, scale, p,
                    seed, what="vlpet_attn_fwd_bias" if family == "short" else None)
        ctx.save_for_backward(qkv, o, lse, key_mask)
        ctx.bias = bias
        ctx.cfg = (family, H, int(causal), float(scale), float(p), seed)
        return o

    @staticmethod
    def backward(ctx, dout):
        qkv, o, lse, key_mask = ctx.saved_tensors
        family, H, causal, scale, p, seed = ctx.cfg
        B, L, E3 = qkv.shape
        E = E3 // 3
        dqkv = torch.empty_like(qkv)
        base, dbase, esz = qkv.data_ptr(), dqkv.data_ptr(), qkv.element_size()
        _launch_bwd(family, base, base + E * esz, base + 2 * E * esz, o, _grad_out(dout, qkv), lse, key_mask, ctx.bias,
                    dbase, dbase + E * esz, dbase + 2 * E * esz, B, H, L, L, E3, E3, E3, causal, scale, p, seed,
                    what="vlpet_attn_bwd_bias" if family == "short" else None)
        ctx.bias = None
        return dqkv, None, None, None, None, None, None, None, None


def supported_qkv(qkv: torch.Tensor, num_heads: int) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.shape[-1] == 3 * num_heads * HEAD_DIM
            and qkv.shape[1] <= MAX_LEN)


# The kernels take the key mask as [B, Lk] bytes; the models hand every layer the same boolean mask (a fresh view of it per layer), so
# the conversion is kept for the last two sources: same storage, same version counter (an in-place write to the mask bumps it),
# same geometry -> the same bytes.  The entry holds the source view, which keeps its storage from being recycled under the key.
_KM_CACHE: list = []


def _key_mask_u8(key_mask: torch.Tensor, B: int, L: int) -> torch.Tensor:
    if key_mask.dtype == torch.uint8 and key_mask.shape == (B, L) and key_mask.is_contiguous():
        return key_mask
    if key_mask.is_inference():             # tensors made under torch.inference_mode() track no version: nothing to key the cache on
        return key_mask.reshape(B, L).to(torch.uint8).contiguous()
    for src, ver, out in _KM_CACHE:
        if (src.data_ptr() == key_mask.data_ptr() and ver == key_mask._version and src.dtype == key_mask.dtype
                and src.shape == key_mask.shape and src.stride() == key_mask.stride() and out.shape == (B, L)):
            return out
    out = key_mask.reshape(B, L).to(torch.uint8).contiguous()
    _KM_CACHE.insert(0, (key_mask, key_mask._version, out))
    del _KM_CACHE[2:]
    return out


def _train_args(key_mask, B, Lk, p, training, seed, scale):
    """The preamble of the four training wrappers: the key mask as bytes, the default scale, the dropout rate in effect and its seed"""
    if key_mask is not None:
        key_mask = _key_mask_u8(key_mask, B, Lk)
    pe = float(p) if training else 0.0
    if seed is None:
        seed = _draw_seed() if pe > 0.0 else 0
    return key_mask, HEAD_DIM ** -0.5 if scale is None else float(scale), pe, int(seed)


def short_self_attention(qkv: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None, causal: bool = False,
                         p: float = 0.0, training: bool = False, scale: Optional[float] = None, seed=None,
                         bias: Optional[AttnBias] = None):
    """qkv [B, L, 3*H*64] (bf16; the output of one fused q|k|v projection) -> [B, L, H*64].  bias: see short_attention."""
    if not supported_qkv(qkv, num_heads):
        raise RuntimeError("vl-pet_amd: short_self_attention needs a bf16 CUDA [B, L, 3*H*64] tensor with L <= 128")
    key_mask, scale, pe, seed = _train_args(key_mask, qkv.shape[0], qkv.shape[1], p, training, seed, scale)
    return _AttnQkvFn.apply(qkv, key_mask, num_heads, bool(causal), scale, pe, seed, bias, "short")


def short_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None,
                    causal: bool = False, p: float = 0.0, training: bool = False, scale: Optional[float] = None, seed=None,
                    return_mask: bool = False, bias: Optional[AttnBias] = None, k_slot=None):
    """q [B, Lq, H*64], k / v [B, Lk, H*64] (bf16) -> [B, Lq, H*64].  key_mask: [B, Lk] bool / uint8, True = attend.
    bias: an ``AttnBias`` ([H, Lq, Lk] added to the scaled scores of every sample; no gradient).  k_slot: (KeyGradSlot, index) when
    ``k`` is a column block of a fused key projection (read in place; its gradient goes into the slot's shared buffer)."""
    if not supported(q, k, num_heads):
        raise RuntimeError("vl-pet_amd: short_attention needs bf16 CUDA tensors, head dim 64 and at most 128 keys / queries")
    key_mask, scale, pe, seed = _train_args(key_mask, k.shape[0], k.shape[1], p, training, seed, scale)
    return _AttnFn.apply(q, k, v, key_mask, num_heads, bool(causal), scale, pe, seed, bool(return_mask), bias, k_slot, "short")


# ---- up to MAX_LONG keys / queries (csrc/attn_long.hip, csrc/attn_long_bwd.hip)
def supported_long(q: torch.Tensor, k: torch.Tensor, num_heads: int) -> bool:
    return (q.is_cuda and k.is_cuda and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and q.dim() == 3 and k.dim() == 3
            and q.shape[-1] == num_heads * HEAD_DIM and k.shape[-1] == num_heads * HEAD_DIM
            and 1 <= q.shape[1] <= MAX_LONG and 1 <= k.shape[1] <= MAX_LONG)


def _need_long(name, q, k, v, num_heads) -> None:
    if not (isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor) and isinstance(v, torch.Tensor)) or not supported_long(q, k, num_heads) \
            or v.dtype != q.dtype or not v.is_cuda or v.shape != k.shape or k.shape[0] != q.shape[0]:
        raise RuntimeError(f"vl-pet_amd: {name} needs bf16 CUDA tensors [B, L, H*64] with 1 <= Lq, Lk <= 1024 (k and v alike)")


def _need_long_qkv(name, qkv, num_heads) -> None:
    if not (isinstance(qkv, torch.Tensor) and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.shape[-1] == 3 * num_heads * HEAD_DIM and 1 <= qkv.shape[1] <= MAX_LONG):
        raise RuntimeError(f"vl-pet_amd: {name} needs a bf16 CUDA [B, L, 3*H*64] tensor with L <= 1024")


def _no_grad_needed(*tensors) -> None:
    if needs_grad(*tensors):
        raise RuntimeError("vl-pet_amd: long_attention is forward only (no autograd): call it under torch.no_grad() or on tensors "
                           "that need no gradient")


def long_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None,
                   causal: bool = False, scale: Optional[float] = None, bias: Optional[AttnBias] = None, return_lse: bool = False):
    """q [B, Lq, H*64], k / v [B, Lk, H*64] (bf16, 1 <= Lq, Lk <= 1024) -> softmax(scale q k^T + bias + masks) v [B, Lq, H*64]; with
    ``return_lse`` also the rows' log-sum-exp [B, H, Lq] (fp32, log2 units of the scaled scores, +inf for a row with no visible
    key -- such a row's output is zero).  Masks and bias as in ``short_attention``; no dropout, no autograd, no CPU fallback.
    k and v are read in place when they are column blocks of wider row-major buffers.  Bitwise reproducible; an item's result
    does not depend on the rest of the batch."""
    _need_long("long_attention", q, k, v, num_heads)
    _no_grad_needed(q, k, v)
    q, k, v = (t if _is_row_block(t) else t.contiguous() for t in (q.detach(), k.detach(), v.detach()))
    B, Lq, E = q.shape
    Lk = k.shape[1]
    if key_mask is not None:
        key_mask = _key_mask_u8(key_mask, B, Lk)
    o = torch.empty(B, Lq, E, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, num_heads, Lq, dtype=torch.float32, device=q.device)
    _launch_long(q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask, bias, o, lse, B, num_heads, Lq, Lk, q.stride(1), k.stride(1),
                 v.stride(1), causal, HEAD_DIM ** -0.5 if scale is None else float(scale))
    return (o, lse) if return_lse else o


def long_self_attention(qkv: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None, causal: bool = False,
                        scale: Optional[float] = None, bias: Optional[AttnBias] = None):
    """qkv [B, L, 3*H*64] (bf16; the output of one fused q|k|v projection, L <= 1024) -> [B, L, H*64]: ``long_attention`` on the three
    column blocks, read in place."""
    _need_long_qkv("long_self_attention", qkv, num_heads)
    _no_grad_needed(qkv)
    qkv = qkv.detach().contiguous()
    B, L, E3 = qkv.shape
    E = E3 // 3
    if key_mask is not None:
        key_mask = _key_mask_u8(key_mask, B, L)
    o = torch.empty(B, L, E, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, num_heads, L, dtype=torch.float32, device=qkv.device)
    base, esz = qkv.data_ptr(), qkv.element_size()
    _launch_long(base, base + E * esz, base + 2 * E * esz, key_mask, bias, o, lse, B, num_heads, L, L, E3, E3, E3, causal,
                 HEAD_DIM ** -0.5 if scale is None else float(scale))
    return o


# (the training form: dropout by the short kernels' mask rule -- seed + the device step counter -- and a backward without atomics whose
# sums have an order fixed by (Lq, Lk))
def long_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None,
                         causal: bool = False, p: float = 0.0, training: bool = False, scale: Optional[float] = None, seed=None,
                         return_mask: bool = False, bias: Optional[AttnBias] = None, k_slot=None):
    """``short_attention`` for 1 <= Lq, Lk <= 1024: q [B, Lq, H*64], k / v [B, Lk, H*64] (bf16) -> dropout(softmax(scale q k^T + bias +
    masks), p) v, with autograd.  Arguments as in ``short_attention``.  The output and the three gradients are bitwise reproducible and
    an item's do not depend on the rest of the batch; with ``p = 0`` (or ``training=False``) the output has the bits of
    ``long_attention``.  No CPU fallback."""
    _need_long("long_attention_train", q, k, v, num_heads)
    key_mask, scale, pe, seed = _train_args(key_mask, k.shape[0], k.shape[1], p, training, seed, scale)
    return _AttnFn.apply(q, k, v, key_mask, num_heads, bool(causal), scale, pe, seed, bool(return_mask), bias, k_slot, "long_train")


def long_self_attention_train(qkv: torch.Tensor, num_heads: int, key_mask: Optional[torch.Tensor] = None, causal: bool = False,
                              p: float = 0.0, training: bool = False, scale: Optional[float] = None, seed=None,
                              bias: Optional[AttnBias] = None):
    """``short_self_attention`` for L <= 1024: qkv [B, L, 3*H*64] (bf16; the output of one fused q|k|v projection) -> [B, L, H*64], the
    column blocks read in place and the gradient written as one [B, L, 3*H*64] tensor."""
    _need_long_qkv("long_self_attention_train", qkv, num_heads)
    key_mask, scale, pe, seed = _train_args(key_mask, qkv.shape[0], qkv.shape[1], p, training, seed, scale)
    return _AttnQkvFn.apply(qkv, key_mask, num_heads, bool(causal), scale, pe, seed, bias, "long_train")


# ---- routing: which family a call runs on, and the call
def needs_grad(*tensors, grad: bool = False) -> bool:
    """autograd will ask for a gradient of this call (``grad``: the caller knows of one that the tensors do not show)"""
    return torch.is_grad_enabled() and (grad or any(t.requires_grad for t in tensors))


def route(Lq: int, Lk: int, p: float, training: bool, needs_grad: bool, *, eager: bool, long_on: bool, long_train_on: bool):
    """The kernel family of an attention call by its lengths and by what it needs -- "short" | "long" | "long_train" -- or None: the
    library path.  ``eager`` / ``long_on`` / ``long_train_on``: the caller's EAGER_ATTENTION / LONG_ATTENTION / LONG_ATTENTION_TRAIN
    switches.  Whether the tensors are ones the family takes is ``fits``."""
    if eager:
        return None
    if max(Lq, Lk) <= MAX_LEN:
        return "short"
    if Lq > MAX_LONG or Lk > MAX_LONG:
        return None
    if (training and p > 0) or needs_grad:          # dropout or a backward: only the training form has them
        return "long_train" if long_train_on else None
    return "long" if long_on else None


def fits(kind, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int) -> bool:
    """q, k, v are tensors the wrappers of family ``kind`` (a ``route`` result) take"""
    if kind == "short":
        return supported(q, k, num_heads)
    return kind is not None and v.dtype == q.dtype and supported_long(q, k, num_heads)


def attend(kind, q, k, v, num_heads, key_mask=None, causal=False, p=0.0, training=False, scale=None, bias=None, k_slot=None):
    """separate q, k, v on family ``kind``; arguments as in ``short_attention`` (the forward-only family has no dropout and no slot to fill).
    The wrappers are this module's attributes at the time of the call: tests put spies there."""
    if kind == "long":
        return long_attention(q, k, v, num_heads, key_mask, causal, scale=scale, bias=bias)
    fn = {"short": short_attention, "long_train": long_attention_train}[kind]
    return fn(q, k, v, num_heads, key_mask, causal, p, training, scale=scale, bias=bias, k_slot=k_slot)


def attend_qkv(kind, qkv, num_heads, key_mask=None, causal=False, p=0.0, training=False, scale=None, bias=None):
    """one fused ``qkv [B, L, 3E]`` on family ``kind``; arguments as in ``short_self_attention``"""
    if kind == "long":
        return long_self_attention(qkv, num_heads, key_mask, causal, scale=scale, bias=bias)
    fn = {"short": short_self_attention, "long_train": long_self_attention_train}[kind]
    return fn(qkv, num_heads, key_mask, causal, p, training, scale=scale, bias=bias)
