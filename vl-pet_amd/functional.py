"""torch.autograd glue over the C ABI (device memory, streams and autograd only -- the
arithmetic lives in csrc/).  Every function here requires CUDA(ROCm) tensors and raises if the
HIP library is unavailable; there is deliberately no eager fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib

GATE_NONE, GATE_MUL, GATE_ADD = _lib.GATE_NONE, _lib.GATE_MUL, _lib.GATE_ADD


class KernelTimer:
    """Optional HIP-event bracketing of individual launches (bench.py's live roofline measurement).
    Events are recorded on the stream the kernels are enqueued on (torch's current stream)."""

    def __init__(self, names=None):
        self.records = []      # (name, rows, start_event, end_event)
        self.names = None if names is None else frozenset(names)     # bracket only these launch groups (None: all)

    def wants(self, name):
        return self.names is None or name in self.names

    def bracket(self, name, rows, fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.records.append((name, rows, e0, e1))
        return out

    def summary(self):
        """name -> dict(launches, rows, total_us, by_rows = {rows of a launch: [launches, total_us]}); call after torch.cuda.synchronize()."""
        agg = {}
        for name, rows, e0, e1 in self.records:
            a = agg.setdefault(name, dict(launches=0, rows=0, total_us=0.0, by_rows={}))
            us = e0.elapsed_time(e1) * 1e3
            a["launches"] += 1
            a["rows"] += rows
            a["total_us"] += us
            b = a["by_rows"].setdefault(int(rows), [0, 0.0])
            b[0] += 1
            b[1] += us
        return agg


TIMER: Optional[KernelTimer] = None

# Optional side stream for the weight-gradient half of the K1 backward (train.Trainer(overlap_wgrad=True); OFF by
# default: on one MI355X the step is GPU-bound and the overlap measured 5 % slower, 15.2 k vs 16.0 k samples/s).
# The row-parallel half stays
# on the autograd stream -- the next backward op needs dx1 / dx2 -- while the column-parallel weight gradients, which
# nobody reads before the optimizer step, run concurrently with the frozen backward that follows.  Only used when
# every weight gradient of the call goes straight into the trainer's flat buffer (train.GradSink).
WGRAD_STREAM: Optional["torch.cuda.Stream"] = None


# Deferred reductions of parameter gradients (bias column sums, LayerNorm dgamma / dbeta): a trainer sets DEFER_REDUCES for its
# backward and calls flush_reduces() once after it -- one batched launch (vlpet_reduce_batch) instead of one 5.6-us launch per
# parameter (127 per step in the LoRA runs, which train every bias).  Only gradients written straight into the trainer's flat buffer
# are deferred (train.GradSink: nobody reads them before the optimizer); with bucketed all-reduces running from inside the backward the
# trainer leaves the switch off.
DEFER_REDUCES = False
_PENDING_REDUCES: list = []


def discard_pending():
    """Error path of a trainer's backward: nothing queued survives the step."""
    _PENDING_REDUCES.clear()


def reduce_partials(part: torch.Tensor, nb: int, d: int, out0: Optional[torch.Tensor], out1: Optional[torch.Tensor], deferrable: bool):
    """``part`` viewed as [nb][2 d] -> out0 [d], out1 [d] (fp32, overwritten; either may be None): now, or at flush_reduces()."""
    if DEFER_REDUCES and deferrable:
        _PENDING_REDUCES.append((part, int(nb), int(d), out0, out1))
        return
    rc = _lib.load().vlpet_sublayer_tail_reduce(part.data_ptr(), int(nb), int(d), _ptr(out0), _ptr(out1), _stream())
    _lib.check(rc, "vlpet_sublayer_tail_reduce")


def flush_reduces():
    if not _PENDING_REDUCES:
        return 0
    jobs, n = list(_PENDING_REDUCES), len(_PENDING_REDUCES)
    _PENDING_REDUCES.clear()
    vp, ip = ctypes.c_void_p * n, ctypes.c_int * n
    rc = _lib.load().vlpet_reduce_batch(vp(*[j[0].data_ptr() for j in jobs]), vp(*[_ptr(j[3]) for j in jobs]), vp(*[_ptr(j[4]) for j in jobs]),
                                        ip(*[j[1] for j in jobs]), ip(*[j[2] for j in jobs]), n, _stream())
    _lib.check(rc, "vlpet_reduce_batch")
    return n


def _timed(name, rows, fn):
    if TIMER is None or not TIMER.wants(name):
        return fn()
    return TIMER.bracket(name, rows, fn)


def _io_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _lib.VLPET_BF16
    if t.dtype == torch.float32:
        return _lib.VLPET_F32
    raise RuntimeError(f"vl-pet_amd: unsupported activation dtype {t.dtype} (bf16 or fp32)")


def _param_dtype(t: torch.Tensor) -> int:
    return _io_dtype(t)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vl-pet_amd: the PET hot path runs on the GPU only (got a CPU tensor)")


def rank_tiles(r: int) -> int:
    t = _lib.load().vlpet_rank_tiles(int(r))
    if t < 0:
        _lib.check(t, f"rank_tiles({r})")
    return t


class PackedPair:
    """MFMA-fragment pack of one (down, up) projection pair (see tests/packing_spec.py / csrc/pack.hip)."""

    __slots__ = ("buf", "tiles", "r", "d", "io_dtype")

    def __init__(self, buf, tiles, r, d, io_dtype):
        self.buf, self.tiles, self.r, self.d, self.io_dtype = buf, tiles, r, d, io_dtype


def pack_pair(down_w: Sequence[torch.Tensor], down_b: Optional[Sequence[torch.Tensor]],
              up_w: torch.Tensor, up_b: Optional[torch.Tensor], io_dtype: int,
              tiles: Optional[int] = None, out: Optional["PackedPair"] = None) -> PackedPair:
    """``out``: an earlier pack of the same geometry to refresh IN PLACE (its buffer may be baked into a captured graph: a cache that
    answered a miss with a new buffer would leave the graph reading the old one -- or freed memory)."""
    lib = _lib.load()
    _need_cuda(up_w, *down_w)
    n = len(down_w)
    rh, d = down_w[0].shape
    r = rh * n
    if tuple(up_w.shape) != (d, r):
        raise RuntimeError(f"vl-pet_amd: up weight {tuple(up_w.shape)} does not match down {r}x{d}")
    if tiles is None:
        tiles = rank_tiles(r)
    ws = [w.detach().contiguous() for w in down_w]
    bs = [b.detach().contiguous() for b in down_b] if down_b is not None else None
    uw = up_w.detach().contiguous()
    ub = up_b.detach().contiguous() if up_b is not None else None
    pd = _param_dtype(uw)
    for t in ws + (bs or []) + ([ub] if ub is not None else []):
        if _param_dtype(t) != pd:
            raise RuntimeError("vl-pet_amd: mixed parameter dtypes in one projection pair")
    nbytes = lib.vlpet_packed_bytes(tiles, d, io_dtype)
    if (out is not None and out.buf.numel() == nbytes and out.buf.device == uw.device and out.tiles == tiles and out.r == r
            and out.d == d and out.io_dtype == io_dtype):
        buf = out.buf
    else:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=uw.device)
    arr_w = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    arr_b = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bs]) if bs is not None else None
    rc = lib.vlpet_pack_pair(arr_w, arr_b, n, uw.data_ptr(), _ptr(ub), r, d, tiles, pd, io_dtype,
                             buf.data_ptr(), _stream())
    _lib.check(rc, "vlpet_pack_pair")
    return PackedPair(buf, tiles, r, d, io_dtype)


# keep the gated forward's bottleneck activations for the backward (vlpet_adapter_gate_fwd_save / _bwd_saved); False = the
# backward recomputes them from x1, x2 (no extra memory between forward and backward)
SAVE_ACTIVATIONS = True
# A/B switch for benches and tests: True = the round-2 split of the gated K1 backward (row kernel that also writes dh / dq +
# streaming weight-gradient kernel, ABI phases bit 2) instead of pass 1 + the column-parallel pass
K1_BWD_PREVIOUS_SPLIT = False
# round 5: the multiplicative gate's backward starts from the forward's OUTPUT y = gs * h * g when the forward saved its
# activations: dq = dy * y * (1 - g), so pass 1 recomputes the gate's up projection only (vlpet_adapter_gate_bwd_saved_y).
# False = from x2 (recompute h = s2 * x2 + sd * up_A(z_a)), the rounds 2-4 form.
K1_BWD_FROM_OUTPUT = True
# round 6: pass 2 of the gated K1 backward (r <= 96) sums its row-chunk partials inside the launch (csrc/cols_reduce.h).  True = the
# round-3 form (partial slabs + a finalize launch, ABI phases bit 5), read per call; the results are bit-identical.  Set it where
# other kernels run beside the backward: train.Trainer does so around a backward that overlaps gradient collectives or the side-stream
# weight gradients.
K1_BWD_FINALIZE_LAUNCH = False

# Bumped by optimizers that update parameters behind autograd's back (the fused flat-buffer AdamW writes through
# raw pointers, which does not touch ``Tensor._version``); part of every pack-cache key.
WEIGHTS_EPOCH = 0
# Part of the keys of the derived copies of FROZEN tensors (fused q|k|v weight, padded LM head, fp32 LayerNorm copies, the
# logits-bias flag).  Those keys also carry (data_ptr, Tensor._version), but ``p.data`` has its own version counter: in-place
# edits through ``.data`` (``m.weight.data.normal_()``, ``p.data.copy_()`` in hand-written checkpoint loaders) or through raw
# pointers are invisible to them.  ``invalidate_caches()`` is the explicit way out; the hosts call it from a
# ``load_state_dict`` post-hook.  (Not bumped by optimizer steps: frozen tensors do not change there.)
FROZEN_EPOCH = 0


def bump_weights_epoch():
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


def invalidate_caches():
    """Drop every derived copy of a parameter (weight packs and the caches of frozen tensors): call after changing weights in
    a way autograd's version counters do not see (``.data`` edits, raw-pointer writes, custom checkpoint loaders)."""
    global FROZEN_EPOCH
    FROZEN_EPOCH += 1
    bump_weights_epoch()


_PACK_CACHES = None       # weak set of the PackCache objects that packed parameters directly (see repack_all)


class PackCache:
    """Re-pack only when a parameter changed (optimizer steps bump ``Tensor._version`` or ``WEIGHTS_EPOCH``)."""

    def __init__(self):
        self._key = None
        self._val = None
        self._src = None      # (down_w, down_b, up_w, up_b, io_dtype, tiles, epoch of last use): what repack_all re-packs

    @staticmethod
    def _make_key(down_w, down_b, up_w, up_b, io_dtype, tiles):
        ts = list(down_w) + (list(down_b) if down_b is not None else []) + [up_w] + ([up_b] if up_b is not None else [])
        return (io_dtype, tiles, WEIGHTS_EPOCH) + tuple((t.data_ptr(), t._version) for t in ts)

    def get(self, down_w, down_b, up_w, up_b, io_dtype, tiles=None) -> PackedPair:
        key = self._make_key(down_w, down_b, up_w, up_b, io_dtype, tiles)
        if key != self._key:
            self._val = pack_pair(down_w, down_b, up_w, up_b, io_dtype, tiles, out=self._val)
            self._key = key
        global _PACK_CACHES
        if _PACK_CACHES is None:
            import weakref
            _PACK_CACHES = weakref.WeakSet()
        _PACK_CACHES.add(self)
        self._src = (list(down_w), list(down_b) if down_b is not None else None, up_w, up_b, io_dtype, tiles, WEIGHTS_EPOCH)
        return self._val

    def get_derived(self, sources, tag, build, io_dtype, tiles=None) -> PackedPair:
        """Pack of tensors DERIVED from parameters (slices, concatenations, ``.contiguous()`` copies): the key is made from
        the source parameters (+ ``tag``, the derivation's geometry), never from the temporaries -- their ``_version`` is
        always 0 and their address is whatever the caching allocator hands out -- and ``build()`` -> (down_w, down_b,
        up_w, up_b) runs only on a miss."""
        key = (io_dtype, tiles, WEIGHTS_EPOCH, tag) + tuple((t.data_ptr(), t._version) for t in sources)
        if key != self._key:
            self._val = pack_pair(*build(), io_dtype, tiles, out=self._val)
            self._key = key
        return self._val


def repack_all(every_pair: bool = False) -> int:
    """Re-pack, in a few batched launches (vlpet_pack_pairs: 8 pairs each), every projection pair that was used since the
    previous call -- what a trainer does right after its optimizer step, instead of ~30 single 7.6-us pack launches spread over
    the next forward.  Pairs are re-packed INTO their existing buffers and their cache keys moved to the current weights
    epoch, so the next ``PackCache.get`` is a hit; anything that does not fit (contiguity, mixed dtypes, a parameter that
    was replaced) is simply left to the lazy path.  Returns the number of pairs packed."""
    if not _PACK_CACHES:
        return 0
    lib = _lib.load()
    groups = {}
    for c in list(_PACK_CACHES):
        src, val = c._src, c._val
        if src is None or val is None:
            continue
        down_w, down_b, up_w, up_b, io_dtype, tiles, used = src
        if used < WEIGHTS_EPOCH - 1 and not every_pair:   # not used in the step that just ended: leave it to the lazy path
            continue                                      # (every_pair: a trainer replaying captured steps runs no Python forward)
        ts = down_w + (down_b or []) + [up_w] + ([up_b] if up_b is not None else [])
        if not all(t.is_cuda and t.is_contiguous() for t in ts) or len({t.dtype for t in ts}) != 1:
            continue
        n, (rh, d) = len(down_w), down_w[0].shape
        if tuple(up_w.shape) != (d, rh * n) or val.d != d or val.tiles != (tiles if tiles is not None else val.tiles):
            continue
        g = (n, rh * n, d, val.tiles, _param_dtype(up_w), io_dtype, down_b is not None, up_b is not None, up_w.device)
        groups.setdefault(g, []).append(c)
    done = 0
    for (n, r, d, tiles, pd, io_dtype, has_bd, has_bu, dev), caches in groups.items():
        k = len(caches)
        wd = (ctypes.c_void_p * (k * n))(*[w.data_ptr() for c in caches for w in c._src[0]])
        bd = (ctypes.c_void_p * (k * n))(*[b.data_ptr() for c in caches for b in c._src[1]]) if has_bd else None
        wu = (ctypes.c_void_p * k)(*[c._src[2].data_ptr() for c in caches])
        bu = (ctypes.c_void_p * k)(*[c._src[3].data_ptr() for c in caches]) if has_bu else None
        out = (ctypes.c_void_p * k)(*[c._val.buf.data_ptr() for c in caches])
        with torch.cuda.device(dev):
            rc = lib.vlpet_pack_pairs(k, wd, bd, n, wu, bu, r, d, tiles, pd, io_dtype, out, _stream())
        _lib.check(rc, "vlpet_pack_pairs")
        for c in caches:
            down_w, down_b, up_w, up_b, io, tl, _ = c._src
            c._key = PackCache._make_key(down_w, down_b, up_w, up_b, io, tl)
        done += k
    return done


def _flat(x: torch.Tensor, d: int) -> torch.Tensor:
    x = x.reshape(-1, d)
    return x if x.is_contiguous() else x.contiguous()


def _grad_like(g32: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    return g32 if p.dtype == torch.float32 else g32.to(p.dtype)


def _empty_result(x: torch.Tensor, params) -> torch.Tensor:
    """Zero-row input: nothing to launch.  The (empty) result stays connected to every parameter so that
    their gradients are zeros rather than None, like the reference's op chain on an empty batch."""
    out = x.clone()
    for p in params:
        if p is not None and p.requires_grad:
            out = out + (p.reshape(-1)[:1].sum() * 0).to(out.dtype)
    return out


class GradSlot:
    """Where one weight-gradient kernel writes and what autograd gets back for it.  ``t``: the fp32 tensor the kernel fills --
    the parameter's slot of the trainer's flat gradient buffer (``sunk``) or a fresh tensor.  ``finish()``, called once the
    launches are enqueued, tells a sink that its slot is written and returns ``None`` (no accumulate kernel runs), else returns
    the tensor in the parameter's dtype."""

    __slots__ = ("t", "_sink", "_p")

    def __init__(self, t, sink, p):
        self.t, self._sink, self._p = t, sink, p

    @staticmethod
    def scratch(shape, device) -> "GradSlot":
        """A destination nobody owns: the kernel needs somewhere to write, autograd gets nothing."""
        return GradSlot(torch.empty(*shape, dtype=torch.float32, device=device), None, None)

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    @property
    def sunk(self) -> bool:
        return self._sink is not None

    def finish(self):
        if self._sink is not None:
            self._sink.done()
            return None
        return None if self._p is None else _grad_like(self.t, self._p)

    def finish_heads(self, params):
        """The slot holds the row blocks of ``len(params)`` heads stacked (the multi-head down projection): one gradient per head."""
        if self._sink is not None:
            self._sink.done()
            return [None] * len(params)
        rh = self.t.shape[0] // len(params)
        return [_grad_like(self.t[i * rh:(i + 1) * rh], p) for i, p in enumerate(params)]


def grad_slot(p: torch.Tensor, shape, block: bool = False) -> GradSlot:
    """The slot for parameter ``p``: its part of the trainer's flat gradient buffer when that offers one for this step
    (train.GradSink: first write of the step, fp32, matching shape and device), else a fresh fp32 tensor.  ``block``: the
    sink that spans the stacked heads ``p`` is the first of."""
    sink = getattr(p, "_vlpet_block_sink" if block else "_vlpet_sink", None)
    if sink is not None and tuple(sink.view.shape) == tuple(shape) and sink.view.device == p.device:
        v = sink.take()
        if v is not None:
            return GradSlot(v, sink, p)
    return GradSlot(torch.empty(*shape, dtype=torch.float32, device=p.device), None, p)


class AdapterSlots:
    """The gradient slots of one adapter pair in the order of the kernels' eight gradient arguments: down weight and bias (the heads
    stacked, one block slot each), up weight and bias, then -- with ``rg`` -- the gate's four.  ``params``: N_h down weights, N_h down
    biases, up w, up b, [the gate's four].  ``d_in``: the down projections' input width (K1: d; the low-rank projector: feat_dim)."""

    __slots__ = ("slots",)

    def __init__(self, params, n_heads, r, rg, d, d_in=None):
        d_in, n = d if d_in is None else d_in, 2 * n_heads
        shapes = [(r, d_in), (r,), (d, r), (d,)] + ([(rg, d_in), (rg,), (d, rg), (d,)] if rg else [])
        owners = [params[0], params[n_heads]] + list(params[n:n + len(shapes) - 2])
        self.slots = [grad_slot(p, shape, block=i < 2) for i, (p, shape) in enumerate(zip(owners, shapes))]

    def ptrs(self):         # (NULL for the gate's four without a gate)
        return (*(s.ptr for s in self.slots), *((None,) * (8 - len(self.slots))))

    @property
    def all_sunk(self) -> bool:
        return all(s.sunk for s in self.slots)

    def finish(self, params, n_heads):      # one gradient per parameter (see GradSlot.finish)
        return (self.slots[0].finish_heads(params[:n_heads]) + self.slots[1].finish_heads(params[n_heads:2 * n_heads])
                + [s.finish() for s in self.slots[2:]])


FANOUT_SUM = True          # A/B switch (tools/ab_switches.py: VLPET_NO_FANOUT_SUM=1): fanout() below


class _FanoutFn(torch.autograd.Function):
    """``n`` aliases of one tensor for ``n`` consumers, so that their gradients arrive TOGETHER and are summed in one launch
    (vlpet_sum_n: n + 1 row units, fp32 accumulation, one rounding) instead of autograd's pairwise accumulation (n - 1 passes of three
    units, a bf16 rounding each).  The encoder output under the decoder layers' cross-attention is the case
    (my_transformers/modeling_bart.py:2300-2330: every layer takes encoder_hidden_states)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [g for g in gs if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        g0 = live[0]
        same = all(g.dtype == g0.dtype and g.shape == g0.shape and g.is_contiguous() for g in live)
        if not (same and g0.is_cuda and g0.dtype in (torch.bfloat16, torch.float32) and g0.numel() % 8 == 0 and g0.numel() > 0):
            total = live[0]
            for g in live[1:]:
                total = total + g
            return total, None
        import ctypes
        lib = _lib.load()
        out = torch.empty_like(g0)
        arr = (ctypes.c_void_p * len(live))(*[g.data_ptr() for g in live])
        rc = _timed("fanout_sum", g0.numel() // g0.shape[-1], lambda: lib.vlpet_sum_n(arr, len(live), out.data_ptr(), g0.numel(), _io_dtype(g0), _stream()))
        _lib.check(rc, "vlpet_sum_n")
        return out, None


def fanout(x: torch.Tensor, n: int):
    """``n`` references to ``x`` for ``n`` consumers; on the GPU with gradients on, aliases whose gradients are summed in one launch."""
    if n <= 1 or not FANOUT_SUM or not x.is_cuda or not (x.requires_grad and torch.is_grad_enabled()):
        return (x,) * max(1, n)
    return _FanoutFn.apply(x, n)


class _CrossKeyProjFn(torch.autograd.Function):
    """``n`` frozen projections of ONE input as ONE GEMM: ``x [.., E] -> [.., n * E]``, handed out as its n column blocks (views).  The
    decoder layers' cross-attention key projections of the encoder output (my_transformers/modeling_bart.py:2300-2330 hands every layer
    the same encoder_hidden_states; each layer's ``encoder_attn.k_proj`` projects it, :425) -- n small GEMMs that all read x, and in
    the backward n dgrad GEMMs that all accumulate into d/dx.  Here: one GEMM forward; backward, the attention calls write their dk
    into the blocks of one gradient buffer (attention.KeyGradSlot) and ONE GEMM with K = n * E produces d/dx."""

    @staticmethod
    def forward(ctx, x, w_all, b_all, n, slot, *biases):
        # ``biases``: the layers' k_proj.bias parameters where any of them trains (BitFit), else nothing; b_all is their current fused copy
        y = F.linear(x, w_all, b_all)
        E = w_all.shape[0] // n
        ctx.save_for_backward(w_all, *biases)
        ctx.slot, ctx.n, ctx.xshape = slot, n, x.shape
        return tuple(y[..., i * E:(i + 1) * E] for i in range(n))

    @staticmethod
    def backward(ctx, *dks):
        w_all, *biases = ctx.saved_tensors
        n, slot = ctx.n, ctx.slot
        ctx.slot = None
        E = w_all.shape[0] // n
        buf = slot.buf if slot is not None else None
        if slot is not None:
            slot.buf = None
        whole = buf is not None and all(
            dk is not None and dk.data_ptr() == buf.data_ptr() + i * E * buf.element_size() and dk.shape[:-1] == buf.shape[:-1]
            and dk.stride() == buf.stride() for i, dk in enumerate(dks))
        bslots = [grad_slot(b, (E,)) if (ctx.needs_input_grad[5 + i] and dks[i] is not None) else None for i, b in enumerate(biases)]
        if whole:
            dx = buf.view(-1, n * E) @ w_all
            if any(sl is not None for sl in bslots):        # every layer's k_proj.bias gradient: ONE segmented sum over the shared dk buffer
                full = buf.view(-1, n * E)                  # (more layers than one call takes segments: 16 at a time)
                for s0 in range(0, n, MAX_COLSUM_SEGS):
                    part = bslots[s0:s0 + MAX_COLSUM_SEGS]
                    if any(sl is not None for sl in part):
                        colsum_seg_into(full[:, s0 * E:(s0 + len(part)) * E], part, E)
        else:                       # (a consumer that went another way: per-block products)
            dx = None
            for i, dk in enumerate(dks):
                if dk is None:
                    continue
                d2 = dk.reshape(-1, E).to(w_all.dtype)
                t = d2 @ w_all[i * E:(i + 1) * E]
                dx = t if dx is None else dx.add_(t)
                if biases and bslots[i] is not None:
                    BITFIT_CALLS["fallback"] += 1
                    colsum_seg_into(d2, [bslots[i]], E)
        return ((None if dx is None else dx.view(ctx.xshape)), None, None, None, None) + tuple(None if sl is None else sl.finish() for sl in bslots)


def cross_key_blocks(x: torch.Tensor, w_all: torch.Tensor, b_all: torch.Tensor, n: int, biases=()):
    """(k_0 .. k_{n-1}, slot): the n key projections of ``x`` as column blocks of one GEMM's output and the KeyGradSlot their attention
    calls pass on (``short_attention(..., k_slot=(slot, i))``).  ``biases``: the n bias parameters when any of them trains (BitFit) --
    their gradients are one segmented column sum over the shared dk buffer."""
    from .attention import KeyGradSlot
    biases = tuple(biases) if (torch.is_grad_enabled() and any(b is not None and b.requires_grad for b in biases)) else ()
    slot = KeyGradSlot(n, w_all.shape[0] // n) if ((x.requires_grad or biases) and torch.is_grad_enabled()) else None
    return _CrossKeyProjFn.apply(x, w_all, b_all, n, slot, *biases), slot


class ResidualLink:
    """Hand-over of an input gradient between two ops that read the same tensor x, one of them downstream of the other's
    output.  Autograd would sum their two contributions to d/dx with a separate elementwise pass over [M, d].  With a link
    the upstream op arms it in its forward; the downstream op, whose backward runs first, parks its d/dx (whatever it is the
    gradient of: the tail's residual add, K1's gate, K2, K3, or a sum that already holds an earlier hand-over) and returns
    no gradient for x; the upstream op's backward takes it, adds its own inside its kernel or GEMM epilogue and returns the
    sum.  The first pair was the sublayer tail LayerNorm(x1 + dropout(y)) and the gate of K1
    (my_transformers/modeling_bart.py:1196, 1259-1261; vlpet_adapter_gate_bwd_saved_acc); DESIGN.md lists them all.
    An op arms only when its backward will take the hand-over, and parks only in an armed link."""

    __slots__ = ("armed", "_grad", "_shared")

    def __init__(self):
        self.armed = False
        self._grad = None
        self._shared = False       # the parked tensor is also somebody else's gradient: nobody may write into it

    def arm(self) -> "ResidualLink":
        self.armed = True
        return self

    @staticmethod
    def if_armed(link: Optional["ResidualLink"]) -> Optional["ResidualLink"]:
        """``link`` where a producer may park in it, else None."""
        return link if (link is not None and link.armed) else None

    @property
    def holds(self) -> bool:
        return self._grad is not None

    def park(self, grad: torch.Tensor, shared: bool = False):
        """``shared``: ``grad`` is also handed to somebody else (autograd's own tensor, or returned for another input)."""
        if self._grad is not None:
            raise RuntimeError("vl-pet_amd: a gradient is already parked in this ResidualLink (it would be lost)")
        self._grad, self._shared = grad, bool(shared)

    def take(self, shape, dtype, writable: bool = False) -> Optional[torch.Tensor]:
        """The parked gradient as a contiguous ``shape`` / ``dtype`` tensor (None if nothing was parked); the link is empty
        afterwards.  ``writable``: the caller accumulates into the result in place, so a shared tensor comes back as a copy."""
        g, shared = self._grad, self._shared
        self._grad, self._shared = None, False
        if g is None:
            return None
        parked = g
        if g.shape != shape:
            g = g.reshape(shape)
        if g.dtype != dtype:
            g = g.to(dtype)
        if not g.is_contiguous():
            g = g.contiguous()
        if writable and shared and g.data_ptr() == parked.data_ptr():      # (a repair above already made a private copy)
            g = g.clone()
        return g


class _LinearAccFn(torch.autograd.Function):
    """``n`` frozen projections of ONE input (``x -> x W_i^T + b_i``) whose input gradient starts from a parked one.

    The input of a sublayer's first GEMM is read by a second op further down (the gate of K1, the sublayer tail's
    residual add, the value-parallel adapter of K2: my_transformers/modeling_bart.py:1147-1155, 1259-1261, 427-430), and
    autograd sums the two input gradients with an elementwise pass over ``[M, d]``.  That other op is downstream of this
    GEMM's output, so its backward always runs first: it parks its gradient in the ``ResidualLink`` this forward armed and
    returns none, and the dgrad GEMM here accumulates onto it (``C += dY W``, beta = 1 in the library GEMM's epilogue) --
    one gradient for x, no add kernel.  Weights and biases are frozen (no gradient is produced for them)."""

    @staticmethod
    def forward(ctx, x, link, *wb):
        n = len(wb) // 2
        ws, bs = wb[:n], wb[n:]
        ctx.link = link.arm() if (link is not None and ctx.needs_input_grad[0]) else None
        ctx.save_for_backward(*ws)
        ctx.xshape = x.shape
        outs = tuple(F.linear(x, w, b) for w, b in zip(ws, bs))
        return outs if n > 1 else outs[0]

    @staticmethod
    def backward(ctx, *dys):
        ws = ctx.saved_tensors
        link, ctx.link = ctx.link, None
        acc = link.take(ctx.xshape, ws[0].dtype, writable=True) if link is not None else None
        if acc is not None:
            acc = acc.view(-1, ctx.xshape[-1])
        for dy, w in zip(dys, ws):
            if dy is None:
                continue
            dy2 = dy.reshape(-1, dy.shape[-1])
            if dy2.dtype != w.dtype:
                dy2 = dy2.to(w.dtype)
            if acc is None:
                acc = dy2 @ w
            else:
                acc.addmm_(dy2, w)
        dx = acc.view(ctx.xshape) if acc is not None else None
        return (dx, None) + (None,) * (2 * len(ws))


def io_view(p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``p`` in the activation dtype: the parameter's slice of its trainer's IO-dtype shadow buffer when that is current
    (train.FlatGrads.refresh_io_shadow: one cast launch per optimizer step for all trainable parameters), else a cast."""
    if p.dtype == dtype:
        return p
    sh = getattr(p, "_vlpet_io", None)
    if sh is not None and sh[0].io_epoch == WEIGHTS_EPOCH and sh[1].dtype == dtype:
        return sh[1]
    return p.to(dtype)


class _LinearTrainBiasFn(torch.autograd.Function):
    """``x W^T + b`` with a FROZEN weight and a TRAINABLE bias (the reference's LoRA runs unfreeze every bias next to the frozen
    projections): the bias gradient = column sums of dy through vlpet_colsum (two HIP launches, fp32, straight into the
    parameter's slot of the flat gradient buffer when the trainer offers one) instead of autograd's bf16 ``sum(0)`` + cast +
    accumulate."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        # (K3's delta on this projection -- same x, downstream of this output -- parks its d/dx)
        ctx.link = link.arm() if (link is not None and ctx.needs_input_grad[0]) else None
        ctx.save_for_backward(w, b)
        return F.linear(x, w, io_view(b, x.dtype))

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        w, b = ctx.saved_tensors
        n = dy.shape[-1]
        dy2 = _flat(dy, n)
        if dy2.dtype != w.dtype:
            dy2 = dy2.to(w.dtype)
        dx = None
        link, ctx.link = ctx.link, None
        if ctx.needs_input_grad[0]:
            xshape = (*dy.shape[:-1], w.shape[1])
            base = link.take(xshape, w.dtype, writable=True) if link is not None else None
            if base is not None:
                dx = base.view(-1, w.shape[1]).addmm_(dy2, w).view(xshape)      # C += dY W in the GEMM epilogue
            else:
                dx = (dy2 @ w).view(xshape)
        db = None
        if ctx.needs_input_grad[2]:
            M = dy2.shape[0]
            slot = grad_slot(b, (n,))
            nb = lib.vlpet_sublayer_tail_partials(M)
            ws = torch.empty(nb * n, dtype=torch.float32, device=dy2.device)
            if DEFER_REDUCES and slot.sunk:       # pass 1 now, the reduction with the step's other ones (flush_reduces)
                rc = lib.vlpet_colsum_partial(dy2.data_ptr(), M, n, ws.data_ptr(), _io_dtype(dy2), _stream())
                _lib.check(rc, "vlpet_colsum_partial")
                tf = slot.t.reshape(-1)
                reduce_partials(ws, nb, n // 2, tf[:n // 2], tf[n // 2:], True)
            else:
                rc = lib.vlpet_colsum(dy2.data_ptr(), M, n, ws.data_ptr(), slot.ptr, _io_dtype(dy2), _stream())
                _lib.check(rc, "vlpet_colsum")
            db = slot.finish()
        return dx, None, db, None


def linear_train_bias_ok(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> bool:
    """Whether ``linear_train_bias`` applies: CUDA bf16 / fp32 activations, frozen weight in that dtype, trainable bias."""
    return (b is not None and b.requires_grad and not w.requires_grad and x.is_cuda and w.dtype == x.dtype
            and x.dtype in (torch.bfloat16, torch.float32) and w.shape[0] % 16 == 0 and w.shape[0] <= (4096 if x.dtype == torch.bfloat16 else 2048)
            and x.numel() > 0 and torch.is_grad_enabled())


def linear_train_bias(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, link: Optional["ResidualLink"] = None) -> torch.Tensor:
    """``link``: shared with the K3 delta applied on top of this projection (lora_delta(..., link=link))."""
    return _LinearTrainBiasFn.apply(x, w, b, link)


def linear_acc(x: torch.Tensor, link: Optional[ResidualLink], *mods):
    """``F.linear`` of ``x`` through each of ``mods`` (``nn.Linear``-like, or ``(weight, bias)`` pairs), frozen, with the
    input gradient accumulated onto whatever the op sharing ``link`` parks (see _LinearAccFn).  One result per module."""
    ws, bs = [], []
    for m in mods:
        w, b = (m.weight, m.bias) if hasattr(m, "weight") else m
        if w.requires_grad or (b is not None and b.requires_grad):
            raise RuntimeError("vl-pet_amd: linear_acc is for frozen projections")
        ws.append(w if w.dtype == x.dtype else w.to(x.dtype))
        bs.append(b if b is None or b.dtype == x.dtype else b.to(x.dtype))
    return _LinearAccFn.apply(x, link, *ws, *bs)


# ---- BitFit: bias gradients produced where the data already is (csrc/biasgrad.hip) ------------------------------------------------
# A/B switch (tools/ab_switches.py: VLPET_NO_BIAS_GRAD_SITES=1): False = a model with trainable biases next to frozen projections takes
# the separate-projection path with one vlpet_colsum pair per bias (linear_train_bias), as a hand-unfrozen model did before these sites.
FUSE_BIAS_GRAD_SITES = True
# launches issued (tests assert on them; a replayed graph does not count): segmented column sums, fused activation backwards, and
# calls that wanted a site but had to take linear_train_bias / act_dropout instead
BITFIT_CALLS = {"seg": 0, "act": 0, "fallback": 0}
MAX_COLSUM_SEGS = 16       # segments of one vlpet_colsum_seg call (include/vlpet_hip.h)


def colsum_seg_into(dy2: torch.Tensor, slots, w: int):
    """Column sums of ``dy2 [M, len(slots) * w]`` (any row stride), segment s into ``slots[s].t`` (a GradSlot, or None: not wanted):
    one vlpet_colsum_seg call.  Not deferred (DEFER_REDUCES is bypassed: the call's second launch writes every wanted slot at once,
    there is no per-parameter reduction left to batch)."""
    import ctypes
    lib = _lib.load()
    S, (M, n) = len(slots), dy2.shape
    if dy2.stride(1) != 1:
        dy2 = dy2.contiguous()
    nbytes = lib.vlpet_colsum_seg_workspace_bytes(M, n)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dy2.device)
    ptrs = (ctypes.c_void_p * S)(*[None if sl is None else sl.ptr for sl in slots])
    rc = _timed("colsum_seg", M, lambda: lib.vlpet_colsum_seg(dy2.data_ptr(), M, S, w, dy2.stride(0), ptrs, ws.data_ptr(), nbytes,
                                                              _io_dtype(dy2), _stream()))
    _lib.check(rc, "vlpet_colsum_seg")
    BITFIT_CALLS["seg"] += 1


class _LinearAccBiasFn(torch.autograd.Function):
    """_LinearAccFn for ONE fused GEMM of n projections (``w_all [n E, in]``, frozen) whose biases may train: ``biases`` are the n
    modules' bias parameters, ``b_all`` their concatenation in the activation dtype.  The input gradient accumulates onto the parked one
    exactly as in _LinearAccFn; the gradients of the trainable biases are one segmented column sum of the fused dy, each segment
    straight into its bias's slot (GradSlot.finish as in _LinearTrainBiasFn); a frozen bias is a NULL segment."""

    @staticmethod
    def forward(ctx, x, link, w_all, b_all, *biases):
        ctx.link = link.arm() if (link is not None and ctx.needs_input_grad[0]) else None
        ctx.save_for_backward(w_all, *biases)
        ctx.xshape = x.shape
        return F.linear(x, w_all, b_all)

    @staticmethod
    def backward(ctx, dy):
        w_all, *biases = ctx.saved_tensors
        link, ctx.link = ctx.link, None
        n = dy.shape[-1]
        dy2 = _flat(dy, n)
        if dy2.dtype != w_all.dtype:
            dy2 = dy2.to(w_all.dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            acc = link.take(ctx.xshape, w_all.dtype, writable=True) if link is not None else None
            dx = (dy2 @ w_all if acc is None else acc.view(-1, ctx.xshape[-1]).addmm_(dy2, w_all)).view(ctx.xshape)
        w = n // len(biases)
        slots = [grad_slot(b, (w,)) if ctx.needs_input_grad[4 + i] else None for i, b in enumerate(biases)]
        if any(sl is not None for sl in slots):
            colsum_seg_into(dy2, slots, w)
        return (dx, None, None, None) + tuple(None if sl is None else sl.finish() for sl in slots)


class _LinearAccSepBiasFn(torch.autograd.Function):
    """_LinearAccFn (n SEPARATE GEMMs of one input, one input gradient on top of the parked one) whose biases may train: the consumers
    hand back n separate dy tensors, so each trainable bias gets the segmented sum of its own dy (one segment)."""

    @staticmethod
    def forward(ctx, x, link, n, *args):
        ws, bios, biases = args[:n], args[n:2 * n], args[2 * n:]
        ctx.link = link.arm() if (link is not None and ctx.needs_input_grad[0]) else None
        ctx.save_for_backward(*ws, *biases)
        ctx.xshape, ctx.n = x.shape, n
        outs = tuple(F.linear(x, w, b) for w, b in zip(ws, bios))
        return outs if n > 1 else outs[0]

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        ws, biases = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        link, ctx.link = ctx.link, None
        acc = link.take(ctx.xshape, ws[0].dtype, writable=True) if (link is not None and ctx.needs_input_grad[0]) else None
        if acc is not None:
            acc = acc.view(-1, ctx.xshape[-1])
        dbs = []
        for i, (dy, w, b) in enumerate(zip(dys, ws, biases)):
            if dy is None:
                dbs.append(None)
                continue
            dy2 = _flat(dy, dy.shape[-1])
            if dy2.dtype != w.dtype:
                dy2 = dy2.to(w.dtype)
            if ctx.needs_input_grad[0]:
                if acc is None:
                    acc = dy2 @ w
                else:
                    acc.addmm_(dy2, w)
            if ctx.needs_input_grad[3 + 2 * n + i]:
                sl = grad_slot(b, (dy2.shape[1],))
                colsum_seg_into(dy2, [sl], dy2.shape[1])
                dbs.append(sl.finish())
            else:
                dbs.append(None)
        dx = acc.view(ctx.xshape) if acc is not None else None
        return (dx, None, None) + (None,) * (2 * n) + tuple(dbs)


def linear_acc_sep_bias_ok(x: torch.Tensor, *mods) -> bool:
    return (FUSE_BIAS_GRAD_SITES and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.numel() > 0 and torch.is_grad_enabled()
            and all(m.bias is not None and not m.weight.requires_grad and m.weight.shape[0] % 16 == 0 and m.weight.shape[0] <= 65536
                    for m in mods) and any(m.bias.requires_grad for m in mods))


def linear_acc_sep_bias(x: torch.Tensor, link: Optional[ResidualLink], *mods):
    """linear_acc for ``nn.Linear`` modules with frozen weights and any subset of trainable biases (BitFit's cross-attention k | v)."""
    ws = [m.weight if m.weight.dtype == x.dtype else m.weight.to(x.dtype) for m in mods]
    bios = [io_view(m.bias, x.dtype).detach() for m in mods]
    return _LinearAccSepBiasFn.apply(x, link, len(mods), *ws, *bios, *[m.bias for m in mods])


def linear_acc_bias_ok(x: torch.Tensor, w_all: torch.Tensor, biases) -> bool:
    """Whether linear_acc_bias applies: the switch, CUDA bf16 / fp32 activations, the fused weight frozen and in that dtype, at most 16
    segments of a width that is a multiple of 16, at least one trainable bias."""
    n = len(biases)
    return (FUSE_BIAS_GRAD_SITES and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and w_all.dtype == x.dtype
            and not w_all.requires_grad and 1 <= n <= 16 and w_all.shape[0] % n == 0 and (w_all.shape[0] // n) % 16 == 0
            and w_all.shape[0] <= 65536 and all(b is not None for b in biases) and any(b.requires_grad for b in biases)
            and x.numel() > 0 and torch.is_grad_enabled())


def linear_acc_bias(x: torch.Tensor, link: Optional[ResidualLink], w_all: torch.Tensor, b_all: torch.Tensor, biases) -> torch.Tensor:
    """``x w_all^T + b_all`` as ONE GEMM (the fused output; the caller slices its column blocks).  ``b_all``: the concatenation of
    ``biases`` in the activation dtype, CURRENT -- host.common.derived_weights keys it on WEIGHTS_EPOCH while a bias trains, so it is
    rebuilt after every optimizer step and, inside a captured step, by a node of the graph."""
    return _LinearAccBiasFn.apply(x, link, w_all, b_all, *biases)


def _saved_block(ctx, nbytes, device):
    """Training (SAVE_ACTIVATIONS, read per call): a fresh block of ``nbytes()`` in which the forward of K1 / K2 / K3 leaves z and
    gelu'(pre) of its chains (up to 4 x [M, 32*tiles], IO dtype), so that the backward neither recomputes the down projections nor
    reads their inputs for them.  Kept in ``ctx.act`` until the backward; None otherwise."""
    ctx.act = torch.empty(nbytes(), dtype=torch.uint8, device=device) if (SAVE_ACTIVATIONS and any(ctx.needs_input_grad)) else None
    return ctx.act


def _block_call(entry, suffix, block, timer, M, head, tail):
    """One launch of K1 / K2 / K3: with the saved block, ``entry + suffix`` and the block between ``head`` and ``tail``; else ``entry``."""
    fn = getattr(_lib.load(), entry if block is None else entry + suffix)
    args = (*head, *tail) if block is None else (*head, block.data_ptr(), *tail)
    _lib.check(_timed(timer, M, lambda: fn(*args, _stream())), entry)


def _bwd_workspace(lib, M, d, tiles, gate, io, device):
    nws = lib.vlpet_bwd_workspace_bytes(M, d, tiles, int(gate), io)
    return torch.empty(nws, dtype=torch.uint8, device=device), nws


def _park_or_return(ctx, attr, g):
    """The ending of a backward whose d/dx may be handed over: into the armed link ``ctx.<attr>`` (autograd gets None) or back."""
    link = getattr(ctx, attr)
    setattr(ctx, attr, None)
    if link is None:
        return g
    link.park(g)
    return None


def k1_bwd_schedule(gate: bool, saved: bool, side: bool, previous_split: bool, bracketed: bool, form: int, finalize_due: bool):
    """The calls of one K1 backward, in order: [(timer name or None, ``phases`` bits, on the side stream)].  ``side``: the weight
    gradients go to WGRAD_STREAM; ``bracketed``: the timer wants ``k1_bwd_rows``; ``form``: vlpet_adapter_gate_bwd_form's answer;
    ``finalize_due``: pass 2 ends in a finalize launch.  The split forms (bit 2: the first half already delivers dx1 / dx2 -- the
    two-pass form produces them in its second) come first, and a timer brackets the half whose name it wants.  Else the op is one
    call, or -- bracketed -- the same work with its kernels bracketed separately, EVERY step once ``k1_bwd_rows`` is wanted (bit 3:
    pass 2 leaves its partial sums, bit 4: the finalize launch alone).  Bit 5 (K1_BWD_FINALIZE_LAUNCH) is the caller's."""
    rows, wgrad = "k1_bwd_rows", "k1_bwd_wgrad"
    if side or previous_split:
        return [(rows, 1 | 4, False), (wgrad, 2 | 4, bool(side))]
    if not bracketed:
        return [(None, 3, False)]
    if not gate:
        # adapter-only K1 (small / middle gate scripts): its two-pass form is taken for the WHOLE op only (csrc/api.hip bwd_plan: ROWS_NG), so the
        # bracketed path issues it as one call too -- split phases would time the round-2 row kernel instead of what ships
        return [(rows, 3, False)]
    if not (saved and form == 2):
        return [(rows, 1, False), (wgrad, 2, False)]
    return [(rows, 1, False), (wgrad, 2 | 8, False)] + ([("k1_bwd_fin", 16, False)] if finalize_due else [])


def _k1_bwd_entry(lib, gate, dy, x1, x2, pk_a, pk_g, act, y, dx1_in):
    """The K1 backward's C call for what is present, and its arguments between ``phases`` and ``dx1``.  With a gate and the forward's
    block: the entry point that takes ``y`` and ``dx1_in``, either of which may be NULL (the same call as _bwd_saved / _bwd_saved_acc)."""
    head = (dy.data_ptr(), _ptr(x1) if gate else None, x2.data_ptr())
    packs = (pk_a.buf.data_ptr(), pk_g.buf.data_ptr() if gate else None)
    if act is None:
        return lib.vlpet_adapter_gate_bwd_phase, (*head, *packs)
    if not gate:
        return lib.vlpet_adapter_gate_bwd_saved, (*head, act.data_ptr(), *packs)
    return lib.vlpet_adapter_gate_bwd_saved_y, (*head, _ptr(y), act.data_ptr(), *packs, _ptr(dx1_in))


class _AdapterGateFn(torch.autograd.Function):
    """K1.  inputs: x1, x2, then N_h down weights, N_h down biases, up w, up b, gate down w/b, gate up w/b."""

    @staticmethod
    def forward(ctx, x1, x2, pk_a, pk_g, n_heads, gate_mode, delta_scale, x2_scale, gate_scale, link, out_link, *params):
        lib = _lib.load()
        _need_cuda(x1, x2)
        d = x2.shape[-1]
        io = _io_dtype(x2)
        x2f = _flat(x2, d)
        x1f = _flat(x1, d) if gate_mode != GATE_NONE else None
        M = x2f.shape[0]
        out = torch.empty_like(x2f)
        act = _saved_block(ctx, lambda: lib.vlpet_saved_bytes(M, pk_a.tiles, io), x2f.device)
        _block_call("vlpet_adapter_gate_fwd", "_save", act, "k1_fwd", M,
                    (_ptr(x1f), x2f.data_ptr(), pk_a.buf.data_ptr(), pk_g.buf.data_ptr() if pk_g is not None else None, out.data_ptr()),
                    (M, d, pk_a.tiles, gate_mode, float(delta_scale), float(x2_scale), float(gate_scale), io))
        # the tail that follows may park its d/dx1 for this op's backward
        ctx.link = link.arm() if (link is not None and act is not None and gate_mode != GATE_NONE and x1.requires_grad) else None
        # the other direction: the sublayer's first GEMM (upstream of x2) armed `out_link` -- this backward parks d/dx1 there
        ctx.out_link = ResidualLink.if_armed(out_link) if gate_mode != GATE_NONE else None
        # the multiplicative gate's backward can start from this output (dq = dy * y * (1 - g): csrc/pet_dz2.hip "YF").  Keeping it is
        # NOT free: the sublayer tail that consumes it saves its own output / pre-norm sum, not y, so one more [M, d] tensor of
        # the IO dtype lives from this forward to its backward -- 12 of them in a BART-base encoder, 24 in T5-base (43 MB each at 28,000
        # rows: +0.5 GB of peak activation memory at the configs[1] batch, measured by bench.py's peak_memory_GB with
        # VLPET_K1_BWD_FROM_X2=1 beside the default).  On a 288 GB device the 3 % faster pass 1
        # is the better trade; memory-constrained runs set K1_BWD_FROM_OUTPUT = False.
        ctx.has_y = bool(K1_BWD_FROM_OUTPUT and act is not None and gate_mode == GATE_MUL)
        ctx.save_for_backward(x1f if x1f is not None else x2f, x2f, *params, *((out,) if ctx.has_y else ()))
        ctx.pk = (pk_a, pk_g)
        ctx.cfg = (n_heads, gate_mode, float(delta_scale), float(x2_scale), float(gate_scale), x2.shape,
                   x1.shape if x1 is not None else None)
        return out.view(x2.shape)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x1f, x2f, *params = ctx.saved_tensors
        yf = params.pop() if ctx.has_y else None
        pk_a, pk_g = ctx.pk
        n_heads, gate_mode, sd, s2, gs, shp2, shp1 = ctx.cfg
        M, d = x2f.shape
        io = _io_dtype(x2f)
        gate = gate_mode != GATE_NONE
        dyf = _flat(dy, d)
        r, rg = pk_a.r, (pk_g.r if gate else 0)
        slots = AdapterSlots(params, n_heads, r, rg, d)
        dx2 = torch.empty_like(x2f)
        dx1 = torch.empty_like(x2f) if gate else None
        ws, nws = _bwd_workspace(lib, M, d, pk_a.tiles, gate, io, x2f.device)
        act, ctx.act = ctx.act, None
        # the sublayer tail's residual-stream gradient, if it was handed over (ResidualLink): summed inside the kernel
        link, ctx.link = ctx.link, None
        dx1_in = link.take(x2f.shape, x2f.dtype) if link is not None else None
        fn, lead = _k1_bwd_entry(lib, gate, dyf, x1f, x2f, pk_a, pk_g, act, yf, dx1_in)
        args = (*lead, _ptr(dx1), dx2.data_ptr(), *slots.ptrs(), r, rg, ws.data_ptr(), nws, M, d, pk_a.tiles, gate_mode, sd, s2, gs, io)
        side = WGRAD_STREAM if slots.all_sunk else None
        split = side is not None or K1_BWD_PREVIOUS_SPLIT
        # (the schedule's bracketed branch, the only one that asks the library for the form: there the timer brackets EVERY step)
        bracketed = not split and TIMER is not None and TIMER.wants("k1_bwd_rows")
        form = lib.vlpet_adapter_gate_bwd_form(M, d, pk_a.tiles, io) if (bracketed and gate and act is not None) else 0
        fin = form == 2 and (K1_BWD_FINALIZE_LAUNCH or lib.vlpet_adapter_gate_bwd_finalize_launch(M, d, pk_a.tiles, io) == 1)
        # (A/B, bit 5: the round-3 form -- partial slabs + a finalize launch -- instead of the in-launch reduce-scatter)
        fin_bit = 32 if K1_BWD_FINALIZE_LAUNCH else 0

        def step(name, bits):
            call = lambda: fn(bits | fin_bit, *args, _stream())     # (the current stream: the side stream's inside its context)
            if name is None or TIMER is None or not (bracketed or TIMER.wants(name)):
                return call()
            return TIMER.bracket(name, M, call)

        rc = 0
        for name, bits, on_side in k1_bwd_schedule(gate, act is not None, side is not None, K1_BWD_PREVIOUS_SPLIT, bracketed, form, fin):
            if rc != 0:
                break
            if not on_side:
                rc = step(name, bits)
                continue
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                rc = step(name, bits)
            for t in (x1f, x2f, dyf, ws, pk_a.buf) + ((pk_g.buf,) if gate else ()) + ((act,) if act is not None else ()) \
                    + ((yf,) if yf is not None else ()):
                t.record_stream(side)        # the caching allocator must not recycle them under the side stream
        _lib.check(rc, "vlpet_adapter_gate_bwd")
        if not gate:
            # without a gate the kernel returns the adapter-branch gradient only; add the residual path
            dx2 = dx2 + s2 * dyf
        grads = slots.finish(params, n_heads)
        # (out_link: the dgrad GEMM of the sublayer's first projection accumulates onto d/dx1 -- _LinearAccFn)
        gx1 = _park_or_return(ctx, "out_link", dx1.view(shp1)) if gate else None
        return (gx1, dx2.view(shp2), None, None, None, None, None, None, None, None, None, *grads)


def adapter_gate(x1, x2, down_w, down_b, up_w, up_b, gate_params, pk_a: PackedPair, pk_g: Optional[PackedPair],
                 gate_mode=GATE_MUL, delta_scale=1.0, x2_scale=1.0, gate_scale=1.0, link: Optional[ResidualLink] = None,
                 out_link: Optional[ResidualLink] = None):
    """Encoder granularity-controlled adapter (+ low-rank gate).  ``gate_params`` =
    (gate_down_w, gate_down_b, gate_up_w, gate_up_b) or None.  ``link``: see ResidualLink (the tail's d/dx1 comes in);
    ``out_link``: armed by the sublayer's first GEMM (linear_acc) -- this op's d/dx1 goes out through it.
    A caller outside ``train.Trainer`` whose other kernels share the device during the backward (gradient collectives on another
    stream, a second trainer) sets ``K1_BWD_FINALIZE_LAUNCH = True`` around it: the in-launch reduce of pass 2 waits for partner
    workgroups, which such kernels can keep from starting (a bounded wait: the results stay right, the time is lost)."""
    params = list(down_w) + list(down_b) + [up_w, up_b]
    if gate_mode != GATE_NONE:
        params += list(gate_params)
    if x2.numel() == 0:
        return _empty_result(x2, params)
    return _AdapterGateFn.apply(x1, x2, pk_a, pk_g, len(down_w), gate_mode, delta_scale, x2_scale, gate_scale, link, out_link,
                                *params)


class _ParallelAdapterFn(torch.autograd.Function):
    """K2: out = y + scale * up(gelu_new(down(x)))."""

    @staticmethod
    def forward(ctx, x, y, pk, scale, link, wd, bd, wu, bu):
        lib = _lib.load()
        _need_cuda(x, y)
        ctx.link = ResidualLink.if_armed(link) if ctx.needs_input_grad[0] else None
        d = x.shape[-1]
        io = _io_dtype(x)
        xf, yf = _flat(x, d), _flat(y, d)
        M = xf.shape[0]
        out = torch.empty_like(xf)
        act = _saved_block(ctx, lambda: lib.vlpet_saved_bytes(M, pk.tiles, io), xf.device)      # (z / gelu'(pre) for the backward, see K1)
        _block_call("vlpet_parallel_adapter_fwd", "_save", act, "k2_fwd", M, (xf.data_ptr(), yf.data_ptr(), pk.buf.data_ptr(), out.data_ptr()),
                    (M, d, pk.tiles, float(scale), io))
        ctx.save_for_backward(xf, wd, bd, wu, bu)
        ctx.pk, ctx.scale, ctx.shape = pk, float(scale), x.shape
        return out.view(y.shape)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        xf, wd, bd, wu, bu = ctx.saved_tensors
        pk = ctx.pk
        M, d = xf.shape
        io = _io_dtype(xf)
        dyf = _flat(dy, d)
        r = pk.r
        # bu is None when the up bias belongs to another half of a split bottleneck (encoder_pet._apply_pet_split)
        dwd, dbd, dwu, dbu = (grad_slot(wd, (r, d)), grad_slot(bd, (r,)), grad_slot(wu, (d, r)),
                              grad_slot(bu, (d,)) if bu is not None else GradSlot.scratch((d,), xf.device))
        dx = torch.empty_like(xf)
        ws, nws = _bwd_workspace(lib, M, d, pk.tiles, False, io, xf.device)
        act, ctx.act = ctx.act, None
        _block_call("vlpet_parallel_adapter_bwd", "_saved", act, "k2_bwd", M, (dyf.data_ptr(), xf.data_ptr()),
                    (pk.buf.data_ptr(), dx.data_ptr(), dwd.ptr, dbd.ptr, dwu.ptr, dbu.ptr, r, ws.data_ptr(), nws, M, d, pk.tiles, ctx.scale, io))
        grads = [s.finish() for s in (dwd, dbd, dwu, dbu)]
        # (link: the projection that made `y` from the same `x` accumulates its dgrad onto dx -- _LinearAccFn)
        gx = _park_or_return(ctx, "link", dx.view(ctx.shape))
        return (gx, dy, None, None, None, *grads)


def parallel_adapter(x, y, wd, bd, wu, bu, pk: PackedPair, scale: float = 1.0, link: Optional[ResidualLink] = None):
    """``link``: armed by the frozen projection that produced ``y`` from the same ``x`` (linear_acc); d/dx is parked there."""
    if x.numel() == 0:
        return _empty_result(y, [wd, bd, wu, bu])
    return _ParallelAdapterFn.apply(x, y, pk, scale, link, wd, bd, wu, bu)


LORA_R8_STREAMING = True     # A/B switch (tools/): False = the MFMA kernels at every rank


class _LoraDeltaFn(torch.autograd.Function):
    """K3: out = base + scaling * ((dropout(x) A^T) B^T); base comes from the library GEMM.

    Dropout (lora/controller.py:66): ``p`` > 0 with ``keep`` None -> the kernels' counter-based generator keyed by
    ``seed`` (forward, backward rows kernel and weight-gradient kernel regenerate the same mask; nothing is stored);
    ``keep`` given -> that explicit 0/1 mask.  ``want_mask``: also return the applied mask (parity tests)."""

    @staticmethod
    def forward(ctx, x, base, pk, scaling, keep, p, seed, want_mask, lora_a, lora_b, link=None):
        # (`link`: armed by the frozen projection that produced `base` from the same x -- its dgrad GEMM takes over d/dx)
        ctx.link = ResidualLink.if_armed(link) if ctx.needs_input_grad[0] else None
        lib = _lib.load()
        _need_cuda(x, base)
        d = x.shape[-1]
        io = _io_dtype(x)
        xf, bf = _flat(x, d), _flat(base, d)
        M = xf.shape[0]
        out = torch.empty_like(bf)
        kf = None
        if keep is not None:
            kf = _flat(keep, d)
            if kf.dtype != torch.uint8:
                kf = kf.to(torch.uint8)
        mask = torch.empty(M, d, dtype=torch.uint8, device=xf.device) if (want_mask and p > 0) else None
        head = (xf.data_ptr(), bf.data_ptr(), pk.buf.data_ptr(), _ptr(kf), float(p), int(seed), _ptr(mask), out.data_ptr())
        act = _saved_block(ctx, lambda: lib.vlpet_lora_saved_bytes(M, d, pk.tiles, io), xf.device)     # (z = dropout(x) A^T, see K1 / K2)
        if LORA_R8_STREAMING and lib.vlpet_lora_r8_applies(M, d, pk.r, io):
            # rank <= 8: the streaming row kernel (csrc/lora8.hip) -- same pack, same masks, same saved block as the MFMA form
            rc = _timed("k3_fwd", M, lambda: lib.vlpet_lora_delta_fwd_r8(*head, _ptr(act), M, d, pk.r, float(scaling), io, _stream()))
            _lib.check(rc, "vlpet_lora_delta_fwd")
        else:
            _block_call("vlpet_lora_delta_fwd", "_save", act, "k3_fwd", M, head, (M, d, pk.tiles, float(scaling), io))
        ctx.save_for_backward(xf, lora_a, lora_b)
        ctx.keep = kf
        ctx.cfg = (pk, float(scaling), float(p), int(seed), x.shape)
        out = out.view(base.shape)
        if want_mask:
            if mask is None:
                mask = torch.ones(M, d, dtype=torch.uint8, device=xf.device)
            ctx.mark_non_differentiable(mask)
            return out, mask.view(x.shape)
        return out

    @staticmethod
    def backward(ctx, dy, *unused):
        lib = _lib.load()
        xf, lora_a, lora_b = ctx.saved_tensors
        pk, scaling, p, seed, shape = ctx.cfg
        M, d = xf.shape
        io = _io_dtype(xf)
        dyf = _flat(dy, d)
        r = pk.r
        da, db = grad_slot(lora_a, (r, d)), grad_slot(lora_b, (d, r))
        dx = torch.empty_like(xf)
        ws, nws = _bwd_workspace(lib, M, d, pk.tiles, False, io, xf.device)
        act, ctx.act = ctx.act, None
        _block_call("vlpet_lora_delta_bwd", "_saved", act, "k3_bwd", M, (dyf.data_ptr(), xf.data_ptr()),
                    (pk.buf.data_ptr(), _ptr(ctx.keep), p, seed, dx.data_ptr(), da.ptr, db.ptr, r, ws.data_ptr(), nws, M, d, pk.tiles, scaling, io))
        gx = _park_or_return(ctx, "link", dx.view(shape))
        return (gx, dy, None, None, None, None, None, None, da.finish(), db.finish(), None)


def lora_delta(x, base, lora_a, lora_b, pk: PackedPair, scaling: float, keep=None, p: float = 0.0, seed: int = 0,
               return_mask: bool = False, link: Optional["ResidualLink"] = None):
    """``base + scaling * (dropout(x, p) @ A^T @ B^T)``.  ``keep`` (uint8 [.., d]) overrides the generator's mask."""
    if x.numel() == 0:
        out = _empty_result(base, [lora_a, lora_b])
        return (out, torch.empty(x.shape, dtype=torch.uint8, device=x.device)) if return_mask else out
    return _LoraDeltaFn.apply(x, base, pk, scaling, keep, p, seed, return_mask, lora_a, lora_b, link)


# ---- Compacter: the weights of one adapter's (down, up) pair of PHM layers, generated by csrc/phm.hip
PHM_MAX_DIVISION = 8       # the kernels take 1 <= n <= 8 (include/vlpet_hip.h); other divisions run eager.phm_weight
PHM_CALLS = 0              # expansion launches issued (tests assert on it; a replayed graph does not count)


def phm_expand_pair_into(rule_d, W_d, rule_u, W_u, n: int, out=None):
    """``(wt_d [r, d], wt_u [d, r])`` = (H_down^T, H_up^T) in the parameters' dtype, one launch, no autograd.  ``out``: an earlier
    result of the same geometry to refresh IN PLACE (its buffers may be baked into a captured graph, as for ``pack_pair(out=)``)."""
    global PHM_CALLS
    lib = _lib.load()
    ts = [t.detach() for t in (rule_d, W_d, rule_u, W_u)]
    _need_cuda(*ts)
    ts = [t if t.is_contiguous() else t.contiguous() for t in ts]
    if len({t.dtype for t in ts}) != 1:
        raise RuntimeError("vl-pet_amd: mixed parameter dtypes in one PHM pair")
    n = int(n)
    d, r = n * W_d.shape[1], n * W_d.shape[2]
    if tuple(W_u.shape) != (n, r // n, d // n) or tuple(rule_d.shape) != (n, n, n) or tuple(rule_u.shape) != (n, n, n):
        raise RuntimeError(f"vl-pet_amd: PHM pair shapes {tuple(rule_d.shape)}, {tuple(W_d.shape)}, {tuple(rule_u.shape)}, "
                           f"{tuple(W_u.shape)} do not belong to one adapter with n = {n}")
    ok = (out is not None and out[0].shape == (r, d) and out[1].shape == (d, r) and out[0].dtype == ts[1].dtype
          and out[1].dtype == ts[1].dtype and out[0].device == ts[1].device and out[1].device == ts[1].device)
    wt_d, wt_u = out if ok else (torch.empty(r, d, dtype=ts[1].dtype, device=ts[1].device),
                                 torch.empty(d, r, dtype=ts[1].dtype, device=ts[1].device))
    rc = _timed("phm_fwd", d, lambda: lib.vlpet_phm_expand_pair_fwd(
        ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), wt_d.data_ptr(), wt_u.data_ptr(), d, r, n,
        _param_dtype(ts[1]), _stream()))
    _lib.check(rc, "vlpet_phm_expand_pair_fwd")
    PHM_CALLS += 1
    return wt_d, wt_u


class _PhmExpandPairFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rule_d, W_d, rule_u, W_u, n):
        ctx.save_for_backward(rule_d, W_d, rule_u, W_u)
        ctx.n = int(n)
        return phm_expand_pair_into(rule_d, W_d, rule_u, W_u, n)

    @staticmethod
    def backward(ctx, dwt_d, dwt_u):
        lib = _lib.load()
        rule_d, W_d, rule_u, W_u = (t.detach() if t.is_contiguous() else t.detach().contiguous() for t in ctx.saved_tensors)
        n = ctx.n
        d, r = n * W_d.shape[1], n * W_d.shape[2]
        f32 = dict(dtype=torch.float32, device=W_d.device)
        # K2 / K1 hand the gradients of non-leaf weights back as fresh fp32 tensors (grad_slot finds no sink); an unused output has none
        g_d = torch.zeros(r, d, **f32) if dwt_d is None else dwt_d.float().contiguous()
        g_u = torch.zeros(d, r, **f32) if dwt_u is None else dwt_u.float().contiguous()
        drule_d, drule_u = torch.empty(n, n, n, **f32), torch.empty(n, n, n, **f32)       # (a shared rule: autograd sums the two)
        dW_d, dW_u = grad_slot(ctx.saved_tensors[1], W_d.shape), grad_slot(ctx.saved_tensors[3], W_u.shape)
        nws = lib.vlpet_phm_workspace_bytes(d, r, n)
        ws = torch.empty(nws, dtype=torch.uint8, device=W_d.device)
        rc = _timed("phm_bwd", d, lambda: lib.vlpet_phm_expand_pair_bwd(
            g_d.data_ptr(), g_u.data_ptr(), rule_d.data_ptr(), W_d.data_ptr(), rule_u.data_ptr(), W_u.data_ptr(), drule_d.data_ptr(),
            dW_d.ptr, drule_u.data_ptr(), dW_u.ptr, ws.data_ptr(), nws, d, r, n, _param_dtype(W_d), _stream()))
        _lib.check(rc, "vlpet_phm_expand_pair_bwd")
        gW_d, gW_u = dW_d.finish(), dW_u.finish()
        return _grad_like(drule_d, rule_d), gW_d, _grad_like(drule_u, rule_u), gW_u, None


def phm_expand_pair(rule_d, W_d, rule_u, W_u, n: int):
    """``(wt_d, wt_u)``: the nn.Linear-layout weights of a Compacter adapter's down and up PHM layers (rule [n, n, n]; W_d
    [n, d / n, r / n], W_u [n, r / n, d / n]; one dtype, fp32 or bf16), differentiable in all four.  They go to ``parallel_adapter`` /
    ``adapter_gate`` as ``wd`` / ``wu``.  A rule shared by both layers is the same tensor passed twice."""
    return _PhmExpandPairFn.apply(rule_d, W_d, rule_u, W_u, n)


# ---- Hyperformer: the adapter weights of every layer of one stack, generated by csrc/hyper.hip
HYPER_MAX_MAPS, HYPER_MAX_ROWS, HYPER_MAX_DIM, HYPER_MAX_ROW_POINTERS = 16, 64, 64, 256      # include/vlpet_hip.h; beyond: eager.hyper_generate
HYPER_CALLS = 0            # generator launches issued (tests assert on it; a replayed graph does not count)


def hyper_applies(n_maps: int, n_rows: int, dim: int, dtype=torch.float32) -> bool:
    """whether the generator kernels take S = n_maps linear maps on E = n_rows embedding rows of width P = dim in ``dtype``"""
    return (1 <= n_maps <= HYPER_MAX_MAPS and 1 <= n_rows <= HYPER_MAX_ROWS and 1 <= dim <= HYPER_MAX_DIM
            and n_maps * n_rows <= HYPER_MAX_ROW_POINTERS and dtype in (torch.float32, torch.bfloat16))


def _ptr_table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _hyper_check(maps, e):
    """-> (weights, biases, n) of ``maps`` = [(G_s [n_s, P], g_s [n_s])], detached and contiguous; ``e`` [E, P] fp32"""
    if not maps:
        raise RuntimeError("vl-pet_amd: hyper_generate needs at least one (weight, bias) map")
    Gs, gs = [m[0].detach() for m in maps], [m[1].detach() for m in maps]
    _need_cuda(e, *Gs, *gs)
    if e.dim() != 2 or e.dtype != torch.float32:
        raise RuntimeError(f"vl-pet_amd: hyper_generate takes fp32 embeddings [E, P] (got {tuple(e.shape)}, {e.dtype})")
    P = e.shape[1]
    if len({t.dtype for t in Gs + gs}) != 1:
        raise RuntimeError("vl-pet_amd: mixed parameter dtypes in one hyper-network")
    for G, g in zip(Gs, gs):
        if G.dim() != 2 or G.shape[1] != P or tuple(g.shape) != (G.shape[0],):
            raise RuntimeError(f"vl-pet_amd: generator shapes {tuple(G.shape)}, {tuple(g.shape)} do not map embeddings of width {P}")
    if not hyper_applies(len(maps), e.shape[0], P, Gs[0].dtype):
        raise RuntimeError(f"vl-pet_amd: hyper_generate takes up to {HYPER_MAX_MAPS} maps, {HYPER_MAX_ROWS} embedding rows of width <= "
                           f"{HYPER_MAX_DIM}, maps x rows <= {HYPER_MAX_ROW_POINTERS}, fp32 or bf16 parameters (got {len(maps)} maps, "
                           f"embeddings {tuple(e.shape)}, {Gs[0].dtype})")
    Gs = [t if t.is_contiguous() else t.contiguous() for t in Gs]
    gs = [t if t.is_contiguous() else t.contiguous() for t in gs]
    return Gs, gs, [int(G.shape[0]) for G in Gs]


def hyper_generate_into(maps, e, out=None):
    """``[out_s [E, n_s]]`` with ``out_s[l] = G_s e[l] + g_s`` for every map of ``maps`` = [(G_s [n_s, P], g_s [n_s])], in the
    parameters' dtype: one launch, no autograd.  ``out``: an earlier result of the same geometry to refresh IN PLACE (its buffers may
    be baked into a captured graph, as for ``pack_pair(out=)``)."""
    global HYPER_CALLS
    lib = _lib.load()
    Gs, gs, n = _hyper_check(maps, e)
    ed = e.detach()
    ed = ed if ed.is_contiguous() else ed.contiguous()
    E, P = ed.shape
    ok = out is not None and len(out) == len(n) and all(
        o.shape == (E, k) and o.dtype == Gs[0].dtype and o.device == Gs[0].device and o.is_contiguous() for o, k in zip(out, n))
    outs = list(out) if ok else [torch.empty(E, k, dtype=Gs[0].dtype, device=Gs[0].device) for k in n]
    tabs = (_ptr_table([t.data_ptr() for t in Gs]), _ptr_table([t.data_ptr() for t in gs]), (ctypes.c_int * len(n))(*n),
            _ptr_table([t.data_ptr() for t in outs]))
    rc = _timed("hyper_fwd", sum(n), lambda: lib.vlpet_hyper_gen_fwd(len(n), tabs[0], tabs[1], tabs[2], ed.data_ptr(), E, P, tabs[3],
                                                                     _param_dtype(Gs[0]), _stream()))
    _lib.check(rc, "vlpet_hyper_gen_fwd")
    HYPER_CALLS += 1
    return outs


class _HyperGenerateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, *flat):
        maps = list(zip(flat[0::2], flat[1::2]))
        ctx.save_for_backward(e, *flat)
        outs = hyper_generate_into(maps, e)
        # one output per map and row, so that a row nobody uses costs the backward nothing (its gradient arrives as None)
        return tuple(o[l] for o in outs for l in range(o.shape[0]))

    @staticmethod
    def backward(ctx, *douts):
        lib = _lib.load()
        e, *flat = ctx.saved_tensors
        maps = list(zip(flat[0::2], flat[1::2]))
        Gs, _, n = _hyper_check(maps, e)
        ed = e.detach()
        ed = ed if ed.is_contiguous() else ed.contiguous()
        E, P = ed.shape
        # K2 / K1 hand the gradients of non-leaf weights back as fresh fp32 tensors (grad_slot finds no sink); an unused row has none
        rows = [None if g is None else g.detach().reshape(-1).float().contiguous() for g in douts]
        dG = [grad_slot(G, (k, P)) for (G, _), k in zip(maps, n)]
        dg = [grad_slot(g, (k,)) for (_, g), k in zip(maps, n)]
        de = torch.empty(E, P, dtype=torch.float32, device=ed.device)
        n_tab = (ctypes.c_int * len(n))(*n)
        nws = lib.vlpet_hyper_gen_workspace_bytes(len(n), n_tab, E, P)
        ws = torch.empty(nws, dtype=torch.uint8, device=ed.device)
        tabs = (_ptr_table([_ptr(t) for t in rows]), _ptr_table([t.data_ptr() for t in Gs]), _ptr_table([s.ptr for s in dG]),
                _ptr_table([s.ptr for s in dg]))
        rc = _timed("hyper_bwd", sum(n), lambda: lib.vlpet_hyper_gen_bwd(len(n), tabs[0], tabs[1], n_tab, ed.data_ptr(), E, P, tabs[2],
                                                                         tabs[3], de.data_ptr(), ws.data_ptr(), nws,
                                                                         _param_dtype(Gs[0]), _stream()))
        _lib.check(rc, "vlpet_hyper_gen_bwd")
        grads = []
        for a, b in zip(dG, dg):
            grads += [a.finish(), b.finish()]
        return (de, *grads)


def hyper_generate(maps, e):
    """Hyperformer's weight generator for one stack: ``maps`` = [(G_s [n_s, P], g_s [n_s])] (the ``.0`` Linears of the weight and bias
    generators, one dtype, fp32 or bf16), ``e`` [E, P] fp32 (the layers' projected embeddings).  Returns ``rows[s][l]`` [n_s] =
    ``G_s e[l] + g_s`` in the parameters' dtype: one launch for all maps and rows, differentiable in every G_s, g_s and in e (two
    launches).  Row l of a weight generator, viewed [r, d] / [d, r], goes to ``parallel_adapter`` / ``adapter_gate`` as ``wd`` / ``wu``."""
    flat = [t for m in maps for t in m[:2]]
    E = e.shape[0]
    out = _HyperGenerateFn.apply(e, *flat)
    return [list(out[s * E:(s + 1) * E]) for s in range(len(maps))]
