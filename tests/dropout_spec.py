"""Dropout masks of the HIP kernels -- host-side specification of both generators.

The reference applies ``F.dropout(p)``: every element kept i.i.d. with probability 1 - p, independently across elements,
call sites and steps.  The kernels never store a mask; they regenerate it from (seed, element index), so the whole mask is a
pure function that numpy can restate.  This module is that restatement.  The CPU tests (tests/test_dropout_spec.py) check
its statistics; the GPU test (tests/test_gpu_dropout_masks.py) checks that every site of the library applies exactly it.

Two generators:

* **Philox-4x32-7** (csrc/rng.h: ``philox7``, ``keep8``, ``drop_pos``, ``vlpet_eff_seed``) -- the sublayer tail (LayerNorm and
  RMS forms, csrc/tail.hip), ``act.act_dropout`` / ``act.concat_dropout`` (csrc/actdrop.hip) and the LoRA kernels (pet_fwd,
  pet_bwd, wgrad, lora8).  Counter = index of the 8-element group of the row-major tensor, key = the 64-bit seed; element j of a
  group keeps iff 16-bit lane j of the 128-bit output (word j >> 1, half j & 1) is >= ``thr``, with ``thr`` from
  ``tail_thr`` / ``make_drop`` (csrc/api.hip): ``min(int(float32(p) * 65536 + 0.5), 65535)``; ``thr == 0`` means no dropout.
* **the attention's element hash** (csrc/attn_common.h: ``hash32``, ``row_key``, ``hash_elem``, ``keep_elem``) -- one 32-bit key
  per (b, h, i) row, then per key j ``hash_elem(rk + j * 0x9E3779B9) >= thr`` with ``thr`` from ``attn_thr`` (csrc/api.hip):
  ``min(int(float32(p) * 2^32 + 0.5), 2^32 - 1)``; ``thr == 0`` keeps everything.

Both take the graph-replay step counter the same way (``vlpet_eff_seed``): ``seed + ctr * 0x9E3779B97F4A7C15`` mod 2^64.

All arithmetic is numpy uint64 with explicit 32-bit masking, vectorised over the whole mask.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GOLDEN64 = 0x9E3779B97F4A7C15
WEYL32 = 0x9E3779B9


def _u64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ shared: thresholds, seeds
def tail_thr(p: float) -> int:
    """csrc/api.hip tail_thr / make_drop: the 16-bit drop threshold.  p arrives as a C float."""
    t = float(np.float32(p)) * 65536.0 + 0.5
    return int(min(t, 65535.0))


def attn_thr(p: float) -> int:
    """csrc/api.hip attn_thr: the 32-bit drop threshold of the attention."""
    t = float(np.float32(p)) * 4294967296.0 + 0.5
    return int(min(t, 4294967295.0))


def keep_scale(p: float) -> np.float32:
    """1.0f / (1.0f - p) as the kernels compute it (float arithmetic)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def vlpet_eff_seed(seed: int, ctr=None) -> int:
    """csrc/rng.h vlpet_eff_seed: the call's seed with the device step counter mixed in (None = no counter registered)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    if ctr is None:
        return seed
    return (seed + (int(ctr) & 0xFFFFFFFFFFFFFFFF) * GOLDEN64) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ Philox-4x32-7 (csrc/rng.h)
def philox7(c0, c1, k0: int, k1: int):
    """csrc/rng.h philox7: counter (c0, c1, 0x5bd1e995, 0x2545f491), key (k0, k1), seven rounds -> four uint32 words (as uint64
    arrays holding 32-bit values)."""
    c0 = _u64(c0) & M32
    c1 = _u64(c1) & M32
    c2 = np.full(c0.shape, 0x5BD1E995, dtype=np.uint64)
    c3 = np.full(c0.shape, 0x2545F491, dtype=np.uint64)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(7):
        p0 = m0 * c0            # < 2^64: no wrap
        p1 = m1 * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def lanes16(group, seed: int) -> np.ndarray:
    """The eight 16-bit uniforms of 8-element group(s) ``group``: [..., 8], lane j = element 8 group + j."""
    group = _u64(group)
    o = philox7(group & M32, group >> np.uint64(32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty(group.shape + (8,), dtype=np.uint32)
    for j in range(8):
        out[..., j] = (o[j >> 1] >> np.uint64(16 * (j & 1))) & np.uint64(0xFFFF)
    return out


def keep8(group, seed: int, thr: int) -> np.ndarray:
    """csrc/rng.h keep8 as a bit field: bit j set = element j of the group kept."""
    kept = lanes16(group, seed) >= np.uint32(thr)
    return (kept.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=-1).astype(np.uint32)


def keep_mask(M: int, d: int, seed: int, p: float, ctr=None) -> np.ndarray:
    """[M, d] bool keep mask of a Philox site for a row-major [M, d] tensor (d % 8 == 0): the tail, act_dropout, the LoRA
    kernels; concat_dropout with M = B * (La + Lv)."""
    assert d % 8 == 0
    thr = tail_thr(p)
    if thr == 0:
        return np.ones((M, d), dtype=bool)
    groups = np.arange(M * d // 8, dtype=np.uint64)
    kept = lanes16(groups, vlpet_eff_seed(seed, ctr)) >= np.uint32(thr)
    return kept.reshape(M, d)


def drop_pos(G):
    """csrc/rng.h drop_pos: byte position, inside a row's d / 8 mask bytes, of 8-element group G."""
    G = np.asarray(G)
    return (G & ~7) + ((G & 1) << 2) + ((G >> 1) & 3)


def packed_bits(mask: np.ndarray) -> np.ndarray:
    """The [M, d / 8] uint8 packed form of a keep mask, as the LoRA forward leaves it for the backward (bit j of the byte at
    drop_pos(G) = element 8 G + j)."""
    M, d = mask.shape
    ng = d // 8
    by = (mask.reshape(M, ng, 8).astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
    out = np.empty_like(by)
    out[:, drop_pos(np.arange(ng))] = by
    return out


# ------------------------------------------------------------------------------------------------ attention (csrc/attn_common.h)
def hash32(x) -> np.ndarray:
    """csrc/attn_common.h hash32: xorshift-multiply, two rounds."""
    x = _u64(x) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def row_key(seed: int, row) -> np.ndarray:
    """csrc/attn_common.h row_key: the 32-bit key of attention row(s) ``row`` = (b * H + h) * Lq + i."""
    row = _u64(row)
    k = hash32(np.uint64(seed & 0xFFFFFFFF) ^ hash32((np.uint64((seed >> 32) & 0xFFFFFFFF) + (row >> np.uint64(32))) & M32))
    return hash32((k + (row & M32)) & M32)


def row_key_xor(seed: int, row) -> np.ndarray:
    """The row key before the fix (seed_lo ^ row): kept so that the CPU tests show what their seed-neighbour check catches."""
    row = _u64(row)
    lo = hash32(np.uint64(seed & 0xFFFFFFFF) ^ (row & M32))
    hi = hash32((np.uint64((seed >> 32) & 0xFFFFFFFF) + (row >> np.uint64(32))) & M32)
    return lo ^ hi


def hash_elem(x) -> np.ndarray:
    """csrc/attn_common.h hash_elem: the per-element finaliser over (row key + j * golden) -- one multiply-xorshift round, a rotation
    by 16 (v_alignbit_b32 of x with itself), a second multiply."""
    x = hash_elem_one_round(x)
    x = ((x >> np.uint64(16)) | (x << np.uint64(16))) & M32
    return (x * np.uint64(0x846CA68B)) & M32


def hash_elem_one_round(x) -> np.ndarray:
    """The element hash before the fix (one multiply-xorshift round): kept so that the CPU tests show what their column-pair
    bound catches."""
    x = _u64(x) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    return x ^ (x >> np.uint64(15))


def elem_uniform(rk, j, elem=hash_elem) -> np.ndarray:
    """The 32-bit uniform of element (row with key ``rk``, key ``j``) (broadcasting)."""
    return elem((_u64(rk) + _u64(j) * np.uint64(WEYL32)) & M32)


def keep_elem(rk, j, thr: int, elem=hash_elem) -> np.ndarray:
    """csrc/attn_common.h keep_elem."""
    return elem_uniform(rk, j, elem) >= np.uint64(thr)


def attn_keep(B: int, H: int, Lq: int, Lk: int, seed: int, p: float, ctr=None, elem=hash_elem, rkey=row_key) -> np.ndarray:
    """[B, H, Lq, Lk] bool keep mask of the attention probabilities (short_attention, short_self_attention).  ``elem`` / ``rkey``:
    the element hash and the row key (the defaults are the kernels')."""
    thr = attn_thr(p)
    if thr == 0:
        return np.ones((B, H, Lq, Lk), dtype=bool)
    rows = np.arange(B * H * Lq, dtype=np.uint64)
    rk = rkey(vlpet_eff_seed(seed, ctr), rows)
    keep = keep_elem(rk[:, None], np.arange(Lk, dtype=np.uint64)[None, :], thr, elem)
    return keep.reshape(B, H, Lq, Lk)
