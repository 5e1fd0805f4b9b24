"""Host glue of the cached greedy decode step (csrc/decode.hip) and the generation loop of ``VLBart.generate`` / ``VLT5.generate``.

HF 4.2.1 ``greedy_search`` as the reference evaluates with it (src/multitask.py:480-516 test_step -> ``model.generate(**batch)``,
vqa_model.py:128-136; captioning at ``max_length = gen_max_length``, :587-588): the output starts with the decoder start token, the
logits processors ``NoRepeatNGramLogitsProcessor`` / ``MinLengthLogitsProcessor`` act on the last position's logits, the argmax is
the next token, a row that has emitted eos emits pad from then on, the loop ends when every row has finished or the output has
``max_length`` tokens.  The reference recomputes nothing: HF feeds ``past_key_values`` back; here every decoder layer keeps a key /
value cache allocated once per call at ``max_length`` rows, and the cross-attention caches are projected once from the encoder output.

Two kernels per step are ours: ``decode_attention`` (one query row against a cache; the self-attention step appends its key / value
row in the same launch) and ``greedy_pick`` (processors + argmax + finish bookkeeping from one read of the logits).  Inputs the
kernels do not take -- CPU tensors, other head dims, strides they cannot read -- run the torch forms below (the package's eager
fallback; ``EAGER = True`` forces them, the "torch cached" leg of tools/genbench.py).  The attention fallback goes through
``host.bart.attention_core`` so that the CPU parity harness of the test suite, which swaps that attribute, covers it."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import _lib
from .functional import _io_dtype, _stream

EAGER = False                   # A/B switch: the torch forms for every call (tools/genbench.py "torch cached")
LAUNCHES = {"attn_decode": 0, "greedy_pick": 0}      # kernel launches so far (tests assert that a GPU run reached both kernels)

MAX_KEYS = 1024
HEAD_DIMS = (16, 64)
MAX_VOCAB = 65536


def _rows_ok(t: torch.Tensor) -> bool:
    """16-byte aligned start, unit column stride, every other stride a multiple of 8 elements"""
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1]))


def _kernel_attention_ok(q, k_cache, v_cache, num_heads, n_keys, k_new, v_new, key_mask, bias) -> bool:
    if EAGER or not q.is_cuda or q.dtype not in (torch.bfloat16, torch.float32):
        return False
    E = q.shape[-1]
    D = E // num_heads
    if D not in HEAD_DIMS or D * num_heads != E or k_cache.shape[1] > MAX_KEYS or n_keys > MAX_KEYS:
        return False
    ts = [q, k_cache, v_cache] + [t for t in (k_new, v_new) if t is not None]
    if any(t.dtype != q.dtype or not t.is_cuda or not _rows_ok(t) for t in ts):
        return False
    if k_new is not None and k_new.stride(0) != v_new.stride(0):
        return False
    if key_mask is not None and (key_mask.stride(-1) != 1 or key_mask.dtype not in (torch.bool, torch.uint8)):
        return False
    return bias is None or (bias.dtype == torch.float32 and bias.stride(-1) == 1)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, num_heads: int, *, pos: Optional[int] = None,
                     k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                     key_mask: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None) -> torch.Tensor:
    """``softmax(scale * q k^T + bias + mask) v`` for one query row per sequence: q ``[B, H*D]`` (any row stride), caches
    ``[B, Lmax, H*D]`` (unit column stride: a column block of a wider buffer is read in place).  With ``k_new`` / ``v_new``
    ``[B, H*D]`` and ``pos``: they are written into cache row ``pos`` and keys ``0..pos`` are attended (self-attention step); else
    all ``Lmax`` keys.  ``key_mask`` ``[B, Lk]`` (bool / u8, False = masked), ``bias`` ``[H, >= Lk]`` fp32 (T5's relative position
    bias row of the query position).  ``scale`` defaults to ``D**-0.5`` (BART); T5 passes 1.0.  Returns ``[B, H*D]``."""
    B, E = q.shape
    D = E // num_heads
    scale = D ** -0.5 if scale is None else float(scale)
    append = k_new is not None
    if append and pos is None:
        raise ValueError("decode_attention: k_new / v_new need the cache row `pos`")
    n_keys = pos + 1 if append else k_cache.shape[1]
    if not _kernel_attention_ok(q, k_cache, v_cache, num_heads, n_keys, k_new, v_new, key_mask, bias):
        return _torch_attention(q, k_cache, v_cache, num_heads, pos, k_new, v_new, key_mask, bias, scale)
    out = torch.empty(B, E, dtype=q.dtype, device=q.device)
    km = None
    if key_mask is not None:
        km = key_mask.view(torch.uint8) if key_mask.dtype == torch.bool else key_mask
    lib = _lib.load()
    code = lib.vlpet_attn_decode(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1),
                                 k_cache.stride(0), v_cache.stride(1), v_cache.stride(0),
                                 k_new.data_ptr() if append else None, v_new.data_ptr() if append else None,
                                 k_new.stride(0) if append else 0, pos if append else 0,
                                 None if km is None else km.data_ptr(), 0 if km is None else km.stride(0),
                                 None if bias is None else bias.data_ptr(), 0 if bias is None else bias.stride(0),
                                 out.data_ptr(), out.stride(0), B, num_heads, D, pos + 1 if append else k_cache.shape[1],
                                 scale, _io_dtype(q), _stream())
    _lib.check(code, "vlpet_attn_decode")
    LAUNCHES["attn_decode"] += 1
    return out


def _torch_attention(q, k_cache, v_cache, num_heads, pos, k_new, v_new, key_mask, bias, scale):
    """The torch form: append with an indexed copy, then host.bart.attention_core with Lq = 1 (its 1/sqrt(D) is undone on q when
    ``scale`` differs; the bias and the key mask become one additive mask)."""
    from .host import bart as HB
    B, E = q.shape
    D = E // num_heads
    if k_new is not None:
        k_cache[:, pos] = k_new
        v_cache[:, pos] = v_new
        k, v = k_cache[:, :pos + 1], v_cache[:, :pos + 1]
    else:
        k, v = k_cache, v_cache
    Lk = k.shape[1]
    mask = None
    if bias is not None:
        mask = bias[None, :, None, :Lk].to(q.dtype).expand(B, -1, -1, -1)
        if key_mask is not None:
            mask = mask.masked_fill(~key_mask[:, None, None, :Lk].bool(), float("-inf"))
    elif key_mask is not None:
        mask = key_mask[:, None, None, :Lk].bool()
    if abs(scale - D ** -0.5) > 1e-12 * scale:
        q = q * (scale * D ** 0.5)
    return HB.attention_core(q[:, None], k, v, num_heads, mask, False, 0.0, False)[:, 0]


def greedy_pick(logits: torch.Tensor, vocab: int, ids: torch.Tensor, pos: int, unfinished: torch.Tensor, counters: torch.Tensor, *,
                eos_token_id: Optional[int], pad_token_id: int, min_length: int = 0, no_repeat_ngram_size: int = 0) -> None:
    """Pick ``ids[:, pos + 1]`` from ``logits`` ``[B, >= vocab]`` (the first ``vocab`` columns count) after the reference's
    greedy processors; finished rows (``unfinished`` int32 ``[B]`` == 0) get pad; ``unfinished`` is cleared where eos is emitted and
    ``counters[pos]`` (int32, zero before the step) gets the number of rows still unfinished.  Nothing is returned or synchronised."""
    B = logits.shape[0]
    eos = -1 if eos_token_id is None else int(eos_token_id)
    ok = (not EAGER and logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float32) and logits.dim() == 2
          and _rows_ok(logits) and logits.shape[1] >= (vocab + 7) // 8 * 8 and vocab <= MAX_VOCAB and ids.is_cuda
          and ids.dtype == torch.int64 and ids.stride(1) == 1 and unfinished.dtype == torch.int32 and unfinished.is_contiguous()
          and counters.dtype == torch.int32 and counters.is_contiguous() and eos < vocab)
    if not ok:
        return _torch_pick(logits, vocab, ids, pos, unfinished, counters, eos, pad_token_id, min_length, no_repeat_ngram_size)
    lib = _lib.load()
    code = lib.vlpet_greedy_pick(logits.data_ptr(), logits.stride(0), vocab, ids.data_ptr(), ids.stride(0), pos,
                                 unfinished.data_ptr(), counters.data_ptr() + 4 * pos, B, eos, int(pad_token_id),
                                 int(min_length), int(no_repeat_ngram_size), _io_dtype(logits), _stream())
    _lib.check(code, "vlpet_greedy_pick")
    LAUNCHES["greedy_pick"] += 1


def _banned_ngram_tokens(prefix: list, n: int) -> list:
    """NoRepeatNGramLogitsProcessor (HF 4.2.1 _calc_banned_ngram_tokens) for one row: the tokens that followed every earlier
    occurrence of the row's last n - 1 tokens."""
    cur = len(prefix)
    if cur + 1 < n:
        return []
    last = prefix[cur - n + 1:]
    return [prefix[i + n - 1] for i in range(cur - n + 1) if prefix[i:i + n - 1] == last]


def _torch_pick(logits, vocab, ids, pos, unfinished, counters, eos, pad, min_length, ngram):
    scores = logits[:, :vocab].float().clone()
    cur_len = pos + 1
    if ngram > 0 and cur_len + 1 >= ngram:
        for b, prefix in enumerate(ids[:, :cur_len].tolist()):
            banned = _banned_ngram_tokens(prefix, ngram)
            if banned:
                scores[b, torch.tensor(banned, device=scores.device)] = float("-inf")
    if eos >= 0 and cur_len < min_length:
        scores[:, eos] = float("-inf")
    tok = scores.argmax(-1)
    if eos >= 0:
        tok = torch.where(unfinished.bool(), tok, torch.full_like(tok, pad))
        unfinished.mul_((tok != eos).to(unfinished.dtype))
    ids[:, cur_len] = tok
    counters[pos] += unfinished.sum().to(counters.dtype)


def greedy_generate(step: Callable[[torch.Tensor, int], torch.Tensor], vocab: int, B: int, device, max_length: int,
                    start_token_id: int, eos_token_id: Optional[int], pad_token_id: int, min_length: int = 0,
                    no_repeat_ngram_size: int = 0) -> torch.Tensor:
    """The loop of HF 4.2.1 greedy_search.  ``step(tokens [B], pos)`` runs the decoder on the token at position ``pos`` and returns
    that position's logits ``[B, >= vocab]``.  One host synchronisation per step: the count of unfinished rows."""
    ids = torch.full((B, max_length), int(pad_token_id), dtype=torch.int64, device=device)
    ids[:, 0] = int(start_token_id)
    unfinished = torch.ones(B, dtype=torch.int32, device=device)
    counters = torch.zeros(max(max_length, 1), dtype=torch.int32, device=device)
    cur_len = 1
    for pos in range(max_length - 1):
        logits = step(ids[:, pos], pos)
        greedy_pick(logits, vocab, ids, pos, unfinished, counters, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                    min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size)
        cur_len = pos + 2
        if eos_token_id is not None and int(counters[pos]) == 0:
            break
    return ids[:, :cur_len]
