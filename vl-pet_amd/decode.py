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

import collections
import itertools
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib
from .functional import _io_dtype, _stream

EAGER = False                   # A/B switch: the torch forms for every call (tools/genbench.py "torch cached")
LAUNCHES = {"attn_decode": 0, "greedy_pick": 0, "beam_rows": 0, "beam_advance": 0}   # kernel launches so far (tests assert them)

MAX_KEYS = 1024
HEAD_DIMS = (16, 64)
MAX_VOCAB = 65536
MAX_BEAMS = 8                   # num_beams 2..MAX_BEAMS on the beam kernels
MAX_GRAPHS = 8                  # captured decode steps kept by generate(graph=True) (least recently used evicted)
# generate(graph=True) so far: steps captured, steps replayed, first calls of a key (run eagerly on the device-position path) and calls
# that took the plain loop instead (CPU tensors, EAGER, an input the kernels do not take, a key whose capture failed)
GRAPH_STATS = {"captures": 0, "replays": 0, "warmups": 0, "eager": 0}


def _rows_ok(t: torch.Tensor) -> bool:
    """16-byte aligned start, unit column stride, every other stride a multiple of 8 elements"""
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1]))


def _kernel_attention_ok(q, k_cache, v_cache, num_heads, n_keys, k_new, v_new, key_mask, bias, key_rows=None) -> bool:
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
    if key_rows is not None and (key_rows.dtype != torch.int32 or not key_rows.is_cuda or key_rows.stride(-1) != 1):
        return False
    return bias is None or (bias.dtype == torch.float32 and bias.stride(-1) == 1)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, num_heads: int, *, pos: Optional[int] = None,
                     k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                     key_mask: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None, group: int = 1, key_rows: Optional[torch.Tensor] = None,
                     pos_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``softmax(scale * q k^T + bias + mask) v`` for one query row per sequence: q ``[B, H*D]`` (any row stride), caches
    ``[B, Lmax, H*D]`` (unit column stride: a column block of a wider buffer is read in place).  With ``k_new`` / ``v_new``
    ``[B, H*D]`` and ``pos``: they are written into cache row ``pos`` and keys ``0..pos`` are attended (self-attention step); else
    all ``Lmax`` keys.  ``key_mask`` ``[B, Lk]`` (bool / u8, False = masked), ``bias`` ``[H, >= Lk]`` fp32 (T5's relative position
    bias row of the query position).  ``scale`` defaults to ``D**-0.5`` (BART); T5 passes 1.0.  Returns ``[B, H*D]``.
    A ``-inf`` entry of ``bias`` means "excluded", exactly like a masked key; a (row, head) whose keys are all excluded, by the
    mask, the bias or both, gets zeros -- in the kernel and in the torch form alike.

    Beam search (``beam_generate``): ``group`` -- query row r reads cache batch ``r // group`` and key-mask row ``r // group`` (the
    cross-attention caches of an item serve its ``group`` beams, never expanded); ``key_rows`` int32 ``[B, >= n_keys]`` -- key j of
    query row r lives in cache batch ``key_rows[r, j]`` (a self-attention cache that is never reordered: the rows' histories are
    followed through the table); the appended row still goes to batch r, row ``pos``.

    ``pos_dev`` (int32 ``[1]`` on the device, the position word of a replayed step; self-attention step only) replaces ``pos``: the
    kernel reads the position from it (``vlpet_attn_decode_at``), ``bias`` is then the whole ``[positions, H, >= Lmax]`` table (row
    ``pos`` is used) and ``key_rows`` the whole ``[2, B, >= Lmax]`` ping-pong table (half ``pos % 2`` is read).  The result is
    bitwise that of the int form; a position outside ``0..Lmax-1`` writes nothing.  The torch form reads the word back."""
    if pos_dev is not None:
        return _decode_attention_at(q, k_cache, v_cache, num_heads, pos_dev, k_new, v_new, key_mask, bias, scale, group, key_rows)
    B, E = q.shape
    D = E // num_heads
    scale = D ** -0.5 if scale is None else float(scale)
    append = k_new is not None
    if append and pos is None:
        raise ValueError("decode_attention: k_new / v_new need the cache row `pos`")
    n_keys = pos + 1 if append else k_cache.shape[1]
    if append and group != 1:
        raise ValueError("decode_attention: the appended row goes to batch r; group must be 1 with k_new / v_new")
    if k_cache.shape[0] * group < B or v_cache.shape[0] * group < B:
        raise ValueError("decode_attention: the caches hold fewer than B / group batches")
    if key_rows is not None and (key_rows.shape[0] != B or key_rows.shape[1] < n_keys or k_cache.shape[0] < B):
        raise ValueError("decode_attention: key_rows must be [B, >= n_keys] over caches of B batches")
    if not _kernel_attention_ok(q, k_cache, v_cache, num_heads, n_keys, k_new, v_new, key_mask, bias, key_rows):
        return _torch_attention(q, k_cache, v_cache, num_heads, pos, k_new, v_new, key_mask, bias, scale, group, key_rows)
    out = torch.empty(B, E, dtype=q.dtype, device=q.device)
    km = None
    if key_mask is not None:
        km = key_mask.view(torch.uint8) if key_mask.dtype == torch.bool else key_mask
    args = (q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1), k_cache.stride(0),
            v_cache.stride(1), v_cache.stride(0), k_new.data_ptr() if append else None, v_new.data_ptr() if append else None,
            k_new.stride(0) if append else 0, pos if append else 0, None if km is None else km.data_ptr(),
            0 if km is None else km.stride(0), None if bias is None else bias.data_ptr(), 0 if bias is None else bias.stride(0),
            out.data_ptr(), out.stride(0), B, num_heads, D, n_keys, scale)
    lib = _lib.load()
    if group != 1 or key_rows is not None:        # the beam entry point: the same arguments, then the group and the key-row table
        code = lib.vlpet_attn_decode_beam(*args, int(group), None if key_rows is None else key_rows.data_ptr(),
                                          0 if key_rows is None else key_rows.stride(0), _io_dtype(q), _stream())
        _lib.check(code, "vlpet_attn_decode_beam")
    else:
        code = lib.vlpet_attn_decode(*args, _io_dtype(q), _stream())
        _lib.check(code, "vlpet_attn_decode")
    LAUNCHES["attn_decode"] += 1
    return out


def _pos_dev_ok(pos_dev) -> bool:
    return pos_dev.is_cuda and pos_dev.dtype == torch.int32 and pos_dev.numel() == 1


def _decode_attention_at(q, k_cache, v_cache, num_heads, pos_dev, k_new, v_new, key_mask, bias, scale, group, key_rows):
    """decode_attention with the position word: the ``vlpet_attn_decode_at`` launch, or the int form at the word's value"""
    B, E = q.shape
    D = E // num_heads
    scale = D ** -0.5 if scale is None else float(scale)
    if k_new is None or v_new is None or group != 1:
        raise ValueError("decode_attention: a device position goes with the self-attention step (k_new / v_new, group 1)")
    L = k_cache.shape[1]
    if bias is not None and (bias.dim() != 3 or bias.shape[0] < L or bias.shape[2] < L):
        raise ValueError("decode_attention: with a device position `bias` is the [positions, H, Lmax] table")
    if key_rows is not None and (key_rows.dim() != 3 or key_rows.shape[0] != 2 or key_rows.shape[1] != B or key_rows.shape[2] < L
                                 or k_cache.shape[0] < B):
        raise ValueError("decode_attention: with a device position `key_rows` is the [2, B, >= Lmax] ping-pong table")
    if not (_pos_dev_ok(pos_dev) and _kernel_attention_ok(q, k_cache, v_cache, num_heads, L, k_new, v_new, key_mask, bias, key_rows)):
        pos = int(pos_dev)
        return decode_attention(q, k_cache, v_cache, num_heads, pos=pos, k_new=k_new, v_new=v_new, key_mask=key_mask,
                                bias=None if bias is None else bias[pos], scale=scale,
                                key_rows=None if key_rows is None else key_rows[pos & 1])
    out = torch.empty(B, E, dtype=q.dtype, device=q.device)
    km = None
    if key_mask is not None:
        km = key_mask.view(torch.uint8) if key_mask.dtype == torch.bool else key_mask
    code = _lib.load().vlpet_attn_decode_at(
        q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1), k_cache.stride(0), v_cache.stride(1),
        v_cache.stride(0), k_new.data_ptr(), v_new.data_ptr(), k_new.stride(0), pos_dev.data_ptr(), L,
        None if km is None else km.data_ptr(), 0 if km is None else km.stride(0), None if bias is None else bias.data_ptr(),
        0 if bias is None else bias.stride(1), 0 if bias is None else bias.stride(0), out.data_ptr(), out.stride(0), B, num_heads,
        D, L, scale, None if key_rows is None else key_rows.data_ptr(), 0 if key_rows is None else key_rows.stride(1),
        0 if key_rows is None else key_rows.stride(0), _io_dtype(q), _stream())
    _lib.check(code, "vlpet_attn_decode_at")
    LAUNCHES["attn_decode"] += 1
    return out


def _torch_attention(q, k_cache, v_cache, num_heads, pos, k_new, v_new, key_mask, bias, scale, group=1, key_rows=None):
    """The torch form: append with an indexed copy, then host.bart.attention_core with Lq = 1 (its 1/sqrt(D) is undone on q when
    ``scale`` differs; the bias and the key mask become one additive mask).  ``group`` / ``key_rows`` gather the caches per row."""
    from .host import bart as HB
    B, E = q.shape
    D = E // num_heads
    if k_new is not None:
        k_cache[:, pos] = k_new
        v_cache[:, pos] = v_new
        k, v = k_cache[:, :pos + 1], v_cache[:, :pos + 1]
    else:
        k, v = k_cache, v_cache
    if group != 1:
        k, v = k.repeat_interleave(group, 0), v.repeat_interleave(group, 0)
        if key_mask is not None:
            key_mask = key_mask.repeat_interleave(group, 0)
    if key_rows is not None:
        n = k.shape[1]
        kr = key_rows[:, :n].long()
        if k_new is not None:
            kr = kr.clone()
            kr[:, pos] = torch.arange(B, device=kr.device)
        j = torch.arange(n, device=kr.device)[None].expand(B, n)
        k, v = k_cache[kr, j], v_cache[kr, j]
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
                eos_token_id: Optional[int], pad_token_id: int, min_length: int = 0, no_repeat_ngram_size: int = 0,
                pos_dev: Optional[torch.Tensor] = None, next_tokens: Optional[torch.Tensor] = None) -> None:
    """Pick ``ids[:, pos + 1]`` from ``logits`` ``[B, >= vocab]`` (the first ``vocab`` columns count) after the reference's
    greedy processors; finished rows (``unfinished`` int32 ``[B]`` == 0) get pad; ``unfinished`` is cleared where eos is emitted and
    ``counters[pos]`` (int32, zero before the step) gets the number of rows still unfinished.  Nothing is returned or synchronised.

    ``pos_dev`` (int32 ``[1]`` on the device) replaces ``pos`` (``vlpet_greedy_pick_at``: the same pick, bitwise); ``next_tokens``
    (int64 ``[B]``, needed with it) also gets the column written to ``ids``, so that the next step's embedding reads a fixed address.
    A position outside ``0 .. min(ids.shape[1] - 1, len(counters)) - 1`` writes nothing.  The torch form reads the word back."""
    B = logits.shape[0]
    eos = -1 if eos_token_id is None else int(eos_token_id)
    ok = (not EAGER and logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float32) and logits.dim() == 2
          and _rows_ok(logits) and logits.shape[1] >= (vocab + 7) // 8 * 8 and vocab <= MAX_VOCAB and ids.is_cuda
          and ids.dtype == torch.int64 and ids.stride(1) == 1 and unfinished.dtype == torch.int32 and unfinished.is_contiguous()
          and counters.dtype == torch.int32 and counters.is_contiguous() and eos < vocab)
    if pos_dev is not None:
        if next_tokens is None or next_tokens.shape != (B,):
            raise ValueError("greedy_pick: a device position needs next_tokens [B]")
        ok = (ok and _pos_dev_ok(pos_dev) and next_tokens.is_cuda and next_tokens.dtype == torch.int64
              and next_tokens.is_contiguous())
        if not ok:
            pos = int(pos_dev)
            _torch_pick(logits, vocab, ids, pos, unfinished, counters, eos, pad_token_id, min_length, no_repeat_ngram_size)
            next_tokens.copy_(ids[:, pos + 1])
            return
        code = _lib.load().vlpet_greedy_pick_at(
            logits.data_ptr(), logits.stride(0), vocab, ids.data_ptr(), ids.stride(0), pos_dev.data_ptr(),
            min(ids.shape[1] - 1, counters.numel()), unfinished.data_ptr(), counters.data_ptr(), next_tokens.data_ptr(), B, eos,
            int(pad_token_id), int(min_length), int(no_repeat_ngram_size), _io_dtype(logits), _stream())
        _lib.check(code, "vlpet_greedy_pick_at")
        LAUNCHES["greedy_pick"] += 1
        return
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


# ---- beam search: HF 4.2.1 beam_search with num_return_sequences = 1 (src/multitask_video.py: generate(num_beams = 5)) ----------
#
# Rows are B * K, item-major (row = item * K + beam).  The cross-attention caches stay per item (decode_attention's ``group``), the
# self-attention caches are never reordered (its ``key_rows``).  Per step two kernels follow the decoder: ``vlpet_beam_rows`` (per row
# and column slice: log-sum-exp partials and the top 2K of the logits after BART's forced eos and the bans) and
# ``vlpet_beam_advance`` (per item: the top 2K of the flat scores, BeamSearchScorer.process, the reordered ids / key rows, the next
# tokens, the count of items not done).  ``finalize`` runs once, on the host.

def _beam_slices(rows: int, vocab: int) -> int:
    """column slices per row: enough workgroups to give every CU a few (250 rows x 5 slices at the video shape), >= 1024 columns each"""
    return max(1, min(64, -(-1024 // rows), -(-vocab // 1024)))


class BeamState:
    """The device state of one beam_generate() call: ping-pong ids / key rows, beam scores, next tokens, the hypothesis table
    (K slots per item: score, (length, insertion), tokens) and per item (worst score; count, insertions, done)."""

    def __init__(self, B, K, max_length, device, start, pad, key_rows=None):
        rows = B * K
        self.B, self.K, self.L = B, K, max_length
        self.ids = torch.empty((2, rows, max_length), dtype=torch.int64, device=device)
        self.key_rows = key_rows
        self.scores = torch.empty(rows, dtype=torch.float32, device=device)
        self.tokens = torch.empty((rows,), dtype=torch.int64, device=device)
        self.hyp_score = torch.empty(rows, dtype=torch.float32, device=device)
        self.hyp_meta = torch.empty(rows, 2, dtype=torch.int32, device=device)
        self.hyp_tokens = torch.empty((rows, max_length), dtype=torch.int64, device=device)
        self.worst = torch.empty((B,), dtype=torch.float32, device=device)
        self.state = torch.empty(B, 3, dtype=torch.int32, device=device)
        self.counters = torch.empty(max(max_length, 1), dtype=torch.int32, device=device)
        self.reset(start, pad)

    def reset(self, start, pad):
        """the state of a fresh call, in place (``key_rows`` belongs to the decode state: ``reset_key_rows``)"""
        self.ids.fill_(int(pad))
        self.ids[:, :, 0] = int(start)
        sc = self.scores.view(self.B, self.K)
        sc.zero_()
        sc[:, 1:] = -1e9
        self.tokens.fill_(int(start))
        self.hyp_score.zero_()
        self.hyp_meta.zero_()
        self.hyp_tokens.fill_(int(pad))
        self.worst.fill_(1e9)
        self.state.zero_()
        self.counters.zero_()


def beam_key_rows(rows: int, max_length: int, device) -> torch.Tensor:
    """the ping-pong key-row tables [2, rows, max_length] int32 of a fresh call: every key in the row's own cache batch"""
    return torch.arange(rows, dtype=torch.int32, device=device).view(1, rows, 1).expand(2, rows, max_length).contiguous()


def reset_key_rows(key_rows: torch.Tensor) -> None:
    """``beam_key_rows`` again, in place"""
    rows = key_rows.shape[1]
    key_rows.copy_(torch.arange(rows, dtype=torch.int32, device=key_rows.device).view(1, rows, 1))


class DecodeState(NamedTuple):
    """The caches of one generate() call.  ``layers``: per decoder layer ``(self_k, self_v, cross_k, cross_v)`` -- self-attention
    caches [B * group, max_length, E] filled row by row, cross-attention caches [B, Lk, E] of the encoder output, kept per item.
    Once per call: ``key_mask`` [B, Lk] of the encoder output (or None), ``group`` (beams per item; 1 = greedy), ``key_rows`` (the
    ping-pong key-row tables of beam search, ``beam_key_rows``; None = greedy) and ``bias_table`` (T5: fp32 [max_length, H,
    max_length], row ``pos`` = the relative position bias of query position ``pos``; else None).  ``pos_dev``: the position word
    (int32 [1] on the device) of a replayed step -- with it the decoders' ``step`` ignores its int ``pos``: the self-attention
    launches, BART's learned position and the pick / beam step all read the word; None (every plain call) = the int path."""
    layers: list
    key_mask: Optional[torch.Tensor]
    group: int
    key_rows: Optional[torch.Tensor]
    bias_table: Optional[torch.Tensor]
    pos_dev: Optional[torch.Tensor] = None


def new_decode_state(enc: torch.Tensor, width: int, max_length: int, cross_k, cross_v, key_mask, num_beams: int = 1,
                     bias_table: Optional[torch.Tensor] = None) -> DecodeState:
    """The state of a fresh call over the encoder output ``enc`` [B, Lk, d]: ONE allocation [n, 2, B * num_beams, max_length, width]
    holds every layer's self-attention caches; ``cross_k`` / ``cross_v`` are the layers' projected cross-attention keys / values."""
    B, n = enc.shape[0], len(cross_v)
    selfc = enc.new_empty(n, 2, B * num_beams, max_length, width)
    key_rows = beam_key_rows(B * num_beams, max_length, enc.device) if num_beams > 1 else None
    return DecodeState([(selfc[i, 0], selfc[i, 1], cross_k[i], cross_v[i]) for i in range(n)], key_mask, num_beams, key_rows,
                       bias_table)


def beam_step(logits: torch.Tensor, vocab: int, st: BeamState, pos: int, *, eos_token_id: int, pad_token_id: int,
              min_length: int = 0, no_repeat_ngram_size: int = 0, length_penalty: float = 1.0, early_stopping: bool = False,
              force_eos: bool = False, slices: Optional[int] = None, pos_dev: Optional[torch.Tensor] = None,
              force_eos_pos: int = -1) -> None:
    """One step after the decoder: ``logits`` [B*K, >= vocab] of position ``pos``; reads ``st.ids[pos % 2]`` / ``st.key_rows[pos % 2]``
    and writes the other halves, the beam scores, ``st.tokens`` and ``st.counters[pos]`` (items not done).  Nothing is synchronised.

    ``pos_dev`` (int32 ``[1]`` on the device) replaces ``pos`` (``vlpet_beam_rows_at`` / ``vlpet_beam_advance_at``: the same step,
    bitwise) and ``force_eos_pos`` replaces ``force_eos``: the position of BART's forced step, -1 for never.  A position outside
    ``0..st.L-2`` writes nothing.  The torch form reads the word back."""
    rows, K = logits.shape[0], st.K
    kr = st.key_rows
    ok = (not EAGER and logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float32) and logits.dim() == 2
          and _rows_ok(logits) and logits.shape[1] >= (vocab + 7) // 8 * 8 and vocab <= MAX_VOCAB and 2 <= K <= MAX_BEAMS
          and rows == st.B * K and 0 <= eos_token_id < vocab and st.ids.is_cuda
          and (kr is None or (kr.is_cuda and kr.dtype == torch.int32 and kr.is_contiguous()))
          and (pos_dev is None or (_pos_dev_ok(pos_dev) and st.ids.stride(2) == 1)))
    if not ok:
        if pos_dev is not None:
            pos, force_eos = int(pos_dev), int(pos_dev) == force_eos_pos
        return _torch_beam_step(logits, vocab, st, pos, eos_token_id, pad_token_id, min_length, no_repeat_ngram_size,
                                length_penalty, early_stopping, force_eos)
    S = _beam_slices(rows, vocab) if slices is None else int(slices)
    T = 2 * K
    ws = getattr(st, "_ws", None)
    if ws is None or ws[0].shape[0] != rows * S * 2:
        ws = (torch.empty(rows * S * 2, dtype=torch.float32, device=logits.device),
              torch.empty(rows * S * T, dtype=torch.float32, device=logits.device),
              torch.empty(rows * S * T, dtype=torch.int32, device=logits.device))
        st._ws = ws
    stats, val, tok = ws
    lib = _lib.load()
    if pos_dev is not None:
        ids = st.ids
        limit = min(ids.shape[2] - 1, st.hyp_tokens.shape[1], st.counters.numel(), ids.shape[2] if kr is None else kr.shape[2] - 1)
        code = lib.vlpet_beam_rows_at(logits.data_ptr(), logits.stride(0), vocab, ids.data_ptr(), ids.stride(1), ids.stride(0),
                                      pos_dev.data_ptr(), limit, rows, K, S, int(eos_token_id), int(min_length),
                                      int(no_repeat_ngram_size), int(force_eos_pos), stats.data_ptr(), val.data_ptr(),
                                      tok.data_ptr(), _io_dtype(logits), _stream())
        _lib.check(code, "vlpet_beam_rows_at")
        LAUNCHES["beam_rows"] += 1
        code = lib.vlpet_beam_advance_at(stats.data_ptr(), val.data_ptr(), tok.data_ptr(), S, vocab, st.B, K, st.scores.data_ptr(),
                                         ids.data_ptr(), ids.stride(1), ids.stride(0), None if kr is None else kr.data_ptr(),
                                         0 if kr is None else kr.stride(1), 0 if kr is None else kr.stride(0),
                                         st.tokens.data_ptr(), st.hyp_score.data_ptr(), st.hyp_meta.data_ptr(),
                                         st.hyp_tokens.data_ptr(), st.hyp_tokens.stride(0), st.worst.data_ptr(), st.state.data_ptr(),
                                         st.counters.data_ptr(), pos_dev.data_ptr(), limit, int(eos_token_id), int(pad_token_id),
                                         float(length_penalty), int(bool(early_stopping)), _stream())
        _lib.check(code, "vlpet_beam_advance_at")
        LAUNCHES["beam_advance"] += 1
        return
    src, dst = pos & 1, (pos + 1) & 1
    ids_in, ids_out = st.ids[src], st.ids[dst]
    code = lib.vlpet_beam_rows(logits.data_ptr(), logits.stride(0), vocab, ids_in.data_ptr(), ids_in.stride(0), pos, rows, K, S,
                               int(eos_token_id), int(min_length), int(no_repeat_ngram_size), int(bool(force_eos)),
                               stats.data_ptr(), val.data_ptr(), tok.data_ptr(), _io_dtype(logits), _stream())
    _lib.check(code, "vlpet_beam_rows")
    LAUNCHES["beam_rows"] += 1
    code = lib.vlpet_beam_advance(stats.data_ptr(), val.data_ptr(), tok.data_ptr(), S, vocab, st.B, K, st.scores.data_ptr(),
                                  ids_in.data_ptr(), ids_out.data_ptr(), ids_in.stride(0),
                                  None if kr is None else kr[src].data_ptr(), None if kr is None else kr[dst].data_ptr(),
                                  0 if kr is None else kr.stride(1), st.tokens.data_ptr(), st.hyp_score.data_ptr(),
                                  st.hyp_meta.data_ptr(), st.hyp_tokens.data_ptr(), st.hyp_tokens.stride(0), st.worst.data_ptr(),
                                  st.state.data_ptr(), st.counters.data_ptr() + 4 * pos, pos, int(eos_token_id),
                                  int(pad_token_id), float(length_penalty), int(bool(early_stopping)), _stream())
    _lib.check(code, "vlpet_beam_advance")
    LAUNCHES["beam_advance"] += 1


def _torch_beam_rows(logits, vocab, ids, pos, eos, min_length, ngram, force_eos):
    """the processed fp32 log-probs [rows, vocab]: BART's forced eos, log_softmax, then the bans (no renormalisation).
    The softmax runs on rows padded with -inf columns to a multiple of 8 (exp(-inf) = 0: the sum is the same): torch's device
    kernel orders a row's sum by the row's alignment, and with an odd vocab (50265) two bitwise identical rows would otherwise get
    log-probs one ulp apart -- an exact cross-beam tie must stay one, to be ordered by index as the kernels and HF's CPU form do."""
    x = logits.new_full((logits.shape[0], (vocab + 7) // 8 * 8), float("-inf"), dtype=torch.float32)
    if force_eos:
        x[:, eos] = logits[:, eos]
    else:
        x[:, :vocab] = logits[:, :vocab]
    x = torch.log_softmax(x, -1)[:, :vocab]
    cur_len = pos + 1
    if ngram > 0 and cur_len + 1 >= ngram:
        for r, prefix in enumerate(ids[:, :cur_len].tolist()):
            banned = _banned_ngram_tokens(prefix, ngram)
            if banned:
                x[r, torch.tensor(banned, device=x.device)] = float("-inf")
    if cur_len < min_length:
        x[:, eos] = float("-inf")
    return x


class _Hyps:
    """an item's hypothesis table on the host (the torch forms and finalize): K slots of (score, insertion, tokens)"""

    def __init__(self, K, lp, early, beams, worst, n_added):
        self.K, self.lp, self.early = K, lp, early
        self.beams, self.worst, self.n_added = beams, worst, n_added

    def add(self, tokens, sum_logprobs):
        score = sum_logprobs / (len(tokens) ** self.lp)
        if len(self.beams) < self.K or score > self.worst:
            if len(self.beams) < self.K:
                self.beams.append([score, self.n_added, list(tokens)])
                self.worst = min(score, self.worst)
            else:
                at = min(range(self.K), key=lambda j: (self.beams[j][0], self.beams[j][1]))
                self.beams[at] = [score, self.n_added, list(tokens)]
                self.worst = min(b[0] for b in self.beams)
            self.n_added += 1

    def is_done(self, best, cur_len):
        return len(self.beams) >= self.K and (self.early or self.worst >= best / cur_len ** self.lp)


def _load_hyps(st, lp, early):
    """the hypothesis tables of ``st`` as host objects (slot order kept)"""
    hs, hm = st.hyp_score.tolist(), st.hyp_meta.tolist()
    ht, worst, state = st.hyp_tokens.tolist(), st.worst.tolist(), st.state.tolist()
    K = st.K
    out = []
    for b in range(st.B):
        cnt, nadd, _ = state[b]
        beams = [[hs[b * K + j], hm[b * K + j][1], ht[b * K + j][:hm[b * K + j][0]]] for j in range(cnt)]
        out.append(_Hyps(K, lp, early, beams, worst[b], nadd))
    return out


def _store_hyps(st, hyps, done):
    K = st.K
    for b, h in enumerate(hyps):
        for j, (score, order, toks) in enumerate(h.beams):
            r = b * K + j
            st.hyp_score[r] = score
            st.hyp_meta[r, 0] = len(toks)
            st.hyp_meta[r, 1] = order
            st.hyp_tokens[r, :len(toks)] = torch.tensor(toks, dtype=torch.int64)
        st.worst[b] = h.worst
        st.state[b, 0] = len(h.beams)
        st.state[b, 1] = h.n_added
        st.state[b, 2] = int(done[b])


def _torch_beam_step(logits, vocab, st, pos, eos, pad, min_length, ngram, lp, early, force_eos):
    """The torch form of beam_step: the same state, BeamSearchScorer.process in a host loop over the items"""
    B, K = st.B, st.K
    src, dst = pos & 1, (pos + 1) & 1
    cur_len = pos + 1
    ids_in = st.ids[src]
    x = _torch_beam_rows(logits, vocab, ids_in, pos, eos, min_length, ngram, force_eos)
    scores = (x + st.scores[:, None]).view(B, K * vocab)
    top_v, top_i = torch.sort(scores, dim=-1, descending=True, stable=True)
    top_v, top_i = top_v[:, :2 * K].tolist(), top_i[:, :2 * K].tolist()
    hyps = _load_hyps(st, lp, early)
    done = [bool(d) for d in st.state[:, 2].tolist()]
    prefixes = ids_in[:, :cur_len].tolist()
    nscore, ntok, nsrc = st.scores.tolist(), [pad] * (B * K), list(range(B * K))
    for b in range(B):
        if done[b]:
            continue
        slot = 0
        for rank in range(2 * K):
            s, flat = top_v[b][rank], top_i[b][rank]
            beam, tok = flat // vocab, flat % vocab
            if tok == eos:
                if rank >= K:
                    continue
                hyps[b].add(prefixes[b * K + beam], s)
            else:
                nscore[b * K + slot], ntok[b * K + slot], nsrc[b * K + slot] = s, tok, b * K + beam
                slot += 1
            if slot == K:
                break
        done[b] = hyps[b].is_done(top_v[b][0], cur_len)
    dev = st.ids.device
    idx = torch.tensor(nsrc, device=dev)
    tok = torch.tensor(ntok, dtype=torch.int64, device=dev)
    st.ids[dst, :, :cur_len] = ids_in[idx, :cur_len]
    st.ids[dst, :, cur_len] = tok
    if st.key_rows is not None:
        st.key_rows[dst, :, :cur_len] = st.key_rows[src][idx, :cur_len]
        st.key_rows[dst, :, cur_len] = torch.arange(B * K, dtype=torch.int32, device=dev)
    st.scores.copy_(torch.tensor(nscore, dtype=torch.float32))
    st.tokens.copy_(tok)
    _store_hyps(st, hyps, done)
    st.counters[pos] += sum(1 for d in done if not d)


def beam_finalize(st: BeamState, cur_len: int, vocab: int, eos_token_id: int, pad_token_id: int, length_penalty: float,
                  early_stopping: bool):
    """BeamSearchScorer.finalize (num_beam_hyps_to_keep = 1): the open beams of items not done are added, each item's best
    hypothesis (ties: the one added last) becomes its output.  Returns (ids [B, min(max len + 1, max_length)], scores [B] fp32)."""
    hyps = _load_hyps(st, length_penalty, early_stopping)
    done = st.state[:, 2].tolist()
    final = st.ids[(cur_len - 1) & 1][:, :cur_len].tolist()
    bs = st.scores.tolist()
    K = st.K
    best = []
    for b, h in enumerate(hyps):
        if not done[b]:
            for k in range(K):
                h.add(final[b * K + k], bs[b * K + k])
        best.append(max(h.beams, key=lambda x: (x[0], x[1])))
    lens = [len(t) for _, _, t in best]
    width = min(max(lens) + 1, st.L)
    out = torch.full((st.B, width), int(pad_token_id), dtype=torch.int64)
    for b, (_, _, t) in enumerate(best):
        out[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
        if len(t) < st.L:
            out[b, len(t)] = int(eos_token_id)
    dev = st.ids.device
    return out.to(dev), torch.tensor([s for s, _, _ in best], dtype=torch.float32, device=dev)


def beam_generate(step: Callable[[torch.Tensor, int], torch.Tensor], vocab: int, B: int, num_beams: int, device, max_length: int,
                  start_token_id: int, eos_token_id: int, pad_token_id: int, min_length: int = 0, no_repeat_ngram_size: int = 0,
                  length_penalty: float = 1.0, early_stopping: bool = False, force_eos: bool = False,
                  key_rows: Optional[torch.Tensor] = None):
    """The loop of HF 4.2.1 beam_search.  ``step(tokens [B*K], pos)`` runs the decoder on the rows' tokens at ``pos`` and returns
    their logits [B*K, >= vocab]; it follows ``key_rows[pos % 2]`` (``beam_key_rows``) when the caches use them.  ``force_eos``:
    BART's adjust_logits_during_generation (every column but eos at -inf when cur_len == max_length - 1).  One host
    synchronisation per step: the count of items not done.  Returns (ids [B, <= max_length], sequence scores [B])."""
    if eos_token_id is None:
        raise ValueError("beam search needs an eos token")
    st = BeamState(B, num_beams, max_length, device, start_token_id, pad_token_id, key_rows)
    cur_len = 1
    for pos in range(max_length - 1):
        logits = step(st.tokens, pos)
        beam_step(logits, vocab, st, pos, eos_token_id=int(eos_token_id), pad_token_id=int(pad_token_id), min_length=min_length,
                  no_repeat_ngram_size=no_repeat_ngram_size, length_penalty=length_penalty, early_stopping=early_stopping,
                  force_eos=force_eos and pos + 1 == max_length - 1)
        cur_len = pos + 2
        if int(st.counters[pos]) == 0:
            break
    return beam_finalize(st, cur_len, vocab, eos_token_id, pad_token_id, length_penalty, early_stopping)


def generate(step: Callable[[torch.Tensor, int], torch.Tensor], vocab: int, B: int, device, key_rows: Optional[torch.Tensor],
             start_token_id: int, eos_token_id: Optional[int], pad_token_id: int, max_length: int, min_length: int = 0,
             no_repeat_ngram_size: int = 0, num_beams: int = 1, length_penalty: float = 1.0, early_stopping: bool = False,
             force_eos: bool = False) -> torch.Tensor:
    """The driver behind ``VLBart.generate`` / ``VLT5.generate``: beam search for ``num_beams`` > 1 (over ``key_rows``, the state's
    tables), else greedy search.  Returns the ids [B, <= max_length].  (Both loops are looked up in this module when called.)"""
    if num_beams > 1:
        return beam_generate(step, vocab, B, num_beams, device, max_length, start_token_id, eos_token_id, pad_token_id, min_length,
                             no_repeat_ngram_size, length_penalty, early_stopping, force_eos=force_eos, key_rows=key_rows)[0]
    return greedy_generate(step, vocab, B, device, max_length, start_token_id, eos_token_id, pad_token_id, min_length,
                           no_repeat_ngram_size)


# ---- generate(graph=True): one captured decode step per shape, replayed ----------------------------------------------------------
#
# A step's launches read the position from ``DecodeState.pos_dev`` (the *_at kernels, BART's position gather) and the step's last
# operation advances the word, so the launches of one step are the launches of every step: captured once (``torch.cuda.graph``, one
# stream, no branches) and replayed.  An entry owns every buffer the captured launches touch; a call copies the encoder's side (cross
# caches, key mask) in, resets the rest, and replays until the per-step counter -- the one host read of the plain loop -- says stop.

_GRAPHS: "collections.OrderedDict[tuple, _GraphEntry]" = collections.OrderedDict()
# Test / measurement instrument: called as GRAPH_STEP_HOOK(entry, pos) after every step of a graph_generate() call, replayed or
# eager, before the host reads the step's counter.  ``entry.logits`` is the step's logits: under replay the captured step's own
# output buffer, which the next replay overwrites.
GRAPH_STEP_HOOK: Optional[Callable] = None


def clear_graphs() -> None:
    """drop every captured decode step and its static buffers (and the models they keep alive)"""
    _GRAPHS.clear()


class GenSettings(NamedTuple):
    """what ``generate`` bakes into a step's launches (part of the graph key)"""
    start: int
    eos: Optional[int]
    pad: int
    max_length: int
    min_length: int
    ngram: int
    num_beams: int
    length_penalty: float
    early_stopping: bool
    force_eos: bool


class _GraphEntry:
    """The static side of one key: the decode state (self caches, cross caches, key mask, key rows, bias table, position word), the
    ids / unfinished / counters / next tokens of greedy search or the BeamState, and the captured step once there is one."""

    def __init__(self, model, state: DecodeState, make_step, vocab: int, gs: GenSettings):
        kx = state.layers[0][2]
        dev, B = kx.device, kx.shape[0]
        self.model = model                  # (an entry keeps its model alive -- the step's closure does anyway -- until it is evicted)
        self.gs, self.vocab, self.B = gs, vocab, B
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        layers = [(ks, vs, torch.empty(kx.shape, dtype=kx.dtype, device=dev), torch.empty(vx.shape, dtype=vx.dtype, device=dev))
                  for ks, vs, kx, vx in state.layers]           # (the first call's own self caches, key rows and bias table are kept)
        self.state = state._replace(layers=layers, key_mask=None if state.key_mask is None else torch.empty_like(state.key_mask),
                                    pos_dev=self.pos)
        self.step = make_step(self.state)
        L = gs.max_length
        if gs.num_beams > 1:
            self.beam = BeamState(B, gs.num_beams, L, dev, gs.start, gs.pad, self.state.key_rows)
            self.counters = self.beam.counters
        else:
            self.beam = None
            self.ids = torch.empty(B, L, dtype=torch.int64, device=dev)
            self.unfinished = torch.empty(B, dtype=torch.int32, device=dev)
            self.counters = torch.empty(max(L, 1), dtype=torch.int32, device=dev)
            self.tokens = torch.empty(B, dtype=torch.int64, device=dev)
        self.graph, self.calls, self.failed, self.steps, self.logits = None, 0, False, 0, None

    def load(self, state: DecodeState):
        """a call's encoder side into the static buffers, everything else back to the state of a fresh call"""
        src = [t for l in state.layers for t in l[2:]]
        dst = [t for l in self.state.layers for t in l[2:]]
        if state.key_mask is not None:
            src.append(state.key_mask)
            dst.append(self.state.key_mask)
        torch._foreach_copy_(dst, src)
        gs = self.gs
        if self.beam is not None:
            self.beam.reset(gs.start, gs.pad)
            reset_key_rows(self.state.key_rows)
        else:
            self.ids.fill_(gs.pad)
            self.ids[:, 0] = gs.start
            self.unfinished.fill_(1)
            self.counters.zero_()
            self.tokens.fill_(gs.start)
        self.pos.zero_()

    def fail(self):
        """this key stays on the plain loop: nothing here is used again, so the static buffers and the model go now, not at eviction"""
        self.failed = True
        self.model = self.state = self.step = self.beam = self.graph = self.logits = None
        self.ids = self.unfinished = self.counters = self.tokens = self.pos = None

    def one_step(self):
        """decoder + pick (or beam step) + position advance: what a capture records"""
        gs = self.gs
        if self.beam is not None:
            logits = self.step(self.beam.tokens, None)
            beam_step(logits, self.vocab, self.beam, None, eos_token_id=int(gs.eos), pad_token_id=gs.pad, min_length=gs.min_length,
                      no_repeat_ngram_size=gs.ngram, length_penalty=gs.length_penalty, early_stopping=gs.early_stopping,
                      pos_dev=self.pos, force_eos_pos=gs.max_length - 2 if gs.force_eos else -1)
        else:
            logits = self.step(self.tokens, None)
            greedy_pick(logits, self.vocab, self.ids, None, self.unfinished, self.counters, eos_token_id=gs.eos,
                        pad_token_id=gs.pad, min_length=gs.min_length, no_repeat_ngram_size=gs.ngram, pos_dev=self.pos,
                        next_tokens=self.tokens)
        self.pos.add_(1)
        self.logits = logits                # (captured: the graph's output buffer, kept alive by this reference)

    def kernels_per_step(self) -> int:
        return 2 * len(self.state.layers) + (2 if self.beam is not None else 1)

    def capture(self) -> bool:
        """record one step (train.Trainer._capture's discipline: timers off, nothing inside waits for the device)"""
        from . import functional as VF
        timer, VF.TIMER = VF.TIMER, None
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.one_step()
        except Exception as e:
            import warnings                 # (once per key: a failed key never captures again)
            warnings.warn(f"vl-pet_amd: capturing the decode step failed ({type(e).__name__}: {e}); generate(graph=True) runs this "
                          "shape with eager launches")
            self.fail()
            torch.cuda.synchronize()
            return False
        finally:
            VF.TIMER = timer
        self.graph = g
        GRAPH_STATS["captures"] += 1
        return True

    def run(self):
        """the loop of greedy_generate / beam_generate over the static state: a replay (or, before there is a graph, the same
        launches issued eagerly) per step, then the one host read"""
        gs = self.gs
        cur_len = 1
        for pos in range(gs.max_length - 1):
            if self.graph is not None:
                self.graph.replay()
                GRAPH_STATS["replays"] += 1
            else:
                self.one_step()
            if GRAPH_STEP_HOOK is not None:
                GRAPH_STEP_HOOK(self, pos)
            cur_len = pos + 2
            if gs.eos is not None and int(self.counters[pos]) == 0:
                break
        self.steps = cur_len - 1
        if self.beam is not None:
            return beam_finalize(self.beam, cur_len, self.vocab, gs.eos, gs.pad, gs.length_penalty, gs.early_stopping)
        return self.ids[:, :cur_len].clone(), None


def _graph_eligible(state: DecodeState, vocab: int, num_heads: int, head: torch.Tensor, gs: GenSettings) -> bool:
    """whether every launch of a step would take its kernel (the warm-up call's launch count settles what this cannot see)"""
    ks, _, kx, vx = state.layers[0]
    E = ks.shape[-1]
    if EAGER or not kx.is_cuda or kx.dtype not in (torch.bfloat16, torch.float32) or gs.max_length < 2:
        return False
    if E % num_heads or E // num_heads not in HEAD_DIMS or max(gs.max_length, kx.shape[1]) > MAX_KEYS or vocab > MAX_VOCAB:
        return False
    if head.shape[0] < (vocab + 7) // 8 * 8 or any(not _rows_ok(t) for l in state.layers for t in l):
        return False
    if gs.num_beams > 1:
        return gs.num_beams <= MAX_BEAMS and gs.eos is not None and 0 <= gs.eos < vocab
    return gs.eos is None or gs.eos < vocab


def graph_generate(model, state: DecodeState, make_step: Callable[[DecodeState], Callable], vocab: int, num_heads: int,
                   head: torch.Tensor, gs: GenSettings, key_extra: tuple = ()):
    """``generate`` with the decode step replayed from a captured graph.  ``state``: the call's fresh decode state (its encoder side is
    copied into the entry's); ``make_step(state)`` builds the ``step(tokens, pos)`` of a state; ``head``: the padded LM head the step
    multiplies by.  The first call of a key runs the device-position launches eagerly (warm-up: weight caches, library workspaces),
    the second captures one step, from then on every step is a replay.  Anything a step's kernels do not take: the plain loop.
    Returns (ids, sequence scores or None)."""
    from . import functional as VF

    def plain():
        GRAPH_STATS["eager"] += 1
        kx = state.layers[0][2]
        step = make_step(state)
        if gs.num_beams > 1:
            return beam_generate(step, vocab, kx.shape[0], gs.num_beams, kx.device, gs.max_length, gs.start, gs.eos, gs.pad,
                                 gs.min_length, gs.ngram, gs.length_penalty, gs.early_stopping, force_eos=gs.force_eos,
                                 key_rows=state.key_rows)
        return greedy_generate(step, vocab, kx.shape[0], kx.device, gs.max_length, gs.start, gs.eos, gs.pad, gs.min_length,
                               gs.ngram), None

    if not _graph_eligible(state, vocab, num_heads, head, gs):
        return plain()
    kx = state.layers[0][2]
    shape = (id(model), model.training, kx.device, kx.dtype, kx.shape[0], kx.shape[1], state.key_mask is not None, gs,
             tuple(key_extra))
    key = shape + (VF.FROZEN_EPOCH, VF.WEIGHTS_EPOCH,
                   tuple(t._version for t in itertools.chain(model.parameters(), model.buffers())))
    ent = _GRAPHS.get(key)
    if ent is None:
        for k in [k for k in _GRAPHS if k[:len(shape)] == shape]:       # the same call over changed weights: that graph is dead
            del _GRAPHS[k]
        while len(_GRAPHS) >= max(1, int(MAX_GRAPHS)):
            _GRAPHS.popitem(last=False)
        ent = _GRAPHS[key] = _GraphEntry(model, state, make_step, vocab, gs)
    else:
        _GRAPHS.move_to_end(key)
    if ent.failed:
        return plain()
    ent.calls += 1
    if ent.graph is None and ent.calls >= 2 and not ent.capture():
        return plain()
    ent.load(state)
    if ent.graph is not None:
        return ent.run()
    GRAPH_STATS["warmups"] += 1
    before = sum(LAUNCHES.values())
    out = ent.run()
    if sum(LAUNCHES.values()) - before != ent.steps * ent.kernels_per_step():
        ent.fail()                                              # some launch took a torch form: nothing to capture
    return out
