"""Torch restatement of one greedy step of HF 4.2.1 (test infrastructure): the logits processors the reference's greedy search applies,
the argmax and the finish bookkeeping, written from the HF 4.2.1 source semantics (generation_logits_process.py:
NoRepeatNGramLogitsProcessor / _calc_banned_ngram_tokens, MinLengthLogitsProcessor; generation_utils.py greedy_search).
tests/test_gpu_generate.py holds vlpet_greedy_pick to it."""
import torch


def banned_tokens(prefix, n):
    """the tokens that followed every earlier occurrence of the last n - 1 tokens of ``prefix`` (n-grams of the whole prefix,
    the start token included)"""
    cur = len(prefix)
    if n <= 0 or cur + 1 < n:
        return set()
    gens = {}
    for i in range(cur - n + 1):
        gens.setdefault(tuple(prefix[i:i + n - 1]), []).append(prefix[i + n - 1])
    return set(gens.get(tuple(prefix[cur - n + 1:cur]), []))


def greedy_step(logits, vocab, ids, pos, unfinished, eos, pad, min_length, ngram):
    """(tokens [B], new unfinished [B]) for the step that writes ids[:, pos + 1]; ``logits`` [B, >= vocab] on any device"""
    scores = logits[:, :vocab].double().cpu().clone()
    cur_len = pos + 1
    prefixes = ids[:, :cur_len].cpu().tolist()
    for b, prefix in enumerate(prefixes):
        for t in banned_tokens(prefix, ngram):
            scores[b, t] = float("-inf")
    if eos is not None and cur_len < min_length:
        scores[:, eos] = float("-inf")
    tok = scores.argmax(-1)
    unf = unfinished.cpu().long()
    if eos is not None:
        tok = tok * unf + pad * (1 - unf)
        unf = unf * (tok != eos).long()
    return tok, unf
