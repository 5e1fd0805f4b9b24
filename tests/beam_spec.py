"""Torch restatement of HF 4.2.1 beam search with ``num_return_sequences = 1`` (test infrastructure), written from the HF 4.2.1
source semantics (generation_utils.py beam_search, generation_beam_search.py BeamSearchScorer / BeamHypotheses,
generation_logits_process.py, the reference's BartForConditionalGeneration.adjust_logits_during_generation).  Plain torch and Python
loops; ``cur_len`` is the number of tokens so far, the start token included.  tests/golden/make_beam_goldens.py decodes the
fixtures with it, tests/test_gpu_beam.py holds vlpet_beam_rows / vlpet_beam_advance to it.

One step of an item's K rows (laid out item-major, row = item * K + beam):
  1. row logits; BART at ``cur_len == max_length - 1``: every column but eos is -inf (before the log-softmax)
  2. log_softmax over the vocabulary in fp32, then the processors on the log-probs: no_repeat_ngram bans (per row, on its own
     prefix), eos banned while ``cur_len < min_length`` -- a ban does not renormalise
  3. + the row's beam score; per item the top 2K of the flat [K * V] scores, descending, ties to the lower flat index
  4. ``process``: the candidates in rank order; an eos of rank >= K is skipped, one of rank < K becomes a hypothesis (the source
     row's tokens, score sum_logprobs / cur_len ** length_penalty); a non-eos one fills the next beam slot; K slots end the walk
  5. the rows are reordered by source row and the tokens appended; the loop ends at ``max_length`` or when every item is done
  6. ``finalize``: open beams of items not done are added; each item's best hypothesis (ties: the one added last) is the output."""
import math

import torch

from generate_spec import banned_tokens

NEG_INIT = -1e9


class Hyps:
    """BeamHypotheses: at most K (score, tokens) pairs, kept in insertion order"""

    def __init__(self, K, length_penalty, early_stopping):
        self.K, self.lp, self.early = K, length_penalty, early_stopping
        self.beams = []                 # [(score, tokens list, insertion number)]
        self.worst = 1e9
        self.n_added = 0

    def __len__(self):
        return len(self.beams)

    def add(self, tokens, sum_logprobs):
        score = sum_logprobs / (len(tokens) ** self.lp)
        if len(self) < self.K or score > self.worst:
            self.beams.append((score, list(tokens), self.n_added))
            self.n_added += 1
            if len(self) > self.K:
                ranked = sorted((s, i) for i, (s, _, _) in enumerate(self.beams))     # ties: the earlier insertion goes
                del self.beams[ranked[0][1]]
                self.worst = ranked[1][0]
            else:
                self.worst = min(score, self.worst)
            return True
        return False

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self) < self.K:
            return False
        if self.early:
            return True
        return self.worst >= best_sum_logprobs / cur_len ** self.lp

    def best(self):
        """(score, tokens) of the best hypothesis; on equal scores the one added last (sorted by score, stable, then pop())"""
        return sorted(self.beams, key=lambda x: x[0])[-1][:2]


def row_scores(logits, vocab, prefixes, cur_len, eos, min_length, ngram, force_eos):
    """steps 1-2 for rows of ``logits`` [R, >= vocab]: the processed fp32 log-probs [R, vocab] (CPU)"""
    x = logits[:, :vocab].float().cpu().clone()
    if force_eos:
        keep = x[:, eos].clone()
        x.fill_(float("-inf"))
        x[:, eos] = keep
    x = torch.log_softmax(x, -1)
    for r, prefix in enumerate(prefixes):
        for t in banned_tokens(prefix, ngram):
            x[r, t] = float("-inf")
    if eos is not None and cur_len < min_length:
        x[:, eos] = float("-inf")
    return x


def top_flat(scores, n):
    """per item the top ``n`` of ``scores`` [B, K * V]: (values, flat indices), descending, ties to the lower index"""
    v, i = torch.sort(scores, dim=-1, descending=True, stable=True)
    return v[:, :n], i[:, :n]


def process(ids, top_v, top_i, vocab, K, hyps, done, eos, pad):
    """BeamSearchScorer.process.  ``ids`` [B*K, cur_len] (lists or a tensor), top_v / top_i [B, 2K].  Returns the next beam scores,
    tokens and source rows ([B*K] lists; a done item's rows get 0, pad, 0 as in HF) and updates ``hyps`` / ``done`` in place.
    Also returns the ranks of skipped eos candidates (for the fixtures' coverage checks)."""
    ids = ids.tolist() if torch.is_tensor(ids) else ids
    B = len(hyps)
    cur_len = len(ids[0])
    nscore, ntok, nsrc = [0.0] * (B * K), [pad] * (B * K), [0] * (B * K)
    skipped = []
    for b in range(B):
        if done[b]:
            continue
        slot = 0
        for rank in range(2 * K):
            s, flat = float(top_v[b, rank]), int(top_i[b, rank])
            beam, tok = flat // vocab, flat % vocab
            src = b * K + beam
            if tok == eos:
                if rank >= K:
                    skipped.append(rank)
                    continue
                hyps[b].add(ids[src], s)
            else:
                nscore[b * K + slot], ntok[b * K + slot], nsrc[b * K + slot] = s, tok, src
                slot += 1
            if slot == K:
                break
        done[b] = done[b] or hyps[b].is_done(float(top_v[b].max()), cur_len)
    return nscore, ntok, nsrc, skipped


def finalize(ids, beam_scores, hyps, done, K, max_length, eos, pad):
    """BeamSearchScorer.finalize with num_beam_hyps_to_keep = 1: (output ids [B, min(max len + 1, max_length)], scores [B])"""
    ids = ids.tolist() if torch.is_tensor(ids) else ids
    for b, h in enumerate(hyps):
        if done[b]:
            continue
        for k in range(K):
            h.add(ids[b * K + k], float(beam_scores[b * K + k]))
    best = [h.best() for h in hyps]
    lens = [len(t) for _, t in best]
    width = min(max(lens) + 1, max_length)
    out = torch.full((len(hyps), width), pad, dtype=torch.long)
    for b, (_, t) in enumerate(best):
        out[b, :len(t)] = torch.tensor(t)
        if len(t) < max_length:
            out[b, len(t)] = eos
    return out, torch.tensor([s for s, _ in best], dtype=torch.float64)


def beam_search(step_logits, vocab, B, K, start, eos, pad, max_length, min_length=0, ngram=0, length_penalty=1.0,
                early_stopping=False, force_eos=False, processed=None):
    """The whole loop.  ``step_logits(ids [B*K, cur_len] long)`` returns the last position's raw logits [B*K, >= vocab];
    ``force_eos``: BART's adjustment at cur_len == max_length - 1.  ``processed(ids, logits, cur_len)``, when given, replaces
    steps 1-2 (the fixture generator passes the reference's own adjustment and the installed processors).  Returns (ids [B, w],
    scores [B] float64, trace): trace holds per step the [B, 2K] top values / flat indices, the live flags and the skipped eos ranks."""
    ids = torch.full((B * K, 1), start, dtype=torch.long)
    beam_scores = torch.zeros(B, K)
    beam_scores[:, 1:] = NEG_INIT
    beam_scores = beam_scores.view(-1)
    hyps = [Hyps(K, length_penalty, early_stopping) for _ in range(B)]
    done = [False] * B
    trace = []
    cur_len = 1
    while cur_len < max_length:
        logits = step_logits(ids)
        if processed is not None:
            lp = processed(ids, logits, cur_len)
        else:
            lp = row_scores(logits, vocab, ids.tolist(), cur_len, eos, min_length, ngram,
                            force_eos and cur_len == max_length - 1)
        scores = (lp + beam_scores[:, None]).view(B, K * vocab)
        top_v, top_i = top_flat(scores, 2 * K)
        live = [not d for d in done]
        nscore, ntok, nsrc, skipped = process(ids, top_v, top_i, vocab, K, hyps, done, eos, pad)
        trace.append(dict(top_v=top_v.clone(), top_i=top_i.clone(), live=live, skipped=skipped, scores=scores))
        beam_scores = torch.tensor(nscore, dtype=torch.float32)
        ids = torch.cat([ids[torch.tensor(nsrc)], torch.tensor(ntok)[:, None]], 1)
        cur_len += 1
        if all(done):
            break
    out, best = finalize(ids, beam_scores, hyps, done, K, max_length, eos, pad)
    return out, best, trace, hyps


def hyp_margin(hyps):
    """the smallest gap between an item's best and second-best hypothesis (inf with one hypothesis)"""
    m = math.inf
    for h in hyps:
        s = sorted((x[0] for x in h.beams), reverse=True)
        if len(s) > 1:
            m = min(m, s[0] - s[1])
    return m
