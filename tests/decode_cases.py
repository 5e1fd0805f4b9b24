"""Input builders and the step-by-step reference of the decode-kernel edge tests (test infrastructure, like gpu_cases.py):
tests/test_decode_ties.py (CPU: the inputs meet their conditions on the reference alone; the torch form against the spec) and
tests/test_gpu_decode_edges.py (vlpet_beam_rows / vlpet_beam_advance / vlpet_greedy_pick / vlpet_attn_decode at their edges).

  * ``tie_logits``: logits on a grid that bf16 holds exactly, so a row repeats its top values and bf16 and fp32 tables are the same
    numbers; ``plant_ties`` puts exact top ties at columns that straddle every unit the kernels split a row into;
  * ``SpecBeam``: beam_spec (row_scores / top_flat / process) driven one step at a time from a fresh or a planted state, with the
    carried-over rows of a done item as decode.beam_step documents them; ``assert_state_matches_spec`` holds a BeamState to it;
  * ``decision_margin``: the smallest non-zero gap of any decision the reference takes by value (float64 on the trace).  A run
    whose margin is well above the fp32 noise of a log-sum-exp has one right answer: ties resolve by index, the rest by value;
  * ``ref_attention64``: fp64 attention of one query row per sequence; a row with every key excluded is zeros."""
import math

import torch

import beam_spec as BS
from generate_spec import banned_tokens

START, PAD, EOS = 2, 1, 3
TOP = 16.0                       # planted top values: above the +-15 clamp of the draw; multiples of 1/8 below 32 are exact in bf16
KINDS = ("group", "lane", "slice", "cut", "eos_first", "last", "wave", "eos_second", "stride")

# The committed beam tie cases: (V, K, B, L, grid, seed).  Seeds chosen on the reference alone (tests/test_decode_ties.py: the
# decision margin and the tie count hold for both early_stopping values); V = 500 on the 1/4 grid, the real vocabularies on 1/8.
TIE_CASES_SMALL = [(500, 2, 3, 8, 0.25, 1), (500, 3, 3, 8, 0.25, 1), (500, 4, 3, 8, 0.25, 2), (500, 5, 3, 8, 0.25, 2),
                   (500, 6, 2, 8, 0.25, 1), (500, 7, 2, 8, 0.25, 1), (500, 8, 2, 8, 0.25, 5)]
TIE_CASES_LARGE = [(50265, 5, 4, 8, 0.125, 5), (50265, 8, 3, 8, 0.125, 10), (32100, 5, 4, 8, 0.125, 2), (32100, 8, 3, 8, 0.125, 7)]
TIE_SLICES = {500: (None, 1, 3), 50265: (None, 1, 7), 32100: (None, 1, 7)}
TIE_SETTINGS = dict(min_length=3, ngram=2, lp=0.8)

# planted states (long prefixes): (K, pos, seed) at B = 4, L = 320, V = 500, no_repeat_ngram_size = 3
LONG_B, LONG_L, LONG_V, LONG_NGRAM, LONG_LP = 4, 320, 500, 3, 0.8
LONG_CASES = [(K, pos, 2) for K in (3, 5) for pos in (63, 64, 65, 130, 300)]
LATE_BAN = (20, 21, 22)          # planted_beam_state: beam 1's last two tokens occurred once before, 20 positions back, followed by 22


def padded_width(V):
    return (V + 7) // 8 * 8 + 8


def slice_cols(V, S):
    """the columns per slice of vlpet_beam_rows (a multiple of 8)"""
    return ((V + S - 1) // S + 7) // 8 * 8


def slice_boundaries(V, rows):
    """the first slice boundary of every slice count the case runs with (None = decode._beam_slices)"""
    from vlpet_amd.decode import _beam_slices
    out = []
    for S in TIE_SLICES[V]:
        S = _beam_slices(rows, V) if S is None else S
        if S > 1:
            out.append(slice_cols(V, S))
    return sorted(set(out))


def tie_logits(rows, V, Vp, grid, gen, dtype):
    """randn * 3 rounded to a multiple of ``grid`` (>= 1/8) and clamped to +-15: every value is exact in bf16.  Padding columns
    V..Vp-1 are +inf (they never count)."""
    x = torch.randn(rows, Vp, generator=gen) * 3
    x = (torch.round(x / grid) * grid).clamp_(-15.0, 15.0).to(dtype)
    x[:, V:] = float("inf")
    return x


def plant_ties(row, V, K, eos, kind, c, boundaries, value=TOP):
    """equal top values in ``row`` [>= V] at columns that straddle one unit of the kernels' split of a row (c: a multiple of 8,
    >= 16).  Returns the planted columns.  A kind that does not fit the vocabulary falls back to "lane"."""
    if kind == "slice" and boundaries:
        b = boundaries[(c // 8) % len(boundaries)]
        cols = [b - 1, b]                                            # the last column of one slice, the first of the next
    elif kind == "group":
        cols = [c, c + 1]                                            # one 16-byte load
    elif kind == "wave":
        cols = [c, c + 8 * 64]                                       # the same lane of two waves
    elif kind == "stride":
        cols = [c, c + 8 * 256]                                      # one thread's consecutive loads (GP_U)
    elif kind == "last":
        cols = [c, V - 1]                                            # the last valid column (V % 8 = 1 and 4 at the real sizes)
    elif kind == "eos_first":
        cols = [eos, c]                                              # eos wins the tie
    elif kind == "eos_second":
        cols = [0, eos]                                              # eos loses it
    elif kind == "cut":
        cols = [c + 1 + i * ((V - c - 2) // (2 * K + 1)) for i in range(2 * K + 1)]    # the cut at rank 2K falls inside the tie
    else:
        cols = [c, c + 8]
    if max(cols) >= V or len(set(cols)) != len(cols):
        cols = [c, c + 8]                                            # two neighbouring lanes
    row[cols] = value
    return cols


def beam_tie_tables(V, K, B, L, grid, seed):
    """the fp32 master tables of one case, one [B * K, Vp] per step: the grid draw; eos high in the rows of every other item
    (hypotheses, done items); beam 0 of every item gets one planted tie per step, the kinds cycling over steps and items; item 0
    gets the one cross-beam exact tie: its step-0 plant is a pair, whose two survivors (beams 0 and 1, bitwise equal scores) read
    bitwise identical rows at step 1.  No other two rows of an item are alike."""
    gen = torch.Generator().manual_seed(seed)
    Vp = padded_width(V)
    bounds = slice_boundaries(V, B * K)
    tables = []
    for step in range(L - 1):
        x = tie_logits(B * K, V, Vp, grid, gen, torch.float32)
        hot = 9.0 if V <= 1000 else 12.5                            # (near the top of a row's draw at either vocabulary size)
        for b in range(0, B, 2):
            for k in range(K):
                x[b * K + k, EOS] = hot + grid * ((step + k) % 5)
        for b in range(B):
            kind = KINDS[(step * B + b) % len(KINDS)]
            c = 16 + 8 * ((5 + 13 * step + 7 * b) % 40)
            plant_ties(x[b * K], V, K, EOS, kind, c, bounds, TOP + 0.5 * ((step + b) % 3))
        if step == 1:
            x[1] = x[0]
        tables.append(x)
    return tables


def planted_beam_state(B, K, L, pos, gen, device):
    """a decode.BeamState as it looks before the step at ``pos``: random prefixes over the alphabet 10..19 in
    ``ids[pos & 1][:, :pos + 1]`` (n-gram bans fire), a scattered ``key_rows[pos & 1]``, finite distinct descending beam scores
    within every item, an empty hypothesis table.  With pos >= 40, beam 1 of every item ends in LATE_BAN[:2], a pair that occurs
    once more, 20 positions back, followed by LATE_BAN[2]: a 3-gram ban found only by the thread that scans that position."""
    import vlpet_amd.decode as D
    rows = B * K
    st = D.BeamState(B, K, L, device, START, PAD, D.beam_key_rows(rows, L, device))
    half = pos & 1
    ids = torch.randint(10, 20, (rows, pos + 1), generator=gen)
    ids[:, 0] = START
    if pos >= 40:
        x, y, z = LATE_BAN
        for b in range(B):
            r = b * K + 1
            ids[r, pos - 20:pos - 17] = torch.tensor([x, y, z])
            ids[r, pos - 1:pos + 1] = torch.tensor([x, y])
    st.ids[half, :, :pos + 1] = ids.to(device)
    st.key_rows[half, :, :pos + 1] = torch.randint(0, rows, (rows, pos + 1), generator=gen, dtype=torch.int32).to(device)
    steps = 0.25 + torch.rand(B, K, generator=gen)
    st.scores.copy_((-steps.cumsum(1) - pos * 0.5).view(-1))
    st.tokens.copy_(st.ids[half, :, pos])
    return st


def long_prefix_logits(B, K, V, pos, gen, dtype):
    """the one table of a planted-state step: the 1/4 grid draw with the prefixes' alphabet favoured (bans decide); item 1: eos on
    top of beam 0 (a hypothesis of pos + 1 tokens is copied); beam 1 of every item: LATE_BAN's continuation on top (banned)"""
    x = tie_logits(B * K, V, padded_width(V), 0.25, gen, torch.float32)
    x[:, 10:20] += 6.0
    x[:, V:] = float("inf")
    x[1 * K, EOS] = TOP
    if pos >= 40:
        for b in range(B):
            x[b * K + 1, LATE_BAN[2]] = TOP
    return x.to(dtype)


class SpecBeam:
    """beam_spec one step at a time.  A done item's rows are carried over (ids unchanged with pad appended, scores unchanged, source
    = the row itself), as decode.beam_step keeps them; HF's scorer leaves such rows undefined."""

    def __init__(self, B, K, L, lp=1.0, early=False, keep_trace=False):
        self.B, self.K, self.L = B, K, L
        self.ids = [[START] for _ in range(B * K)]
        s = torch.zeros(B, K)
        s[:, 1:] = BS.NEG_INIT
        self.scores = s.view(-1)
        self.key_rows = torch.arange(B * K)[:, None].expand(B * K, L).clone()
        self.hyps = [BS.Hyps(K, lp, early) for _ in range(B)]
        self.done = [False] * B
        self.tokens = [START] * (B * K)
        self.trace = [] if keep_trace else None

    @classmethod
    def from_state(cls, st, pos, lp, early, keep_trace=False):
        self = cls(st.B, st.K, st.L, lp, early, keep_trace)
        assert int(st.state[:, :2].abs().sum()) == 0, "planted states start with empty hypothesis tables"
        self.ids = st.ids[pos & 1][:, :pos + 1].cpu().tolist()
        self.scores = st.scores.detach().cpu().clone()
        self.key_rows = st.key_rows[pos & 1].cpu().long().clone()
        self.done = [bool(d) for d in st.state[:, 2].tolist()]
        return self

    def step(self, logits, V, eos=EOS, pad=PAD, min_length=0, ngram=0, force_eos=False):
        """one step on ``logits`` [B * K, >= V]; returns the number of items not done after it"""
        B, K = self.B, self.K
        cur_len = len(self.ids[0])
        self.bans = [set(banned_tokens(p, ngram)) | ({eos} if cur_len < min_length else set()) for p in self.ids]
        x = BS.row_scores(logits, V, self.ids, cur_len, eos, min_length, ngram, force_eos)
        flat = (x + self.scores[:, None]).view(B, K * V)
        top_v, top_i = BS.top_flat(flat, 2 * K + 1)
        live = [not d for d in self.done]
        old = self.scores.tolist()
        nscore, ntok, nsrc, _ = BS.process(self.ids, top_v[:, :2 * K], top_i[:, :2 * K], V, K, self.hyps, self.done, eos, pad)
        for b in range(B):
            if not live[b]:
                for r in range(b * K, (b + 1) * K):
                    nscore[r], nsrc[r] = old[r], r
        if self.trace is not None:
            self.trace.append(dict(top_v=top_v, top_i=top_i, live=live, cur_len=cur_len, flat=flat))
        self.scores = torch.tensor(nscore, dtype=torch.float32)
        self.ids = [self.ids[s] + [t] for s, t in zip(nsrc, ntok)]
        self.tokens = ntok
        kr = self.key_rows[torch.tensor(nsrc)].clone()
        kr[:, cur_len] = torch.arange(B * K)
        self.key_rows = kr
        return sum(1 for d in self.done if not d)

    def snapshot(self):
        return dict(ids=[list(r) for r in self.ids], scores=self.scores.clone(), key_rows=self.key_rows.clone(),
                    tokens=list(self.tokens), bans=self.bans, done=list(self.done),
                    hyps=[dict(worst=h.worst, n_added=h.n_added, beams={n: (s, list(t)) for s, t, n in h.beams}) for h in self.hyps])


def assert_state_matches_spec(st, snap, cur_len, tol=1e-4):
    """every tensor of the BeamState ``st`` after the step that made the rows ``cur_len`` + 1 tokens long, against a SpecBeam
    snapshot: ids, key rows, tokens, hypothesis tables (by insertion number) and done flags exactly, scores to ``tol``"""
    K, half = st.K, cur_len & 1
    assert st.ids[half][:, :cur_len + 1].cpu().tolist() == snap["ids"]
    if st.key_rows is not None:
        assert torch.equal(st.key_rows[half][:, :cur_len + 1].cpu().long(), snap["key_rows"][:, :cur_len + 1])
    assert st.tokens.cpu().tolist() == snap["tokens"]
    torch.testing.assert_close(st.scores.cpu(), snap["scores"], rtol=0, atol=tol)
    state, worst = st.state.cpu().tolist(), st.worst.cpu().tolist()
    hs, hm, ht = st.hyp_score.cpu().tolist(), st.hyp_meta.cpu().tolist(), st.hyp_tokens.cpu().tolist()
    for b, h in enumerate(snap["hyps"]):
        assert state[b] == [len(h["beams"]), h["n_added"], int(snap["done"][b])], (b, state[b], h)
        assert abs(worst[b] - h["worst"]) <= tol * max(1.0, abs(h["worst"]) * 1e-9 / tol), (b, worst[b], h["worst"])
        got = {hm[b * K + j][1]: (hs[b * K + j], ht[b * K + j][:hm[b * K + j][0]]) for j in range(len(h["beams"]))}
        assert sorted(got) == sorted(h["beams"]), (b, sorted(got), sorted(h["beams"]))
        for n, (score, toks) in h["beams"].items():
            assert abs(got[n][0] - score) <= tol and got[n][1] == toks, (b, n, got[n], score, toks)


def count_ties(trace, K):
    """exact ties among the finite top-2K entries of the live items, over the run"""
    n = 0
    for e in trace:
        for b, live in enumerate(e["live"]):
            if live:
                v = e["top_v"][b, :2 * K]
                n += int(((v[1:] == v[:-1]) & torch.isfinite(v[1:])).sum())
    return n


def eos_ties(trace, K, V, eos):
    """how many of those ties have eos on one side"""
    n = 0
    for e in trace:
        for b, live in enumerate(e["live"]):
            if live:
                v, t = e["top_v"][b, :2 * K], e["top_i"][b, :2 * K] % V
                same = (v[1:] == v[:-1]) & torch.isfinite(v[1:])
                n += int((same & ((t[1:] == eos) | (t[:-1] == eos))).sum())
    return n


def decision_margin(trace, K, V, eos, lp, early):
    """The smallest non-zero gap, in float64, of the decisions a run takes by value: between adjacent entries of every live item's
    top 2K + 1 flat scores (the order, the eos rule at rank K, the cut at 2K), and in the hypothesis table (``score > worst``, which
    one is evicted, ``worst >= best / cur_len ** lp``).  Exact zeros do not count -- both sides resolve them by index -- unless they
    stand between two beams whose whole score rows differ: such a tie is one of rounding, which nothing obliges an implementation
    to reproduce, and the margin is 0."""
    m = math.inf
    hyps = [BS.Hyps(K, lp, early) for _ in e_items(trace)]
    for e in trace:
        cur_len = e["cur_len"]
        for b, live in enumerate(e["live"]):
            if not live:
                continue
            v, idx = e["top_v"][b].double().tolist(), e["top_i"][b].tolist()
            for a in range(2 * K):
                if math.isinf(v[a]) or math.isinf(v[a + 1]):
                    continue
                g = v[a] - v[a + 1]
                if g > 0:
                    m = min(m, g)
                else:
                    ka, kb = idx[a] // V, idx[a + 1] // V
                    if ka != kb and not torch.equal(e["flat"][b, ka * V:(ka + 1) * V], e["flat"][b, kb * V:(kb + 1) * V]):
                        return 0.0
            h, slot = hyps[b], 0
            for rank in range(2 * K):
                if idx[rank] % V == eos:
                    if rank >= K:
                        continue
                    score = v[rank] / cur_len ** lp
                    if len(h) >= K:
                        if score != h.worst:
                            m = min(m, abs(score - h.worst))
                        kept = sorted(s for s, _, _ in h.beams)
                        if score > h.worst and kept[1] > kept[0]:
                            m = min(m, kept[1] - kept[0])
                    h.add([0] * cur_len, v[rank])
                else:
                    slot += 1
                if slot == K:
                    break
            if len(h) >= K and not early:
                g = abs(h.worst - v[0] / cur_len ** lp)
                if g > 0:
                    m = min(m, g)
    return m


def e_items(trace):
    return trace[0]["live"] if trace else []


def run_tie_case(case, early, keep_trace=False, tables=None):
    """the reference run of one committed case: (tables, per-step snapshots, per-step items not done, the SpecBeam)"""
    V, K, B, L, grid, seed = case
    tables = beam_tie_tables(*case) if tables is None else tables
    spec = SpecBeam(B, K, L, TIE_SETTINGS["lp"], early, keep_trace)
    snaps, counts = [], []
    for pos, x in enumerate(tables):
        counts.append(spec.step(x, V, min_length=TIE_SETTINGS["min_length"], ngram=TIE_SETTINGS["ngram"], force_eos=pos == L - 2))
        snaps.append(spec.snapshot())
    return tables, snaps, counts, spec


def run_long_case(K, pos, seed, device, dtype=torch.float32, keep_trace=False):
    """a planted state with item 2 held done, its table, and the reference's one step from it"""
    gen = torch.Generator().manual_seed(seed * 1000 + pos * 10 + K)
    st = planted_beam_state(LONG_B, K, LONG_L, pos, gen, device)
    st.state[2, 2] = 1
    logits = long_prefix_logits(LONG_B, K, LONG_V, pos, gen, dtype)
    spec = SpecBeam.from_state(st, pos, LONG_LP, False, keep_trace)
    left = spec.step(logits, LONG_V, ngram=LONG_NGRAM)
    return st, logits, spec, left


def expected_part_tok(table, V, S, T, bans, force_eos, eos=EOS):
    """vlpet_beam_rows' per (row, slice) top T: a stable descending sort of the slice's processed logits (banned columns and, on
    the forced step, every column but eos at -inf; -inf entries take part, lowest index first).  (values, tokens) [rows, S, T]"""
    x = table[:, :V].float().cpu().clone()
    if force_eos:
        keep = x[:, eos].clone()
        x.fill_(float("-inf"))
        x[:, eos] = keep
    for r, ban in enumerate(bans):
        if ban:
            x[r, sorted(ban)] = float("-inf")
    sc = slice_cols(V, S)
    vals, toks = [], []
    for s in range(S):
        c0, c1 = s * sc, min(V, (s + 1) * sc)
        assert c1 - c0 >= T
        v, i = torch.sort(x[:, c0:c1], dim=-1, descending=True, stable=True)
        vals.append(v[:, :T])
        toks.append(i[:, :T] + c0)
    return torch.stack(vals, 1), torch.stack(toks, 1)


# ---- decode attention ------------------------------------------------------------------------------------------------------------

def ref_attention64(q, k, v, H, mask=None, bias=None, scale=None):
    """fp64 ``softmax(scale * q k^T + bias + mask) v``: q [R, E], k / v [R, n, E] already gathered per query row, mask [R, n]
    (False = excluded), bias [H, >= n] (-inf = excluded).  A row with every key excluded is zeros.  Returns (o [R, E], max |s|
    over the counted keys)."""
    R, E = q.shape
    D = E // H
    n = k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    s = torch.einsum("bhd,bjhd->bhj", q.double().view(R, H, D), k.double().view(R, n, H, D)) * scale
    if bias is not None:
        s = s + bias[None, :, :n].double()
    if mask is not None:
        s = s.masked_fill(~mask[:, None, :n].bool(), float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(torch.isinf(s).all(-1, keepdim=True), torch.zeros_like(p), p)
    finite = s[torch.isfinite(s)]
    smax = float(finite.abs().max()) if finite.numel() else 0.0
    return torch.einsum("bhj,bjhd->bhd", p, v.double().view(R, n, H, D)).reshape(R, E), smax


def inf_bias(kind, H, n, gen):
    """an fp32 bias [H, n] with -inf entries: "some" keys of head 0, the "first" 40 keys of head 0 (every lane's first key) or
    "all" keys of head 0; the other heads get a few -inf of their own in the first two kinds"""
    b = torch.randn(H, n, generator=gen) * 2
    if kind == "some":
        b[0, torch.randperm(n, generator=gen)[:n // 3]] = float("-inf")
        b[-1, 0] = float("-inf")
    elif kind == "first":
        b[0, :40] = float("-inf")
        b[-1, n - 1] = float("-inf")
    else:
        b[0, :] = float("-inf")
    return b
