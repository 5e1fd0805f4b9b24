"""The decode and beam kernels of csrc/decode.hip at the edges the main-road tests (test_gpu_generate.py, test_gpu_beam.py) do not
reach.  Inputs and the step-by-step reference come from tests/decode_cases.py; tests/test_decode_ties.py checks on the CPU that the
inputs meet their conditions (decision margin, ties present) and that the torch form agrees with the spec on them.

  * vlpet_beam_rows + vlpet_beam_advance on bf16 and fp32 tie tables (values exact in bf16; planted exact ties across an 8-group,
    two lanes, two waves, a thread's consecutive loads, a slice boundary, the last valid column, with eos on either side, a
    2K + 1 group over the cut, one cross-beam tie of bitwise identical rows), every K in 2..8, both early_stopping values, the forced
    step last: every state tensor against beam_spec (CPU) and against the torch form (device) after every step, and the per-slice
    top lists of vlpet_beam_rows against a stable sort;
  * one step from planted states at pos 63 / 64 / 65 / 130 / 300 (second and later trips of every copy loop and of the ban scan);
  * vlpet_greedy_pick when the lowest-index top tie is banned, and its ban scan past 512 positions;
  * vlpet_attn_decode / _beam at B * H not a multiple of 4 (a wave without a pair, workgroups over two sequences), key counts
    around the unroll and at the limit, NaN in the cache rows past pos, fully masked rows, scores in the hundreds, -inf bias."""
import functools

import pytest
import torch

import decode_cases as C
from test_gpu_beam import _same_state, _states
from test_gpu_generate import _pick_both, _tol

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case_id(c):
    return "V%d-K%d-B%d-s%d" % (c[0], c[1], c[2], c[5])


@functools.lru_cache(maxsize=None)
def _tables(case):
    return C.beam_tie_tables(*case)


@functools.lru_cache(maxsize=None)
def _spec(case, early):
    """the reference run of a case: computed once, shared by every slices / dtype case, never modified"""
    _, snaps, counts, _ = C.run_tie_case(case, early, tables=_tables(case))
    return snaps, counts


def _eager_step(D, *a, **k):
    saved = D.EAGER
    D.EAGER = True
    try:
        D.beam_step(*a, **k)
    finally:
        D.EAGER = saved


def _check_part_lists(D, st, table, V, slices, bans, force_eos):
    """the workspace vlpet_beam_rows left: per (row, slice) the top 2K (value, token) of the processed logits"""
    rows, T = table.shape[0], 2 * st.K
    S = D._beam_slices(rows, V) if slices is None else slices
    _, val, tok = st._ws
    want_v, want_t = C.expected_part_tok(table, V, S, T, bans, force_eos)
    got_t, got_v = tok.view(rows, S, T).cpu().long(), val.view(rows, S, T).cpu()
    assert torch.equal(got_t, want_t), torch.nonzero(got_t != want_t)[:4].tolist()
    assert torch.equal(got_v, want_v)


def _run_tie_case(case, slices, dtype, early):
    import vlpet_amd.decode as D
    V, K, B, L, _, _ = case
    snaps, counts = _spec(case, early)
    hip, ref = _states(B, K, L, C.START, C.PAD)
    kw = dict(eos_token_id=C.EOS, pad_token_id=C.PAD, min_length=C.TIE_SETTINGS["min_length"],
              no_repeat_ngram_size=C.TIE_SETTINGS["ngram"], length_penalty=C.TIE_SETTINGS["lp"], early_stopping=early)
    n0 = dict(D.LAUNCHES)
    for pos, table in enumerate(_tables(case)):
        logits = table.to(DEV, dtype)
        force = pos == L - 2
        D.beam_step(logits, V, hip, pos, slices=slices, force_eos=force, **kw)
        _eager_step(D, logits, V, ref, pos, force_eos=force, **kw)
        torch.cuda.synchronize()
        _check_part_lists(D, hip, table, V, slices, snaps[pos]["bans"], force)
        C.assert_state_matches_spec(hip, snaps[pos], pos + 1)
        _same_state(hip, ref, pos + 1, 1e-4)
        assert int(hip.counters[pos]) == counts[pos] == int(ref.counters[pos])
    assert D.LAUNCHES["beam_rows"] - n0["beam_rows"] == L - 1 and D.LAUNCHES["beam_advance"] - n0["beam_advance"] == L - 1


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("slices", C.TIE_SLICES[500])
@pytest.mark.parametrize("case", C.TIE_CASES_SMALL, ids=_case_id)
def test_beam_kernels_order_exact_ties_by_index_for_every_beam_width(case, slices, dtype, early):
    _run_tie_case(case, slices, dtype, early)


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("slices", [None, 1, 7])
@pytest.mark.parametrize("case", C.TIE_CASES_LARGE, ids=_case_id)
def test_beam_kernels_order_exact_ties_by_index_at_the_real_vocabularies(case, slices, dtype, early):
    _run_tie_case(case, slices, dtype, early)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K,pos,seed", C.LONG_CASES)
def test_beam_kernels_one_step_from_a_planted_long_prefix(K, pos, seed, dtype):
    """cur_len = pos + 1 > 64: the later trips of the copy loops (ids, key rows, the tokens of a new hypothesis, the carried rows of
    a done item) and, at pos = 300, of vlpet_beam_rows' ban scan (a 3-gram ban whose only occurrence lies past position 256)"""
    import vlpet_amd.decode as D
    V = C.LONG_V
    st, table, spec, left = C.run_long_case(K, pos, seed, DEV, dtype)
    ref = C.run_long_case(K, pos, seed, DEV, dtype)[0]
    snap = spec.snapshot()
    src = (st.ids[pos & 1].clone(), st.key_rows[pos & 1].clone())
    logits = table.to(DEV)
    kw = dict(eos_token_id=C.EOS, pad_token_id=C.PAD, no_repeat_ngram_size=C.LONG_NGRAM, length_penalty=C.LONG_LP)
    D.beam_step(logits, V, st, pos, slices=3, **kw)
    _eager_step(D, logits, V, ref, pos, **kw)
    torch.cuda.synchronize()
    _check_part_lists(D, st, table, V, 3, snap["bans"], False)
    C.assert_state_matches_spec(st, snap, pos + 1)
    _same_state(st, ref, pos + 1, 1e-4)
    assert int(st.counters[pos]) == left == int(ref.counters[pos])
    assert torch.equal(st.ids[pos & 1], src[0]) and torch.equal(st.key_rows[pos & 1], src[1])     # the halves read are left alone
    assert len(snap["hyps"][1]["beams"][0][1]) == pos + 1 and snap["done"][2]


# ---- vlpet_greedy_pick ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ban", ["ngram", "min_length"])
@pytest.mark.parametrize("V", [500, 50465])
def test_greedy_pick_gives_a_banned_lowest_tie_to_the_next_lowest_index(V, ban):
    """three columns tie at the top of a bf16 row; the lowest is banned (by a bigram of the prefix, or as eos below min_length):
    the second lowest wins, whatever unit of the scan separates them"""
    B, L, pos = 12, 24, 5
    gen = torch.Generator().manual_seed(V)
    logits = C.tie_logits(B, V, C.padded_width(V), 0.125, gen, torch.float32)
    offs = [o for o in (1, 8, 64, 8 * 64, 8 * 512, 8 * 512 * 4) if 3 * o < V - 200]
    ids = torch.randint(30, 40, (B, L), generator=gen)
    ids[:, 0] = C.START
    want = []
    for b in range(B):
        c1 = C.EOS if ban == "min_length" else 48 + 8 * b + b % 7
        c2 = c1 + offs[b % len(offs)]
        c3 = c2 + offs[(b + 1) % len(offs)]
        logits[b, [c1, c2, c3]] = C.TOP
        if ban == "ngram":
            ids[b, 2], ids[b, 3] = ids[b, pos], c1                   # the last token was followed by c1 before
        want.append(c2)
    ids = ids.to(DEV)
    unfinished = torch.ones(B, dtype=torch.int32, device=DEV)
    _pick_both(logits.to(DEV, torch.bfloat16), V, ids, pos, unfinished, C.EOS, C.PAD, pos + 5 if ban == "min_length" else 0,
               2 if ban == "ngram" else 0)
    assert ids[:, pos + 1].tolist() == want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_greedy_pick_ban_scan_strides_past_512_positions(dtype):
    """pos = 600 in ids rows of 640: the bigram that bans the top column occurs once, at position 550 -- the second trip of the scan"""
    B, V, L, pos = 4, 500, 640, 600
    gen = torch.Generator().manual_seed(9)
    logits = C.tie_logits(B, V, C.padded_width(V), 0.125, gen, torch.float32)
    ids = torch.randint(30, 60, (B, L), generator=gen)
    ids[:, 0] = C.START
    want = []
    for b in range(B):
        c1 = 100 + 8 * b
        logits[b, [c1, c1 + 9]] = C.TOP
        ids[b, pos], ids[b, 550], ids[b, 551] = 70 + b, 70 + b, c1
        want.append(c1 + 9)
    ids = ids.to(DEV)
    unfinished = torch.ones(B, dtype=torch.int32, device=DEV)
    _pick_both(logits.to(DEV, dtype), V, ids, pos, unfinished, C.EOS, C.PAD, 0, 2)
    assert ids[:, pos + 1].tolist() == want


# ---- decode attention -------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _self_step(q, k, v, H, dtype, gen, *, rows=False, bias=None, scale=None):
    """the append form on keys ``k`` / values ``v`` [B, n, E] (row n - 1 is the appended one): caches of min(n + 3, 1024) rows whose
    rows past pos hold NaN, optionally read through a scattered key-row table.  Returns (o, fp64 reference, max |s|) after checking
    the append (bit-exact, batch r) and that no other cache row changed."""
    from vlpet_amd.decode import LAUNCHES, decode_attention
    B, n, E = k.shape
    pos, Lmax = n - 1, min(n + 3, 1024)
    kc = torch.full((B, Lmax, E), float("nan"), dtype=dtype, device=DEV)
    vc = torch.full((B, Lmax, E), float("nan"), dtype=dtype, device=DEV)
    kc[:, :pos], vc[:, :pos] = k[:, :pos], v[:, :pos]
    qkv = torch.cat([q, k[:, pos], v[:, pos]], 1).contiguous()          # the fused q | k | v row
    qq, kn, vn = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    table = None
    if rows:
        table = torch.randint(0, B, (B, Lmax), generator=gen, dtype=torch.int32)
        table[:, pos:] = -7                                              # never read: the appended key is the row's own
        table = table.to(DEV)
    k0, v0 = kc.clone(), vc.clone()
    n0 = LAUNCHES["attn_decode"]
    o = decode_attention(qq, kc, vc, H, pos=pos, k_new=kn, v_new=vn, key_rows=table, bias=bias, scale=scale)
    torch.cuda.synchronize()
    assert LAUNCHES["attn_decode"] == n0 + 1
    assert torch.equal(kc[:, pos], kn) and torch.equal(vc[:, pos], vn)
    keep = torch.ones(Lmax, dtype=torch.bool, device=DEV)
    keep[pos] = False
    assert torch.equal(_bits(kc)[:, keep], _bits(k0)[:, keep]) and torch.equal(_bits(vc)[:, keep], _bits(v0)[:, keep])
    if rows:
        kr = table[:, :n].long().clone()
        kr[:, pos] = torch.arange(B, device=DEV)
        j = torch.arange(n, device=DEV)[None].expand(B, -1)
        kg, vg = kc[kr, j], vc[kr, j]
    else:
        kg, vg = kc[:, :n], vc[:, :n]
    ref, smax = C.ref_attention64(qq, kg, vg, H, bias=bias, scale=scale)
    return o, ref, smax


def _cross_step(q, k, v, H, *, group=1, mask=None, bias=None, scale=None):
    """the in-place form: ``k`` / ``v`` [ceil(B / group), n, E]; the key cache is handed over as a column block of a fused projection"""
    from vlpet_amd.decode import LAUNCHES, decode_attention
    B, E = q.shape
    fused = torch.cat([torch.zeros_like(k), k, torch.ones_like(k)], 2)
    kc = fused[..., E:2 * E]
    n0 = LAUNCHES["attn_decode"]
    o = decode_attention(q, kc, v, H, key_mask=mask, group=group, bias=bias, scale=scale)
    assert LAUNCHES["attn_decode"] == n0 + 1
    rep = lambda t: t.repeat_interleave(group, 0)[:B]
    ref, smax = C.ref_attention64(q, rep(k), rep(v), H, mask=None if mask is None else rep(mask), bias=bias, scale=scale)
    return o, ref, smax


def _rand(*shape, dtype, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV, dtype)


def _close(o, ref, dtype, extra=0.0):
    assert torch.isfinite(o).all()
    err = float((o.double() - ref).abs().max())
    assert err <= _tol(dtype, ref) + extra, (err, _tol(dtype, ref) + extra)
    return err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("form", ["self", "self_rows", "cross", "cross_group"])
@pytest.mark.parametrize("D", [16, 64])
def test_attention_geometry_odd_pairs_key_counts_and_nan_past_pos(D, form, dtype):
    """H in {1, 3, 5} x B in {1, 3, 7}: B * H is no multiple of 4 (the last workgroup has waves without a pair) and workgroups span
    two sequences; key counts around the unroll of the key loop and at the limit of 1024; the self-attention caches hold NaN past
    pos -- a key past the end must not be read into the sum, not even at weight zero -- and stay bitwise untouched"""
    gen = torch.Generator().manual_seed(D + len(form))
    counts = ((31, 33, 65) if D == 64 else (63, 65, 129)) + (1024,)
    for H in (1, 3, 5):
        for B in (1, 3, 7):
            for n in counts:
                E = H * D
                q = _rand(B, E, dtype=dtype, gen=gen, scale=2.0)
                if form.startswith("self"):
                    k, v = _rand(B, n, E, dtype=dtype, gen=gen), _rand(B, n, E, dtype=dtype, gen=gen)
                    o, ref, _ = _self_step(q, k, v, H, dtype, gen, rows=form == "self_rows")
                else:
                    group = 3 if form == "cross_group" else 1
                    Bc = -(-B // group)
                    k, v = _rand(Bc, n, E, dtype=dtype, gen=gen), _rand(Bc, n, E, dtype=dtype, gen=gen)
                    lens = torch.randint(1, n + 1, (Bc,), generator=gen)
                    lens[0] = n
                    mask = (torch.arange(n)[None] < lens[:, None]).to(DEV)
                    o, ref, _ = _cross_step(q, k, v, H, group=group, mask=mask)
                _close(o, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("D", [16, 64])
def test_attention_fully_masked_rows_are_exact_zeros(D, group, with_bias, dtype):
    H, B, n = 3, 7, 70
    E = H * D
    gen = torch.Generator().manual_seed(D + group)
    Bc = -(-B // group)
    q = _rand(B, E, dtype=dtype, gen=gen, scale=2.0)
    k, v = _rand(Bc, n, E, dtype=dtype, gen=gen), _rand(Bc, n, E, dtype=dtype, gen=gen)
    mask = torch.ones(Bc, n, dtype=torch.bool)
    mask[0] = False                                                     # item 0: every key masked
    mask[-1, 5:] = False
    if group == 1:
        mask[4] = False
    mask = mask.to(DEV)
    bias = (torch.randn(H, n, generator=gen) * 2).to(DEV) if with_bias else None
    o, ref, _ = _cross_step(q, k, v, H, group=group, mask=mask, bias=bias, scale=1.0 if with_bias else None)
    dead = (~mask.any(1)).repeat_interleave(group, 0)[:B]
    assert int(dead.sum()) == (3 if group == 3 else 2)
    assert float(o[dead].float().abs().max()) == 0.0
    assert float(ref[~dead].abs().max()) > 0.1
    _close(o, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("D", [16, 64])
def test_attention_scores_in_the_hundreds(D, form, dtype):
    """q scaled so that max |s| of the reference is 150..300: one key leads clearly in the odd heads, two keys tie exactly for the
    lead in the even heads (the output is the mean of their values).  A missing or misplaced max-subtraction overflows exp here.
    Tolerance: the file's _tol plus the rounding of the scores themselves, from the reference's own magnitudes:
    8 * 2**-23 * max|s_ref| * max|v| (a 64-term fp32 dot product; 8 = sqrt(64) ulp with margin), about 1e-3 at these sizes.
    Measured on an MI355X (self and cross forms alike): fp32 2.96e-6 (D = 16) and 2.86e-6 (D = 64) under 9.0e-4 and 9.7e-4; bf16
    3.9e-3 and 7.8e-3 (one output rounding) under 3.2e-2 and 4.1e-2.  The test prints both figures."""
    H, B, n = 5, 3, 129
    E = H * D
    gen = torch.Generator().manual_seed(D)
    q = torch.randn(B, E, generator=gen)
    k, v = torch.randn(B, n, E, generator=gen), torch.randn(B, n, E, generator=gen)
    s = torch.einsum("bhd,bjhd->bhj", q.view(B, H, D), k.view(B, n, H, D)) * D ** -0.5
    q = q * (220.0 / float(s.abs().max()))
    lead = s.argmax(-1)                                                  # [B, H]: the scaling keeps the order
    for b in range(B):
        for h in range(0, H, 2):
            j1 = int(lead[b, h])
            k[b, (j1 + 37) % n, h * D:(h + 1) * D] = k[b, j1, h * D:(h + 1) * D]
    q, k, v = q.to(DEV, dtype), k.to(DEV, dtype), v.to(DEV, dtype)
    if form == "self":
        o, ref, smax = _self_step(q, k, v, H, dtype, gen)
    else:
        o, ref, smax = _cross_step(q, k, v, H)
    assert 150.0 <= smax <= 300.0, smax
    extra = 8 * 2.0 ** -23 * smax * float(v.float().abs().max())
    err = float((o.double() - ref).abs().max())
    print("large scores D=%d %s %s: err %.3e tol %.3e (score term %.3e) max|s| %.1f" % (D, form, dtype, err, _tol(dtype, ref) + extra,
                                                                                       extra, smax))
    _close(o, ref, dtype, extra)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", ["some", "first", "all"])
@pytest.mark.parametrize("form", ["self", "self_rows", "cross"])
@pytest.mark.parametrize("D", [16, 64])
def test_attention_minus_inf_bias_entries_mean_excluded(D, form, kind, dtype):
    """-inf in the bias: some keys of a head, its first 40 keys (the first key every lane counts), every key of a head (zeros, as for
    a full mask).  tests/test_decode_ties.py holds decode._torch_attention to the same rule on the CPU."""
    H, B, n = 3, 3, 70
    E = H * D
    gen = torch.Generator().manual_seed(D + len(kind))
    bias = C.inf_bias(kind, H, n, gen).to(DEV)
    q = _rand(B, E, dtype=dtype, gen=gen)
    k, v = _rand(B, n, E, dtype=dtype, gen=gen), _rand(B, n, E, dtype=dtype, gen=gen)
    if form == "cross":
        mask = torch.ones(B, n, dtype=torch.bool)
        mask[1, 50:] = False
        o, ref, _ = _cross_step(q, k, v, H, mask=mask.to(DEV), bias=bias, scale=1.0)
    else:
        o, ref, _ = _self_step(q, k, v, H, dtype, gen, rows=form == "self_rows", bias=bias, scale=1.0)
    if kind == "all":
        assert float(o[:, :D].float().abs().max()) == 0.0
    _close(o, ref, dtype)
