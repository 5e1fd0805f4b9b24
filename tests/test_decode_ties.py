"""CPU leg of the decode-kernel edge tests (tests/decode_cases.py builds the inputs, tests/test_gpu_decode_edges.py runs the kernels):

  * the committed tie cases meet their conditions on the reference alone: every decision beam_spec takes by value has a margin of
    1e-3 (ten times the 1e-4 score tolerance the kernels are held to, so fp32 log-sum-exp noise flips none), and every run holds
    at least 10 exact ties among its finite top-2K entries (so the GPU leg tests what it claims);
  * decode.beam_step's torch form -- the GPU tests' second yardstick -- against beam_spec on the same tie tables, step by step, in
    bf16 and fp32, and one step from planted long-prefix states;
  * decode._torch_attention with -inf bias entries against fp64 math: "excluded", and zeros when every key is, as the kernel."""
import functools

import pytest
import torch

import decode_cases as C

ALL_TIE_CASES = C.TIE_CASES_SMALL + C.TIE_CASES_LARGE
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _reference(case, early):
    tables, snaps, counts, spec = C.run_tie_case(case, early, keep_trace=True)
    V, K = case[0], case[1]
    facts = dict(margin=C.decision_margin(spec.trace, K, V, C.EOS, C.TIE_SETTINGS["lp"], early), ties=C.count_ties(spec.trace, K),
                 eos_ties=C.eos_ties(spec.trace, K, V, C.EOS), hyps=sum(h.n_added for h in spec.hyps))
    if V > 1000:
        tables = None                     # (the large tables are rebuilt where needed: a few hundred MB would stay cached)
    return tables, snaps, counts, facts


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("case", ALL_TIE_CASES, ids=lambda c: "V%d-K%d-B%d-s%d" % (c[0], c[1], c[2], c[5]))
def test_committed_tie_cases_keep_the_decision_margin_and_hold_ties(case, early):
    _, snaps, counts, facts = _reference(case, early)
    print(case, early, facts, counts)
    assert facts["margin"] >= MARGIN
    assert facts["ties"] >= 10
    assert facts["hyps"] > 0                                          # hypotheses were made
    assert not early or counts[-1] == 0                               # the forced step fills every table: early stopping ends all


def test_the_tie_cases_reach_every_planted_kind():
    """the tables are the same numbers in bf16 and fp32; an eos tie shows among the top 2K of some run; some item is done before the
    last step under early stopping and goes on without it; every plant kind lands at both real vocabularies"""
    for case in ALL_TIE_CASES:
        if case[0] == 500:
            for x in C.beam_tie_tables(*case):
                assert torch.equal(x.to(torch.bfloat16).float(), x)
    assert sum(_reference(c, e)[3]["eos_ties"] for c in ALL_TIE_CASES for e in (False, True)) >= 10
    assert any(0 < _reference(c, True)[2][-2] < c[2] for c in ALL_TIE_CASES)
    assert any(_reference(c, False)[2][-2] == c[2] for c in ALL_TIE_CASES)
    for V in (50265, 32100):
        row = torch.zeros(V)
        bounds = C.slice_boundaries(V, 20)
        assert len(bounds) == 2
        want = dict(group=1, lane=8, wave=512, stride=2048, slice=1)
        for kind in C.KINDS:
            cols = C.plant_ties(row, V, 5, C.EOS, kind, 24, bounds)
            if kind in want:
                assert cols[1] - cols[0] == want[kind] and (kind != "slice" or cols[1] in bounds)
            elif kind == "last":
                assert cols[1] == V - 1 and V % 8 != 0
            elif kind == "cut":
                assert len(cols) == 11 and max(cols) < V
            else:
                assert C.EOS in cols


def _torch_form_step(st, logits, V, pos, **kw):
    import vlpet_amd.decode as D
    saved = D.EAGER
    D.EAGER = True
    try:
        D.beam_step(logits, V, st, pos, **kw)
    finally:
        D.EAGER = saved


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ALL_TIE_CASES, ids=lambda c: "V%d-K%d-B%d-s%d" % (c[0], c[1], c[2], c[5]))
def test_torch_form_matches_the_spec_on_tie_tables_step_by_step(case, dtype, early):
    import vlpet_amd.decode as D
    V, K, B, L, _, _ = case
    tables, snaps, counts, _ = _reference(case, early)
    tables = tables or C.beam_tie_tables(*case)
    st = D.BeamState(B, K, L, "cpu", C.START, C.PAD, D.beam_key_rows(B * K, L, "cpu"))
    for pos, x in enumerate(tables):
        _torch_form_step(st, x.to(dtype), V, pos, eos_token_id=C.EOS, pad_token_id=C.PAD, min_length=C.TIE_SETTINGS["min_length"],
                         no_repeat_ngram_size=C.TIE_SETTINGS["ngram"], length_penalty=C.TIE_SETTINGS["lp"], early_stopping=early,
                         force_eos=pos == L - 2)
        C.assert_state_matches_spec(st, snaps[pos], pos + 1)
        assert int(st.counters[pos]) == counts[pos]


@pytest.mark.parametrize("K,pos,seed", C.LONG_CASES)
def test_torch_form_matches_the_spec_one_step_from_a_planted_long_prefix(K, pos, seed):
    st, logits, spec, left = C.run_long_case(K, pos, seed, "cpu", keep_trace=True)
    assert C.decision_margin(spec.trace, K, C.LONG_V, C.EOS, C.LONG_LP, False) >= MARGIN
    snap = spec.snapshot()
    # the state is what it claims: an item held done, a hypothesis of pos + 1 tokens, bans that fire, the late 3-gram ban
    assert snap["done"][2] and left == C.LONG_B - 1
    assert [len(h["beams"]) for h in snap["hyps"]] == [0, 1, 0, 0] and len(snap["hyps"][1]["beams"][0][1]) == pos + 1
    assert sum(1 for b in snap["bans"] for t in b if 10 <= t < 20) >= C.LONG_B
    assert all(C.LATE_BAN[2] in snap["bans"][b * K + 1] and C.LATE_BAN[2] not in snap["tokens"] for b in range(C.LONG_B))
    kr0 = st.key_rows[pos & 1].clone()
    _torch_form_step(st, logits, C.LONG_V, pos, eos_token_id=C.EOS, pad_token_id=C.PAD, no_repeat_ngram_size=C.LONG_NGRAM,
                     length_penalty=C.LONG_LP)
    C.assert_state_matches_spec(st, snap, pos + 1)
    assert int(st.counters[pos]) == left
    assert torch.equal(st.key_rows[pos & 1], kr0)                      # the half that was read is left alone


# ---- -inf bias entries: the torch form of decode_attention ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["some", "first", "all"])
@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("D", [16, 64])
def test_torch_attention_treats_minus_inf_bias_as_excluded(D, form, kind):
    """the fallback of decode_attention on the inputs of the GPU leg's -inf cases (fp32, CPU): excluded keys carry no weight, a head
    whose keys are all excluded gives zeros -- the kernel's rule, so both stay in agreement"""
    from vlpet_amd.decode import decode_attention
    H, B, n = 3, 3, 70
    E = H * D
    gen = torch.Generator().manual_seed(D + len(kind))
    bias = C.inf_bias(kind, H, n, gen)
    q = torch.randn(B, E, generator=gen)
    kc, vc = torch.randn(B, n + 2, E, generator=gen), torch.randn(B, n + 2, E, generator=gen)
    if form == "self":
        kn, vn = torch.randn(B, E, generator=gen), torch.randn(B, E, generator=gen)
        o = decode_attention(q, kc, vc, H, pos=n - 1, k_new=kn, v_new=vn, bias=bias, scale=1.0)
        assert torch.equal(kc[:, n - 1], kn) and torch.equal(vc[:, n - 1], vn)
        ref, _ = C.ref_attention64(q, kc[:, :n], vc[:, :n], H, bias=bias, scale=1.0)
    else:
        mask = torch.ones(B, n, dtype=torch.bool)
        mask[1, 50:] = False
        o = decode_attention(q, kc[:, :n], vc[:, :n], H, key_mask=mask, bias=bias, scale=1.0)
        ref, _ = C.ref_attention64(q, kc[:, :n], vc[:, :n], H, mask=mask, bias=bias, scale=1.0)
    assert torch.isfinite(o).all()
    if kind == "all":
        assert float(o[:, :D].abs().max()) == 0.0
    assert float((o.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
