"""The replayed decode step without a GPU: the argument checks of the four position-on-device entry points (vlpet_*_at), the torch
forms of decode_attention / greedy_pick / beam_step with a position tensor against the same forms with the int, and
generate(graph=True) on CPU tensors -- the plain loop, token for token the gen_* / beam_* goldens, counted as an eager fallback."""
import pytest
import torch

from test_beam import BEAM_FIXTURES, build_beam_host, load_beam
from test_beam import check_against_fixture as check_beam
from test_generate import GEN_FIXTURES, build_host, load_gen

A = 4096                  # a 16-byte aligned non-NULL value: every call below returns before it could be dereferenced
E_SHAPE, E_ALIGN, E_NULL, E_DTYPE = -1, -3, -5, -6


def test_at_entry_points_reject_bad_arguments_without_gpu():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert lib.vlpet_version() >= 640

    def attn(q=A, k=A, v=A, o=A, kn=A, vn=A, pd=A, lim=56, ld=256, ldk=256, D=64, H=4, Lk=56, B=2, dt=1, mask=None, lm=0, bias=None,
             lb=0, psb=0, kr=None, ldkr=0, pskr=0):
        return lib.vlpet_attn_decode_at(q, ld, k, v, ldk, 56 * ldk, ldk, 56 * ldk, kn, vn, ld, pd, lim, mask, lm, bias, lb, psb, o, ld,
                                        B, H, D, Lk, 0.125, kr, ldkr, pskr, dt, None)
    assert attn(pd=None) == E_SHAPE                                                   # no position word
    assert attn(pd=A + 2) == E_ALIGN
    assert attn(lim=0) == E_SHAPE and attn(lim=57) == E_SHAPE                         # the limit against the caches' rows
    assert attn(q=None) == E_NULL and attn(o=None) == E_NULL and attn(kn=None) == E_NULL and attn(kn=None, vn=None) == E_NULL
    assert attn(dt=7) == E_DTYPE
    assert attn(D=32) == E_SHAPE and attn(Lk=1025, lim=1) == E_SHAPE and attn(B=0) == E_SHAPE and attn(ld=128) == E_SHAPE
    assert attn(mask=A, lm=8) == E_SHAPE and attn(bias=A, lb=8, psb=256) == E_SHAPE   # rows shorter than the limit
    assert attn(kr=A, ldkr=55, pskr=110) == E_SHAPE and attn(bias=A, lb=56, psb=-8) == E_SHAPE
    assert attn(q=A + 8) == E_ALIGN and attn(ld=260) == E_ALIGN and attn(bias=A + 2, lb=56) == E_ALIGN and attn(kr=A + 2, ldkr=56) == E_ALIGN

    def pick(lg=A, ids=A, V=500, ld=504, pd=A, lim=19, ldi=20, eos=2, ngram=0, B=3, dt=1, nt=A):
        return lib.vlpet_greedy_pick_at(lg, ld, V, ids, ldi, pd, lim, A, A, nt, B, eos, 1, 0, ngram, dt, None)
    assert pick(pd=None) == E_SHAPE and pick(pd=A + 1) == E_ALIGN
    assert pick(lim=0) == E_SHAPE and pick(lim=20) == E_SHAPE                         # pos + 1 must stay inside an ids row
    assert pick(lg=None) == E_NULL and pick(ids=None) == E_NULL and pick(nt=None) == E_NULL
    assert pick(dt=3) == E_DTYPE
    assert pick(ld=496) == E_SHAPE and pick(V=70000, ld=70000) == E_SHAPE and pick(eos=500) == E_SHAPE
    assert pick(ngram=-1) == E_SHAPE and pick(B=0) == E_SHAPE
    assert pick(lg=A + 4) == E_ALIGN and pick(ld=508) == E_ALIGN and pick(ids=A + 4) == E_ALIGN and pick(nt=A + 4) == E_ALIGN

    def rows(lg=A, ids=A, V=500, ld=504, pd=A, lim=19, ldi=20, ps=160, K=4, S=1, eos=2, ngram=0, st=A, dt=1):
        return lib.vlpet_beam_rows_at(lg, ld, V, ids, ldi, ps, pd, lim, 8, K, S, eos, 0, ngram, 18, st, A, A, dt, None)
    assert rows(pd=None) == E_SHAPE and rows(pd=A + 2) == E_ALIGN and rows(lim=0) == E_SHAPE and rows(lim=21) == E_SHAPE
    assert rows(ps=-160) == E_SHAPE
    assert rows(lg=None) == E_NULL and rows(ids=None) == E_NULL and rows(st=None) == E_NULL
    assert rows(dt=5) == E_DTYPE
    assert rows(K=1) == E_SHAPE and rows(K=9) == E_SHAPE and rows(S=0) == E_SHAPE and rows(S=65) == E_SHAPE
    assert rows(eos=-1) == E_SHAPE and rows(eos=500) == E_SHAPE and rows(ld=496) == E_SHAPE and rows(ngram=-1) == E_SHAPE
    assert rows(lg=A + 8) == E_ALIGN and rows(ids=A + 4) == E_ALIGN and rows(st=A + 4) == E_ALIGN

    def adv(stats=A, ids=A, kr=A, pd=A, lim=19, ldi=20, ldh=20, ldkr=20, K=4, S=1, V=500, eos=2, ctr=A):
        return lib.vlpet_beam_advance_at(stats, A, A, S, V, 3, K, A, ids, ldi, 240, kr, ldkr, 240, A, A, A, A, ldh, A, A, ctr, pd, lim,
                                         eos, 1, 1.0, 0, None)
    assert adv(pd=None) == E_SHAPE and adv(pd=A + 2) == E_ALIGN and adv(lim=0) == E_SHAPE
    assert adv(lim=20) == E_SHAPE and adv(ldh=18) == E_SHAPE and adv(ldkr=19) == E_SHAPE     # pos + 1 inside ids, hyp and key rows
    assert adv(stats=None) == E_NULL and adv(ids=None) == E_NULL and adv(ctr=None) == E_NULL
    assert adv(K=1) == E_SHAPE and adv(K=9) == E_SHAPE and adv(S=0) == E_SHAPE and adv(eos=500) == E_SHAPE and adv(V=70000) == E_SHAPE
    assert adv(ids=A + 4) == E_ALIGN and adv(kr=A + 2) == E_ALIGN and adv(stats=A + 2) == E_ALIGN


# ---- the torch forms with a position tensor -----------------------------------------------------------------------------------

def _word(pos):
    return torch.tensor([pos], dtype=torch.int32)


@pytest.mark.parametrize("pos", [0, 3, 8])
@pytest.mark.parametrize("t5,beam", [(False, False), (True, False), (False, True), (True, True)])
def test_torch_attention_with_a_position_tensor_is_the_int_form(pos, t5, beam):
    from vlpet_amd.decode import decode_attention
    B, H, Dh, L = 3, 4, 16, 10
    E = H * Dh
    gen = torch.Generator().manual_seed(pos + 2 * t5 + beam)
    kc, vc = torch.randn(B, L, E, generator=gen), torch.randn(B, L, E, generator=gen)
    q, kn, vn = (torch.randn(B, E, generator=gen) for _ in range(3))
    table = torch.randn(L, H, L, generator=gen) if t5 else None
    kr = torch.randint(0, B, (2, B, L), generator=gen, dtype=torch.int32) if beam else None
    ka, va, kb, vb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a = decode_attention(q, ka, va, H, pos=pos, k_new=kn, v_new=vn, bias=None if table is None else table[pos],
                         key_rows=None if kr is None else kr[pos & 1], scale=1.0 if t5 else None)
    b = decode_attention(q, kb, vb, H, k_new=kn, v_new=vn, bias=table, key_rows=kr, scale=1.0 if t5 else None, pos_dev=_word(pos))
    assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(va, vb)


@pytest.mark.parametrize("pos", [0, 5, 12])
@pytest.mark.parametrize("ngram,min_length,eos", [(0, 0, None), (2, 6, 3), (3, 0, 3)])
def test_torch_pick_with_a_position_tensor_is_the_int_form(pos, ngram, min_length, eos):
    from vlpet_amd.decode import greedy_pick
    B, V, L = 5, 40, 16
    gen = torch.Generator().manual_seed(pos + ngram)
    logits = torch.randn(B, V, generator=gen)
    ids = torch.randint(10, 14, (B, L), generator=gen)
    unf = (torch.rand(B, generator=gen) < 0.7).to(torch.int32)
    ia, ib, ua, ub = ids.clone(), ids.clone(), unf.clone(), unf.clone()
    ca, cb = torch.zeros(L, dtype=torch.int32), torch.zeros(L, dtype=torch.int32)
    nt = torch.full((B,), -1, dtype=torch.int64)
    kw = dict(eos_token_id=eos, pad_token_id=1, min_length=min_length, no_repeat_ngram_size=ngram)
    greedy_pick(logits, V, ia, pos, ua, ca, **kw)
    greedy_pick(logits, V, ib, None, ub, cb, pos_dev=_word(pos), next_tokens=nt, **kw)
    assert torch.equal(ia, ib) and torch.equal(ua, ub) and torch.equal(ca, cb) and torch.equal(nt, ia[:, pos + 1])


def test_torch_beam_step_with_a_position_tensor_is_the_int_form():
    import vlpet_amd.decode as D
    B, K, V, L, eos, pad = 3, 3, 40, 7, 3, 1
    gen = torch.Generator().manual_seed(4)
    a = D.BeamState(B, K, L, "cpu", 2, pad, D.beam_key_rows(B * K, L, "cpu"))
    b = D.BeamState(B, K, L, "cpu", 2, pad, D.beam_key_rows(B * K, L, "cpu"))
    word = _word(0)
    kw = dict(eos_token_id=eos, pad_token_id=pad, min_length=2, no_repeat_ngram_size=2, length_penalty=0.8)
    for pos in range(L - 1):
        logits = torch.randn(B * K, V, generator=gen) * 3
        logits[:K, eos] += 6.0
        D.beam_step(logits, V, a, pos, force_eos=pos == L - 2, **kw)
        D.beam_step(logits, V, b, None, pos_dev=word, force_eos_pos=L - 2, **kw)
        word.add_(1)
        for name in ("ids", "key_rows", "scores", "tokens", "hyp_score", "hyp_meta", "hyp_tokens", "worst", "state", "counters"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (pos, name)


def test_beam_state_reset_gives_the_fresh_state():
    import vlpet_amd.decode as D
    a = D.BeamState(2, 3, 6, "cpu", 2, 1, D.beam_key_rows(6, 6, "cpu"))
    b = D.BeamState(2, 3, 6, "cpu", 2, 1, D.beam_key_rows(6, 6, "cpu"))
    for t in (b.ids, b.key_rows, b.scores, b.tokens, b.hyp_score, b.hyp_meta, b.hyp_tokens, b.worst, b.state, b.counters):
        t.fill_(7)
    b.reset(2, 1)
    D.reset_key_rows(b.key_rows)
    for name in ("ids", "key_rows", "scores", "tokens", "hyp_score", "hyp_meta", "hyp_tokens", "worst", "state", "counters"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.scores.view(2, 3).tolist() == [[0.0, -1e9, -1e9]] * 2


# ---- generate(graph=True) on CPU tensors: the plain loop ------------------------------------------------------------------------

@pytest.mark.parametrize("name", GEN_FIXTURES)
def test_graph_generate_on_cpu_is_the_plain_loop_and_matches_the_greedy_golden(name):
    import vlpet_amd.decode as D
    from oracle.host_patch import cpu_reference_ops
    g = load_gen(name)
    model = build_host(g["fixture"])
    before = dict(D.GRAPH_STATS)
    with cpu_reference_ops():
        out = model.generate(g["ids"], g["vis"], g["task"], max_length=g["max_length"], min_length=g["min_length"],
                             no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"], graph=True)
    assert out.shape == g["out"].shape and torch.equal(out, g["out"])
    after = D.GRAPH_STATS
    assert after["eager"] == before["eager"] + 1
    assert all(after[k] == before[k] for k in ("captures", "replays", "warmups"))


@pytest.mark.parametrize("name", BEAM_FIXTURES)
def test_graph_generate_on_cpu_is_the_plain_loop_and_matches_the_beam_golden(name):
    import vlpet_amd.decode as D
    from oracle.host_patch import cpu_reference_ops
    g = load_beam(name)
    model = build_beam_host(g)
    before = dict(D.GRAPH_STATS)
    seen = []
    fin = D.beam_finalize
    D.beam_finalize = lambda *a, **k: seen.append(fin(*a, **k)) or seen[-1]
    try:
        with cpu_reference_ops():
            out = model.generate(g["ids"], g["vis"], g["task"], max_length=g["max_length"], min_length=g["min_length"],
                                 no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"], num_beams=g["K"], length_penalty=g["lp"],
                                 early_stopping=g["early"], graph=True)
    finally:
        D.beam_finalize = fin
    check_beam(out, seen[0][1], g)
    after = D.GRAPH_STATS
    assert after["eager"] == before["eager"] + 1
    assert all(after[k] == before[k] for k in ("captures", "replays", "warmups"))


def test_a_failed_entry_lets_go_of_its_buffers_and_its_model():
    """a key that stays on the plain loop (capture failed, a launch took a torch form) keeps nothing until eviction"""
    import vlpet_amd.decode as D
    enc = torch.randn(2, 5, 64)
    model = torch.nn.Linear(2, 2)
    for K in (1, 3):
        state = D.new_decode_state(enc, 64, 6, [enc], [enc], None, K)
        ent = D._GraphEntry(model, state, lambda st: (lambda tok, pos: None), 40, D.GenSettings(2, 3, 1, 6, 0, 0, K, 1.0, False, False))
        assert ent.state.pos_dev is ent.pos and not ent.failed
        ent.fail()
        assert ent.failed
        assert all(v is None for k, v in vars(ent).items() if torch.is_tensor(v) or k in ("model", "state", "step", "beam", "graph"))
        assert not any(torch.is_tensor(v) for v in vars(ent).values())
