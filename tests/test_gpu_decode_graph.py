"""GPU leg of the replayed decode step (csrc/decode.hip vlpet_*_at, vlpet_amd.decode.graph_generate, generate(graph=True)):
  * the four position-on-device kernel forms against their int siblings, bitwise on the output and on every buffer they write;
  * the guard: a position outside 0..pos_limit-1 writes nothing (the buffers are 8 rows larger than the limit handed over, so a
    launch without the guard would still stay inside its memory);
  * generate(graph=True) on the fp32 tiny fixtures: eager, capture, replay each equal the fixture, permuted rows come back permuted,
    a short call followed by a full-length one on the same entry equals the plain loop, an edited weight drops the graph, the cache
    stays at its bound;
  * full-size bf16 models: the replayed call under the teacher-forced rule of test_gpu_generate.py / test_gpu_beam.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _word(pos):
    return torch.tensor([pos], dtype=torch.int32, device=DEV)


# ---- the _at kernels against the int kernels --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D,H", [(16, 3), (16, 4), (64, 3), (64, 4)])
def test_attention_append_at_is_bitwise_the_int_form(D, H, dtype):
    import vlpet_amd.decode as DC
    B, L = 3, 72
    E = H * D
    gen = torch.Generator().manual_seed(D + H)
    kc0 = torch.randn(B, L, E, generator=gen).to(DEV, dtype)
    vc0 = torch.randn(B, L, E, generator=gen).to(DEV, dtype)
    table = (torch.randn(L, H, L, generator=gen) * 3).to(DEV)
    rows = torch.randint(0, B, (2, B, L), generator=gen, dtype=torch.int32).to(DEV)       # scattered histories, both parities
    n0 = DC.LAUNCHES["attn_decode"]
    cases = 0
    for pos in (0, 1, 7, 8, 63, 64):
        qkv = (torch.randn(B, 3 * E, generator=gen) * 2).to(DEV, dtype)
        q, kn, vn = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        for bias in (None, table):
            for kr in (None, rows):
                ka, va, kb, vb = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
                scale = 1.0 if bias is not None else None
                a = DC.decode_attention(q, ka, va, H, pos=pos, k_new=kn, v_new=vn, bias=None if bias is None else bias[pos],
                                        key_rows=None if kr is None else kr[pos & 1], scale=scale)
                b = DC.decode_attention(q, kb, vb, H, k_new=kn, v_new=vn, bias=bias, key_rows=kr, scale=scale, pos_dev=_word(pos))
                assert torch.equal(a, b), (pos, bias is not None, kr is not None)
                assert torch.equal(ka, kb) and torch.equal(va, vb)
                assert torch.equal(kb[:, pos], kn) and torch.equal(vb[:, pos], vn)
                cases += 1
    assert DC.LAUNCHES["attn_decode"] - n0 == 2 * cases          # both forms ran their kernels, no torch form


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [500, 50265])
def test_greedy_pick_at_is_bitwise_the_int_form(V, dtype):
    import vlpet_amd.decode as DC
    B, L = 3, 24
    gen = torch.Generator().manual_seed(V)
    n0 = DC.LAUNCHES["greedy_pick"]
    cases = 0
    for pos in (0, 5, 22):
        for eos, min_length, ngram in ((None, 0, 0), (3, 0, 0), (3, 8, 2), (3, 0, 3)):
            ids = torch.randint(10, 16, (B, L), generator=gen)
            ids[:, 0] = 2
            logits = torch.randn(B, (V + 7) // 8 * 8 + 8, generator=gen)
            logits[:, 10:16] += 6.0
            logits[0, 3] += 12.0                                        # row 0 wants eos
            unf = torch.tensor([1, 1, 0], dtype=torch.int32)            # row 2 has finished
            logits = logits.to(DEV, dtype)
            ia, ib, ua, ub = ids.to(DEV), ids.to(DEV), unf.to(DEV), unf.to(DEV)
            ca, cb = (torch.zeros(L, dtype=torch.int32, device=DEV) for _ in range(2))
            nt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
            kw = dict(eos_token_id=eos, pad_token_id=1, min_length=min_length, no_repeat_ngram_size=ngram)
            DC.greedy_pick(logits, V, ia, pos, ua, ca, **kw)
            DC.greedy_pick(logits, V, ib, None, ub, cb, pos_dev=_word(pos), next_tokens=nt, **kw)
            assert torch.equal(ia, ib) and torch.equal(ua, ub) and torch.equal(ca, cb), (pos, eos, min_length, ngram)
            assert torch.equal(nt, ib[:, pos + 1])
            cases += 1
    assert DC.LAUNCHES["greedy_pick"] - n0 == 2 * cases


BEAM_TENSORS = ("ids", "key_rows", "scores", "tokens", "hyp_score", "hyp_meta", "hyp_tokens", "worst", "state", "counters")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V,K,slices", [(500, 2, 1), (500, 2, 3), (500, 5, 1), (500, 5, 3), (500, 8, 1), (500, 8, 3), (50265, 5, None)])
def test_beam_kernels_at_are_bitwise_the_int_forms_over_six_steps(V, K, slices, dtype):
    """two states from fresh, one driven by ints and one by the device word advanced with add_: both parities, hypotheses, done
    items, the ban window and the forced step at force_eos_pos; every state tensor and the kernels' workspace after every step"""
    import vlpet_amd.decode as DC
    B, L, eos, pad, start = 3, 7, 3, 1, 2
    gen = torch.Generator().manual_seed(V + K + (slices or 0))
    a = DC.BeamState(B, K, L, DEV, start, pad, DC.beam_key_rows(B * K, L, DEV))
    b = DC.BeamState(B, K, L, DEV, start, pad, DC.beam_key_rows(B * K, L, DEV))
    word = _word(0)
    n0 = dict(DC.LAUNCHES)
    kw = dict(eos_token_id=eos, pad_token_id=pad, min_length=3, no_repeat_ngram_size=2, length_penalty=0.8, early_stopping=K % 2 == 0,
              slices=slices)
    for pos in range(L - 1):
        logits = torch.randn(B * K, (V + 7) // 8 * 8 + 8, generator=gen) * 3
        logits[:, V:] = float("inf")
        logits[:K, eos] += 6.0 + 2 * torch.rand(K, generator=gen)        # item 0 collects hypotheses and finishes early
        logits = logits.to(DEV, dtype)
        DC.beam_step(logits, V, a, pos, force_eos=pos == L - 2, **kw)
        DC.beam_step(logits, V, b, None, pos_dev=word, force_eos_pos=L - 2, **kw)
        word.add_(1)
        for name in BEAM_TENSORS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (pos, name)
        assert all(torch.equal(x, y) for x, y in zip(a._ws, b._ws)), pos
    assert int(word) == L - 1
    assert DC.LAUNCHES["beam_rows"] - n0["beam_rows"] == 2 * (L - 1) and DC.LAUNCHES["beam_advance"] - n0["beam_advance"] == 2 * (L - 1)


# ---- the guard ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos", ["limit", -1])
def test_a_position_outside_the_limit_writes_nothing(pos):
    """every buffer is allocated 8 rows (positions) past the limit the launch is given"""
    import vlpet_amd.decode as DC
    from vlpet_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    B, H, Dh, limit, cap = 3, 4, 16, 16, 24
    E = H * Dh
    word = _word(limit if pos == "limit" else pos)

    kc, vc = torch.randn(B, cap, E, generator=gen).to(DEV), torch.randn(B, cap, E, generator=gen).to(DEV)
    q, kn, vn = (torch.randn(B, E, generator=gen).to(DEV) for _ in range(3))
    table = torch.randn(cap, H, cap, generator=gen).to(DEV)
    rows = torch.zeros(2, B, cap, dtype=torch.int32, device=DEV)
    o = torch.full((B, E), 7.0, device=DEV)
    k0, v0 = kc.clone(), vc.clone()
    code = lib.vlpet_attn_decode_at(q.data_ptr(), E, kc.data_ptr(), vc.data_ptr(), E, cap * E, E, cap * E, kn.data_ptr(), vn.data_ptr(),
                                    E, word.data_ptr(), limit, None, 0, table.data_ptr(), cap, H * cap, o.data_ptr(), E, B, H, Dh,
                                    limit, 1.0, rows.data_ptr(), cap, B * cap, _lib.VLPET_F32, stream)
    assert code == 0
    assert torch.equal(kc, k0) and torch.equal(vc, v0) and bool((o == 7.0).all())

    V = 500
    logits = torch.randn(B, 504, generator=gen).to(DEV)
    ids = torch.randint(0, V, (B, limit + 1 + 8), generator=gen).to(DEV)
    unf = torch.ones(B, dtype=torch.int32, device=DEV)
    counters = torch.zeros(limit + 8, dtype=torch.int32, device=DEV)
    nt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    i0 = ids.clone()
    n0 = DC.LAUNCHES["greedy_pick"]
    DC.greedy_pick(logits, V, ids[:, :limit + 1], None, unf, counters[:limit], eos_token_id=3, pad_token_id=1, min_length=0,
                   no_repeat_ngram_size=2, pos_dev=word, next_tokens=nt)
    assert DC.LAUNCHES["greedy_pick"] == n0 + 1
    assert torch.equal(ids, i0) and bool((unf == 1).all()) and int(counters.sum()) == 0 and bool((nt == -7).all())

    K = 3
    st = DC.BeamState(B, K, limit + 1 + 8, DEV, 2, 1, DC.beam_key_rows(B * K, limit + 1 + 8, DEV))
    blog = torch.randn(B * K, 504, generator=gen).to(DEV)
    DC.beam_step(blog, V, st, 0, eos_token_id=3, pad_token_id=1)         # one int step: a live state and the workspace
    before = {n: getattr(st, n).clone() for n in BEAM_TENSORS}
    ws0 = [t.clone() for t in st._ws]
    big = {n: getattr(st, n) for n in ("ids", "hyp_tokens", "counters")}
    st.ids, st.hyp_tokens, st.counters = st.ids[:, :, :limit + 1], st.hyp_tokens[:, :limit], st.counters[:limit]     # the limit: 16
    n0 = DC.LAUNCHES["beam_advance"]
    DC.beam_step(blog, V, st, None, eos_token_id=3, pad_token_id=1, pos_dev=word, force_eos_pos=limit)
    assert DC.LAUNCHES["beam_advance"] == n0 + 1
    for n, t in big.items():
        setattr(st, n, t)
    for n in BEAM_TENSORS:
        assert torch.equal(getattr(st, n), before[n]), n
    assert all(torch.equal(x, y) for x, y in zip(st._ws, ws0))


# ---- generate(graph=True) on the fp32 tiny fixtures -----------------------------------------------------------------------------

def _names():
    from test_beam import BEAM_FIXTURES
    from test_generate import GEN_FIXTURES
    return list(GEN_FIXTURES) + list(BEAM_FIXTURES)


def _load(name):
    """(fixture dict, model on the device, generate keywords)"""
    if name.startswith("beam_"):
        from test_beam import build_beam_host, load_beam
        g = load_beam(name)
        model = build_beam_host(g)
        kw = dict(num_beams=g["K"], length_penalty=g["lp"], early_stopping=g["early"])
    else:
        from test_generate import build_host, load_gen
        g = load_gen(name)
        model = build_host(g["fixture"])
        kw = {}
    kw.update(max_length=g["max_length"], min_length=g["min_length"], no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"])
    return g, model.to(DEV), kw


def _gen(model, g, kw, rows=None, **more):
    """(ids on the host, beam scores or None, GRAPH_STATS delta) of one generate() call over the fixture's batch (or its ``rows``)"""
    import vlpet_amd.decode as DC
    ids, vis = g["ids"], g["vis"]
    if rows is not None:
        ids, vis = ids[rows], tuple(t[rows] for t in vis)
    seen = []
    fin = DC.beam_finalize
    DC.beam_finalize = lambda *a, **k: seen.append(fin(*a, **k)) or seen[-1]
    s0 = dict(DC.GRAPH_STATS)
    try:
        out = model.generate(ids.to(DEV), tuple(t.to(DEV) for t in vis), g["task"], **{**kw, **more})
    finally:
        DC.beam_finalize = fin
    return out.cpu(), (seen[0][1].cpu() if seen else None), {k: DC.GRAPH_STATS[k] - s0[k] for k in s0}


def _check(out, scores, g, rows=None):
    want, ws = g["out"], g.get("scores")
    if rows is not None:                    # a permutation of the batch: the same rows (the output width is the batch's longest row)
        want, ws = want[rows], None if ws is None else ws[rows]
    assert out.shape == want.shape and torch.equal(out, want), (out.tolist(), want.tolist())
    if ws is not None:
        torch.testing.assert_close(scores.double(), ws.double(), rtol=0, atol=1e-4)      # tests/test_beam.py's tolerance


@pytest.mark.parametrize("name", _names())
def test_graph_generate_eager_capture_replay_and_permuted_rows_match_the_fixture(name):
    import vlpet_amd.decode as DC
    g, model, kw = _load(name)
    steps = g["steps"] if "steps" in g else g["out"].shape[1] - 1
    n0 = dict(DC.LAUNCHES)
    out, scores, d = _gen(model, g, kw, graph=True)                      # first call of the key: eager, device-position launches
    _check(out, scores, g)
    assert d == dict(captures=0, replays=0, warmups=1, eager=0)
    n_layers = len(model.model.decoder.layers) if hasattr(model, "model") else len(model.decoder.block)
    assert DC.LAUNCHES["attn_decode"] - n0["attn_decode"] == 2 * n_layers * steps
    out, scores, d = _gen(model, g, kw, graph=True)                      # second: capture, then replays
    _check(out, scores, g)
    assert d == dict(captures=1, replays=steps, warmups=0, eager=0)
    out, scores, d = _gen(model, g, kw, graph=True)                      # third: replays only
    _check(out, scores, g)
    assert d == dict(captures=0, replays=steps, warmups=0, eager=0)
    perm = torch.tensor([2, 0, 3, 1])
    out, scores, d = _gen(model, g, kw, rows=perm, graph=True)           # the static buffers are refilled: nothing stale is read
    _check(out, scores, g, rows=perm)
    assert d == dict(captures=0, replays=steps, warmups=0, eager=0)


@pytest.mark.parametrize("name,row", [("gen_vlbart_vqa", 1), ("gen_vlt5_vqa", 0)])
def test_a_short_call_then_a_full_length_call_on_the_same_entry(name, row):
    """A batch of four copies of a row that ends early, then the fixture's batch, which runs to max_length: counters, unfinished
    flags, ids and the position start afresh.  (Beam search: the scripted decoder below -- the fixtures' models end on the same
    step whatever their input.)"""
    g, model, kw = _load(name)
    short = torch.tensor([row] * 4)
    want_short = _gen(model, g, kw, rows=short)[0]
    assert want_short.shape[1] < g["max_length"] == g["out"].shape[1]
    for _ in range(2):
        assert torch.equal(_gen(model, g, kw, rows=short, graph=True)[0], want_short)
    out, _, d = _gen(model, g, kw, rows=short, graph=True)
    assert torch.equal(out, want_short) and d["replays"] == want_short.shape[1] - 1
    out, _, d = _gen(model, g, kw, graph=True)
    _check(out, None, g)
    assert d == dict(captures=0, replays=g["max_length"] - 1, warmups=0, eager=0)
    out, _, d = _gen(model, g, kw, rows=short, graph=True)               # and back
    assert torch.equal(out, want_short) and d["replays"] == want_short.shape[1] - 1


class _ScriptedDecoder(torch.nn.Module):
    """A one-layer decoder over decode_attention whose cross-attention values decide when eos wins: graph_generate's own interface
    (state, make_step), small enough that a batch can be made to end at once or to run to max_length under ONE cache key."""
    H, Dh, V = 4, 16, 40

    def __init__(self):
        super().__init__()
        E = self.H * self.Dh
        gen = torch.Generator().manual_seed(0)
        self.emb = torch.nn.Parameter(torch.randn(self.V, E, generator=gen))
        self.head = torch.nn.Parameter(torch.randn(self.V, E, generator=gen) * 0.5)

    def state(self, enc, L, K):
        import vlpet_amd.decode as DC
        return DC.new_decode_state(enc, enc.shape[2], L, [enc], [enc], None, K)

    def make_step(self, st):
        import vlpet_amd.decode as DC

        def step(tok, pos):
            x = self.emb[tok]
            kr = st.key_rows if st.key_rows is None or st.pos_dev is not None else st.key_rows[pos & 1]
            ks, vs, kx, vx = st.layers[0]
            x = x + DC.decode_attention(x, ks, vs, self.H, pos=pos, k_new=x, v_new=x, key_rows=kr, pos_dev=st.pos_dev)
            x = x + DC.decode_attention(x, kx, vx, self.H, group=st.group)
            return F.linear(x, self.head)
        return step


@pytest.mark.parametrize("K", [1, 3])
def test_scripted_decoder_short_then_full_length_on_one_entry(K):
    """eos = 3: an encoder output along +head[eos] ends every row (item) at the first step, one along -head[eos] never lets eos
    win, so the loop runs to max_length; both under one key.  Each replayed call equals the plain loop over a fresh state."""
    import vlpet_amd.decode as DC
    torch.manual_seed(0)
    model = _ScriptedDecoder().to(DEV)
    B, Lk, L, eos = 3, 8, 9, 3
    E = model.H * model.Dh
    gs = DC.GenSettings(2, eos, 1, L, 0, 0, K, 1.0, False, K > 1)
    u = model.head[eos].detach() / model.head[eos].detach().norm()
    with torch.no_grad():
        encs = {"short": (60.0 * u).expand(B, Lk, E).contiguous(), "full": (-60.0 * u).expand(B, Lk, E).contiguous(),
                "mixed": torch.stack([60.0 * u, -60.0 * u, -60.0 * u])[:, None].expand(B, Lk, E).contiguous()}

        def plain(enc):
            st = model.state(enc, L, K)
            step = model.make_step(st)
            kernel = "beam_advance" if K > 1 else "greedy_pick"
            n0 = DC.LAUNCHES[kernel]
            if K > 1:
                out, scores = DC.beam_generate(step, model.V, B, K, DEV, L, 2, eos, 1, force_eos=True, key_rows=st.key_rows)
            else:
                out, scores = DC.greedy_generate(step, model.V, B, DEV, L, 2, eos, 1), None
            return out, scores, DC.LAUNCHES[kernel] - n0

        def replayed(enc):
            s0 = dict(DC.GRAPH_STATS)
            out = DC.graph_generate(model, model.state(enc, L, K), model.make_step, model.V, model.H, model.head, gs)
            return out, {k: DC.GRAPH_STATS[k] - s0[k] for k in s0}

        want = {n: plain(e) for n, e in encs.items()}
        assert want["short"][2] <= 3 and want["full"][2] == L - 1 == want["mixed"][2]      # steps
        assert replayed(encs["short"])[1]["warmups"] == 1
        assert replayed(encs["short"])[1]["captures"] == 1
        for name in ("short", "full", "mixed", "short", "full"):
            (out, scores), d = replayed(encs[name])
            assert torch.equal(out, want[name][0]), (name, out.tolist(), want[name][0].tolist())
            if K > 1:
                torch.testing.assert_close(scores, want[name][1], rtol=0, atol=1e-5)
            assert d["captures"] == 0 and d["eager"] == 0 and d["warmups"] == 0
            assert d["replays"] == want[name][2]


def test_an_edited_weight_drops_the_graph():
    import vlpet_amd.decode as DC
    g, model, kw = _load("gen_vlbart_vqa")
    for _ in range(3):
        out, _, d = _gen(model, g, kw, graph=True)
    assert d["replays"] > 0 and d["captures"] == 0
    name, p = next((n, p) for n, p in model.named_parameters() if "adapter" in n and p.dim() == 2)
    with torch.no_grad():
        p.mul_(-3.0)                                                    # in place: the parameter's version moves
    n_before = len(DC._GRAPHS)
    out, _, d = _gen(model, g, kw, graph=True)
    assert d == dict(captures=0, replays=0, warmups=1, eager=0), (name, d)           # the first-call rule again, no old graph
    assert len(DC._GRAPHS) == n_before                                 # the dead entry went, the new one came
    want = _gen(model, g, kw)[0]
    assert torch.equal(out, want)
    out, _, d = _gen(model, g, kw, graph=True)
    assert d["captures"] == 1 and torch.equal(out, want)
    out, _, d = _gen(model, g, kw, graph=True)
    assert d["captures"] == 0 and d["replays"] == want.shape[1] - 1 and torch.equal(out, want)


def test_the_graph_cache_stays_at_its_bound():
    import vlpet_amd.decode as DC
    g, model, kw = _load("gen_vlt5_vqa")
    saved = DC.MAX_GRAPHS
    DC.MAX_GRAPHS = 2
    try:
        DC._GRAPHS.clear()
        lengths = (4, 5, 6, 7)
        want = {L: _gen(model, g, {**kw, "max_length": L})[0] for L in lengths}
        for L in lengths:
            for _ in range(3):
                out, _, d = _gen(model, g, {**kw, "max_length": L}, graph=True)
                assert torch.equal(out, want[L]) and len(DC._GRAPHS) <= 2
            assert d["replays"] == want[L].shape[1] - 1
        assert len(DC._GRAPHS) == 2
        out, _, d = _gen(model, g, {**kw, "max_length": 7}, graph=True)  # the newest entry is still there
        assert d["replays"] > 0 and d["warmups"] == 0 and torch.equal(out, want[7])
        out, _, d = _gen(model, g, {**kw, "max_length": 4}, graph=True)  # the oldest went: first-call rule again, still correct
        assert d["warmups"] == 1 and torch.equal(out, want[4]) and len(DC._GRAPHS) == 2
    finally:
        DC.MAX_GRAPHS = saved
        DC._GRAPHS.clear()


# ---- full-size bf16 -------------------------------------------------------------------------------------------------------------

def _teacher_forced_check(model, kind, ids, vis, task, out, eos):
    """tests/test_gpu_generate.py's rule on tokens: equal to the teacher-forced argmax wherever its top-2 margin exceeds 0.05"""
    from test_gpu_generate import _teacher_forced_logits
    ref = _teacher_forced_logits(model, kind, ids, vis, task, out.to(DEV)).cpu()
    top = ref.topk(2, -1)
    sure = (top.values[..., 0] - top.values[..., 1]) > 0.05
    produced = out[:, 1:]
    alive = torch.ones_like(produced, dtype=torch.bool)
    alive[:, 1:] = (produced[:, :-1] != eos).cumprod(1).bool()
    check = sure & alive
    assert torch.equal(produced[check], top.indices[..., 0][check])
    return ref, check


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_full_size_bf16_replayed_greedy_matches_the_teacher_forced_decoder(kind):
    """VQA shape (B = 8, max_length 20).  Every step's logits (decode.GRAPH_STEP_HOOK: the captured step's output buffer after each
    replay) within 1e-2 of the scale of the teacher-forced decoder's, on the first (eager, device-position) call and on the replayed
    third call; the tokens of both equal to the teacher-forced argmax wherever its top-2 margin exceeds 0.05, and the replayed
    call's to the plain call's wherever that rule decides."""
    import vlpet_amd.decode as DC
    import vlpet_amd.train as TR
    from test_gpu_generate import _full_model
    model, cfg = _full_model(kind)
    b = TR.synthetic_batch("vqa", 8, cfg, DEV, torch.Generator(device=DEV).manual_seed(5), no_padding=False)
    ids, vis = b["input_ids"], b["vis_inputs"]
    ids[1, ids.shape[1] // 2:] = cfg.pad_token_id
    eos = 2 if kind != "t5" else 1
    kw = dict(max_length=20, eos_token_id=eos)
    plain = model.generate(ids, vis, "vqa", **kw).cpu()
    V = (model.shared if kind == "t5" else model.model.shared).weight.shape[0]
    seen = []
    DC.GRAPH_STEP_HOOK = lambda ent, pos: seen.append(ent.logits[:, :V].float().cpu())
    try:
        first = model.generate(ids, vis, "vqa", graph=True, **kw).cpu()
        first_logits = torch.stack(seen, 1)
        s0 = dict(DC.GRAPH_STATS)
        model.generate(ids, vis, "vqa", graph=True, **kw)
        del seen[:]
        third = model.generate(ids, vis, "vqa", graph=True, **kw).cpu()
        third_logits = torch.stack(seen, 1)
    finally:
        DC.GRAPH_STEP_HOOK = None
    assert DC.GRAPH_STATS["captures"] == s0["captures"] + 1 and DC.GRAPH_STATS["eager"] == s0["eager"]
    assert DC.GRAPH_STATS["replays"] - s0["replays"] >= third.shape[1] - 1
    ref, _ = _teacher_forced_check(model, kind, ids, vis, "vqa", first, eos)
    assert first_logits.shape == ref.shape and float((first_logits - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    ref, check = _teacher_forced_check(model, kind, ids, vis, "vqa", third, eos)
    assert third_logits.shape == ref.shape and float((third_logits - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    n = min(third.shape[1], plain.shape[1]) - 1
    same = check[:, :n]
    assert torch.equal(third[:, 1:n + 1][same], plain[:, 1:n + 1][same])


def test_full_size_bf16_replayed_beam_search_matches_the_teacher_forced_decoder():
    """BART, num_beams = 3, B = 4: the replayed call's sequence scores against the training-path decoder re-run on the returned
    sequences (tests/test_gpu_beam.py's rule), and against the plain call's under the same bound"""
    import vlpet_amd.decode as DC
    import vlpet_amd.train as TR
    from test_gpu_beam import _hyp_lengths
    from test_gpu_generate import _full_model, _teacher_forced_logits
    model, cfg = _full_model("bart")
    B, K, L, lp, eos, task = 4, 3, 20, 1.0, 2, "caption"
    b = TR.synthetic_batch(task, B, cfg, DEV, torch.Generator(device=DEV).manual_seed(7), no_padding=False)
    ids, vis = b["input_ids"], b["vis_inputs"]
    ids[1, ids.shape[1] // 2:] = cfg.pad_token_id
    seen, fin = [], DC.beam_finalize
    DC.beam_finalize = lambda *a, **k: seen.append(fin(*a, **k)) or seen[-1]
    s0 = dict(DC.GRAPH_STATS)
    try:
        kw = dict(max_length=L, eos_token_id=eos, num_beams=K, length_penalty=lp)
        model.generate(ids, vis, task, **kw)
        for _ in range(3):
            out = model.generate(ids, vis, task, graph=True, **kw)
    finally:
        DC.beam_finalize = fin
    assert DC.GRAPH_STATS["captures"] == s0["captures"] + 1 and DC.GRAPH_STATS["eager"] == s0["eager"]
    assert DC.GRAPH_STATS["replays"] > s0["replays"]
    plain_scores, scores = seen[0][1].float().cpu(), seen[-1][1].float().cpu()
    assert out.shape[0] == B and 2 <= out.shape[1] <= L
    lp_ref = torch.log_softmax(_teacher_forced_logits(model, "bart", ids, vis, task, out), -1).cpu()
    outc = out.cpu()
    for r, n in enumerate(_hyp_lengths(outc, eos, L)):
        last = min(n, outc.shape[1] - 1)
        total = sum(0.0 if p == L - 1 else float(lp_ref[r, p - 1, int(outc[r, p])]) for p in range(1, last + 1))
        want = total / n ** lp
        assert abs(want - float(scores[r])) <= 0.05 + 0.02 * abs(want), (r, want, float(scores[r]))
        assert abs(float(plain_scores[r]) - float(scores[r])) <= 0.05 + 0.02 * abs(want), (r, float(plain_scores[r]), float(scores[r]))
