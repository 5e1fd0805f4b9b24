"""GPU leg of beam search (csrc/decode.hip vlpet_attn_decode_beam / vlpet_beam_rows / vlpet_beam_advance, vlpet_amd.decode
beam_generate, VLBart.generate / VLT5.generate with num_beams > 1):

  * grouped cross-attention and key-row self-attention against fp64 torch math on scattered tables (append bit-exact into batch r);
  * vlpet_beam_rows + vlpet_beam_advance against beam_spec: the top 2K and the scorer walk on random and planted tables, one slice
    against several, the forced-eos step, bans, done items; every state tensor against the torch form step by step;
  * generate() in fp32 against the reference models' own beam search (tests/golden/beam_*.npz) through the kernels;
  * full-size bf16 generate(num_beams = 5) against the training-path decoder re-run on the returned sequences (their scores);
  * full-size fp32: the kernels and decode.EAGER give the same ids; num_beams = 1 is the greedy path and launches no beam kernel."""
import pytest
import torch
import torch.nn.functional as F

import beam_spec as BS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ref_attention(q, k, v, H, mask=None, bias=None, scale=None):
    """q [R, E], k / v [R, n, E] already gathered per row"""
    R, E = q.shape
    D = E // H
    n = k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    s = torch.einsum("bhd,bjhd->bhj", q.double().view(R, H, D), k.double().view(R, n, H, D)) * scale
    if bias is not None:
        s = s + bias[None, :, :n].double()
    if mask is not None:
        s = s.masked_fill(~mask[:, None, :n].bool(), float("-inf"))
    return torch.einsum("bhj,bjhd->bhd", torch.softmax(s, -1), v.double().view(R, n, H, D)).reshape(R, E)


def _tol(dtype, ref):
    return (1e-2 if dtype == torch.bfloat16 else 1e-5) * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,K,Lk,D", [(1, 1, 56, 64), (3, 5, 664, 64), (50, 5, 664, 64), (3, 5, 92, 16), (30, 5, 76, 64)])
def test_grouped_cross_attention_reads_each_item_cache_for_its_beams(B, K, Lk, D, dtype):
    from vlpet_amd.decode import LAUNCHES, decode_attention
    H = 12 if D == 64 else 4
    E = H * D
    gen = torch.Generator().manual_seed(B * 7 + Lk)
    fused = (torch.randn(B, Lk, 3 * E, generator=gen)).to(DEV, dtype)      # the key cache: a column block of a fused projection
    kc, vc = fused[:, :, E:2 * E], torch.randn(B, Lk, E, generator=gen).to(DEV, dtype)
    q = torch.randn(B * K, E, generator=gen).to(DEV, dtype) * 2
    mask = torch.ones(B, Lk, dtype=torch.bool)
    for b in range(B):
        mask[b, Lk - (b * 13) % (Lk // 2):] = False
    mask = mask.to(DEV)
    n0 = LAUNCHES["attn_decode"]
    o = decode_attention(q, kc, vc, H, key_mask=mask, group=K)
    assert LAUNCHES["attn_decode"] == n0 + 1
    ref = ref_attention(q, kc.repeat_interleave(K, 0), vc.repeat_interleave(K, 0), H, mask=mask.repeat_interleave(K, 0))
    assert float((o.double() - ref).abs().max()) <= _tol(dtype, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,pos,D,t5", [(1, 0, 64, False), (15, 19, 64, False), (15, 39, 16, True), (250, 25, 64, False),
                                            (250, 33, 64, True)])
def test_key_row_self_attention_follows_the_table_and_appends_into_row_r(rows, pos, D, t5, dtype):
    from vlpet_amd.decode import decode_attention
    H = 12 if D == 64 else 4
    E, Lmax = H * D, 40
    gen = torch.Generator().manual_seed(rows + pos + D)
    kc = torch.randn(rows, Lmax, E, generator=gen).to(DEV, dtype)
    vc = torch.randn(rows, Lmax, E, generator=gen).to(DEV, dtype)
    qkv = torch.randn(rows, 3 * E, generator=gen).to(DEV, dtype)
    q, kn, vn = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    table = torch.randint(0, rows, (rows, Lmax), generator=gen, dtype=torch.int32).to(DEV)     # scattered histories
    bias = (torch.randn(H, Lmax, generator=gen) * 3).to(DEV) if t5 else None
    k0, v0 = kc.clone(), vc.clone()
    o = decode_attention(q, kc, vc, H, pos=pos, k_new=kn, v_new=vn, key_rows=table, bias=bias, scale=1.0 if t5 else None)
    torch.cuda.synchronize()
    assert torch.equal(kc[:, pos], kn) and torch.equal(vc[:, pos], vn)                        # the append, bit-exact, batch r
    keep = torch.ones(Lmax, dtype=torch.bool, device=DEV)
    keep[pos] = False
    assert torch.equal(kc[:, keep], k0[:, keep]) and torch.equal(vc[:, keep], v0[:, keep])
    kr = table[:, :pos + 1].long().clone()
    kr[:, pos] = torch.arange(rows, device=DEV)
    j = torch.arange(pos + 1, device=DEV)[None].expand(rows, -1)
    ref = ref_attention(q, kc[kr, j], vc[kr, j], H, bias=bias, scale=1.0 if t5 else None)
    assert float((o.double() - ref).abs().max()) <= _tol(dtype, ref)


# ---- vlpet_beam_rows + vlpet_beam_advance --------------------------------------------------------------------------------------

def _states(B, K, L, start, pad):
    import vlpet_amd.decode as D
    a = D.BeamState(B, K, L, DEV, start, pad, D.beam_key_rows(B * K, L, DEV))
    b = D.BeamState(B, K, L, DEV, start, pad, D.beam_key_rows(B * K, L, DEV))
    return a, b


def _same_state(a, b, cur_len, tol):
    nxt = cur_len & 1           # the half the last step wrote
    assert torch.equal(a.ids[nxt][:, :cur_len + 1], b.ids[nxt][:, :cur_len + 1])
    assert torch.equal(a.key_rows[nxt][:, :cur_len + 1], b.key_rows[nxt][:, :cur_len + 1])
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.state, b.state)
    torch.testing.assert_close(a.scores, b.scores, rtol=0, atol=tol)
    torch.testing.assert_close(a.worst, b.worst, rtol=0, atol=tol)
    live = torch.arange(a.K, device=DEV)[None] < a.state[:, :1]
    live = live.reshape(-1)
    torch.testing.assert_close(a.hyp_score[live], b.hyp_score[live], rtol=0, atol=tol)
    assert torch.equal(a.hyp_meta[live], b.hyp_meta[live])
    for r in torch.nonzero(live).flatten().tolist():
        n = int(a.hyp_meta[r, 0])
        assert torch.equal(a.hyp_tokens[r, :n], b.hyp_tokens[r, :n])


@pytest.mark.parametrize("dtype", [torch.float32])
@pytest.mark.parametrize("V,K,B,slices", [(500, 2, 4, None), (500, 5, 3, 1), (500, 8, 2, 3), (32100, 5, 6, None),
                                          (32100, 8, 3, 1), (50265, 5, 50, None), (50265, 5, 5, 1), (50265, 2, 7, 7)])
def test_beam_kernels_match_the_torch_form_step_by_step(V, K, B, slices, dtype):
    """eos planted high in half of the items (hypotheses, eos of rank >= K, early done items), a ban window (min_length and
    no_repeat_ngram_size = 2), the forced-eos step last; every state tensor compared after every step"""
    import vlpet_amd.decode as D
    L, eos, pad, start = 8, 3, 1, 2
    gen = torch.Generator().manual_seed(V + K + B)
    hip, ref = _states(B, K, L, start, pad)
    Vp = (V + 7) // 8 * 8 + 8
    n0 = dict(D.LAUNCHES)
    for pos in range(L - 1):
        logits = torch.randn(B * K, Vp, generator=gen) * 3
        logits[:, V:] = float("inf")                                  # padding columns past V never count
        hot = (torch.arange(B * K) // K) % 2 == 0
        logits[hot, eos] += 6.0 + 2 * torch.rand(int(hot.sum()), generator=gen)
        logits = logits.to(DEV, dtype)
        kw = dict(eos_token_id=eos, pad_token_id=pad, min_length=3, no_repeat_ngram_size=2, length_penalty=0.8,
                  early_stopping=K % 2 == 0, force_eos=pos == L - 2)
        D.beam_step(logits, V, hip, pos, slices=slices, **kw)
        saved = D.EAGER
        D.EAGER = True
        try:
            D.beam_step(logits, V, ref, pos, **kw)
        finally:
            D.EAGER = saved
        torch.cuda.synchronize()
        _same_state(hip, ref, pos + 1, 1e-4)
        assert int(hip.counters[pos]) == int(ref.counters[pos])
    assert D.LAUNCHES["beam_rows"] - n0["beam_rows"] == L - 1 and D.LAUNCHES["beam_advance"] - n0["beam_advance"] == L - 1


@pytest.mark.parametrize("K", [2, 5, 8])
def test_beam_kernels_first_step_against_beam_spec(K):
    """the first step (only beam 0 live) of random fp32 tables: the kernels' next tokens / sources / scores are beam_spec's"""
    import vlpet_amd.decode as D
    B, V, L, eos, pad = 5, 50265, 6, 7, 1
    gen = torch.Generator().manual_seed(K)
    logits = torch.randn(B * K, V + 7, generator=gen) * 4
    logits[:2 * K, eos] += 20.0                                    # item 0-1: eos on top of beam 0 -> one hypothesis each
    hip = D.BeamState(B, K, L, DEV, 2, pad)
    D.beam_step(logits.to(DEV), V, hip, 0, eos_token_id=eos, pad_token_id=pad)
    x = BS.row_scores(logits, V, [[2]] * (B * K), 1, eos, 0, 0, False)
    bs = torch.zeros(B, K)
    bs[:, 1:] = BS.NEG_INIT
    top_v, top_i = BS.top_flat((x + bs.view(-1, 1)).view(B, K * V), 2 * K)
    hyps = [BS.Hyps(K, 1.0, False) for _ in range(B)]
    s, t, src, _ = BS.process([[2]] * (B * K), top_v, top_i, V, K, hyps, [False] * B, eos, pad)
    assert hip.tokens.tolist() == t
    assert hip.ids[1][:, 0].tolist() == [2] * (B * K) and hip.ids[1][:, 1].tolist() == t
    torch.testing.assert_close(hip.scores.cpu(), torch.tensor(s), rtol=0, atol=1e-4)
    assert hip.state[:, 0].tolist() == [len(h) for h in hyps]
    for b, h in enumerate(hyps):
        for j, (score, toks, _) in enumerate(h.beams):
            assert abs(float(hip.hyp_score[b * K + j]) - score) < 1e-4 and hip.hyp_tokens[b * K + j, :len(toks)].tolist() == toks


# ---- generate() -----------------------------------------------------------------------------------------------------------------

def _beam_names():
    from test_beam import BEAM_FIXTURES
    return BEAM_FIXTURES


@pytest.mark.parametrize("name", _beam_names())
def test_generate_matches_reference_beam_search_gpu_fp32(name):
    from test_beam import build_beam_host, check_against_fixture, load_beam, run_beam
    from vlpet_amd.decode import LAUNCHES
    g = load_beam(name)
    model = build_beam_host(g).to(DEV)
    n0 = dict(LAUNCHES)
    out, scores = run_beam(model, g, DEV)
    check_against_fixture(out, scores, g)
    steps = g["steps"]
    n_layers = len(model.model.decoder.layers) if hasattr(model, "model") else len(model.decoder.block)
    assert LAUNCHES["beam_rows"] - n0["beam_rows"] == steps and LAUNCHES["beam_advance"] - n0["beam_advance"] == steps
    assert LAUNCHES["attn_decode"] - n0["attn_decode"] == 2 * n_layers * steps


def _hyp_lengths(out, eos, max_length):
    """the hypothesis length of every output row: the position of its eos, or max_length for an open beam"""
    lens = []
    for row in out.tolist():
        lens.append(next((i for i, t in enumerate(row) if i > 0 and t == eos), len(row)))
    assert all(n == max_length or n < len(r) for n, r in zip(lens, out.tolist()))
    return lens


@pytest.mark.parametrize("kind,task,B", [("bart", "caption", 16), ("t5", "caption", 12), ("lora", "vqa", 16), ("video", "tvc", 6)])
def test_full_size_bf16_beam_scores_match_the_teacher_forced_decoder(kind, task, B):
    import vlpet_amd.train as TR
    import vlpet_amd.decode as D
    from test_gpu_generate import _full_model, _teacher_forced_logits
    model, cfg = _full_model(kind)
    gen = torch.Generator(device=DEV).manual_seed(7)
    b = TR.synthetic_batch(task, B, cfg, DEV, gen, no_padding=False)
    ids = b["input_ids"]
    ids[1, ids.shape[1] // 2:] = cfg.pad_token_id
    eos = 2 if kind != "t5" else 1
    K, L, lp = 5, 20, 1.0
    seen = []
    bg = D.beam_generate
    D.beam_generate = lambda *a, **k: seen.append(bg(*a, **k)) or seen[-1]
    n0 = dict(D.LAUNCHES)
    try:
        out = model.generate(ids, b["vis_inputs"], task, max_length=L, eos_token_id=eos, num_beams=K, length_penalty=lp)
    finally:
        D.beam_generate = bg
    assert D.LAUNCHES["beam_rows"] > n0["beam_rows"] and D.LAUNCHES["attn_decode"] > n0["attn_decode"]
    scores = seen[0][1].float().cpu()
    assert out.shape[0] == B and 2 <= out.shape[1] <= L
    lp_ref = torch.log_softmax(_teacher_forced_logits(model, kind, ids, b["vis_inputs"], task, out), -1).cpu()
    outc = out.cpu()
    for r, n in enumerate(_hyp_lengths(outc, eos, L)):
        last = min(n, outc.shape[1] - 1)                               # the eos (if any) is scored, the positions after it not
        total = 0.0
        for p in range(1, last + 1):
            tok = int(outc[r, p])
            forced = kind != "t5" and p == L - 1                        # BART's forced step: eos at log-prob 0
            total += 0.0 if forced else float(lp_ref[r, p - 1, tok])
        want = total / n ** lp
        assert abs(want - float(scores[r])) <= 0.05 + 0.02 * abs(want), (r, want, float(scores[r]))


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_full_size_fp32_kernels_and_eager_give_the_same_beams(kind):
    import vlpet_amd.train as TR
    import vlpet_amd.decode as D
    import vlpet_amd.host.bart as HB
    model, cfg = _full_model_fp32(kind)
    gen = torch.Generator(device=DEV).manual_seed(11)
    task = "caption"
    b = TR.synthetic_batch(task, 6, cfg, DEV, gen, no_padding=False)
    eos = 2 if kind != "t5" else 1
    kw = dict(max_length=12, eos_token_id=eos, num_beams=4, length_penalty=1.0)
    hip = model.generate(b["input_ids"], b["vis_inputs"], task, **kw)
    saved = (D.EAGER, HB.EAGER_ATTENTION)
    D.EAGER = HB.EAGER_ATTENTION = True
    try:
        n0 = dict(D.LAUNCHES)
        eager = model.generate(b["input_ids"], b["vis_inputs"], task, **kw)
        assert D.LAUNCHES == n0
    finally:
        D.EAGER, HB.EAGER_ATTENTION = saved
    assert torch.equal(hip, eager), (hip.tolist(), eager.tolist())


def _full_model_fp32(kind):
    from test_gpu_generate import _full_model
    return _full_model(kind, torch.float32)


def test_num_beams_one_is_the_greedy_path_and_launches_no_beam_kernel():
    import vlpet_amd.train as TR
    import vlpet_amd.decode as D
    from test_gpu_generate import _full_model
    model, cfg = _full_model("bart")
    gen = torch.Generator(device=DEV).manual_seed(3)
    b = TR.synthetic_batch("vqa", 32, cfg, DEV, gen, no_padding=False)
    a = model.generate(b["input_ids"], b["vis_inputs"], "vqa", max_length=10)
    n0 = dict(D.LAUNCHES)
    c = model.generate(b["input_ids"], b["vis_inputs"], "vqa", max_length=10, num_beams=1)
    assert torch.equal(a, c)
    assert D.LAUNCHES["beam_rows"] == n0["beam_rows"] and D.LAUNCHES["beam_advance"] == n0["beam_advance"]
    assert D.LAUNCHES["greedy_pick"] > n0["greedy_pick"]
