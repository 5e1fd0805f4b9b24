"""GPU leg of greedy generation (csrc/decode.hip, vlpet_amd.decode, VLBart.generate / VLT5.generate):

  * vlpet_attn_decode against fp32 torch math on the same inputs: the self-attention step (append bit-exact, keys 0..pos), the
    cross-attention step over padded key masks with the key cache a column block of a fused projection, T5's bias row;
  * vlpet_greedy_pick against the torch restatement of tests/generate_spec.py: exact argmax with planted ties and +inf padding
    columns, min_length, no_repeat_ngram_size, finished rows, the per-step counter;
  * generate() in fp32 against the reference models' own greedy decoding (tests/golden/gen_*.npz) through both kernels;
  * full-size bf16 generate() (BART-base and T5-base VL-PET, LoRA r = 8, the VQA / caption / video encoder lengths) against the
    training-path decoder re-run on the produced ids (teacher forcing)."""
import pytest
import torch
import torch.nn.functional as F

import generate_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ref_attention(q, k, v, H, n, mask=None, bias=None, scale=None):
    B, E = q.shape
    D = E // H
    scale = D ** -0.5 if scale is None else scale
    qh = q.double().view(B, H, D)
    kh, vh = k[:, :n].double().reshape(B, n, H, D), v[:, :n].double().reshape(B, n, H, D)
    s = torch.einsum("bhd,bjhd->bhj", qh, kh) * scale
    if bias is not None:
        s = s + bias[None, :, :n].double()
    if mask is not None:
        s = s.masked_fill(~mask[:, None, :n].bool(), float("-inf"))
    return torch.einsum("bhj,bjhd->bhd", torch.softmax(s, -1), vh).reshape(B, E)


def _tol(dtype, ref):
    return (1e-2 if dtype == torch.bfloat16 else 1e-5) * max(1.0, float(ref.abs().max()))


def _rand(*shape, dtype, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV, dtype)


# B = 500 (the VQA evaluation batch) at two positions keeps the run short
SELF_CASES = [(pos, D, B) for pos in (0, 1, 31, 127, 511) for D, B in ((64, 1), (64, 3), (16, 3))] + [(0, 64, 500), (127, 64, 500)]
CROSS_CASES = [(Lk, D, B) for Lk in (56, 76, 92, 664) for D, B in ((64, 1), (64, 3), (16, 3))] + [(56, 64, 500), (664, 64, 500)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("pos,D,B", SELF_CASES)
def test_self_attention_step_appends_and_attends(pos, D, B, dtype):
    from vlpet_amd.decode import decode_attention
    H = 12 if D == 64 else 4
    E, Lmax = H * D, pos + 5
    gen = torch.Generator().manual_seed(pos * 7 + D + B)
    kc, vc = _rand(B, Lmax, E, dtype=dtype, gen=gen), _rand(B, Lmax, E, dtype=dtype, gen=gen)
    qkv = _rand(B, 3 * E, dtype=dtype, gen=gen, scale=2.0)          # the fused q|k|v row: column blocks read in place
    q, kn, vn = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    k0, v0 = kc.clone(), vc.clone()
    o = decode_attention(q, kc, vc, H, pos=pos, k_new=kn, v_new=vn)
    torch.cuda.synchronize()
    assert torch.equal(kc[:, pos], kn) and torch.equal(vc[:, pos], vn)                      # the append, bit-exact
    keep = torch.ones(Lmax, dtype=torch.bool, device=DEV)
    keep[pos] = False
    assert torch.equal(kc[:, keep], k0[:, keep]) and torch.equal(vc[:, keep], v0[:, keep])  # nothing else written
    ref = ref_attention(q, kc, vc, H, pos + 1)
    assert float((o.double() - ref).abs().max()) <= _tol(dtype, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("pos", [0, 5, 63])
def test_self_attention_step_with_t5_bias_row(pos, D, dtype):
    from vlpet_amd.decode import decode_attention
    H, B, Lmax = (12 if D == 64 else 4), 3, 64
    E = H * D
    gen = torch.Generator().manual_seed(11 + pos)
    kc, vc = _rand(B, Lmax, E, dtype=dtype, gen=gen), _rand(B, Lmax, E, dtype=dtype, gen=gen)
    q, kn, vn = (_rand(B, E, dtype=dtype, gen=gen) for _ in range(3))
    table = (torch.randn(Lmax, H, Lmax, generator=gen) * 3).to(DEV)          # [q, H, k] fp32, as T5Decoder.init_cache builds it
    o = decode_attention(q, kc, vc, H, pos=pos, k_new=kn, v_new=vn, bias=table[pos], scale=1.0)
    ref = ref_attention(q, kc, vc, H, pos + 1, bias=table[pos], scale=1.0)
    assert float((o.double() - ref).abs().max()) <= _tol(dtype, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lk,D,B", CROSS_CASES)
def test_cross_attention_step_over_a_fused_key_block_with_padding(Lk, D, B, dtype):
    from vlpet_amd.decode import decode_attention
    H = 12 if D == 64 else 4
    E, n_layers, layer = H * D, 6, 4
    gen = torch.Generator().manual_seed(Lk + D + B)
    keys = _rand(B, Lk, n_layers * E, dtype=dtype, gen=gen)              # functional.cross_key_blocks' output
    kc = keys[..., layer * E:(layer + 1) * E]
    vc = _rand(B, Lk, E, dtype=dtype, gen=gen)
    q = _rand(B, E, dtype=dtype, gen=gen, scale=3.0)
    lens = torch.randint(1, Lk + 1, (B,), generator=gen)
    lens[0] = Lk
    mask = (torch.arange(Lk)[None] < lens[:, None]).to(DEV)
    mask[:, -36:] = True                                                  # the visual tokens are always attended
    o = decode_attention(q, kc, vc, H, key_mask=mask)
    ref = ref_attention(q, kc, vc, H, Lk, mask=mask)
    assert float((o.double() - ref).abs().max()) <= _tol(dtype, ref)
    o2 = decode_attention(q, kc, vc, H)                                   # no mask
    ref2 = ref_attention(q, kc, vc, H, Lk)
    assert float((o2.double() - ref2).abs().max()) <= _tol(dtype, ref2)


def _pick_both(logits, V, ids, pos, unfinished, eos, pad, min_length, ngram):
    from vlpet_amd.decode import greedy_pick
    counters = torch.zeros(ids.shape[1], dtype=torch.int32, device=DEV)
    counters[pos] = 0
    want_tok, want_unf = S.greedy_step(logits, V, ids, pos, unfinished, eos, pad, min_length, ngram)
    greedy_pick(logits, V, ids, pos, unfinished, counters, eos_token_id=eos, pad_token_id=pad, min_length=min_length,
                no_repeat_ngram_size=ngram)
    torch.cuda.synchronize()
    assert torch.equal(ids[:, pos + 1].cpu(), want_tok)
    assert torch.equal(unfinished.cpu().long(), want_unf)
    assert int(counters[pos]) == int(want_unf.sum()) and int(counters.sum()) == int(want_unf.sum())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V,B", [(500, 3), (50465, 500), (32200, 7)])
def test_greedy_pick_exact_argmax_ties_and_padding_columns(V, B, dtype):
    from vlpet_amd.decode import LAUNCHES
    gen = torch.Generator().manual_seed(V + B)
    Vp = (V + 7) // 8 * 8 + 8
    logits = torch.randn(B, Vp, generator=gen)
    logits[:, V:] = float("inf")                                         # padded head columns: never picked
    top = logits[:, :V].max(1).values
    for b in range(B):                                                   # planted ties: the lowest index wins
        cols = torch.randperm(V, generator=gen)[:3]
        logits[b, cols] = top[b] + 1.0
    logits = logits.to(DEV, dtype)
    ids = torch.randint(0, V, (B, 20), generator=gen).to(DEV)
    unfinished = torch.ones(B, dtype=torch.int32, device=DEV)
    n0 = LAUNCHES["greedy_pick"]
    _pick_both(logits, V, ids, 4, unfinished, None, 1, 0, 0)
    assert LAUNCHES["greedy_pick"] == n0 + 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("ngram", [0, 2, 3])
def test_greedy_pick_processors_and_finished_rows(ngram, dtype):
    V, B, L = 500, 64, 24
    gen = torch.Generator().manual_seed(ngram)
    for pos in (0, 1, 2, 5, 12, 22):
        # a small alphabet makes repeated n-grams common; the logits favour that alphabet, so bans decide the pick
        ids = torch.randint(10, 16, (B, L), generator=gen)
        ids[:, 0] = 2
        logits = torch.randn(B, V + 4, generator=gen)
        logits[:, 10:16] += 6.0
        logits[:, 3] += 8.0 * (torch.rand(B, generator=gen) < 0.5)      # eos = 3 is the argmax of half the rows
        unfinished = (torch.rand(B, generator=gen) < 0.8).to(torch.int32)
        _pick_both(logits.to(DEV, dtype), V, ids.to(DEV), pos, unfinished.to(DEV), 3, 1, 6, ngram)


def _load_gen_and_model(name):
    from test_generate import build_host, load_gen
    g = load_gen(name)
    return g, build_host(g["fixture"]).to(DEV)


def _gen_names():
    from test_generate import GEN_FIXTURES
    return GEN_FIXTURES


@pytest.mark.parametrize("name", _gen_names())
def test_generate_matches_reference_greedy_gpu_fp32(name):
    from test_generate import check_against_fixture, run_generate
    from vlpet_amd.decode import LAUNCHES
    g, model = _load_gen_and_model(name)
    n0 = dict(LAUNCHES)
    out, logits = run_generate(model, g, DEV)
    check_against_fixture(out, logits, g, 1e-3)
    steps = out.shape[1] - 1
    n_layers = len(model.model.decoder.layers) if hasattr(model, "model") else len(model.decoder.block)
    assert LAUNCHES["greedy_pick"] - n0["greedy_pick"] == steps
    assert LAUNCHES["attn_decode"] - n0["attn_decode"] == 2 * n_layers * steps


def _full_model(kind, dtype=torch.bfloat16):
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    torch.manual_seed(0)
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        cfg = HT.vlt5_config()
        model = HT.VLT5(cfg)
    elif kind == "lora":
        cfg = HB.vlpet_config(use_adapter=False, use_encoder_adapter_down_multihead=False,
                              use_encoder_adapter_gating_large_x_lowrank=False,
                              use_decoder_enc_attn_value_parallel_adapter_down_dim=False, unfreeze_encoder_layer_norms=False,
                              use_lora=True, lora_dim=8, use_single_lora=True)
        model = HB.VLBart(cfg)
    elif kind == "video":
        cfg = HB.vlpet_config(feat_dim=512, n_boxes=64, tasks="tvqa,how2qa,tvc,yc2c")
        model = HB.VLBart(cfg)
    else:
        cfg = HB.vlpet_config()
        model = HB.VLBart(cfg)
    with torch.no_grad():                       # non-zero adapter / LoRA deltas so that K2 / K3 change the values they feed
        for n, p in model.named_parameters():
            if "lora_B" in n or "adapter" in n and "up" in n:
                p.normal_(0.0, 0.02)
    TR.trainable_names(model, cfg)
    model.to(DEV)
    TR.cast_frozen(model, dtype)
    return model.eval(), cfg


def _teacher_forced_logits(model, kind, ids, vis, task, out):
    from vlpet_amd.lmloss import _padded_head
    with torch.no_grad():
        if kind == "t5":
            enc, keep = model.encoder(ids, vis, None, task)
            h = model.decoder(out[:, :-1], enc, keep, task) * (model.config.d_model ** -0.5)
            w = model.shared.weight
        else:
            enc, mask = model.model.encoder(ids, vis, None, task, False)
            h = model.model.decoder(out[:, :-1], enc, mask, task)
            w = model.model.shared.weight
        V = w.shape[0]
        return F.linear(h, _padded_head(w, h.dtype))[..., :V].float()


@pytest.mark.parametrize("kind,task,B,max_length", [("bart", "vqa", 96, 20), ("bart", "caption", 48, 40), ("t5", "vqa", 64, 20),
                                                    ("t5", "caption", 32, 40), ("lora", "vqa", 64, 20), ("video", "tvqa", 8, 20)])
def test_full_size_bf16_generate_matches_the_teacher_forced_decoder(kind, task, B, max_length):
    import vlpet_amd.train as TR
    from test_generate import run_generate
    from vlpet_amd.decode import LAUNCHES
    model, cfg = _full_model(kind)
    gen = torch.Generator(device=DEV).manual_seed(5)
    b = TR.synthetic_batch(task, B, cfg, DEV, gen, no_padding=False)
    ids = b["input_ids"]
    ids[1, ids.shape[1] // 2:] = cfg.pad_token_id                      # one padded row: the key mask is live
    eos = 2 if kind != "t5" else 1
    g = dict(ids=ids, vis=b["vis_inputs"], task=task, max_length=max_length, min_length=0, ngram=0, eos=eos)
    n0 = dict(LAUNCHES)
    out, logits = run_generate(model, g, DEV)
    assert LAUNCHES["attn_decode"] > n0["attn_decode"] and LAUNCHES["greedy_pick"] > n0["greedy_pick"]
    assert out.shape[0] == B and 2 <= out.shape[1] <= max_length
    ref = _teacher_forced_logits(model, kind, ids, b["vis_inputs"], task, out.to(DEV)).cpu()
    assert ref.shape == logits.shape
    err = float((logits - ref).abs().max())
    assert err <= 1e-2 * float(ref.abs().max()), (err, float(ref.abs().max()))
    top = ref.topk(2, -1)
    sure = (top.values[..., 0] - top.values[..., 1]) > 0.05
    produced = out[:, 1:]
    alive = torch.ones_like(produced, dtype=torch.bool)                 # positions before (and at) a row's eos
    alive[:, 1:] = (produced[:, :-1] != eos).cumprod(1).bool()
    check = sure & alive
    assert torch.equal(produced[check], top.indices[..., 0][check])
