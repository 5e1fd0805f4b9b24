"""BitFit on the product path (GPU): the two reference fixtures (tests/golden/make_bitfit_goldens.py) on VLBart / VLT5 -- logits,
training, generation from the trained state -- and the bias-gradient sites (functional.linear_acc_bias / linear_acc_sep_bias /
cross_key_blocks with biases, act.linear_act_dropout) against the switch-off path, which is what a hand-unfrozen model ran before them.

Two models.  The fixtures are fp32 with 16-wide heads: the fc1 + activation site and the cross-attention k | v site run there; the
fused q | k | v projection and the fused cross keys need bf16 and 64-wide heads, so the call counts, the staleness check and the
partial-bias case use a randomly initialised VLBart of width 128 with two heads (``_wide``), frozen part cast to bf16.

Bounds.  Every bias gradient a site produces is held to tests/bitfit_spec.py: the fp64 sums of the dy THAT SITE READ (recorded in the
test), element by element under gamma_h sum |t|.  Across the switch-on and the switch-off leg the upstream differs by bf16 roundings, so
there only the losses are compared, at the repository's tolerances (fp32 1e-3, bf16 1e-2)."""
import copy

import pytest
import torch

import bitfit_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _restore_switch():
    import vlpet_amd.functional as VF
    saved = VF.FUSE_BIAS_GRAD_SITES
    yield
    VF.FUSE_BIAS_GRAD_SITES = saved
    from vlpet_amd import _lib
    _lib.load().vlpet_set_seed_counter(None)


def _calls():
    import vlpet_amd.functional as VF
    return dict(VF.BITFIT_CALLS)


def _delta(before):
    import vlpet_amd.functional as VF
    return {k: VF.BITFIT_CALLS[k] - before[k] for k in before}


def _wide(dropout=0.0, seed=0):
    """VLBart, d = 128, two heads of 64, two layers each side, frozen part in bf16, BitFit trainable set"""
    import vlpet_amd.train as TR
    cfg = C.config("bart", dropout, d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64)
    torch.manual_seed(seed)
    model = C.new_model("bart", cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "bias" in n:
                p.normal_(0.0, 0.05)            # (biases that matter: nn.Linear's default ones are fine, LayerNorm's are zero)
    names = TR.trainable_names(model, cfg)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    return model, cfg, names


def _batch(i=0):
    from test_host_golden import _to
    return _to(C.fixture("bart")[1][i], DEV)


def _loss_and_grads(model, b, seed=5):
    import vlpet_amd.train as TR
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    per, logits = model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    loss = TR.task_loss(per.float(), b["labels"], b["scores"], b["task"])
    loss.backward()
    return float(loss), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}, logits.detach().float()


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_eval_logits_training_losses_and_final_parameters_match_the_reference(kind, fused):
    from test_host_golden import _check
    import vlpet_amd.functional as VF
    VF.FUSE_BIAS_GRAD_SITES = fused
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, _ = C.build(kind)
    c0 = _calls()
    _check(model.to(DEV), cfg, names, batches, ref_losses, hp, final, DEV, 1e-3)
    d = _delta(c0)
    if kind == "bart" and fused:        # five steps: an fc1 + activation site per FFN (4), a cross-attention k | v site per decoder layer (2)
        assert d["act"] == 5 * 4 and d["seg"] >= 5 * 2 and d["fallback"] == 0, d
    else:                               # T5 has no Linear bias: no site, and the dense attention path gives the position tables their gradient
        assert d == {"seg": 0, "act": 0, "fallback": 0}, d


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_bf16_eval_logits_are_within_the_pinned_tolerance(kind):
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(kind)[1]
    model, cfg, names, _ = C.build(kind)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    model.eval()
    with torch.no_grad():
        for b in batches:
            bb = _to(b, DEV)
            per, logits = model(bb["input_ids"], bb["vis_inputs"], bb["labels"], b["task"])
            ref = b["logits"]
            assert float((logits.float().cpu() - ref).abs().max()) <= 1e-2 * max(1.0, float(ref.abs().max()))


def test_greedy_tokens_from_the_trained_state_equal_the_reference():
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen()
    model = C.load_trained(C.build("bart")[0]).to(DEV)
    out, logits = run_generate(model, g, DEV)
    check_against_fixture(out, logits, g, 1e-3)
    # ... and they are the TRAINED state's: the untrained biases give other logits
    out0, logits0 = run_generate(C.build("bart")[0].to(DEV), g, DEV)
    n = min(logits0.shape[1], logits.shape[1])
    assert float((logits0[:, :n] - g["logits"][:, :n]).abs().max()) > 2e-3          # (twice the tolerance the trained state is held to)


# ------------------------------------------------------------------------------------------------ every site against the spec
def _record_sites(monkeypatch):
    """Every site call of a backward, with what it summed: (kind, a copy of the dy it read -- the fused qkv dy, the shared dk buffer, a
    v dy, or the dpre the activation backward STORED --, its GradSlots, segment width)."""
    import vlpet_amd.act as ACT
    import vlpet_amd.functional as VF
    rec = []
    real_seg, real_act = VF.colsum_seg_into, ACT.act_bwd_cols_into

    def seg(dy2, slots, w):
        real_seg(dy2, slots, w)
        rec.append(("seg", dy2.detach().clone(), list(slots), w))

    def act(dy, pre, a, p, seed, io, slot):
        dpre = real_act(dy, pre, a, p, seed, io, slot)
        rec.append(("act", dpre.detach().reshape(-1, dpre.shape[-1]).clone(), [slot], dpre.shape[-1]))
        return dpre
    monkeypatch.setattr(VF, "colsum_seg_into", seg)
    monkeypatch.setattr(ACT, "act_bwd_cols_into", act)
    return rec


def _hold_sites_to_the_spec(rec, tag):
    """each recorded site's bias gradients against tests/bitfit_spec.py's fp64 sums OF THE SAME dy, element by element under the derived
    bound gamma_h sum |t|; a slot nobody asked for (NULL segment) does not exist; the parameter's .grad IS the slot's tensor"""
    import bitfit_spec as B
    torch.cuda.synchronize()
    worst, n_grads = 0.0, 0
    for kind, d, slots, w in rec:
        S = len(slots)
        assert d.shape[1] == S * w
        if kind == "seg":
            r = B.colsum_seg(d, S, w)
            ref, e = r.out, r.e_out
        else:
            s_, e_, _ = B.colsums_of_stored(d, w)
            ref, e = s_[None], e_[None]
        for i, sl in enumerate(slots):
            if sl is None:
                continue
            wr = B.worst(sl.t.reshape(-1), ref[i], e[i])
            worst, n_grads = max(worst, wr), n_grads + 1
            assert wr <= 1.0, (tag, kind, S, w, i, wr)
            if not sl.sunk:
                assert sl._p.grad is not None and torch.equal(sl._p.grad.float().reshape(-1), sl.t.reshape(-1)), (tag, kind, i)
    print(f"BITFIT sites {tag}: {len(rec)} site calls, {n_grads} bias gradients, worst err / bound {worst:.3f}")
    return n_grads


def test_fp32_every_site_gradient_is_the_spec_sum_of_the_dy_it_read(monkeypatch):
    """the fixture model in fp32: an fc1 + activation site per FFN (4) and the cross-attention's k | v sites (k and v of two decoder
    layers: 4 single-segment sums); the switch-off leg gives the same loss"""
    import vlpet_amd.functional as VF
    model = C.build("bart")[0].to(DEV)
    b = _batch()
    rec = _record_sites(monkeypatch)
    VF.FUSE_BIAS_GRAD_SITES = True
    c0 = _calls()
    l_on, g_on, _ = _loss_and_grads(model, b)
    d = _delta(c0)
    assert d["act"] == 4 and d["seg"] == 4 and d["fallback"] == 0, d
    assert _hold_sites_to_the_spec(rec, "fp32 fixture") == 8
    del rec[:]
    VF.FUSE_BIAS_GRAD_SITES = False
    c0 = _calls()
    l_off, g_off, _ = _loss_and_grads(model, b)
    assert _delta(c0) == {"seg": 0, "act": 0, "fallback": 0} and not rec
    assert l_on == pytest.approx(l_off, rel=1e-6)
    assert set(g_on) == set(g_off) == set(C.reference_names("bart"))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_bf16_every_site_gradient_is_the_spec_sum_of_the_dy_it_read(p, monkeypatch):
    """the bf16 model whose step holds every site: 4 fused q | k | v sums (3 segments each), the cross keys (2 segments), two v sums, four
    activation backwards -- 12 + 2 + 2 + 4 bias gradients, each against the fp64 sums of the dy its site read.  Between the switch-on and
    the switch-off leg the upstream differs by bf16 roundings, so across the legs only the losses are compared (bf16 tolerance)."""
    import vlpet_amd.functional as VF
    import vlpet_amd.train as TR
    model, cfg, names = _wide(dropout=p)
    b = _batch()
    rec = _record_sites(monkeypatch)
    VF.FUSE_BIAS_GRAD_SITES = True
    l_on, g_on, _ = _loss_and_grads(model, b)
    assert [k for k, *_ in rec].count("seg") == 7 and [k for k, *_ in rec].count("act") == 4
    assert _hold_sites_to_the_spec(rec, f"bf16 p={p}") == 20
    del rec[:]
    VF.FUSE_BIAS_GRAD_SITES = False
    l_off, g_off, _ = _loss_and_grads(model, b)
    assert not rec
    assert abs(l_on - l_off) <= 1e-2 * abs(l_off)
    assert set(g_on) == set(g_off) == set(names)
    monkeypatch.undo()
    losses = {}
    for fused in (True, False):
        VF.FUSE_BIAS_GRAD_SITES = fused
        m = copy.deepcopy(model)
        tr = TR.Trainer(m, cfg, lr=5e-3, total_steps=10, warmup_ratio=0.1)
        torch.manual_seed(11)
        losses[fused] = [float(tr.step(_batch(i % 3))) for i in range(5)]
    for a, r in zip(losses[True], losses[False]):
        assert abs(a - r) <= 1e-2 * max(1.0, abs(r)), losses


def test_call_counts_of_one_step():
    """two encoder layers, two decoder layers: a segmented sum per self-attention (4), one for the decoder's cross keys, one per
    cross-attention for v_proj.bias (its dy is a tensor of its own: one segment each, 2); a fused activation backward per FFN (4); no
    fallback"""
    model, cfg, names = _wide()
    c0 = _calls()
    _, grads, _ = _loss_and_grads(model, _batch())
    d = _delta(c0)
    assert d == {"seg": 4 + 1 + 2, "act": 4, "fallback": 0}, d
    assert set(grads) == set(names)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_only_q_bias_trainable_takes_the_fused_path_and_leaves_k_and_v_alone(monkeypatch):
    import vlpet_amd.functional as VF
    model, cfg, names = _wide()
    att = model.model.encoder.layers[0].self_attn.train()
    for p in att.parameters():
        p.requires_grad = False
    att.q_proj.bias.requires_grad = True
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 9, 128, generator=g).to(DEV, torch.bfloat16).requires_grad_(True)
    dy = torch.randn(3, 9, 128, generator=g).to(DEV, torch.bfloat16)
    res = {}
    rec = _record_sites(monkeypatch)
    for fused in (True, False):
        VF.FUSE_BIAS_GRAD_SITES = fused
        x.grad = att.q_proj.bias.grad = None
        c0 = _calls()
        att(x).backward(dy)
        res[fused] = (_delta(c0), att.q_proj.bias.grad.float().clone(), x.grad.float().clone())
        assert att.k_proj.bias.grad is None and att.v_proj.bias.grad is None
        if fused:       # one call, three segments, k and v not wanted
            assert len(rec) == 1 and [sl is None for sl in rec[0][2]] == [False, True, True]
            assert _hold_sites_to_the_spec(rec, "q bias only") == 1
    assert len(rec) == 1
    assert res[True][0] == {"seg": 1, "act": 0, "fallback": 0} and res[False][0] == {"seg": 0, "act": 0, "fallback": 0}
    for i in (1, 2):
        assert float((res[True][i] - res[False][i]).abs().max()) <= 1e-2 * float(res[False][i].abs().max())


def test_the_fused_bias_is_not_stale_after_fused_adamw_steps():
    """two optimizer steps through the flat-buffer AdamW (raw-pointer writes: no version counter moves), then the fused projection
    against the separate one; the cached fused bias must be the CURRENT parameters, bit for bit"""
    import vlpet_amd.functional as VF
    import vlpet_amd.train as TR
    model, cfg, names = _wide()
    att = model.model.encoder.layers[0].self_attn
    tr = TR.Trainer(model, cfg, lr=5e-2, total_steps=10, warmup_ratio=0.0)
    before = torch.cat([m.bias.detach().clone() for m in (att.q_proj, att.k_proj, att.v_proj)])
    for i in range(2):
        tr.step(_batch(i))
    now = torch.cat([m.bias.detach() for m in (att.q_proj, att.k_proj, att.v_proj)])
    assert float((now - before).abs().max()) > 1e-2                  # the biases moved: a bias two steps old would show
    model.train()
    x = torch.randn(2, 8, 128, device=DEV).to(torch.bfloat16).requires_grad_(True)
    VF.FUSE_BIAS_GRAD_SITES = True
    c0 = _calls()
    y_on = att(x)
    y_on.float().sum().backward()
    assert _delta(c0)["seg"] == 1
    assert torch.equal(att._qkv_cache[3], now.to(torch.bfloat16))
    VF.FUSE_BIAS_GRAD_SITES = False
    y_off = att(x)
    assert float((y_on.float() - y_off.float()).abs().max()) <= 1e-2 * float(y_off.float().abs().max())
    stale = torch.nn.functional.linear(x, att._qkv_cache[1], before.to(torch.bfloat16))
    fresh = torch.nn.functional.linear(x, att._qkv_cache[1], now.to(torch.bfloat16))
    assert float((stale.float() - fresh.float()).abs().max()) > 1e-2 * float(fresh.float().abs().max())


def test_a_captured_step_and_its_replays_give_the_eager_losses():
    """Trainer(graph=True) as the prompt baseline's graph test: eager step, capture + replay, replay -- on the fp32 fixture (1e-5) and on
    the bf16 model whose step holds every site (bf16 tolerance; the legs run the same kernels)"""
    import vlpet_amd.train as TR
    for model, cfg, tol in ((C.build("bart")[0].to(DEV), C.config("bart"), 1e-5), (*_wide()[:2], 1e-2)):
        m_eager, m_graph = copy.deepcopy(model), copy.deepcopy(model)
        b = _batch()
        tre = TR.Trainer(m_eager, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1)
        trg = TR.Trainer(m_graph, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1, graph=True)
        assert trg.graph
        le = [float(tre.step(b)) for _ in range(4)]
        lg = [float(trg.step(b)) for _ in range(4)]
        assert len(trg._graphs) == 1
        for x, y in zip(lg, le):
            assert abs(x - y) <= tol * abs(y), (lg, le)
        assert le[0] != le[3]                   # the biases train: the loss moves


def test_generate_after_training_uses_the_new_biases():
    """generate() before training fills the caches (fused q | k | v of the decode step, fused cross keys); after two FusedAdamW steps it
    must give what a model freshly built from the trained parameters gives"""
    import vlpet_amd.train as TR
    g = C.load_gen()
    model, cfg, names = _wide()
    kw = dict(max_length=8, min_length=8)
    ids, vis = g["ids"].to(DEV), tuple(t.to(DEV) for t in g["vis"])
    model.generate(ids, vis, g["task"], **kw)
    tr = TR.Trainer(model, cfg, lr=5e-2, total_steps=10, warmup_ratio=0.0)
    for i in range(2):
        tr.step(_batch(i))
    dec = model.model.decoder
    out = model.generate(ids, vis, g["task"], **kw)
    a0 = dec.layers[0].self_attn
    now = torch.cat([m.bias.detach() for m in (a0.q_proj, a0.k_proj, a0.v_proj)]).to(torch.bfloat16)
    assert torch.equal(a0._qkv_cache[3], now)
    ck = torch.cat([l.encoder_attn.k_proj.bias.detach() for l in dec.layers]).to(torch.bfloat16)
    assert torch.equal(dec._ck_cache[3], ck)
    fresh = C.new_model("bart", cfg)
    TR.trainable_names(fresh, cfg)
    fresh.to(DEV)
    TR.cast_frozen(fresh, torch.bfloat16)
    fresh.load_state_dict(model.state_dict(), strict=True)
    assert torch.equal(fresh.generate(ids, vis, g["task"], **kw), out)


def test_more_key_segments_than_one_call_takes_go_in_column_blocks():
    """a decoder with more than 16 layers: the shared dk buffer is summed 16 segments at a time, each call reading its column block of
    the buffer in place (row stride = the whole buffer's) -- the loop of functional._CrossKeyProjFn.backward"""
    import bitfit_spec as B
    import vlpet_amd.functional as VF
    n, E, M = 19, 64, 37
    g = torch.Generator().manual_seed(4)
    full = (torch.randn(M, n * E, generator=g) + 0.25).to(DEV, torch.bfloat16)
    slots = [None if i in (3, 17) else VF.GradSlot.scratch((E,), DEV) for i in range(n)]
    c0 = _calls()
    for s0 in range(0, n, VF.MAX_COLSUM_SEGS):
        part = slots[s0:s0 + VF.MAX_COLSUM_SEGS]
        VF.colsum_seg_into(full[:, s0 * E:(s0 + len(part)) * E], part, E)
    assert _delta(c0)["seg"] == 2
    torch.cuda.synchronize()
    r = B.colsum_seg(full, n, E)
    assert max(B.worst(sl.t, r.out[i], r.e_out[i]) for i, sl in enumerate(slots) if sl is not None) <= 1.0
