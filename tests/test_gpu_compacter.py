"""The Compacter baseline on the product path (GPU), mirroring test_gpu_single_adapter.py: the three model fixtures at test_host_golden.py's
GPU tolerance, a training step with dropout, greedy / beam generation against the reference's tokens, the replayed decode step against the
eager one, how often the weight expansion (csrc/phm.hip) runs during generate(), the staleness rule of the cached expanded weights under
an eager and an already captured decode, the fused adapter + tail launch on the expanded weights, and the captured train step."""
import copy

import pytest
import torch

import compacter_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _fresh_graphs():
    import vlpet_amd.decode as D
    from vlpet_amd import _lib
    D.clear_graphs()
    yield
    D.clear_graphs()
    _lib.load().vlpet_set_seed_counter(None)


@pytest.mark.parametrize("which", ["bart", "t5", "shared_fac"])
def test_eval_logits_and_training_losses_match_the_reference(which):
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(which)
    model, cfg, names, _ = C.build(which)
    assert names == C.trainable_names(which)
    _check(model.to(DEV), cfg, names, batches, ref_losses, hp, final, DEV, 1e-3)       # fp32 IO tolerance, as test_host_golden's GPU leg


@pytest.mark.parametrize("which", ["bart", "t5", "shared_fac"])
def test_training_step_with_dropout_reaches_every_phm_parameter(which):
    import vlpet_amd.functional as VF
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(which)[1]
    model, cfg, names, _ = C.build(which, dropout=0.1)
    model.to(DEV).train()
    torch.manual_seed(3)
    b = _to(batches[0], DEV)
    n0 = VF.PHM_CALLS
    per, _ = model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    assert VF.PHM_CALLS - n0 == len(C.adapters(model)) == 10          # one expansion per adapter and forward: 2 x 2 encoder, 3 x 2 decoder
    loss = TR.task_loss(per.float(), b["labels"], b["scores"], b["task"])
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    phm = [n for n in names if n.rsplit(".", 1)[-1] in ("phm_rule", "W", "W_left", "W_right", "b")]
    assert len(phm) == (61 if which == "shared_fac" else 60)           # per layer (W_left, W_right, b) + the model's rule | (rule, W, b)
    for n in phm:
        g = params[n].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n


def test_greedy_and_beam_tokens_equal_the_reference():
    from test_beam import check_against_fixture as check_beam, run_beam
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen()
    model = C.build("bart")[0].to(DEV)
    out, logits = run_generate(model, g, DEV)
    check_against_fixture(out, logits, g, 1e-3)
    b = C.load_beam()
    C.sharpen(model, b["logit_scale"])
    out, scores = run_beam(model, b, DEV)
    check_beam(out, scores, b)


def _gen_kwargs(kind, num_beams):
    if kind == "bart":
        g = C.load_gen()
        return g["ids"], g["vis"], g["task"], dict(max_length=g["max_length"], min_length=g["min_length"], no_repeat_ngram_size=g["ngram"],
                                                   eos_token_id=g["eos"], num_beams=num_beams)
    b = C.fixture("t5")[1][0]
    return b["input_ids"], b["vis_inputs"], b["task"], dict(max_length=8, min_length=8, num_beams=num_beams)


def _on_dev(kind, num_beams=1):
    ids, vis, task, kw = _gen_kwargs(kind, num_beams)
    return ids.to(DEV), tuple(t.to(DEV) for t in vis), task, kw


@pytest.mark.parametrize("num_beams", [1, 3])
@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_replayed_decode_step_gives_the_eager_tokens(kind, num_beams):
    import vlpet_amd.decode as D
    ids, vis, task, kw = _on_dev(kind, num_beams)
    model = C.build(kind)[0].to(DEV)
    eager = model.generate(ids, vis, task, **kw)
    s0 = dict(D.GRAPH_STATS)
    outs = [model.generate(ids, vis, task, graph=True, **kw) for _ in range(3)]          # eager warm-up, capture, replay
    d = {k: D.GRAPH_STATS[k] - s0[k] for k in s0}
    assert d["captures"] == 1 and d["replays"] > 0, d
    for o in outs:
        assert torch.equal(o, eager), (o.tolist(), eager.tolist())


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_generate_expands_each_adapter_at_most_once(kind):
    import vlpet_amd.functional as VF
    ids, vis, task, kw = _on_dev(kind)
    model = C.build(kind)[0].to(DEV)
    n_adapters = len(C.adapters(model))
    assert n_adapters == 10
    n0 = VF.PHM_CALLS
    out = model.generate(ids, vis, task, **kw)
    steps = out.shape[1] - 1
    assert steps >= 3
    assert 0 < VF.PHM_CALLS - n0 <= n_adapters, (VF.PHM_CALLS - n0, steps)              # not steps times that
    n0 = VF.PHM_CALLS
    model.generate(ids, vis, task, **kw)
    assert VF.PHM_CALLS == n0                                                           # nothing changed: every cache hits


def _scale_W(model, f):
    """an edit autograd's version counters do not see"""
    for _, m in C.phm_layers(model):
        m.W.data.mul_(f)


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_cached_weights_follow_a_parameter_change_eager_and_captured(kind):
    import vlpet_amd.decode as D
    import vlpet_amd.functional as VF
    ids, vis, task, kw = _on_dev(kind)
    model = C.build(kind)[0].to(DEV)
    before = model.generate(ids, vis, task, **kw)
    for _ in range(3):                                                                  # eager warm-up, capture, replay
        assert torch.equal(model.generate(ids, vis, task, graph=True, **kw), before)
    fresh = C.build(kind)[0]
    _scale_W(fresh, 10.0)
    want = fresh.to(DEV).generate(ids, vis, task, **kw)
    assert want.shape != before.shape or not torch.equal(want, before)                  # the change matters: other tokens
    buffers = [tuple(t.data_ptr() for t in ad.cached_weights()) for ad in C.adapters(model)]
    _scale_W(model, 10.0)
    VF.invalidate_caches()
    got_eager = model.generate(ids, vis, task, **kw)
    assert torch.equal(got_eager, want), (got_eager.tolist(), want.tolist())
    s0 = dict(D.GRAPH_STATS)
    for _ in range(3):          # (the decode graph is keyed on the weights epoch: the old one is dropped; warm-up, capture, replay again)
        got_graph = model.generate(ids, vis, task, graph=True, **kw)
        assert torch.equal(got_graph, want), (got_graph.tolist(), want.tolist())
    assert D.GRAPH_STATS["captures"] == s0["captures"] + 1 and D.GRAPH_STATS["replays"] > s0["replays"]
    # refreshed in place: the addresses an earlier capture holds are the ones the new weights were written to
    assert buffers == [tuple(t.data_ptr() for t in ad.cached_weights()) for ad in C.adapters(model)]


def _on_off(model, kind, run):
    """``run()`` with FUSE_ADAPTER_TAIL off, then on: (result off, result on, fused launches counted while on / while off)"""
    import vlpet_amd.adapter_tail as AT
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    mod = HB if kind == "bart" else HT
    saved = mod.FUSE_ADAPTER_TAIL
    try:
        mod.FUSE_ADAPTER_TAIL = False
        n0 = AT.CALLS
        off = run()
        n_off = AT.CALLS - n0
        mod.FUSE_ADAPTER_TAIL = True
        n0 = AT.CALLS
        on = run()
        n_on = AT.CALLS - n0
    finally:
        mod.FUSE_ADAPTER_TAIL = saved
    return off, on, n_on, n_off


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_fused_adapter_tail_runs_on_the_expanded_weights_and_changes_no_token(kind):
    from test_generate import run_generate
    ids, vis, task, kw = _gen_kwargs(kind, 1)
    g = dict(ids=ids, vis=vis, task=task, max_length=kw["max_length"], min_length=kw["min_length"], ngram=kw.get("no_repeat_ngram_size", 0),
             eos=kw.get("eos_token_id"))
    model = C.build(kind)[0].to(DEV)
    (out0, lg0), (out1, lg1), n_on, n_off = _on_off(model, kind, lambda: run_generate(model, g, DEV))
    assert torch.equal(out0, out1)
    steps = out1.shape[1] - 1
    # per step: 3 adapters per decoder layer x 2 layers; the prefill adds 2 per encoder layer x 2 layers
    assert n_off == 0 and n_on == 6 * steps + 4, (n_on, n_off, steps)
    err = float((lg1[:, 0] - lg0[:, 0]).abs().max())
    assert err <= 1e-2 * max(1.0, float(lg0[:, 0].abs().max())), err                 # the bf16 tolerance (fp32 run: far inside)


@pytest.mark.parametrize("which", ["bart", "shared_fac"])
def test_captured_train_step_reproduces_the_eager_trainer(which):
    """tolerances: tests/test_gpu_graph.py test_replayed_trainer_equals_eager_trainer (1e-5 relative on the losses and the parameters)"""
    import vlpet_amd.train as TR
    from test_host_golden import _to
    model, cfg, _, _ = C.build(which)
    model.train()
    m_eager, m_graph = copy.deepcopy(model).to(DEV), copy.deepcopy(model).to(DEV)
    b = _to(C.fixture(which)[1][0], DEV)
    tre = TR.Trainer(m_eager, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1)
    le = [float(tre.step(b)) for _ in range(4)]
    trg = TR.Trainer(m_graph, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1, graph=True)
    assert trg.graph
    lg = [float(trg.step(b)) for _ in range(4)]                                        # eager, capture + replay, replay, replay
    assert len(trg._graphs) == 1
    assert le[0] != le[3]                                                             # the steps change the weights
    for a, r in zip(lg, le):
        assert abs(a - r) <= 1e-5 * abs(r), (lg, le)
    ref = dict(m_eager.named_parameters())
    worst = max(float((p.detach() - ref[n].detach()).abs().max() / (ref[n].detach().abs().max() + 1e-12))
                for n, p in m_graph.named_parameters() if p.requires_grad)
    assert worst <= 1e-5, worst
