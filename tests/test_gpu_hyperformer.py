"""The Hyperformer baseline on the product path (GPU), mirroring test_gpu_compacter.py on both hosts: the three model fixtures at
test_host_golden.py's GPU tolerance, a training step with dropout that reaches every hyper-network parameter with one generator launch
(csrc/hyper.hip) per stack, greedy and beam generation against the reference's tokens, the replayed decode step against the eager one for two
tasks alternating on one model, how often the generator runs during generate(), the staleness rule of the cached generated weights
under an eager and an already captured decode, the fused adapter + tail launch on the generated weights, and the captured train step (one graph per task)."""
import copy

import pytest
import torch

import hyperformer_host_cases as C

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


@pytest.mark.parametrize("which", C.WHICH)
def test_eval_logits_and_training_losses_match_the_reference(which):
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(which)
    model, cfg, names, _ = C.build(which)
    assert names == C.trainable_names(which)
    _check(model.to(DEV), cfg, names, batches, ref_losses, hp, final, DEV, 1e-3)       # fp32 IO tolerance, as test_host_golden's GPU leg


@pytest.mark.parametrize("which", C.WHICH)
def test_training_step_with_dropout_reaches_every_hypernet_parameter_with_one_launch_per_stack(which):
    import vlpet_amd.functional as VF
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(which)[1]
    model, cfg, names, _ = C.build(which, dropout=0.1)
    model.to(DEV).train()
    torch.manual_seed(3)
    b = _to(batches[0], DEV)
    n0 = VF.HYPER_CALLS
    per, _ = model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    assert VF.HYPER_CALLS - n0 == 2                                   # one generator launch per stack and forward
    loss = TR.task_loss(per.float(), b["labels"], b["scores"], b["task"])
    loss.backward()
    assert torch.isfinite(loss)
    hyper = C.hyper_parameters(model)
    # 4 task embeddings; per stack the layer-id (and block-type) embeddings, the MLP's 4 and the LayerNorm's 2; 4 per generator pair
    assert len(hyper) == (4 + 2 * (8 + 2 * 4) if which == "one" else 4 + 7 + 4 * 4 + 7 + 6 * 4) and all(n in names for n, _ in hyper)
    for n, p in hyper:
        if "task_to_embeddings" in n and not n.endswith("." + b["task"]):
            assert p.grad is None or not bool(p.grad.any()), n        # another task's embedding
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n


@pytest.mark.parametrize("kind,which", [("bart", "unique"), ("t5", "t5")])
def test_greedy_tokens_equal_the_reference(kind, which):
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen(kind)
    model = C.build(which)[0].to(DEV)
    out, logits = run_generate(model, g, DEV)
    check_against_fixture(out, logits, g, 1e-3)


def test_beam_tokens_and_scores_equal_the_reference():
    """(the beam fixture is the T5 model's: tests/golden/make_hyperformer_goldens.py says why)"""
    from test_beam import check_against_fixture as check_beam, run_beam
    b = C.load_beam()
    model = C.build("t5")[0].to(DEV)
    C.sharpen_t5(model, b["logit_scale"])
    out, scores = run_beam(model, b, DEV)
    check_beam(out, scores, b)


def _on_dev(num_beams=1, which="unique"):
    g = C.load_gen(C.KIND[which])
    kw = dict(max_length=g["max_length"], min_length=g["min_length"], no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"],
              num_beams=num_beams)
    return g["ids"].to(DEV), tuple(t.to(DEV) for t in g["vis"]), kw


@pytest.mark.parametrize("num_beams", [1, 3])
@pytest.mark.parametrize("which", C.WHICH)
def test_replayed_decode_of_two_alternating_tasks_gives_the_eager_tokens(which, num_beams):
    """one model, two tasks in turn: each task has a captured step of its own (the task is in the graph key) that reads that task's
    generated weights"""
    import vlpet_amd.decode as D
    ids, vis, kw = _on_dev(num_beams, which)
    model = C.build(which)[0].to(DEV)
    tasks = ("vqa", "caption")
    eager = {t: model.generate(ids, vis, t, **kw) for t in tasks}
    s0 = dict(D.GRAPH_STATS)
    for rnd in range(4):                                              # per task: eager warm-up, capture, replay, replay
        for t in tasks:
            out = model.generate(ids, vis, t, graph=True, **kw)
            assert torch.equal(out, eager[t]), (rnd, t, out.tolist(), eager[t].tolist())
    d = {k: D.GRAPH_STATS[k] - s0[k] for k in s0}
    assert d["captures"] == 2 and d["replays"] > 0, d


@pytest.mark.parametrize("which", C.WHICH)
def test_generate_launches_the_generator_at_most_once_per_stack(which):
    import vlpet_amd.functional as VF
    ids, vis, kw = _on_dev(1, which)
    model = C.build(which)[0].to(DEV)
    n0 = VF.HYPER_CALLS
    out = model.generate(ids, vis, "vqa", **kw)
    assert out.shape[1] - 1 >= 3
    assert VF.HYPER_CALLS - n0 == 2                                   # not steps times that
    n0 = VF.HYPER_CALLS
    model.generate(ids, vis, "vqa", **kw)
    assert VF.HYPER_CALLS == n0                                       # nothing changed: both caches hit
    model.generate(ids, vis, "gqa", **kw)
    assert VF.HYPER_CALLS == n0 + 2                                   # another task: its own weights, once
    model.generate(ids, vis, "vqa", **kw)
    assert VF.HYPER_CALLS == n0 + 2


def _scale_generators(model, f):
    """an edit autograd's version counters do not see"""
    for n, p in model.named_parameters():
        if "sampler_hyper_net" in n and n.endswith("weight"):
            p.data.mul_(f)


def _cached_ptrs(model, task):
    out = []
    for stack in C.stacks(model)[1:]:
        for key, slot in stack.adapter_layers_hyper_net._cache.items():
            if key[0] == task:
                out += [t.data_ptr() for t in slot[1]] + [pk.buf.data_ptr() for pk in slot[2].values()]
    return out


@pytest.mark.parametrize("which", ["unique", "t5"])
def test_cached_weights_follow_a_parameter_change_eager_and_captured(which):
    import vlpet_amd.decode as D
    import vlpet_amd.functional as VF
    ids, vis, kw = _on_dev(1, which)
    task = "vqa"
    model = C.build(which)[0].to(DEV)
    before = model.generate(ids, vis, task, **kw)
    for _ in range(3):                                                                  # eager warm-up, capture, replay
        assert torch.equal(model.generate(ids, vis, task, graph=True, **kw), before)
    fresh = C.build(which)[0]
    _scale_generators(fresh, -3.0)
    want = fresh.to(DEV).generate(ids, vis, task, **kw)
    assert want.shape != before.shape or not torch.equal(want, before)                  # the change matters: other tokens
    buffers = _cached_ptrs(model, task)
    assert buffers
    _scale_generators(model, -3.0)
    VF.invalidate_caches()
    got_eager = model.generate(ids, vis, task, **kw)
    assert torch.equal(got_eager, want), (got_eager.tolist(), want.tolist())
    for _ in range(3):
        got_graph = model.generate(ids, vis, task, graph=True, **kw)
        assert torch.equal(got_graph, want), (got_graph.tolist(), want.tolist())
    # refreshed in place: the addresses an earlier capture holds are the ones the new weights were written to
    assert buffers == _cached_ptrs(model, task)
    # a change the version counters DO see needs no epoch: the next generate() refreshes, the captured step follows
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "sampler_hyper_net" in n and n.endswith("weight"):
                p.mul_(-1.0 / 3.0)
    back = model.generate(ids, vis, task, graph=True, **kw)
    assert torch.equal(back, before), (back.tolist(), before.tolist())


def test_fused_adapter_tail_runs_on_the_generated_weights_and_changes_no_token():
    import vlpet_amd.adapter_tail as AT
    import vlpet_amd.host.bart as HB
    from test_generate import run_generate
    g = C.load_gen()
    model = C.build("unique")[0].to(DEV)
    saved = HB.FUSE_ADAPTER_TAIL
    try:
        HB.FUSE_ADAPTER_TAIL = False
        n0 = AT.CALLS
        out0, lg0 = run_generate(model, g, DEV)
        n_off = AT.CALLS - n0
        HB.FUSE_ADAPTER_TAIL = True
        n0 = AT.CALLS
        out1, lg1 = run_generate(model, g, DEV)
        n_on = AT.CALLS - n0
    finally:
        HB.FUSE_ADAPTER_TAIL = saved
    assert torch.equal(out0, out1)
    steps = out1.shape[1] - 1
    # per step: 3 adapters per decoder layer x 2 layers; the prefill adds 2 per encoder layer x 2 layers
    assert n_off == 0 and n_on == 6 * steps + 4, (n_on, n_off, steps)
    err = float((lg1[:, 0] - lg0[:, 0]).abs().max())
    assert err <= 1e-2 * max(1.0, float(lg0[:, 0].abs().max())), err                 # the bf16 tolerance (fp32 run: far inside)


@pytest.mark.parametrize("which", ["unique", "t5"])
def test_captured_train_step_reproduces_the_eager_trainer(which):
    """three tasks in turn, three rounds: per task an eager step, the capture + replay, a replay.  The task embeddings are per-task
    parameters (only the current task's gets a gradient, AdamW skips the others: the ``final::`` fixtures pin that); each task's graph
    carries the set of parameters its step touches.  Tolerances: tests/test_gpu_graph.py test_replayed_trainer_equals_eager_trainer
    (1e-5 relative on the losses and the parameters)"""
    import vlpet_amd.functional as VF
    import vlpet_amd.train as TR
    from test_host_golden import _to
    model, cfg, _, _ = C.build(which)
    model.train()
    m_eager, m_graph = copy.deepcopy(model).to(DEV), copy.deepcopy(model).to(DEV)
    batches = [_to(b, DEV) for b in C.fixture(which)[1]]
    tre = TR.Trainer(m_eager, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1)
    le = [float(tre.step(batches[i % 3])) for i in range(9)]
    trg = TR.Trainer(m_graph, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1, graph=True)
    assert trg.graph and trg.flat.per_task
    lg = [float(trg.step(batches[i % 3])) for i in range(6)]
    assert len(trg._graphs) == 3
    n0 = VF.HYPER_CALLS
    lg += [float(trg.step(batches[i % 3])) for i in range(6, 9)]                        # replays only: no generator call from Python
    assert VF.HYPER_CALLS == n0 and len(trg._graphs) == 3
    assert le[0] != le[3]                                                             # the steps change the weights
    for a, r in zip(lg, le):
        assert abs(a - r) <= 1e-5 * abs(r), (lg, le)
    ref = dict(m_eager.named_parameters())
    worst = max(float((p.detach() - ref[n].detach()).abs().max() / (ref[n].detach().abs().max() + 1e-12))
                for n, p in m_graph.named_parameters() if p.requires_grad)
    assert worst <= 1e-5, worst
    # gqa never had a step: its embedding is untouched in both trainers
    name = [n for n, _ in m_graph.named_parameters() if n.endswith("task_to_embeddings.gqa")][0]
    assert torch.equal(dict(m_graph.named_parameters())[name].detach().cpu(), model.state_dict()[name])
