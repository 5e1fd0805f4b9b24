"""The Single-Adapter baseline on the product path (GPU): the two model fixtures at test_host_golden.py's GPU tolerances, a training step
with dropout, greedy / beam generation against the reference's tokens, the replayed decode step against the eager one, and the fused
adapter + tail launch (vlpet_amd.adapter_tail) against the K2 + K5 composition it replaces inside generate()."""
import pytest
import torch

import single_adapter_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _fresh_graphs():
    import vlpet_amd.decode as D
    D.clear_graphs()
    yield
    D.clear_graphs()


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_eval_logits_and_training_losses_match_the_reference(kind):
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, _ = C.build(kind)
    _check(model.to(DEV), cfg, names, batches, ref_losses, hp, final, DEV, 1e-3)       # fp32 IO tolerance, as test_host_golden's GPU leg


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_training_step_with_dropout_reaches_every_trainable_parameter(kind):
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(kind)[1]
    model, cfg, names, _ = C.build(kind, dropout=0.1)
    model.to(DEV).train()
    torch.manual_seed(3)
    b = _to(batches[0], DEV)
    per, _ = model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    loss = TR.task_loss(per.float(), b["labels"], b["scores"], b["task"])
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    for n in names:
        g = params[n].grad
        if "obj_order_embedding" in n or "img_order_embedding" in n:      # (tables the vqa batch may not index)
            continue
        assert g is not None and bool(torch.isfinite(g).all()), n
    adapters = [n for n in names if "adapter" in n]
    assert adapters and all(float(params[n].grad.abs().max()) > 0 for n in adapters)


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


@pytest.mark.parametrize("num_beams", [1, 3])
@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_replayed_decode_step_gives_the_eager_tokens(kind, num_beams):
    import vlpet_amd.decode as D
    ids, vis, task, kw = _gen_kwargs(kind, num_beams)
    model = C.build(kind)[0].to(DEV)
    ids, vis = ids.to(DEV), tuple(t.to(DEV) for t in vis)
    eager = model.generate(ids, vis, task, **kw)
    s0 = dict(D.GRAPH_STATS)
    outs = [model.generate(ids, vis, task, graph=True, **kw) for _ in range(3)]          # eager warm-up, capture, replay
    d = {k: D.GRAPH_STATS[k] - s0[k] for k in s0}
    assert d["captures"] == 1 and d["replays"] > 0, d
    for o in outs:
        assert torch.equal(o, eager), (o.tolist(), eager.tolist())


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
def test_fused_launch_is_taken_and_changes_no_token(kind):
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


def test_full_size_bf16_decode_takes_the_fused_launch_within_tolerance():
    """BART-base with the script's adapters (d = 768, r = 96), bf16 backbone, fp32 adapters: the (768, 96) kernel inside generate()"""
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    from test_generate import run_generate
    torch.manual_seed(0)
    cfg = HB.vlpet_config(**C.FLAGS)
    model = HB.VLBart(cfg)
    TR.trainable_names(model, cfg)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    model.eval()
    ad = model.model.decoder.layers[0].ff_adapter.adapters["vqa"]
    assert ad.down_sample_size == 96 and ad.down_sampler.weight.dtype == torch.float32
    gen = torch.Generator(device=DEV).manual_seed(5)
    b = TR.synthetic_batch("vqa", 24, cfg, DEV, gen, no_padding=False)
    g = dict(ids=b["input_ids"], vis=b["vis_inputs"], task="vqa", max_length=6, min_length=6, ngram=0, eos=2)
    (out0, lg0), (out1, lg1), n_on, n_off = _on_off(model, "bart", lambda: run_generate(model, g, DEV))
    assert n_off == 0 and n_on >= 18 * 5                                              # 3 per decoder layer and step (the prefill's 24 x 56 rows compose or fuse by ADAPTER_TAIL_MAX_ROWS)
    err = float((lg1[:, 0] - lg0[:, 0]).abs().max())
    assert err <= 1e-2 * max(1.0, float(lg0[:, 0].abs().max())), err
    # a token may change where two logits lie within twice the tolerance of each other (each may move by it, in opposite directions)
    first = lg0[:, 0].clone()
    first[:, g["eos"]] = float("-inf")                                                 # (min_length bans eos: it is not among the candidates)
    top = first.topk(2, -1).values
    sure = (top[:, 0] - top[:, 1]) > 2 * 1e-2 * max(1.0, float(lg0[:, 0].abs().max()))
    assert torch.equal(out0[sure, 1], out1[sure, 1])                                  # first step: where the margin is clear, the same token
    graph = [model.generate(b["input_ids"], b["vis_inputs"], "vqa", max_length=6, min_length=6, graph=True) for _ in range(3)]
    eager = model.generate(b["input_ids"], b["vis_inputs"], "vqa", max_length=6, min_length=6)
    assert all(torch.equal(o, eager) for o in graph)
