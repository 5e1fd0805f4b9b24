"""The prompt-tuning baseline (scripts/image-text/single_prompt.sh) on the host models, without a GPU: ``encoder_prompt_len`` learned
rows, re-parametrised through a two-layer MLP, in front of the text rows of the joint encoder; the visual embedding and the prompts
train.  The fixtures are the reference's own VLBart (one shared prompt) / VLT5 (one per task) under that flag set
(tests/golden/make_prompt_goldens.py); harness and tolerances are test_single_adapter_host.py's (HIP-backed ops swapped for the eager
restatement, 2e-5)."""
import numpy as np
import pytest
import torch

import prompt_cases as C
import prompt_spec as PS

KINDS = ["bart", "t5"]


def test_the_config_fields_exist_and_build_the_prompt_config():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    from vlpet_amd.prompt import EncoderPromptConfig
    for make, d in ((HB.vlpet_config, 768), (HT.vlt5_config, 768)):
        cfg = make(encoder_prompt_len=5, mid_dim=24, use_single_prompt=True)
        pc = cfg.encoder_prompt_config
        assert isinstance(pc, EncoderPromptConfig)
        assert (pc.prompt_len, pc.mid_dim, pc.input_dim, pc.use_single_prompt, pc.use_input_prompt) == (5, 24, d, True, True)
        assert pc.tasks == ["vqa", "gqa", "nlvr", "caption"]
        off = make()
        assert off.encoder_prompt_config is None
        assert (off.encoder_prompt_len, off.decoder_prompt_len, off.mid_dim, off.use_single_prompt) == (0, 0, 768, False)
    assert C.config("bart").encoder_prompt_config.input_dim == 64           # the model's width, not the reference's fixed 768


@pytest.mark.parametrize("kind", KINDS)
def test_decoder_prompts_are_refused_by_name(kind):
    with pytest.raises(NotImplementedError, match="decoder_prompt_len"):
        C.config(kind, decoder_prompt_len=1)
    with pytest.raises(NotImplementedError, match="decoder_prompt_len"):
        C.config(kind, prompt=False, decoder_prompt_len=3)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_shapes_are_the_references_and_loading_is_strict(kind):
    sd = C.fixture(kind)[0]
    model = C.new_model(kind, C.config(kind))
    host = model.state_dict()
    head = {"lm_head.weight"}                                # tied head: the host reuses the shared embedding
    assert set(host) == set(sd) - head
    assert all(tuple(host[k].shape) == tuple(sd[k].shape) for k in host)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and set(unexpected) <= head
    pre = ("model." if kind == "bart" else "") + "encoder.prompt_modules.prompts."
    want = {f"{pre}{t}.prefix_embedding.{i}.{w}" for t in C.TASKS for i, w in ((0, "weight"), (1, "weight"), (1, "bias"), (3, "weight"),
                                                                               (3, "bias"))}
    assert {k for k in host if "prompt" in k} == want
    d = 64
    assert tuple(host[f"{pre}vqa.prefix_embedding.0.weight"].shape) == (C.P, d)
    assert tuple(host[f"{pre}vqa.prefix_embedding.1.weight"].shape) == (C.MID, d)
    assert tuple(host[f"{pre}vqa.prefix_embedding.3.weight"].shape) == (d, C.MID)


@pytest.mark.parametrize("kind", KINDS)
def test_single_prompt_is_one_module_under_every_task_and_per_task_prompts_are_four(kind):
    from vlpet_amd.prompt import InputPrompts, PromptController
    for single in (True, False):
        model = C.new_model(kind, C.config(kind, use_single_prompt=single))
        ctl = C.encoder(model, kind).prompt_modules
        assert isinstance(ctl, PromptController) and list(ctl.prompts) == list(C.TASKS)
        assert all(isinstance(ctl.prompts[t], InputPrompts) for t in C.TASKS)
        named = [n for n, _ in model.named_parameters() if "prompt" in n]
        listed = [k for k in model.state_dict() if "prompt" in k]
        assert len(listed) == 5 * len(C.TASKS)                                  # the state dict lists the module per task either way
        if single:
            assert all(ctl.prompts[t] is ctl.prompts["vqa"] for t in C.TASKS)
            assert len(named) == 5 and all(".prompts.vqa." in n for n in named)     # named_parameters lists it once
        else:
            assert len({id(ctl.prompts[t]) for t in C.TASKS}) == len(C.TASKS) and len(named) == 5 * len(C.TASKS)
    assert ctl.get_prompt("gqa") is ctl.prompts["gqa"] and ctl.get_task("gqa") == "gqa" and ctl.convert_to_list("a") == ["a"]
    m = ctl.prompts["vqa"]
    assert (m.prompt_len, m.input_dim, m.mid_dim) == (C.P, 64, C.MID) and m.prefix_tokens.tolist() == list(range(C.P))


@pytest.mark.parametrize("kind", KINDS)
def test_trainable_set_logits_and_training_losses_match_the_reference(kind):
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, unexpected = C.build(kind)
    assert set(unexpected) <= {"lm_head.weight"}, unexpected
    assert sorted(names) == sorted(final.keys())           # the reference's trainable set, name for name (also inside _check)
    assert all("visual_embedding" in n or "prompt_modules" in n for n in names)
    assert sum("prompt_modules" in n for n in names) == (5 if kind == "bart" else 20)
    with cpu_reference_ops():
        _check(model, cfg, names, batches, ref_losses, hp, final, "cpu", 2e-5)


def test_generate_matches_the_reference_greedy_and_beam_cpu():
    from oracle.host_patch import cpu_reference_ops
    from test_beam import check_against_fixture as check_beam, run_beam
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen()
    model = C.build("bart")[0]
    with cpu_reference_ops():
        out, logits = run_generate(model, g, "cpu")
    check_against_fixture(out, logits, g, 1e-3)
    b = C.load_beam()
    C.sharpen(model, b["logit_scale"])
    with cpu_reference_ops():
        out, scores = run_beam(model, b, "cpu")
    check_beam(out, scores, b)


@pytest.mark.parametrize("kind", KINDS)
def test_controller_forward_is_an_expanded_view_of_the_prompt_rows(kind):
    model = C.build(kind)[0]
    ctl = C.encoder(model, kind).prompt_modules
    for task in ("vqa", "caption"):
        rows = ctl.prompt_rows(task)
        assert tuple(rows.shape) == (C.P, 64)
        m = ctl.prompts[task]
        emb, down, act, up = m.prefix_embedding
        ids = m.prefix_tokens.unsqueeze(0).expand(3, -1)                     # what the reference runs: the MLP on B * P looked-up rows
        torch.testing.assert_close(rows.expand(3, -1, -1), up(act(down(emb(ids)))), rtol=1e-6, atol=1e-6)
        out = ctl(7, "cpu", task)
        assert tuple(out.shape) == (7, C.P, 64) and out.stride(0) == 0       # a view: no B * P rows exist
        assert torch.equal(out, rows.expand(7, -1, -1))
    if kind == "t5":
        assert not torch.equal(ctl.prompt_rows("vqa"), ctl.prompt_rows("caption"))       # one prompt per task
    else:
        assert torch.equal(ctl.prompt_rows("vqa"), ctl.prompt_rows("caption"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_fallback_equals_the_spec_without_dropout(dtype):
    from vlpet_amd.act import prefix_concat_dropout
    gen = torch.Generator().manual_seed(4)
    pre, a, v = (torch.randn(*s, generator=gen).to(dtype) for s in ((5, 16), (3, 7, 16), (3, 2, 16)))
    for training in (False, True):
        x = prefix_concat_dropout(pre, a, v, 0.0, training=training, seed=9)
        ref, keep = PS.forward(pre.float().numpy(), a.float().numpy(), v.float().numpy(), 9, 0.0)
        assert keep.all() and x.dtype == dtype and tuple(x.shape) == (3, 14, 16)
        assert np.array_equal(x.float().numpy().astype(np.float64), ref)
    # ... and its gradients are the spec's backward: the slices, and the batch sum for the prompt
    pre, a, v = (t.float().requires_grad_() for t in (pre, a, v))
    dx = torch.randn(3, 14, 16, generator=gen)
    prefix_concat_dropout(pre, a, v, 0.0, training=True).backward(dx)
    dpre, da, dv, _ = PS.backward(dx.numpy(), 5, 7, 2, 0, 0.0)
    np.testing.assert_allclose(pre.grad.numpy(), dpre, rtol=1e-6, atol=1e-6)
    assert np.array_equal(a.grad.numpy(), da) and np.array_equal(v.grad.numpy(), dv)


@pytest.mark.parametrize("kind", KINDS)
def test_without_the_flag_nothing_changes(kind):
    """No ``prompt_modules`` attribute or key, the trainable set of before, and an output identical to a config that never heard of
    the fields."""
    import vlpet_amd.host.common as HC
    import vlpet_amd.train as TR
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _to
    cfg = C.config(kind, prompt=False)
    torch.manual_seed(0)
    model = C.new_model(kind, cfg)
    assert cfg.encoder_prompt_config is None and not [k for k in model.state_dict() if "prompt" in k]
    assert not hasattr(C.encoder(model, kind), "prompt_modules")
    assert TR.trainable_names(model, cfg) == [n for n, _ in model.named_parameters() if "visual_embedding" in n]
    bare = C.config(kind, prompt=False)
    for f in list(HC.PROMPT_DEFAULTS) + ["encoder_prompt_config"]:
        delattr(bare, f)
    torch.manual_seed(0)
    old = C.new_model(kind, bare)
    assert list(old.state_dict()) == list(model.state_dict())
    b = _to(C.fixture(kind)[1][0], "cpu")
    with cpu_reference_ops(), torch.no_grad():
        per0, lg0 = old.eval()(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
        per1, lg1 = model.eval()(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    assert torch.equal(lg0, lg1) and torch.equal(per0, per1)
    assert TR.trainable_names(old, bare) == TR.trainable_names(model, cfg)
