"""The Single-Adapter baseline (scripts/image-text/single_adapter.sh) on the host models, without a GPU: sequential adapters behind every
attention and feed-forward block of both stacks, every LayerNorm trainable.  The fixtures are the reference's own VLBart / VLT5 under that
flag set (tests/golden/make_single_adapter_goldens.py); harness and tolerances are test_host_golden.py's CPU leg (HIP-backed ops swapped for
the eager restatement)."""
import pytest
import torch

import single_adapter_cases as C


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_state_dict_trainable_set_logits_and_training_losses_match_the_reference(kind):
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, unexpected = C.build(kind)
    assert not unexpected, unexpected                      # (the fixture leaves the aliases of the shared embedding out)
    assert sorted(names) == sorted(final.keys())           # the reference's trainable set, name for name (also inside _check)
    assert any("decoder" in n and "layer_norm" in n for n in names) and any("visual_embedding" in n for n in names)
    with cpu_reference_ops():
        _check(model, cfg, names, batches, ref_losses, hp, final, "cpu", 2e-5)


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_adapter_keys_are_the_references(kind):
    sd = C.fixture(kind)[0]
    model = C.build(kind)[0]
    host = {k for k in model.state_dict() if "adapter" in k}
    assert host == {k for k in sd if "adapter" in k} and host
    tasks = ("vqa", "gqa", "nlvr", "caption")
    leaf = {f"adapters.{t}.{m}_sampler.{p}" for t in tasks for m in ("down", "up") for p in ("weight", "bias")}
    if kind == "bart":
        want = {f"model.encoder.layers.{l}.{a}.{x}" for l in range(2) for a in ("attn_adapter", "ff_adapter") for x in leaf}
        want |= {f"model.decoder.layers.{l}.{a}.{x}" for l in range(2) for a in ("self_attn_adapter", "enc_attn_adapter", "ff_adapter")
                 for x in leaf}
        ctl = model.model.decoder.layers[0].self_attn_adapter
    else:
        want = {f"encoder.block.{l}.layer.{i}.{a}.{x}" for l in range(2) for i, a in ((0, "attn_adapter"), (1, "ff_adapter")) for x in leaf}
        want |= {f"decoder.block.{l}.layer.{i}.{a}.{x}" for l in range(2)
                 for i, a in ((0, "attn_adapter"), (1, "enc_attn_adapter"), (2, "ff_adapter")) for x in leaf}
        ctl = model.decoder.block[0].layer[0].attn_adapter
    assert host == want
    assert all(ctl.adapters[t] is ctl.adapters["vqa"] for t in tasks)          # use_single_adapter: one object under every task key
    assert ctl.adapters["vqa"].down_sample_size == 8                           # d_model // reduction_factor


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_refused_flag_combinations_name_the_flags(kind):
    with pytest.raises(ValueError, match="no_encoder_adapter.*use_encoder_adapter_down_multihead"):
        C.config(kind, use_encoder_adapter_down_multihead=True)
    with pytest.raises(ValueError, match="no_encoder_adapter.*use_encoder_adapter_gating_large_x_lowrank"):
        C.config(kind, use_encoder_adapter_gating_large_x_lowrank=True)
    with pytest.raises(ValueError, match="no_encoder_adapter.*use_encoder_adapter_gating_middle_xy_add"):
        C.config(kind, use_encoder_adapter_gating_middle_xy_add=True)
    with pytest.raises(ValueError, match="no_decoder_adapter.*use_decoder_enc_attn_value_parallel_adapter_down_dim"):
        C.config(kind, use_decoder_enc_attn_value_parallel_adapter_down_dim=True)
    # each refused only together with the sequential adapters of ITS side
    C.config(kind, no_encoder_adapter=True, use_encoder_adapter_down_multihead=True, use_encoder_adapter_gating_large_x_lowrank=True)
    C.config(kind, no_decoder_adapter=True, use_decoder_enc_attn_value_parallel_adapter_down_dim=True)


def _model(kind, **over):
    cfg = C.config(kind, **over)
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.VLT5(cfg), cfg
    import vlpet_amd.host.bart as HB
    return HB.VLBart(cfg), cfg


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_each_side_alone_and_the_cross_attention_switch(kind):
    import vlpet_amd.train as TR
    both = {k for k in _model(kind)[0].state_dict() if "adapter" in k}
    enc_only = {k for k in _model(kind, no_decoder_adapter=True)[0].state_dict() if "adapter" in k}
    dec_only = {k for k in _model(kind, no_encoder_adapter=True)[0].state_dict() if "adapter" in k}
    assert enc_only == {k for k in both if "encoder." in k} and enc_only
    assert dec_only == {k for k in both if "decoder." in k} and dec_only
    no_cross = {k for k in _model(kind, add_adapter_cross_attn=False)[0].state_dict() if "adapter" in k}
    assert both - no_cross == {k for k in both if "enc_attn_adapter" in k} and both - no_cross and no_cross < both
    # the defaults (both no_* flags set) build no sequential adapter: today's models, key for key
    model, cfg = _model(kind, no_encoder_adapter=True, no_decoder_adapter=True, unfreeze_layer_norms=False)
    assert not [k for k in model.state_dict() if "adapter" in k]
    assert TR.trainable_names(model, cfg) == [n for n, _ in model.named_parameters() if "visual_embedding" in n]


def test_unfreeze_layer_norms_reaches_every_norm_and_leaves_decay_rules_alone():
    import vlpet_amd.train as TR
    import vlpet_amd.host.bart as HB
    assert TR.NO_DECAY == ("bias", "LayerNorm.weight")
    for kind in ("bart", "t5"):
        model, cfg = _model(kind)
        names = set(TR.trainable_names(model, cfg))
        norms = {f"{mn}.{pn}" for mn, m in model.named_modules()
                 if isinstance(m, torch.nn.LayerNorm) or type(m).__name__ == "T5LayerNorm" for pn, _ in m.named_parameters(recurse=False)}
        assert norms and norms <= names
        assert any(n.startswith(("model.decoder.", "decoder.")) for n in norms) and any("visual_embedding" in n for n in norms)
        off = set(TR.trainable_names(model, C.config(kind, unfreeze_layer_norms=False)))
        assert off == {n for n in names if "adapter" in n or "visual_embedding" in n}
    cfg = HB.vlpet_config()                                 # VL-PET's own default set is what it was
    assert cfg.add_adapter_cross_attn is True and cfg.unfreeze_layer_norms is False and cfg.no_encoder_adapter and cfg.no_decoder_adapter


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
