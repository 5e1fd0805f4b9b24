"""The Hyperformer baseline (scripts/image-text/hyperformer.sh) on the host models, without a GPU: generated adapters behind every
attention and feed-forward block of both stacks and behind the decoder's cross-attention.  The fixtures are the reference's own VLBart
under ``--unique_hyper_net`` and under ``--efficient_unique_hyper_net`` and its VLT5 under ``--unique_hyper_net`` (tests/golden/make_hyperformer_goldens.py); harness and
tolerances are test_single_adapter_host.py's CPU leg: the HIP-backed ops swapped for the eager restatement, the hyper-networks on the
package's own plain-torch composition (vl-pet_amd/eager.py)."""
import pytest
import torch

import hyperformer_host_cases as C


def _per_token(out):
    """the per-token loss of a forward (the CPU harness's lm_loss also returns the logits)"""
    return out[0] if isinstance(out, tuple) else out


@pytest.mark.parametrize("which", C.WHICH)
def test_state_dict_trainable_set_logits_and_training_losses_match_the_reference(which):
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(which)
    model, cfg, names, unexpected = C.build(which)
    assert not unexpected, unexpected
    assert set(model.state_dict()) == set(sd)                    # key for key, the three registrations of the task embeddings included
    assert names == C.trainable_names(which)                     # the reference's trainable set, in named_parameters order
    with cpu_reference_ops():
        _check(model, cfg, names, batches, ref_losses, hp, final, "cpu", 2e-5)


@pytest.mark.parametrize("which", C.WHICH)
def test_task_embeddings_are_registered_three_times_and_listed_once(which):
    from vlpet_amd.adapters import AdapterLayersHyperNetController, AdapterLayersOneHyperNetController, MetaLayersAdapterController
    model, cfg = C.new_model(which)
    m, enc_stack, dec_stack = C.stacks(model)
    pre = "model." if C.KIND[which] == "bart" else ""
    assert m.shared_task_embed is enc_stack.task_embed is dec_stack.task_embed
    keys = sorted(k for k in model.state_dict() if k.endswith("task_to_embeddings.gqa"))
    assert keys == [pre + "decoder.task_embed.task_to_embeddings.gqa", pre + "encoder.task_embed.task_to_embeddings.gqa",
                    pre + "shared_task_embed.task_to_embeddings.gqa"]
    assert [n for n, _ in model.named_parameters() if "task_to_embeddings" in n] == [
        pre + "shared_task_embed.task_to_embeddings." + t for t in ("vqa", "gqa", "nlvr", "caption")]
    cls = AdapterLayersOneHyperNetController if which == "one" else AdapterLayersHyperNetController
    enc, dec = enc_stack.adapter_layers_hyper_net, dec_stack.adapter_layers_hyper_net
    assert type(enc) is cls and type(dec) is cls and not enc.include_cross_attention and dec.include_cross_attention
    assert enc.projected_dim == 8 and enc.down_sample_size == 8 and enc.task_embedding_dim == C.TASK_DIM
    metas = [mod for mod in model.modules() if isinstance(mod, MetaLayersAdapterController)]
    # BART: one per layer (2 + 2); T5: one per sublayer module (2 x 2 encoder, 2 x 3 decoder), as the reference places them
    assert len(metas) == (4 if C.KIND[which] == "bart" else 10)
    assert not any("adapter_hypernet" in k for k in model.state_dict())          # it has no parameters
    # the class defaults when the flag does not set the projected dimension
    ac = C.config(which, projected_task_embedding_dim=-1).adapter_config
    assert ac.projected_task_embedding_dim == 64 and ac.task_hidden_dim == 128 and ac.unique_hyper_net_layer_norm
    import vlpet_amd.host.bart as HB
    assert HB.vlpet_config(**C.FLAGS["unique"]).adapter_config.task_embedding_dim == 512


def test_cross_attention_adapter_follows_add_adapter_cross_attn():
    """the decoder's controller always generates the cross-attention set; the layer applies it only with the flag"""
    from oracle.host_patch import cpu_reference_ops
    sd, batches, *_ = C.fixture("unique")
    on = C.build("unique")[0].eval()
    off = C.build("unique", add_adapter_cross_attn=False)[0].eval()
    b = batches[0]
    with cpu_reference_ops(), torch.no_grad():
        a = _per_token(on(b["input_ids"], b["vis_inputs"], b["labels"], b["task"]))
        c = _per_token(off(b["input_ids"], b["vis_inputs"], b["labels"], b["task"]))
    assert float((a - c).abs().max()) > 1e-3


def test_another_task_and_zeroed_generators_move_the_loss():
    """the fixture can tell a dead hyper-network from a working one"""
    from oracle.host_patch import cpu_reference_ops
    sd, batches, *_ = C.fixture("unique")
    model = C.build("unique")[0].eval()
    b = batches[0]
    with cpu_reference_ops(), torch.no_grad():
        base = _per_token(model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"]))
        other = _per_token(model(b["input_ids"], b["vis_inputs"], b["labels"], "caption"))
        for n, p in model.named_parameters():
            if "sampler_hyper_net" in n:
                p.zero_()
        dead = _per_token(model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"]))
    assert float((base - other).abs().max()) > 1e-2 and float((base - dead).abs().max()) > 1e-2


def test_mixed_adapter_kinds_and_clashing_flags_are_refused():
    with pytest.raises(ValueError, match="use_hyperformer and use_adapter"):
        C.config("t5", use_adapter=True)
    with pytest.raises(ValueError, match="unique_hyper_net or efficient_unique_hyper_net"):
        C.config("t5", unique_hyper_net=False)
    with pytest.raises(ValueError, match="use_hyperformer.*use_encoder_adapter_down_multihead"):
        C.config("t5", use_encoder_adapter_down_multihead=True)
    with pytest.raises(ValueError, match="use_hyperformer and use_adapter"):
        C.config("unique", use_adapter=True)
    with pytest.raises(ValueError, match="use_hyperformer and use_compacter"):
        C.config("unique", use_compacter=True)
    with pytest.raises(ValueError, match="unique_hyper_net or efficient_unique_hyper_net"):
        C.config("unique", unique_hyper_net=False)
    for flag in ("use_encoder_adapter_down_multihead", "use_decoder_enc_attn_value_parallel_adapter_down_dim",
                 "use_encoder_adapter_gating_large_x_lowrank", "use_lora"):
        with pytest.raises(ValueError, match="use_hyperformer.*" + flag):
            C.config("unique", **{flag: True})
    import vlpet_amd.host.bart as HB
    with pytest.raises(AttributeError):
        HB.vlpet_config(use_hyper_former=True)


def test_existing_flag_sets_build_the_same_module_tree():
    import vlpet_amd.host.bart as HB
    import single_adapter_cases as SA
    cfg = HB.vlpet_config()
    assert (cfg.use_hyperformer, cfg.unique_hyper_net, cfg.efficient_unique_hyper_net, cfg.projected_task_embedding_dim) == (False, False, False, -1)
    assert type(cfg.adapter_config).__name__ == "AdapterConfig"
    for model in (SA.build("bart")[0], HB.VLBart(HB.vlpet_config(**SA.BART_GEOMETRY))):
        names = [n for n, _ in model.named_modules()]
        assert not any("task_embed" in n or "hyper_net" in n or "adapter_hypernet" in n for n in names)
        assert not hasattr(model.model, "shared_task_embed") and not hasattr(model.model.encoder, "adapter_layers_hyper_net")
        assert all(l.adapter_hypernet is None for l in list(model.model.encoder.layers) + list(model.model.decoder.layers))
    import vlpet_amd.host.t5 as HT
    t5 = SA.build("t5")[0]
    assert HT.vlt5_config().use_hyperformer is False and not hasattr(t5, "shared_task_embed")
    assert not any("task_embed" in n or "hyper_net" in n or "adapter_hypernet" in n for n, _ in t5.named_modules())


@pytest.mark.parametrize("kind,which", [("bart", "unique"), ("t5", "t5")])
def test_generate_matches_the_reference_greedy_cpu(kind, which):
    from oracle.host_patch import cpu_reference_ops
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen(kind)
    model = C.build(which)[0]
    with cpu_reference_ops():
        out, logits = run_generate(model, g, "cpu")
    check_against_fixture(out, logits, g, 1e-3)


def test_beam_search_matches_the_reference_cpu():
    from oracle.host_patch import cpu_reference_ops
    from test_beam import check_against_fixture as check_beam, run_beam
    b = C.load_beam()
    model = C.build("t5")[0]
    C.sharpen_t5(model, b["logit_scale"])
    with cpu_reference_ops():
        out, scores = run_beam(model, b, "cpu")
    check_beam(out, scores, b)
