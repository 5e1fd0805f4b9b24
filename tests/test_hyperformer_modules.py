"""Hyperformer's modules (vl-pet_amd/adapters/adapter_hypernetwork.py, adapter_utils.py, config.py) without a GPU, against the fixtures
made from the reference's controllers: parameter names in the reference's order, the batched ``generate()`` and the per-layer
``forward`` (outputs and every gradient), the fp64 specification of the generator on the fixtures' tensors, init rules, config
defaults, the shared task-embedding controller, the refused flags by name."""
import numpy as np
import pytest
import torch

import hyper_spec as S
import hyperformer_cases as C

TOL = 1e-5          # fp32 on both sides, |values| <= ~3: the reference's per-layer chain against the batched one (measured 2e-7)


@pytest.mark.parametrize("form", C.FORMS)
def test_parameter_names_and_order_are_the_references(form):
    ctl, _ = C.controller(form)
    want = [k[3:] for k in C.fixture(form) if k.startswith("p::")]          # saved in the reference's named_parameters() order
    assert [n for n, _ in ctl.named_parameters()] == want
    assert sorted(ctl.state_dict()) == sorted(want)
    assert "task_hypernet.task_embeding_generator.0.weight" in want and "LayerNorm.weight" in want
    if form == "unique":
        assert "cross_attention_down_sampler_hyper_net.weight_generator.0.weight" in want
    else:
        assert "adapters_block_type.weight" in want and "down_sampler_hyper_net.bias_generator.0.bias" in want


@pytest.mark.parametrize("form", C.FORMS)
def test_generate_and_per_layer_forward_match_the_reference(form):
    z = C.fixture(form)
    ctl, te = C.controller(form)
    weights = ctl.generate(te)
    assert len(weights) == int(z["layers"]) and set(weights[0]) == set(C.BLOCKS)
    assert weights[0]["self_attention"].down_w.shape == (8, 64) and weights[1]["cross_attention"].up_w.shape == (64, 8)
    assert weights[0]["feed_forward"].pack is None
    for key, t in C.each_output(weights):
        assert C.rel(t.detach(), z["out::" + key]) <= TOL, key
    for layer in range(int(z["layers"])):
        for key, t in C.each_output([ctl(te, layer)]):
            assert C.rel(t.detach(), z["out::" + key.replace("0::", f"{layer}::", 1)]) <= TOL, (layer, key)
    C.fixture_loss(form, weights).backward()
    for n, p in ctl.named_parameters():
        assert C.rel(p.grad, z["d::" + n]) <= TOL, n
    assert C.rel(te.grad, z["d_task_embedding"]) <= TOL


@pytest.mark.parametrize("form", C.FORMS)
def test_embedding_rows_are_the_references(form):
    z = C.fixture(form)
    ctl, te = C.controller(form)
    e = ctl.embedding_rows(te).detach()
    assert e.shape == (ctl.n_rows, 8)
    for layer in range(int(z["layers"])):
        for block in C.BLOCKS:
            row, _ = ctl.locate(layer, block)
            want = z[f"emb::{layer}"] if form == "unique" else z[f"emb::{layer}::{block}"]
            assert C.rel(e[row], want) <= TOL, (layer, block)


@pytest.mark.parametrize("form", C.FORMS)
def test_spec_reproduces_the_fixtures(form):
    """tests/hyper_spec.py on the fixture's own tensors: the generators' outputs from the recorded embeddings, and the generators'
    gradients from the recorded upstream gradients"""
    z = C.fixture(form)
    ctl, te = C.controller(form)
    maps = [(G.detach().numpy(), g.detach().numpy()) for G, g in ctl.maps()]
    E = ctl.n_rows
    e = np.zeros((E, 8))
    dout = [[None] * E for _ in maps]
    for layer in range(int(z["layers"])):
        for block in C.BLOCKS:
            row, base = ctl.locate(layer, block)
            e[row] = z[f"emb::{layer}"] if form == "unique" else z[f"emb::{layer}::{block}"]
            for k, (side, what, _) in enumerate(C.PARTS):
                dout[base + k][row] = z[f"dout::{layer}::{block}::{side}::{what}"].reshape(-1)
    outs = S.generate(maps, e)
    for layer in range(int(z["layers"])):
        for block in C.BLOCKS:
            row, base = ctl.locate(layer, block)
            for k, (side, what, _) in enumerate(C.PARTS):
                want = z[f"out::{layer}::{block}::{side}::{what}"].reshape(-1)
                out, mag = outs[base + k]
                assert (np.abs(out[row] - want) <= 2 * S.budget(mag[row], 9) + 1e-7 * np.abs(want)).all()      # (fp32 e, fp32 result)
    g = S.grads(maps, e, dout)
    names = [n for n, _ in ctl.named_parameters() if "_generator.0." in n and "task_hypernet" not in n]
    by_ptr = {p.data_ptr(): n for n, p in ctl.named_parameters()}
    for s, (G, b) in enumerate(ctl.maps()):
        assert C.rel(g["dG"][s], z["d::" + by_ptr[G.data_ptr()]]) <= TOL and C.rel(g["dg"][s], z["d::" + by_ptr[b.data_ptr()]]) <= TOL
    assert len(names) == 2 * len(maps)


def test_init_rules_and_config_defaults():
    from vlpet_amd.adapters import (AdapterLayersHyperNetController, MetaAdapterConfig, MetaLayersAdapterController,
                                    TaskEmbeddingController)
    cfg = MetaAdapterConfig()
    assert (cfg.task_embedding_dim, cfg.task_hidden_dim, cfg.projected_task_embedding_dim) == (512, 128, 64)
    assert cfg.unique_hyper_net and cfg.unique_hyper_net_layer_norm and not cfg.efficient_unique_hyper_net
    assert not cfg.train_task_embeddings and cfg.task_to_embeddings is None and cfg.non_linearity == "gelu_new"
    torch.manual_seed(0)
    cfg = C.config(task_embedding_dim=512, input_dim=768, d_model=768)
    ctl = AdapterLayersHyperNetController(cfg, 6, True)
    assert ctl.LayerNorm.eps == 1e-6 and ctl.down_sample_size == 96 and len(ctl.maps()) == 12 and ctl.n_rows == 6
    for n, p in ctl.named_parameters():
        if n.endswith("bias") and "LayerNorm" not in n:
            assert not bool(p.any()), n                                         # zero biases
        elif "_generator." in n and n.endswith("weight"):
            sd = float(p.detach().std())
            assert abs(sd - 1e-2) < (2e-3 if p.numel() < 5000 else 2e-4), (n, sd)       # N(0, 1e-2)
    assert abs(float(ctl.layer_id_embeddings.weight.detach().std()) - 1.0) < 0.1         # nn.Embedding's N(0, 1)
    tec = TaskEmbeddingController(cfg)
    assert list(tec.task_to_embeddings) == C.TASKS and tec("gqa").shape == (512,) and abs(float(tec("vqa").detach().std()) - 1.0) < 0.15
    assert [n for n, _ in tec.named_parameters()] == ["task_to_embeddings." + t for t in C.TASKS]
    assert not list(MetaLayersAdapterController(cfg).parameters())


def test_shared_task_embedding_controller_appears_three_times_in_the_state_dict_and_once_in_named_parameters():
    """the reference registers the one TaskEmbeddingController under the model and under both stacks"""
    from vlpet_amd.adapters import TaskEmbeddingController
    tec = TaskEmbeddingController(C.config())
    model, enc, dec = torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
    model.shared_task_embed, enc.task_embed, dec.task_embed = tec, tec, tec
    model.encoder, model.decoder = enc, dec
    keys = [k for k in model.state_dict() if k.endswith("task_to_embeddings.vqa")]
    assert sorted(keys) == ["decoder.task_embed.task_to_embeddings.vqa", "encoder.task_embed.task_to_embeddings.vqa",
                            "shared_task_embed.task_to_embeddings.vqa"]
    assert [n for n, _ in model.named_parameters()] == ["shared_task_embed.task_to_embeddings." + t for t in C.TASKS]


def test_refused_flags_are_named():
    from vlpet_amd.adapters import (AdapterLayersHyperNetController, AdapterLayersOneHyperNetController, MetaLayersAdapterController,
                                    TaskEmbeddingController)
    for flag in ("add_layer_norm_before_adapter", "add_layer_norm_after_adapter"):
        for make in (lambda c: AdapterLayersHyperNetController(c, 2), lambda c: AdapterLayersOneHyperNetController(c, 2, True),
                     MetaLayersAdapterController):
            with pytest.raises(ValueError, match=flag + ".*use_hyperformer"):
                make(C.config(**{flag: True}))
    with pytest.raises(ValueError, match="train_task_embeddings"):
        TaskEmbeddingController(C.config(train_task_embeddings=True))
    with pytest.raises(ValueError, match="train_task_embeddings"):
        AdapterLayersHyperNetController(C.config(train_task_embeddings=True), 2)
    with pytest.raises(ValueError, match="task_to_embeddings"):
        TaskEmbeddingController(C.config(task_to_embeddings={"vqa": "gqa"}))


@pytest.mark.parametrize("form", C.FORMS)
def test_meta_adapter_applies_handed_in_weights_like_the_reference(form):
    """adapter_controller.py:231-250: up(gelu_new(down(x))) + x; ``fused`` adds a residual of its own; track_z keeps the bottleneck"""
    from vlpet_amd.adapters import MetaLayersAdapterController
    from vlpet_amd.activations import get_activation
    ctl, te = C.controller(form)
    w = ctl.generate(te)[1]["cross_attention"]
    x, res = torch.randn(5, 64), torch.randn(5, 64)
    z = get_activation("gelu_new")(torch.nn.functional.linear(x, w.down_w, w.down_b))
    want = torch.nn.functional.linear(z, w.up_w, w.up_b)
    meta = MetaLayersAdapterController(C.config())
    assert torch.allclose(meta(x, w), want + x, atol=1e-6) and torch.allclose(meta.fused(x, res, w, 0.5), res + 0.5 * want, atol=1e-6)
    tracked = MetaLayersAdapterController(C.config(track_z=True))
    assert torch.allclose(tracked(x, w), want + x, atol=1e-6) and torch.allclose(tracked.z, z, atol=1e-6)
    relu = MetaLayersAdapterController(C.config(non_linearity="relu"))
    want = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, w.down_w, w.down_b)), w.up_w, w.up_b)
    assert relu.eager and torch.allclose(relu(x, w), want + x, atol=1e-6)
