"""The Compacter baseline (scripts/image-text/single_compacter.sh) on the host models, without a GPU: PHM adapters behind every attention
and feed-forward block of both stacks.  The fixtures are the reference's own VLBart / VLT5 under that flag set, and a VLBart under
param.py's defaults (one rule shared by the model, factorized W) (tests/golden/make_compacter_goldens.py); harness and tolerances are
test_single_adapter_host.py's CPU leg: the HIP-backed ops swapped for the eager restatement, the PHM adapters on the package's own
plain-torch composition (vl-pet_amd/eager.py)."""
import pytest
import torch

import compacter_cases as C

WHICH = ["bart", "t5", "shared_fac"]


@pytest.mark.parametrize("which", WHICH)
def test_state_dict_trainable_set_logits_and_training_losses_match_the_reference(which):
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(which)
    model, cfg, names, unexpected = C.build(which)
    assert not unexpected, unexpected
    assert set(model.state_dict()) == set(sd)                    # key for key, the aliases of a shared rule included
    assert names == C.trainable_names(which)                     # the reference's trainable set, in named_parameters order
    with cpu_reference_ops():
        _check(model, cfg, names, batches, ref_losses, hp, final, "cpu", 2e-5)


@pytest.mark.parametrize("which", WHICH)
def test_controller_builds_phm_adapters_with_the_references_keys(which):
    from vlpet_amd.adapters import HyperComplexAdapter
    sd = C.fixture(which)[0]
    model, cfg = C.new_model(which)
    host = {k for k in model.state_dict() if "adapter" in k}
    assert host == {k for k in sd if "adapter" in k} and host
    ctl = model.model.decoder.layers[0].self_attn_adapter if C.KIND[which] == "bart" else model.decoder.block[0].layer[0].attn_adapter
    tasks = ("vqa", "gqa", "nlvr", "caption")
    ad = ctl.adapters["vqa"]
    assert ctl.hypercomplex_adapters and isinstance(ad, HyperComplexAdapter) and all(ctl.adapters[t] is ad for t in tasks)
    assert ad.down_sample_size == 8 and not ad.eager
    leaves = {k.rsplit(".", 1)[1] for k in host}
    if which == "shared_fac":
        assert leaves == {"phm_rule", "W_left", "W_right", "b"} and ad.phm_dim == 4
        assert tuple(ad.down_sampler.W_left.shape) == (4, 16, 1) and tuple(ad.down_sampler.W_right.shape) == (4, 1, 2)
        assert tuple(model.phm_rule.shape) == (4, 4, 4) and "phm_rule" in sd
        assert all(m.phm_rule is model.phm_rule for _, m in C.phm_layers(model))
        assert [n for n, _ in model.named_parameters() if "phm_rule" in n] == ["phm_rule"]
    else:
        assert leaves == {"phm_rule", "W", "b"} and ad.phm_dim == 2 and not hasattr(model, "phm_rule")
        assert tuple(ad.down_sampler.W.shape) == (2, 32, 4) and tuple(ad.up_sampler.W.shape) == (2, 4, 32)
        assert tuple(ad.down_sampler.phm_rule.shape) == (2, 2, 2) and tuple(ad.down_sampler.b.shape) == (8,)
        assert ad.down_sampler.phm_rule is not ad.up_sampler.phm_rule


def _ac(**over):
    from vlpet_amd.adapters import AdapterConfig
    return AdapterConfig(**{**dict(tasks=["vqa", "gqa"], input_dim=64, d_model=64, reduction_factor=8, hypercomplex_adapters=True,
                                   hypercomplex_division=2, factorized_phm=False), **over})


def test_adapter_config_defaults_are_the_compactor_configs():
    from vlpet_amd.adapters import AdapterConfig
    c = AdapterConfig()
    assert (c.hypercomplex_division, c.learn_phm, c.hypercomplex_nonlinearity, c.factorized_phm, c.phm_c_init, c.phm_rank,
            c.phm_init_range) == (4, True, "glorot-uniform", True, "normal", 1, 0.0001)
    assert not c.hypercomplex_adapters


def test_init_rules_and_down_sample_size():
    from vlpet_amd.adapters import AdapterController, PHMLinear
    torch.manual_seed(0)
    lay = PHMLinear(64, 8, 2, w_init="glorot-uniform", c_init="normal", phm_init_range=0.01)
    bound = 2 ** 0.5 * (6.0 / (32 + 4)) ** 0.5                           # xavier_uniform_ with gain sqrt(2) on each [32, 4] slice
    assert float(lay.W.detach().abs().max()) <= bound and float(lay.W.detach().abs().max()) > 0.5 * bound
    assert float(lay.b.detach().abs().max()) == 0 and 0 < float(lay.phm_rule.detach().std()) < 0.05
    lay = PHMLinear(64, 8, 2, w_init="normal", c_init="uniform", phm_init_range=0.01)
    assert float(lay.phm_rule.detach().abs().max()) <= 0.01 and 0 < float(lay.W.detach().std()) < 0.02
    lay = PHMLinear(64, 8, 2, w_init="glorot-normal", factorized_phm=True, phm_rank=3)
    assert tuple(lay.W_left.shape) == (2, 32, 3) and tuple(lay.W_right.shape) == (2, 3, 4) and tuple(lay.slices().shape) == (2, 32, 4)
    new = torch.nn.Parameter(torch.ones(2, 2, 2))
    lay.set_phm_rule(new)
    assert lay.phm_rule is new and dict(lay.named_parameters())["phm_rule"] is new
    for bad in (dict(w_init="phm"), dict(c_init="random")):
        with pytest.raises(ValueError):
            PHMLinear(64, 8, 2, **bad)
    with pytest.raises(ValueError):
        PHMLinear(64, 9, 2)
    assert AdapterController(_ac()).adapters["vqa"].down_sample_size == 8
    assert AdapterController(_ac(use_adapter_down_dim=True, adapter_down_dim=16)).adapters["vqa"].down_sample_size == 16


def test_learn_phm_off_freezes_the_rules():
    from vlpet_amd.adapters import AdapterController
    import vlpet_amd.train as TR
    ctl = AdapterController(_ac(learn_phm=False))
    ctl.disable_adapters(["vqa", "gqa"])
    ctl.enable_adapters(["vqa", "gqa"])
    on = {n for n, p in ctl.named_parameters() if p.requires_grad}
    assert on and not any("phm_rule" in n for n in on)
    assert {n.rsplit(".", 1)[1] for n in on} == {"W", "b"}
    ctl = AdapterController(_ac())
    ctl.disable_adapters(["vqa", "gqa"])
    ctl.enable_adapters(["vqa"])
    assert ctl.adapters["vqa"].down_sampler.phm_rule.requires_grad and not ctl.adapters["gqa"].down_sampler.W.requires_grad
    # the trainer's name rules keep them frozen too, the model's shared rule included
    for which in ("bart", "shared_fac"):
        model, cfg = C.new_model(which)
        cfg.adapter_config.learn_phm = False
        names = TR.trainable_names(model, cfg)
        assert names and not any("phm_rule" in n for n in names)
        assert any(n.endswith(".b") for n in names)


def test_shared_phm_rule_over_tasks_aliases_the_rules():
    from vlpet_amd.adapters import AdapterController
    ctl = AdapterController(_ac(shared_phm_rule_over_tasks=True))
    a, b = ctl.adapters["vqa"], ctl.adapters["gqa"]
    assert a is not b and a.down_sampler.W is not b.down_sampler.W
    assert a.down_sampler.phm_rule is b.down_sampler.phm_rule and a.up_sampler.phm_rule is b.up_sampler.phm_rule
    assert a.down_sampler.phm_rule is not a.up_sampler.phm_rule
    assert len([n for n, _ in ctl.named_parameters() if "phm_rule" in n]) == 2
    ctl = AdapterController(_ac())
    assert ctl.adapters["vqa"].down_sampler.phm_rule is not ctl.adapters["gqa"].down_sampler.phm_rule


@pytest.mark.parametrize("field", ["shared_W_phm", "factorized_phm_rule", "kronecker_prod"])
def test_unreachable_phm_forms_are_refused_by_name(field):
    from vlpet_amd.adapters import AdapterController, PHMLinear
    with pytest.raises(ValueError, match=field):
        AdapterController(_ac(**{field: True}))
    with pytest.raises(ValueError, match=field):
        PHMLinear(64, 8, 2, **{field: True})


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_mixed_adapter_kinds_and_clashing_flags_are_refused(kind):
    with pytest.raises(ValueError, match="use_adapter.*use_compacter"):
        C.config(kind, use_adapter=True)
    with pytest.raises(ValueError, match="use_compacter.*no_encoder_adapter.*use_encoder_adapter_down_multihead"):
        C.config(kind, use_encoder_adapter_down_multihead=True)
    with pytest.raises(ValueError, match="use_compacter.*no_decoder_adapter.*use_decoder_enc_attn_value_parallel_adapter_down_dim"):
        C.config(kind, use_decoder_enc_attn_value_parallel_adapter_down_dim=True)
    # each side alone builds only that side's adapters
    model, _ = C.new_model(kind, no_decoder_adapter=True)
    keys = [k for k in model.state_dict() if "adapter" in k]
    assert keys and all("encoder." in k for k in keys)


def test_eager_fallback_serves_other_nonlinearities_track_z_and_large_divisions():
    from vlpet_amd.adapters import AdapterController
    import phm_spec as S
    x = torch.randn(3, 64)
    for over in (dict(non_linearity="relu"), dict(track_z=True), dict(hypercomplex_division=16, input_dim=64, reduction_factor=4)):
        ctl = AdapterController(_ac(tasks=["vqa"], **over))
        ad = ctl.adapters["vqa"]
        assert ad.eager
        with torch.no_grad():
            ad.down_sampler.b.normal_(); ad.up_sampler.b.normal_(); ad.down_sampler.phm_rule.normal_(); ad.up_sampler.phm_rule.normal_()
        out = ctl(x, "vqa")
        d, u = ad.down_sampler, ad.up_sampler
        z = torch.from_numpy(S.linear(x.numpy(), d.phm_rule.detach().numpy(), d.W.detach().numpy(), d.b.detach().numpy())).float()
        z = ad.activation(z)
        want = S.linear(z.numpy(), u.phm_rule.detach().numpy(), u.W.detach().numpy(), u.b.detach().numpy()) + x.numpy()
        torch.testing.assert_close(out.detach(), torch.from_numpy(want).float(), rtol=1e-4, atol=1e-4)
        if over.get("track_z"):
            assert tuple(ad.z.shape) == (3, 8)
    assert not AdapterController(_ac()).adapters["vqa"].eager and not AdapterController(_ac(hypercomplex_division=8)).adapters["vqa"].eager


def test_existing_paths_build_as_before():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    from vlpet_amd.adapters import Adapter
    for cfg in (HB.vlpet_config(), HT.vlt5_config()):
        assert cfg.use_compacter is False and not cfg.adapter_config.hypercomplex_adapters
        assert (cfg.hypercomplex_division, cfg.phm_rank, cfg.shared_phm_rule, cfg.factorized_phm, cfg.phm_init_range,
                cfg.shared_phm_rule_over_tasks) == (4, 1, True, True, 0.01, False)          # param.py:163-170
    import single_adapter_cases as SA
    model = SA.build("bart")[0]
    assert type(model.model.decoder.layers[0].ff_adapter.adapters["vqa"]) is Adapter


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
