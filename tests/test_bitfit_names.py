"""The BitFit baseline (scripts/image-text/bitfit.sh: ``--unfreeze_bias``) on the host models, without a GPU: the trainable set is the
reference's name for name and in order, the state dict is the reference's, the flag combines with the other PET flags by union, and the
library, its header and the ctypes table agree on the entry points of csrc/biasgrad.hip.  The fixtures are the reference's own VLBart /
VLT5 under that flag set (tests/golden/make_bitfit_goldens.py)."""
import os
import re

import pytest

import bitfit_cases as C

KINDS = ["bart", "t5"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vlpet_colsum_seg", "vlpet_colsum_seg_workspace_bytes", "vlpet_act_dropout_bwd_cols")


def test_the_config_field_exists_and_defaults_to_off():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    for make in (HB.vlpet_config, HT.vlt5_config):
        assert make().unfreeze_bias is False and make(unfreeze_bias=True).unfreeze_bias is True


@pytest.mark.parametrize("kind", KINDS)
def test_trainable_names_are_the_references_in_order(kind):
    model, cfg, names, unexpected = C.build(kind)
    assert set(unexpected) <= {"lm_head.weight"}, unexpected
    want = C.reference_names(kind)
    assert sorted(names) == sorted(want)
    # ... and in the reference's order, up to the one place where the host registers its modules in another order than the reference:
    # inside an attention the host lists q, v, k (the LoRA pair first), the reference k, v, q
    blur = lambda ns: [re.sub(r"\.[qkv]_proj\.", ".qkv_proj.", n) for n in ns]
    assert blur(names) == blur(want)
    assert list(C.fixture(kind)[4]) == want                  # the fixture's final parameters are listed in the same order
    assert all(p.requires_grad == (n in set(want)) for n, p in model.named_parameters())
    if kind == "bart":
        for part in ("q_proj.bias", "k_proj.bias", "v_proj.bias", "out_proj.bias", "fc1.bias", "fc2.bias", "self_attn_layer_norm.bias",
                     "encoder_attn_layer_norm.bias", "final_layer_norm.bias", "layernorm_embedding.bias", "visual_embedding"):
            assert any(part in n for n in names), part
        assert not [n for n in names if "bias" not in n and "visual_embedding" not in n]
        assert not [n for n in names if n.endswith("layer_norm.weight") or n.endswith("layernorm_embedding.weight")]
    else:
        # T5 has no Linear bias and its norms have none: besides the visual embedding the substring rule catches the relative-position tables
        other = [n for n in names if "visual_embedding" not in n]
        assert other == ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
                         "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]


@pytest.mark.parametrize("kind", KINDS)
def test_without_the_flag_only_the_visual_embedding_trains(kind):
    _, _, names, _ = C.build(kind, bitfit=False)
    assert names and all("visual_embedding" in n for n in names)
    assert set(names) < set(C.reference_names(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_shapes_are_the_references(kind):
    sd = C.fixture(kind)[0]
    model = C.new_model(kind, C.config(kind))
    host = model.state_dict()
    head = {"lm_head.weight"}                                # tied head: the host reuses the shared embedding
    assert set(host) == set(sd) - head
    assert all(tuple(host[k].shape) == tuple(sd[k].shape) for k in host)
    assert set(host) == set(C.new_model(kind, C.config(kind, bitfit=False)).state_dict())        # the flag adds no parameter


@pytest.mark.parametrize("kind", KINDS)
def test_the_flag_joins_other_pet_flags_by_union(kind):
    """unfreeze_bias next to the layer-norm rule, and (BART) next to the VL-PET adapters: what either flag set trains alone, and nothing else"""
    import vlpet_amd.train as TR

    def names(**over):
        cfg = C.config(kind, **over)
        return set(TR.trainable_names(C.new_model(kind, cfg), cfg))
    both = names(unfreeze_layer_norms=True)
    assert both == names() | names(bitfit=False, unfreeze_layer_norms=True)
    assert any(n.endswith("layer_norm.weight") for n in both)
    if kind == "bart":
        pet = dict(use_encoder_adapter_down_multihead=True, use_encoder_adapter_gating_large_x_lowrank=True, unfreeze_encoder_layer_norms=True,
                   adapter_down_dim=8, adapter_gating_down_dim=8)
        with_pet = names(**pet)
        alone = names(bitfit=False, **pet)
        biases = {n for n in with_pet if "bias" in n}
        assert alone < with_pet and with_pet == alone | biases
        assert any("adapter" in n for n in alone) and any("q_proj.bias" in n for n in with_pet - alone)


def test_header_ctypes_table_and_library_agree_on_the_new_entry_points():
    from vlpet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "vlpet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    assert lib.vlpet_version() >= 690
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} is not declared in include/vlpet_hip.h"
        assert s in _lib.SIGNATURES and hasattr(lib, s)
        n_args = len(re.search(r"\b" + s + r"\s*\(([^;]*)\)\s*;", txt, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[s][1]), s
    # argument errors come back as negative codes before any launch (no GPU needed)
    assert lib.vlpet_colsum_seg_workspace_bytes(28000, 2304) == 1024 * 2304 * 4 and lib.vlpet_colsum_seg_workspace_bytes(0, 64) == 0
    assert lib.vlpet_colsum_seg(None, 8, 3, 64, 192, None, None, 0, _lib.VLPET_BF16, None) == -5
    assert lib.vlpet_colsum_seg(None, 8, 17, 16, 272, None, None, 0, _lib.VLPET_BF16, None) == -1
    assert lib.vlpet_colsum_seg(None, 8, 3, 72, 216, None, None, 0, _lib.VLPET_BF16, None) == -1
    assert lib.vlpet_colsum_seg(None, 8, 3, 64, 128, None, None, 0, _lib.VLPET_BF16, None) == -1
    assert lib.vlpet_act_dropout_bwd_cols(None, None, None, 8, 60, 0, 0.0, 0, None, 0, None, None, _lib.VLPET_BF16, None) == -1
    assert lib.vlpet_act_dropout_bwd_cols(None, None, None, 8, 64, 0, 0.0, 0, None, 0, None, None, _lib.VLPET_BF16, None) == -5


@pytest.mark.parametrize("kind", KINDS)
def test_logits_and_training_losses_match_the_reference_cpu(kind):
    """the host and the trainer under the flag against the reference's run, HIP-backed ops swapped for the eager restatement"""
    from oracle.host_patch import cpu_reference_ops
    from test_host_golden import _check
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, _ = C.build(kind)
    with cpu_reference_ops():
        _check(model, cfg, names, batches, ref_losses, hp, final, "cpu", 2e-5)
