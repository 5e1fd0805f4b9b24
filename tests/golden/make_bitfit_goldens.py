#!/usr/bin/env python3
"""Generate the BitFit fixtures from the reference's OWN classes (run where the reference checkout is, next to make_goldens.py):

    python tests/golden/make_bitfit_goldens.py

Flag set = scripts/image-text/bitfit.sh: ``--unfreeze_bias`` and no PET module of any kind; the visual embedding and every parameter
whose name contains "bias" train (trainer_base.py:309-315, :469-475), everything else is frozen (:296-306).  Written:

  vlbart_tiny_bitfit_d64.npz       every Linear and LayerNorm bias of both stacks + the visual embedding
  vlt5_tiny_bitfit_d64.npz         T5 has no Linear bias and its norms none either: the trainable set is the visual embedding plus what
                                   else the substring rule catches, the two ``relative_attention_bias.weight`` tables
      layout of the Single-Adapter fixtures (make_single_adapter_goldens.golden_model: ``sd::``, ``b{i}::``, ``train::``, ``final::``)
      plus ``train::names``, the trainable names in named_parameters() order
  bitfit/gen_vlbart_bitfit.npz     greedy tokens FROM THE TRAINED STATE (sd:: overlaid with final::): layout of make_generate_goldens.case

The model geometry, the batches, the training loop and the greedy driver are make_single_adapter_goldens' (imported, with this file's
build_model / set_trainable / NAMES in their place).  Every trainable parameter gets a gradient in every step (there is no per-task
module), so the loop's global AdamW step count is every parameter's own; main() checks the number of updates."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG  # noqa: E402
import make_generate_goldens as MGG  # noqa: E402
import make_single_adapter_goldens as MSA  # noqa: E402

FLAGS = ["--tasks", "vqa,gqa,nlvr,caption", "--unfreeze_bias", "--downsample", "--n_boxes", "36"]
NAMES = {"bart": "vlbart_tiny_bitfit_d64", "t5": "vlt5_tiny_bitfit_d64"}
SUB = "bitfit"
STEPS = 5


def build_model(kind, seed=None):
    mod = MG.load_vl_module(kind)
    config, args = MG.make_config(kind, list(FLAGS), d_model=64, heads=4, ffn=MSA.FFN)
    assert args.unfreeze_bias and not config.use_adapter and config.adapter_config is None and not config.use_lora
    assert not config.use_decoder_enc_attn_value_parallel_adapter_down_dim and not config.unfreeze_layer_norms
    if kind == "t5":
        MG.install_t5_runtime_shim()
        config.decoder_start_token_id = 0
        config.pad_token_id = 0
    config.vocab_size = MSA.VOCAB
    if kind == "bart":
        config.max_position_embeddings = MSA.MAX_POS
    config.feat_dim = MSA.FEAT
    config.default_obj_order_ids = list(range(MSA.TOK_HI, MSA.VOCAB))
    config.encoder_prompt_config = None
    config.decoder_prompt_config = None
    from transformers import PreTrainedModel
    PreTrainedModel.init_weights = lambda self: self.apply(self._init_weights)
    torch.manual_seed(0 if seed is None else seed)
    model = mod.VLBart(config) if kind == "bart" else mod.VLT5(config)
    return model, config


def set_trainable(model):
    """TrainerBase.unfreeze_parameters for this flag set: everything frozen (trainer_base.py:296-306), then the visual embedding
    (:309-315: ``any(t in n for t in ["visual_embedding"])``) and every bias (:469-475: ``any(t in n for t in ["bias"])``)"""
    for p in model.parameters():
        p.requires_grad = False
    for n, p in model.named_parameters():
        if "visual_embedding" in n:
            p.requires_grad = True
    for n, p in model.named_parameters():
        if "bias" in n:
            p.requires_grad = True


def golden_model(kind, seed):
    """make_single_adapter_goldens.golden_model on this file's model and trainable set, then ``train::names`` added"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import vlpet_oracle as O
    kept = {}

    def build(kind_, seed_=None):
        model, config = build_model(kind_, seed_)
        kept["model"] = model
        return model, config
    updates = []
    real_step = O.hf_adamw_step

    def counted(p, g, m, v, step, *a, **kw):
        updates.append(step)
        return real_step(p, g, m, v, step, *a, **kw)
    saved = MSA.build_model, MSA.set_trainable, MSA.NAMES
    MSA.build_model, MSA.set_trainable, MSA.NAMES, O.hf_adamw_step = build, set_trainable, NAMES, counted
    try:
        MSA.golden_model(kind, seed)
    finally:
        MSA.build_model, MSA.set_trainable, MSA.NAMES = saved
        O.hf_adamw_step = real_step
    names = [n for n, p in kept["model"].named_parameters() if p.requires_grad]
    # every parameter got a gradient at every step: the global step count the loop passes is each parameter's own
    assert len(updates) == STEPS * len(names) and sorted(set(updates)) == list(range(1, STEPS + 1)), (len(updates), len(names))
    if kind == "t5":
        # T5 has no Linear or norm bias, but the substring rule also catches the two relative-position tables
        other = [n for n in names if "visual_embedding" not in n]
        assert other == ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
                         "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], other
    else:
        assert any("q_proj.bias" in n for n in names) and any("fc1.bias" in n for n in names) and any("layernorm_embedding.bias" in n for n in names)
    path = os.path.join(HERE, NAMES[kind] + ".npz")
    z = np.load(path, allow_pickle=False)
    arrs = {k: z[k] for k in z.files}
    assert [k[7:] for k in z.files if k.startswith("final::")] == names
    arrs["train::names"] = np.array(names)
    MG.save(NAMES[kind], **arrs)


def build_reference(name, lora=False, kind="bart", video=False):
    """stands in for make_generate_goldens.build_reference: the BitFit model in its TRAINED state -- ``sd::`` of ``name``.npz overlaid with
    its ``final::`` parameters (generation after training must see the updated biases)"""
    model, config = build_model(kind)
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    sd.update({k[7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("final::")})
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(MSA.ALIASES) for k in missing), missing
    MSA.tie(model, kind)
    model.eval()
    return model, config


def main():
    MG.install_shim()
    which = sys.argv[1:] or ["models", "generate"]
    if "models" in which:
        golden_model("bart", 42)
        golden_model("t5", 43)
    if "generate" in which:
        os.makedirs(os.path.join(HERE, SUB), exist_ok=True)
        MGG.build_reference = build_reference
        MGG.make_inputs = MSA.make_inputs
        MGG.case(SUB + "/gen_vlbart_bitfit", NAMES["bart"], "vqa", max_length=10, min_length=3, ngram=2, seed0=1500, mixed=False)


if __name__ == "__main__":
    main()
