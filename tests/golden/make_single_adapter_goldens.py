#!/usr/bin/env python3
"""Generate the Single-Adapter fixtures from the reference's OWN classes (run where the reference checkout is, next to make_goldens.py):

    python tests/golden/make_single_adapter_goldens.py

Flag set = scripts/image-text/single_adapter.sh: ``--use_adapter --unfreeze_layer_norms --reduction_factor 8 --use_single_adapter``
(one shared bottleneck adapter of width d / 8 behind every attention and feed-forward block of encoder and decoder; every LayerNorm
trains).  Written:

  vlbart_tiny_single_adapter_d64.npz, vlt5_tiny_single_adapter_d64.npz   layout of vlbart_tiny_d64.npz (make_goldens.golden_vlbart_tiny:
      ``sd::`` state dict, ``b{i}::`` three task batches with eval logits / per-token losses, ``train::`` five training-step losses,
      ``final::`` the trainable parameters afterwards), d = 64, r = 8
  single_adapter/gen_vlbart_single_adapter.npz, single_adapter/beam_vlbart_single_adapter.npz          layouts of make_generate_goldens.case / make_beam_goldens.case

The helpers (import shim, config mirror, batches' conventions, greedy / beam drivers) are make_goldens' / make_generate_goldens' /
make_beam_goldens', imported; only the model geometry differs, to keep each file small: feed-forward width 32, 240 tokens (object-order
ids 140 .. 239), 40 positions, 64-dimensional visual features in steps of 1/8 (they compress), two rows per batch, and the aliases of the shared embedding (lm_head, embed_tokens)
left out of ``sd::``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG  # noqa: E402
import make_generate_goldens as MGG  # noqa: E402
import make_beam_goldens as MBG  # noqa: E402

FLAGS = ["--tasks", "vqa,gqa,nlvr,caption", "--use_adapter", "--unfreeze_layer_norms", "--reduction_factor", "8", "--use_single_adapter",
         "--downsample", "--n_boxes", "36"]
VOCAB, FEAT, FFN, TOK_HI, MAX_POS = 240, 64, 32, 140, 40
NAMES = {"bart": "vlbart_tiny_single_adapter_d64", "t5": "vlt5_tiny_single_adapter_d64"}
SUB = "single_adapter"     # the generation fixtures' folder: tests/test_generate.py / test_beam.py take every golden/gen_*.npz / beam_*.npz for their own models
ALIASES = ("lm_head.weight", "embed_tokens.weight")


def build_model(kind, seed=None):
    mod = MG.load_vl_module(kind)
    config, _ = MG.make_config(kind, list(FLAGS), d_model=64, heads=4, ffn=FFN)
    assert config.use_adapter and not config.no_encoder_adapter and not config.no_decoder_adapter and config.add_adapter_cross_attn
    assert not config.adapter_config.use_adapter_down_dim and config.adapter_config.reduction_factor == 8
    if kind == "t5":
        MG.install_t5_runtime_shim()
        config.decoder_start_token_id = 0
        config.pad_token_id = 0
    config.vocab_size = VOCAB
    if kind == "bart":
        config.max_position_embeddings = MAX_POS
    config.feat_dim = FEAT
    config.default_obj_order_ids = list(range(TOK_HI, VOCAB))
    config.encoder_prompt_config = None
    config.decoder_prompt_config = None
    from transformers import PreTrainedModel
    PreTrainedModel.init_weights = lambda self: self.apply(self._init_weights)
    torch.manual_seed(0 if seed is None else seed)
    model = mod.VLBart(config) if kind == "bart" else mod.VLT5(config)
    return model, config


def tie(model, kind):
    model.lm_head.weight = model.model.shared.weight if kind == "bart" else model.shared.weight
    if kind == "bart":
        model.model.encoder.embed_tokens = model.model.shared
        model.model.decoder.embed_tokens = model.model.shared


def set_trainable(model):
    """TrainerBase.unfreeze_parameters for this flag set (trainer_base.py:309-315 visual embedding, :375-380 every LayerNorm /
    T5LayerNorm module, :389-393 every AdapterController), everything else frozen (:296-306)"""
    import torch.nn as nn
    from adapters import AdapterController
    from my_transformers.modeling_t5 import T5LayerNorm
    for p in model.parameters():
        p.requires_grad = False
    for n, p in model.named_parameters():
        if "visual_embedding" in n:
            p.requires_grad = True
    for m in model.modules():
        if isinstance(m, (T5LayerNorm, nn.LayerNorm, AdapterController)):
            for p in m.parameters():
                p.requires_grad = True


def coarse(x):
    """visual features in steps of 1/8: as good as any for the models, a fraction of the bytes in the compressed file"""
    return (x * 8).round() / 8


def golden_model(kind, seed):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import vlpet_oracle as O
    model, config = build_model(kind, seed)
    gen = torch.Generator().manual_seed(seed)
    MG.randomize(model, gen)
    tie(model, kind)
    set_trainable(model)
    B = 2

    def batch(task, L, T):
        ids = torch.randint(5, TOK_HI, (B, L), generator=gen)
        labels = torch.randint(5, TOK_HI, (B, T), generator=gen)
        if task == "nlvr":
            feats = coarse(torch.randn(B, 98, FEAT, generator=gen))
            boxes = torch.zeros(B, 98, 4)
            img = torch.cat([torch.zeros(49), torch.ones(49)]).long().unsqueeze(0).expand(B, -1).contiguous()
            obj = torch.cat([torch.arange(49), torch.arange(49)]).unsqueeze(0).expand(B, -1).contiguous()
            vis = (feats, boxes, img, obj)
        else:
            vis = (coarse(torch.randn(B, 49, FEAT, generator=gen)), torch.zeros(B, 49, 4))
        scores = torch.rand(B, generator=gen) * 0.5 + 0.5
        return dict(task=task, ids=ids, labels=labels, vis=vis, scores=scores)
    batches = [batch("vqa", 20, 5), batch("nlvr", 20, 2), batch("caption", 12, 9)]

    def run(b):
        out = model(input_ids=b["ids"], vis_inputs=b["vis"], labels=b["labels"], return_dict=True, task=b["task"])
        return out["loss"].view(b["labels"].shape), out["logits"]

    def reduce(b, per):
        mask = (b["labels"] != -100).float()
        if b["task"] in ("vqa", "gqa"):
            return ((per * mask).sum(1) / mask.sum(1).clamp(min=1) * b["scores"]).mean()
        return (per * mask).sum() / mask.sum().clamp(min=1)

    arrs = {"sd::" + k: MG.T(v) for k, v in model.state_dict().items() if not k.endswith(ALIASES)}
    model.eval()
    with torch.no_grad():
        for i, b in enumerate(batches):
            per, logits = run(b)
            arrs.update({f"b{i}::task": np.array(b["task"]), f"b{i}::ids": b["ids"].numpy(), f"b{i}::labels": b["labels"].numpy(),
                         f"b{i}::scores": MG.T(b["scores"]), f"b{i}::per_token": MG.T(per), f"b{i}::logits": MG.T(logits),
                         f"b{i}::loss": MG.T(reduce(b, per))})
            for j, v in enumerate(b["vis"]):
                arrs[f"b{i}::vis{j}"] = v.numpy()
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    state = {n: (torch.zeros_like(p), torch.zeros_like(p)) for n, p in named}
    losses = []
    total, warm, base_lr = 10, 1, 5e-3
    for step in range(5):
        b = batches[step % 3]
        for _, p in named:
            p.grad = None
        per, _ = run(b)
        loss = reduce(b, per)
        loss.backward()
        losses.append(float(loss))
        torch.nn.utils.clip_grad_norm_([p for _, p in named], 5.0)
        lr = O.linear_warmup_lr(step, base_lr, warm, total)
        for n, p in named:
            wd = 0.0 if any(nd in n for nd in ("bias", "LayerNorm.weight")) else 0.01
            m, v = state[n]
            if p.grad is None:
                continue
            O.hf_adamw_step(p.data, p.grad, m, v, step + 1, lr, eps=1e-6, weight_decay=wd)
    arrs["train::losses"] = np.array(losses, dtype=np.float64)
    arrs["train::hparams"] = np.array([base_lr, total, warm, 5.0])
    for n, p in named:
        arrs["final::" + n] = MG.T(p.data)
    MG.save(NAMES[kind], **arrs)


def build_reference(name, lora=False, kind="bart", video=False):
    """stands in for make_generate_goldens.build_reference: the Single-Adapter model with the weights of ``name``.npz"""
    model, config = build_model(kind)
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(ALIASES) for k in missing), missing
    tie(model, kind)
    model.eval()
    return model, config


def make_inputs(gen, kind, video, L, pad):
    """make_generate_goldens.make_inputs at this model's feature width"""
    B = MGG.B
    ids = torch.randint(5, TOK_HI, (B, 1), generator=gen).expand(B, L).contiguous()
    feats = torch.randn(B, 1, FEAT, generator=gen).expand(B, 49, FEAT).contiguous()
    vis = (feats, torch.rand(B, 49, 4, generator=gen))
    for i, n in enumerate((L, L, L - 4, L)):
        ids[i, n:] = pad
    return ids, vis


def main():
    MG.install_shim()
    which = sys.argv[1:] or ["models", "generate"]
    if "models" in which:
        golden_model("bart", 22)
        golden_model("t5", 23)
    if "generate" in which:
        os.makedirs(os.path.join(HERE, SUB), exist_ok=True)
        MGG.build_reference = build_reference
        MGG.make_inputs = make_inputs
        # (the tiny model decodes every row alike and, left alone, repeats one token: the n-gram ban and the minimum length make the
        # steps differ, as in make_generate_goldens' caption case; ``mixed=False`` as for its LoRA and video cases)
        MGG.case(SUB + "/gen_vlbart_single_adapter", NAMES["bart"], "vqa", max_length=12, min_length=4, ngram=2, seed0=1100, mixed=False)
        MBG.case(SUB + "/beam_vlbart_single_adapter", NAMES["bart"], "caption", K=4, max_length=12, min_length=4, ngram=2, seed0=1200)


if __name__ == "__main__":
    main()
