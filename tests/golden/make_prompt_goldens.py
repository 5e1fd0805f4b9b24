#!/usr/bin/env python3
"""Generate the prompt-tuning fixtures from the reference's OWN classes (run where the reference checkout is, next to make_goldens.py):

    python tests/golden/make_prompt_goldens.py

Flag set = scripts/image-text/single_prompt.sh: ``--encoder_prompt_len P --mid_dim M --use_single_prompt`` (one InputPrompts module --
Embedding(P, d) -> Linear(d, M) -> Tanh -> Linear(M, d) -- whose P rows go in front of the text rows of the joint encoder; no adapter of
any kind; the visual embedding and every PromptController train, trainer_base.py:309-315, :347).  Written, with P = 5 and M = 24:

  vlbart_tiny_prompt_d64.npz       --use_single_prompt: one module under every task key
  vlt5_tiny_prompt_d64.npz         --use_single_prompt dropped: one module per task (the controller's other branch)
      layout of the Single-Adapter fixtures (make_single_adapter_goldens.golden_model: ``sd::``, ``b{i}::``, ``train::``, ``final::``)
  prompt/gen_vlbart_prompt.npz, prompt/beam_vlbart_prompt.npz      layouts of make_generate_goldens.case / make_beam_goldens.case

The model geometry, the batches' conventions and the greedy / beam drivers are make_single_adapter_goldens' (imported); the flag set, the
config's prompt fields and the trainable set differ, and so does one point of the training loop: with one prompt per task a parameter
gets a gradient only in its own task's steps, and transformers.AdamW counts the steps of every parameter separately (state['step'],
the bias correction) -- the loops of the other generators, whose trainable parameters all get a gradient in every step, pass the global
count.  The reference leaves ``encoder_prompt_config.input_dim`` at its
default 768 (trainer_base.py:184-189: the backbones it is run with are 768 wide); the tiny model needs its own width there."""
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
import make_single_adapter_goldens as MSA  # noqa: E402

P, MID = 5, 24
BASE = ["--tasks", "vqa,gqa,nlvr,caption", "--encoder_prompt_len", str(P), "--mid_dim", str(MID), "--downsample", "--n_boxes", "36"]
FLAGS = {"bart": BASE + ["--use_single_prompt"], "t5": BASE}
NAMES = {"bart": "vlbart_tiny_prompt_d64", "t5": "vlt5_tiny_prompt_d64"}
SUB = "prompt"


def build_model(kind, seed=None):
    import re
    from prompt import EncoderPromptConfig
    mod = MG.load_vl_module(kind)
    config, args = MG.make_config(kind, list(FLAGS[kind]), d_model=64, heads=4, ffn=MSA.FFN)
    assert not config.use_adapter and config.adapter_config is None and not config.use_lora
    if kind == "t5":
        MG.install_t5_runtime_shim()
        config.decoder_start_token_id = 0
        config.pad_token_id = 0
    config.vocab_size = MSA.VOCAB
    if kind == "bart":
        config.max_position_embeddings = MSA.MAX_POS
    config.feat_dim = MSA.FEAT
    config.default_obj_order_ids = list(range(MSA.TOK_HI, MSA.VOCAB))
    # trainer_base.py:184-200
    pc = EncoderPromptConfig()
    pc.prompt_len = args.encoder_prompt_len
    pc.tasks = re.split("[, ]+", args.tasks)
    pc.use_single_prompt = args.use_single_prompt
    pc.mid_dim = args.mid_dim
    pc.input_dim = config.d_model
    assert pc.prompt_len == P and pc.mid_dim == MID and pc.use_single_prompt == (kind == "bart") and args.decoder_prompt_len == 0
    config.encoder_prompt_config = pc
    config.decoder_prompt_config = None
    from transformers import PreTrainedModel
    PreTrainedModel.init_weights = lambda self: self.apply(self._init_weights)
    torch.manual_seed(0 if seed is None else seed)
    model = mod.VLBart(config) if kind == "bart" else mod.VLT5(config)
    return model, config


def set_trainable(model):
    """TrainerBase.unfreeze_parameters for this flag set (trainer_base.py:309-315 visual embedding, :347-351 every PromptController),
    everything else frozen (:296-306)"""
    from prompt import PromptController
    for p in model.parameters():
        p.requires_grad = False
    for n, p in model.named_parameters():
        if "visual_embedding" in n:
            p.requires_grad = True
    for m in model.modules():
        if isinstance(m, PromptController):
            for p in m.parameters():
                p.requires_grad = True


def golden_model(kind, seed):
    """make_single_adapter_goldens.golden_model with per-parameter AdamW step counts (see the module docstring)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import vlpet_oracle as O
    FEAT, TOK_HI, coarse = MSA.FEAT, MSA.TOK_HI, MSA.coarse
    model, config = build_model(kind, seed)
    gen = torch.Generator().manual_seed(seed)
    MG.randomize(model, gen)
    MSA.tie(model, kind)
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

    arrs = {"sd::" + k: MG.T(v) for k, v in model.state_dict().items() if not k.endswith(MSA.ALIASES)}
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
    count = {n: 0 for n, _ in named}
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
            if p.grad is None:              # another task's prompt: transformers.AdamW skips it (no decay, no moments, no count)
                continue
            wd = 0.0 if any(nd in n for nd in ("bias", "LayerNorm.weight")) else 0.01
            m, v = state[n]
            count[n] += 1
            O.hf_adamw_step(p.data, p.grad, m, v, count[n], lr, eps=1e-6, weight_decay=wd)
    if kind == "t5":
        assert sorted(set(count.values())) == [0, 1, 2, 5], sorted(set(count.values()))     # gqa never, caption once, vqa / nlvr twice
    arrs["train::losses"] = np.array(losses, dtype=np.float64)
    arrs["train::hparams"] = np.array([base_lr, total, warm, 5.0])
    for n, p in named:
        arrs["final::" + n] = MG.T(p.data)
    MG.save(NAMES[kind], **arrs)


def build_reference(name, lora=False, kind="bart", video=False):
    """stands in for make_generate_goldens.build_reference: the prompt-tuned model with the weights of ``name``.npz"""
    model, config = build_model(kind)
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
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
        golden_model("bart", 32)
        golden_model("t5", 33)
    if "generate" in which:
        os.makedirs(os.path.join(HERE, SUB), exist_ok=True)
        MGG.build_reference = build_reference
        MGG.make_inputs = MSA.make_inputs
        # (as make_single_adapter_goldens: the n-gram ban and the minimum length make the steps of the tiny model differ; the lengths are
        # shorter than there so that neither file outgrows its Single-Adapter counterpart)
        MGG.case(SUB + "/gen_vlbart_prompt", NAMES["bart"], "vqa", max_length=10, min_length=3, ngram=2, seed0=1300, mixed=False)
        MBG.case(SUB + "/beam_vlbart_prompt", NAMES["bart"], "caption", K=4, max_length=7, min_length=3, ngram=2, seed0=1400)


if __name__ == "__main__":
    main()
