#!/usr/bin/env python3
"""Generate the Hyperformer fixtures (controllers alone, host models, generation) from the reference's OWN classes (run where the reference checkout is, next to
make_goldens.py):

    python tests/golden/make_hyperformer_goldens.py

  hyper_ctl_unique_d64_r8_p8.npz     AdapterLayersHyperNetController (``--unique_hyper_net``), two layers, with cross-attention
  hyper_ctl_one_d64_r8_p8.npz        AdapterLayersOneHyperNetController (``--efficient_unique_hyper_net``), likewise

Each holds the reference controller ALONE at the tiny geometry of the model fixtures (d = 64, reduction 8, task_hidden_dim 128,
projected_task_embedding_dim 8 as scripts/image-text/hyperformer.sh sets it; task_embedding_dim 64 instead of the default 512, which
only widens the MLP's first layer and would put each file above 1 MiB): the parameters (``p::<name>``), a
task embedding (``task_embedding``), every layer's outputs (``out::<layer>::<block>::<down|up>::<weight|bias>``), upstream gradients
of all of them (``dout::...``), every parameter gradient (``d::<name>``) and the task embedding's (``d_task_embedding``) of
``sum(out * dout)`` over every output of every layer, and the embeddings the generators see (``emb::<layer>`` or
``emb::<layer>::<block>``).

  vlbart_tiny_hyperformer_d64, vlbart_tiny_hyperformer_one_d64, vlt5_tiny_hyperformer_d64     the reference's VLBart (both hyper-network
      forms) and VLT5 under scripts/image-text/hyperformer.sh's flags at make_single_adapter_goldens' tiny geometry, each as TWO files
      below 1 MiB: ``<name>.npz`` (``sd::``, the task embeddings under all three of their names) and ``<name>_steps.npz`` (``b{i}::``,
      ``train::``, ``final::``, ``names::trainable``; per-parameter AdamW step counts as in make_prompt_goldens).  ``assert_alive`` holds
      each to: another task moves the logits by >= 10 x the checks' tolerance, so do zeroed generators, and no hyper-network parameter
      of a task in the batches has a zero gradient
  hyperformer/gen_vlbart_hyperformer.npz, gen_vlt5_hyperformer.npz, beam_vlt5_hyperformer.npz     layouts of make_generate_goldens.case /
      make_beam_goldens.case

The controllers' parameters are make_goldens.randomize's (std 0.05), then rescaled so that the hyper-network is alive: LayerNorm weight + 1, the
layer-id (and block-type) embeddings and the task embedding x 20 -- with everything at 0.05 the MLP's output is a rounding error of
its biases and the LayerNorm divides noise by noise."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG  # noqa: E402

D, REDUCTION, P, LAYERS, TASK_DIM = 64, 8, 8, 2, 64
BLOCKS = ("self_attention", "feed_forward", "cross_attention")


def meta_config():
    """trainer_base.py:127-178 for --use_hyperformer --projected_task_embedding_dim 8 --reduction_factor 8"""
    from adapters.config import MetaAdapterConfig
    ac = MetaAdapterConfig()
    ac.tasks = ["vqa", "gqa", "nlvr", "caption"]
    ac.input_dim = D
    ac.d_model = D
    ac.reduction_factor = REDUCTION
    ac.projected_task_embedding_dim = P
    ac.task_embedding_dim = TASK_DIM
    ac.track_z = False
    return ac


def golden_controller(form, seed):
    MG.install_shim()
    from adapters.adapter_hypernetwork import AdapterLayersHyperNetController, AdapterLayersOneHyperNetController
    ac = meta_config()
    ac.unique_hyper_net, ac.efficient_unique_hyper_net = form == "unique", form == "one"
    torch.manual_seed(seed)
    ctl = (AdapterLayersHyperNetController if form == "unique" else AdapterLayersOneHyperNetController)(ac, LAYERS, True)
    gen = torch.Generator().manual_seed(seed)
    MG.randomize(ctl, gen)
    with torch.no_grad():
        ctl.LayerNorm.weight.add_(1.0)
        ctl.layer_id_embeddings.weight.mul_(20.0)
        if form == "one":
            ctl.adapters_block_type.weight.mul_(20.0)
    task_embedding = (torch.randn(ac.task_embedding_dim, generator=gen) * 0.05 * 20.0).requires_grad_(True)
    arrs = {"task_embedding": MG.T(task_embedding), "layers": np.array(LAYERS), "d": np.array(D), "r": np.array(D // REDUCTION),
            "P": np.array(P)}
    loss = 0
    for layer in range(LAYERS):
        out = ctl(task_embedding, layer)
        if form == "unique":
            arrs[f"emb::{layer}"] = MG.T(ctl.get_embedding(task_embedding, layer))
        else:
            for b, block in ((0, "feed_forward"), (1, "self_attention"), (2, "cross_attention")):
                arrs[f"emb::{layer}::{block}"] = MG.T(ctl.get_embedding(task_embedding, layer, b))
        for block in BLOCKS:
            pair = getattr(out, block)
            for side in ("down", "up"):
                for what in ("weight", "bias"):
                    t = getattr(getattr(pair, side), what)
                    dt = torch.randn(t.shape, generator=gen)
                    key = f"{layer}::{block}::{side}::{what}"
                    arrs["out::" + key], arrs["dout::" + key] = MG.T(t), dt
                    loss = loss + (t * dt).sum()
    loss.backward()
    arrs["d_task_embedding"] = MG.T(task_embedding.grad)
    for k, p in ctl.named_parameters():
        arrs["p::" + k] = MG.T(p)
        arrs["d::" + k] = MG.T(p.grad)
        assert float(p.grad.abs().max()) > 0, k
    assert float(task_embedding.grad.abs().max()) > 0
    # the hyper-network is alive: another task embedding moves the generated weights by far more than a test's tolerance
    with torch.no_grad():
        other = ctl(torch.randn(ac.task_embedding_dim, generator=gen), 0).self_attention.down.weight
        moved = float((other - arrs["out::0::self_attention::down::weight"]).abs().max())
    assert moved > 1e-2, moved
    print(f"  {form}: another task embedding moves layer 0's self-attention down weight by {moved:.3e}")
    MG.save(f"hyper_ctl_{form}_d{D}_r{D // REDUCTION}_p{P}", **arrs)


# ---------------------------------------------------------------------------------------------------------------- the host models
import make_generate_goldens as MGG  # noqa: E402
import make_beam_goldens as MBG  # noqa: E402
import make_single_adapter_goldens as MSA  # noqa: E402
import make_prompt_goldens as MP  # noqa: E402

COMMON = ["--tasks", "vqa,gqa,nlvr,caption", "--use_hyperformer", "--unfreeze_layer_norms", "--projected_task_embedding_dim", "8",
          "--reduction_factor", "8", "--downsample", "--n_boxes", "36"]
FLAGS = {"unique": COMMON + ["--unique_hyper_net"], "one": COMMON + ["--efficient_unique_hyper_net"]}
NAMES = {("bart", "unique"): "vlbart_tiny_hyperformer_d64", ("t5", "unique"): "vlt5_tiny_hyperformer_d64",
         ("bart", "one"): "vlbart_tiny_hyperformer_one_d64"}
SUB = "hyperformer"
STEPS = "_steps"             # <name>.npz holds ``sd::``; <name>_steps.npz the batches, ``train::``, ``final::`` and ``names::trainable``
TOL = 1e-3                   # the tolerance of the checks that use the model fixtures (tests/test_host_golden._check on the GPU)
SCALE = {"bart": 20.0, "t5": 20.0}      # layer-id / block-type embeddings
TASK_SCALE = {"bart": 20.0, "t5": 20.0}  # the task embeddings
# T5: larger hyper-network factors do not help (measured: generators x 4, x 8, x 32 and task embeddings x 80 all leave the task swap at
# 8e-3) because randomize leaves the stacks' final RMS norms with weights ~ 0.05 and every logit below 8e-3; the two final norms get
# weight + 1 (as the hyper-networks' LayerNorm does), which puts the logits at BART's scale
GEN_SCALE = {"bart": 4.0, "t5": 8.0}    # the adapter generators' weights; T5's logits move less per unit, it needs the larger factor


def model_meta_config(config, args):
    """trainer_base.py:127-178 for --use_hyperformer; task_embedding_dim 64 as for the controller fixtures (the file size)"""
    ac = meta_config()
    ac.use_single_adapter = args.use_single_adapter
    ac.unique_hyper_net = args.unique_hyper_net
    ac.efficient_unique_hyper_net = args.efficient_unique_hyper_net
    ac.add_layer_norm_before_adapter = args.add_layer_norm_before_adapter
    ac.add_layer_norm_after_adapter = args.add_layer_norm_after_adapter
    ac.use_adapter_down_dim = bool(args.use_adapter_down_dim)
    ac.adapter_down_dim = args.adapter_down_dim
    return ac


def make_build_model(form):
    def build_model(kind, seed=None):
        mod = MG.load_vl_module(kind)
        config, args = MG.make_config(kind, list(FLAGS[form]), d_model=64, heads=4, ffn=MSA.FFN)
        assert config.use_hyperformer and not config.use_adapter and config.add_adapter_cross_attn
        config.adapter_config = model_meta_config(config, args)
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
    return build_model


def hyper_modules(model):
    from adapters import TaskEmbeddingController, AdapterLayersHyperNetController, AdapterLayersOneHyperNetController
    return [m for m in model.modules() if isinstance(m, (TaskEmbeddingController, AdapterLayersHyperNetController,
                                                         AdapterLayersOneHyperNetController))]


_randomize = MG.randomize


def make_randomize(kind):
    def randomize(module, gen, std=0.05):
        """make_goldens.randomize, then the hyper-network rescaled so that it is alive (module docstring; the adapter generators' weights
        x 4 as well)"""
        _randomize(module, gen, std)
        with torch.no_grad():
            for n, p in module.named_parameters():
                if "adapter_layers_hyper_net" in n:
                    if n.endswith("LayerNorm.weight"):
                        p.add_(1.0)
                    elif "layer_id_embeddings" in n or "adapters_block_type" in n:
                        p.mul_(SCALE[kind])
                    elif "sampler_hyper_net" in n and n.endswith("weight"):
                        p.mul_(GEN_SCALE[kind])
                elif "task_to_embeddings" in n:
                    p.mul_(TASK_SCALE[kind])
                elif kind == "t5" and n in ("encoder.final_layer_norm.weight", "decoder.final_layer_norm.weight"):
                    p.add_(1.0)
    return randomize


def set_trainable(model):
    """make_single_adapter_goldens.set_trainable plus trainer_base.py:401-405: the task embeddings and both hyper-network controllers"""
    MSA_set_trainable(model)
    for m in hyper_modules(model):
        for p in m.parameters():
            p.requires_grad = True


MSA_set_trainable = MSA.set_trainable


def assert_alive(kind, form, name):
    """the three conditions on a model fixture: (i) another task moves the eval logits by >= 10 x TOL, (ii) zeroed adapter generators
    do, (iii) no hyper-network parameter of a task in the batches has a zero gradient after the training steps' first backward"""
    z = np.load(os.path.join(HERE, name + STEPS + ".npz"), allow_pickle=False)
    model, _ = MSA.build_reference(name, kind=kind)

    def logits(task):
        vis = tuple(torch.from_numpy(z[f"b0::vis{j}"]) for j in range(2))
        lab = torch.from_numpy(z["b0::labels"])
        with torch.no_grad():
            return model(input_ids=torch.from_numpy(z["b0::ids"]), vis_inputs=vis, labels=lab, return_dict=True, task=task)["logits"]
    base = logits(str(z["b0::task"]))
    assert float((base - torch.from_numpy(z["b0::logits"])).abs().max()) < 1e-5
    swap = float((logits("caption") - base).abs().max())
    model.train()
    for p in model.parameters():
        p.requires_grad = True
    used = set()
    for i in range(3):
        task = str(z[f"b{i}::task"])
        used.add(task)
        vis = tuple(torch.from_numpy(z[f"b{i}::vis{j}"]) for j in range(4 if task == "nlvr" else 2))
        out = model(input_ids=torch.from_numpy(z[f"b{i}::ids"]), vis_inputs=vis, labels=torch.from_numpy(z[f"b{i}::labels"]),
                    return_dict=True, task=task)
        out["loss"].sum().backward()
    seen = set()
    for m in hyper_modules(model):
        for n, p in m.named_parameters():
            if id(p) in seen or ("task_to_embeddings" in n and n.rsplit(".", 1)[1] not in used):
                continue
            seen.add(id(p))
            assert p.grad is not None and float(p.grad.abs().max()) > 0, n
    model.eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "sampler_hyper_net" in n:
                p.zero_()
    zeroed = float((logits(str(z["b0::task"])) - base).abs().max())
    print(f"  {name}: task swap moves the logits by {swap:.3e}, zeroed generators by {zeroed:.3e} (needed: {10 * TOL:.0e})")
    assert swap >= 10 * TOL and zeroed >= 10 * TOL, (swap, zeroed)


def golden_model(kind, form, seed):
    name = NAMES[(kind, form)]
    # make_prompt_goldens.golden_model: make_single_adapter_goldens' with per-parameter AdamW step counts -- a task embedding gets a
    # gradient only in its own task's steps, and transformers.AdamW skips a parameter without one (no decay, no moments, no count)
    MSA.build_model = MP.build_model = make_build_model(form)
    MP.NAMES = {kind: name}
    MP.set_trainable = set_trainable
    MG.randomize = make_randomize(kind)
    try:
        MP.golden_model(kind, seed)
    finally:
        MG.randomize = _randomize
    path = os.path.join(HERE, name + ".npz")
    z = dict(np.load(path, allow_pickle=False))
    # (the shared TaskEmbeddingController sits in the state dict three times -- the model's, the encoder's, the decoder's -- and stays so)
    model, _ = MSA.build_model(kind, seed)
    set_trainable(model)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert sorted(names) == sorted(k[7:] for k in z if k.startswith("final::"))
    z["names::trainable"] = np.array(names)
    # two files, each below 1 MiB: the state dict, and everything recorded from running it
    steps = path[:-4] + STEPS + ".npz"
    np.savez_compressed(path, **{k: v for k, v in z.items() if k.startswith("sd::")})
    np.savez_compressed(steps, **{k: v for k, v in z.items() if not k.startswith("sd::")})
    for f in (path, steps):
        print(f"  {os.path.basename(f)}: {os.path.getsize(f) / 1024:.0f} KiB")
        assert os.path.getsize(f) < (1 << 20)
    assert_alive(kind, form, name)


def main():
    MG.install_shim()
    which = sys.argv[1:] or ["controllers", "models", "generate"]
    if "controllers" in which:
        golden_controller("unique", 41)
        golden_controller("one", 42)
    if "models" in which:
        golden_model("bart", "unique", 51)
        golden_model("bart", "one", 53)
    if "t5" in which or not sys.argv[1:]:
        golden_model("t5", "unique", 52)
    if "generate" in which:
        os.makedirs(os.path.join(HERE, SUB), exist_ok=True)
        MSA.build_model = make_build_model("unique")
        MGG.build_reference = MSA.build_reference
        MGG.make_inputs = MSA.make_inputs
        MGG.case(SUB + "/gen_vlbart_hyperformer", NAMES[("bart", "unique")], "vqa", max_length=12, min_length=4, ngram=2, seed0=1500, mixed=False)
        # the beam fixture is T5's: under the BART fixture's parameters the tiny decoder's step distribution hardly depends on the history,
        # so sums of the same step scores in another order tie exactly and make_beam_goldens.case finds no seed with a margin; the T5
        # fixture (final norms at unit scale) has margins of 1e-2
        MGG.case(SUB + "/gen_vlt5_hyperformer", NAMES[("t5", "unique")], "vqa", max_length=12, min_length=4, ngram=2, kind="t5", seed0=1800,
                 mixed=False)
        # (make_beam_goldens sharpens T5's logits 1000-fold because its fixtures' final norm weighs ~ 0.05; here it weighs ~ 1)
        saved, MBG.LOGIT_SCALE = MBG.LOGIT_SCALE, dict(MBG.LOGIT_SCALE, t5=50.0)
        try:
            MBG.case(SUB + "/beam_vlt5_hyperformer", NAMES[("t5", "unique")], "caption", K=3, max_length=10, min_length=3, ngram=2,
                     kind="t5", seed0=1700)
        finally:
            MBG.LOGIT_SCALE = saved


if __name__ == "__main__":
    main()
