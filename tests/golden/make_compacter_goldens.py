#!/usr/bin/env python3
"""Generate the Compacter fixtures from the reference's OWN classes (run where the reference checkout is, next to make_goldens.py):

    python tests/golden/make_compacter_goldens.py

Flag set = scripts/image-text/single_compacter.sh: ``--use_compacter --hypercomplex_division 2 --shared_phm_rule False --factorized_phm
False --reduction_factor 8 --use_single_adapter --unfreeze_layer_norms`` (one shared PHM adapter of width d / 8 behind every attention and
feed-forward block of encoder and decoder; every LayerNorm trains).  Written, with the tiny geometry of make_single_adapter_goldens.py:

  vlbart_tiny_compacter_d64.npz, vlt5_tiny_compacter_d64.npz      layout of vlbart_tiny_single_adapter_d64.npz (``sd::``, ``b{i}::``,
      ``train::``, ``final::``) plus ``names::trainable`` (the trainable names, in ``named_parameters`` order)
  vlbart_tiny_compacter_shared_fac_d64.npz                        the flag defaults of param.py instead: division 4, one rule shared by
      the whole model (in ``sd::`` under the model's name AND under every PHMLinear's, as the reference registers it), factorized W, rank 1
  compacter/gen_vlbart_compacter.npz, compacter/beam_vlbart_compacter.npz      layouts of make_generate_goldens.case / make_beam_goldens.case
  phm_linear_{in}x{out}_n{n}.npz     the reference's PHMLinear alone: parameters, ``x``, ``y``, the upstream gradient ``dy`` and every
      gradient (``d_<name>``); (64, 8, 2), (8, 64, 4) and a factorized (12, 6, 3) of rank 2

The helpers are make_goldens' / make_single_adapter_goldens' / make_generate_goldens' / make_beam_goldens', imported; the adapter config
mirrors TrainerBase.create_config for ``--use_compacter`` (trainer_base.py:136-178: the reference's CompactorConfig)."""
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

COMMON = ["--tasks", "vqa,gqa,nlvr,caption", "--use_compacter", "--unfreeze_layer_norms", "--reduction_factor", "8", "--use_single_adapter",
          "--downsample", "--n_boxes", "36"]
SCRIPT = COMMON + ["--hypercomplex_division", "2", "--shared_phm_rule", "False", "--factorized_phm", "False"]
DEFAULTS = COMMON                  # param.py:163-170: division 4, shared rule, factorized W, rank 1
NAMES = {"bart": "vlbart_tiny_compacter_d64", "t5": "vlt5_tiny_compacter_d64"}
SHARED_FAC = "vlbart_tiny_compacter_shared_fac_d64"
SUB = "compacter"


def compactor_config(config, args):
    """trainer_base.py:136-178 for --use_compacter"""
    import re
    from adapters.config import CompactorConfig
    ac = CompactorConfig()
    ac.tasks = re.split("[, ]+", args.tasks)
    ac.input_dim = config.d_model
    ac.d_model = config.d_model
    ac.use_single_adapter = args.use_single_adapter
    ac.hypercomplex_division = args.hypercomplex_division
    ac.phm_rank = args.phm_rank
    ac.shared_phm_rule = args.shared_phm_rule
    ac.factorized_phm = args.factorized_phm
    ac.low_rank_rank = args.low_rank_rank
    ac.phm_init_range = args.phm_init_range
    ac.share_down_sampler = args.share_down_sampler
    ac.share_up_sampler = args.share_up_sampler
    ac.reduction_factor = args.reduction_factor
    ac.shared_phm_rule_over_tasks = args.shared_phm_rule_over_tasks
    ac.add_layer_norm_before_adapter = args.add_layer_norm_before_adapter
    ac.add_layer_norm_after_adapter = args.add_layer_norm_after_adapter
    ac.track_z = args.track_z
    ac.use_adapter_down_dim = bool(args.use_adapter_down_dim)
    ac.adapter_down_dim = args.adapter_down_dim
    ac.use_parallel_adapter = False
    ac.use_scaling_factor = False
    ac.scaling_factor = 1.0
    return ac


def make_build_model(flags):
    def build_model(kind, seed=None):
        mod = MG.load_vl_module(kind)
        config, args = MG.make_config(kind, list(flags), d_model=64, heads=4, ffn=MSA.FFN)
        assert config.use_compacter and not config.use_adapter and not config.no_encoder_adapter and not config.no_decoder_adapter
        config.adapter_config = compactor_config(config, args)
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


_randomize = MG.randomize


def randomize(module, gen, std=0.05):
    """make_goldens.randomize, then every rule times 10: H is a product of a rule and a W entry, and with both at 0.05 the adapters
    would hardly move the logits"""
    _randomize(module, gen, std)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if "phm_rule" in n:
                p.mul_(10.0)


def golden_model(kind, seed, flags, name):
    """make_single_adapter_goldens.golden_model on the Compacter model, plus the list of trainable names"""
    MSA.build_model = make_build_model(flags)
    MSA.NAMES = {kind: name}
    MG.randomize = randomize
    try:
        MSA.golden_model(kind, seed)
    finally:
        MG.randomize = _randomize
    path = os.path.join(HERE, name + ".npz")
    z = dict(np.load(path, allow_pickle=False))
    model, _ = MSA.build_model(kind, seed)
    MSA.set_trainable(model)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert sorted(names) == sorted(k[7:] for k in z if k.startswith("final::"))
    z["names::trainable"] = np.array(names)
    np.savez_compressed(path, **z)
    print(f"  + names::trainable ({len(names)})  ({os.path.getsize(path) / 1024:.0f} KiB)")


def golden_phm_linear(in_f, out_f, n, factorized=False, rank=1, seed=0, rows=5):
    MG.install_shim()
    from adapters.hypercomplex.layers import PHMLinear
    torch.manual_seed(seed)
    layer = PHMLinear(in_features=in_f, out_features=out_f, phm_dim=n, bias=True, w_init="glorot-uniform", c_init="normal",
                      learn_phm=True, factorized_phm=factorized, phm_rank=rank, phm_init_range=0.01)
    gen = torch.Generator().manual_seed(seed)
    _randomize(layer, gen, std=0.5)
    x = torch.randn(rows, in_f, generator=gen, requires_grad=True)
    dy = torch.randn(rows, out_f, generator=gen)
    y = layer(x)
    (y * dy).sum().backward()
    arrs = {"x": MG.T(x), "y": MG.T(y), "dy": dy, "d_x": MG.T(x.grad), "n": np.array(n), "rank": np.array(rank if factorized else 0)}
    for k, p in layer.named_parameters():
        arrs[k] = MG.T(p)
        arrs["d_" + k] = MG.T(p.grad)
    MG.save(f"phm_linear_{in_f}x{out_f}_n{n}", **arrs)


def main():
    MG.install_shim()
    which = sys.argv[1:] or ["layers", "models", "generate"]
    if "layers" in which:
        golden_phm_linear(64, 8, 2, seed=31)
        golden_phm_linear(8, 64, 4, seed=32)
        golden_phm_linear(12, 6, 3, factorized=True, rank=2, seed=33)
    if "models" in which:
        golden_model("bart", 24, SCRIPT, NAMES["bart"])
        golden_model("t5", 25, SCRIPT, NAMES["t5"])
        golden_model("bart", 26, DEFAULTS, SHARED_FAC)
    if "generate" in which:
        os.makedirs(os.path.join(HERE, SUB), exist_ok=True)
        MSA.build_model = make_build_model(SCRIPT)
        MGG.build_reference = MSA.build_reference
        MGG.make_inputs = MSA.make_inputs
        # (n-gram ban and minimum length as in make_single_adapter_goldens: the tiny model, left alone, repeats one token)
        MGG.case(SUB + "/gen_vlbart_compacter", NAMES["bart"], "vqa", max_length=12, min_length=4, ngram=2, seed0=1300, mixed=False)
        MBG.case(SUB + "/beam_vlbart_compacter", NAMES["bart"], "caption", K=4, max_length=12, min_length=4, ngram=2, seed0=1400)


if __name__ == "__main__":
    main()
