"""Shared by the prompt-tuning tests (CPU and GPU legs): the host models of the two fixtures captured from the reference's own classes
with the flag set of scripts/image-text/single_prompt.sh at P = 5, mid_dim = 24 (tests/golden/make_prompt_goldens.py).  BART: one prompt
shared by the tasks (--use_single_prompt); T5: one per task."""
import functools
import os

import numpy as np
import torch

import single_adapter_cases as SA

G = os.path.join(os.path.dirname(__file__), "golden")
NAMES = {"bart": "vlbart_tiny_prompt_d64", "t5": "vlt5_tiny_prompt_d64"}
P, MID = 5, 24
TASKS = ("vqa", "gqa", "nlvr", "caption")
# single_prompt.sh: --encoder_prompt_len --mid_dim --use_single_prompt and no adapter flag of any kind
OFF = dict(use_adapter=False, use_single_adapter=False, no_encoder_adapter=False, no_decoder_adapter=False, unfreeze_layer_norms=False,
           use_adapter_down_dim=False, use_encoder_adapter_down_multihead=False, use_encoder_adapter_gating_large_x_lowrank=False,
           use_decoder_enc_attn_value_parallel_adapter_down_dim=False, unfreeze_encoder_layer_norms=False)
PROMPT = {"bart": dict(encoder_prompt_len=P, mid_dim=MID, use_single_prompt=True),
          "t5": dict(encoder_prompt_len=P, mid_dim=MID, use_single_prompt=False)}


@functools.lru_cache(maxsize=None)
def fixture(kind):
    """(state dict, batches, training losses, hyper-parameters, final trainable parameters) -- test_host_golden._load's tuple, with the
    aliases of the shared embedding the generator leaves out put back (single_adapter_cases.fixture)"""
    from test_host_golden import _load
    sd, *rest = _load(NAMES[kind])
    shared = "model.shared.weight" if kind == "bart" else "shared.weight"
    prefix = shared[:-len("shared.weight")]
    for stack in ("encoder", "decoder"):
        sd.setdefault(f"{prefix}{stack}.embed_tokens.weight", sd[shared])
    return (sd, *rest)


def config(kind, dropout=0.0, prompt=True, **over):
    flags = {**OFF, **(PROMPT[kind] if prompt else {})}
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.vlt5_config(**{**SA.T5_GEOMETRY, **flags, **SA.T5_OFF, "dropout_rate": dropout, **over})
    import vlpet_amd.host.bart as HB
    return HB.vlpet_config(**{**SA.BART_GEOMETRY, **flags, "dropout": dropout, "attention_dropout": dropout,
                              "activation_dropout": dropout, **over})


def new_model(kind, cfg):
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.VLT5(cfg)
    import vlpet_amd.host.bart as HB
    return HB.VLBart(cfg)


def build(kind, dropout=0.0, **over):
    """(model with the fixture's weights, config, trainable names, unexpected keys); no host key may be missing from the fixture"""
    import vlpet_amd.train as TR
    cfg = config(kind, dropout, **over)
    model = new_model(kind, cfg)
    missing, unexpected = model.load_state_dict(fixture(kind)[0], strict=False)
    assert not missing, missing
    return model, cfg, TR.trainable_names(model, cfg), unexpected


def encoder(model, kind):
    return model.model.encoder if kind == "bart" else model.encoder


def _npz(name):
    return np.load(os.path.join(G, "prompt", name + ".npz"), allow_pickle=False)


def load_gen():
    z = _npz("gen_vlbart_prompt")
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length,
                ngram=ngram, eos=eos, pad=pad, start=start)


def load_beam():
    z = _npz("beam_vlbart_prompt")
    K, lp, early, max_length, min_length, ngram, eos, pad, start = z["settings"].tolist()
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), scores=torch.from_numpy(z["scores"]), K=int(K), lp=float(lp), early=bool(early),
                max_length=int(max_length), min_length=int(min_length), ngram=int(ngram), eos=int(eos), pad=int(pad), start=int(start),
                logit_scale=float(z["logit_scale"]), fixture=NAMES["bart"])


sharpen = SA.sharpen
