"""Shared by the BitFit tests (CPU and GPU legs): the host models of the two fixtures captured from the reference's own classes with the
flag set of scripts/image-text/bitfit.sh (tests/golden/make_bitfit_goldens.py): ``--unfreeze_bias`` and no PET module of any kind."""
import functools
import os

import numpy as np
import torch

import single_adapter_cases as SA

G = os.path.join(os.path.dirname(__file__), "golden")
NAMES = {"bart": "vlbart_tiny_bitfit_d64", "t5": "vlt5_tiny_bitfit_d64"}
TASKS = ("vqa", "gqa", "nlvr", "caption")
OFF = dict(use_adapter=False, use_single_adapter=False, no_encoder_adapter=False, no_decoder_adapter=False, unfreeze_layer_norms=False,
           use_adapter_down_dim=False, use_encoder_adapter_down_multihead=False, use_encoder_adapter_gating_large_x_lowrank=False,
           use_decoder_enc_attn_value_parallel_adapter_down_dim=False, unfreeze_encoder_layer_norms=False)
BITFIT = dict(unfreeze_bias=True)


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


@functools.lru_cache(maxsize=None)
def reference_names(kind):
    """the reference's trainable names, in named_parameters() order"""
    z = np.load(os.path.join(G, NAMES[kind] + ".npz"), allow_pickle=False)
    return [str(n) for n in z["train::names"]]


def config(kind, dropout=0.0, bitfit=True, **over):
    flags = {**OFF, **(BITFIT if bitfit else {})}
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


def load_gen():
    z = np.load(os.path.join(G, "bitfit", "gen_vlbart_bitfit.npz"), allow_pickle=False)
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length,
                ngram=ngram, eos=eos, pad=pad, start=start)


def load_trained(model, kind="bart"):
    """overlay the fixture's final trainable parameters: the state the generation fixture was captured from"""
    final = fixture(kind)[4]
    cur = dict(model.named_parameters())
    with torch.no_grad():
        for n, v in final.items():
            cur[n].copy_(v.to(cur[n].device, cur[n].dtype))
    return model
