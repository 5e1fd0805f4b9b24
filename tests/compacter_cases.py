"""Shared by the Compacter tests (CPU and GPU legs): the host models of the fixtures captured from the reference's own classes with the
flag set of scripts/image-text/single_compacter.sh, and with param.py's defaults (shared rule, factorized W)
(tests/golden/make_compacter_goldens.py); geometry and loaders are single_adapter_cases'."""
import functools
import os

import numpy as np
import torch

import single_adapter_cases as SA

G = SA.G
NAMES = {"bart": "vlbart_tiny_compacter_d64", "t5": "vlt5_tiny_compacter_d64", "shared_fac": "vlbart_tiny_compacter_shared_fac_d64"}
KIND = {"bart": "bart", "t5": "t5", "shared_fac": "bart"}          # which host a fixture belongs to
# single_compacter.sh: --use_compacter --hypercomplex_division 2 --shared_phm_rule False --factorized_phm False --reduction_factor 8
#                      --use_single_adapter --unfreeze_layer_norms
SCRIPT = dict(SA.FLAGS, use_adapter=False, use_compacter=True, hypercomplex_division=2, shared_phm_rule=False, factorized_phm=False)
# the same without the three PHM flags: param.py's defaults (division 4, one rule for the model, factorized W of rank 1)
DEFAULTS = dict(SA.FLAGS, use_adapter=False, use_compacter=True)
FLAGS = {"bart": SCRIPT, "t5": SCRIPT, "shared_fac": DEFAULTS}


@functools.lru_cache(maxsize=None)
def fixture(which):
    """(state dict, batches, training losses, hyper-parameters, final trainable parameters) -- test_host_golden._load's tuple"""
    from test_host_golden import _load
    sd, *rest = _load(NAMES[which])
    shared = "model.shared.weight" if KIND[which] == "bart" else "shared.weight"
    prefix = shared[:-len("shared.weight")]
    for stack in ("encoder", "decoder"):            # (the aliases of the shared embedding, left out of the file: single_adapter_cases.fixture)
        sd.setdefault(f"{prefix}{stack}.embed_tokens.weight", sd[shared])
    return (sd, *rest)


@functools.lru_cache(maxsize=None)
def trainable_names(which):
    z = np.load(os.path.join(G, NAMES[which] + ".npz"), allow_pickle=False)
    return [str(n) for n in z["names::trainable"]]


def config(which, dropout=0.0, **over):
    flags = {**FLAGS[which], **over}
    if KIND[which] == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.vlt5_config(**{**SA.T5_GEOMETRY, **SA.T5_OFF, **flags, "dropout_rate": dropout})
    import vlpet_amd.host.bart as HB
    return HB.vlpet_config(**{**SA.BART_GEOMETRY, "dropout": dropout, "attention_dropout": dropout, "activation_dropout": dropout, **flags})


def new_model(which, dropout=0.0, **over):
    cfg = config(which, dropout, **over)
    if KIND[which] == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.VLT5(cfg), cfg
    import vlpet_amd.host.bart as HB
    return HB.VLBart(cfg), cfg


def build(which, dropout=0.0, **over):
    """(model with the fixture's weights, config, trainable names, keys of the fixture the host does not have)"""
    import vlpet_amd.train as TR
    model, cfg = new_model(which, dropout, **over)
    missing, unexpected = model.load_state_dict(fixture(which)[0], strict=False)
    assert not missing, missing
    return model, cfg, TR.trainable_names(model, cfg), unexpected


def phm_layers(model):
    from vlpet_amd.adapters import PHMLinear
    return [(n, m) for n, m in model.named_modules() if isinstance(m, PHMLinear)]


def adapters(model):
    from vlpet_amd.adapters import HyperComplexAdapter
    seen, out = set(), []
    for m in model.modules():
        if isinstance(m, HyperComplexAdapter) and id(m) not in seen:
            seen.add(id(m))
            out.append(m)
    return out


def _npz(name):
    return np.load(os.path.join(G, "compacter", name + ".npz"), allow_pickle=False)


def load_gen():
    z = _npz("gen_vlbart_compacter")
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length,
                ngram=ngram, eos=eos, pad=pad, start=start)


def load_beam():
    z = _npz("beam_vlbart_compacter")
    K, lp, early, max_length, min_length, ngram, eos, pad, start = z["settings"].tolist()
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), scores=torch.from_numpy(z["scores"]), K=int(K), lp=float(lp), early=bool(early),
                max_length=int(max_length), min_length=int(min_length), ngram=int(ngram), eos=int(eos), pad=int(pad), start=int(start),
                logit_scale=float(z["logit_scale"]), fixture=NAMES["bart"])


sharpen = SA.sharpen
