"""Shared by tests/test_hyperformer_host.py and tests/test_gpu_hyperformer.py: the host models of the fixtures captured from the
reference's own VLBart / VLT5 with the flag set of scripts/image-text/hyperformer.sh (``--unique_hyper_net``) and with
``--efficient_unique_hyper_net`` (tests/golden/make_hyperformer_goldens.py).  Each fixture is two files: ``<name>.npz`` (``sd::``) and
``<name>_steps.npz`` (batches, ``train::``, ``final::``, ``names::trainable``).  Geometry and loaders are single_adapter_cases'."""
import functools
import os

import numpy as np
import torch

import single_adapter_cases as SA

G = SA.G
NAMES = {"unique": "vlbart_tiny_hyperformer_d64", "one": "vlbart_tiny_hyperformer_one_d64", "t5": "vlt5_tiny_hyperformer_d64"}
WHICH = list(NAMES)
KIND = {"unique": "bart", "one": "bart", "t5": "t5"}          # which host a fixture belongs to
COMMON = dict(SA.FLAGS, use_adapter=False, use_hyperformer=True, projected_task_embedding_dim=8)
FLAGS = {"unique": dict(COMMON, unique_hyper_net=True), "one": dict(COMMON, efficient_unique_hyper_net=True),
         "t5": dict(COMMON, unique_hyper_net=True)}
TASK_DIM = 64       # the fixtures' task_embedding_dim (the class default 512 would put the files above 1 MiB)


@functools.lru_cache(maxsize=None)
def fixture(which):
    """(state dict, batches, training losses, hyper-parameters, final trainable parameters) -- test_host_golden._load's tuple"""
    z = dict(np.load(os.path.join(G, NAMES[which] + ".npz"), allow_pickle=False))
    z.update(np.load(os.path.join(G, NAMES[which] + "_steps.npz"), allow_pickle=False))
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z if k.startswith("sd::")}
    prefix = "model." if KIND[which] == "bart" else ""
    for stack in ("encoder", "decoder"):            # (the aliases of the shared embedding, left out of the file)
        sd.setdefault(f"{prefix}{stack}.embed_tokens.weight", sd[prefix + "shared.weight"])
    batches = []
    for i in range(3):
        vis = tuple(torch.from_numpy(z[f"b{i}::vis{j}"]) for j in range(4) if f"b{i}::vis{j}" in z)
        batches.append(dict(task=str(z[f"b{i}::task"]), input_ids=torch.from_numpy(z[f"b{i}::ids"]),
                            labels=torch.from_numpy(z[f"b{i}::labels"]), scores=torch.from_numpy(z[f"b{i}::scores"]),
                            vis_inputs=vis, per_token=torch.from_numpy(z[f"b{i}::per_token"]),
                            logits=torch.from_numpy(z[f"b{i}::logits"]), loss=float(z[f"b{i}::loss"])))
    final = {k[7:]: torch.from_numpy(z[k]) for k in z if k.startswith("final::")}
    return sd, batches, z["train::losses"], z["train::hparams"], final


@functools.lru_cache(maxsize=None)
def trainable_names(which):
    z = np.load(os.path.join(G, NAMES[which] + "_steps.npz"), allow_pickle=False)
    return [str(n) for n in z["names::trainable"]]


def config(which, dropout=0.0, **over):
    if KIND[which] == "t5":
        import vlpet_amd.host.t5 as HT
        cfg = HT.vlt5_config(**{**SA.T5_GEOMETRY, **SA.T5_OFF, **FLAGS[which], "dropout_rate": dropout, **over})
    else:
        import vlpet_amd.host.bart as HB
        cfg = HB.vlpet_config(**{**SA.BART_GEOMETRY, "dropout": dropout, "attention_dropout": dropout, "activation_dropout": dropout,
                                 **FLAGS[which], **over})
    if cfg.adapter_config is not None and hasattr(cfg.adapter_config, "task_embedding_dim"):
        cfg.adapter_config.task_embedding_dim = TASK_DIM
    return cfg


def new_model(which, dropout=0.0, **over):
    cfg = config(which, dropout, **over)
    if KIND[which] == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.VLT5(cfg), cfg
    import vlpet_amd.host.bart as HB
    return HB.VLBart(cfg), cfg


def stacks(model):
    m = model.model if hasattr(model, "model") else model
    return m, m.encoder, m.decoder


def build(which, dropout=0.0, **over):
    """(model with the fixture's weights, config, trainable names, keys of the fixture the host does not have)"""
    import vlpet_amd.train as TR
    model, cfg = new_model(which, dropout, **over)
    missing, unexpected = model.load_state_dict(fixture(which)[0], strict=False)
    assert not missing, missing
    return model, cfg, TR.trainable_names(model, cfg), unexpected


def hyper_parameters(model):
    """(name, parameter) of the task embeddings and both stacks' hyper-networks, each once"""
    return [(n, p) for n, p in model.named_parameters() if "task_to_embeddings" in n or "adapter_layers_hyper_net" in n]


def load_gen(kind="bart"):
    z = np.load(os.path.join(G, "hyperformer", f"gen_vl{kind}_hyperformer.npz"), allow_pickle=False)
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length,
                ngram=ngram, eos=eos, pad=pad, start=start)


def load_beam():
    """the beam fixture is the T5 model's (tests/golden/make_hyperformer_goldens.py says why)"""
    z = np.load(os.path.join(G, "hyperformer", "beam_vlt5_hyperformer.npz"), allow_pickle=False)
    K, lp, early, max_length, min_length, ngram, eos, pad, start = z["settings"].tolist()
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), scores=torch.from_numpy(z["scores"]), K=int(K), lp=float(lp), early=bool(early),
                max_length=int(max_length), min_length=int(min_length), ngram=int(ngram), eos=int(eos), pad=int(pad), start=int(start),
                logit_scale=float(z["logit_scale"]), fixture=NAMES["t5"])


def sharpen_t5(model, scale):
    """make_beam_goldens.sharpen on the T5 host: the decoder's last norm (and so the logits) times ``scale``"""
    with torch.no_grad():
        model.decoder.final_layer_norm.weight.mul_(scale)
