"""Shared by the Single-Adapter tests (CPU and GPU legs): the host models of the two fixtures captured from the reference's own classes
with the flag set of scripts/image-text/single_adapter.sh (tests/golden/make_single_adapter_goldens.py), built once per process."""
import functools
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
NAMES = {"bart": "vlbart_tiny_single_adapter_d64", "t5": "vlt5_tiny_single_adapter_d64"}
# single_adapter.sh: --use_adapter --unfreeze_layer_norms --reduction_factor 8 --use_single_adapter (nothing of VL-PET's own)
FLAGS = dict(use_adapter=True, use_single_adapter=True, no_encoder_adapter=False, no_decoder_adapter=False, unfreeze_layer_norms=True,
             use_adapter_down_dim=False, reduction_factor=8, use_encoder_adapter_down_multihead=False,
             use_encoder_adapter_gating_large_x_lowrank=False, use_decoder_enc_attn_value_parallel_adapter_down_dim=False,
             unfreeze_encoder_layer_norms=False)
BART_GEOMETRY = dict(d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4,
                     encoder_ffn_dim=32, decoder_ffn_dim=32, vocab_size=240, max_position_embeddings=40, feat_dim=64)
T5_GEOMETRY = dict(d_model=64, d_kv=16, d_ff=32, num_layers=2, num_decoder_layers=2, num_heads=4, vocab_size=240, feat_dim=64)
T5_OFF = dict(use_encoder_gating_scaling=False, use_encoder_multihead_up_zero_init=False,
              use_encoder_gating_large_x_lowrank_up_zero_init=False, use_decoder_enc_vpa_up_zero_init=False)


@functools.lru_cache(maxsize=None)
def fixture(kind):
    """(state dict, batches, training losses, hyper-parameters, final trainable parameters) -- test_host_golden._load's tuple"""
    from test_host_golden import _load
    sd, *rest = _load(NAMES[kind])
    # the fixture stores the shared embedding once: its aliases in the reference's state dict (the same tensor under the stacks'
    # ``embed_tokens``; the generator's tie()) are put back here
    shared = "model.shared.weight" if kind == "bart" else "shared.weight"
    prefix = shared[:-len("shared.weight")]
    for stack in ("encoder", "decoder"):
        sd.setdefault(f"{prefix}{stack}.embed_tokens.weight", sd[shared])
    return (sd, *rest)


def config(kind, dropout=0.0, **over):
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        return HT.vlt5_config(**{**T5_GEOMETRY, **FLAGS, **T5_OFF, "dropout_rate": dropout, **over})
    import vlpet_amd.host.bart as HB
    return HB.vlpet_config(**{**BART_GEOMETRY, **FLAGS, "dropout": dropout, "attention_dropout": dropout, "activation_dropout": dropout,
                              **over})


def build(kind, dropout=0.0, **over):
    """(model with the fixture's weights, config, trainable names); asserts that no host key is missing from the reference's state dict"""
    import vlpet_amd.train as TR
    cfg = config(kind, dropout, **over)
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        model = HT.VLT5(cfg)
    else:
        import vlpet_amd.host.bart as HB
        model = HB.VLBart(cfg)
    missing, unexpected = model.load_state_dict(fixture(kind)[0], strict=False)
    assert not missing, missing
    return model, cfg, TR.trainable_names(model, cfg), unexpected


def load_npz(name):
    return np.load(os.path.join(G, "single_adapter", name + ".npz"), allow_pickle=False)


def load_gen():
    z = load_npz("gen_vlbart_single_adapter")
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length,
                ngram=ngram, eos=eos, pad=pad, start=start)


def load_beam():
    z = load_npz("beam_vlbart_single_adapter")
    K, lp, early, max_length, min_length, ngram, eos, pad, start = z["settings"].tolist()
    return dict(task=str(z["task"]), ids=torch.from_numpy(z["ids"]), vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])),
                out=torch.from_numpy(z["out"]), scores=torch.from_numpy(z["scores"]), K=int(K), lp=float(lp), early=bool(early),
                max_length=int(max_length), min_length=int(min_length), ngram=int(ngram), eos=int(eos), pad=int(pad), start=int(start),
                logit_scale=float(z["logit_scale"]), fixture=NAMES["bart"])


def sharpen(model, scale):
    """make_beam_goldens.sharpen on the BART host: the decoder's last norm (and so the logits) times ``scale``"""
    with torch.no_grad():
        ln = model.model.decoder.layers[-1].final_layer_norm
        ln.weight.mul_(scale)
        ln.bias.mul_(scale)
