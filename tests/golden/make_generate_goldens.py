#!/usr/bin/env python3
"""Generate tests/golden/gen_*.npz: greedy generation of the reference's own tiny VLBart / LoRA VLBart / VLT5 / video VLBart.

Run in the build container only, next to make_goldens.py (it needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_generate_goldens.py

The models are the ones of make_goldens.golden_vlbart_tiny, built from the reference's classes through that script's import shim,
with the weights of the existing vlbart_tiny*_d64.npz / vlt5_tiny_d64.npz fixtures (loaded from there, not copied into the new
files).  Decoding is HF 4.2.1 greedy_search restated without a cache: at every step the reference model's forward runs on the whole
``decoder_input_ids`` (fp32, CPU), the installed transformers' MinLengthLogitsProcessor / NoRepeatNGramLogitsProcessor act on the last
position's logits, the argmax is the next token, finished rows emit pad, the loop stops when every row has finished.  Stored: the
inputs, the generation settings, the token ids and every step's raw last-position logits.  Each case's seed is the first one whose
every step has a top-2 margin of at least 1e-4 on every unfinished row (asserted), and its eos is a token that some rows emit early
and others not at all, so that finishing and padding are exercised."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402

MARGIN = 1e-4
B = 4


def build_reference(name, lora=False, kind="bart", video=False):
    """make_goldens.golden_vlbart_tiny's model, weights from ``name``.npz"""
    mod = MG.load_vl_module(kind)
    if lora:
        flags = list(MG.LORA_FLAGS) + ["--downsample", "--n_boxes", "36"]
    else:
        base = MG.VLPET_LARGE_FLAGS if kind == "bart" else MG.T5_VLPET_FLAGS
        flags = list(base) + ["--adapter_down_dim", "8", "--encoder_adapter_multihead_num_head", "4",
                              "--adapter_gating_down_dim", "16", "--decoder_enc_attn_value_parallel_adapter_down_dim", "8",
                              "--downsample", "--n_boxes", "64" if video else "36"]
        if video:
            flags[flags.index("--tasks") + 1] = "tvqa,how2qa,tvc,yc2c"
    config, _ = MG.make_config(kind, flags, d_model=64, heads=4, ffn=128)
    if kind == "t5":
        MG.install_t5_runtime_shim()
        config.decoder_start_token_id = 0
        config.pad_token_id = 0
    if lora:
        config.lora_config.lora_dropout = 0.0
    config.vocab_size = 500
    config.feat_dim = 128
    config.default_obj_order_ids = list(range(400, 500))
    config.encoder_prompt_config = None
    config.decoder_prompt_config = None
    from transformers import PreTrainedModel
    PreTrainedModel.init_weights = lambda self: self.apply(self._init_weights)
    torch.manual_seed(0)
    model = mod.VLBart(config) if kind == "bart" else mod.VLT5(config)
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("lm_head" in k or "embed_tokens" in k for k in missing), missing
    model.lm_head.weight = model.model.shared.weight if kind == "bart" else model.shared.weight
    if kind == "bart":
        model.model.encoder.embed_tokens = model.model.shared
        model.model.decoder.embed_tokens = model.model.shared
    model.eval()
    return model, config


def greedy(model, ids, vis, task, start, eos, pad, max_length, min_length, ngram):
    from transformers import MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor
    procs = []
    if ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    if eos is not None and min_length > 0:
        procs.append(MinLengthLogitsProcessor(min_length, eos))
    dec = torch.full((ids.shape[0], 1), start, dtype=torch.long)
    unfinished = torch.ones(ids.shape[0], dtype=torch.long)
    steps, margins = [], []
    with torch.no_grad():
        while dec.shape[1] < max_length:
            out = model(input_ids=ids, vis_inputs=vis, decoder_input_ids=dec, task=task, return_dict=True)
            logits = out["logits"][:, -1, :].float()
            scores = logits
            for p in procs:
                scores = p(dec, scores)
            top = scores.topk(2, dim=-1).values
            margins.append(torch.where(unfinished.bool(), top[:, 0] - top[:, 1], torch.full_like(top[:, 0], float("inf"))))
            nxt = scores.argmax(-1)
            if eos is not None:
                nxt = nxt * unfinished + pad * (1 - unfinished)
            steps.append(logits)
            dec = torch.cat([dec, nxt[:, None]], 1)
            if eos is not None:
                unfinished = unfinished * (nxt != eos).long()
                if int(unfinished.max()) == 0:
                    break
    return dec, torch.stack(steps, 1), float(torch.stack(margins).min())


def make_inputs(gen, kind, video, L, pad):
    """One token and one feature vector repeated along each row: the tiny models' cross-attention averages nearly uniformly over the
    encoder positions, so rows of independent random tokens all decode alike; rows that differ as wholes do not."""
    ids = torch.randint(5, 300, (B, 1), generator=gen).expand(B, L).contiguous()
    n_vis = 64 if video else 49
    feats = torch.randn(B, 1, 128, generator=gen).expand(B, n_vis, 128).contiguous()
    vis = (feats, torch.rand(B, n_vis, 4, generator=gen))
    lens = (L, L - 9, L - 15, 7) if video else (L, L, L - 4, L)
    for i, n in enumerate(lens):
        ids[i, n:] = pad                          # padded rows: the cross-attention key mask matters
    return ids, vis


def case(tag, fixture, task, max_length, min_length=0, ngram=0, lora=False, kind="bart", video=False, L=12, seed0=100, mixed=True):
    """``mixed``: some rows must finish and some not (False: the model decodes every row alike -- the LoRA fixture, whose only
    trainable deltas start at zero, and the video fixture -- and only an early finish of all rows is asked for)"""
    model, config = build_reference(fixture, lora=lora, kind=kind, video=video)
    start, pad = int(config.decoder_start_token_id), int(config.pad_token_id)
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        ids, vis = make_inputs(gen, kind, video, L, pad)
        # eos: a token some rows emit early and some rows never emit (looked up on the run without an eos)
        free, _, _ = greedy(model, ids, vis, task, start, None, pad, max_length, 0, ngram)
        eos = None
        for t in free[:, 1:max_length - 1].reshape(-1).tolist():
            rows = [(free[r, 1:] == t).any().item() for r in range(B)]
            if t not in (pad, start) and 0 < sum(rows) and (sum(rows) < B or not mixed):
                eos = int(t)
                break
        if eos is None:
            continue
        out, logits, margin = greedy(model, ids, vis, task, start, eos, pad, max_length, min_length, ngram)
        finished = [(out[r, 1:] == eos).any().item() for r in range(B)]
        if margin < MARGIN or not any(finished) or (mixed and all(finished)):
            continue
        print(f"{tag}: seed {seed} eos {eos} length {out.shape[1]} margin {margin:.3g}")
        print(out.tolist())
        MG.save(tag, ids=ids.numpy(), vis0=vis[0].numpy(), vis1=vis[1].numpy(), task=np.array(task), fixture=np.array(fixture),
                settings=np.array([max_length, min_length, ngram, eos, pad, start]), out=out.numpy(), logits=logits.numpy(),
                margin=np.array(margin))
        return
    raise AssertionError(f"{tag}: no seed with a top-2 margin >= {MARGIN} and an early eos")


def main():
    MG.install_shim()
    torch.manual_seed(0)
    case("gen_vlbart_vqa", "vlbart_tiny_d64", "vqa", max_length=10)
    case("gen_vlbart_caption_minlen_ngram", "vlbart_tiny_d64", "caption", max_length=14, min_length=5, ngram=2, seed0=300)
    case("gen_vlbart_lora", "vlbart_tiny_lora_d64", "vqa", max_length=10, lora=True, seed0=500, mixed=False)
    case("gen_vlt5_vqa", "vlt5_tiny_d64", "vqa", max_length=10, kind="t5", seed0=700)
    case("gen_vlbart_video", "vlbart_tiny_video_d64", "tvqa", max_length=10, video=True, L=24, seed0=900, mixed=False)


if __name__ == "__main__":
    main()
