#!/usr/bin/env python3
"""Generate tests/golden/beam_*.npz: beam search (HF 4.2.1, num_return_sequences = 1) of the reference's own tiny VLBart / LoRA
VLBart / VLT5 / video VLBart.

Run in the build container only, next to make_generate_goldens.py (it needs the reference checkout, which never travels to the GPU
box):

    python tests/golden/make_beam_goldens.py

The models and inputs are make_generate_goldens' (build_reference / make_inputs).  Decoding has no cache: at every step the reference
model's forward runs on the whole ``decoder_input_ids`` of the B * K rows (fp32, CPU), with the encoder inputs expanded K times as the
reference's _expand_inputs_for_generation does; BART's logits pass the reference model's own adjust_logits_during_generation, then the
log-softmax, the installed transformers' NoRepeatNGramLogitsProcessor / MinLengthLogitsProcessor, and the scorer of
tests/beam_spec.py.  Stored: the inputs, the settings, the output ids, each item's chosen sequence score and every step's top 2K
(score, token, beam) per item.  Each case's seed is the first one whose every decision has a margin of at least 1e-4 (asserted):
the top 2K + 1 flat scores of every live item at every step, and the best against the second-best hypothesis at finalize.

The tiny models' logits are nearly flat (a spread of ~0.03 for BART, ~0.002 for T5), too flat for 2K + 1 ranks a margin apart.  So
every case multiplies the decoder's last norm (BART: the last layer's final_layer_norm weight and bias; T5: the decoder's
final_layer_norm weight) by ``logit_scale``, which scales the logits exactly, and stores the factor: the tests apply it to the host
model the same way (sharpen())."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG  # noqa: E402
import make_generate_goldens as MGG  # noqa: E402
import beam_spec as BS  # noqa: E402

MARGIN = 1e-4
LOGIT_SCALE = {"bart": 100.0, "t5": 1000.0}


def sharpen(model, kind, scale):
    """multiply the logits by ``scale``: the decoder's last norm (names shared by the reference models and host/)"""
    with torch.no_grad():
        if kind == "bart":
            ln = model.model.decoder.layers[-1].final_layer_norm
            ln.weight.mul_(scale)
            ln.bias.mul_(scale)
        else:
            model.decoder.final_layer_norm.weight.mul_(scale)


def run(model, kind, ids, vis, task, K, start, eos, pad, max_length, min_length, ngram, lp, early):
    from transformers import MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor
    procs = []
    if ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    if min_length > 0:
        procs.append(MinLengthLogitsProcessor(min_length, eos))
    B = ids.shape[0]
    ids_x = ids.repeat_interleave(K, 0)
    vis_x = tuple(v.repeat_interleave(K, 0) for v in vis)
    model.config.eos_token_id = eos           # adjust_logits_during_generation forces the config's eos
    if kind == "bart" and not hasattr(model.config, "force_bos_token_to_be_generated"):
        model.config.force_bos_token_to_be_generated = False       # BartConfig 4.2.1's default (the installed one lacks the key)

    def step_logits(dec):
        with torch.no_grad():
            out = model(input_ids=ids_x, vis_inputs=vis_x, decoder_input_ids=dec, task=task, return_dict=True)
        return out["logits"][:, -1, :].float().clone()

    def processed(dec, logits, cur_len):
        if kind == "bart":
            logits = model.adjust_logits_during_generation(logits, cur_len=cur_len, max_length=max_length)
        x = torch.log_softmax(logits, -1)
        for p in procs:
            x = p(dec, x)
        return x

    V = model.config.vocab_size
    return BS.beam_search(step_logits, V, B, K, start, eos, pad, max_length, length_penalty=lp, early_stopping=early,
                          processed=processed)


def margin_of(trace, hyps, K):
    m = BS.hyp_margin(hyps)
    for t in trace:
        v, _ = BS.top_flat(t["scores"], 2 * K + 1)
        for b, live in enumerate(t["live"]):
            if not live:
                continue
            f = v[b][torch.isfinite(v[b])].double()
            if f.numel() > 1:
                m = min(m, float((f[:-1] - f[1:]).min()))
    return m


def case(tag, fixture, task, K, max_length, lp=1.0, early=False, min_length=0, ngram=0, lora=False, kind="bart", video=False,
         L=12, seed0=100, want=()):
    """``want``: coverage the case must show -- "skip" (an eos of rank >= K skipped), "maxlen" (the loop reaches max_length with an
    open item: BART's forced eos and finalize's open beams).  (The tiny models decode the items of a batch alike, so items that
    finish at different steps are left to the kernel tests' planted tables.)"""
    model, config = MGG.build_reference(fixture, lora=lora, kind=kind, video=video)
    scale = LOGIT_SCALE[kind]
    sharpen(model, kind, scale)
    start, pad = int(config.decoder_start_token_id), int(config.pad_token_id)
    V = config.vocab_size
    for seed in range(seed0, seed0 + 300):
        gen = torch.Generator().manual_seed(seed)
        ids, vis = MGG.make_inputs(gen, kind, video, L, pad)
        # eos: a token the greedy free run emits after the first step (a few of them tried, the rarest first)
        free, _, _ = MGG.greedy(model, ids, vis, task, start, None, pad, max_length, 0, ngram)
        toks = [t for t in free[:, 2:max_length - 1].reshape(-1).tolist() if t not in (pad, start)]
        found = None
        for eos in sorted(set(toks), key=lambda t: (toks.count(t), t))[:4]:
            out, scores, trace, hyps = run(model, kind, ids, vis, task, K, start, eos, pad, max_length, min_length, ngram, lp,
                                           early)
            margin = margin_of(trace, hyps, K)
            done_at = [next((i for i, t in enumerate(trace) if not t["live"][b]), len(trace)) for b in range(ids.shape[0])]
            if margin < MARGIN:
                continue
            if "staggered" in want and len(set(done_at)) < 2:
                continue
            if "skip" in want and not any(t["skipped"] for t in trace):
                continue
            if "maxlen" in want and not (len(trace) == max_length - 1 and trace[-1]["live"].count(True) > 0):
                continue
            found = eos
            break
        if found is None:
            continue
        print(f"{tag}: seed {seed} eos {eos} width {out.shape[1]} steps {len(trace)} done at {done_at} margin {margin:.3g}")
        print(out.tolist(), scores.tolist())
        top_s = torch.stack([t["top_v"] for t in trace], 1).numpy()                # [B, steps, 2K]
        flat = torch.stack([t["top_i"] for t in trace], 1)
        live = np.array([t["live"] for t in trace], dtype=np.uint8).T              # [B, steps]
        MG.save(tag, ids=ids.numpy(), vis0=vis[0].numpy(), vis1=vis[1].numpy(), task=np.array(task), fixture=np.array(fixture),
                settings=np.array([K, lp, float(early), max_length, min_length, ngram, eos, pad, start], dtype=np.float64),
                out=out.numpy(), scores=scores.numpy(), top_score=top_s, top_token=(flat % V).numpy().astype(np.int32),
                top_beam=(flat // V).numpy().astype(np.int32), live=live, steps=np.array(len(trace)), margin=np.array(margin),
                logit_scale=np.array(scale))
        return
    raise AssertionError(f"{tag}: no seed with margins >= {MARGIN} and {want}")


def main():
    MG.install_shim()
    torch.manual_seed(0)
    case("beam_vlbart_vqa", "vlbart_tiny_d64", "vqa", K=4, max_length=10, seed0=100, want=("skip",))
    case("beam_vlbart_early_lp06", "vlbart_tiny_d64", "caption", K=3, max_length=12, lp=0.6, early=True, seed0=200)
    case("beam_vlbart_maxlen_lp2", "vlbart_tiny_d64", "caption", K=3, max_length=7, lp=2.0, seed0=300, want=("maxlen",))
    case("beam_vlbart_minlen_ngram", "vlbart_tiny_d64", "caption", K=5, max_length=12, min_length=5, ngram=2, seed0=400)
    case("beam_vlbart_lora", "vlbart_tiny_lora_d64", "vqa", K=3, max_length=10, lora=True, seed0=500)
    case("beam_vlbart_video_tvc", "vlbart_tiny_video_d64", "tvc", K=5, max_length=10, video=True, L=24, seed0=600)
    case("beam_vlt5_vqa", "vlt5_tiny_d64", "vqa", K=4, max_length=10, kind="t5", seed0=700)


if __name__ == "__main__":
    main()
