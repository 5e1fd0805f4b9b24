#!/usr/bin/env python3
"""Greedy-generation speed at the evaluation shapes (BART-base VL-PET, configs[1], bf16): per-step ms and generated tokens/s of

  hip      VLBart.generate: per-layer caches, decode.decode_attention / decode.greedy_pick on csrc/decode.hip
  torch    the same cached loop on the torch forms (decode.EAGER, host.bart.EAGER_ATTENTION: SDPA, eager argmax + processors)
  nocache  what a user writes without generate(): the training-path decoder re-run on the whole prefix at every step
  graph    generate(graph=True): the hip step captured once and replayed (decode.graph_generate).  Its first call (eager warm-up) and
           second call (capture + replays) are timed on their own and never enter the timed calls.  With hip and graph both asked
           for, ``--ab-rounds N`` rounds of alternating hip / graph calls follow (same process, same inputs): the spread of each
           leg and the ratio; ``--launches`` counts the kernel launches of one decode step of each leg with the torch profiler
           (a run of its own: tracing slows the host).

Every path runs max_length - 1 steps (min_length = max_length bans eos throughout).  Shapes: VQA (B = 500, S_enc = 20 + 36 = 56,
max_length 20), caption (B = 416, S_enc = 40 + 36 = 76, max_length 40).

    python tools/genbench.py [--shapes vqa caption] [--paths hip torch nocache] [--reps 3] [--out FILE]
    python tools/genbench.py --stats kernel_stats.csv     # rocprofv3 --kernel-trace --stats output of a `--paths hip --reps 1`
                                                          # run at the VQA shape -> both kernels' time against their bytes

Beam search (``--num-beams K``, K > 1): generate(num_beams = K) at the video captioning shape (task tvc, encoder length 600 + 64 =
664, max_length 20, every step run: min_length = max_length) for BART-base VL-PET on the video config (B = 50) and T5-base VL-PET
(B = 30), hip against torch (decode.EAGER).  ``--stats FILE --num-beams K`` reads the kernel stats of a `--num-beams K --paths hip
--reps 1 --warmup 0 --models bart` run.

``--pet single_adapter``: the Single-Adapter baseline instead of VL-PET (scripts/image-text/single_adapter.sh: a sequential adapter of
width 96 behind every attention and feed-forward block of both stacks, no VL-PET module).  ``--adapter-tail-ab N``: after the legs, N
rounds of alternating FUSE_ADAPTER_TAIL off / on calls of every hip / graph leg asked for (same process, same inputs; a graph leg
re-captures after every flip, untimed): ms per call and per step of both settings, and whether the tokens agree.

``--pet compacter``: the Compacter baseline (scripts/image-text/single_compacter.sh: the same placement with PHM adapters, division 2,
no shared rule, no factorization); the expanded weights are cached for the whole call, so the decode step runs the Single-Adapter
launches.

``--long-attention``: the hosts' LONG_ATTENTION switch on for every leg (the 664-token encoder on csrc/attn_long.hip).
``--long-ab N`` (with ``--num-beams``): after the legs, N rounds of alternating switch-off / switch-on hip calls, two successive
calls each: ms per call of both settings and the fraction of tokens on which the two successive calls agree (1.0 = reproducible).
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"vqa": dict(task="vqa", B=500, max_length=20, S_enc=56), "caption": dict(task="caption", B=416, max_length=40, S_enc=76)}
HBM = 8.0e12          # bytes/s: the HBM rate the repository's roofline figures use


def decode_bytes(B, S_enc, E, n_layers, max_length, V, esz=2):
    """algorithmic bytes of one generate() call: attention (q, K, V read, o written; self-attention keys 0..pos plus the appended
    row written) and logits (one read of [B, V] per step)"""
    steps = max_length - 1
    cross = n_layers * steps * B * (2 * S_enc * E + 2 * E) * esz
    selfa = n_layers * sum(B * (2 * (p + 1) * E + 2 * E + 2 * E) * esz for p in range(steps))
    logits = steps * B * V * esz
    return dict(attn=cross + selfa, attn_calls=2 * n_layers * steps, pick=logits, pick_calls=steps)


BEAM_SHAPES = {"bart": dict(task="tvc", B=50, max_length=20, S_enc=664), "t5": dict(task="tvc", B=30, max_length=20, S_enc=664)}


def beam_bytes(B, K, S_enc, E, n_layers, max_length, V, esz=2):
    """algorithmic bytes of one generate(num_beams = K) call: attention (cross caches read once per item -- never expanded --, the
    self-attention keys of each of the B * K rows, q / o / appended rows), beam_rows (one read of the [B * K, V] logits per step plus
    the partials) and beam_advance (the partials, the ids / key rows moved)"""
    rows, steps = B * K, max_length - 1
    cross = n_layers * steps * (B * 2 * S_enc * E + rows * 2 * E) * esz
    selfa = n_layers * sum(rows * (2 * (p + 1) * E + 4 * E) * esz for p in range(steps))
    return dict(attn=cross + selfa, attn_calls=2 * n_layers * steps, rows=steps * rows * V * esz, rows_calls=steps,
                advance=sum(rows * (4 * 2 * K + 2 * 8 * (p + 2) + 2 * 4 * (p + 2)) for p in range(steps)), advance_calls=steps)


SINGLE_ADAPTER = dict(use_adapter=True, use_single_adapter=True, no_encoder_adapter=False, no_decoder_adapter=False,
                      unfreeze_layer_norms=True, use_adapter_down_dim=False, reduction_factor=8, use_encoder_adapter_down_multihead=False,
                      use_encoder_adapter_gating_large_x_lowrank=False, use_decoder_enc_attn_value_parallel_adapter_down_dim=False,
                      unfreeze_encoder_layer_norms=False)      # single_adapter.sh
COMPACTER = dict(SINGLE_ADAPTER, use_adapter=False, use_compacter=True, hypercomplex_division=2, shared_phm_rule=False,
                 factorized_phm=False)                         # single_compacter.sh


def build(dev, kind="bart", video=False, pet="vlpet"):
    import torch
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    torch.manual_seed(0)
    over = dict(feat_dim=512, n_boxes=64, tasks="tvqa,how2qa,tvc,yc2c") if video else {}
    if pet in ("single_adapter", "compacter"):
        over.update(SINGLE_ADAPTER if pet == "single_adapter" else COMPACTER)
    if kind == "t5":
        import vlpet_amd.host.t5 as HT
        if pet in ("single_adapter", "compacter"):
            over.update(use_encoder_gating_scaling=False)
        cfg = HT.vlt5_config(**over)
        model = HT.VLT5(cfg)
    else:
        cfg = HB.vlpet_config(**over)
        model = HB.VLBart(cfg)
    TR.trainable_names(model, cfg)
    model.to(dev)
    TR.cast_frozen(model, torch.bfloat16)
    return model.eval(), cfg


def nocache_generate(model, ids, vis, task, max_length, eos, start):
    import torch
    import torch.nn.functional as F
    from vlpet_amd.lmloss import _padded_head
    with torch.no_grad():
        enc, mask = model.model.encoder(ids, vis, None, task, False)
        w = model.model.shared.weight
        head = _padded_head(w, enc.dtype)
        out = torch.full((ids.shape[0], 1), start, dtype=torch.long, device=ids.device)
        for _ in range(max_length - 1):
            h = model.model.decoder(out, enc, mask, task)[:, -1]
            scores = F.linear(h, head)[:, :w.shape[0]].float()
            scores[:, eos] = float("-inf")              # min_length = max_length
            out = torch.cat([out, scores.argmax(-1, keepdim=True)], 1)
        return out


def timed_legs(args, path, call):
    """(ms per call over args.reps calls after the warm-up, the last output, extras): the graph leg's first two calls -- eager
    warm-up, capture -- are timed separately, from an empty graph cache, so they are what a fresh process pays"""
    import torch
    import vlpet_amd.decode as D
    extra = {}
    if path == "graph":
        D.clear_graphs()
        s0 = dict(D.GRAPH_STATS)
        for name in ("first_call_ms", "capture_call_ms"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            extra[name] = round((time.perf_counter() - t) * 1e3, 2)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.reps):
        out = call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3 / args.reps
    if path == "graph":
        d = {k: D.GRAPH_STATS[k] - s0[k] for k in s0}
        assert d["captures"] == 1 and d["eager"] == 0 and d["replays"] > 0, d      # the timed calls replayed; nothing fell back
        extra["replays_per_call"] = d["replays"] // (1 + args.warmup + args.reps)
    return ms, out, extra


def ab_rounds(args, calls, steps, tag):
    """alternating hip / graph calls: per leg the ms per call of every round, and graph / hip of the means"""
    import torch
    per = {p: [] for p in calls}
    for _ in range(args.ab_rounds):
        for p, call in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
            per[p].append((time.perf_counter() - t) * 1e3 / args.reps)
    mean = {p: sum(v) / len(v) for p, v in per.items()}
    row = dict(tag, ab_rounds=args.ab_rounds, reps=args.reps,
               **{f"{p}_ms": [round(x, 2) for x in v] for p, v in per.items()},
               **{f"{p}_mean_ms": round(m, 2) for p, m in mean.items()},
               **{f"{p}_step_ms": round(m / steps, 3) for p, m in mean.items()},
               graph_over_hip=round(mean["graph"] / mean["hip"], 3))
    print(json.dumps(row), flush=True)
    return row


def adapter_tail_ab(args, calls, steps, tag):
    """alternating FUSE_ADAPTER_TAIL off / on calls of each leg in ``calls``"""
    import torch
    import vlpet_amd.adapter_tail as AT
    import vlpet_amd.decode as D
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    saved = (HB.FUSE_ADAPTER_TAIL, HT.FUSE_ADAPTER_TAIL)
    rows = []
    try:
        for path, call in calls.items():
            per, outs, fused_calls = {"off": [], "on": []}, {}, {}
            for _ in range(args.adapter_tail_ab):
                for leg in ("off", "on"):
                    HB.FUSE_ADAPTER_TAIL = HT.FUSE_ADAPTER_TAIL = leg == "on"
                    D.clear_graphs()
                    n0 = AT.CALLS
                    call(), call()                                   # (a graph leg: eager warm-up, capture)
                    fused_calls[leg] = (AT.CALLS - n0) // 2
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.reps):
                        outs[leg] = call()
                    torch.cuda.synchronize()
                    per[leg].append((time.perf_counter() - t) * 1e3 / args.reps)
            mean = {leg: sum(v) / len(v) for leg, v in per.items()}
            same = outs["on"].shape == outs["off"].shape and bool((outs["on"] == outs["off"]).all())
            row = dict(tag, path=path, adapter_tail_ab_rounds=args.adapter_tail_ab, reps=args.reps, max_rows=AT.ADAPTER_TAIL_MAX_ROWS,
                       fused_launches_per_eager_call=fused_calls,
                       **{f"fuse_{leg}_ms": [round(x, 2) for x in v] for leg, v in per.items()},
                       **{f"fuse_{leg}_step_ms": round(m / steps, 3) for leg, m in mean.items()},
                       on_over_off=round(mean["on"] / mean["off"], 3), tokens_equal=same)
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        HB.FUSE_ADAPTER_TAIL, HT.FUSE_ADAPTER_TAIL = saved
        D.clear_graphs()
    return rows


def launches_per_step(make_call):
    """kernel launches of ONE decode step: a call of three tokens minus a call of two, counted by the torch profiler.
    ``make_call(max_length)`` returns the call."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    counts = []
    for ml in (2, 3):
        call = make_call(ml)
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        counts.append(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                          and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()))
    return counts[1] - counts[0]


def run(args):
    import torch
    import vlpet_amd.decode as D
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    dev = "cuda"
    model, cfg = build(dev, pet=args.pet)
    rows = []
    for shape in args.shapes:
        sh = SHAPES[shape]
        gen = torch.Generator(device=dev).manual_seed(1)
        b = TR.synthetic_batch(sh["task"], sh["B"], cfg, dev, gen, no_padding=False)
        ids, vis, ml = b["input_ids"], b["vis_inputs"], sh["max_length"]
        steps = ml - 1
        with torch.no_grad():
            for _ in range(2):
                model.model.encoder(ids, vis, None, sh["task"], False)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                model.model.encoder(ids, vis, None, sh["task"], False)
            torch.cuda.synchronize()
            enc_ms = (time.perf_counter() - t) * 1e3 / args.reps
        outs, calls = {}, {}
        for path in args.paths:
            def call(path=path, ml=ml):
                if path == "nocache":
                    return nocache_generate(model, ids, vis, sh["task"], ml, 2, cfg.decoder_start_token_id)
                return model.generate(ids, vis, sh["task"], max_length=ml, min_length=ml, graph=path == "graph")
            calls[path] = call
            if args.launches:
                if path in ("hip", "graph"):     # (graph: its first call of a key issues the launches a capture records)
                    def make_call(n, path=path, call=call):
                        return lambda: (D.clear_graphs(), call(path, n))
                    print(json.dumps(dict(shape=shape, path=path, launches_per_step=launches_per_step(make_call))), flush=True)
                continue
            saved = (D.EAGER, HB.EAGER_ATTENTION)
            D.EAGER = HB.EAGER_ATTENTION = path == "torch"
            try:
                ms, out, extra = timed_legs(args, path, call)
            finally:
                D.EAGER, HB.EAGER_ATTENTION = saved
            outs[path] = out
            assert out.shape == (sh["B"], ml), out.shape
            row = dict(shape=shape, path=path, B=sh["B"], S_enc=sh["S_enc"], max_length=ml, total_ms=round(ms, 2),
                       encoder_ms=round(enc_ms, 2), step_ms=round((ms - enc_ms) / steps, 3),
                       tokens_per_s=round(sh["B"] * steps / (ms / 1e3), 1), **extra)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if "hip" in outs and "graph" in outs and args.ab_rounds > 0:
            ab_rounds(args, {p: calls[p] for p in ("hip", "graph")}, steps, dict(shape=shape, encoder_ms=round(enc_ms, 2)))
        if args.adapter_tail_ab > 0:
            adapter_tail_ab(args, {p: calls[p] for p in ("hip", "graph") if p in outs}, steps, dict(shape=shape, B=sh["B"], pet=args.pet))
        if "hip" in outs:
            for p, o in outs.items():       # bf16 paths may part ways where two logits are within rounding: report, do not fail
                agree = float((o == outs["hip"]).float().mean())
                print(json.dumps(dict(shape=shape, tokens_equal_to_hip=p, fraction=round(agree, 4))), flush=True)
    return rows


def run_beams(args):
    import torch
    import vlpet_amd.decode as D
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    dev = "cuda"
    rows = []
    for kind in args.models:
        sh = BEAM_SHAPES[kind]
        model, cfg = build(dev, kind, video=True, pet=args.pet)
        gen = torch.Generator(device=dev).manual_seed(1)
        b = TR.synthetic_batch(sh["task"], sh["B"], cfg, dev, gen, no_padding=False)
        ids, vis, ml = b["input_ids"], b["vis_inputs"], sh["max_length"]
        enc_len = ids.shape[1] + vis[0].shape[1]
        outs, calls = {}, {}
        for path in args.paths:
            if path == "nocache":
                continue
            def call(path=path, ml=ml):
                return model.generate(ids, vis, sh["task"], max_length=ml, min_length=ml, num_beams=args.num_beams,
                                      graph=path == "graph")
            calls[path] = call
            if args.launches:
                if path in ("hip", "graph"):
                    def make_call(n, path=path, call=call):
                        return lambda: (D.clear_graphs(), call(path, n))
                    print(json.dumps(dict(model=kind, path=path, launches_per_step=launches_per_step(make_call))), flush=True)
                continue
            saved = (D.EAGER, HB.EAGER_ATTENTION)
            D.EAGER = HB.EAGER_ATTENTION = path == "torch"
            try:
                ms, out, extra = timed_legs(args, path, call)
            finally:
                D.EAGER, HB.EAGER_ATTENTION = saved
            outs[path] = out
            row = dict(model=kind, path=path, num_beams=args.num_beams, B=sh["B"], enc_len=enc_len, max_length=ml,
                       total_ms=round(ms, 2), step_ms=round(ms / (ml - 1), 3), **extra)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if "hip" in outs and "graph" in outs:
            agree = float((outs["graph"] == outs["hip"]).float().mean()) if outs["graph"].shape == outs["hip"].shape else 0.0
            print(json.dumps(dict(model=kind, tokens_equal_to_hip="graph", fraction=round(agree, 4))), flush=True)
            if args.ab_rounds > 0:
                ab_rounds(args, {p: calls[p] for p in ("hip", "graph")}, ml - 1, dict(model=kind, num_beams=args.num_beams))
        if args.adapter_tail_ab > 0:
            adapter_tail_ab(args, {p: calls[p] for p in ("hip", "graph") if p in outs}, ml - 1,
                            dict(model=kind, num_beams=args.num_beams, B=sh["B"], pet=args.pet))
        if args.long_ab > 0 and "hip" in calls:
            import vlpet_amd.host.t5 as HT
            per, agree = {"off": [], "on": []}, {"off": [], "on": []}
            saved = (HB.LONG_ATTENTION, HT.LONG_ATTENTION)
            try:
                for _ in range(args.long_ab):
                    for leg in ("off", "on"):
                        HB.LONG_ATTENTION = HT.LONG_ATTENTION = leg == "on"
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        a, b2 = calls["hip"](), calls["hip"]()
                        torch.cuda.synchronize()
                        per[leg].append((time.perf_counter() - t) * 1e3 / 2)
                        agree[leg].append(float((a == b2).float().mean()) if a.shape == b2.shape else 0.0)
            finally:
                HB.LONG_ATTENTION, HT.LONG_ATTENTION = saved
            print(json.dumps(dict(model=kind, num_beams=args.num_beams, B=sh["B"], enc_len=enc_len, long_ab_rounds=args.long_ab,
                                  **{f"long_{leg}_ms": [round(x, 2) for x in per[leg]] for leg in per},
                                  **{f"long_{leg}_mean_ms": round(sum(per[leg]) / len(per[leg]), 2) for leg in per},
                                  **{f"long_{leg}_successive_calls_token_agreement": [round(x, 4) for x in agree[leg]] for leg in agree})),
                  flush=True)
        if "hip" in outs and "torch" in outs:
            o, h = outs["torch"], outs["hip"]
            agree = float((o == h).float().mean()) if o.shape == h.shape else 0.0
            print(json.dumps(dict(model=kind, tokens_equal_to_hip="torch", fraction=round(agree, 4))), flush=True)
        del model
        torch.cuda.empty_cache()
    return rows


def beam_stats(path, K):
    """rocprofv3 kernel stats of one `--num-beams K --paths hip --reps 1 --warmup 0 --models bart` run: each kernel's time against
    its algorithmic bytes"""
    sh = BEAM_SHAPES["bart"]
    by = beam_bytes(sh["B"], K, sh["S_enc"], 768, 6, sh["max_length"], 50465)
    tot = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key, pat in (("attn", "attn_decode_kernel"), ("rows", "beam_rows_kernel"), ("advance", "beam_advance_kernel")):
                if pat in name:
                    t = tot.setdefault(key, [0, 0.0])
                    t[0] += int(r["Calls"])
                    t[1] += float(r["TotalDurationNs"])
    names = dict(attn="vlpet_attn_decode_beam", rows="vlpet_beam_rows", advance="vlpet_beam_advance")
    out = []
    for key in ("attn", "rows", "advance"):
        if key not in tot:
            continue
        calls, ns = tot[key]
        reps = max(1, round(calls / by[key + "_calls"]))
        rate = by[key] * reps / (ns * 1e-9)
        out.append(dict(kernel=names[key], calls=calls, total_us=round(ns / 1e3, 1), us_per_call=round(ns / 1e3 / calls, 2),
                        algorithmic_MB_per_call=round(by[key] / by[key + "_calls"] / 1e6, 3), TB_per_s=round(rate / 1e12, 2),
                        hbm_fraction=round(rate / HBM, 3)))
    return out


def table(rows):
    lines = ["| shape | path | B | S_enc | max_length | total ms | encoder ms | ms / step | tokens / s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['path']} | {r['B']} | {r['S_enc']} | {r['max_length']} | {r['total_ms']} | {r['encoder_ms']} | "
                     f"{r['step_ms']} | {r['tokens_per_s']} |")
    return "\n".join(lines)


def beam_table(rows):
    lines = ["| model | path | num_beams | B | encoder length | max_length | total ms | ms / step |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['model']} | {r['path']} | {r['num_beams']} | {r['B']} | {r['enc_len']} | {r['max_length']} | "
                     f"{r['total_ms']} | {r['step_ms']} |")
    return "\n".join(lines)


def stats(path, shape="vqa"):
    """rocprofv3 kernel stats of one `--paths hip --reps 1 --warmup 0` run at ``shape``: time of each decode kernel against its bytes"""
    sh = SHAPES[shape]
    by = decode_bytes(sh["B"], sh["S_enc"], 768, 6, sh["max_length"], 50465)
    tot = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key, pat in (("attn", "attn_decode_kernel"), ("pick", "greedy_pick_kernel")):
                if pat in name:
                    t = tot.setdefault(key, [0, 0.0])
                    t[0] += int(r["Calls"])
                    t[1] += float(r["TotalDurationNs"])
    out = []
    for key in ("attn", "pick"):
        if key not in tot:
            continue
        calls, ns = tot[key]
        reps = max(1, round(calls / by[key + "_calls"]))
        rate = by[key] * reps / (ns * 1e-9)
        out.append(dict(kernel="vlpet_attn_decode" if key == "attn" else "vlpet_greedy_pick", calls=calls, total_us=round(ns / 1e3, 1),
                        us_per_call=round(ns / 1e3 / calls, 2), algorithmic_MB_per_call=round(by[key] / by[key + "_calls"] / 1e6, 2),
                        TB_per_s=round(rate / 1e12, 2), hbm_fraction=round(rate / HBM, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["vqa", "caption"], choices=list(SHAPES))
    ap.add_argument("--paths", nargs="+", default=["hip", "torch", "nocache"], choices=["hip", "torch", "nocache", "graph"])
    ap.add_argument("--ab-rounds", type=int, default=3, help="alternating hip / graph rounds after the legs (0: none)")
    ap.add_argument("--launches", action="store_true", help="count one decode step's kernel launches (hip, graph) instead of timing")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--models", nargs="+", default=["bart", "t5"], choices=list(BEAM_SHAPES))
    ap.add_argument("--pet", default="vlpet", choices=["vlpet", "single_adapter", "compacter"], help="the PET method the models are built with")
    ap.add_argument("--adapter-tail-ab", type=int, default=0, help="alternating FUSE_ADAPTER_TAIL off / on rounds of the hip / graph legs")
    ap.add_argument("--long-attention", action="store_true", help="set the hosts' LONG_ATTENTION switch for every leg")
    ap.add_argument("--long-ab", type=int, default=0, help="with --num-beams: alternating switch-off / switch-on rounds of the hip leg")
    args = ap.parse_args()
    if args.long_attention:
        import vlpet_amd.host.bart as HB
        import vlpet_amd.host.t5 as HT
        HB.LONG_ATTENTION = HT.LONG_ATTENTION = True
    if args.stats:
        for r in (stats(args.stats) if args.num_beams == 1 else beam_stats(args.stats, args.num_beams)):
            print(json.dumps(r))
        return
    if args.num_beams > 1:
        rows = run_beams(args)
        text = beam_table(rows)
    else:
        rows = run(args)
        text = table(rows)
    if args.launches:
        return
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
