#!/usr/bin/env python3
"""Hyperformer's weight generation for ONE stack (adapters.AdapterLayersHyperNetController with cross-attention: 12 generators, every
layer's adapters from one task embedding), three ways, fp32 parameters, packs for bf16 IO:

  kernel     ``controller.generate()``: the embedding chain in torch, then ONE functional.hyper_generate launch (csrc/hyper.hip), backward
             two launches
  (a) batched  the same embedding chain, then eager.hyper_generate: one F.linear per generator on all layers' embeddings
  (b) per layer  the reference's shape: ``controller(task_embedding, layer)`` per layer -- a lookup, a cat, the MLP, a LayerNorm and four
             nn.Linear generators per block, call by call

at (d, r, P, E) = (768, 96, 8, 6) (BART-base as scripts/image-text/hyperformer.sh sets it) and (768, 96, 64, 12) (T5-base's depth at the
config's default projected dimension).  Three tables: generate; generate + pack; generate + pack + backward (upstream gradients on
every generated tensor).  One process, the legs timed in ALTERNATING rounds (HIP events), warm (``ITERS`` back-to-back calls per round)
and cold (a read-modify-write over 1 GiB before every timed call, as tools/phm_bench.py).  profiles/r17_hyperformer.md keeps them.
usage: hyper_bench.py"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vlpet_amd.functional as F  # noqa: E402
from vlpet_amd import _lib, eager  # noqa: E402
from vlpet_amd.adapters import AdapterLayersHyperNetController, MetaAdapterConfig  # noqa: E402

dev = "cuda"
ROUNDS, ITERS, COLD_CALLS = 7, 20, 3
IO = _lib.VLPET_BF16
evict = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
PARTS = ("down_w", "down_b", "up_w", "up_b")


def warm(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) / ITERS * 1e3]


def cold(fn):
    out = []
    for _ in range(COLD_CALLS):
        evict.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def cell(t):
    return f"{statistics.median(t):.0f} ({min(t):.0f}..{max(t):.0f})"


def flat(weights):
    return [getattr(per[b], a) for per in weights for b in per for a in PARTS]


rows = {"generate": [], "generate + pack": [], "generate + pack + backward": []}
for d, r, P, E in ((768, 96, 8, 6), (768, 96, 64, 12)):
    torch.manual_seed(P)
    cfg = MetaAdapterConfig(input_dim=d, d_model=d, reduction_factor=d // r, projected_task_embedding_dim=P, tasks=["vqa"])
    ctl = AdapterLayersHyperNetController(cfg, E, True).to(dev)
    with torch.no_grad():
        for p in ctl.parameters():
            p.copy_(torch.randn_like(p) * 0.05)
        ctl.LayerNorm.weight.add_(1.0)
    te = torch.randn(cfg.task_embedding_dim, device=dev, requires_grad=True)
    params = [te] + list(ctl.parameters())
    packs = [{}, {}, {}]

    def kernel(pack):
        return ctl.generate(te, io_dtype=IO if pack else None)

    def batched(pack):
        w = ctl._collect(eager.hyper_generate(ctl.maps(), ctl.embedding_rows(te)), None)
        if pack:
            ctl._pack_all(w, packs[1], IO)
        return w

    def per_layer(pack):
        w = [ctl(te, layer) for layer in range(E)]
        if pack:
            ctl._pack_all(w, packs[2], IO)
        return w

    grads = [torch.randn_like(t) for t in flat(kernel(False))]

    def fwd_bwd(leg):
        return torch.autograd.grad(flat(leg(True)), params, grads)

    ref = fwd_bwd(per_layer)
    err = [max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fwd_bwd(leg), ref)) for leg in (kernel, batched)]
    legs = (kernel, batched, per_layer)
    for what, call in (("generate", lambda leg: (lambda: leg(False))), ("generate + pack", lambda leg: (lambda: leg(True))),
                       ("generate + pack + backward", lambda leg: (lambda: fwd_bwd(leg)))):
        fns = [call(leg) for leg in legs]
        for mode, timer in (("warm", warm), ("cold", cold)):
            for fn in fns:
                for _ in range(3):
                    fn()
            t = [[], [], []]
            for _ in range(ROUNDS):                             # alternating rounds
                for i, fn in enumerate(fns):
                    t[i] += timer(fn)
            m = [statistics.median(x) for x in t]
            rows[what].append(f"| ({d}, {r}, {P}, {E}) | {mode} | {cell(t[0])} | {cell(t[1])} | {cell(t[2])} | {m[0] / m[1]:.2f} | "
                              f"{m[0] / m[2]:.2f} | {err[0]:.1g} / {err[1]:.1g} |")
            print(what, (d, r, P, E), mode, "done", file=sys.stderr, flush=True)

for what, lines in rows.items():
    print(f"\n{what}: one stack with cross-attention (12 generators), fp32 parameters; us per call: median (min..max) over {ROUNDS} "
          f"alternating rounds")
    print("| (d, r, P, E) | calls | kernel | (a) batched torch | (b) per-layer chain | kernel / (a) | kernel / (b) | max rel. gradient "
          "difference to (b): kernel / (a) |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(lines), flush=True)
