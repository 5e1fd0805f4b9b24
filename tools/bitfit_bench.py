#!/usr/bin/env python3
"""BitFit's bias-gradient kernels (csrc/biasgrad.hip) alone and in a BART-base train step, everything in ONE process with the legs timed
in ALTERNATING rounds (HIP events), bf16:

  kernels, cold (a read-modify-write over 1 GiB before every timed call, as tools/prompt_bench.py) and warm, M = 28,000 rows:
    vlpet_colsum_seg  28,000 x 2,304 (q | k | v, 3 segments of 768)      against 3 x vlpet_colsum on [M, 768] (the separate dq, dk, dv)
    vlpet_colsum_seg  28,000 x 4,608 (six layers' cross keys)            against 6 x vlpet_colsum on [M, 768]
    vlpet_act_dropout_bwd_cols 28,000 x 3,072 (fc1 bias path, p = 0.1)   against vlpet_act_dropout_bwd + vlpet_colsum on [M, 3,072]
  one BART-base BitFit train step (vqa shape), eager and replayed (Trainer(graph=True)), FUSE_BIAS_GRAD_SITES on and off, plus a
  second switch-on leg: the spread between the two identical legs is the yardstick a difference has to beat.

``--batch`` sets the step's batch (default 500: 28,000 encoder rows).  profiles/r18_bitfit.md keeps the output."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vlpet_amd.functional as VF  # noqa: E402
import vlpet_amd.host.bart as HB  # noqa: E402
import vlpet_amd.train as TR  # noqa: E402
from vlpet_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=500)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=6, help="train steps per leg and round")
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()

lib = _lib.load()
dev, dtype, BF = "cuda", torch.bfloat16, _lib.VLPET_BF16
M, ITERS, COLD_CALLS = 28000, 30, 5
evict = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
st = torch.cuda.current_stream().cuda_stream


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
    return f"{statistics.median(t):.1f} ({min(t):.1f}..{max(t):.1f})"


def ab(name, new, old, traffic_bytes):
    rows = []
    for mode, timer in (("cold", cold), ("warm", warm)):
        for fn in (new, old):
            for _ in range(3):
                fn()
        t = [[], []]
        for _ in range(args.rounds):
            for i, fn in enumerate((new, old)):
                t[i] += timer(fn)
        m = [statistics.median(x) for x in t]
        rows.append(f"| {name} | {mode} | {cell(t[0])} | {cell(t[1])} | {m[0] / m[1]:.2f} | {traffic_bytes / m[0] / 1e6:.2f} |")
    return rows


lines = []
g = torch.Generator(device=dev).manual_seed(1)
for S, w, what in ((3, 768, "q|k|v"), (6, 768, "cross keys")):
    n = S * w
    x = torch.randn(M, n, device=dev, generator=g).to(dtype)
    blocks = [x[:, s * w:(s + 1) * w].contiguous() for s in range(S)]
    outs = torch.empty(S, w, device=dev)
    ptrs = (ctypes.c_void_p * S)(*[outs[s].data_ptr() for s in range(S)])
    nbytes = lib.vlpet_colsum_seg_workspace_bytes(M, n)
    ws = torch.empty(nbytes // 4, device=dev)
    ws1 = torch.empty(lib.vlpet_sublayer_tail_partials(M) * w, device=dev)

    def seg():
        assert lib.vlpet_colsum_seg(x.data_ptr(), M, S, w, n, ptrs, ws.data_ptr(), nbytes, BF, st) == 0

    def pairs():
        for s in range(S):
            assert lib.vlpet_colsum(blocks[s].data_ptr(), M, w, ws1.data_ptr(), outs[s].data_ptr(), BF, st) == 0
    lines += ab(f"colsum_seg {M} x {n} ({what}) vs {S} x colsum", seg, pairs, M * n * 2)

n = 3072
x = (torch.randn(M, n, device=dev, generator=g) * 2).to(dtype)
dy = torch.randn(M, n, device=dev, generator=g).to(dtype)
dx = torch.empty_like(x)
out = torch.empty(n, device=dev)
wsa = torch.empty(min((M + 3) // 4, 2048) * n, device=dev)
wsc = torch.empty(lib.vlpet_sublayer_tail_partials(M) * n, device=dev)


def fused_act():
    assert lib.vlpet_act_dropout_bwd_cols(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), M, n, 0, 0.1, 7, wsa.data_ptr(), wsa.numel() * 4,
                                          out.data_ptr(), None, BF, st) == 0


def act_then_colsum():
    assert lib.vlpet_act_dropout_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), M * n, 0, 0.1, 7, BF, st) == 0
    assert lib.vlpet_colsum(dx.data_ptr(), M, n, wsc.data_ptr(), out.data_ptr(), BF, st) == 0


lines += ab(f"act_dropout_bwd_cols {M} x {n} vs act_dropout_bwd + colsum", fused_act, act_then_colsum, M * n * 2 * 3)
print(f"kernels through the C ABI, bf16, us per call: median (min..max) over {args.rounds} alternating rounds; TB/s = the new kernel's "
      "compulsory traffic (input once; the activation backward: two reads and a write) over its median")
print("| site | calls | new | replaced | new / replaced | TB/s |")
print("|---|---|---|---|---|---|")
print("\n".join(lines), flush=True)

if args.skip_step:
    sys.exit(0)

# ---- one BART-base BitFit train step: switch on, off, on again -- alternating, same process
OFF = dict(use_adapter=False, use_single_adapter=False, no_encoder_adapter=False, no_decoder_adapter=False, use_adapter_down_dim=False,
           use_encoder_adapter_down_multihead=False, use_encoder_adapter_gating_large_x_lowrank=False,
           use_decoder_enc_attn_value_parallel_adapter_down_dim=False, unfreeze_encoder_layer_norms=False, unfreeze_bias=True)


def make(graph, fused):
    VF.FUSE_BIAS_GRAD_SITES = fused
    torch.manual_seed(0)
    cfg = HB.vlpet_config(**OFF)
    model = HB.VLBart(cfg)
    TR.trainable_names(model, cfg)
    model.to(dev)
    TR.cast_frozen(model, dtype)
    tr = TR.Trainer(model, cfg, lr=1e-4, total_steps=100000, graph=graph)
    b = TR.synthetic_batch("vqa", args.batch, cfg, dev, torch.Generator(device=dev).manual_seed(3))
    for _ in range(4):                      # eager warm-up, capture, replays
        tr.step(b)
    torch.cuda.synchronize()
    return tr, b, fused


def time_leg(leg):
    tr, b, fused = leg
    VF.FUSE_BIAS_GRAD_SITES = fused
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        tr.step(b)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


print(f"\nBART-base BitFit train step, vqa shape, batch {args.batch}, bf16, ms per step: median (min..max) over {args.rounds} alternating rounds of "
      f"{args.steps} steps")
print("| step | sites on (A) | sites off | sites on (B: the same leg again) | A / off | A / B |")
print("|---|---|---|---|---|---|")
for graph in (False, True):
    c0 = dict(VF.BITFIT_CALLS)
    legs = [make(graph, True), make(graph, False), make(graph, True)]
    t = [[], [], []]
    for _ in range(args.rounds):
        for i, leg in enumerate(legs):
            t[i].append(time_leg(leg))
    m = [statistics.median(x) for x in t]
    f = lambda x: f"{statistics.median(x):.3f} ({min(x):.3f}..{max(x):.3f})"
    print(f"| {'replayed (hipGraph)' if graph else 'eager'} | {f(t[0])} | {f(t[1])} | {f(t[2])} | {m[0] / m[1]:.3f} | {m[0] / m[2]:.3f} |", flush=True)
    print(f"  (host-side site calls while this row ran: { {k: VF.BITFIT_CALLS[k] - c0[k] for k in c0} })", flush=True)
    del legs
