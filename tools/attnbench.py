#!/usr/bin/env python3
"""Short-sequence attention kernels vs torch SDPA at the configs[1] encoder shapes (HIP events on the launch stream).

    python tools/attnbench.py                  # the short kernels, forward and backward, ATTNBENCH_P = dropout
    python tools/attnbench.py long [rounds]    # the long forward (csrc/attn_long.hip) against the SDPA forward the hosts otherwise call,
                                               # at the video encoder's shapes, no_grad, key mask present, alternating legs; every
                                               # timed call starts cold (ATTNBENCH_WARM=1: back-to-back calls instead)
    python tools/attnbench.py long-train [rounds]   # forward + backward of the long training kernels (csrc/attn_long.hip with dropout,
                                               # csrc/attn_long_bwd.hip) against the SDPA forward + backward the hosts otherwise call:
                                               # encoder self-attention (BART B = 50, T5 + bias B = 30, S = 664) and the decoder's
                                               # cross-attention (20 x 664, B = 50); ATTNBENCH_P = dropout (default 0.1); same rules
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from vlpet_amd.attention import short_attention

MFMA_PEAK = 2.5e15      # bf16 dense MFMA FLOP/s of the chip (the roofline figure of DESIGN.md)


def long_bench(rounds):
    """us per call (median over the rounds' calls) of long_attention and of F.scaled_dot_product_attention on the same inputs; as in
    tools/k1bench.py's K1BENCH_COLD a read-modify-write over 1 GiB runs before every timed call, so that neither leg reads its
    inputs from the Infinity Cache the previous call filled"""
    import statistics
    from vlpet_amd.attention import AttnBias, long_attention
    H, S = 12, 664
    cold = not os.environ.get("ATTNBENCH_WARM")
    evict = torch.zeros(1 << 28, dtype=torch.float32, device="cuda") if cold else None

    def one(fn):
        if cold:
            evict.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    with torch.no_grad():
        for name, B, biased in [("bart", 50, False), ("t5", 30, True)]:
            g = torch.Generator(device="cuda").manual_seed(1)
            amp = 0.4 if biased else 1.5
            q, k, v = ((torch.randn(B, S, H * 64, device="cuda", generator=g) * amp).bfloat16() for _ in range(3))
            lens = torch.randint(400, S + 1, (B,), device="cuda", generator=g)
            keep = torch.arange(S, device="cuda")[None, :] < lens[:, None]
            sh = lambda t: t.view(B, S, H, 64).transpose(1, 2)
            if biased:      # T5: scale 1, the shared bias; the library path takes the merged dense additive mask (host/t5.py AttnSpec.dense)
                rel = torch.randn(1, H, S, S, device="cuda", generator=g)
                bias = AttnBias(rel, transposed=False)
                dense = (rel + (1.0 - keep[:, None, None, :].float()) * -10000.0).bfloat16()
                ours = lambda: long_attention(q, k, v, H, keep, scale=1.0, bias=bias)
                lib = lambda: F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=dense, scale=1.0).transpose(1, 2).reshape(B, S, H * 64)
            else:
                mask = keep[:, None, None, :]
                ours = lambda: long_attention(q, k, v, H, keep)
                lib = lambda: F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=mask).transpose(1, 2).reshape(B, S, H * 64)
            a, b = ours().float(), lib().float()
            live = keep[:, :, None].float()
            err = float(((a - b) * live).abs().max() / b.abs().max())
            t = {"long": [], "sdpa": []}
            for _ in range(3):
                one(ours); one(lib)
            for _ in range(rounds):
                for leg, fn in (("long", ours), ("sdpa", lib)):
                    t[leg] += [one(fn) for _ in range(5)]
            flops = 4.0 * B * H * S * S * 64
            for leg in ("long", "sdpa"):
                us = statistics.median(t[leg])
                print(f"attnbench long {name:4s} B={B} H={H} S={S} {'cold' if cold else 'warm'} {leg:4s}: median {us:8.1f} us  min {min(t[leg]):8.1f}  "
                      f"max {max(t[leg]):8.1f}  ({len(t[leg])} calls)  {flops / (us * 1e-6) / 1e12:6.1f} TFLOP/s = {flops / (us * 1e-6) / MFMA_PEAK:.3f} of the bf16 MFMA peak")
            print(f"attnbench long {name:4s}: long / sdpa = {statistics.median(t['long']) / statistics.median(t['sdpa']):.3f}   max |long - sdpa| / max |sdpa| = {err:.2e}",
                  flush=True)


def long_train_bench(rounds):
    """us per forward + backward (median over the rounds' calls) of long_attention_train and of F.scaled_dot_product_attention on the same
    inputs, timed as long_bench times the forward: cold calls, alternating legs"""
    import statistics
    from vlpet_amd.attention import AttnBias, long_attention_train
    H = 12
    p = float(os.environ.get("ATTNBENCH_P", "0.1"))
    cold = not os.environ.get("ATTNBENCH_WARM")
    evict = torch.zeros(1 << 28, dtype=torch.float32, device="cuda") if cold else None

    def one(fn):
        if cold:
            evict.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for name, B, Lq, Lk, biased in [("bart", 50, 664, 664, False), ("t5", 30, 664, 664, True), ("cross", 50, 20, 664, False)]:
        g = torch.Generator(device="cuda").manual_seed(1)
        amp = 0.4 if biased else 1.5
        mk = lambda L: (torch.randn(B, L, H * 64, device="cuda", generator=g) * amp).bfloat16().requires_grad_(True)
        q, k, v = mk(Lq), mk(Lk), mk(Lk)
        dout = torch.randn(B, Lq, H * 64, device="cuda", generator=g).bfloat16()
        lens = torch.randint(400, Lk + 1, (B,), device="cuda", generator=g)
        keep = torch.arange(Lk, device="cuda")[None, :] < lens[:, None]
        sh = lambda t, L: t.view(B, L, H, 64).transpose(1, 2)
        if biased:      # T5: scale 1, the shared bias; the library path takes the merged dense additive mask (host/t5.py AttnSpec.dense)
            rel = torch.randn(1, H, Lq, Lk, device="cuda", generator=g)
            bias = AttnBias(rel, transposed=False)
            dense = (rel + (1.0 - keep[:, None, None, :].float()) * -10000.0).bfloat16()
            fwd_ours = lambda: long_attention_train(q, k, v, H, keep, p=p, training=True, scale=1.0, bias=bias)
            fwd_lib = lambda: F.scaled_dot_product_attention(sh(q, Lq), sh(k, Lk), sh(v, Lk), attn_mask=dense, dropout_p=p,
                                                             scale=1.0).transpose(1, 2).reshape(B, Lq, H * 64)
        else:
            mask = keep[:, None, None, :]
            fwd_ours = lambda: long_attention_train(q, k, v, H, keep, p=p, training=True)
            fwd_lib = lambda: F.scaled_dot_product_attention(sh(q, Lq), sh(k, Lk), sh(v, Lk), attn_mask=mask,
                                                             dropout_p=p).transpose(1, 2).reshape(B, Lq, H * 64)

        def both(fwd):
            def run():
                q.grad = k.grad = v.grad = None
                fwd().backward(dout)
            return run
        ours, lib = both(fwd_ours), both(fwd_lib)
        t = {"long": [], "sdpa": []}
        for _ in range(3):
            one(ours); one(lib)
        for _ in range(rounds):
            for leg, fn in (("long", ours), ("sdpa", lib)):
                t[leg] += [one(fn) for _ in range(5)]
        flops = 4.0 * B * H * Lq * Lk * 64 * 3.5          # forward 2 products, backward 5 (the algorithmic count; ours recomputes 2 more)
        for leg in ("long", "sdpa"):
            us = statistics.median(t[leg])
            print(f"attnbench long-train {name:5s} B={B} H={H} Lq={Lq} Lk={Lk} p={p} {'cold' if cold else 'warm'} {leg:4s}: median {us:8.1f} us  "
                  f"min {min(t[leg]):8.1f}  max {max(t[leg]):8.1f}  ({len(t[leg])} calls)  {flops / (us * 1e-6) / 1e12:6.1f} TFLOP/s")
        print(f"attnbench long-train {name:5s}: long / sdpa = {statistics.median(t['long']) / statistics.median(t['sdpa']):.3f}", flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "long-train":
    long_train_bench(int(sys.argv[2]) if len(sys.argv) > 2 else 4)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "long":
    long_bench(int(sys.argv[2]) if len(sys.argv) > 2 else 4)
    sys.exit(0)

def timeit(fn, iters=30, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3

H = 12
P = float(os.environ.get("ATTNBENCH_P", "0.1"))
for name, B, S in [("vqa", 500, 56), ("gqa", 833, 56), ("nlvr", 166, 92), ("caption", 416, 76), ("dec-self", 500, 5)]:
    q, k, v, do = (torch.randn(B, S, H * 64, device="cuda").bfloat16().requires_grad_(i < 3) for i in range(4))
    o = short_attention(q, k, v, H, p=P, training=True, seed=1)
    t_f = timeit(lambda: short_attention(q, k, v, H, p=P, training=True, seed=1))
    t_fb = timeit(lambda: torch.autograd.grad(short_attention(q, k, v, H, p=P, training=True, seed=1), (q, k, v), do))
    sh = lambda t: t.view(B, S, H, 64).transpose(1, 2)
    sd = lambda: F.scaled_dot_product_attention(sh(q), sh(k), sh(v), dropout_p=P).transpose(1, 2).reshape(B, S, H * 64)
    t_sf = timeit(sd)
    t_sfb = timeit(lambda: torch.autograd.grad(sd(), (q, k, v), do))
    unit = B * S * H * 64 * 2 / 1e6
    print(f"{name:8s} B={B} S={S}: fwd {t_f:7.1f} us ({4*unit/t_f/1e3*1e3:6.0f} GB/s)  bwd {t_fb - t_f:7.1f} us ({8*unit/(t_fb-t_f)*1e3/1e3:6.0f} GB/s)"
          f"   | SDPA fwd {t_sf:7.1f}  bwd {t_sfb - t_sf:7.1f}")
