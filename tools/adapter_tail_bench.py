#!/usr/bin/env python3
"""Fused adapter + tail launch (vlpet_adapter_tail_fwd) against the composition it replaces (vlpet_parallel_adapter_fwd with x = y = h,
then vlpet_sublayer_tail_fwd without dropout), both through the C ABI, one process, the two timed in ALTERNATING rounds (HIP events
around ``iters`` back-to-back calls each), bf16, d = 768, r = 96, LayerNorm form.  Prints a markdown table: the median round of each and
the spread; profiles/r14_single_adapter.md keeps it, vlpet_amd.adapter_tail.ADAPTER_TAIL_MAX_ROWS is read off it.
usage: adapter_tail_bench.py [M ...]      (default 250 500 2080 3500 28000)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vlpet_amd.functional as F  # noqa: E402
from vlpet_amd import _lib  # noqa: E402

Ms = [int(a) for a in sys.argv[1:]] or [250, 500, 2080, 3500, 28000]
lib = _lib.load()
dev, dt, d, r = "cuda", torch.bfloat16, 768, 96
st = torch.cuda.current_stream().cuda_stream
ROUNDS, ITERS = 9, 200


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


print("| M | fused us (median, min..max) | K2 + K5 us (median, min..max) | fused / composed | max abs difference |")
print("|---|---|---|---|---|")
for M in Ms:
    g = torch.Generator(device=dev).manual_seed(0)
    h, res = (torch.randn(M, d, device=dev, generator=g).to(dt) for _ in range(2))
    mk = lambda *s: torch.randn(*s, device=dev, generator=g) * 0.05
    wd, bd, wu, bu = mk(r, d), mk(r), mk(d, r), mk(d)
    gamma, beta = 1.0 + mk(d), mk(d)
    io, tiles = _lib.VLPET_BF16, F.rank_tiles(r)
    pk = F.pack_pair([wd], [bd], wu, bu, io, tiles)
    mid, out_c, out_f = (torch.empty_like(h) for _ in range(3))
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)

    def composed():
        rc = lib.vlpet_parallel_adapter_fwd(h.data_ptr(), h.data_ptr(), pk.buf.data_ptr(), mid.data_ptr(), M, d, tiles, 1.0, io, st)
        rc |= lib.vlpet_sublayer_tail_fwd(mid.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out_c.data_ptr(), None,
                                          mean.data_ptr(), rstd.data_ptr(), None, M, d, 1e-5, 0.0, 0, 1, io, st)
        assert rc == 0

    def fused():
        rc = lib.vlpet_adapter_tail_fwd(h.data_ptr(), res.data_ptr(), wd.data_ptr(), bd.data_ptr(), wu.data_ptr(), bu.data_ptr(),
                                        gamma.data_ptr(), beta.data_ptr(), out_f.data_ptr(), M, d, r, 1.0, 1e-5, 1, _lib.VLPET_F32, io, st)
        assert rc == 0

    iters = max(20, min(ITERS, 2_000_000 // M))
    for fn in (composed, fused):
        timed(fn, 10)                                   # warm-up of both
    tf, tc = [], []
    for _ in range(ROUNDS):                             # alternating rounds
        tf.append(timed(fused, iters))
        tc.append(timed(composed, iters))
    diff = float((out_f.float() - out_c.float()).abs().max())
    mf, mc = statistics.median(tf), statistics.median(tc)
    print(f"| {M} | {mf:.1f} ({min(tf):.1f}..{max(tf):.1f}) | {mc:.1f} ({min(tc):.1f}..{max(tc):.1f}) | {mf / mc:.2f} | {diff:.3g} |", flush=True)
