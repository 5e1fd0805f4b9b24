#!/usr/bin/env python3
"""Compacter's weight expansion of one adapter (csrc/phm.hip: vlpet_phm_expand_pair_fwd / _bwd through the C ABI, and the same through
functional.phm_expand_pair's autograd) against the plain-torch composition it replaces, per PHM layer
``einsum('bac,bkp->bakcp') -> view -> sum(0) -> t().contiguous()`` and its autograd -- fp32 parameters, d = 768, r = 96, one process,
the legs timed in ALTERNATING rounds (HIP events).  Two tables (forward; forward + backward), each warm (``iters`` back-to-back calls
per round) and cold (a read-modify-write over 1 GiB before every timed call, as tools/attnbench.py).  profiles/r15_compacter.md keeps
them; the routing (adapters.adapter_modeling.HyperComplexAdapter) is judged by the forward + backward row at n = 2.
usage: phm_bench.py [n ...]      (default 2 4)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vlpet_amd.functional as F  # noqa: E402
from vlpet_amd import _lib  # noqa: E402

Ns = [int(a) for a in sys.argv[1:]] or [2, 4]
lib = _lib.load()
dev, d, r = "cuda", 768, 96
st = torch.cuda.current_stream().cuda_stream
ROUNDS, ITERS, COLD_CALLS = 9, 200, 5
evict = torch.zeros(1 << 28, dtype=torch.float32, device=dev)


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


def torch_weight(rule, W, n, fin, fout):
    return torch.einsum("bac,bkp->bakcp", rule, W).view(n, fin, fout).sum(0).t().contiguous()


rows = {"forward": [], "forward + backward": []}
for n in Ns:
    g = torch.Generator(device=dev).manual_seed(n)
    mk = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.05).requires_grad_(True)
    rule_d, W_d, rule_u, W_u = mk(n, n, n), mk(n, d // n, r // n), mk(n, n, n), mk(n, r // n, d // n)
    P = [rule_d, W_d, rule_u, W_u]
    g_d, g_u = torch.randn(r, d, device=dev, generator=g), torch.randn(d, r, device=dev, generator=g)
    wt_d, wt_u = torch.empty(r, d, device=dev), torch.empty(d, r, device=dev)
    outs = [torch.empty_like(p) for p in P]
    nws = lib.vlpet_phm_workspace_bytes(d, r, n)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def abi_fwd():
        rc = lib.vlpet_phm_expand_pair_fwd(rule_d.data_ptr(), W_d.data_ptr(), rule_u.data_ptr(), W_u.data_ptr(), wt_d.data_ptr(),
                                           wt_u.data_ptr(), d, r, n, _lib.VLPET_F32, st)
        assert rc == 0

    def abi_fwd_bwd():
        abi_fwd()
        rc = lib.vlpet_phm_expand_pair_bwd(g_d.data_ptr(), g_u.data_ptr(), rule_d.data_ptr(), W_d.data_ptr(), rule_u.data_ptr(),
                                           W_u.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                           ws.data_ptr(), nws, d, r, n, _lib.VLPET_F32, st)
        assert rc == 0

    def fn_fwd():
        with torch.no_grad():
            return F.phm_expand_pair(rule_d, W_d, rule_u, W_u, n)

    def fn_fwd_bwd():
        a, b = F.phm_expand_pair(rule_d, W_d, rule_u, W_u, n)
        return torch.autograd.grad([a, b], P, [g_d, g_u])

    def torch_fwd():
        with torch.no_grad():
            return torch_weight(rule_d, W_d, n, d, r), torch_weight(rule_u, W_u, n, r, d)

    def torch_fwd_bwd():
        a, b = torch_weight(rule_d, W_d, n, d, r), torch_weight(rule_u, W_u, n, r, d)
        return torch.autograd.grad([a, b], P, [g_d, g_u])

    ref, got = torch_fwd_bwd(), fn_fwd_bwd()
    err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref))
    err = max(err, max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fn_fwd(), torch_fwd())))
    for what, legs in (("forward", (abi_fwd, fn_fwd, torch_fwd)), ("forward + backward", (abi_fwd_bwd, fn_fwd_bwd, torch_fwd_bwd))):
        for mode, timer in (("warm", warm), ("cold", cold)):
            for fn in legs:
                for _ in range(10):
                    fn()
            t = [[], [], []]
            for _ in range(ROUNDS):                             # alternating rounds
                for i, fn in enumerate(legs):
                    t[i] += timer(fn)
            m = [statistics.median(x) for x in t]
            rows[what].append(f"| {n} | {mode} | {cell(t[0])} | {cell(t[1])} | {cell(t[2])} | {m[0] / m[2]:.2f} | {m[1] / m[2]:.2f} | {err:.2g} |")

for what, lines in rows.items():
    print(f"\n{what}, (d, r) = ({d}, {r}), fp32 parameters; us per call: median (min..max) over {ROUNDS} alternating rounds")
    print("| n | calls | HIP, C ABI | HIP, functional.phm_expand_pair | torch composition | ABI / torch | functional / torch | max rel. difference |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(lines), flush=True)
