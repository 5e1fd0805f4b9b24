#!/usr/bin/env python3
"""Same launches, same bits: the K1 / K2 backward entry points over one case per plan row (csrc/api.hip bwd_plan; the shapes of
tests/test_gpu_k1_bwd_forms.py) plus the sizes of tests/test_gpu_cols.py, in a fixed order with fixed seeds.

    VLPET_LIB=<library> python tools/k1_bwd_hashes.py OUT.json          one line per case: a sha256 of every output tensor
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/k1_bwd_hashes.py OUT.json
    python tools/k1_bwd_hashes.py --launches DIR OUT.txt                the ordered (kernel, grid, workgroup, LDS) list of a trace
    python tools/k1_bwd_hashes.py --compare A B                         two outputs of either kind, line by line

Run it once per library, each in a fresh process; profiles/k1_bwd_plan_same_launches.md has the protocol and a result."""
import csv
import glob
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (M, d, r, dtype, gate_mode, saved block, [phases of the calls]): gate_mode 0 = K2
ROWS = [(129, 256, 32), (129, 256, 96), (33, 128, 96), (8191, 128, 96), (8192, 128, 96), (129, 384, 192), (129, 256, 192), (5377, 384, 192),
        (8193, 128, 192), (16385, 128, 192), (4096, 64, 96), (4097, 64, 96)]
COLS = [(M, 768, 96) for M in (1, 32, 33, 127, 129, 224, 1000, 3500, 8232, 28000, 31616)] + \
       [(777, 768, 8), (640, 256, 32), (257, 128, 16), (5000, 1024, 96), (3000, 1024, 192), (32, 768, 192), (1000, 768, 192), (18250, 768, 192)]
CASES = [(M, d, r, "bfloat16", 1, True, [3]) for M, d, r in ROWS + COLS] + [
    (33, 64, 192, "float32", 1, True, [3]), (129, 256, 96, "bfloat16", 1, True, [1 | 4, 2 | 4]), (129, 256, 96, "bfloat16", 1, False, [3]),
    (1000, 768, 96, "bfloat16", 2, True, [3]), (999, 768, 192, "bfloat16", 2, True, [3]),
    (5000, 768, 96, "bfloat16", 1, True, [1, 2 | 8, 16]), (9000, 768, 96, "bfloat16", 1, True, [3 | 32]),
    (33, 128, 96, "bfloat16", 0, True, [3]), (33, 64, 96, "bfloat16", 0, True, [3]), (777, 768, 96, "bfloat16", 0, True, [3])]


def run_case(lib, F, torch, M, d, r, dtype, gate_mode, saved, phases, seed):
    """[(variant, [sha256 of dx1, dx2 and the parameter gradients])]: gated cases run with y and without dx1_in, then the reverse"""
    dev, dt = "cuda", getattr(torch, dtype)
    g = torch.Generator(device=dev).manual_seed(seed)
    x1, x2, dy, dxin = (torch.randn(M, d, device=dev, generator=g).to(dt) for _ in range(4))
    mk = lambda *s: torch.randn(*s, device=dev, generator=g) * 0.05
    W = [mk(r, d), mk(r), mk(d, r), mk(d), mk(r, d), mk(r), mk(d, r), mk(d)]
    io, tiles, st = F._io_dtype(x2), F.rank_tiles(r), torch.cuda.current_stream().cuda_stream
    pa, pg = F.pack_pair([W[0]], [W[1]], W[2], W[3], io, tiles), F.pack_pair([W[4]], [W[5]], W[6], W[7], io, tiles)
    nws = lib.vlpet_bwd_workspace_bytes(M, d, tiles, int(gate_mode != 0), io)
    out = torch.empty_like(x2)
    sv = torch.empty(lib.vlpet_saved_bytes(M, tiles, io), dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()
    if gate_mode == 0:
        assert lib.vlpet_parallel_adapter_fwd_save(P(x2), P(x1), P(pa.buf), P(out), P(sv), M, d, tiles, 0.7, io, st) == 0
    elif saved:
        assert lib.vlpet_adapter_gate_fwd_save(P(x1), P(x2), P(pa.buf), P(pg.buf), P(out), P(sv), M, d, tiles, gate_mode, 1.0, 0.5, 0.7, io, st) == 0
    res = []
    for variant in (("k2",) if gate_mode == 0 else ("plain",) if not saved else ("from_y", "dx1_in")):
        dx1, dx2 = torch.zeros_like(x1), torch.zeros_like(x2)
        ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
        G = [torch.zeros_like(w) for w in W]
        for ph in phases:
            if variant == "k2":
                rc = lib.vlpet_parallel_adapter_bwd_saved(P(dy), P(x2), P(sv), P(pa.buf), P(dx2), *[P(t) for t in G[:4]], r, P(ws), nws, M, d, tiles, 0.7, io, st)
            else:
                tail = [P(t) for t in G] + [r, r, P(ws), nws, M, d, tiles, gate_mode, 1.0, 0.5, 0.7, io, st]
                if variant == "plain":
                    rc = lib.vlpet_adapter_gate_bwd_phase(ph, P(dy), P(x1), P(x2), P(pa.buf), P(pg.buf), P(dx1), P(dx2), *tail)
                else:
                    rc = lib.vlpet_adapter_gate_bwd_saved_y(ph, P(dy), P(x1), P(x2), P(out) if variant == "from_y" else None, P(sv), P(pa.buf),
                                                            P(pg.buf), P(dxin) if variant == "dx1_in" else None, P(dx1), P(dx2), *tail)
            assert rc == 0, (M, d, r, dtype, gate_mode, saved, ph, variant, rc)
        torch.cuda.synchronize()
        outs = ([dx2] + G[:4]) if variant == "k2" else [dx1, dx2] + G
        res.append((variant, [hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16] for t in outs]))
    return res


def launches(trace_dir):
    """the kernel dispatches of a rocprofv3 --kernel-trace csv, in start order"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: int(r["start_timestamp"]))
    dims = lambda r, what: "x".join(r[f"{what}_size_{a}"] for a in "xyz")
    return [f'{r["kernel_name"]} grid={dims(r, "grid")} wg={dims(r, "workgroup")} lds={r["lds_block_size"]}' for r in rows]


def main():
    if sys.argv[1] == "--launches":
        lines = launches(sys.argv[2])
        open(sys.argv[3], "w").write("\n".join(lines) + "\n")
        print(f"{len(lines)} dispatches -> {sys.argv[3]}")
        return 0
    if sys.argv[1] == "--compare":
        a, b = (open(p).read().split("\n") for p in sys.argv[2:4])
        diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
        print(f"{sys.argv[2]}: {len(a) - 1} lines, {sys.argv[3]}: {len(b) - 1} lines, differing: {len(diff)}" + (f" (first at {diff[0] + 1}: {a[diff[0]]!r} | {b[diff[0]]!r})" if diff else ""))
        return 1 if diff or len(a) != len(b) else 0
    import torch
    import vlpet_amd.functional as F
    from vlpet_amd import _lib
    lib = _lib.load()
    with open(sys.argv[1], "w") as f:
        for i, case in enumerate(CASES):
            f.write(json.dumps([list(case), run_case(lib, F, torch, *case, seed=100 + i)]) + "\n")
    print(f"{len(CASES)} cases -> {sys.argv[1]} ({_lib.LIB_PATH})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
