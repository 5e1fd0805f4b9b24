"""GPU: the five entry points of csrc/rowgate.hip through the C ABI, against their fp64 statements (tests/rowgate_spec.py), past
the launch cap and at every piece count.

The kernel launches at most RG_CAP workgroups of RG_WAVES waves, one row per wave; past RG_CAP * RG_WAVES rows a wave walks
several rows and carries the weight-gradient partials across them.  A lane owns the 16-byte pieces lane, lane + 64, ... of a row
(NP = 1..4 of them); the widths below give every NP with a full and a ragged last group in both dtypes.

Bounds are derived, not measured (u = 2^-24; arithmetic is fp32 on the IO-dtype inputs; ``abs`` is the sum of |product| over the
products that form the element, computed by the spec in fp64 from the same inputs):
  * element-wise output:        |err| <= 4 u abs  (+ one rounding when the output is bf16: half a unit in the last of bf16's 8
                                significant bits at the magnitude of the result, see _el_bound)
  * a row dot:                  |err| <= (n + 8) u abs,  n = d / 64 additions per lane + 6 shuffle steps
  * a partial, summed in fp64:  |err| <= (n + 8) u abs,  n = rows per wave + 4
Every element is held to its own bound: no per-tensor norm, no floor.  Every output has sentinel rows behind it and a NaN body
(tests/sentinel.py)."""
import functools
import math

import pytest
import torch

import rowgate_spec as RS
from sentinel import pad_intact, padded_flat, padded_rows

pytestmark = pytest.mark.gpu

# ---- launch geometry (csrc/rowgate.hip) -------------------------------------------------------------------------------------
RG_WAVES = 4            # rowgate.hip:22   constexpr int RG_WAVES = 4: waves (= rows in flight) per workgroup
RG_CAP = 2048           # rowgate.hip:168  const int64_t cap = 256 * 8 -- never used to size anything below: the block count is read
                        #                  from vlpet_rowgate_partials, and test_the_cap_is_where_the_shapes_assume holds it to this
MAX_PIECES = 4 * 64     # api.hip:1603     d / E > 4 * 64 is refused (E = 8 bf16, 4 fp32 elements per 16-byte piece)
E_SHAPE, E_ALIGN, E_NULL, E_DTYPE = -1, -3, -5, -6      # include/vlpet_hip.h:31-36

U = 2.0 ** -24
ROWS = [1, 3, 4, 5, 8191, 8192, 8193, 16387, 24581]      # one wave, idle waves, the cap, one wave with two rows, three rows ragged
WIDTHS = {torch.bfloat16: [8, 512, 520, 768, 1024, 1032, 1536, 1544, 2048],      # NP 1, 1, 2, 2, 2, 3, 3, 4, 4
          torch.float32: [8, 256, 264, 768, 1024]}                               # NP 1, 1, 2, 3, 4
OPS = ["dot_pair", "dot_single", "dot_product", "affine", "affine_gamma", "bwd", "vec_fwd", "vec_fwd_u", "vec_bwd"]


def _shapes():
    out = []
    for dt in (torch.bfloat16, torch.float32):
        s = [(M, d) for d in WIDTHS[dt] for M in (5, 8193)] + [(M, d) for M in ROWS for d in (64, 768)]
        out += [(dt, M, d) for M, d in sorted(set(s))]
    return out


CASES = [(dt, M, d, op) for dt, M, d in _shapes() for op in OPS]       # shape-major: the inputs of a shape are made once
_id = lambda c: f"{'bf16' if c[0] == torch.bfloat16 else 'fp32'}-M{c[1]}-d{c[2]}-{c[3]}"


def _lib():
    from vlpet_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=1)
def _inputs(dtype, M, d):
    """Seeded inputs of one shape: the row tensors already rounded to the IO dtype, the vectors fp32; each on the GPU (``g``) and,
    for the spec, in fp64 on the CPU (``c``)."""
    gen = torch.Generator().manual_seed(1000 * d + M)
    row = lambda: torch.randn(M, d, generator=gen).to(dtype)
    c = dict(dy=row(), x1=row(), h=row(), ra=torch.randn(M, generator=gen), rb=torch.randn(M, generator=gen),
             va=torch.randn(d, generator=gen), vc=torch.randn(d, generator=gen))
    g = {k: v.cuda() for k, v in c.items()}
    return g, {k: v.double() for k, v in c.items()}


def _hold(name, got, ref, bound, log):
    """Every element within its own bound (a NaN -- an unwritten element -- fails); the worst err / bound goes to ``log``."""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    ok = err <= bound
    log.append(f"{name} {float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max()):.3f}")
    assert bool(ok.all()), (name, int((~ok).sum()), "elements over their bound; worst err/bound", log[-1])


def _el_bound(abs_terms, ref, dtype):
    """4 u abs, plus for a bf16 output the one rounding: half a unit in the last place, 2^(e - 8) for a result in [2^e, 2^(e + 1)).
    The bound first written for this rounding was 2^-9 |ref|.  No correctly rounding kernel can meet it: bf16 keeps 8 significant
    bits, so round-to-nearest errs by up to 2^-8 of a value just above a power of two (1 + 2^-8 lies halfway between 1 and 1 + 2^-7).
    Measured against 4 u abs + 2^-9 |ref| the worst element of every bf16 output sat between 1.3 and 2.0 (worst 1.99), never above
    2 -- correct rounding, not a kernel error (csrc/rowops.h Piece::store converts with (__bf16)v, round-to-nearest-even).  The
    half-ulp form is the exact statement of one rounding and is tighter than 2^-8 |ref| everywhere but at the powers of two."""
    b = 4 * U * abs_terms
    if dtype != torch.bfloat16:
        return b
    mag = (ref.abs() + b).clamp_min(2.0 ** -126)
    return b + torch.exp2(torch.floor(torch.log2(mag)) - 8)


def _partials(lib, M, d):
    nb = lib.vlpet_rowgate_partials(M)
    assert nb == min((M + RG_WAVES - 1) // RG_WAVES, RG_CAP)
    buf, body = padded_rows(nb * 2, d, torch.float32)
    return nb, buf, body


def _part_bound(M, nb, abs_terms):
    rows_per_wave = math.ceil(M / (nb * RG_WAVES))
    return (rows_per_wave + 4 + 8) * U * abs_terms


def test_the_cap_is_where_the_shapes_assume():
    """A changed cap must fail here, not silently stop ROWS from reaching the row loop."""
    _, lib = _lib()
    assert lib.vlpet_rowgate_partials(RG_CAP * RG_WAVES) == RG_CAP == 2048
    assert lib.vlpet_rowgate_partials(10 ** 6) == RG_CAP
    assert lib.vlpet_rowgate_partials(RG_CAP * RG_WAVES - 1) == RG_CAP and lib.vlpet_rowgate_partials(8188) == 2047
    assert lib.vlpet_rowgate_partials(1) == 1 and lib.vlpet_rowgate_partials(5) == 2 and lib.vlpet_rowgate_partials(0) == 0
    assert max(ROWS) > 3 * RG_CAP * RG_WAVES and max(ROWS) % (RG_CAP * RG_WAVES) != 0          # three rows per wave, ragged


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rowgate_entry_point_matches_its_statement(case):
    dtype, M, d, op = case
    L, lib = _lib()
    io = L.VLPET_F32 if dtype == torch.float32 else L.VLPET_BF16
    st = torch.cuda.current_stream().cuda_stream
    g, c = _inputs(dtype, M, d)
    p = lambda t: t.data_ptr()
    log = []
    if op.startswith("dot"):
        a, cc, wa, wc = {"dot_pair": ("x1", "h", "va", "vc"), "dot_single": ("dy", None, "va", None),
                         "dot_product": ("dy", "h", None, None)}[op]
        gp = lambda k: p(g[k]) if k else None
        sbuf, s = padded_flat(M, torch.float32)
        assert lib.vlpet_row_dot(gp(a), gp(cc), gp(wa), gp(wc), p(s), M, d, io, st) == 0
        r = RS.row_dot(c[a], c[cc] if cc else None, c[wa] if wa else None, c[wc] if wc else None)
        _hold("s", s, r.s, (math.ceil(d / 64) + 6 + 8) * U * r.s_abs, log)
        assert pad_intact(sbuf, s)
    elif op.startswith("affine"):
        gamma = op == "affine_gamma"
        ybuf, y = padded_rows(M, d, dtype)
        assert lib.vlpet_row_affine(p(g["h"]), p(g["ra"]), p(g["rb"]) if gamma else None, p(y), M, d, io, st) == 0
        r = RS.row_affine(c["h"], c["ra"], c["rb"] if gamma else None)
        _hold("y", y, r.o1, _el_bound(r.o1_abs, r.o1, dtype), log)
        assert pad_intact(ybuf, y)
    elif op == "bwd":
        dhbuf, dh = padded_rows(M, d, dtype)
        dxbuf, dx1 = padded_rows(M, d, dtype)
        nb, pbuf, part = _partials(lib, M, d)
        assert lib.vlpet_rowgate_bwd(p(g["dy"]), p(g["x1"]), p(g["h"]), p(g["ra"]), p(g["rb"]), p(g["va"]), p(g["vc"]), p(dh), p(dx1),
                                     p(part), M, d, io, st) == 0
        r = RS.row_bwd(c["dy"], c["x1"], c["h"], c["ra"], c["rb"], c["va"], c["vc"])
        _hold("dh", dh, r.dh, _el_bound(r.dh_abs, r.dh, dtype), log)
        _hold("dx1", dx1, r.dx1, _el_bound(r.dx1_abs, r.dx1, dtype), log)
        ps = part.double().cpu().view(nb, 2, d).sum(0)          # partials [blocks, 2, d], summed in fp64
        _hold("p0", ps[0], r.p0, _part_bound(M, nb, r.p0_abs), log)
        _hold("p1", ps[1], r.p1, _part_bound(M, nb, r.p1_abs), log)
        assert pad_intact(dhbuf, dh) and pad_intact(dxbuf, dx1) and pad_intact(pbuf, part)
    elif op.startswith("vec_fwd"):
        u = op == "vec_fwd_u"
        ybuf, y = padded_rows(M, d, dtype)
        assert lib.vlpet_vecgate_fwd(p(g["h"]), p(g["va"]), p(g["vc"]) if u else None, p(y), M, d, io, st) == 0
        r = RS.vec_fwd(c["h"], c["va"], c["vc"] if u else None)
        _hold("y", y, r.o1, _el_bound(r.o1_abs, r.o1, dtype), log)
        assert pad_intact(ybuf, y)
    else:
        dhbuf, dh = padded_rows(M, d, dtype)
        nb, pbuf, part = _partials(lib, M, d)
        assert lib.vlpet_vecgate_bwd(p(g["dy"]), p(g["h"]), p(g["va"]), p(dh), p(part), M, d, io, st) == 0
        r = RS.vec_bwd(c["dy"], c["h"], c["va"])
        _hold("dh", dh, r.dh, _el_bound(r.dh_abs, r.dh, dtype), log)
        ps = part.double().cpu().view(nb, 2, d).sum(0)
        _hold("p0", ps[0], r.p0, _part_bound(M, nb, r.p0_abs), log)
        _hold("p1", ps[1], r.p1, _part_bound(M, nb, r.p1_abs), log)
        assert pad_intact(dhbuf, dh) and pad_intact(pbuf, part)
    print("ROWGATE worst err/bound", _id(case), " ".join(log))


def _calls(L, lib, t, M, d, io, st):
    """name -> (function, argument list, indices of required pointers, indices of row operands) with every pointer valid."""
    p = lambda k: t[k].data_ptr()
    tail = [M, d, io, st]
    return {
        "row_dot": (lib.vlpet_row_dot, [p("x1"), p("h"), p("va"), p("vc"), p("s")] + tail, [0, 4], [0, 1]),
        "row_affine": (lib.vlpet_row_affine, [p("h"), p("ra"), p("rb"), p("o1")] + tail, [0, 1, 3], [0, 3]),
        "rowgate_bwd": (lib.vlpet_rowgate_bwd, [p("dy"), p("x1"), p("h"), p("ra"), p("rb"), p("va"), p("vc"), p("o1"), p("o2"),
                                                p("part")] + tail, list(range(10)), [0, 1, 2, 7, 8]),
        "vecgate_fwd": (lib.vlpet_vecgate_fwd, [p("h"), p("va"), p("vc"), p("o1")] + tail, [0, 1, 3], [0, 3]),
        "vecgate_bwd": (lib.vlpet_vecgate_bwd, [p("dy"), p("h"), p("va"), p("o1"), p("part")] + tail, [0, 1, 2, 3, 4], [0, 1, 3]),
    }


@pytest.mark.parametrize("name", ["row_dot", "row_affine", "rowgate_bwd", "vecgate_fwd", "vecgate_bwd"])
def test_rowgate_refusals_launch_nothing(name):
    """Shape, NULL, alignment and dtype refusals; every output stays NaN (nothing was launched)."""
    L, lib = _lib()
    st = torch.cuda.current_stream().cuda_stream
    M, dmax = 6, 2056
    t = {k: torch.randn(M, dmax, device="cuda") for k in ("dy", "x1", "h")}
    t.update({k: torch.randn(M, device="cuda") for k in ("ra", "rb")})
    t.update({k: torch.randn(dmax, device="cuda") for k in ("va", "vc")})
    outs = dict(o1=torch.full((M, dmax), float("nan"), device="cuda"), o2=torch.full((M, dmax), float("nan"), device="cuda"),
                s=torch.full((M,), float("nan"), device="cuda"), part=torch.full((2, 2, dmax), float("nan"), device="cuda"))
    t.update(outs)

    def call(M=M, d=64, io=L.VLPET_BF16, edit=None):
        fn, args, _, _ = _calls(L, lib, t, M, d, io, st)[name]
        if edit:
            edit(args)
        return fn(*args)

    assert call(d=2056, io=L.VLPET_BF16) == E_SHAPE and call(d=1032, io=L.VLPET_F32) == E_SHAPE       # d / E > MAX_PIECES
    assert 2056 // 8 == MAX_PIECES + 1 and 1032 // 4 > MAX_PIECES
    assert call(M=0) == E_SHAPE and call(M=-3) == E_SHAPE
    assert call(d=12) == E_SHAPE and call(d=12, io=L.VLPET_F32) == E_SHAPE and call(d=0) == E_SHAPE
    assert call(io=7) == E_DTYPE
    _, _, required, rows = _calls(L, lib, t, M, 64, L.VLPET_BF16, st)[name]

    def null(*idx):
        return lambda a: [a.__setitem__(i, None) for i in idx]

    for i in required:
        assert call(edit=null(i)) == E_NULL, (name, i)
    for i in rows:          # a row operand offset by 8 bytes
        assert call(edit=lambda a, i=i: a.__setitem__(i, a[i] + 8)) == E_ALIGN, (name, i)
    if name == "row_dot":   # the two mode-dependent rules: the plain pair product (wa NULL) needs c; a weighted pair needs wc
        assert call(edit=null(1, 2)) == E_NULL
        assert call(edit=null(3)) == E_NULL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())
