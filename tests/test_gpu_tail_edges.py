"""GPU: every entry point of csrc/tail.hip through the C ABI, against its fp64 statement (tests/tail_spec.py), at every
instantiation launch_io / launch_np can choose, past the three launch caps, with both parameter alignments, element by element.

One wave owns a row; a lane owns the pieces lane, lane + 64, ... (PB = 8 or 16 bytes, NP of them per lane); FULL is the branch-free
form taken when the row is exactly NP x 64 pieces AND gamma / beta / gamma_next are 16-byte aligned.  tail_blocks caps the grid at
256 / 512 / 1,024 workgroups of 4 waves; past the cap a wave walks several rows, the next one prefetched through a clamped load,
and carries the dgamma / dbeta sums across them.

Bounds are derived, not measured (u = 2^-24; arithmetic is fp32 on the IO-dtype inputs; every ``abs`` below is a sum of absolute
terms computed by the spec in fp64 from the same inputs; tests/tail_spec.py evaluates exactly these expressions as ``e_*``):

  * the sum h = x1 + keep y / (1 - p): the product, then the addition (or one fused step): |err| <= 2 u (|x1| + |y / (1 - p)|) = e_h;
    a dropped element is x1 itself (0); without dropout it is ONE correctly rounded fp32 addition, whose error the spec knows exactly.
  * a row statistic: n = ceil(d / 64) additions per lane + 6 shuffle steps, + 8 for the products, the division by d and the errors of
    the terms:  |err mean| <= (n + 8) u mean|h|;  the variance is CENTRED, so with c = h - mean, e_c = e_h + e_mean + u |c|:
    |err var| <= (n + 8) u var + mean(2 |c| e_c + e_c^2).  A one-pass variance misses this at a row offset of 1e3 by three orders.
  * rstd = rsqrt(var + eps): relative error 1/2 rel (1 + rel) with rel = (e_var + u v) / v, plus the device rsqrtf.  Its error is
    not stated in the headers or documents that come with the toolchain, so it is 4 x the worst relative error of the fp32 CPU
    restatement (1 / sqrt, 1.31 u on the suite's inputs; tests/test_tail_spec.py holds the figure): 5.24 u.
  * out = c rstd gamma + beta:  |gamma| (e_c rstd + |c| e_rstd) + 4 u (|c rstd gamma| + |beta| [+ |r|, post-norm residual]).
  * RMS tail: the norm reads the sum ROUNDED to the IO dtype.  Where the exact sum lies within e_h of a bf16 rounding boundary the
    kernel may land on either neighbour: e_hr = one unit in the last place there, 0 elsewhere (about 2 % of the elements under
    dropout with 1 / (1 - p) = 10 / 9, none without dropout), and e_hr takes e_h's place in the statistic and the output.
  * backward: xhat from (h, mean, rstd): 2 u |xhat| (RMS: u |xhat|; saved xhat: 0; from the output rows: 4 u (|out / gamma| +
    |beta / gamma|) -- out_save is an INPUT, so what its rounding cost is not in this bound and nothing here grows with
    |beta / gamma| beyond fp32 cancellation).  g = dout gamma;  c1 = mean(g): (n + 8) u mean|g|;  c2 = mean(g xhat): (n + 8) u
    mean|g xhat| + mean(|g| e_x);  dx = (g - c1 - xhat c2) rstd:  rstd (e_c1 + |xhat| e_c2 + |c2| e_x + 4 u (|g| + |c1| + |xhat c2|))
    + u |dx| [+ u (|dx| + |dres|) with a parked gradient];  dy = dx keep / (1 - p): that times 1 / (1 - p), + u |dy|.
  * a partial [workgroup][2][d]: rows per wave + the 4-wave combine (+ 8) additions, u each on the sum of |dout xhat| (|dout|) over
    that workgroup's rows, plus |dout| e_x + u |dout xhat| per term.  Each entry is held against the fp64 sum of ITS rows.
  * the reduce: ceil(nb / 16) additions per thread + 16 to combine (+ 8);  the column sum: the partial's and the reduce's together.
  * one half-ulp rounding where the output is bf16 (tail_spec.hold_bound, the form of test_gpu_rowgate._el_bound).
Every element is held to its own bound: no per-tensor norm, no floor.  keep_out equals dropout_spec.keep_mask bit for bit and dy is
exactly 0 where the spec drops.  Every output has a NaN body and sentinels behind it (tests/sentinel.py)."""
import functools

import pytest
import torch

import tail_spec as T
from sentinel import pad_intact, padded_flat, padded_rows

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
E_SHAPE, E_ALIGN, E_NULL, E_DTYPE = -1, -3, -5, -6      # include/vlpet_hip.h:31-36

# width -> (piece bytes PB, pieces per lane NP, FULL with 16-byte-aligned parameters), as launch_io / launch_np / tail_pieces8 choose
FORMS = {
    BF: {8: (8, 1, False), 248: (8, 1, False), 256: (8, 1, True),               # d <= 256: 8-byte pieces, one per lane
         264: (16, 1, False), 512: (16, 1, True),                              # 256 < d <= 512
         520: (8, 3, False), 760: (8, 3, False), 768: (8, 3, True),             # 512 < d <= 768: 8-byte pieces, three per lane
         776: (16, 2, False), 1024: (16, 2, True),                             # 768 < d <= 1024
         1032: (16, 3, False), 1536: (16, 3, True),                            # 1024 < d <= 1536
         1544: (16, 4, False), 2048: (16, 4, True),                            # 1536 < d <= 2048
         2056: (16, 8, False), 4096: (16, 8, False)},                          # 2048 < d <= 4096: never FULL
    F32: {8: (16, 1, False), 256: (16, 1, False), 264: (16, 2, False), 512: (16, 2, False), 520: (16, 3, False),
          768: (16, 3, False), 776: (16, 4, False), 1024: (16, 4, False), 1032: (16, 8, False), 2048: (16, 8, False)}}   # never FULL
WIDTHS = {dt: sorted(FORMS[dt]) for dt in FORMS}
FULL_WIDTHS = [256, 512, 768, 1024, 1536, 2048]
# rows: one wave, idle waves, two workgroups; the first cap and its first wave with two rows; cap 256 -> 512; ragged second rows;
# cap 512 -> 1,024 (8500 = 5 rows in some waves of 512 workgroups, 8501 = three rows per wave, ragged, of 1,024)
ROWS = [1, 3, 4, 5, 1024, 1025, 2500, 2501, 4099, 8500, 8501]
BLOCKS = {1: 1, 3: 1, 4: 1, 5: 2, 1024: 256, 1025: 256, 2500: 256, 2501: 512, 4099: 512, 8500: 512, 8501: 1024, 1029: 256, 37: 10}
NORM_OPS = [op for op in T.OPS if op not in ("fwd_res", "bwd_res", "bwd_res_p0", "colsum")]
DROP_OPS = ["fwd_ln", "fwd_res", "rms2_fwd", "bwd_ln", "bwd_res", "bwd_out", "rms_tail_bwd"]


def _shapes():
    out = []
    for dt in (BF, F32):
        s = [(M, d) for d in WIDTHS[dt] for M in (5, 1029)] + [(M, d) for M in ROWS for d in (64, 768)]
        out += [(dt, M, d) for M, d in sorted(set(s))]
    return out


CASES = [(dt, M, d, op) for dt, M, d in _shapes() for op in T.OPS if not (op == "colsum" and d % 16)]     # shape-major
_dn = lambda dt: "bf16" if dt == BF else "fp32"
_id = lambda c: f"{_dn(c[0])}-M{c[1]}-d{c[2]}-{c[3]}"


def _lib():
    from vlpet_amd import _lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def _no_seed_counter_left_behind():
    yield
    _lib()[1].vlpet_set_seed_counter(None)


def _to_gpu(I, d):
    """The inputs on the GPU; the per-column vectors also at a 4-byte offset inside a larger buffer (``*_mis``)."""
    G = {k: v.cuda() for k, v in I.items()}
    for k in ("gamma", "beta", "gamma2"):
        buf = torch.zeros(d + 8, device="cuda")
        buf[1:1 + d] = G[k]
        G[k + "_mis"] = buf[1:1 + d]
        assert G[k].data_ptr() % 16 == 0 and G[k + "_mis"].data_ptr() % 16 == 4
    return G


@functools.lru_cache(maxsize=2)
def _inputs(dtype, M, d):
    I = T.make_inputs(dtype, M, d)
    return I, _to_gpu(I, d)


def _run(op, G, M, d, dtype, p=None, mis=False):
    """The ABI call of one operation of tail_spec.OPS.  -> ({output name: body}, [(buffer, body)] for the sentinel check)"""
    L, lib = _lib()
    io = L.VLPET_F32 if dtype == F32 else L.VLPET_BF16
    st = torch.cuda.current_stream().cuda_stream
    P = lambda k: G[k + "_mis" if mis and k in ("gamma", "beta", "gamma2") else k].data_ptr()
    pads = []

    def rows(dt=dtype):
        pads.append(padded_rows(M, d, dt))
        return pads[-1][1]

    def flat(n=M):
        pads.append(padded_flat(n, torch.float32))
        return pads[-1][1]

    q = lambda t: t.data_ptr()
    pp = lambda default: default if p is None else p
    nb = lib.vlpet_sublayer_tail_partials(M)
    part = lambda: flat(nb * 2 * d).view(nb, 2, d)
    o = {}
    if op == "fwd_ln":
        o = dict(out=rows(), h=rows(), mean=flat(), rstd=flat(), keep=rows(torch.uint8))
        rc = lib.vlpet_sublayer_tail_fwd(P("y"), P("x1"), P("gamma"), P("beta"), q(o["out"]), q(o["h"]), q(o["mean"]), q(o["rstd"]),
                                         q(o["keep"]), M, d, T.EPS, pp(T.P0), T.SEED, 1, io, st)
    elif op == "fwd_ln_p0":
        o = dict(out=rows(), mean=flat(), rstd=flat())
        rc = lib.vlpet_sublayer_tail_fwd(P("y"), P("x1"), P("gamma"), None, q(o["out"]), None, q(o["mean"]), q(o["rstd"]), None, M, d,
                                         T.EPS, 0.0, T.SEED, 1, io, st)
    elif op == "fwd_res":
        o = dict(out=rows(), keep=rows(torch.uint8))
        rc = lib.vlpet_sublayer_tail_fwd(P("y"), P("x1"), None, None, q(o["out"]), None, None, None, q(o["keep"]), M, d, T.EPS,
                                         pp(0.5), T.SEED + 1, 0, io, st)
    elif op == "post":
        o = dict(out=rows(), mean=flat(), rstd=flat())
        rc = lib.vlpet_norm_residual_fwd(P("y"), P("x1"), P("gamma"), P("beta"), q(o["out"]), q(o["mean"]), q(o["rstd"]), M, d, T.EPS,
                                         io, st)
    elif op == "rms_fwd":
        o = dict(out=rows(), rstd=flat())
        rc = lib.vlpet_rmsnorm_fwd(P("x1"), P("gamma"), q(o["out"]), q(o["rstd"]), M, d, T.EPS, io, st)
    elif op in ("rms2_fwd", "rms2_fwd_p0"):
        o = dict(sum=rows(), normed=rows(), rstd=flat())
        rc = lib.vlpet_sublayer_tail_rms_fwd(P("y"), P("x1"), P("gamma2"), q(o["sum"]), q(o["normed"]), q(o["rstd"]), M, d, T.EPS,
                                             pp(T.P0) if op == "rms2_fwd" else 0.0, T.SEED, io, st)
    elif op == "bwd_ln":
        o = dict(dx1=rows(), dy=rows(), partials=part())
        rc = lib.vlpet_sublayer_tail_bwd(P("dout"), P("h"), P("mean"), P("rstd"), P("gamma"), q(o["dx1"]), q(o["dy"]), q(o["partials"]),
                                         M, d, pp(T.P0), T.SEED, 1, io, st)
    elif op == "bwd_ln_p0":
        o = dict(dx1=rows())
        rc = lib.vlpet_sublayer_tail_bwd(P("dout"), P("h"), P("mean"), P("rstd"), P("gamma"), q(o["dx1"]), None, None, M, d, 0.0,
                                         T.SEED, 1, io, st)
    elif op == "bwd_res":
        o = dict(dy=rows())
        rc = lib.vlpet_sublayer_tail_bwd(P("dout"), None, None, None, None, None, q(o["dy"]), None, M, d, pp(0.5), T.SEED + 1, 0, io, st)
    elif op == "bwd_res_p0":
        o = dict(dx1=rows())
        rc = lib.vlpet_sublayer_tail_bwd(P("dout"), None, None, None, None, q(o["dx1"]), None, None, M, d, 0.0, T.SEED, 0, io, st)
    elif op == "bwd_out":
        o = dict(dx1=rows(), dy=rows(), partials=part())
        rc = lib.vlpet_sublayer_tail_bwd_out(P("dout"), P("out"), P("rstd"), P("gamma"), P("beta"), q(o["dx1"]), q(o["dy"]),
                                             q(o["partials"]), M, d, pp(T.P0), T.SEED, io, st)
    elif op == "bwd_xhat":
        o = dict(dx1=rows(), partials=part())
        rc = lib.vlpet_layernorm_bwd_xhat(P("dout"), P("xhat"), P("rstd"), P("gamma"), q(o["dx1"]), q(o["partials"]), M, d, io, st)
    elif op == "rms_bwd":
        o = dict(dx1=rows(), partials=part())
        rc = lib.vlpet_rmsnorm_bwd(P("dout"), P("sum"), P("rstd2"), P("gamma2"), P("dres"), q(o["dx1"]), q(o["partials"]), M, d, io, st)
    elif op == "rms_bwd_plain":
        o = dict(dx1=rows())
        rc = lib.vlpet_rmsnorm_bwd(P("dout"), P("sum"), P("rstd2"), P("gamma2"), None, q(o["dx1"]), None, M, d, io, st)
    elif op == "rms_tail_bwd":
        o = dict(dx1=rows(), dy=rows(), partials=part())
        rc = lib.vlpet_rmsnorm_tail_bwd(P("dout"), P("sum"), P("rstd2"), P("gamma2"), P("dres"), q(o["dx1"]), q(o["dy"]),
                                        q(o["partials"]), M, d, pp(T.P0), T.SEED, io, st)
    elif op == "rms_tail_bwd_plain":
        o = dict(dx1=rows())
        rc = lib.vlpet_rmsnorm_tail_bwd(P("dout"), P("sum"), P("rstd2"), P("gamma2"), None, q(o["dx1"]), None, None, M, d, 0.0,
                                        T.SEED, io, st)
    else:
        assert op == "colsum"
        ws = flat(nb * d)
        o = dict(out=flat(d))
        rc = lib.vlpet_colsum(P("dout"), M, d, q(ws), q(o["out"]), io, st)
    assert rc == 0, (op, rc)
    return o, pads


def _hold(op, I, outs, pads, dtype, log, tag="", **spec_kw):
    """Every output of one call against the spec, element by element; the mask bit for bit; the sentinels."""
    ref = T.spec_op(op, I, **spec_kw)
    assert set(ref) == set(outs), (op, set(ref), set(outs))
    bad = []
    for name, (v, e, kind) in ref.items():
        got = outs[name]
        if kind == "mask":
            assert torch.equal(got.cpu() != 0, v) and bool((got <= 1).all()), (op, name, "keep_out is not dropout_spec.keep_mask")
            continue
        if T.check(f"{tag}{name}", got, v, e, kind, dtype, log):
            bad.append(log[-1])
        if name == "dy":         # exactly zero where the spec drops (no dout element is zero: a kept one cannot be)
            assert bool((got.cpu()[v == 0] == 0).all()) and bool((got.cpu()[v != 0] != 0).all()), (op, "dy and the spec's mask differ")
    assert not bad, (op, "elements over their bound; worst err/bound", bad)
    assert all(pad_intact(buf, body) for buf, body in pads), (op, "a write behind the output")
    return ref


def _reduce(outs, ref, d, dtype, log):
    """vlpet_sublayer_tail_reduce on the partials the backward just wrote, against the fp64 sum of those partials."""
    _, lib = _lib()
    part = outs["partials"]
    nb = part.shape[0]
    gbuf, dg = padded_flat(d, torch.float32)
    bbuf, db = padded_flat(d, torch.float32)
    assert lib.vlpet_sublayer_tail_reduce(part.data_ptr(), nb, d, dg.data_ptr(), db.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    r = T.sublayer_tail_reduce(part, d)
    bad = T.check("dgamma", dg, r.dgamma, r.e_dgamma, "f32", dtype, log) + T.check("dbeta", db, r.dbeta, r.e_dbeta, "f32", dtype, log)
    assert not bad and pad_intact(gbuf, dg) and pad_intact(bbuf, db), log[-2:]


def test_the_caps_are_where_the_rows_assume():
    """A changed cap must fail here, not silently stop ROWS from reaching the row loop."""
    _, lib = _lib()
    for M, nb in BLOCKS.items():
        assert lib.vlpet_sublayer_tail_partials(M) == nb == T.tail_blocks(M), M
    assert lib.vlpet_sublayer_tail_partials(10 ** 6) == 1024 and lib.vlpet_sublayer_tail_partials(0) == 0
    assert lib.vlpet_sublayer_tail_partials(8504) == 1024 and lib.vlpet_sublayer_tail_partials(2504) == 512
    assert set(ROWS) <= set(BLOCKS) and 8501 > 2 * 1024 * 4 and 8501 % (1024 * 4) != 0        # three rows per wave, ragged
    assert 1025 == 256 * 4 + 1 and 8500 > 4 * 512 * 4                                        # first wave with two rows; five with 512


def test_every_form_of_the_table_is_reached():
    """The host restatement of tail_pieces8 / launch_io / launch_np gives the annotated form at every width, and the widths reach
    every (IO, PB, NP, FULL) that can be chosen (the 8-byte forms with 2 and 4 pieces per lane cannot: see the profile)."""
    reach = {dt: set() for dt in FORMS}
    for dt in FORMS:
        for d, f in FORMS[dt].items():
            assert T.form(dt, d) == f, (dt, d)
            reach[dt].add(f)
            if f[2]:
                reach[dt].add((f[0], f[1], False))                 # the same width with parameters at a 4-byte offset
        choosable = set()
        for d in range(8, 4097, 8):
            g = T.form(dt, d)
            if g is not None:
                choosable |= {g, (g[0], g[1], False)}
        assert reach[dt] == choosable, dt
    assert [d for d in WIDTHS[BF] if FORMS[BF][d][2]] == FULL_WIDTHS and not any(f[2] for f in FORMS[F32].values())
    assert reach[BF] >= {(8, 3, False), (8, 3, True), (16, 3, False), (16, 3, True), (16, 8, False)}
    assert reach[F32] == {(16, n, False) for n in (1, 2, 3, 4, 8)}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tail_entry_point_matches_its_statement(case):
    dtype, M, d, op = case
    I, G = _inputs(dtype, M, d)
    log = []
    outs, pads = _run(op, G, M, d, dtype)
    ref = _hold(op, I, outs, pads, dtype, log)
    if "partials" in outs:
        _reduce(outs, ref, d, dtype, log)
    print("TAIL worst err/bound", _id(case), " ".join(log))


FWD_OPS = ["fwd_ln", "fwd_ln_p0", "post", "rms_fwd", "rms2_fwd", "rms2_fwd_p0"]


@pytest.mark.parametrize("d", FULL_WIDTHS)
def test_both_parameter_alignments(d):
    """gamma / beta / gamma_next 16-byte aligned (FULL) and at a 4-byte offset, as a view into a flat parameter buffer may be (the
    bounds-checked form with element loads): both to the spec, and their bits compared.  The forward forms agreed bit for bit at
    every width and row count when this was first run, so that is asserted; the backward forms do not (a few elements per
    thousand differ in the last bf16 place: the two instantiations are compiled to different fused multiply-add groupings), so
    they are held to the spec alone and the count of differing elements is printed (profiles/tail_edges_tests.md)."""
    differ = {}
    for M in (5, 1029):
        I, G = _inputs(BF, M, d)
        for op in NORM_OPS:
            log = []
            a, pa = _run(op, G, M, d, BF)
            b, pb = _run(op, G, M, d, BF, mis=True)
            _hold(op, I, a, pa, BF, log, tag="aligned.")
            _hold(op, I, b, pb, BF, log, tag="offset.")
            n = sum(int((a[k] != b[k]).sum()) for k in a)
            if op in FWD_OPS:
                assert all(torch.equal(a[k], b[k]) for k in a), (op, M, "FULL and non-FULL forward bits differ")
            elif n:
                differ[(M, op)] = n
    print("TAIL FULL against non-FULL: forward bits equal; backward elements that differ", d, differ or "none")


@pytest.mark.parametrize("dtype,d", [(dt, d) for dt in (BF, F32) for d in WIDTHS[dt]], ids=lambda v: str(v).replace("torch.", ""))
def test_same_bits_twice_and_whatever_the_row_count(dtype, d):
    """Two calls give equal bits; rows [0, 5) of every row output (and their statistics) do not depend on M (5 against 1029: two
    workgroups against 256 with a second row for some waves)."""
    I5, G5 = _inputs(dtype, 5, d)
    I, G = _inputs(dtype, 1029, d)
    assert torch.equal(I5["x1"], I["x1"][:5]) and torch.equal(I5["h"], I["h"][:5]) and torch.equal(I5["rstd2"], I["rstd2"][:5])
    for op in T.OPS:
        if op == "colsum":
            continue
        a, _ = _run(op, G, 1029, d, dtype)
        b, _ = _run(op, G, 1029, d, dtype)
        s, _ = _run(op, G5, 5, d, dtype)
        for k in a:
            assert torch.equal(a[k], b[k]), (op, k, "two calls differ")
            if k != "partials":
                assert torch.equal(a[k][:5], s[k]), (op, k, "rows [0, 5) depend on M")


P_THR1, P_CLAMP = 2.0 ** -16, 0.99999


@pytest.mark.parametrize("ctr", [None, 1])
@pytest.mark.parametrize("dtype,d", [(BF, 520), (BF, 760), (BF, 768), (BF, 1032), (F32, 520), (F32, 768)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_dropout_rates_and_the_step_counter(dtype, d, ctr):
    """p = 0.1, 0.5, the smallest rate that drops at all (threshold 1), the clamp (threshold 65,535); the seed counter unset and 1.
    The widths are those where lanes 2j / 2j + 1 share a generator call with an odd piece count and a ragged group, and their
    neighbours.  (p = 0 is every *_p0 operation of the main test.)"""
    assert T.DS.tail_thr(P_THR1) == 1 and T.DS.tail_thr(P_CLAMP) == 65535 and T.DS.tail_thr(0.999995) == 65535
    _, lib = _lib()
    M = 37
    I, G = _inputs(dtype, M, d)
    c = None
    if ctr is not None:
        c = torch.tensor([ctr], dtype=torch.int64, device="cuda")
        assert lib.vlpet_set_seed_counter(c.data_ptr()) == 0
    try:
        for p in (0.1, 0.5, P_THR1, P_CLAMP):
            log = []
            for op in DROP_OPS:
                outs, pads = _run(op, G, M, d, dtype, p=p)
                ref = _hold(op, I, outs, pads, dtype, log, tag=op + ".", p=p, ctr=ctr)
                if "keep" in ref and ctr is not None and p in (0.1, 0.5):
                    assert not torch.equal(ref["keep"][0], T.spec_op(op, I, p=p)["keep"][0])
            print("TAIL dropout worst err/bound", _dn(dtype), d, p, ctr, " ".join(log))
        torch.cuda.synchronize()
    finally:
        lib.vlpet_set_seed_counter(None)
    del c


def _extreme_inputs(dtype, d):
    """Rows 0..: constant (variance 0); common offset 1e3 with unit spread; |h| in the hundreds; the rest as usual."""
    I = T.make_inputs(dtype, 8, d)
    I["x1"][0] = 1.5
    I["y"][0] = 0.0
    I["x1"][1] = (1000.0 + T._rn(20, d, d)).to(dtype)
    I["y"][1] = T._nonzero(0.25 * T._rn(21, d, d)).to(dtype)
    I["x1"][2] = (300.0 * T._rn(22, d, d)).to(dtype)
    I["y"][2] = T._nonzero(200.0 * T._rn(23, d, d)).to(dtype)
    return T.derive_saved(I, dtype)


@pytest.mark.parametrize("dtype,d", [(BF, 768), (BF, 760), (F32, 768), (F32, 520)], ids=lambda v: str(v).replace("torch.", ""))
def test_extreme_rows(dtype, d):
    I = _extreme_inputs(dtype, d)
    G = _to_gpu(I, d)
    log = []
    for op in T.OPS:
        if op == "colsum":
            continue
        outs, pads = _run(op, G, 8, d, dtype)
        ref = T.spec_op(op, I)
        for name, (v, e, kind) in ref.items():
            if kind != "mask":
                assert T.check(f"{op}.{name}", outs[name], v, e, kind, dtype, log) == 0, log[-1]
        assert all(pad_intact(buf, body) for buf, body in pads)
        if op == "post":        # the constant row: variance 0, the norm's output is beta, rstd = rsqrt(eps)
            r0 = ref["rstd"][0][0]
            assert abs(float(outs["rstd"][0]) - float(r0)) <= float(ref["rstd"][1][0]) and abs(float(r0) - T.EPS ** -0.5) < 1e-9
    # (the constant row sits in y for the post-norm form: statistics of y alone)
    I2 = dict(I, y=I["x1"], x1=I["y"])
    o2, _ = _run("post", _to_gpu(I2, d), 8, d, dtype)
    r2 = T.spec_op("post", I2)
    assert T.check("post.const", o2["out"], r2["out"][0], r2["out"][1], "row", dtype, log) == 0
    assert torch.equal(r2["out"][0][0], I["beta"].double() + I2["x1"][0].double())
    # gamma with zeros in the from-output backward: finite everywhere, every column to its bound (xhat and g are 0 where gamma is)
    I3 = dict(I, gamma=I["gamma"].clone())
    I3["gamma"][::7] = 0.0
    I3 = T.derive_saved(I3, dtype)
    o3, p3 = _run("bwd_out", _to_gpu(I3, d), 8, d, dtype)
    assert all(bool(torch.isfinite(t).all()) for t in o3.values())
    _hold("bwd_out", I3, o3, p3, dtype, log, tag="gamma0.")
    print("TAIL extreme rows worst err/bound", _dn(dtype), d, " ".join(log))


COLSUM_WIDTHS = {BF: [16, 528, 1040, 2064], F32: [16, 272, 528, 1040]}       # a ragged last group at 1, 2, 4, 8 pieces per lane


@pytest.mark.parametrize("M", [5, 1029])
@pytest.mark.parametrize("dtype", [BF, F32], ids=_dn)
def test_colsum_ragged_widths(dtype, M):
    log = []
    for n in COLSUM_WIDTHS[dtype]:
        x = T._nonzero(T._rn(2, n, M, n) + 0.5).to(dtype)
        I = dict(x1=x, dout=x)
        outs, pads = _run("colsum", dict(dout=x.cuda()), M, n, dtype)
        _hold("colsum", I, outs, pads, dtype, log, tag=f"{n}.")
    print("TAIL colsum ragged worst err/bound", _dn(dtype), M, " ".join(log))


def test_refusals_launch_nothing():
    """Shape, NULL, alignment, dtype and rate refusals; every output stays NaN (nothing was launched)."""
    L, lib = _lib()
    st = torch.cuda.current_stream().cuda_stream
    M, dmax = 6, 4104
    row = lambda: torch.randn(M, dmax, device="cuda")
    t = dict(y=row(), x1=row(), dout=row(), h=row(), gamma=torch.randn(dmax, device="cuda"), beta=torch.randn(dmax, device="cuda"),
             mean=torch.randn(M, device="cuda"), rstd=torch.rand(M, device="cuda") + 0.5)
    nan_rows = lambda: torch.full((M, dmax), float("nan"), device="cuda")
    outs = dict(o1=nan_rows(), o2=nan_rows(), s1=torch.full((M,), float("nan"), device="cuda"), s2=torch.full((M,), float("nan"), device="cuda"),
                part=torch.full((2, 2, dmax), float("nan"), device="cuda"))
    t.update(outs)
    p = lambda k: t[k].data_ptr()

    def calls(M=M, d=64, io=L.VLPET_BF16, rate=0.1):
        """name -> (function, arguments, required pointers, row operands)"""
        tail, ptail = [M, d], [M, d, rate, 7]
        return {
            "fwd": (lib.vlpet_sublayer_tail_fwd, [p("y"), p("x1"), p("gamma"), p("beta"), p("o1"), p("o2"), p("s1"), p("s2"), None] + tail
                    + [1e-5, rate, 7, 1, io, st], [0, 1, 2, 4, 6, 7], [0, 1, 4, 5]),
            "post": (lib.vlpet_norm_residual_fwd, [p("y"), p("x1"), p("gamma"), p("beta"), p("o1"), p("s1"), p("s2")] + tail + [1e-5, io, st],
                     [0, 1, 2, 4, 5, 6], [0, 1, 4]),
            "rms_fwd": (lib.vlpet_rmsnorm_fwd, [p("x1"), p("gamma"), p("o1"), p("s1")] + tail + [1e-5, io, st], [0, 1, 2, 3], [0, 2]),
            "rms2_fwd": (lib.vlpet_sublayer_tail_rms_fwd, [p("y"), p("x1"), p("gamma"), p("o1"), p("o2"), p("s1")] + tail + [1e-5, rate, 7, io, st],
                         [0, 1, 2, 3, 4, 5], [0, 1, 3, 4]),
            "bwd": (lib.vlpet_sublayer_tail_bwd, [p("dout"), p("h"), p("mean"), p("rstd"), p("gamma"), p("o1"), p("o2"), p("part")] + ptail
                    + [1, io, st], [0, 1, 2, 3, 4, 5] + ([6] if rate else []), [0, 1, 5, 6]),
            "bwd_out": (lib.vlpet_sublayer_tail_bwd_out, [p("dout"), p("h"), p("rstd"), p("gamma"), p("beta"), p("o1"), p("o2"), p("part")]
                        + ptail + [io, st], [0, 1, 2, 3, 5] + ([6] if rate else []), [0, 1, 5, 6]),
            "bwd_xhat": (lib.vlpet_layernorm_bwd_xhat, [p("dout"), p("h"), p("rstd"), p("gamma"), p("o1"), p("part")] + tail + [io, st],
                         [0, 1, 2, 3, 4], [0, 1, 4]),
            "rms_bwd": (lib.vlpet_rmsnorm_bwd, [p("dout"), p("h"), p("rstd"), p("gamma"), p("x1"), p("o1"), p("part")] + tail + [io, st],
                        [0, 1, 2, 3, 5], [0, 1, 4, 5]),
            "rms_tail_bwd": (lib.vlpet_rmsnorm_tail_bwd, [p("dout"), p("h"), p("rstd"), p("gamma"), p("x1"), p("o1"), p("o2"), p("part")]
                             + ptail + [io, st], [0, 1, 2, 3, 5] + ([6] if rate else []), [0, 1, 4, 5, 6]),
        }

    has_rate = ("fwd", "rms2_fwd", "bwd", "bwd_out", "rms_tail_bwd")
    for name in calls():
        def call(edit=None, **kw):
            fn, args, _, _ = calls(**kw)[name]
            if edit:
                edit(args)
            return fn(*args)

        assert call(d=4104) == E_SHAPE and call(d=2056, io=L.VLPET_F32) == E_SHAPE, name          # more than 8 x 64 pieces
        assert call(d=12) == E_SHAPE and call(d=12, io=L.VLPET_F32) == E_SHAPE and call(d=68) == E_SHAPE and call(d=0) == E_SHAPE, name
        assert call(M=0) == E_SHAPE and call(M=-3) == E_SHAPE, name
        assert call(io=7) == E_DTYPE, name
        _, _, required, rows = calls()[name]
        for i in required:
            assert call(edit=lambda a, i=i: a.__setitem__(i, None)) == E_NULL, (name, i)
        for i in rows:           # a row operand offset by 8 bytes
            assert call(edit=lambda a, i=i: a.__setitem__(i, a[i] + 8)) == E_ALIGN, (name, i)
        if name in has_rate:
            for bad in (1.0, -0.1, 1.5, float("nan")):
                assert call(rate=bad) == E_SHAPE, (name, bad)
    # the plain residual backward: dx1 may be NULL only under dropout; dropout needs dy
    res = lambda dx1, dy, rate: lib.vlpet_sublayer_tail_bwd(p("dout"), None, None, None, None, dx1, dy, None, M, 64, rate, 7, 0, L.VLPET_BF16, st)
    assert res(None, None, 0.0) == E_NULL and res(p("o1"), None, 0.1) == E_NULL
    assert lib.vlpet_sublayer_tail_fwd(p("y"), p("x1"), p("gamma"), p("beta"), p("o1"), None, p("s1"), p("s2"), None, M, 64, 1e-5, 0.1, 7, 2,
                                       L.VLPET_BF16, st) == E_SHAPE                              # norm_mode 2
    assert lib.vlpet_sublayer_tail_reduce(None, 2, 64, p("s1"), p("s2"), st) == E_NULL
    assert lib.vlpet_sublayer_tail_reduce(p("part"), 2, 64, None, None, st) == E_NULL
    assert lib.vlpet_sublayer_tail_reduce(p("part"), 0, 64, p("s1"), p("s2"), st) == E_SHAPE
    assert lib.vlpet_colsum(p("dout"), M, 72, p("part"), p("s1"), L.VLPET_BF16, st) == E_SHAPE        # n % 16
    assert lib.vlpet_colsum(p("dout"), M, 4112, p("part"), p("s1"), L.VLPET_BF16, st) == E_SHAPE
    assert lib.vlpet_colsum(None, M, 64, p("part"), p("s1"), L.VLPET_BF16, st) == E_NULL
    assert lib.vlpet_colsum(p("dout") + 8, M, 64, p("part"), p("s1"), L.VLPET_BF16, st) == E_ALIGN
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs.values())


def _flat_norms(dtype):
    """Two LayerNorm(768) whose parameters are views of ONE flat buffer (train.FlatGrads(flatten_params=True), no padding between
    parameters): a 1-element parameter in front puts the first at a 4-byte offset, three more elements put the second on 16 bytes.
    (The tiny-BART layout has no misaligned LayerNorm: every trainable parameter in front of one has a multiple of 4 elements.)"""
    import vlpet_amd.train as TR

    class Fill(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.v = torch.nn.Parameter(torch.zeros(n))

    class Holder(torch.nn.Module):          # (FlatGrads keeps the registration order of submodules)
        def __init__(self):
            super().__init__()
            self.a_scalar, self.b_norm, self.c_fill, self.d_norm = Fill(1), torch.nn.LayerNorm(768), Fill(3), torch.nn.LayerNorm(768)

    m = Holder().cuda()
    I = T.make_inputs(dtype, 37, 768)
    with torch.no_grad():
        for ln in (m.b_norm, m.d_norm):
            ln.weight.copy_(I["gamma"])
            ln.bias.copy_(I["beta"])
    fg = TR.FlatGrads(m, flatten_params=True)
    assert fg.flat_p.data_ptr() % 16 == 0 and fg.slices == [(0, 1), (1, 769), (769, 1537), (1537, 1540), (1540, 2308), (2308, 3076)]
    return m, fg, I


@pytest.mark.parametrize("dtype", [BF, F32], ids=_dn)
def test_layernorm_inside_a_flat_parameter_buffer(dtype):
    """tail.sublayer_tail forward + backward on a LayerNorm whose gamma / beta sit at a 4-byte offset of the trainer's flat parameter
    buffer, and on one at a 16-byte offset: the output and all five gradients to the spec."""
    from vlpet_amd import functional as VF
    from vlpet_amd import tail as TL
    m, fg, I = _flat_norms(dtype)
    offs = {n: (ln.weight.data_ptr() % 16, ln.bias.data_ptr() % 16) for n, ln in (("b_norm", m.b_norm), ("d_norm", m.d_norm))}
    assert offs["b_norm"] == (4, 4) and offs["d_norm"] == (0, 0), offs
    M, d = 37, 768
    log = []
    old = TL.SAVE_PRENORM
    try:
        for prenorm in (True, False):           # the backward from the saved sum, and from the output rows
            TL.SAVE_PRENORM = prenorm
            for name in ("b_norm", "d_norm"):
                ln = getattr(m, name)
                x1 = I["x1"].cuda().view(1, M, d).requires_grad_(True)
                y = I["y"].cuda().view(1, M, d).requires_grad_(True)
                out = TL.sublayer_tail(x1, y, ln, p=T.P0, training=True, seed=T.SEED)
                sv = [t.cpu() if t is not None else None for t in out.grad_fn.saved_tensors[:3]]      # (freed by the backward)
                gx1, gy, gg, gb = torch.autograd.grad(out, [x1, y, ln.weight, ln.bias], I["dout"].cuda().view(1, M, d))
                VF.flush_reduces()
                f = T.spec_op("fwd_ln", I)
                assert T.check(f"{name}.out", out.view(M, d), f["out"][0], f["out"][1], "row", dtype, log) == 0, log[-1]
                # the backward's inputs are what the forward left: its own output or saved sum, and its statistics
                Ib = dict(I, mean=sv[1], rstd=sv[2], **{"h" if prenorm else "out": sv[0]})
                b = T.spec_op("bwd_ln" if prenorm else "bwd_out", Ib)
                assert T.check(f"{name}.dx1", gx1.view(M, d), b["dx1"][0], b["dx1"][1], "row", dtype, log) == 0, log[-1]
                assert T.check(f"{name}.dy", gy.view(M, d), b["dy"][0], b["dy"][1], "row", dtype, log) == 0, log[-1]
                pv, pe, _ = b["partials"]
                r = T.sublayer_tail_reduce(pv, d)
                e = pe.sum(0) + torch.stack([r.e_dgamma, r.e_dbeta])
                assert T.check(f"{name}.dgamma", gg, r.dgamma, e[0], "f32", dtype, log) == 0, log[-1]
                assert T.check(f"{name}.dbeta", gb, r.dbeta, e[1], "f32", dtype, log) == 0, log[-1]
    finally:
        TL.SAVE_PRENORM = old
    print("TAIL flat-buffer LayerNorm worst err/bound", _dn(dtype), " ".join(log))
