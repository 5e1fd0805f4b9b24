"""CPU: tests/tail_spec.py tied down from three sides.

* It IS the operation: the forward functions equal oracle.vlpet_oracle.bart_sublayer_tail / t5_sublayer_tail (and F.layer_norm / the
  T5 RMS form for the other entry points), the backward functions equal fp64 autograd of the same expressions.  The from-output and
  from-xhat forms are fed the exact (unrounded) out / xhat here: what rounding them costs is the forward's business.
* The bounds can be met: the same formulas in fp32 torch on the same inputs -- the reference alone, in another summation order --
  stay inside every bound that tests/test_gpu_tail_edges.py uses, at every width it uses.
* The bounds can be missed: each listed mis-statement of the spec leaves elements outside them at the suite's own inputs."""
import pytest
import torch
import torch.nn.functional as F

import tail_spec as T
from oracle import vlpet_oracle as O

BF, F32 = torch.bfloat16, torch.float32
WIDTHS = {BF: [8, 248, 256, 264, 512, 520, 760, 768, 776, 1024, 1032, 1536, 1544, 2048, 2056, 4096],
          F32: [8, 256, 264, 512, 520, 768, 776, 1024, 1032, 2048]}
M, D = 7, 72
TOL = dict(rtol=1e-11, atol=1e-11)


def _exact():
    """fp64 inputs (nothing rounded) for the oracle / autograd comparisons"""
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(y=rn(M, D), x1=rn(M, D) + 2 * rn(M, 1), dout=rn(M, D) + 0.5, dres=rn(M, D), gamma=1 + 0.3 * rn(D), beta=0.5 * rn(D))


def _close(a, b):
    torch.testing.assert_close(a, b, **TOL)


# ---------------------------------------------------------------------------------------------------- oracle and autograd
def test_forward_is_the_oracle():
    I = _exact()
    r = T.sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], I["beta"], T.EPS, 0.0, 0, 1)
    _close(r.out, O.bart_sublayer_tail(I["x1"], I["y"], I["gamma"], I["beta"], T.EPS))
    _close(r.h, I["x1"] + I["y"])
    _close(r.mean, (I["x1"] + I["y"]).mean(1))
    _close(r.rstd, ((I["x1"] + I["y"]).var(1, unbiased=False) + T.EPS).rsqrt())
    _close(T.sublayer_tail_fwd(I["y"], I["x1"], None, None, T.EPS, 0.0, 0, 0).out, O.t5_sublayer_tail(I["x1"], I["y"]))
    _close(T.sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], None, T.EPS, 0.0, 0, 1).out,
           F.layer_norm(I["x1"] + I["y"], (D,), I["gamma"], None, T.EPS))
    _close(T.norm_residual_fwd(I["y"], I["x1"], I["gamma"], I["beta"], T.EPS).out,
           F.layer_norm(I["y"], (D,), I["gamma"], I["beta"], T.EPS) + I["x1"])
    rms = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + T.EPS) * w       # T5LayerNorm
    _close(T.rmsnorm_fwd(I["x1"], I["gamma"], T.EPS).out, rms(I["x1"], I["gamma"]))
    s = T.sublayer_tail_rms_fwd(I["y"], I["x1"], I["gamma"], T.EPS, 0.0, 0)
    _close(s.sum, I["x1"] + I["y"])
    _close(s.normed, rms(I["x1"] + I["y"], I["gamma"]))


def test_forward_dropout_is_the_spec_mask_scaled():
    I = _exact()
    for p in (0.1, 0.5):
        k = T.keep_mask(M, D, T.SEED, p).double()
        r = T.sublayer_tail_fwd(I["y"], I["x1"], None, None, T.EPS, p, T.SEED, 0)
        _close(r.out, I["x1"] + I["y"] * k * float(T.DS.keep_scale(p)))
        assert torch.equal(r.keep.double(), k) and 0 < k.mean() < 1
    assert not torch.equal(T.keep_mask(M, D, T.SEED, 0.5), T.keep_mask(M, D, T.SEED, 0.5, ctr=1))


def test_rms2_statistic_reads_the_rounded_sum():
    I = T.make_inputs(BF, 5, 72)
    s = T.sublayer_tail_rms_fwd(I["y"], I["x1"], I["gamma2"], T.EPS, 0.0, 0)
    hr = (I["x1"].double() + I["y"].double()).float().to(BF).double()
    _close(s.rstd, torch.rsqrt(hr.pow(2).mean(1) + T.EPS))
    _close(s.normed, hr * s.rstd[:, None] * I["gamma2"].double())
    assert not torch.equal(hr, s.sum)


def _autograd(fn, *leaves, dout):
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    fn(*leaves).backward(dout)
    return [t.grad for t in leaves]


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_layernorm_backward_forms_are_autograd(p):
    I = _exact()
    sc = float(T.DS.keep_scale(p)) if p else 1.0
    k = T.keep_mask(M, D, T.SEED, p).double()
    f = lambda y, x1, g, b: F.layer_norm(x1 + y * k * sc, (D,), g, b, T.EPS)
    dy, dx1, dg, db = _autograd(f, I["y"], I["x1"], I["gamma"], I["beta"], dout=I["dout"])
    fw = T.sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], I["beta"], T.EPS, p, T.SEED, 1)
    xhat = (fw.h - fw.mean[:, None]) * fw.rstd[:, None]
    forms = [T.sublayer_tail_bwd(I["dout"], fw.h, fw.mean, fw.rstd, I["gamma"], p, T.SEED, 1),
             T.sublayer_tail_bwd_out(I["dout"], fw.out, fw.rstd, I["gamma"], I["beta"], p, T.SEED)]
    if not p:
        forms.append(T.layernorm_bwd_xhat(I["dout"], xhat, fw.rstd, I["gamma"]))
    for r in forms:
        _close(r.dx1, dx1)
        _close(r.dy, dy)
        _close(r.dg_rows.sum(0), dg)
        _close(r.db_rows.sum(0), db)
        for nb in (1, 2):
            pt = torch.stack([T.block_partials(r.dg_rows, nb), T.block_partials(r.db_rows, nb)], 1)
            red = T.sublayer_tail_reduce(pt, D)
            _close(red.dgamma, dg)
            _close(red.dbeta, db)
    r0 = T.sublayer_tail_bwd(I["dout"], None, None, None, None, p, T.SEED, 0)
    dy0, dx0 = _autograd(lambda y, x1: x1 + y * k * sc, I["y"], I["x1"], dout=I["dout"])
    _close(r0.dx1, dx0)
    _close(r0.dy, dy0)


def test_from_output_form_zero_gamma():
    I = _exact()
    I["gamma"][::5] = 0.0
    fw = T.sublayer_tail_fwd(I["y"], I["x1"], I["gamma"], I["beta"], T.EPS, 0.0, 0, 1)
    r = T.sublayer_tail_bwd_out(I["dout"], fw.out, fw.rstd, I["gamma"], I["beta"], 0.0, 0)
    assert bool(torch.isfinite(r.dx1).all()) and bool((r.dg_rows[:, ::5] == 0).all())


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_rms_backward_forms_are_autograd(p):
    I = _exact()
    sc = float(T.DS.keep_scale(p)) if p else 1.0
    k = T.keep_mask(M, D, T.SEED, p).double()
    rms = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + T.EPS) * w
    s = I["x1"] + I["y"] * k * sc
    rstd = torch.rsqrt(s.pow(2).mean(1) + T.EPS)
    dx, dg = _autograd(rms, s, I["gamma"], dout=I["dout"])
    r = T.rmsnorm_bwd(I["dout"], s, rstd, I["gamma"])
    _close(r.dx1, dx)
    _close(r.dg_rows.sum(0), dg)
    _close(T.rmsnorm_bwd(I["dout"], s, rstd, I["gamma"], I["dres"]).dx1, dx + I["dres"])
    dy, dx1, dg2 = _autograd(lambda y, x1, g: rms(x1 + y * k * sc, g), I["y"], I["x1"], I["gamma"], dout=I["dout"])
    for dsum in (None, I["dres"]):
        t = T.rmsnorm_tail_bwd(I["dout"], s, rstd, I["gamma"], dsum, p, T.SEED)
        add = 0 if dsum is None else dsum
        _close(t.dx1, dx1 + add)
        _close(t.dy, dy + add * k * sc)
        _close(t.dg_rows.sum(0), dg2)


def test_colsum_and_block_rows():
    I = _exact()
    _close(T.colsum(I["dout"], 2).out, I["dout"].sum(0))
    assert T.block_rows(11, 2).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert [T.tail_blocks(m) for m in (1, 5, 1024, 1025, 2500, 2501, 8500, 8501, 10 ** 6)] == [1, 2, 256, 256, 256, 512, 512, 1024, 1024]


# ---------------------------------------------------------------------------------------------------- the width table
FORMS = {BF: {8: (8, 1, False), 248: (8, 1, False), 256: (8, 1, True), 264: (16, 1, False), 512: (16, 1, True), 520: (8, 3, False),
              760: (8, 3, False), 768: (8, 3, True), 776: (16, 2, False), 1024: (16, 2, True), 1032: (16, 3, False),
              1536: (16, 3, True), 1544: (16, 4, False), 2048: (16, 4, True), 2056: (16, 8, False), 4096: (16, 8, False)},
         F32: {8: (16, 1, False), 256: (16, 1, False), 264: (16, 2, False), 512: (16, 2, False), 520: (16, 3, False),
               768: (16, 3, False), 776: (16, 4, False), 1024: (16, 4, False), 1032: (16, 8, False), 2048: (16, 8, False)}}


def test_width_table():
    for dt in (BF, F32):
        assert sorted(FORMS[dt]) == WIDTHS[dt]
        for d, f in FORMS[dt].items():
            assert T.form(dt, d) == f, (dt, d)
    assert T.form(BF, 4104) is None and T.form(F32, 2056) is None and T.form(BF, 100) is None
    # the 8-byte forms with 2 and 4 pieces per lane can never be chosen (np8 = 2 needs np16 >= 2, i.e. d > 512; np8 = 4 ties and loses)
    assert {T.form(BF, d)[1] for d in range(8, 4097, 8) if T.form(BF, d)[0] == 8} == {1, 3}


# ---------------------------------------------------------------------------------------------------- the bounds can be met
def _restate(dt, d, log):
    I = T.make_inputs(dt, 5, d)
    bad = []
    for op in T.OPS:
        if op == "colsum" and d % 16:
            continue
        ref, got = T.spec_op(op, I), T.spec_op(op, I, ct=F32)
        for name, (v, e, kind) in ref.items():
            if kind == "mask":
                continue
            g = got[name][0].to(dt) if kind == "row" else got[name][0]
            if T.check(f"{op}.{name}", g, v, e, kind, dt, log):
                bad.append(log[-1])
    return bad


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_fp32_restatement_stays_inside_every_bound(dt):
    for d in WIDTHS[dt]:
        log = []
        assert not _restate(dt, d, log), (d, log)
        print("TAIL restatement worst err/bound", "bf16" if dt == BF else "fp32", d, " ".join(log))


def test_rsqrt_allowance_is_four_times_the_cpu_figure():
    """The one ingredient that is measured: fp32 1 / sqrt (as tail_spec._stats states it) of the fp32 variance + eps against fp64, over every width and dtype of
    the suite, in units of u.  tail_spec.R_RSQRT allows the kernel 4 times RSQRT_CPU_WORST_U, and this holds the figure."""
    worst = 0.0
    for dt in (BF, F32):
        for d in WIDTHS[dt]:
            I = T.make_inputs(dt, 5, d)
            for v in (I["rstd"], I["rstd2"]):
                x = v.double() ** -2                                    # var + eps as fp32 numbers
                x32 = x.float()
                rel = (((1.0 / torch.sqrt(x32)).double() - x32.double() ** -0.5).abs() * x32.double() ** 0.5).max()
                worst = max(worst, float(rel) / T.U)
    print("TAIL rsqrt fp32 CPU worst relative error / u", f"{worst:.3f}")
    assert worst <= T.RSQRT_CPU_WORST_U and T.R_RSQRT == 4 * T.RSQRT_CPU_WORST_U * T.U


# ---------------------------------------------------------------------------------------------------- the bounds can be missed
def _misses(op, I, dt, names, **mutated):
    ref, got = T.spec_op(op, I), T.spec_op(op, I, **mutated)
    return sum(T.check(n, got[n][0], ref[n][0], ref[n][1], ref[n][2], dt, []) for n in names)


MUT_CASES = [(dt, d) for dt in (BF, F32) for d in (520, 768)]


@pytest.mark.parametrize("dt,d", MUT_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_every_listed_misstatement_is_caught(dt, d):
    I = T.make_inputs(dt, 5, d)
    caught = {}
    if T.padded_width(dt, d) != d:                    # a ragged width
        caught["padded_width"] = _misses("fwd_ln", I, dt, ["mean", "rstd", "out"], mut=("padded_width",))
        caught["last_piece"] = _misses("fwd_ln", I, dt, ["mean", "rstd", "out"], mut=("last_piece",))
        assert _misses("rms_fwd", I, dt, ["rstd"], mut=("padded_width",)) and _misses("rms2_fwd_p0", I, dt, ["rstd"], mut=("last_piece",))
    caught["uncentred"] = _misses("fwd_ln", I, dt, ["rstd", "out"], mut=("uncentred",))
    caught["c1_in_rms"] = min(_misses(op, I, dt, ["dx1"], mut=("c1_in_rms",)) for op in ("rms_bwd", "rms_tail_bwd"))
    for op, name in (("fwd_ln", "out"), ("fwd_res", "out"), ("rms2_fwd", "sum"), ("bwd_ln", "dy"), ("bwd_res", "dy"), ("bwd_out", "dy"),
                     ("rms_tail_bwd", "dy")):
        p = T.P0 if op in ("fwd_ln", "rms2_fwd", "bwd_ln", "bwd_out", "rms_tail_bwd") else 0.5
        k = T.keep_mask(5, d, T.SEED if p == T.P0 else T.SEED + 1, p)
        for mname, mk in (("mask_shift", T.shifted_mask(k)), ("mask_swap", T.swapped_mask(k))):
            caught[mname] = min(caught.get(mname, 1 << 30), _misses(op, I, dt, [name], keep=mk))
    caught["no_beta"] = _misses("bwd_out", I, dt, ["dx1", "partials"], mut=("no_beta",))
    pt = T.spec_op("bwd_ln", I)["partials"][0].float()
    ref, mis = T.sublayer_tail_reduce(pt, d), T.sublayer_tail_reduce(pt, d, mut=("partial_missing",))
    caught["partial_missing"] = int(((mis.dgamma - ref.dgamma).abs() > ref.e_dgamma).sum() + ((mis.dbeta - ref.dbeta).abs() > ref.e_dbeta).sum())
    if dt == BF:
        # (under dropout with 1 / (1 - p) = 10 / 9 about 2 % of the sums lie within 2 u of a bf16 rounding boundary, where the bound must
        # allow either neighbour: that honest slack is as large as this mis-statement.  Without dropout the fp32 sum is exact.)
        caught["rms2_unrounded"] = _misses("rms2_fwd_p0", I, dt, ["rstd"], mut=("rms2_unrounded",))
        assert caught["rms2_unrounded"] == 5
    print("TAIL mutations: elements outside their bound", dt, d, caught)
    assert all(v > 0 for v in caught.values()), caught
    want = set(T.MUTATIONS) - (set() if T.padded_width(dt, d) != d else {"padded_width", "last_piece"}) - (set() if dt == BF else {"rms2_unrounded"})
    assert set(caught) == want
