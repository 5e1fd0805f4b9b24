"""Edges of the short attention kernels (csrc/attn.hip through vlpet_amd.attention.short_attention): lengths on and next to the 32-row
tiles, odd numbers of (batch, head) pairs, either side of the backward's occupancy switch, causal with Lq != Lk, rows with no visible
key, -inf / offset / masked bias forms and softmax extremes -- each against tests/attn_spec.py's fp64 chain with the dropout mask
the kernel exported, under the project's tensor-wide bound AND a budget per 32-row tile (the kernels' work unit), so that a wrong
ragged tile or a wrong row of small magnitude cannot hide behind the tensor's largest element.

The per-tile budget: err_kernel <= max(3 * err_restated, 2^-7 * max|ref tile|, 2e-4), both errors against the fp64 reference, the
restated one (attn_spec.chain(rounded=True): the kernels' documented bf16 roundings in fp32) computed here at run time.  3: two
restatements with different summation orders differ by up to 1.86x per tile; 2^-7: two bf16 steps of the tile's largest value; 2e-4:
the existing absolute floor 2e-2 * 1e-2.

Every case is at most B = 3, H = 5, L = 128: each edge is a property of one pair or of the last workgroup.  One forward and one
backward per case, run once and shared by the tests that look at it.  Each case prints an ``EDGE |`` table row (pytest -s):
profiles/r13_attn_short_edges.md is one MI355X run's."""
import pytest
import torch

import attn_spec as S

pytestmark = pytest.mark.gpu

SEED = 99
_RESULTS = {}


def _gpu(q, k, v, do, km, causal, p, bias, scale, H, seed=SEED, fn=None):
    """one forward + backward on the GPU -> (out, dq, dk, dv) as [B, H, L, 64] on the CPU, the exported keep mask, the saved lse"""
    import vlpet_amd.attention as A
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    ab = None if bias is None else A.AttnBias(bias.cuda())
    res = (fn or A.short_attention)(qg, kg, vg, H, None if km is None else km.cuda(), causal, p, True, scale=scale, seed=seed,
                                    return_mask=p > 0, bias=ab)
    out, keep = res if p > 0 else (res, None)
    lse = None
    if fn is None:
        lse = out.grad_fn.saved_tensors[4].cpu()                # what _AttnFn keeps for its backward: [B, H, Lq], log2 units
    out.backward(do.cuda())
    torch.cuda.synchronize()
    got = [S.heads_first(t.detach().cpu(), H) for t in (out, qg.grad, kg.grad, vg.grad)]
    return got, (None if keep is None else keep.cpu().bool()), lse


def _result(case):
    """the case's kernel result, reference and restatement (with the exported mask), computed once"""
    if case.name not in _RESULTS:
        q, k, v, do, km, bias, scale = S.inputs(case)
        got, keep, lse = _gpu(q, k, v, do, km, case.causal, case.p, bias, scale, case.H)
        if keep is not None:
            assert keep.shape == (case.B, case.H, case.Lq, case.Lk)
        args = (q, k, v, do, km, case.causal, keep, case.p, bias, scale, case.H)
        ref = S.chain(*args, torch.float64, False)
        rst = S.chain(*args, torch.float32, True)
        _RESULTS[case.name] = dict(got=got, keep=keep, lse=lse, ref=ref, rst=rst, dead=S.dead_rows(q, k, km, case.causal, bias, case.H))
    return _RESULTS[case.name]


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_edge_case_within_the_tensor_wide_bound_and_the_per_tile_budget(case):
    R = _result(case)
    wide, worst, over = {}, 0.0, []
    for n, a, r, s in zip(S.NAMES, R["got"], R["ref"], R["rst"]):
        assert torch.isfinite(a.float()).all(), n                                         # (a)
        wide[n] = S.wide_error(n, a, r)
        e_k, mag = S.tile_errors(a, r)
        e_r, _ = S.tile_errors(s, r)
        ratio = e_k / S.tile_budget(e_r, mag)
        worst = max(worst, float(ratio.max()))
        if float(ratio.max()) > 1.0:
            b, h, t = (int(x) for x in (ratio == ratio.max()).nonzero()[0])
            over.append(f"{n}: tile (b {b}, h {h}, rows {32 * t}..) kernel {float(e_k[b, h, t]):.3e} restated {float(e_r[b, h, t]):.3e} "
                        f"max|ref| {float(mag[b, h, t]):.3e}")
    note = ""
    if case.zero:
        note = "  (zero-reference " + ", ".join(f"max|{n}| kernel {float(R['got'][S.NAMES.index(n)].float().abs().max()):.3e} restated "
                                                f"{float(R['rst'][S.NAMES.index(n)].abs().max()):.3e}" for n in case.zero) + ")"
    print(f"\nEDGE | {case.name} | " + " | ".join(f"{wide[n]:.2e}" for n in S.NAMES) + f" | {worst:.2f} |{note}")
    for n in S.NAMES:                                                                     # (b)
        if n in case.zero:      # reference identically zero, the value is delta's rounding noise: measured above, bounded per tile below
            assert float(R["ref"][S.NAMES.index(n)].abs().max()) <= 1e-12
            continue
        assert wide[n] <= S.TOL, (n, wide)
    assert not over, over                                                                 # (c)
    if case.zero_q:
        # q = 0: uniform rows.  dk = dS^T q is exactly zero in the reference, the restatement and the kernel's arithmetic (its Q image is
        # zero).  dq = dS k is not zero -- the uniform probabilities weigh keep * dP / (1 - p) - delta, not zero -- and stays under (b), (c).
        assert float(R["ref"][2].abs().max()) == 0.0 and float(R["rst"][2].abs().max()) == 0.0
        assert float(R["got"][2].float().abs().max()) <= S.FLOOR
        assert float(R["ref"][1].abs().max()) > 0.1


def test_a_constant_offset_of_the_bias_cancels():
    """the same bias + 300: the backward recomputes exp2(s * sc2 + kb - lse) and cancels the offset there; each run is checked against
    its own reference above, and the two outputs are within two bf16 steps of the largest output of each other"""
    a = _result(S.BY_NAME["1x3x56x56-p0.1-bias_plain"])
    b = _result(S.BY_NAME["1x3x56x56-p0.1-bias_plus300"])
    assert torch.equal(a["keep"], b["keep"])
    oa, ob = a["got"][0].double(), b["got"][0].double()
    d = float((oa - ob).abs().max())
    print(f"\nEDGE bias + 300: max|out_a - out_b| {d:.3e}, max|out| {float(oa.abs().max()):.3e}")
    assert d <= 2.0 ** -7 * float(oa.abs().max())


def test_single_visible_key_under_dropout_records_the_noise_of_delta():
    """(Lq, Lk) = (128, 1), p = 0.1: dS is zero in exact arithmetic, and the short backward takes delta from the bf16 output, so dq and dk
    carry that rounding.  The kernel must not carry more of it than the restatement of that arithmetic allows; the long
    kernels, which correct their delta, are run at (130, 1) for the record."""
    import vlpet_amd.attention as A
    case = S.BY_NAME["3x1x128x1-p0.1"]
    R = _result(case)
    mx = lambda t: float(t.double().abs().max())
    long_case = S.make_case(3, 1, 130, 1, False, None, 0.1)
    q, k, v, do, km, bias, scale = S.inputs(long_case)
    got_long, keep_long, _ = _gpu(q, k, v, do, km, False, 0.1, None, scale, 1, fn=A.long_attention_train)
    ref_long = S.chain(q, k, v, do, km, False, keep_long, 0.1, None, scale, 1, torch.float64, False)
    assert mx(ref_long[1]) <= 1e-12 and mx(ref_long[2]) <= 1e-12
    print(f"\nEDGE single key (128, 1) p = 0.1: max|dq| short {mx(R['got'][1]):.3e} restated {mx(R['rst'][1]):.3e} | max|dk| short "
          f"{mx(R['got'][2]):.3e} restated {mx(R['rst'][2]):.3e} | long kernels at (130, 1): max|dq| {mx(got_long[1]):.3e} max|dk| "
          f"{mx(got_long[2]):.3e}")
    for i in (1, 2):
        assert mx(R["got"][i]) <= max(3.0 * mx(R["rst"][i]), S.FLOOR)
        assert torch.isfinite(got_long[i].float()).all()


@pytest.mark.parametrize("name", ["3x3x56x20-causal-p0.1", "3x3x33x33-dead1-p0.1", "3x1x56x20-causal-dead1-p0.1",
                                  "3x1x65x33-random-p0.1-bias_row5"])
def test_rows_with_no_visible_key_get_exact_zeros(name):
    """the first Lq - Lk rows under the causal bound, a wholly masked item, a bias row of -inf (all with p = 0.1): output and dq rows of
    zeros, lse = +inf; a dead item adds nothing to dk and dv either; the rows next to them are alive"""
    case = S.BY_NAME[name]
    R = _result(case)
    dead = R["dead"]                                            # [B, H, Lq]
    assert case.p == 0.1 and bool(dead.any()) and not bool(dead.all())
    if case.causal and case.Lq > case.Lk:
        assert bool(dead[:, :, :case.Lq - case.Lk].all())
    if case.bias == "row5":
        assert bool(dead[:, :, 5].all()) and not bool(dead[0, :, 4].any()) and not bool(dead[0, :, 6].any())
    out, dq, dk, dv = (t.float() for t in R["got"])
    zero = torch.zeros(64)
    assert torch.equal(out[dead], zero.expand_as(out[dead])) and torch.equal(dq[dead], zero.expand_as(dq[dead]))
    assert bool(torch.isposinf(R["lse"][dead]).all()) and bool(torch.isfinite(R["lse"][~dead]).all())
    assert float((out[~dead].abs().amax(-1) > 0).float().mean()) > 0.8      # (dropout can empty a row with one or two visible keys)
    if case.mask == "dead1":
        assert bool(dead[1].all())
        assert torch.equal(dk[1], torch.zeros_like(dk[1])) and torch.equal(dv[1], torch.zeros_like(dv[1]))
        assert float(dk[0].abs().max()) > 0 and float(dv[2].abs().max()) > 0


def _fb(q, k, v, do, H, km, p, seed=3):
    from vlpet_amd.attention import short_attention
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = short_attention(qg, kg, vg, H, km, False, p, True, seed=seed)
    out.backward(do)
    return out.detach(), qg.grad, kg.grad, vg.grad


def test_two_calls_are_bitwise_equal():
    case = S.make_case(3, 3, 76, 76, False, "random", 0.1)
    q, k, v, do, km, _, _ = S.inputs(case)
    q, k, v, do, km = (t.cuda() for t in (q, k, v, do, km))
    a, b = _fb(q, k, v, do, 3, km, 0.1), _fb(q, k, v, do, 3, km, 0.1)
    for n, x, y in zip(S.NAMES, a, b):
        assert float(x.float().abs().max()) > 0 and torch.equal(x, y), n


def test_an_item_does_not_depend_on_the_batch():
    """one item repeated 91 times (273 pairs: an odd number, several workgroup rounds; every copy has other (b, h, i) row keys, hence
    p = 0): each copy has the bits of the item run alone"""
    case = S.make_case(1, 3, 76, 76, False, "random", 0.0)
    q, k, v, do, km, _, _ = S.inputs(case)
    q, k, v, do, km = (t.cuda() for t in (q, k, v, do, km))
    one = _fb(q, k, v, do, 3, km, 0.0)
    rep = lambda t: t.expand(91, *t.shape[1:]).contiguous()
    many = _fb(rep(q), rep(k), rep(v), rep(do), 3, rep(km), 0.0)
    for n, x, y in zip(S.NAMES, one, many):
        assert float(x.float().abs().max()) > 0
        assert torch.equal(y, x.expand_as(y)), n


@pytest.mark.parametrize("L", [33, 97])
def test_nothing_outside_the_outputs_is_written(L):
    """q | k | v as column blocks of one [B, L, 3E + 16] buffer (row stride 3E + 16) and dq | dk | dv into another, through the C entry
    points: the 16 spare columns of every row, a spare row past B * L of every output and the inputs keep their sentinels / values
    (L = 33, 97: the last 16-row store of store_rows_T holds one live row), and the results are short_attention's on copies"""
    from vlpet_amd import _lib
    from vlpet_amd.attention import short_attention
    lib = _lib.load()
    B, H = 2, 3
    E, rows = H * 64, B * L
    ld = 3 * E + 16
    g = torch.Generator().manual_seed(L)
    buf = torch.full((rows + 1, ld), 768.0, dtype=torch.bfloat16)
    buf[:rows, :3 * E] = (torch.randn(rows, 3 * E, generator=g) * 1.5).bfloat16()
    do = torch.randn(rows, E, generator=g).bfloat16().cuda()
    km = torch.rand(B, L, generator=g) > 0.25
    km[:, 0] = True
    km = km.to(torch.uint8).cuda()
    buf = buf.cuda()
    buf0, do0 = buf.clone(), do.clone()
    grad = torch.full((rows + 1, ld), -512.0, dtype=torch.bfloat16, device="cuda")
    o = torch.full((rows + 1, E), 320.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B * H * L + 1,), 7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    base, gbase, cb = buf.data_ptr(), grad.data_ptr(), 2 * E
    rc = lib.vlpet_attn_fwd_ld(base, base + cb, base + 2 * cb, km.data_ptr(), o.data_ptr(), lse.data_ptr(), None, B, H, L, L, ld, ld, 0,
                               0.125, 0.1, 7, st)
    assert rc == 0
    rc = lib.vlpet_attn_bwd_ld(base, base + cb, base + 2 * cb, o.data_ptr(), do.data_ptr(), lse.data_ptr(), km.data_ptr(), gbase,
                               gbase + cb, gbase + 2 * cb, B, H, L, L, ld, ld, 0, 0.125, 0.1, 7, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0) and torch.equal(do, do0)
    assert bool((grad[:, 3 * E:] == -512.0).all()) and bool((grad[rows] == -512.0).all())
    assert bool((o[rows] == 320.0).all()) and float(lse[-1]) == 7.0
    q, k, v = (buf[:rows, i * E:(i + 1) * E].reshape(B, L, E).clone().requires_grad_(True) for i in range(3))
    out = short_attention(q, k, v, H, km, False, 0.1, True, seed=7)
    out.backward(do.view(B, L, E))
    assert torch.equal(o[:rows].view(B, L, E), out.detach())
    for i, t in enumerate((q, k, v)):
        assert float(t.grad.float().abs().max()) > 0
        assert torch.equal(grad[:rows, i * E:(i + 1) * E].reshape(B, L, E), t.grad), "qkv"[i]


@pytest.mark.parametrize("L", [33, 97])
def test_fused_qkv_form_with_a_bias_is_the_same_kernel_on_column_blocks(L):
    """short_self_attention with T5's bias + the causal bound + a key mask on one [B, L, 3E] buffer == short_attention on the three
    column copies (same seed -> same dropout pattern): output and the three input gradients bit for bit"""
    from vlpet_amd.attention import AttnBias, short_attention, short_self_attention
    B, H = 2, 3
    E = H * 64
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(B, L, 3 * E, generator=g) * 0.35).bfloat16().cuda()
    do = torch.randn(B, L, E, generator=g).bfloat16().cuda()
    bias = AttnBias((torch.randn(H, L, L, generator=g) * 2.0).cuda())
    km = torch.rand(B, L, generator=g) > 0.25
    km[:, 0] = True
    km = km.cuda()
    a = qkv.clone().requires_grad_(True)
    o1 = short_self_attention(a, H, km, True, 0.1, True, scale=1.0, seed=7, bias=bias)
    o1.backward(do)
    q, k, v = (qkv[..., i * E:(i + 1) * E].clone().requires_grad_(True) for i in range(3))
    o2 = short_attention(q, k, v, H, km, True, 0.1, True, scale=1.0, seed=7, bias=bias)
    o2.backward(do)
    assert float(o1.float().abs().max()) > 0 and torch.equal(o1, o2)
    for i, t in enumerate((q, k, v)):
        assert torch.equal(a.grad[..., i * E:(i + 1) * E], t.grad), "qkv"[i]
