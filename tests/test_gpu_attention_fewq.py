"""The short attention backward for calls with one query block (csrc/attn_bwd_fewq.hip: Lq <= 32, no bias; a wave per (batch, head) pair,
W = AT_FQ waves per workgroup, each score tile evaluated once and dS handed to the dQ product through the wave's LDS), through
vlpet_amd.attention.short_attention and the C entry points: against tests/attn_spec.py's fp64 chain with the dropout mask the forward
exported, under the project's tensor-wide bound AND tests/test_gpu_attention_edges.py's budget per 32-row tile,
err_kernel <= max(3 * err_restated, 2^-7 * max|ref tile|, 2e-4); pair counts around the workgroup; independence of where a pair is placed;
strided k / v / dk / dv with sentinels around them; dead rows and items; both sides of the routing rule (Lq = 32 | 33).

Every case is at most B = 3, H = 5: one forward and one backward, run once and shared by the tests that look at it.  Each case prints a
``FEWQ |`` table row (pytest -s)."""
import os
import re

import pytest
import torch

import attn_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = int(re.search(r"^#define AT_FQ (\d+)", open(os.path.join(ROOT, "vl-pet_amd", "csrc", "attn_bwd_fewq.hip")).read(), re.M).group(1))
SEED = 99
_RESULTS = {}

# (B, H, Lq, Lk, causal, mask, p): Lq in {1, 2, 5, 20, 31, 32}; Lk in {1, 5, 32, 33, 56, 64, 65, 92, 97, 128} and the benchmark's 56 / 56 / 92 / 76;
# a single key runs without dropout (with it dS is zero in exact arithmetic: tests/test_gpu_attention_edges.py records that noise)
CASES = [S.make_case(*c) for c in [
    (3, 1, 1, 1, False, None, 0.0), (1, 5, 2, 5, False, "random", 0.1), (3, 3, 5, 32, False, "suffix", 0.1), (1, 3, 20, 33, False, "random", 0.1),
    (3, 5, 5, 56, False, "random", 0.1), (1, 1, 31, 64, False, None, 0.0), (3, 1, 32, 65, False, "dead1", 0.1), (3, 3, 20, 76, False, "random", 0.1),
    (3, 5, 2, 92, False, "dead1", 0.1), (1, 3, 31, 97, False, "suffix", 0.0), (3, 1, 32, 128, False, "random", 0.1), (1, 5, 1, 128, False, None, 0.1),
    # causal, Lq = Lk (decoder self-attention).  Row 0 sees one key: with dropout its dS is zero in exact arithmetic and the documented
    # arithmetic (delta from the stored bf16 output) leaves that rounding in dq and dk, as above -- at Lq = Lk = 2 it is half
    # of the rows and the tensor-wide measure of dq reads 2.25e-2 for the kernel AND for chain(rounded=True) (per-tile ratio 0.33 = the
    # restatement's own error; one MI355X run), so that length runs at p = 0 and the lengths from 5 up carry the dropout
    (3, 3, 2, 2, True, None, 0.0), (3, 5, 5, 5, True, "random", 0.1), (1, 3, 20, 20, True, None, 0.1), (3, 1, 32, 32, True, "suffix", 0.0),
    # causal, Lq < Lk: the bound crosses key tiles; Lq > Lk: the first Lq - Lk queries see nothing
    (3, 3, 5, 56, True, None, 0.1), (1, 5, 20, 33, True, "random", 0.1), (3, 1, 31, 97, True, "dead1", 0.1), (1, 1, 32, 65, True, None, 0.0),
    (3, 3, 20, 5, True, None, 0.1),
]]
# the routing rule of launch_attn: Lq <= 32 -> attn_bwd_fewq_kernel, Lq = 33 -> attn_bwd_kernel
ROUTE = [S.make_case(3, 3, 32, 56, False, "random", 0.1), S.make_case(3, 3, 33, 56, False, "random", 0.1)]


def _pairs_case(n):
    """n (batch, head) pairs as B <= 3 items of H <= 5 heads at the benchmark's vqa cross-attention lengths"""
    B = next(b for b in (1, 2, 3) if n % b == 0 and n // b <= 5)
    return S.make_case(B, n // B, 5, 56, False, "random", 0.1)


PAIRS = [_pairs_case(n) for n in sorted({1, W - 1, W, W + 1, 2 * W + 1} - {0})]


def _gpu(q, k, v, do, km, causal, p, scale, H, seed=SEED, mask=True):
    """one forward + backward on the GPU -> (out, dq, dk, dv) as [B, H, L, 64] on the CPU and the exported keep mask"""
    import vlpet_amd.attention as A
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    res = A.short_attention(qg, kg, vg, H, None if km is None else km.cuda(), causal, p, True, scale=scale, seed=seed, return_mask=mask and p > 0)
    out, keep = res if (mask and p > 0) else (res, None)
    out.backward(do.cuda())
    torch.cuda.synchronize()
    got = [S.heads_first(t.detach().cpu(), H) for t in (out, qg.grad, kg.grad, vg.grad)]
    return got, (None if keep is None else keep.cpu().bool())


def _result(case):
    if case.name not in _RESULTS:
        q, k, v, do, km, bias, scale = S.inputs(case)
        assert bias is None
        got, keep = _gpu(q, k, v, do, km, case.causal, case.p, scale, case.H)
        args = (q, k, v, do, km, case.causal, keep, case.p, None, scale, case.H)
        _RESULTS[case.name] = dict(got=got, keep=keep, ref=S.chain(*args, torch.float64, False), rst=S.chain(*args, torch.float32, True),
                                   dead=S.dead_rows(q, k, km, case.causal, None, case.H))
    return _RESULTS[case.name]


def _check_bounds(case):
    R = _result(case)
    wide, worst, over = {}, 0.0, []
    for n, a, r, s in zip(S.NAMES, R["got"], R["ref"], R["rst"]):
        assert torch.isfinite(a.float()).all(), n
        wide[n] = S.wide_error(n, a, r)
        e_k, mag = S.tile_errors(a, r)
        e_r, _ = S.tile_errors(s, r)
        ratio = e_k / S.tile_budget(e_r, mag)
        worst = max(worst, float(ratio.max()))
        if float(ratio.max()) > 1.0:
            b, h, t = (int(x) for x in (ratio == ratio.max()).nonzero()[0])
            over.append(f"{n}: tile (b {b}, h {h}, rows {32 * t}..) kernel {float(e_k[b, h, t]):.3e} restated {float(e_r[b, h, t]):.3e} "
                        f"max|ref| {float(mag[b, h, t]):.3e}")
    print(f"\nFEWQ | {case.name} | " + " | ".join(f"{wide[n]:.2e}" for n in S.NAMES) + f" | {worst:.2f} |")
    for n in S.NAMES:
        assert wide[n] <= S.TOL, (n, wide)
    assert not over, over


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_within_the_tensor_wide_bound_and_the_per_tile_budget(case):
    _check_bounds(case)


@pytest.mark.parametrize("case", PAIRS, ids=lambda c: f"{c.B * c.H}pairs")
def test_pair_counts_around_the_workgroup(case):
    """B H in {1, W - 1, W, W + 1, 2 W + 1}: the last workgroup holds fewer pairs than waves"""
    assert case.B <= 3 and case.H <= 5
    _check_bounds(case)


@pytest.mark.parametrize("case", ROUTE, ids=lambda c: c.name)
def test_both_sides_of_the_routing_rule(case):
    _check_bounds(case)


def _fb(q, k, v, do, H, km, causal, p, seed=3):
    from vlpet_amd.attention import short_attention
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = short_attention(qg, kg, vg, H, km, causal, p, True, seed=seed)
    out.backward(do)
    return out.detach(), qg.grad, kg.grad, vg.grad


@pytest.mark.parametrize("H", [1, 5])
def test_an_item_does_not_depend_on_where_its_pairs_run(H):
    """item 0 alone (B = 1) and as the first of B = 3 (p = 0.1: the same (b, h, i) row keys); the same tensors as the LAST of B = 3 (p = 0: other
    row keys), where every pair sits on another wave of another workgroup (pairs 2 H .. 3 H - 1): dq, dk, dv bit for bit"""
    case = S.make_case(3, H, 20, 76, False, "random", 0.1)
    q, k, v, do, km, _, _ = S.inputs(case)
    q, k, v, do, km = (t.cuda() for t in (q, k, v, do, km))
    one = _fb(q[:1], k[:1], v[:1], do[:1], H, km[:1], False, 0.1)
    many = _fb(q, k, v, do, H, km, False, 0.1)
    for n, x, y in zip(S.NAMES, one, many):
        assert float(x.float().abs().max()) > 0
        assert torch.equal(y[:1], x), n
    flip = lambda t: t.flip(0).contiguous()
    one0 = _fb(q[:1], k[:1], v[:1], do[:1], H, km[:1], False, 0.0)
    last = _fb(flip(q), flip(k), flip(v), flip(do), H, flip(km), False, 0.0)
    for n, x, y in zip(S.NAMES, one0, last):
        assert float(x.float().abs().max()) > 0
        assert torch.equal(y[2:], x), n


def test_two_calls_are_bitwise_equal():
    case = S.make_case(3, 5, 20, 76, True, "random", 0.1)
    q, k, v, do, km, _, _ = S.inputs(case)
    q, k, v, do, km = (t.cuda() for t in (q, k, v, do, km))
    a, b = _fb(q, k, v, do, 5, km, True, 0.1), _fb(q, k, v, do, 5, km, True, 0.1)
    for n, x, y in zip(S.NAMES, a, b):
        assert float(x.float().abs().max()) > 0 and torch.equal(x, y), n


def _abi(lib, q, k, v, do, km, dq, dk, dv, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, p, seed=7):
    """forward + backward through vlpet_attn_fwd_kv / vlpet_attn_bwd_kv on raw addresses; returns the forward's output"""
    E = H * 64
    o = torch.empty(B * Lq, E, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H * Lq, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    kmp = None if km is None else km.data_ptr()
    assert lib.vlpet_attn_fwd_kv(q, k, v, kmp, None, o.data_ptr(), lse.data_ptr(), None, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, 0.125, p, seed, st) == 0
    assert lib.vlpet_attn_bwd_kv(q, k, v, o.data_ptr(), do.data_ptr(), lse.data_ptr(), kmp, None, None, dq, dk, dv, B, H, Lq, Lk, ld_q, ld_k, ld_v,
                                 causal, 0.125, p, seed, st) == 0
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("Lk", [33, 92])
def test_strided_keys_and_values_and_nothing_written_outside(Lk):
    """k and v as column blocks of a [B, Lk, 6 * 768] buffer (the decoder layers' fused key projection), dk and dv into the matching blocks of a
    sentinel-filled buffer: dq, dk, dv have the bits of the contiguous call, every sentinel outside the blocks and in the spare row past
    B * Lk is intact, and so are the inputs (Lk = 33, 92: the last 16-row store of a key tile holds one / twelve live rows)"""
    from vlpet_amd import _lib
    lib = _lib.load()
    B, H, Lq = 3, 5, 20
    E, ld, kc, vc = H * 64, 6 * 768, 768, 4 * 768
    g = torch.Generator().manual_seed(Lk)
    buf = torch.full((B * Lk + 1, ld), 768.0, dtype=torch.bfloat16)
    buf[:B * Lk, kc:kc + E] = (torch.randn(B * Lk, E, generator=g) * 1.5).bfloat16()
    buf[:B * Lk, vc:vc + E] = (torch.randn(B * Lk, E, generator=g) * 1.5).bfloat16()
    q = (torch.randn(B * Lq, E, generator=g) * 1.5).bfloat16().cuda()
    do = torch.randn(B * Lq, E, generator=g).bfloat16().cuda()
    km = torch.rand(B, Lk, generator=g) > 0.25
    km[:, 0] = True
    km = km.to(torch.uint8).cuda()
    buf = buf.cuda()
    buf0, q0, do0 = buf.clone(), q.clone(), do.clone()
    grad = torch.full((B * Lk + 1, ld), -512.0, dtype=torch.bfloat16, device="cuda")
    dq = torch.full((B * Lq + 1, E), -512.0, dtype=torch.bfloat16, device="cuda")
    es = 2                                                      # bytes per element
    o1 = _abi(lib, q.data_ptr(), buf.data_ptr() + kc * es, buf.data_ptr() + vc * es, do, km, dq.data_ptr(), grad.data_ptr() + kc * es,
              grad.data_ptr() + vc * es, B, H, Lq, Lk, E, ld, ld, 0, 0.1)
    assert torch.equal(buf, buf0) and torch.equal(q, q0) and torch.equal(do, do0)
    outside = torch.ones(ld, dtype=torch.bool, device="cuda")
    outside[kc:kc + E] = False
    outside[vc:vc + E] = False
    assert bool((grad[:, outside] == -512.0).all()) and bool((grad[B * Lk] == -512.0).all()) and bool((dq[B * Lq] == -512.0).all())
    k2, v2 = buf[:B * Lk, kc:kc + E].contiguous(), buf[:B * Lk, vc:vc + E].contiguous()
    dq2, dk2, dv2 = (torch.full_like(t, float("nan")) for t in (q, k2, v2))
    o2 = _abi(lib, q.data_ptr(), k2.data_ptr(), v2.data_ptr(), do, km, dq2.data_ptr(), dk2.data_ptr(), dv2.data_ptr(), B, H, Lq, Lk, E, E, E, 0, 0.1)
    assert torch.equal(o1, o2)
    for n, x, y in (("dq", dq[:B * Lq], dq2), ("dk", grad[:B * Lk, kc:kc + E], dk2), ("dv", grad[:B * Lk, vc:vc + E], dv2)):
        assert float(y.float().abs().max()) > 0 and torch.isfinite(y.float()).all(), n
        assert torch.equal(x, y), n


def test_a_dead_item_gets_written_zeros():
    """key mask dead1 (item 1 wholly masked) with dq, dk, dv pre-filled with NaN: every element is written, item 1's are exact zeros, the other
    items are alive"""
    from vlpet_amd import _lib
    lib = _lib.load()
    case = S.make_case(3, 3, 20, 76, False, "dead1", 0.1)
    q, k, v, do, km, _, _ = S.inputs(case)
    assert not bool(km[1].any()) and bool(km[0].any()) and bool(km[2].any())
    q, k, v, do = (t.cuda().reshape(-1, 3 * 64).contiguous() for t in (q, k, v, do))
    km = km.to(torch.uint8).cuda()
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    _abi(lib, q.data_ptr(), k.data_ptr(), v.data_ptr(), do, km, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), 3, 3, 20, 76, 192, 192, 192, 0, 0.1)
    for n, t, L in (("dq", dq, 20), ("dk", dk, 76), ("dv", dv, 76)):
        t = t.float().reshape(3, L, 192)
        assert torch.isfinite(t).all(), n
        assert torch.equal(t[1], torch.zeros_like(t[1])), n
        assert float(t[0].abs().max()) > 0 and float(t[2].abs().max()) > 0, n


@pytest.mark.parametrize("name", ["3x3x20x5-causal-p0.1", "3x1x32x65-dead1-p0.1", "3x1x31x97-causal-dead1-p0.1"])
def test_rows_with_no_visible_key_get_exact_zeros(name):
    """the first Lq - Lk rows under the causal bound and a wholly masked item: output and dq rows of exact zeros; a dead item adds nothing
    to dk and dv; the other rows are alive"""
    case = next(c for c in CASES if c.name == name)
    R = _result(case)
    dead = R["dead"]
    assert bool(dead.any()) and not bool(dead.all())
    if case.causal and case.Lq > case.Lk:
        assert bool(dead[:, :, :case.Lq - case.Lk].all()) and not bool(dead[:, :, case.Lq - case.Lk:].any())
    out, dq, dk, dv = (t.float() for t in R["got"])
    zero = torch.zeros(64)
    assert torch.equal(out[dead], zero.expand_as(out[dead])) and torch.equal(dq[dead], zero.expand_as(dq[dead]))
    assert float((dq[~dead].abs().amax(-1) > 0).float().mean()) > 0.8
    if case.mask == "dead1":
        assert bool(dead[1].all())
        assert torch.equal(dk[1], torch.zeros_like(dk[1])) and torch.equal(dv[1], torch.zeros_like(dv[1]))
        assert float(dk[0].abs().max()) > 0 and float(dv[2].abs().max()) > 0
