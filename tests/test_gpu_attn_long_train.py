"""The long attention in its training form (csrc/attn_long.hip with dropout, csrc/attn_long_bwd.hip;
vlpet_amd.attention.long_attention_train / long_self_attention_train: up to 1,024 keys / queries) against the fp32 CPU eager chain of
tests/test_gpu_attention.py::_eager, restated here, on the same bf16 inputs with the EXPORTED keep mask and autograd's gradients.

Sizes the cases straddle: the short kernels end at 128; a streamed chunk is 64 rows (two 32-row MFMA tiles; the bias table's axes are
padded to 32, so a chunk's second tile can lie past them); a workgroup owns 128 queries (dQ pass) or 128 keys (dK / dV pass), a wave 32.

Tolerances are the project's: output rel_err <= 2e-2; each gradient max|a - r| <= 2e-2 * max(max|r|, 1e-2).  Where a long case misses
that, the library SDPA backward (bf16, p = 0) is measured against the same fp32 reference at that shape and max(1.5 x that, 2e-2) is
allowed (the pattern of test_t5_host_attention_fast_path_equals_the_dense_sdpa_path).  Measured on an MI355X: every case holds 2e-2
itself (out <= 4.7e-3, dq <= 1.4e-2, dk <= 5.8e-3, dv <= 4.8e-3; L = 664 and 1,024 at 2e-3 .. 5e-3).  The one-key case (130, 1) with
p = 0.1 is the worst dq: there the true dS cancels to zero and only the kernels' corrected delta (csrc/attn_long_bwd.hip) keeps the
rounding of the bf16 output out of dq and dk."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_spec as spec
from gpu_cases import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-2


def _eager(q, k, v, key_mask, causal, keep, p, bias=None, scale=64 ** -0.5, heads=2):
    """the chain of BartAttention.forward in the dtype of its inputs; a row with no visible key gives zeros and no gradient"""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    sh = lambda t, L: t.view(B, L, heads, 64).transpose(1, 2)
    s = (sh(q, Lq) @ sh(k, Lk).transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias[None]
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :].bool(), float("-inf"))
    if causal:
        i = torch.arange(Lq)[:, None]; j = torch.arange(Lk)[None, :]
        s = s.masked_fill(j > i + (Lk - Lq), float("-inf"))
    dead = torch.isinf(s).all(-1, keepdim=True)
    pr = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1) * (~dead)
    if keep is not None:
        pr = pr * keep.float() / (1.0 - p)
    return (pr @ sh(v, Lk)).transpose(1, 2).reshape(B, Lq, heads * 64)


def _inputs(B, Lq, Lk, heads=2, amp=1.5, seed=None):
    g = torch.Generator().manual_seed(Lq * 131 + Lk if seed is None else seed)
    mk = lambda L, a: (torch.randn(B, L, heads * 64, generator=g) * a).bfloat16()
    return mk(Lq, amp), mk(Lk, amp), mk(Lk, 1.5), mk(Lq, 1.0)          # q, k, v, dout


def _ref(q, k, v, do, key_mask, causal, keep, p, bias, scale, heads):
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    out = _eager(qf, kf, vf, key_mask, causal, keep, p, bias, scale, heads)
    out.backward(do.float())
    return out.detach(), qf.grad, kf.grad, vf.grad


def _gpu(q, k, v, do, key_mask, causal, p, bias, scale, heads, seed=1234, want_mask=True):
    import vlpet_amd.attention as A
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    ab = None if bias is None else A.AttnBias(bias.cuda(), transposed=False)
    n0 = A.LONG_TRAIN_CALLS
    res = A.long_attention_train(qg, kg, vg, heads, None if key_mask is None else key_mask.cuda(), causal, p, True, scale=scale,
                                 seed=seed, return_mask=want_mask, bias=ab)
    assert A.LONG_TRAIN_CALLS == n0 + 1
    out, keep = res if want_mask else (res, None)
    out.backward(do.cuda())
    assert ab is None or ab._bt is None                          # the kernels read the bias along keys: no transposed table is built
    return out.detach().cpu(), qg.grad.cpu(), kg.grad.cpu(), vg.grad.cpu(), (None if keep is None else keep.cpu().bool())


def _sdpa_errs(q, k, v, do, key_mask, causal, bias, scale, heads, ref):
    """the library path (bf16 SDPA forward + backward, no dropout) against the fp32 reference at p = 0: its error per tensor"""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    m = torch.zeros(B, 1, Lq, Lk)
    if bias is not None:
        m = m + bias[None]
    if key_mask is not None:
        m = m.masked_fill(~key_mask[:, None, None, :].bool(), float("-inf"))
    if causal:
        i = torch.arange(Lq)[:, None]; j = torch.arange(Lk)[None, :]
        m = m.masked_fill(j > i + (Lk - Lq), float("-inf"))
    sh = lambda t, L: t.view(B, L, heads, 64).transpose(1, 2)
    out = F.scaled_dot_product_attention(sh(qg, Lq), sh(kg, Lk), sh(vg, Lk), attn_mask=m.expand(B, heads, Lq, Lk).bfloat16().cuda(),
                                         scale=scale).transpose(1, 2).reshape(B, Lq, E)
    out.backward(do.cuda())
    return [rel_err(out, ref[0])] + [_err(a.float().cpu(), r) for a, r in zip((qg.grad, kg.grad, vg.grad), ref[1:])]


def _err(a, r):
    """max|a - r| over max(max|r|, 1e-2): the gradient bound"""
    a = a.float()
    if not torch.isfinite(a).all():
        return float("inf")
    return float((a - r).abs().max() / max(float(r.abs().max()), 1e-2))


def _check(q, k, v, do, key_mask=None, causal=False, p=0.0, bias=None, scale=64 ** -0.5, heads=2, dead_items=(), seed=1234):
    got = _gpu(q, k, v, do, key_mask, causal, p, bias, scale, heads, seed)
    keep = got[4]
    for t in got[:4]:
        assert torch.isfinite(t.float()).all()
    if p == 0.0:
        assert bool(keep.all())
    live = [b for b in range(q.shape[0]) if b not in dead_items]
    for b in dead_items:                                          # a fully masked item: exact zeros in the output and all three gradients
        for t in got[:4]:
            assert torch.equal(t[b], torch.zeros_like(t[b]))
    sl = lambda t: None if t is None else t[live]
    ref = _ref(sl(q), sl(k), sl(v), sl(do), sl(key_mask), causal, sl(keep) if p > 0 else None, p, bias, scale, heads)
    errs = [rel_err(sl(got[0]), ref[0])] + [_err(sl(a), r) for a, r in zip(got[1:4], ref[1:])]
    print("  ".join(f"{n} {e:.3e}" for n, e in zip(("out", "dq", "dk", "dv"), errs)))
    if max(errs) > TOL:
        ref0 = ref if p == 0.0 else _ref(sl(q), sl(k), sl(v), sl(do), sl(key_mask), causal, None, 0.0, bias, scale, heads)
        lib = _sdpa_errs(sl(q), sl(k), sl(v), sl(do), sl(key_mask), causal, bias, scale, heads, ref0)
        print("library SDPA (bf16, p = 0): " + "  ".join(f"{n} {e:.3e}" for n, e in zip(("out", "dq", "dk", "dv"), lib)))
        for e, l in zip(errs, lib):
            assert e <= max(1.5 * l, TOL), (errs, lib)
    return got, ref


# ---------------------------------------------------------------------------------------------------------------- shapes x dropout
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [129, 193, 257, 300])
def test_self_attention_lengths(L, p):
    """129: one past the short limit; 193: one past a chunk and a wave block; 257: one past two workgroups; 300: a last chunk whose second
    tile lies past the padded axes"""
    _check(*_inputs(2, L, L), p=p)


@pytest.mark.parametrize("L,p", [(664, 0.1), (1024, 0.0)])
def test_video_length_and_the_maximum(L, p):
    _check(*_inputs(1, L, L), p=p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Lq,Lk", [(5, 664), (33, 300), (200, 56), (130, 1)])
def test_cross_attention(Lq, Lk, p):
    _check(*_inputs(2, Lq, Lk), p=p)


def test_many_pairs_take_several_workgroup_rounds():
    _check(*_inputs(6, 257, 257, heads=12), p=0.1, heads=12)


def test_half_of_the_probabilities_dropped():
    _check(*_inputs(2, 193, 193), p=0.5)


# ---------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("Lq,Lk", [(300, 300), (100, 300), (300, 100)])
def test_causal(Lq, Lk):
    """(300, 100): the first 200 queries see no key -- zero output and dq rows, nothing added to dk / dv"""
    got, _ = _check(*_inputs(2, Lq, Lk), causal=True, p=0.1)
    if Lq > Lk:
        assert torch.equal(got[1][:, :Lq - Lk], torch.zeros_like(got[1][:, :Lq - Lk]))
        assert got[1][:, Lq - Lk:].abs().max() > 0


def _masks(B, L):
    g = torch.Generator().manual_seed(L)
    rnd = torch.rand(B, L, generator=g) > 0.3
    suffix = torch.arange(L)[None, :] < torch.tensor([L, L - 77])[:B, None]
    mid = torch.ones(B, L, dtype=torch.bool); mid[:, 128:192] = False
    first3 = torch.ones(B, L, dtype=torch.bool); first3[:, :192] = False
    return {"random": rnd, "suffix": suffix, "chunk_in_the_middle": mid, "first_three_chunks": first3}


@pytest.mark.parametrize("which", ["random", "suffix", "chunk_in_the_middle", "first_three_chunks"])
def test_key_masks(which):
    _check(*_inputs(2, 300, 300), key_mask=_masks(2, 300)[which], p=0.1)


def test_a_fully_masked_item_gets_exact_zeros():
    km = torch.ones(3, 257, dtype=torch.bool)
    km[1] = False
    km[2, 200:] = False
    _check(*_inputs(3, 257, 257), key_mask=km, p=0.1, dead_items=(1,))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Lq,Lk", [(300, 300), (33, 300)])
def test_t5_form_scale_one_and_a_shared_bias(Lq, Lk, masked):
    q, k, v, do = _inputs(2, Lq, Lk, amp=0.35)                   # (T5 has no 1 / sqrt(d): scores of a few units)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(2, Lq, Lk, generator=g) * 2.0
    km = _masks(2, Lk)["suffix"] if masked else None
    _check(q, k, v, do, key_mask=km, p=0.1, bias=bias, scale=1.0)


def test_large_scores():
    """|s| ~ 200: the exponent is taken against the saved lse, never against a partial maximum"""
    q, k, v, do = _inputs(2, 193, 193, amp=14.0)
    s = (q.float().view(2, 193, 2, 64).transpose(1, 2) @ k.float().view(2, 193, 2, 64).transpose(1, 2).transpose(-1, -2)) / 8
    assert 150 < float(s.abs().max()) < 1500
    _check(q, k, v, do, p=0.0)


# ---------------------------------------------------------------------------------------------------------------- the dropout mask
@pytest.mark.parametrize("Lq,Lk", [(193, 193), (33, 300)])
def test_exported_mask_equals_the_host_reference(Lq, Lk):
    q, k, v, do = _inputs(2, Lq, Lk)
    keep = _gpu(q, k, v, do, None, False, 0.1, None, 0.125, 2, seed=99)[4]
    assert np.array_equal(keep.numpy(), spec.attn_keep(2, 2, Lq, Lk, 99, 0.1))
    assert 0.85 < float(keep.float().mean()) < 0.95


def test_mask_depends_on_the_seed_only_and_eval_drops_nothing():
    import vlpet_amd.attention as A
    q, k, v, do = _inputs(2, 193, 193)
    q2, k2, v2, _ = _inputs(2, 193, 193, seed=77)
    a = _gpu(q, k, v, do, None, False, 0.1, None, 0.125, 2, seed=5)[4]
    b = _gpu(q2, k2, v2, do, None, False, 0.1, None, 0.125, 2, seed=5)[4]
    c = _gpu(q, k, v, do, None, False, 0.1, None, 0.125, 2, seed=6)[4]
    assert torch.equal(a, b) and not torch.equal(a, c)
    out, keep = A.long_attention_train(q.cuda(), k.cuda(), v.cuda(), 2, p=0.1, training=False, return_mask=True)
    assert bool(keep.all())
    assert torch.equal(out, A.long_attention(q.cuda(), k.cuda(), v.cuda(), 2))


# ---------------------------------------------------------------------------------------------------------------- bitwise equalities
def _fb(q, k, v, do, heads=2, p=0.1, seed=3, **kw):
    import vlpet_amd.attention as A
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = A.long_attention_train(qg, kg, vg, heads, p=p, training=True, seed=seed, **kw)
    out.backward(do)
    return out.detach(), qg.grad, kg.grad, vg.grad


def test_forward_without_dropout_has_the_bits_of_long_attention():
    import vlpet_amd.attention as A
    q, k, v, _ = (t.cuda() for t in _inputs(2, 300, 300))
    km = _masks(2, 300)["suffix"].cuda()
    o_ref, lse_ref = A.long_attention(q, k, v, 2, km, return_lse=True)
    lib = __import__("vlpet_amd._lib", fromlist=["load"]).load()
    o, lse = torch.empty_like(q), torch.empty(2, 2, 300, dtype=torch.float32, device="cuda")
    km8 = km.to(torch.uint8).contiguous()
    rc = lib.vlpet_attn_long_fwd_train(q.data_ptr(), k.data_ptr(), v.data_ptr(), km8.data_ptr(), None, o.data_ptr(), lse.data_ptr(), None,
                                       2, 2, 300, 300, 128, 128, 128, 0, 0.125, 0.0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(A.long_attention_train(q, k, v, 2, km, p=0.0, training=True), o_ref)


def test_two_backward_calls_are_bitwise_equal():
    q, k, v, do = (t.cuda() for t in _inputs(2, 300, 300))
    a, b = _fb(q, k, v, do), _fb(q, k, v, do)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_an_item_does_not_depend_on_the_batch():
    """B = 1 against item 0 of B = 3 (no dropout: the mask's row index holds b * H * Lq, which is 0 for item 0 either way -- p = 0.1 too)"""
    q, k, v, do = (t.cuda() for t in _inputs(3, 257, 257))
    for p in (0.0, 0.1):
        one = _fb(q[:1], k[:1], v[:1], do[:1], p=p)
        three = _fb(q, k, v, do, p=p)
        for x, y in zip(one, three):
            assert torch.equal(x[0], y[0])


def test_column_blocks_are_read_and_written_in_place():
    import vlpet_amd.attention as A
    B, L, E = 2, 200, 128
    g = torch.Generator().manual_seed(11)
    qkv = (torch.randn(B, L, 3 * E, generator=g) * 1.5).bfloat16().cuda()
    do = torch.randn(B, L, E, generator=g).bfloat16().cuda()
    x = qkv.clone().requires_grad_(True)
    out = A.long_self_attention_train(x, 2, p=0.1, training=True, seed=3)
    out.backward(do)
    ref = _fb(qkv[..., :E].contiguous(), qkv[..., E:2 * E].contiguous(), qkv[..., 2 * E:].contiguous(), do)
    assert torch.equal(out.detach(), ref[0])
    assert x.grad.shape == qkv.shape
    for i in range(3):
        assert torch.equal(x.grad[..., i * E:(i + 1) * E], ref[1 + i])
    # k as block 1 of a three-block key buffer, dk into the shared slot
    q, _, v, do2 = (t.cuda() for t in _inputs(B, 33, L))
    wide = (torch.randn(B, L, 3 * E, generator=g) * 1.5).bfloat16().cuda().requires_grad_(True)
    slot = A.KeyGradSlot(3, E)
    qg, vg = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = A.long_attention_train(qg, wide[..., E:2 * E], vg, 2, p=0.1, training=True, seed=3, k_slot=(slot, 1))
    out.backward(do2)
    ref = _fb(q, wide.detach()[..., E:2 * E].contiguous(), v, do2)
    assert slot.buf is not None and slot.buf.shape == (B, L, 3 * E)
    assert torch.equal(out.detach(), ref[0]) and torch.equal(qg.grad, ref[1]) and torch.equal(vg.grad, ref[3])
    assert torch.equal(slot.buf[..., E:2 * E], ref[2])
    assert torch.equal(wide.grad[..., E:2 * E], ref[2])


# ---------------------------------------------------------------------------------------------------------------- the short kernels
@pytest.mark.parametrize("Lq,Lk", [(128, 128), (20, 128)])
def test_agrees_with_the_short_kernels(Lq, Lk):
    import vlpet_amd.attention as A
    q, k, v, do = (t.cuda() for t in _inputs(2, Lq, Lk))
    km = (torch.arange(Lk)[None, :] < torch.tensor([Lk, Lk - 30])[:, None]).cuda()
    long_ = _fb(q, k, v, do, key_mask=km)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = A.short_attention(qg, kg, vg, 2, km, p=0.1, training=True, seed=3)
    out.backward(do)
    for a, r in zip(long_, (out.detach(), qg.grad, kg.grad, vg.grad)):
        assert _err(a.cpu(), r.float().cpu()) <= TOL


# ---------------------------------------------------------------------------------------------------------------- graph capture
def test_forward_and_backward_replay_from_a_captured_graph():
    import vlpet_amd.attention as A
    q, k, v, do = (t.cuda() for t in _inputs(2, 200, 200))
    eager = _fb(q, k, v, do, p=0.0)
    lib = __import__("vlpet_amd._lib", fromlist=["load"]).load()
    B, H, L, E = 2, 2, 200, 128
    o, lse = torch.empty_like(q), torch.empty(B, H, L, dtype=torch.float32, device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(B, H, L, dtype=torch.float32, device="cuda")

    def both(stream):
        rc = lib.vlpet_attn_long_fwd_train(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, o.data_ptr(), lse.data_ptr(), None,
                                           B, H, L, L, E, E, E, 0, 0.125, 0.0, 0, stream)
        assert rc == 0
        rc = lib.vlpet_attn_long_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), None, None,
                                     None, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, H, L, L, E, E, E, 0, 0.125, 0.0, 0,
                                     delta.data_ptr(), stream)
        assert rc == 0

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # (a single stream: the two entry points enqueue three launches on it)
        both(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for t in (o, dq, dk, dv):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, r in zip((o, dq, dk, dv), eager):
            assert torch.equal(a, r)
