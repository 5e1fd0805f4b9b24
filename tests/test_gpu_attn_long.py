"""The long attention forward (csrc/attn_long.hip, vlpet_amd.attention.long_attention: up to 1,024 keys / queries, keys streamed in
chunks with an online softmax) against the eager chain of BartAttention.forward (my_transformers/modeling_bart.py:283-566: scores,
mask, softmax, weighted sum; tests/test_gpu_attention.py: _eager, restated here) in fp32 on the CPU on the same bf16 inputs.

The implementation's sizes, which the cases below straddle: a key CHUNK is 64 keys (two 32-key MFMA tiles; the bias table's key
axis is padded to 32, so a chunk's second tile can lie past it), a workgroup is 128 queries of one (batch, head), a wave 32 of them;
the short kernels end at 128.  Tolerances are the short kernels': output rel_err <= 2e-2, lse within 1e-3 * max(1, |ref|)."""
import math

import pytest
import torch

from gpu_cases import rel_err

pytestmark = pytest.mark.gpu

H = 12
TOL = 2e-2
LOG2E = math.log2(math.e)


def _eager(q, k, v, key_mask, causal, bias=None, scale=64 ** -0.5, heads=H):
    """-> (out [B, Lq, heads * 64], lse2 [B, heads, Lq]); a row with no visible key: NaN out (softmax of all -inf), lse -inf"""
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
    pr = torch.softmax(s, -1)
    return (pr @ sh(v, Lk)).transpose(1, 2).reshape(B, Lq, heads * 64), torch.logsumexp(s, -1) * LOG2E, s


def _inputs(B, Lq, Lk, heads=H, amp=1.5, seed=None):
    g = torch.Generator().manual_seed(Lq * 131 + Lk if seed is None else seed)
    mk = lambda L: (torch.randn(B, L, heads * 64, generator=g) * amp).bfloat16()
    return mk(Lq), mk(Lk), mk(Lk), g


def _check(q, k, v, key_mask=None, causal=False, bias=None, scale=None, heads=H, dead_items=()):
    """launch on the GPU, compare with the fp32 CPU chain; dead_items: batch items whose every key is masked (zeros, lse = +inf)"""
    import vlpet_amd.attention as A
    n0 = A.LONG_CALLS
    ab = None if bias is None else A.AttnBias(bias.cuda(), transposed=False)
    out, lse = A.long_attention(q.cuda(), k.cuda(), v.cuda(), heads, None if key_mask is None else key_mask.cuda(), causal,
                                scale=scale, bias=ab, return_lse=True)
    assert A.LONG_CALLS == n0 + 1
    assert ab is None or ab._bt is None                      # the forward builds no transposed bias table
    out, lse = out.float().cpu(), lse.cpu()
    assert out.shape == q.shape and lse.shape == (q.shape[0], heads, q.shape[1]) and lse.dtype == torch.float32
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    ref, lse_ref, _ = _eager(q.float(), k.float(), v.float(), key_mask, causal, bias, 64 ** -0.5 if scale is None else scale, heads)
    live = [b for b in range(q.shape[0]) if b not in dead_items]
    for b in dead_items:
        assert torch.equal(out[b], torch.zeros_like(out[b])) and bool((lse[b] == float("inf")).all())
    # rows that see no key under the causal rule (Lq > Lk) follow the same convention
    dead_rows = torch.isinf(lse_ref[live]) & (lse_ref[live] < 0)
    if dead_rows.any():
        got_dead = (lse[live] == float("inf"))
        assert torch.equal(got_dead, dead_rows)
        rows = dead_rows.any(1)                                # [B', Lq]: dead for a head = dead for all (masks are per key / per position)
        assert bool((out[live][rows] == 0).all())
        ref = torch.nan_to_num(ref, nan=0.0)
    err = rel_err(out[live], ref[live])
    ok = ~dead_rows
    lse_err = float(((lse[live][ok] - lse_ref[live][ok]).abs() / lse_ref[live][ok].abs().clamp(min=1.0)).max())
    print(f"out rel_err {err:.3e}  lse err {lse_err:.3e}")
    assert err <= TOL, err
    assert lse_err <= 1e-3, lse_err
    return out, lse


SELF = [  # B, L, heads -- which boundary
    (2, 129, H),     # one key past the short kernels' 128: a second workgroup with ONE query, a third chunk with one key
    (2, 192, H),     # whole chunks, a half-filled workgroup (two waves without a query block)
    (2, 193, H),     # one key past a chunk boundary, one query past a wave's block
    (2, 257, H),     # one past two workgroups / four chunks
    (1, 300, H),     # 300 = 4 chunks + 44: the last chunk's second tile lies past the 32-padded key axis (320)
    (2, 664, H),     # the video encoder: 10 chunks + 24, six workgroups per pair
    (1, 1024, H),    # the maximum: 16 whole chunks, eight workgroups per pair
    (1, 257, 1),
    (1, 257, 3),
    (24, 257, H),    # 864 workgroups: several rounds over the chip
]
CROSS = [(5, 664), (20, 129), (33, 300), (200, 56), (1, 1024), (130, 1)]


@pytest.mark.parametrize("B,L,heads", SELF)
def test_self_lengths_around_every_boundary(B, L, heads):
    q, k, v, _ = _inputs(B, L, L, heads)
    _check(q, k, v, heads=heads)


@pytest.mark.parametrize("Lq,Lk", CROSS)
def test_cross_lengths(Lq, Lk):
    """few queries against many keys (most waves only stage), many queries against one chunk, a single key"""
    q, k, v, _ = _inputs(2, Lq, Lk)
    _check(q, k, v)


@pytest.mark.parametrize("Lq,Lk", [(300, 300), (100, 300), (300, 100)])
def test_causal(Lq, Lk):
    """key j visible to query i iff j <= i + Lk - Lq; workgroups stop at the last chunk their queries see; with Lq > Lk the first
    Lq - Lk queries see nothing (zeros, lse = +inf)"""
    q, k, v, _ = _inputs(2, Lq, Lk)
    _check(q, k, v, causal=True)


def _masks(B, L, g):
    ar = torch.arange(L)[None, :].expand(B, L)
    rnd = torch.rand(B, L, generator=g) > 0.25
    rnd[:, -1] = True
    lens = torch.randint(1, L + 1, (B,), generator=g)
    return {
        "random": rnd,
        "suffix": ar < lens[:, None],
        "middle_chunk": ~((ar >= 128) & (ar < 192)),             # chunk 2 entirely masked: the running state must pass through unchanged
        "first_chunk": ar >= 64,                                 # the first visible chunk starts from m = -inf
        "first_three": ar >= 192,
        "all_but_last_key": ar == L - 1,
    }


@pytest.mark.parametrize("kind", ["random", "suffix", "middle_chunk", "first_chunk", "first_three", "all_but_last_key"])
@pytest.mark.parametrize("biased", [False, True])
def test_key_masks(kind, biased):
    B, L = 3, 300
    q, k, v, g = _inputs(B, L, L, amp=0.4 if biased else 1.5)
    bias = torch.randn(H, L, L, generator=g) * 2.0 if biased else None
    _check(q, k, v, key_mask=_masks(B, L, g)[kind], bias=bias, scale=1.0 if biased else None)


@pytest.mark.parametrize("biased", [False, True])
def test_items_with_every_key_masked_give_zeros_and_infinite_lse(biased):
    B, L = 4, 200
    q, k, v, g = _inputs(B, L, L, amp=0.4 if biased else 1.5)
    km = torch.rand(B, L, generator=g) > 0.25
    km[1] = False
    km[3] = False
    bias = torch.randn(H, L, L, generator=g) if biased else None
    _check(q, k, v, key_mask=km, bias=bias, scale=1.0 if biased else None, dead_items=(1, 3))


@pytest.mark.parametrize("Lq,Lk", [(664, 664), (33, 300)])
@pytest.mark.parametrize("masked", [False, True])
def test_bias_t5_form(Lq, Lk, masked):
    """scale = 1.0 and a [H, Lq, Lk] table padded to 32 on both axes; lengths that are no multiple of 32"""
    B = 2
    q, k, v, g = _inputs(B, Lq, Lk, amp=0.4)
    bias = torch.randn(H, Lq, Lk, generator=g) * 2.0
    km = None
    if masked:
        km = torch.rand(B, Lk, generator=g) > 0.25
        km[:, 0] = True
    _check(q, k, v, key_mask=km, bias=bias, scale=1.0)


def test_causal_with_bias_and_mask():
    B, L = 2, 200
    q, k, v, g = _inputs(B, L, L, amp=0.4)
    lens = torch.tensor([200, 77])
    _check(q, k, v, key_mask=torch.arange(L)[None, :] < lens[:, None], causal=True, bias=torch.randn(H, L, L, generator=g), scale=1.0)


def test_large_scores():
    """max |score| about 200 (log2 units: 290): the exponentials are taken against the running maximum and nothing overflows"""
    B, L = 1, 300
    q, k, v, _ = _inputs(B, L, L)
    s = _eager(q.float(), k.float(), v.float(), None, False)[2]
    q = (q.float() * (200.0 / float(s.abs().max()))).bfloat16()
    ref, _, s = _eager(q.float(), k.float(), v.float(), None, False)
    assert 150.0 < float(s.abs().max()) < 250.0 and torch.isfinite(ref).all()       # the reference itself first
    out, lse = _check(q, k, v)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()


def test_bitwise_reproducible_and_independent_of_the_batch():
    import vlpet_amd.attention as A
    B, L = 8, 664
    q, k, v, g = _inputs(B, L, L)
    km = torch.rand(B, L, generator=g) > 0.25
    q, k, v, km = q.cuda(), k.cuda(), v.cuda(), km.cuda()
    runs = [A.long_attention(q, k, v, H, km, return_lse=True) for _ in range(3)]
    for o, l in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(l, runs[0][1])
    o1, l1 = A.long_attention(q[:1].contiguous(), k[:1].contiguous(), v[:1].contiguous(), H, km[:1].contiguous(), return_lse=True)
    assert torch.equal(o1[0], runs[0][0][0]) and torch.equal(l1[0], runs[0][1][0])
    o5, l5 = A.long_attention(q[5:6].contiguous(), k[5:6].contiguous(), v[5:6].contiguous(), H, km[5:6].contiguous(), return_lse=True)
    assert torch.equal(o5[0], runs[0][0][5]) and torch.equal(l5[0], runs[0][1][5])
    ref = _eager(q[:1].float().cpu(), k[:1].float().cpu(), v[:1].float().cpu(), km[:1].cpu(), False)[0]
    assert rel_err(o1, ref) <= TOL


def test_in_place_column_blocks_equal_contiguous_copies():
    import vlpet_amd.attention as A
    B, L, E = 2, 300, H * 64
    g = torch.Generator().manual_seed(7)
    qkv = (torch.randn(B, L, 3 * E, generator=g) * 1.5).bfloat16().cuda()
    km = (torch.rand(B, L, generator=g) > 0.25).cuda()
    q, k, v = (qkv[..., i * E:(i + 1) * E].contiguous() for i in range(3))
    want, want_lse = A.long_attention(q, k, v, H, km, return_lse=True)
    n0 = A.LONG_CALLS
    got = A.long_self_attention(qkv, H, km)
    assert A.LONG_CALLS == n0 + 1
    assert torch.equal(got, want)
    assert torch.equal(A.long_self_attention(qkv, H, km, causal=True), A.long_attention(q, k, v, H, km, causal=True))
    # a key read as a column block of a wider buffer (functional.cross_key_blocks: [B, Lk, n_layers * E])
    Lq = 20
    wide = (torch.randn(B, L, 3 * E, generator=g) * 1.5).bfloat16().cuda()
    qs = (torch.randn(B, Lq, E, generator=g) * 1.5).bfloat16().cuda()
    for blk in range(3):
        kb = wide[..., blk * E:(blk + 1) * E]
        assert not kb.is_contiguous()
        a, al = A.long_attention(qs, kb, v, H, km, return_lse=True)
        b, bl = A.long_attention(qs, kb.contiguous(), v, H, km, return_lse=True)
        assert torch.equal(a, b) and torch.equal(al, bl)
    ref = _eager(qs.float().cpu(), wide[..., E:2 * E].float().cpu(), v.float().cpu(), km.cpu(), False)[0]
    assert rel_err(A.long_attention(qs, wide[..., E:2 * E], v, H, km), ref) <= TOL


@pytest.mark.parametrize("L", [56, 128])
def test_agrees_with_the_short_kernels_where_both_apply(L):
    import vlpet_amd.attention as A
    B = 3
    q, k, v, g = _inputs(B, L, L)
    km = torch.rand(B, L, generator=g) > 0.25
    km[:, 0] = True
    q, k, v, km = q.cuda(), k.cuda(), v.cuda(), km.cuda()
    with torch.no_grad():
        short = A.short_attention(q, k, v, H, km, training=False)
    long_ = A.long_attention(q, k, v, H, km)
    assert rel_err(long_, short) <= TOL


def test_argument_errors():
    import vlpet_amd.attention as A
    n0 = A.LONG_CALLS
    z = lambda L, dt=torch.bfloat16: torch.zeros(1, L, H * 64, dtype=dt, device="cuda")
    with pytest.raises(RuntimeError):
        A.long_attention(z(1025), z(1025), z(1025), H)
    with pytest.raises(RuntimeError):
        A.long_attention(z(200), z(1025), z(1025), H)
    with pytest.raises(RuntimeError):
        A.long_attention(z(200, torch.float32), z(200, torch.float32), z(200, torch.float32), H)
    with pytest.raises(RuntimeError):
        A.long_attention(z(200), z(200), z(100), H)
    with pytest.raises(RuntimeError):
        A.long_attention(z(200).requires_grad_(True), z(200), z(200), H)
    with pytest.raises(RuntimeError):
        A.long_self_attention(torch.zeros(1, 200, 3 * H * 64, dtype=torch.bfloat16, device="cuda").requires_grad_(True), H)
    with pytest.raises(RuntimeError):
        A.long_attention(z(200), z(200), z(200), H, bias=A.AttnBias(torch.zeros(H, 200, 100, device="cuda"), transposed=False))
    assert A.LONG_CALLS == n0
    with torch.no_grad():                                        # under no_grad a leaf that requires grad is fine
        A.long_attention(z(200).requires_grad_(True), z(200), z(200), H)
    assert A.LONG_CALLS == n0 + 1
