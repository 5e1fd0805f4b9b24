"""vlpet_colsum_seg and vlpet_act_dropout_bwd_cols (csrc/biasgrad.hip) through the C ABI against tests/bitfit_spec.py: every output
NaN-prefilled with sentinel elements behind it, both IO dtypes, element by element under the spec's derived bounds, bit for bit across
two calls.  The figures (worst err / bound) are printed before they are asserted."""
import ctypes

import pytest
import torch

import bitfit_spec as B
import tail_spec as T
from sentinel import pad_intact, padded_flat, padded_rows

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
E_SHAPE, E_ALIGN, E_WORKSPACE, E_NULL = -1, -3, -4, -5
SEG_SHAPES = [(1, 16), (3, 64), (3, 768), (6, 768), (16, 16)]
GUARD = 64
SEED = 0x0BADC0FFEE123457


def _lib():
    from vlpet_amd import _lib as L
    return L, L.load()


def _io(dtype):
    from vlpet_amd import _lib as L
    return L.VLPET_F32 if dtype == F32 else L.VLPET_BF16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _seg_call(x, M, S, w, ld, null=()):
    """-> (list of per-segment results on the CPU, None for a NULL segment); asserts the sentinels and the untouched NULL segments"""
    L, lib = _lib()
    n = S * w
    ws_bytes = lib.vlpet_colsum_seg_workspace_bytes(M, n)
    assert ws_bytes == B.tail_blocks(M) * n * 4
    wbuf, ws = padded_flat(ws_bytes // 4, F32)
    outs = [padded_flat(w, F32) for _ in range(S)]
    ptrs = (ctypes.c_void_p * S)(*[None if s in null else outs[s][1].data_ptr() for s in range(S)])
    rc = lib.vlpet_colsum_seg(x.data_ptr(), M, S, w, ld, ptrs, ws.data_ptr(), ws_bytes, _io(x.dtype), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert pad_intact(wbuf, ws)
    res = []
    for s, (buf, body) in enumerate(outs):
        assert pad_intact(buf, body), s
        if s in null:
            assert bool(torch.isnan(body).all()), f"NULL segment {s} was written"
            res.append(None)
        else:
            res.append(body.cpu())
    return res


def _seg_input(M, n, dtype):
    """[M, n + GUARD]: the matrix in the first n columns, large guard values behind (a sum that strays into them shows)"""
    g = torch.Generator().manual_seed(7 + 13 * M + n)
    x = torch.randn(M, n + GUARD, generator=g) + 0.25
    x[:, n:] = 3.0e4
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M", [1, 3, 33] + B.grid_edges())
def test_colsum_seg_against_the_spec(dtype, M):
    L, lib = _lib()
    log = []
    for S, w in SEG_SHAPES:
        n = S * w
        xw = _seg_input(M, n, dtype)
        r = B.colsum_seg(xw, S, w)
        null = (1,) if S >= 3 else ()
        xg_wide, xg_tight = xw.cuda(), xw[:, :n].contiguous().cuda()
        for x, ld in ((xg_tight, n), (xg_wide, n + GUARD)):
            a = _seg_call(x, M, S, w, ld, null)
            b = _seg_call(x, M, S, w, ld, null)
            for s in range(S):
                if s in null:
                    continue
                wr = B.worst(a[s], r.out[s], r.e_out[s])
                log.append(f"S{S} w{w} ld{ld} seg{s} {wr:.3f}")
                assert wr <= 1.0, log[-1]
                assert torch.equal(a[s], b[s]), f"S{S} w{w} ld{ld} seg{s}: two calls differ"
        if S == 1 and n <= 4096:
            # the same sums as vlpet_colsum's, under vlpet_colsum's own bound (tests/tail_spec.py)
            nb = lib.vlpet_sublayer_tail_partials(M)
            c = T.colsum(xw[:, :n], nb)
            assert B.worst(a[0], c.out, c.e_out) <= 1.0
            ws = torch.empty(nb * n, device="cuda")
            obuf, o = padded_flat(n, F32)
            assert lib.vlpet_colsum(xg_tight.data_ptr(), M, n, ws.data_ptr(), o.data_ptr(), _io(dtype), _st()) == 0
            torch.cuda.synchronize()
            assert B.worst(o.cpu(), c.out, c.e_out) <= 1.0 and B.worst(a[0], o.cpu().double(), 2 * c.e_out) <= 1.0
    print(f"COLSUM_SEG {dtype} M={M} worst err / bound:", max(float(l.split()[-1]) for l in log))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_colsum_seg_widest(dtype):
    """n past vlpet_colsum's cap: 6,144 columns at bf16, 3,072 at fp32 (8 segments), three column chunks of the first pass"""
    S, w, M = 8, 768 if dtype == BF else 384, 37
    xw = _seg_input(M, S * w, dtype)
    r = B.colsum_seg(xw, S, w)
    a = _seg_call(xw.cuda(), M, S, w, S * w + GUARD, null=(7,))
    assert max(B.worst(a[s], r.out[s], r.e_out[s]) for s in range(7)) <= 1.0


def test_colsum_seg_refusals_write_nothing():
    L, lib = _lib()
    M, S, w = 9, 3, 64
    n = S * w
    x = torch.randn(M, n + GUARD, device="cuda").to(BF)
    wbuf, ws = padded_flat(B.tail_blocks(M) * n, F32)
    outs = [padded_flat(w, F32) for _ in range(16)]
    ptrs = (ctypes.c_void_p * 16)(*[o[1].data_ptr() for o in outs])
    wsb = ws.numel() * 4
    call = lambda x_, S_, w_, ld_, out_, ws_, wsb_, io_=L.VLPET_BF16: lib.vlpet_colsum_seg(x_, M, S_, w_, ld_, out_, ws_, wsb_, io_, _st())
    assert call(x.data_ptr(), S, 72, 3 * 72 + 8, ptrs, ws.data_ptr(), wsb) == E_SHAPE            # w % 16
    assert call(x.data_ptr(), 17, 16, 17 * 16, ptrs, ws.data_ptr(), wsb) == E_SHAPE              # S > 16
    assert call(x.data_ptr(), 0, 16, 16, ptrs, ws.data_ptr(), wsb) == E_SHAPE
    assert call(x.data_ptr(), S, w, n - 8, ptrs, ws.data_ptr(), wsb) == E_SHAPE                  # ld < n
    assert call(x.data_ptr(), S, w, n + 4, ptrs, ws.data_ptr(), wsb) == E_ALIGN                  # rows off the 16-byte grid
    assert call(x.data_ptr(), S, w, n + GUARD, ptrs, None, wsb) == E_NULL                        # no workspace
    assert call(None, S, w, n + GUARD, ptrs, ws.data_ptr(), wsb) == E_NULL
    assert call(x.data_ptr(), S, w, n + GUARD, None, ws.data_ptr(), wsb) == E_NULL
    assert call(x.data_ptr(), S, w, n + GUARD, ptrs, ws.data_ptr(), wsb - 4) == E_WORKSPACE
    assert call(x.data_ptr() + 2, S, w, n + GUARD, ptrs, ws.data_ptr(), wsb) == E_ALIGN
    assert call(x.data_ptr(), S, w, n + GUARD, ptrs, ws.data_ptr(), wsb, 7) == -6                # dtype
    assert lib.vlpet_colsum_seg(x.data_ptr(), 0, S, w, n + GUARD, ptrs, ws.data_ptr(), wsb, L.VLPET_BF16, _st()) == E_SHAPE
    none = (ctypes.c_void_p * 3)(None, None, None)
    assert call(x.data_ptr(), S, w, n + GUARD, none, ws.data_ptr(), wsb) == 0                    # nothing wanted: no launch, no error
    assert lib.vlpet_colsum_seg_workspace_bytes(0, 64) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()) and pad_intact(wbuf, ws)
    for buf, body in outs:
        assert bool(torch.isnan(body).all()) and pad_intact(buf, body)


# ------------------------------------------------------------------------------------------------------ activation backward + sums
ACT_SHAPES = [(1, 8), (9, 64), (130, 256), (1031, 3072), (4 * B.ACT_COLS_CAP + 9, 64)]      # the last: more rows than 4 x the grid's row slices


def _act_inputs(M, n, dtype):
    g = torch.Generator().manual_seed(5 + M + n)
    x = (torch.randn(M, n, generator=g) * 2.0).to(dtype)
    dy = torch.randn(M, n, generator=g)
    dy = (torch.where(dy < 0, -1.0, 1.0) * (dy.abs() + 0.25)).to(dtype)
    return dy.cuda(), x.cuda()


def _plain_bwd(dy, x, act, p, seed):
    L, lib = _lib()
    buf, dx = padded_rows(x.shape[0], x.shape[1], x.dtype)
    assert lib.vlpet_act_dropout_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), B.ACTS[act], p, seed, _io(x.dtype), _st()) == 0
    torch.cuda.synchronize()
    assert pad_intact(buf, dx)
    return dx


def _cols_bwd(dy, x, act, p, seed, fused_reduce=True):
    """-> dx [M, n] (GPU), sums [n] (CPU fp32)"""
    L, lib = _lib()
    M, n = x.shape
    nb = B.act_cols_partials(M, n)
    buf, dx = padded_rows(M, n, x.dtype)
    wbuf, ws = padded_flat(nb * n, F32)
    obuf, out = padded_flat(n, F32)
    got_nb = ctypes.c_int(-1)
    rc = lib.vlpet_act_dropout_bwd_cols(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), M, n, B.ACTS[act], p, seed, ws.data_ptr(), nb * n * 4,
                                        out.data_ptr() if fused_reduce else None, ctypes.addressof(got_nb), _io(x.dtype), _st())
    assert rc == 0, rc
    assert got_nb.value == nb
    if not fused_reduce:
        assert lib.vlpet_sublayer_tail_reduce(ws.data_ptr(), nb, n // 2, out.data_ptr(), out.data_ptr() + 2 * n, _st()) == 0
    torch.cuda.synchronize()
    assert pad_intact(buf, dx) and pad_intact(wbuf, ws) and pad_intact(obuf, out)
    assert not bool(torch.isnan(ws).any()), "a partial was not written"
    return dx, out.cpu()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
@pytest.mark.parametrize("M,n", ACT_SHAPES)
def test_act_dropout_bwd_cols(dtype, act, M, n):
    L, lib = _lib()
    assert (M + 3) // 4 > B.act_cols_partials(M, n) or M < 4 * B.ACT_COLS_CAP
    dy, x = _act_inputs(M, n, dtype)
    ctr = torch.tensor([3], dtype=torch.int64, device="cuda")
    seen = {}
    try:
        for p in (0.0, 0.1):
            for with_ctr in (False, True):
                lib.vlpet_set_seed_counter(ctr.data_ptr() if with_ctr else None)
                want = _plain_bwd(dy, x, act, p, SEED)
                dx, sums = _cols_bwd(dy, x, act, p, SEED)
                assert torch.equal(dx.view(torch.uint8), want.view(torch.uint8)), f"p={p} ctr={with_ctr}: dx differs from vlpet_act_dropout_bwd"
                ref, e, h = B.colsums_of_stored(dx, n)
                wr = B.worst(sums, ref, e)
                print(f"ACT_COLS {dtype} {act} M={M} n={n} p={p} ctr={with_ctr}: h={h} worst err / bound {wr:.3f}")
                assert wr <= 1.0
                dx2, sums2 = _cols_bwd(dy, x, act, p, SEED, fused_reduce=False)
                assert torch.equal(dx2.view(torch.uint8), dx.view(torch.uint8)) and torch.equal(sums2, sums)
                seen[(p, with_ctr)] = dx
        if M * n >= 512:
            assert not torch.equal(seen[(0.1, False)], seen[(0.1, True)]), "the step counter did not reach the mask"
            assert not torch.equal(seen[(0.0, False)], seen[(0.1, False)])
        assert torch.equal(seen[(0.0, False)], seen[(0.0, True)])
    finally:
        lib.vlpet_set_seed_counter(None)


def test_act_dropout_bwd_cols_mask_is_the_spec():
    """relu of positive inputs has derivative 1: dx = dy * keep_scale where dropout_spec keeps, 0 where it drops"""
    M, n, p = 130, 256, 0.1
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(M, n, generator=g) + 0.5).cuda()
    dy = (torch.rand(M, n, generator=g) + 0.5).cuda()
    _lib()[1].vlpet_set_seed_counter(None)
    dx, sums = _cols_bwd(dy, x, "relu", p, SEED)
    r = B.act_dropout_bwd_cols(dy, x, "relu", p, SEED)
    keep = B.keep_mask(M, n, SEED, p)
    assert bool((dx.cpu()[~keep] == 0).all()) and bool((dx.cpu()[keep] != 0).all())
    assert B.worst(dx.cpu(), r.dx, r.e_dx) <= 1.0


SWEEP = [0.0, 1e-30, 1e-3, 0.5, 1.0, 3.0, 4.0, 5.5, 8.0, 12.0, 40.0, 1e4, 1e18]     # tests/test_gpu_act.py's values, and their negatives


@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
def test_act_dropout_bwd_cols_value_sweep(act):
    """every sweep value in every row position of a 3-row matrix, fp32, p = 0, dy = 1: finite, the plain kernel's bits, sums in bound"""
    v = torch.tensor([s * a for a in SWEEP for s in (1.0, -1.0)], dtype=F32)
    n = 32
    assert len(v) <= n
    row = torch.cat([v, torch.zeros(n - len(v))])
    x = torch.stack([row, row.flip(0), torch.roll(row, 5)]).cuda()
    dy = torch.ones_like(x)
    _lib()[1].vlpet_set_seed_counter(None)
    dx, sums = _cols_bwd(dy, x, act, 0.0, 0)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(sums).all())
    assert torch.equal(dx.view(torch.uint8), _plain_bwd(dy, x, act, 0.0, 0).view(torch.uint8))
    ref, e, _ = B.colsums_of_stored(dx, n)
    assert B.worst(sums, ref, e) <= 1.0
    if act != "gelu_new":       # (tests/test_gpu_act.py holds the tanh form to a bound relative to torch's own fp32 error instead)
        d64 = B.act_df(act, x.double().cpu())
        assert B.worst(dx.cpu(), d64, B.e_act_df(act, x.double().cpu(), d64) + 3 * B.U * d64.abs()) <= 1.0


def test_act_dropout_bwd_cols_refusals():
    L, lib = _lib()
    M, n = 9, 64
    dy, x = _act_inputs(M, n, BF)
    buf, dx = padded_rows(M, n, BF)
    wbuf, ws = padded_flat(B.act_cols_partials(M, n) * n, F32)
    obuf, out = padded_flat(n, F32)
    wsb = ws.numel() * 4
    f = lambda dy_, x_, dx_, M_, n_, act_, p_, ws_, wsb_, out_, io_=L.VLPET_BF16: lib.vlpet_act_dropout_bwd_cols(
        dy_, x_, dx_, M_, n_, act_, p_, 0, ws_, wsb_, out_, None, io_, _st())
    P = lambda t: t.data_ptr()
    assert f(P(dy), P(x), P(dx), M, 60, 0, 0.0, P(ws), wsb, P(out)) == E_SHAPE          # n_cols % 8
    assert f(P(dy), P(x), P(dx), 0, n, 0, 0.0, P(ws), wsb, P(out)) == E_SHAPE
    assert f(P(dy), P(x), P(dx), M, n, 9, 0.0, P(ws), wsb, P(out)) == E_SHAPE           # act
    assert f(P(dy), P(x), P(dx), M, n, 0, 1.0, P(ws), wsb, P(out)) == E_SHAPE           # p
    assert f(None, P(x), P(dx), M, n, 0, 0.0, P(ws), wsb, P(out)) == E_NULL
    assert f(P(dy), P(x), P(dx), M, n, 0, 0.0, None, wsb, P(out)) == E_NULL
    assert f(P(dy), P(x), P(dx), M, n, 0, 0.0, P(ws), wsb, None) == E_NULL              # neither out nor n_partials: the sums would be lost
    assert f(P(dy), P(x) + 2, P(dx), M, n, 0, 0.0, P(ws), wsb, P(out)) == E_ALIGN
    assert f(P(dy), P(x), P(dx), M, n, 0, 0.0, P(ws), wsb - 4, P(out)) == E_WORKSPACE
    assert f(P(dy), P(x), P(dx), M, n, 0, 0.0, P(ws), wsb, P(out), 7) == -6
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all())
    assert pad_intact(buf, dx) and pad_intact(wbuf, ws) and pad_intact(obuf, out)
