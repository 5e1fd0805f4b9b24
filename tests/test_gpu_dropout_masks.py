"""Every dropout site of the library against tests/dropout_spec.py, bit for bit.

The parity tests of the dropout-carrying ops evaluate the oracle with the mask the kernel exported, so they prove forward /
backward consistency *given* the mask.  Here the mask itself is pinned: an exported mask must equal the spec's, and a site that
exports none is read structurally (with inputs chosen so that its output or input gradient is zero exactly where the spec
drops).  The spec's statistics are checked on the CPU (tests/test_dropout_spec.py), so together the two say that each site
applies i.i.d. Bernoulli(1 - p) masks, as ``F.dropout`` in the reference does.  Also: the graph-replay step counter
(vlpet_set_seed_counter) at 0, 1 and 2^40 + 3, a captured trainer step replayed twice, and one seed per site of a train step."""
import numpy as np
import pytest
import torch

import dropout_spec as S

pytestmark = pytest.mark.gpu

MS = (1, 37, 3111)
DS = (64, 768, 3072)
SEED = 0x1F2E3D4C5B6A7988
CTRS = (None, 0, 1, (1 << 40) + 3)


@pytest.fixture(autouse=True)
def _no_seed_counter_left_behind():
    yield
    from vlpet_amd import _lib
    _lib.load().vlpet_set_seed_counter(None)


def _set_ctr(value):
    """Register a device step counter holding ``value`` (None: no counter).  Returns the tensor (keep it alive)."""
    from vlpet_amd import _lib
    lib = _lib.load()
    if value is None:
        lib.vlpet_set_seed_counter(None)
        return None
    t = torch.tensor([value], dtype=torch.int64, device="cuda")
    assert lib.vlpet_set_seed_counter(t.data_ptr()) == 0
    return t


def _nonzero(shape, g, dtype):
    """Random values bounded away from 0 (so that a zero output means a dropped element), exactly representable in ``dtype``."""
    x = torch.randn(*shape, generator=g)
    return (x.sign() + (x == 0).float()) * (x.abs() + 0.25)


def _assert_mask(got, want, what):
    got = got.cpu().numpy().astype(bool)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} elements differ from the spec (first at {np.argwhere(got != want)[0].tolist()})"


def _assert_scaled(got, src, keep, p, dtype, what):
    """got == src * keep_scale where the spec keeps (fp32: exact; bf16: within one rounding), exactly 0 where it drops."""
    got = got.float().cpu().numpy()
    src = src.float().cpu().numpy()
    assert np.all(got[~keep] == 0), f"{what}: {int((got[~keep] != 0).sum())} nonzero where the spec drops"
    want = (src * S.keep_scale(p)).astype(np.float32)
    if dtype == torch.float32:
        assert np.array_equal(got[keep], want[keep]), what
    else:
        assert np.all(np.abs(got[keep] - want[keep]) <= np.abs(want[keep]) * 2.0 ** -8), what


# ------------------------------------------------------------------------------------------------ Philox sites that export
@pytest.mark.parametrize("ctr", CTRS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("norm", [True, False])
def test_sublayer_tail_mask_is_the_spec(norm, M, d, ctr):
    from vlpet_amd.tail import sublayer_tail
    g = torch.Generator().manual_seed(M * 7 + d)
    dtype = torch.bfloat16 if d != 768 else torch.float32
    y, x1 = (torch.randn(M, d, generator=g).to("cuda", dtype) for _ in range(2))
    ln = torch.nn.LayerNorm(d).cuda() if norm else None
    for p in (0.1, 0.5):
        c = _set_ctr(ctr)
        _, mask = sublayer_tail(x1, y, ln, p=p, training=True, seed=SEED + M, return_mask=True)
        torch.cuda.synchronize()
        _assert_mask(mask, S.keep_mask(M, d, SEED + M, p, ctr), f"tail norm={norm} M={M} d={d} p={p} ctr={ctr}")
        del c


@pytest.mark.parametrize("ctr", CTRS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("M", MS)
def test_act_dropout_mask_is_the_spec(M, d, ctr):
    from vlpet_amd.act import act_dropout
    g = torch.Generator().manual_seed(M + d)
    x = torch.randn(2, M, d, generator=g).cuda().to(torch.bfloat16)
    for p in (0.1, 0.5):
        c = _set_ctr(ctr)
        _, keep = act_dropout(x, "gelu", p, True, seed=SEED ^ d, return_mask=True)
        torch.cuda.synchronize()
        _assert_mask(keep.reshape(2 * M, d), S.keep_mask(2 * M, d, SEED ^ d, p, ctr), f"act M={M} d={d} p={p} ctr={ctr}")
        del c


def test_act_dropout_backward_applies_the_spec():
    """relu of positive inputs has derivative 1: dx = dy * keep_scale where the spec keeps, 0 where it drops."""
    from vlpet_amd.act import act_dropout
    g = torch.Generator().manual_seed(4)
    M, d, p = 37, 3072, 0.1
    for dtype in (torch.float32, torch.bfloat16):
        x = (torch.rand(M, d, generator=g) + 0.5).to("cuda", dtype).requires_grad_(True)
        dy = _nonzero((M, d), g, dtype).to(dtype)
        out = act_dropout(x, "relu", p, True, seed=SEED)
        out.backward(dy.cuda())
        _assert_scaled(x.grad, dy, S.keep_mask(M, d, SEED, p), p, dtype, f"act bwd {dtype}")


@pytest.mark.parametrize("ctr", [None, (1 << 40) + 3])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("r", [8, 64])
def test_lora_delta_mask_and_packed_bits_are_the_spec(r, M, d, ctr):
    """K3 on the streaming rank-8 kernel (lora8.hip, where vlpet_lora_r8_applies) and on the MFMA kernels: the exported byte mask,
    and the 1-bit mask the training form leaves in its saved block for the backward (drop_pos order)."""
    import vlpet_amd.functional as F
    from vlpet_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(r + M + d)
    dtype = torch.bfloat16
    x = torch.randn(M, d, generator=g).to("cuda", dtype).requires_grad_(True)
    A = (torch.randn(r, d, generator=g) * 0.05).cuda().requires_grad_(True)
    B = (torch.randn(d, r, generator=g) * 0.05).cuda().requires_grad_(True)
    io = F._io_dtype(x)
    pk = F.pack_pair([A.detach()], None, B.detach(), None, io)
    r8 = bool(lib.vlpet_lora_r8_applies(M, d, r, io)) and F.LORA_R8_STREAMING
    assert r8 == (r == 8 and d == 768)
    for p in (0.1, 0.5):
        c = _set_ctr(ctr)
        out, mask = F.lora_delta(x, torch.zeros_like(x), A, B, pk, 1.0, None, p, SEED - d, return_mask=True)
        torch.cuda.synchronize()
        want = S.keep_mask(M, d, SEED - d, p, ctr)
        _assert_mask(mask, want, f"lora r={r} M={M} d={d} p={p} ctr={ctr}")
        act = out.grad_fn.act                 # the saved block: z, then the packed mask
        assert act is not None
        esz = 2
        off = -(-M * 32 * (1 if r8 else pk.tiles) * esz // 256) * 256
        bits = act[off:off + M * d // 8].view(M, d // 8).cpu().numpy()
        assert np.array_equal(bits, S.packed_bits(want)), f"lora packed bits r={r} M={M} d={d} p={p}"
        out.float().sum().backward()         # (releases the saved block)
        del c


# ------------------------------------------------------------------------------------------------ Philox sites that do not export
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,d", [(1, 64), (37, 768), (3111, 768)])
def test_rms_tail_applies_the_spec(M, d, dtype):
    """sum = x1 + dropout(y) with x1 = 0: the sum is y * keep_scale where the spec keeps and 0 where it drops; the backward's d/dy
    is d_sum * keep_scale / 0 the same way."""
    from vlpet_amd.tail import sublayer_tail_rms
    from vlpet_amd.visual import T5LayerNorm
    g = torch.Generator().manual_seed(M + d)
    p = 0.1
    y = _nonzero((M, d), g, dtype).to(dtype)
    Y = y.cuda().requires_grad_(True)
    X1 = torch.zeros(M, d, dtype=dtype, device="cuda", requires_grad=True)
    norm = T5LayerNorm(d, eps=1e-6).cuda()
    s = sublayer_tail_rms(X1, Y, norm, p=p, training=True, seed=SEED)
    keep = S.keep_mask(M, d, SEED, p)
    _assert_scaled(s.detach(), y, keep, p, dtype, f"rms tail fwd M={M} d={d}")
    ds = _nonzero((M, d), g, dtype).to(dtype)
    n = norm(s)                                 # (the normalised rows get a zero gradient: d_sum = ds exactly)
    ((s.float() * ds.cuda().float()).sum() + (n.float() * 0.0).sum()).backward()
    _assert_scaled(Y.grad, ds, keep, p, dtype, f"rms tail bwd M={M} d={d}")


@pytest.mark.parametrize("ctr", [None, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,La,Lv,d", [(1, 1, 1, 64), (3, 20, 36, 768), (2, 7, 72, 3072)])
def test_concat_dropout_applies_the_spec(B, La, Lv, d, dtype, ctr):
    """x = dropout(cat([a, v], 1)) keyed by the element index of x: forward values and both input gradients."""
    from vlpet_amd.act import concat_dropout
    g = torch.Generator().manual_seed(B + La + Lv + d)
    p = 0.1
    a, v = _nonzero((B, La, d), g, dtype).to(dtype), _nonzero((B, Lv, d), g, dtype).to(dtype)
    A, V = a.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    c = _set_ctr(ctr)
    x = concat_dropout(A, V, p, True, seed=SEED)
    keep = S.keep_mask(B * (La + Lv), d, SEED, p, ctr).reshape(B, La + Lv, d)
    _assert_scaled(x.detach(), torch.cat([a, v], 1), keep, p, dtype, "concat fwd")
    dx = _nonzero((B, La + Lv, d), g, dtype).to(dtype)
    x.backward(dx.cuda())
    _assert_scaled(A.grad, dx[:, :La], keep[:, :La], p, dtype, "concat bwd text")
    _assert_scaled(V.grad, dx[:, La:], keep[:, La:], p, dtype, "concat bwd visual")
    del c


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("ctr", CTRS)
@pytest.mark.parametrize("B,H,Lq,Lk", [(2, 3, 33, 97), (1, 2, 128, 128), (5, 12, 56, 56), (3, 4, 1, 20), (2, 2, 20, 56)])
def test_attention_mask_is_the_spec(B, H, Lq, Lk, ctr):
    from vlpet_amd.attention import short_attention
    g = torch.Generator().manual_seed(B * H + Lq + Lk)
    q = torch.randn(B, Lq, H * 64, generator=g).cuda().bfloat16()
    k, v = (torch.randn(B, Lk, H * 64, generator=g).cuda().bfloat16() for _ in range(2))
    for p in (0.1, 0.5):
        c = _set_ctr(ctr)
        _, keep = short_attention(q, k, v, H, p=p, training=True, seed=SEED + Lk, return_mask=True)
        torch.cuda.synchronize()
        _assert_mask(keep, S.attn_keep(B, H, Lq, Lk, SEED + Lk, p, ctr), f"attn {B}x{H}x{Lq}x{Lk} p={p} ctr={ctr}")
        del c


def _onehot_qkv(B, H, L):
    """q = k = 0 (uniform probabilities 1 / L), v[b, j, h*64 + c] = (j == c): o[b, i, h*64 + j] = keep[b, h, i, j] * keep_scale / L."""
    E = H * 64
    qkv = torch.zeros(B, L, 3 * E)
    eye = torch.eye(L, 64)
    for h in range(H):
        qkv[:, :, 2 * E + 64 * h:2 * E + 64 * (h + 1)] = eye
    return qkv.cuda().bfloat16()


@pytest.mark.parametrize("ctr", [None, 1])
@pytest.mark.parametrize("B,H,L", [(2, 3, 33), (4, 12, 56), (1, 2, 64)])
def test_self_attention_forward_and_backward_apply_the_spec(B, H, L, ctr):
    """short_self_attention exports no mask.  With q = k = 0 and one-hot values, o[b, i, h*64 + j] is nonzero exactly where the spec
    keeps (b, h, i, j); with do[b, i, h*64 + c] = (i == c), dv[b, j, h*64 + i] is too (the backward's regenerated mask)."""
    from vlpet_amd.attention import short_self_attention
    p = 0.1
    E = H * 64
    qkv = _onehot_qkv(B, H, L).requires_grad_(True)
    c = _set_ctr(ctr)
    o = short_self_attention(qkv, H, p=p, training=True, seed=SEED ^ L)
    keep = S.attn_keep(B, H, L, L, SEED ^ L, p, ctr)                      # [B, H, i, j]
    of = o.detach().float().cpu().view(B, L, H, 64).permute(0, 2, 1, 3)[..., :L].numpy()
    _assert_mask(torch.from_numpy(of != 0), keep, f"self-attn fwd {B}x{H}x{L}")
    want = np.float32(np.float32(1.0 / L) * S.keep_scale(p))
    assert np.all(np.abs(of[keep] - want) <= want * 2.0 ** -7)
    do = torch.zeros(B, L, E)
    for h in range(H):
        do[:, :, 64 * h:64 * (h + 1)] = torch.eye(L, 64)
    o.backward(do.cuda().bfloat16())
    dv = qkv.grad[:, :, 2 * E:].float().cpu().view(B, L, H, 64).permute(0, 2, 3, 1)[:, :, :L, :].numpy()   # [B, H, i, j]
    _assert_mask(torch.from_numpy(dv != 0), keep, f"self-attn bwd {B}x{H}x{L}")
    del c


# ------------------------------------------------------------------------------------------------ training steps
def _bart(dropout):
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    cfg = HB.vlpet_config(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
                          encoder_ffn_dim=256, decoder_ffn_dim=256, vocab_size=500, max_position_embeddings=64, feat_dim=128,
                          adapter_down_dim=8, adapter_gating_down_dim=16, decoder_enc_attn_value_parallel_adapter_down_dim=8,
                          dropout=dropout, attention_dropout=dropout, activation_dropout=dropout)
    torch.manual_seed(0)
    model = HB.VLBart(cfg)
    TR.trainable_names(model, cfg)
    model.cuda()
    TR.cast_frozen(model, torch.bfloat16)
    model.train()
    return model, cfg


def _cuda_batch(b):
    bb = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    bb["vis_inputs"] = tuple(t.cuda() for t in b["vis_inputs"])
    return bb


def test_replayed_step_masks_follow_the_counter(monkeypatch):
    """A captured Trainer(graph=True) step replays its kernels with the seeds of the capture; the device counter the trainer bumps
    per step must turn them into the spec's masks at that step's counter value.  The FFN activation dropout's masks are exported
    (act_dropout wrapped with return_mask=True) and read back after the capturing step and after the next replay."""
    import vlpet_amd.act as ACT
    import vlpet_amd.train as TR
    model, cfg = _bart(0.1)
    orig = ACT.act_dropout
    seen = []

    def exporting(x, act="gelu", p=0.0, training=False, seed=None, return_mask=False):
        if not (training and p > 0) or return_mask:
            return orig(x, act, p, training, seed, return_mask)
        seed = ACT._draw_seed() if seed is None else seed
        out, keep = orig(x, act, p, training, seed, True)
        seen.append((torch.cuda.is_current_stream_capturing(), seed, float(p), keep))
        return out
    monkeypatch.setattr(ACT, "act_dropout", exporting)
    tr = TR.Trainer(model, cfg, lr=1e-3, total_steps=20, warmup_ratio=0.1, graph=True)
    b = _cuda_batch(TR.synthetic_batch("vqa", 4, cfg, "cpu", torch.Generator().manual_seed(2)))
    tr.step(b)                                 # eager first step of the shape
    tr.step(b)                                 # capture + replay
    captured = [s for s in seen if s[0]]
    assert len(tr._graphs) == 1 and len(captured) >= 2
    for step in (0, 1):
        if step:
            tr.step(b)                         # replay only
        torch.cuda.synchronize()
        ctr = int(tr.seed_ctr.item())
        for _, seed, p, keep in captured:
            km = keep.reshape(-1, keep.shape[-1])
            _assert_mask(km, S.keep_mask(km.shape[0], km.shape[1], seed, p, ctr), f"replayed act mask ctr={ctr}")
    assert int(tr.seed_ctr.item()) == 3
    tr.close()


def test_every_dropout_site_of_a_step_draws_its_own_seed(monkeypatch):
    """One eager training step of a head-dim-64 BART with dropout on: every dropout call (sublayer tails, FFN activation dropout,
    attention, the encoder's concatenation) draws a seed of its own -- no two sites share a mask."""
    import vlpet_amd.act as ACT
    import vlpet_amd.attention as ATT
    import vlpet_amd.tail as TAIL
    import vlpet_amd.train as TR
    model, cfg = _bart(0.1)
    drawn = {}
    orig = TAIL._draw_seed
    for mod, name in ((TAIL, "tail"), (ACT, "act"), (ATT, "attention")):
        def rec(name=name):
            s = orig()
            drawn.setdefault(name, []).append(s)
            return s
        monkeypatch.setattr(mod, "_draw_seed", rec)
    tr = TR.Trainer(model, cfg, lr=1e-3, total_steps=20, warmup_ratio=0.1)
    b = _cuda_batch(TR.synthetic_batch("vqa", 4, cfg, "cpu", torch.Generator().manual_seed(2)))
    loss = tr.step(b)
    assert bool(torch.isfinite(loss))
    assert set(drawn) == {"tail", "act", "attention"}, drawn.keys()
    seeds = [s for v in drawn.values() for s in v]
    assert min(len(v) for v in drawn.values()) >= 2, {k: len(v) for k, v in drawn.items()}
    assert len(set(seeds)) == len(seeds)
    tr.close()
