"""Short-sequence attention (csrc/attn.hip, vlpet_amd.attention) against the eager chain of BartAttention.forward
(my_transformers/modeling_bart.py:283-566: scores, mask, softmax, dropout, weighted sum) in fp32 on the same bf16 inputs,
with the dropout mask the kernel applied exported so that forward and backward compare element for element."""
import contextlib

import pytest
import torch

from gpu_cases import rel_err

pytestmark = pytest.mark.gpu

H = 12


def _eager(q, k, v, key_mask, causal, keep, p, bias=None, scale=64 ** -0.5):
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    sh = lambda t, L: t.view(B, L, H, 64).transpose(1, 2)
    s = (sh(q, Lq) @ sh(k, Lk).transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias[None]
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :].bool(), float("-inf"))
    if causal:
        i = torch.arange(Lq)[:, None]; j = torch.arange(Lk)[None, :]
        s = s.masked_fill(j > i + (Lk - Lq), float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.float() / (1.0 - p)
    return (pr @ sh(v, Lk)).transpose(1, 2).reshape(B, Lq, H * 64)


CASES = [  # B, Lq, Lk, causal, masked, p
    (3, 56, 56, False, False, 0.0),
    (3, 56, 56, False, True, 0.1),
    (2, 92, 92, False, False, 0.1),
    (3, 76, 76, False, True, 0.1),        # six units: the six-wave backward
    (2, 70, 40, False, True, 0.0),        # five units
    (2, 128, 128, False, True, 0.1),
    (4, 5, 5, True, False, 0.1),
    (4, 20, 20, True, False, 0.0),
    (3, 5, 56, False, True, 0.1),
    (2, 33, 97, False, False, 0.5),
    (2, 1, 1, True, False, 0.0),
    # batches of several workgroup rounds (the small cases above are one partial round): four units, three (cross attention), two, six,
    # five, eight
    (90, 56, 56, False, True, 0.1),
    (90, 20, 56, False, True, 0.1),
    (96, 5, 5, True, False, 0.1),
    (44, 92, 92, False, False, 0.1),
    (44, 70, 40, False, True, 0.0),
    (90, 33, 97, False, False, 0.5),
    (44, 128, 128, False, True, 0.1),
    (90, 20, 20, True, True, 0.1),          # decoder self-attention: causal + padding mask + dropout over several rounds
    (90, 20, 56, False, False, 0.0),
]


@pytest.mark.parametrize("B,Lq,Lk,causal,masked,p", CASES)
def test_short_attention_matches_the_eager_chain(B, Lq, Lk, causal, masked, p):
    from vlpet_amd.attention import short_attention
    g = torch.Generator().manual_seed(Lq * 131 + Lk)
    mk = lambda L: (torch.randn(B, L, H * 64, generator=g) * 1.5).bfloat16()
    q, k, v, do = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
    key_mask = None
    if masked and causal:                                       # decoder self-attention: padding is a suffix (key 0 is visible to every query)
        lens = torch.randint(1, Lk + 1, (B,), generator=g)
        key_mask = torch.arange(Lk)[None, :] < lens[:, None]
    elif masked:
        key_mask = torch.rand(B, Lk, generator=g) > 0.25
        key_mask[:, -1] = True                                  # (at least one key per row)
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    out = short_attention(qg, kg, vg, H, None if key_mask is None else key_mask.cuda(), causal, p, True, seed=99,
                          return_mask=p > 0)
    keep = None
    if p > 0:
        out, keep = out
        keep = keep.cpu()
        assert keep.shape == (B, H, Lq, Lk)
        frac = float(keep.float().mean())
        n = keep.numel()
        assert abs(frac - (1 - p)) < 4.0 * (p * (1 - p) / n) ** 0.5 + 1e-3, frac
    out.backward(do.cuda())
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = _eager(qr, kr, vr, key_mask, causal, keep, p)
    ref.backward(do.float())
    tol = 2e-2                                                  # bf16 outputs and bf16 probabilities in the second product
    def close(a, r):          # (a single visible key makes dq and dk exactly zero in the reference: absolute floor)
        return float((a.float().cpu() - r).abs().max()) <= tol * max(float(r.abs().max()), 1e-2)
    assert rel_err(out, ref) <= tol
    assert close(qg.grad, qr.grad)
    assert close(kg.grad, kr.grad)
    assert close(vg.grad, vr.grad)


BIAS_CASES = [  # B, Lq, Lk, causal, masked, p      (T5: scale 1, a [H, Lq, Lk] bias shared by the batch -- my_transformers/modeling_t5.py:520-560, 640-660)
    (3, 56, 56, False, True, 0.1),          # encoder self-attention of the image-text tasks (20 text + 36 visual tokens)
    (2, 92, 92, False, True, 0.1),          # nlvr
    (2, 76, 76, False, False, 0.0),
    (4, 5, 5, True, False, 0.1),            # decoder self-attention: relative bias + causal
    (3, 20, 20, True, False, 0.0),
    (2, 33, 97, False, True, 0.1),          # ragged against the 32-wide padding of the bias
    (2, 128, 128, False, False, 0.0),
    (90, 56, 56, False, True, 0.1),         # several workgroup rounds (see CASES)
    (44, 92, 92, False, True, 0.1),
    (90, 20, 20, True, False, 0.0),
    (44, 33, 97, False, True, 0.1),
]


@pytest.mark.parametrize("B,Lq,Lk,causal,masked,p", BIAS_CASES)
def test_short_attention_with_a_shared_bias_matches_the_eager_chain(B, Lq, Lk, causal, masked, p):
    from vlpet_amd.attention import AttnBias, short_attention
    g = torch.Generator().manual_seed(Lq * 17 + Lk)
    mk = lambda L: (torch.randn(B, L, H * 64, generator=g) * 0.35).bfloat16()      # scale 1: keep the scores of 64-wide heads in softmax range
    q, k, v, do = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
    bias = torch.randn(H, Lq, Lk, generator=g) * 2.0
    key_mask = None
    if masked:
        key_mask = torch.rand(B, Lk, generator=g) > 0.25
        key_mask[:, -1] = True
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    out = short_attention(qg, kg, vg, H, None if key_mask is None else key_mask.cuda(), causal, p, True, scale=1.0, seed=7,
                          return_mask=p > 0, bias=AttnBias(bias.cuda()[None]))
    keep = None
    if p > 0:
        out, keep = out
        keep = keep.cpu()
    out.backward(do.cuda())
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = _eager(qr, kr, vr, key_mask, causal, keep, p, bias=bias, scale=1.0)
    ref.backward(do.float())
    tol = 2e-2
    def close(a, r):
        return float((a.float().cpu() - r).abs().max()) <= tol * max(float(r.abs().max()), 1e-2)
    assert rel_err(out, ref) <= tol
    assert close(qg.grad, qr.grad) and close(kg.grad, kr.grad) and close(vg.grad, vr.grad)
    # and the bias really took part: without it the output differs
    out0 = short_attention(qg.detach(), kg.detach(), vg.detach(), H, None if key_mask is None else key_mask.cuda(), causal, 0.0, False, scale=1.0)
    ref0 = _eager(q.float(), k.float(), v.float(), key_mask, causal, None, 0.0, bias=bias, scale=1.0)
    assert rel_err(out0, ref0) > 5e-2


def test_t5_host_attention_fast_path_equals_the_dense_sdpa_path():
    """host/t5.py: a VLT5 with 64-wide heads in bf16 runs its three attentions (encoder self with the text-block relative bias +
    padding, decoder self with relative bias + causal, cross with padding) on the on-chip kernels; EAGER_ATTENTION = True sends the
    same model through torch's SDPA with the merged dense mask the reference builds.  Same loss, same gradients."""
    import copy
    import vlpet_amd.host.t5 as HT
    import vlpet_amd.train as TR
    cfg = HT.vlt5_config(d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, num_decoder_layers=2, vocab_size=600,
                         feat_dim=128, adapter_down_dim=8, adapter_gating_down_dim=16, encoder_adapter_multihead_num_head=4,
                         decoder_enc_attn_value_parallel_adapter_down_dim=8, dropout_rate=0.0)
    torch.manual_seed(3)
    model = HT.VLT5(cfg)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.02)
    TR.trainable_names(model, cfg)
    model.cuda()
    TR.cast_frozen(model, torch.bfloat16)
    model.train()
    gen = torch.Generator().manual_seed(4)
    b = TR.synthetic_batch("vqa", 6, cfg, "cpu", gen)
    ids = b["input_ids"].clone()
    ids[2, 15:] = cfg.pad_token_id                    # padded rows: the key mask matters
    ids[4, 9:] = cfg.pad_token_id
    vis = tuple(t.cuda() for t in b["vis_inputs"])
    res = {}
    for mode in ("math", "sdpa", "fast"):       # torch's math SDPA (the yardstick), its default fused SDPA, the on-chip kernels
        HT.EAGER_ATTENTION = mode != "fast"
        try:
            for p in model.parameters():
                p.grad = None
            ctx = torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH) if mode == "math" else contextlib.nullcontext()
            with ctx:
                per_token, _ = model(ids.cuda(), vis, b["labels"].cuda(), "vqa")
                loss = TR.task_loss(per_token, b["labels"].cuda(), b["scores"].cuda(), "vqa")
                loss.backward()
            res[mode] = (float(loss.detach()), torch.cat([p.grad.detach().float().reshape(-1) for _, p in sorted(model.named_parameters())
                                                          if p.grad is not None]))
        finally:
            HT.EAGER_ATTENTION = False
    (lm, gm), (ls, gs), (lf, gf) = res["math"], res["sdpa"], res["fast"]
    assert gm.numel() == gf.numel() > 1000
    assert abs(lm - lf) <= 2e-3 * abs(lm), (lm, ls, lf)
    # bf16 through a 2 + 2-layer stack: two library implementations already differ by a few percent on the (small) PET gradients; the
    # on-chip kernels must sit as close to the math path as the library's fused kernels do
    err = lambda a, r: float((a - r).norm() / r.norm())
    e_fast, e_sdpa = err(gf, gm), err(gs, gm)
    assert e_fast <= max(1.5 * e_sdpa, 2e-2), (e_fast, e_sdpa)


def test_short_attention_mask_depends_on_seed_only_and_eval_has_no_dropout():
    from vlpet_amd.attention import short_attention
    q = torch.randn(2, 40, H * 64, device="cuda").bfloat16()
    _, k1 = short_attention(q, q, q, H, p=0.1, training=True, seed=5, return_mask=True)
    _, k2 = short_attention(q * 2, q, q, H, p=0.1, training=True, seed=5, return_mask=True)
    _, k3 = short_attention(q, q, q, H, p=0.1, training=True, seed=6, return_mask=True)
    assert torch.equal(k1, k2) and not torch.equal(k1, k3)
    o1 = short_attention(q, q, q, H, p=0.1, training=False)
    o2 = short_attention(q, q, q, H, p=0.0, training=True)
    assert torch.equal(o1, o2)


def test_fully_masked_row_gives_zeros():
    from vlpet_amd.attention import short_attention
    q = torch.randn(2, 8, H * 64, device="cuda").bfloat16().requires_grad_(True)
    km = torch.ones(2, 8, dtype=torch.bool, device="cuda")
    km[1] = False
    o = short_attention(q, q, q, H, km)
    assert float(o[1].abs().max()) == 0.0 and torch.isfinite(o).all()
    o.sum().backward()
    assert torch.isfinite(q.grad).all()


def test_short_attention_argument_errors():
    from vlpet_amd import _lib
    from vlpet_amd.attention import short_attention, supported
    q = torch.randn(2, 8, H * 64, device="cuda")
    assert not supported(q, q, H)                                                   # fp32: library path
    assert not supported(q.bfloat16().cpu(), q.bfloat16().cpu(), H)
    assert not supported(torch.randn(1, 200, H * 64, device="cuda").bfloat16(), q.bfloat16(), H)
    with pytest.raises(RuntimeError):
        short_attention(q, q, q, H)
    lib = _lib.load()
    x = torch.randn(1, 8, 64, device="cuda").bfloat16(); l = torch.empty(8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = lambda Lq, Lk, p: (x.data_ptr(), x.data_ptr(), x.data_ptr(), None, x.data_ptr(), l.data_ptr(), None, 1, 1, Lq, Lk, 0, 0.125, p, 0, st)
    assert lib.vlpet_attn_fwd(*args(129, 8, 0.0)) == -1
    assert lib.vlpet_attn_fwd(*args(8, 0, 0.0)) == -1
    assert lib.vlpet_attn_fwd(*args(8, 8, 1.0)) == -1
    assert lib.vlpet_attn_fwd(None, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), l.data_ptr(), None, 1, 1, 8, 8, 0, 0.125, 0.0, 0, st) == -5


@pytest.mark.parametrize("B,L,causal,masked,p", [(3, 56, False, True, 0.1), (2, 92, False, False, 0.0), (4, 5, True, False, 0.1),
                                                 (2, 128, False, True, 0.1)])
def test_fused_qkv_form_is_the_same_kernel_on_column_blocks(B, L, causal, masked, p):
    """vlpet_attn_{fwd,bwd}_ld on the q | k | v columns of one [B, L, 3E] buffer == the dense entry points on three tensors
    (same seed -> same dropout pattern): outputs and the three input gradients bit for bit."""
    from vlpet_amd.attention import short_attention, short_self_attention
    E = H * 64
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(B, L, 3 * E, generator=g) * 1.5).bfloat16().cuda()
    do = (torch.randn(B, L, E, generator=g)).bfloat16().cuda()
    km = None
    if masked:
        km = (torch.rand(B, L, generator=g) > 0.25)
        km[:, -1] = True
        km = km.cuda()
    a = qkv.clone().requires_grad_(True)
    o1 = short_self_attention(a, H, km, causal, p, True, seed=7)
    o1.backward(do)
    q, k, v = (qkv[..., i * E:(i + 1) * E].clone().requires_grad_(True) for i in range(3))
    o2 = short_attention(q, k, v, H, km, causal, p, True, seed=7)
    o2.backward(do)
    assert torch.equal(o1, o2)
    for i, t in enumerate((q, k, v)):
        assert torch.equal(a.grad[..., i * E:(i + 1) * E], t.grad), "qkv"[i]


def test_self_attention_module_fused_projection_equals_separate_projections():
    """BartAttention with frozen projections: the fused [E -> 3E] GEMM + column-block attention against the three separate
    projections (VLPET_NO_FUSED_QKV path), eval mode (no dropout), bf16: output and input gradient within bf16 GEMM rounding."""
    import vlpet_amd.host.bart as HB
    cfg = HB.vlpet_config()
    torch.manual_seed(3)
    att = HB.BartAttention(cfg, 768, 12, 0.1).cuda().to(torch.bfloat16).eval()
    for p_ in att.parameters():
        p_.requires_grad_(False)
    x = (torch.randn(5, 56, 768, device="cuda") * 0.7).bfloat16()
    mask = torch.ones(5, 1, 1, 56, dtype=torch.bool, device="cuda")
    mask[:, :, :, -7:] = False
    res = []
    for fuse in (True, False):
        HB.FUSE_QKV = fuse
        xi = x.clone().requires_grad_(True)
        y = att(xi, attn_mask=mask)
        y.float().square().sum().backward()
        res.append((y.float(), xi.grad.float()))
    HB.FUSE_QKV = True
    assert hasattr(att, "_qkv_cache")
    assert rel_err(res[0][0], res[1][0]) < 1e-2 and rel_err(res[0][1], res[1][1]) < 2e-2
    # the cache follows the source weights
    with torch.no_grad():
        att.k_proj.weight.mul_(0.5)
    xi = x.clone()
    y2 = att(xi, attn_mask=mask)
    HB.FUSE_QKV = False
    y3 = att(xi, attn_mask=mask)
    HB.FUSE_QKV = True
    assert rel_err(y2.float(), y3.float()) < 1e-2
