"""The hosts' LONG_ATTENTION_TRAIN switch (host/bart.py, host/t5.py): past the short kernels' 128 tokens an attention that needs dropout
or a gradient runs on vlpet_amd.attention's long training kernels (csrc/attn_long.hip with dropout, csrc/attn_long_bwd.hip) -- fused
q|k|v and fused cross keys read in place -- and nowhere else; with the switch off nothing of it is reached.  (The helpers are those of
tests/test_gpu_long_hosts.py, restated.)"""
import pytest
import torch

from gpu_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = 200


def _switch(monkeypatch, on):
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    monkeypatch.setattr(HB, "LONG_ATTENTION_TRAIN", on)
    monkeypatch.setattr(HT, "LONG_ATTENTION_TRAIN", on)


def _attention_module(kind, p=0.0):
    """-> call(hidden) of one frozen bf16 self-attention module with a padding mask (T5: + its relative position bias)"""
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    torch.manual_seed(3)
    if kind == "bart":
        att = HB.BartAttention(HB.vlpet_config(), 768, 12, p)
    else:
        att = HT.T5Attention(HT.vlt5_config(dropout_rate=p), False, has_relative_attention_bias=True)
    att = att.to(DEV).bfloat16().requires_grad_(False)

    def call(hidden, lens):
        B, n, _ = hidden.shape
        keep = torch.arange(n, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]
        if kind == "bart":
            return att(hidden, attn_mask=keep[:, None, None, :])
        spec = HT.AttnSpec(att.compute_bias(n, n), keep.float(), causal=False)
        return att(hidden, spec)
    return att, call


def _hidden(B, n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(B, n, 768, generator=g).bfloat16().to(DEV)


def _run(call, n=L, seed=11):
    """forward + backward of one module call -> (output, input gradient, long training calls it made)"""
    import vlpet_amd.attention as A
    x = _hidden(2, n).requires_grad_(True)
    g = torch.Generator().manual_seed(7)
    dout = torch.randn(2, n, 768, generator=g).bfloat16().to(DEV)
    torch.manual_seed(seed)
    n0 = A.LONG_TRAIN_CALLS
    out = call(x, [n, n - 17])
    out.backward(dout)
    return out.detach(), x.grad, A.LONG_TRAIN_CALLS - n0


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_train_mode_with_a_gradient_switch_on_against_off(kind, monkeypatch):
    att, call = _attention_module(kind)
    att.train()
    _switch(monkeypatch, False)
    off = _run(call)
    assert off[2] == 0
    _switch(monkeypatch, True)
    on1, on2 = _run(call), _run(call)
    assert on1[2] == 1 and on2[2] == 1
    errs = rel_err(on1[0], off[0]), rel_err(on1[1], off[1])
    print(f"{kind}: switch on vs off: out {errs[0]:.3e}  dx {errs[1]:.3e}")
    assert errs[0] <= 2e-2 and errs[1] <= 2e-2, errs
    assert torch.equal(on1[0], on2[0]) and torch.equal(on1[1], on2[1])


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_dropout_with_the_same_torch_seed_is_bitwise_repeatable(kind, monkeypatch):
    att, call = _attention_module(kind, p=0.1)
    att.train()
    _switch(monkeypatch, True)
    a, b = _run(call), _run(call)
    assert a[2] == 1 and b[2] == 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _run(call, seed=12)                                       # (and the mask does follow the seed)
    assert not torch.equal(a[0], c[0])


@pytest.mark.parametrize("kind", ["bart", "t5"])
@pytest.mark.parametrize("case", ["short", "no_grad"])
def test_paths_that_never_reach_the_training_kernels(kind, case, monkeypatch):
    """a length the short kernels own, and a call that needs neither dropout nor a gradient: the switch-off numbers"""
    import vlpet_amd.attention as A
    att, call = _attention_module(kind)
    att.train(case == "short")
    n = 128 if case == "short" else L
    outs = []
    for on in (False, True):
        _switch(monkeypatch, on)
        n0 = A.LONG_TRAIN_CALLS
        if case == "short":
            outs.append(_run(call, n)[0])
        else:
            with torch.no_grad():
                outs.append(call(_hidden(2, n), [n, n - 17]))
        assert A.LONG_TRAIN_CALLS == n0
    assert torch.equal(outs[0], outs[1])


def test_teacher_forced_decoder_reads_the_fused_cross_keys_in_place(monkeypatch):
    """a BART decoder's cross-attention against a 200-token encoder output that needs a gradient: the keys are column blocks of the
    layers' fused key projection, read in place, and every layer's dk goes into the shared slot's buffer"""
    import vlpet_amd.attention as A
    import vlpet_amd.host.bart as HB
    import vlpet_amd.train as TR
    torch.manual_seed(21)
    cfg = HB.vlpet_config(encoder_layers=2, decoder_layers=2, vocab_size=1000, feat_dim=512, n_boxes=64, tasks="tvqa,how2qa,tvc,yc2c")
    model = HB.VLBart(cfg)
    TR.trainable_names(model, cfg)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    model.eval()                                                  # (no dropout: the two paths are comparable; the gradient is what asks)
    B = 3
    g = torch.Generator().manual_seed(9)
    enc0 = torch.randn(B, L, 768, generator=g).bfloat16().to(DEV)
    keep = torch.arange(L, device=DEV)[None, :] < torch.tensor([L, 150, 77], device=DEV)[:, None]
    mask = keep[:, None, None, :]
    dec_in = torch.randint(3, 1000, (B, 6), generator=g).to(DEV)

    seen = []
    real_fn, real_block = A.long_attention_train, A.KeyGradSlot.block

    def spy_fn(q, k, v, *a, **kw):
        seen.append(("call", k.shape[1], k.is_contiguous(), k.stride(1), kw.get("k_slot") is not None))
        return real_fn(q, k, v, *a, **kw)

    def spy_block(self, k, index):
        seen.append(("dk", k.shape[1], index))
        return real_block(self, k, index)

    monkeypatch.setattr(A, "long_attention_train", spy_fn)
    monkeypatch.setattr(A.KeyGradSlot, "block", spy_block)
    res = []
    for on in (False, True):
        _switch(monkeypatch, on)
        del seen[:]
        enc = enc0.clone().requires_grad_(True)
        n0 = A.LONG_TRAIN_CALLS
        out = model.model.decoder(dec_in, enc, mask, "tvc")
        out.float().square().mean().backward()
        res.append((out.detach(), enc.grad))
        if on:
            assert A.LONG_TRAIN_CALLS == n0 + 2                   # one cross-attention per decoder layer; self-attention (6 tokens) stays short
            calls = [s for s in seen if s[0] == "call"]
            assert calls == [("call", L, False, 2 * 768, True)] * 2, calls         # a block of the [B, L, 2 * 768] buffer, with the slot
            assert sorted(s[2] for s in seen if s[0] == "dk" and s[1] == L) == [0, 1]
        else:
            assert A.LONG_TRAIN_CALLS == n0 and not seen
    errs = rel_err(res[1][0], res[0][0]), rel_err(res[1][1], res[0][1])
    print(f"decoder: switch on vs off: out {errs[0]:.3e}  d enc {errs[1]:.3e}")
    assert errs[0] <= 2e-2 and errs[1] <= 2e-2, errs
