"""The hosts' LONG_ATTENTION switch (host/bart.py, host/t5.py): at the video configuration's 664-token encoder the attention runs on
vlpet_amd.attention's long kernel wherever no dropout and no gradient is needed -- which makes the encoder, and generate() on top of
it, bitwise reproducible -- and nowhere else; with the switch off nothing of it is reached."""
import pytest
import torch

from gpu_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
L_VIDEO = 600 + 64


def _switch(monkeypatch, on):
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    monkeypatch.setattr(HB, "LONG_ATTENTION", on)
    monkeypatch.setattr(HT, "LONG_ATTENTION", on)


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
        B, L, _ = hidden.shape
        keep = torch.arange(L, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]
        if kind == "bart":
            return att(hidden, attn_mask=keep[:, None, None, :])
        spec = HT.AttnSpec(att.compute_bias(L, L), keep.float(), causal=False)
        return att(hidden, spec)
    return att, call


def _hidden(B, L):
    g = torch.Generator().manual_seed(L)
    return torch.randn(B, L, 768, generator=g).bfloat16().to(DEV)


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_one_attention_module_takes_the_long_kernel_once_and_agrees_with_the_library_path(kind, monkeypatch):
    import vlpet_amd.attention as A
    att, call = _attention_module(kind)
    att.eval()
    x = _hidden(2, L_VIDEO)
    with torch.no_grad():
        _switch(monkeypatch, False)
        n0 = A.LONG_CALLS
        off = call(x, [L_VIDEO, 401])
        assert A.LONG_CALLS == n0
        _switch(monkeypatch, True)
        on = call(x, [L_VIDEO, 401])
        assert A.LONG_CALLS == n0 + 1
        again = call(x, [L_VIDEO, 401])
    err = rel_err(on, off)
    print(f"{kind}: switch on vs off rel_err {err:.3e}")
    assert err <= 2e-2, err
    assert torch.equal(on, again)


@pytest.mark.parametrize("kind", ["bart", "t5"])
@pytest.mark.parametrize("case", ["training_dropout", "needs_grad", "short"])
def test_paths_that_must_not_take_the_long_kernel(kind, case, monkeypatch):
    """dropout, a gradient, or a length the short kernels own: the launches and the numbers of the switch-off run"""
    import contextlib
    import vlpet_amd.attention as A
    att, call = _attention_module(kind, p=0.1 if case == "training_dropout" else 0.0)
    att.train(case == "training_dropout")
    L = 56 if case == "short" else L_VIDEO
    outs = []
    for on in (False, True):
        _switch(monkeypatch, on)
        x = _hidden(2, L).requires_grad_(case == "needs_grad")
        torch.manual_seed(11)                                   # (the library's dropout draws from torch's generator)
        n0 = A.LONG_CALLS
        with (contextlib.nullcontext() if case == "needs_grad" else torch.no_grad()):
            outs.append(call(x, [L, L - 17]))
        assert A.LONG_CALLS == n0
    assert outs[0].requires_grad == (case == "needs_grad")
    assert torch.equal(outs[0], outs[1])


def _video_model(kind):
    """a two-layer model at the video configuration's geometry (tests/test_gpu_video.py), random weights, bf16 backbone"""
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    import vlpet_amd.train as TR
    torch.manual_seed(21)
    if kind == "bart":
        cfg = HB.vlpet_config(encoder_layers=2, decoder_layers=2, vocab_size=1000, feat_dim=512, n_boxes=64, tasks="tvqa,how2qa,tvc,yc2c")
        model = HB.VLBart(cfg)
    else:
        cfg = HT.vlt5_config(num_layers=2, num_decoder_layers=2, vocab_size=1000, feat_dim=512, n_boxes=64, tasks="tvqa,how2qa,tvc,yc2c")
        model = HT.VLT5(cfg)
    TR.trainable_names(model, cfg)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(5)
    b = TR.synthetic_batch("tvc", 4, cfg, DEV, gen, no_padding=False)
    b["input_ids"][1, 400:] = cfg.pad_token_id                  # ragged text: the key mask is live
    return model.eval(), cfg, b


def _encode(model, kind, b):
    with torch.no_grad():
        if kind == "bart":
            return model.model.encoder(b["input_ids"], b["vis_inputs"], None, b["task"], False)[0]
        return model.encoder(b["input_ids"], b["vis_inputs"], None, b["task"])[0]


@pytest.mark.parametrize("kind,beams", [("bart", 5), ("t5", 1)])
def test_video_geometry_encoder_and_generate_are_reproducible_with_the_switch_on(kind, beams, monkeypatch):
    import vlpet_amd.attention as A
    model, cfg, b = _video_model(kind)
    n_enc = 2
    _switch(monkeypatch, True)
    n0 = A.LONG_CALLS
    e1 = _encode(model, kind, b)
    assert e1.shape[1] == L_VIDEO
    assert A.LONG_CALLS == n0 + n_enc                           # every encoder self-attention, nothing else
    e2 = _encode(model, kind, b)
    assert torch.equal(e1, e2)
    n0 = A.LONG_CALLS
    gen = lambda: model.generate(b["input_ids"], b["vis_inputs"], b["task"], max_length=8, num_beams=beams)
    t1 = gen()
    assert A.LONG_CALLS == n0 + n_enc                           # the decode steps run on the decode kernels
    t2 = gen()
    assert torch.equal(t1, t2)
    # and the encoder agrees with the library path
    _switch(monkeypatch, False)
    n0 = A.LONG_CALLS
    e_off = _encode(model, kind, b)
    assert A.LONG_CALLS == n0
    err = rel_err(e1, e_off)
    print(f"{kind}: encoder output, switch on vs off: rel_err {err:.3e}")
    assert err <= 2e-2, err


def test_teacher_forced_decoder_reads_the_fused_cross_keys_in_place(monkeypatch):
    """under no_grad a BART decoder's cross-attention against the 664-token encoder output takes the long kernel with its keys as
    a column block of the layers' fused key projection"""
    import vlpet_amd.attention as A
    model, cfg, b = _video_model("bart")
    with torch.no_grad():
        enc, mask = model.model.encoder(b["input_ids"], b["vis_inputs"], None, b["task"], False)
    assert mask is not None and mask.shape == (4, 1, 1, L_VIDEO)
    dec_in = b["labels"][:, :6].contiguous()
    outs = []
    for on in (False, True):
        _switch(monkeypatch, on)
        n0 = A.LONG_CALLS
        with torch.no_grad():
            outs.append(model.model.decoder(dec_in, enc, mask, b["task"]))
        assert A.LONG_CALLS == n0 + (2 if on else 0)            # one cross-attention per decoder layer; self-attention (6 tokens) stays short
    assert rel_err(outs[1], outs[0]) <= 2e-2


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_switch_off_never_reaches_the_long_kernel(kind):
    import vlpet_amd.attention as A
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    assert HB.LONG_ATTENTION is False and HT.LONG_ATTENTION is False
    model, cfg, b = _video_model(kind)
    n0 = A.LONG_CALLS
    out = model.generate(b["input_ids"], b["vis_inputs"], b["task"], max_length=6)
    assert out.shape[0] == 4 and A.LONG_CALLS == n0
