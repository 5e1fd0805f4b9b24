"""Prompt tuning on the product path (GPU): the input-assembly kernels with a broadcast prompt in front (csrc/prefix_cat.hip) against
tests/prompt_spec.py, ``act.prefix_concat_dropout`` against the torch composition, and the two reference fixtures
(tests/golden/make_prompt_goldens.py) on VLBart / VLT5: logits, training, generation, graph replay.

Bounds.  Forward, da, dv: one product in fp32 and one rounding to the IO dtype -- restated exactly on the host, compared bit for bit.
dpre [P, d] = sum over the batch: fp32 accumulation of B terms in ANY order is within (B - 1) * 2^-24 * sum |term| of the exact sum
(Higham, Accuracy and Stability of Numerical Algorithms, 4.2), each term carries one product rounding (2^-24 |term|), and the bf16 result
one final rounding (2^-9 relative, stated as 2^-8): |err| <= 2^-8 |ref| + B * 2^-23 * sum |term| (bf16), B * 2^-23 * sum |term| (fp32)."""
import functools

import numpy as np
import pytest
import torch

import dropout_spec as DS
import prompt_cases as C
import prompt_spec as PS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x1F2E3D4C5B6A7988
SENTINEL = 123.0
# (B, P, La, Lv, d)
SHAPES = [(1, 1, 1, 1, 8),            # smallest extents
          (2, 5, 7, 3, 64),           # odd lengths
          (33, 40, 20, 36, 768),      # ragged last batch chunk (17 chunks of 2, the last one holds 1); more than one block everywhere
          (67, 3, 1, 49, 776),        # d / 8 odd; 23 chunks of 3, the last one holds 1
          (64, 2, 3, 2, 16)]          # B on a chunk boundary: 32 full chunks of 2, the largest chunk count
DTYPES = {torch.float32: 0, torch.bfloat16: 1}


@pytest.fixture(autouse=True)
def _no_seed_counter_left_behind():
    yield
    from vlpet_amd import _lib
    _lib.load().vlpet_set_seed_counter(None)


def _set_ctr(value):
    from vlpet_amd import _lib
    lib = _lib.load()
    if value is None:
        lib.vlpet_set_seed_counter(None)
        return None
    t = torch.tensor([value], dtype=torch.int64, device=DEV)
    assert lib.vlpet_set_seed_counter(t.data_ptr()) == 0
    return t


def _nonzero(shape, g):
    """Random values bounded away from 0 and exactly representable in bf16 (so both IO dtypes see the same numbers)."""
    x = torch.randn(*shape, generator=g)
    return ((x.sign() + (x == 0).float()) * (x.abs() + 0.25)).bfloat16().float()


@functools.lru_cache(maxsize=None)
def _case(shape, p, ctr):
    """Inputs and the spec's results for one (shape, p, counter): computed once, shared by both IO dtypes, never modified."""
    B, P, La, Lv, d = shape
    g = torch.Generator().manual_seed(sum(shape) + int(p * 100))
    pre, a, v, dx = (_nonzero(s, g) for s in ((P, d), (B, La, d), (B, Lv, d), (B, P + La + Lv, d)))
    keep = PS.keep(B, P, La, Lv, d, SEED, p, ctr)
    dpre, _, _, mag = PS.backward(dx.numpy(), P, La, Lv, SEED, p, ctr)
    return dict(pre=pre, a=a, v=v, dx=dx, keep=torch.from_numpy(keep), dpre=dpre, mag=mag)


def _scaled(src, keep, p, dtype):
    """source * keep_scale in float arithmetic, rounded to the IO dtype; +0 where the spec drops"""
    s = torch.tensor(float(PS.scale(p)), dtype=torch.float32)
    return torch.where(keep, src.float() * s, torch.zeros(())).to(dtype)


def _same_bits(got, want):
    it = torch.int32 if want.dtype == torch.float32 else torch.int16
    return torch.equal(got.detach().cpu().contiguous().view(it), want.contiguous().view(it))


def _bwd(lib, dx, shape, p, dtype, want=(True, True, True)):
    """vlpet_prefix_concat_dropout_bwd into sentinel-filled outputs; an output that is not wanted is passed as NULL"""
    B, P, La, Lv, d = shape
    outs = [torch.full(s, SENTINEL, dtype=dtype, device=DEV) for s in ((P, d), (B, La, d), (B, Lv, d))]
    ws = torch.empty(lib.vlpet_prefix_concat_ws_bytes(B, P, d) // 4, dtype=torch.float32, device=DEV) if want[0] else None
    ptr = [o.data_ptr() if w else None for o, w in zip(outs, want)]
    rc = lib.vlpet_prefix_concat_dropout_bwd(dx.data_ptr(), ptr[0], ptr[1], ptr[2], None if ws is None else ws.data_ptr(), B, P, La, Lv, d,
                                             p, SEED, DTYPES[dtype], None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("ctr", [None, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_the_spec(shape, p, dtype, ctr):
    from vlpet_amd import _lib
    lib = _lib.load()
    B, P, La, Lv, d = shape
    L = P + La + Lv
    c = _case(shape, p, ctr if p > 0 else None)
    keep = c["keep"]
    pre, a, v, dx = (c[k].to(dtype) for k in ("pre", "a", "v", "dx"))
    counter = _set_ctr(ctr)
    # ---- forward, into rows [3, 3 + B * L) of a larger buffer: bit for bit, and nothing outside the slice is touched
    buf = torch.full((3 + B * L + 2, d), SENTINEL, dtype=dtype, device=DEV)
    x = buf[3:3 + B * L]
    gp, ga, gv = pre.to(DEV), a.to(DEV), v.to(DEV)
    rc = lib.vlpet_prefix_concat_dropout_fwd(gp.data_ptr(), ga.data_ptr(), gv.data_ptr(), x.data_ptr(), B, P, La, Lv, d, p, SEED,
                                             DTYPES[dtype], None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    src = torch.cat([pre.expand(B, -1, -1), a, v], 1)
    assert _same_bits(x.view(B, L, d), _scaled(src, keep, p, dtype))
    assert bool((buf[:3] == SENTINEL).all()) and bool((buf[3 + B * L:] == SENTINEL).all())
    if p == 0.0:
        assert torch.equal(x.view(B, L, d).cpu(), src)
    # ---- backward: da, dv bit for bit; dpre within the accumulation bound; twice the same bits
    gdx = dx.to(DEV)
    dpre, da, dv = _bwd(lib, gdx, shape, p, dtype)
    assert _same_bits(da, _scaled(dx[:, P:P + La], keep[:, P:P + La], p, dtype))
    assert _same_bits(dv, _scaled(dx[:, P + La:], keep[:, P + La:], p, dtype))
    err = np.abs(dpre.float().cpu().numpy().astype(np.float64) - c["dpre"])
    bound = B * 2.0 ** -23 * c["mag"] + (2.0 ** -8 * np.abs(c["dpre"]) if dtype == torch.bfloat16 else 0.0)
    worst = float((err - bound).max())
    print(f"dpre {shape} p={p} {dtype} ctr={ctr}: max err {err.max():.3e}, max err - bound {worst:.3e}")
    assert worst <= 0.0, (float(err.max()), worst)
    dpre2 = _bwd(lib, gdx, shape, p, dtype)[0]
    assert _same_bits(dpre2, dpre.cpu())
    # ---- each output left out in turn: the others are what they were, and the one left out is not written
    for drop in range(3):
        want = tuple(i != drop for i in range(3))
        outs = _bwd(lib, gdx, shape, p, dtype, want)
        for i, (o, full) in enumerate(zip(outs, (dpre, da, dv))):
            if want[i]:
                assert _same_bits(o, full.cpu()), (drop, i)
            else:
                assert bool((o == SENTINEL).all()), (drop, i)
    del counter


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_step_counter_changes_the_mask_and_eval_mode_is_the_concatenation(dtype):
    from vlpet_amd.act import prefix_concat_dropout
    shape = SHAPES[1]
    B, P, La, Lv, d = shape
    c = _case(shape, 0.1, None)
    pre, a, v = (c[k].to(DEV, dtype) for k in ("pre", "a", "v"))
    src = torch.cat([pre.expand(B, -1, -1), a, v], 1)
    assert torch.equal(prefix_concat_dropout(pre, a, v, 0.1, training=False), src)
    masks = []
    for ctr in (None, 0, 1, (1 << 40) + 3):
        counter = _set_ctr(ctr)
        x = prefix_concat_dropout(pre, a, v, 0.1, training=True, seed=SEED)
        torch.cuda.synchronize()
        want = PS.keep(B, P, La, Lv, d, SEED, 0.1, ctr)
        assert np.array_equal((x != 0).cpu().numpy(), want), ctr
        masks.append(want)
        del counter
    assert np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2]) and not np.array_equal(masks[2], masks[3])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_autograd_matches_the_torch_composition_under_the_same_mask(p, dtype):
    """Gradients of pre, a and v -- with pre also feeding a second consumer, so that its gradient is accumulated, not assigned.
    fp32: the two sides differ by the order of a 6-term fp32 sum (1e-5).  bf16: each side rounds the prompt's gradient to bf16 and
    then the sum of the two consumers' gradients again -- two roundings of 2^-9 each, on either side (2^-7 of the magnitude)."""
    from vlpet_amd.act import prefix_concat_dropout
    B, P, La, Lv, d = 6, 5, 7, 3, 64
    g = torch.Generator().manual_seed(17)
    pre0, a0, v0, w, w2 = (_nonzero(s, g).to(DEV, dtype) for s in ((P, d), (B, La, d), (B, Lv, d), (B, P + La + Lv, d), (P, d)))

    def leaves():
        return [t.clone().requires_grad_(True) for t in (pre0, a0, v0)]
    pre, a, v = leaves()
    x = prefix_concat_dropout(pre, a, v, p, training=True, seed=SEED)
    ((x.float() * w.float()).sum() + (pre.float() * w2.float()).sum()).backward()
    mask = (x.detach() != 0)
    assert np.array_equal(mask.cpu().numpy(), PS.keep(B, P, La, Lv, d, SEED, p))
    rp, ra, rv = leaves()
    scale = float(PS.scale(p))
    xr = torch.cat([rp.expand(B, -1, -1), ra, rv], 1) * mask.to(dtype) * scale
    assert torch.equal(xr.detach(), x.detach()) or dtype == torch.bfloat16
    ((xr.float() * w.float()).sum() + (rp.float() * w2.float()).sum()).backward()
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    for got, ref, what in ((pre.grad, rp.grad, "pre"), (a.grad, ra.grad, "a"), (v.grad, rv.grad, "v")):
        assert got.dtype == dtype and got.shape == ref.shape
        lim = tol * max(1.0, float(ref.float().abs().max()))
        assert float((got.float() - ref.float()).abs().max()) <= lim, what
    # a frozen prompt / frozen sides: only the wanted gradients come back
    pre, a, v = leaves()
    a.requires_grad_(False)
    v.requires_grad_(False)
    prefix_concat_dropout(pre, a, v, p, training=True, seed=SEED).backward(w)
    assert a.grad is None and v.grad is None and pre.grad is not None


# ------------------------------------------------------------------------------------------------ hosts
@pytest.fixture
def _switch():
    import vlpet_amd.act as ACT
    saved = ACT.FUSE_PREFIX_CONCAT
    yield ACT
    ACT.FUSE_PREFIX_CONCAT = saved


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_eval_logits_and_training_losses_match_the_reference(kind, fused, _switch):
    """fp32: eval logits and per-token losses within 1e-3, the five training losses and the final trainables (test_host_golden._check),
    with the fused assembly and with ``FUSE_PREFIX_CONCAT = False``; the fused run must really take the kernels."""
    from test_host_golden import _check
    import vlpet_amd.functional as VF
    _switch.FUSE_PREFIX_CONCAT = fused
    sd, batches, ref_losses, hp, final = C.fixture(kind)
    model, cfg, names, _ = C.build(kind)
    calls = []
    timed = VF._timed
    saved = _switch._timed
    _switch._timed = lambda name, rows, fn: (calls.append(name), timed(name, rows, fn))[1]
    try:
        _check(model.to(DEV), cfg, names, batches, ref_losses, hp, final, DEV, 1e-3)
    finally:
        _switch._timed = saved
    n_f, n_b = calls.count("prefix_concat_drop_fwd"), calls.count("prefix_concat_drop_bwd")
    if fused:
        assert n_f >= 8 and n_b >= 5, calls             # three eval batches + five steps forward, five backward
    else:
        assert (n_f, n_b) == (0, 0), calls


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_bf16_eval_logits_are_within_the_pinned_tolerance(kind):
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(kind)[1]
    model, cfg, names, _ = C.build(kind)
    model.to(DEV)
    TR.cast_frozen(model, torch.bfloat16)
    model.eval()
    with torch.no_grad():
        for b in batches:
            bb = _to(b, DEV)
            per, logits = model(bb["input_ids"], bb["vis_inputs"], bb["labels"], b["task"])
            torch.testing.assert_close(logits.float().cpu(), b["logits"], rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_training_step_with_dropout_reaches_the_prompt(kind):
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture(kind)[1]
    model, cfg, names, _ = C.build(kind, dropout=0.1)
    model.to(DEV).train()
    torch.manual_seed(3)
    b = _to(batches[0], DEV)
    per, _ = model(b["input_ids"], b["vis_inputs"], b["labels"], b["task"])
    loss = TR.task_loss(per.float(), b["labels"], b["scores"], b["task"])
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    mine = [n for n in names if ".prompts.vqa." in n]
    assert len(mine) == 5
    for n in mine:
        g = params[n].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    others = [n for n in names if "prompt_modules" in n and n not in mine]       # T5: the other tasks' prompts get nothing
    assert len(others) == (0 if kind == "bart" else 15) and all(params[n].grad is None for n in others)


def test_greedy_and_beam_tokens_equal_the_reference():
    from test_beam import check_against_fixture as check_beam, run_beam
    from test_generate import check_against_fixture, run_generate
    g = C.load_gen()
    model = C.build("bart")[0].to(DEV)
    out, logits = run_generate(model, g, DEV)
    check_against_fixture(out, logits, g, 1e-3)
    b = C.load_beam()
    C.sharpen(model, b["logit_scale"])
    out, scores = run_beam(model, b, DEV)
    check_beam(out, scores, b)


@pytest.mark.parametrize("num_beams", [1, 3])
@pytest.mark.parametrize("kind", ["bart", "t5"])
def test_replayed_decode_step_gives_the_eager_tokens(kind, num_beams):
    import vlpet_amd.decode as D
    D.clear_graphs()
    if kind == "bart":
        g = C.load_gen()
        ids, vis, task = g["ids"], g["vis"], g["task"]
        kw = dict(max_length=g["max_length"], min_length=g["min_length"], no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"],
                  num_beams=num_beams)
    else:
        b = C.fixture("t5")[1][0]
        ids, vis, task, kw = b["input_ids"], b["vis_inputs"], b["task"], dict(max_length=8, min_length=8, num_beams=num_beams)
    model = C.build(kind)[0].to(DEV)
    ids, vis = ids.to(DEV), tuple(t.to(DEV) for t in vis)
    try:
        eager = model.generate(ids, vis, task, **kw)
        s0 = dict(D.GRAPH_STATS)
        outs = [model.generate(ids, vis, task, graph=True, **kw) for _ in range(3)]          # eager warm-up, capture, replay
        d = {k: D.GRAPH_STATS[k] - s0[k] for k in s0}
        assert d["captures"] == 1 and d["replays"] > 0, d
        for o in outs:
            assert torch.equal(o, eager), (o.tolist(), eager.tolist())
    finally:
        D.clear_graphs()


def test_a_captured_trainer_step_has_the_eager_steps_loss():
    """Trainer(graph=True) on the BART fixture (one shared prompt: every trainable parameter gets a gradient in every step, so the step
    can be captured) at p = 0: eager step, capture + replay, replay -- each loss equal to the eager trainer's."""
    import copy
    import vlpet_amd.train as TR
    from test_host_golden import _to
    batches = C.fixture("bart")[1]
    model, cfg, names, _ = C.build("bart")
    m_eager, m_graph = copy.deepcopy(model).to(DEV), copy.deepcopy(model).to(DEV)
    b = _to(batches[0], DEV)
    tre = TR.Trainer(m_eager, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1)
    trg = TR.Trainer(m_graph, cfg, lr=1e-2, total_steps=20, warmup_ratio=0.1, graph=True)
    assert trg.graph
    le = [float(tre.step(b)) for _ in range(3)]
    lg = [float(trg.step(b)) for _ in range(3)]
    assert len(trg._graphs) == 1
    for x, y in zip(lg, le):
        assert abs(x - y) <= 1e-5 * abs(y), (lg, le)
