"""Greedy generation (VLBart.generate / VLT5.generate, vlpet_amd.decode) without a GPU: the ABI argument checks of the two decode
entry points, and the host's cached generate() under the CPU reference ops against the reference models' own uncached greedy decoding
(tests/golden/gen_*.npz, make_generate_goldens.py): token for token, every step's logits within 1e-3."""
import glob
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
GEN_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G, "gen_*.npz")))
WHICH = {"vlbart_tiny_d64": "vlpet_large", "vlbart_tiny_lora_d64": "lora", "vlt5_tiny_d64": "t5", "vlbart_tiny_video_d64": "video"}


def load_gen(name):
    z = np.load(os.path.join(G, name + ".npz"), allow_pickle=False)
    max_length, min_length, ngram, eos, pad, start = (int(v) for v in z["settings"])
    return dict(fixture=str(z["fixture"]), task=str(z["task"]), ids=torch.from_numpy(z["ids"]),
                vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])), out=torch.from_numpy(z["out"]),
                logits=torch.from_numpy(z["logits"]), max_length=max_length, min_length=min_length, ngram=ngram, eos=eos, pad=pad,
                start=start)


def build_host(fixture):
    from test_host_golden import FIXTURES, _build, _load
    name, over = FIXTURES[WHICH[fixture]]
    sd = _load(name)[0]
    return _build(sd, over)[0]


def run_generate(model, g, dev):
    """generate() on ``dev``; returns (ids, per-step logits [B, steps, V]) -- the logits recorded where the step hands them to
    greedy_pick"""
    import vlpet_amd.decode as D
    seen = []
    pick = D.greedy_pick

    def recording(logits, vocab, *a, **k):
        seen.append(logits[:, :vocab].float().cpu().clone())
        return pick(logits, vocab, *a, **k)
    D.greedy_pick = recording
    try:
        out = model.generate(g["ids"].to(dev), tuple(t.to(dev) for t in g["vis"]), g["task"], max_length=g["max_length"],
                             min_length=g["min_length"], no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"])
    finally:
        D.greedy_pick = pick
    return out.cpu(), torch.stack(seen, 1)


def check_against_fixture(out, logits, g, tol):
    assert out.shape == g["out"].shape and torch.equal(out, g["out"]), (out.tolist(), g["out"].tolist())
    torch.testing.assert_close(logits, g["logits"], rtol=tol, atol=tol)


def test_the_fixtures_exercise_finish_pad_and_both_processors():
    gs = [load_gen(n) for n in GEN_FIXTURES]
    assert len(gs) >= 5 and {g["fixture"] for g in gs} == set(WHICH)
    assert any(g["min_length"] > 1 and g["ngram"] == 2 for g in gs)
    # some row emits eos before the last step while another one goes on (pad emitted after eos)
    assert any((g["out"][:, 1:-1] == g["eos"]).any(1).any() and (g["out"][:, 1:] != g["eos"]).all(1).any() for g in gs)


def test_decode_entry_points_reject_bad_arguments_without_gpu():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert lib.vlpet_version() >= 620
    A = 4096                  # a 16-byte aligned non-NULL value: every call below returns before it could be dereferenced

    def attn(q=A, k=A, v=A, o=A, kn=None, vn=None, pos=0, ld=256, ldk=256, D=64, H=4, Lk=56, B=2, dt=1, mask=None, bias=None, lm=0):
        return lib.vlpet_attn_decode(q, ld, k, v, ldk, 56 * ldk, ldk, 56 * ldk, kn, vn, ld, pos, mask, lm, bias, lm, o, ld, B, H, D,
                                     Lk, 0.125, dt, None)
    assert attn(q=None) == -5 and attn(o=None) == -5 and attn(kn=A) == -5           # NULL; k_new without v_new
    assert attn(dt=7) == -6                                                            # dtype
    assert attn(D=32) == -1 and attn(D=128) == -1 and attn(Lk=1025) == -1 and attn(B=0) == -1
    assert attn(kn=A, vn=A, pos=56) == -1 and attn(kn=A, vn=A, pos=-1) == -1        # append row outside the cache
    assert attn(ld=128) == -1                                                          # row stride below H * D
    assert attn(mask=A, lm=8) == -1                                                    # mask row shorter than Lk
    assert attn(q=A + 8) == -3 and attn(ld=260) == -3 and attn(ldk=260) == -3         # alignment / strides % 8

    def pick(lg=A, ids=A, V=500, ld=504, pos=0, ldi=20, eos=2, ngram=0, B=3, dt=1):
        return lib.vlpet_greedy_pick(lg, ld, V, ids, ldi, pos, A, A, B, eos, 1, 0, ngram, dt, None)
    assert pick(lg=None) == -5 and pick(ids=None) == -5
    assert pick(dt=3) == -6
    assert pick(ld=496) == -1 and pick(V=70000, ld=70000) == -1 and pick(pos=19) == -1 and pick(eos=500) == -1
    assert pick(ngram=-1) == -1 and pick(B=0) == -1
    assert pick(lg=A + 4) == -3 and pick(ld=508) == -3 and pick(ids=A + 4) == -3


@pytest.mark.parametrize("name", GEN_FIXTURES)
def test_generate_matches_reference_greedy_cpu(name):
    from oracle.host_patch import cpu_reference_ops
    g = load_gen(name)
    model = build_host(g["fixture"])
    with cpu_reference_ops():
        out, logits = run_generate(model, g, "cpu")
    check_against_fixture(out, logits, g, 1e-3)
    assert model.training            # generate() ran in eval mode and restored the mode it found
