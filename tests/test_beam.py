"""Beam search (VLBart.generate / VLT5.generate with num_beams > 1, vlpet_amd.decode.beam_generate) without a GPU: the ABI argument
checks of the three new entry points, self-checks of the HF 4.2.1 restatement in tests/beam_spec.py on hand-made score tables, and
the host's cached generate() under the CPU reference ops against the reference models' own uncached beam search
(tests/golden/beam_*.npz, make_beam_goldens.py): ids exact, sequence scores within 1e-4."""
import glob
import os

import numpy as np
import pytest
import torch

import beam_spec as BS
from test_generate import WHICH, build_host

G = os.path.join(os.path.dirname(__file__), "golden")
BEAM_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G, "beam_*.npz")))


def load_beam(name):
    z = np.load(os.path.join(G, name + ".npz"), allow_pickle=False)
    K, lp, early, max_length, min_length, ngram, eos, pad, start = z["settings"].tolist()
    return dict(fixture=str(z["fixture"]), task=str(z["task"]), ids=torch.from_numpy(z["ids"]),
                vis=(torch.from_numpy(z["vis0"]), torch.from_numpy(z["vis1"])), out=torch.from_numpy(z["out"]),
                scores=torch.from_numpy(z["scores"]), K=int(K), lp=float(lp), early=bool(early), max_length=int(max_length),
                min_length=int(min_length), ngram=int(ngram), eos=int(eos), pad=int(pad), start=int(start),
                logit_scale=float(z["logit_scale"]), steps=int(z["steps"]), live=torch.from_numpy(z["live"]))


def sharpen(model, fixture, scale):
    """make_beam_goldens.sharpen on the host model: the decoder's last norm times ``scale`` (the logits times ``scale``)"""
    with torch.no_grad():
        if WHICH[fixture] == "t5":
            model.decoder.final_layer_norm.weight.mul_(scale)
        else:
            ln = model.model.decoder.layers[-1].final_layer_norm
            ln.weight.mul_(scale)
            ln.bias.mul_(scale)


def build_beam_host(g):
    model = build_host(g["fixture"])
    sharpen(model, g["fixture"], g["logit_scale"])
    return model


def run_beam(model, g, dev, **kw):
    """generate(num_beams = K) on ``dev``; returns (ids, the sequence scores beam_generate handed back)"""
    import vlpet_amd.decode as D
    seen = []
    bg = D.beam_generate

    def recording(*a, **k):
        out = bg(*a, **k)
        seen.append(out[1])
        return out
    D.beam_generate = recording
    try:
        out = model.generate(g["ids"].to(dev), tuple(t.to(dev) for t in g["vis"]), g["task"], max_length=g["max_length"],
                             min_length=g["min_length"], no_repeat_ngram_size=g["ngram"], eos_token_id=g["eos"],
                             num_beams=g["K"], length_penalty=g["lp"], early_stopping=g["early"], **kw)
    finally:
        D.beam_generate = bg
    assert len(seen) == 1
    return out.cpu(), seen[0].cpu()


def check_against_fixture(out, scores, g):
    assert out.shape == g["out"].shape and torch.equal(out, g["out"]), (out.tolist(), g["out"].tolist())
    torch.testing.assert_close(scores.double(), g["scores"].double(), rtol=0, atol=1e-4)


def test_the_fixtures_cover_the_settings():
    gs = [load_beam(n) for n in BEAM_FIXTURES]
    assert len(gs) >= 7 and {g["fixture"] for g in gs} == set(WHICH)
    assert {g["early"] for g in gs} == {False, True} and {0.6, 2.0} <= {g["lp"] for g in gs}
    assert any(g["min_length"] > 1 and g["ngram"] == 2 for g in gs)
    assert any(g["task"] == "tvc" for g in gs)
    # a run reaches max_length with items open: BART's forced eos and finalize's open beams
    assert any(g["steps"] == g["max_length"] - 1 and g["live"][:, -1].any() and WHICH[g["fixture"]] != "t5" for g in gs)


# ---- beam_spec on hand-made tables ----------------------------------------------------------------------------------------------

def test_spec_skips_an_eos_ranked_at_k_or_above():
    K, V, eos = 2, 5, 4
    hyps = [BS.Hyps(K, 1.0, False)]
    # flat [K * V] scores: rank 0 token 1 (beam 0), rank 1 token 2 (beam 1), rank 2 eos (beam 0): skipped, rank 3 token 3
    top_v = torch.tensor([[-1.0, -2.0, -3.0, -4.0]])
    top_i = torch.tensor([[1, V + 2, eos, 3]])
    done = [False]
    s, t, src, skipped = BS.process([[0], [0]], top_v, top_i, V, K, hyps, done, eos, pad=0)
    assert skipped == [] and t == [1, 2] and src == [0, 1] and len(hyps[0]) == 0         # K slots full before rank 2
    top_i = torch.tensor([[1, eos + V, eos, 3]])                                           # eos at rank 1 (kept) and rank 2 (skipped)
    s, t, src, skipped = BS.process([[0], [0]], top_v, top_i, V, K, hyps, done, eos, pad=0)
    assert skipped == [2] and t == [1, 3] and s == [-1.0, -4.0] and len(hyps[0]) == 1 and hyps[0].beams[0][0] == -2.0


def test_spec_add_evicts_the_lowest_earliest_and_tracks_worst():
    h = BS.Hyps(2, 1.0, False)
    h.add([0, 5], -4.0)                  # score -2
    h.add([0, 6], -4.0)                  # -2, a tie
    assert h.worst == -2.0 and len(h) == 2
    assert not h.add([0, 7], -5.0)       # -2.5 <= worst: not added
    h.add([0, 8], -2.0)                  # -1: evicts the earlier of the two -2s
    assert [b[1] for b in h.beams] == [[0, 6], [0, 8]] and h.worst == -2.0
    g = BS.Hyps(2, 2.0, False)
    g.add([0, 1, 2], -9.0)               # -9 / 3**2 = -1
    assert g.beams[0][0] == -1.0 and g.worst == -1.0


@pytest.mark.parametrize("early", [False, True])
def test_spec_is_done_under_both_early_stopping_values(early):
    h = BS.Hyps(2, 1.0, early)
    h.add([0, 1], -2.0)                  # -1
    assert not h.is_done(-0.1, 2)        # fewer than K hypotheses
    h.add([0, 2], -3.0)                  # -1.5: worst
    assert h.is_done(-4.0, 2)            # -1.5 >= -4 / 2 in both modes
    assert h.is_done(-2.0, 2) == early   # -1.5 < -2 / 2 = -1: only early stopping ends it


def test_spec_finalize_pads_appends_eos_and_prefers_the_last_added_on_ties():
    K, eos, pad, L = 2, 9, 0, 5
    hyps = [BS.Hyps(K, 1.0, False), BS.Hyps(K, 1.0, False)]
    hyps[0].add([1, 2], -2.0)                       # -1
    hyps[0].add([1, 3], -2.0)                       # -1, added last: wins the tie
    done = [True, False]
    ids = [[1, 4, 4, 4, 4], [1, 4, 4, 4, 4], [1, 5, 6, 7, 8], [1, 5, 6, 7, 3]]
    scores = [0.0, 0.0, -1.0, -2.0]
    out, best = BS.finalize(ids, scores, hyps, done, K, L, eos, pad)
    assert out.tolist() == [[1, 3, eos, pad, pad], [1, 5, 6, 7, 8]]   # width min(5 + 1, 5); no eos after a max_length row
    assert best.tolist() == [-1.0, -0.2]


def test_spec_forced_eos_and_bans_on_the_log_probs():
    logits = torch.tensor([[1.0, 2.0, 3.0, 0.5]])
    x = BS.row_scores(logits, 4, [[0]], 1, eos=3, min_length=0, ngram=0, force_eos=True)
    assert x[0, 3] == 0 and torch.isinf(x[0, :3]).all()
    y = BS.row_scores(logits, 4, [[0, 1, 0]], 3, eos=3, min_length=5, ngram=2, force_eos=False)
    ref = torch.log_softmax(logits, -1)[0]
    assert torch.isinf(y[0, 1]) and torch.isinf(y[0, 3]) and y[0, 0] == ref[0] and y[0, 2] == ref[2]   # no renormalisation


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_beam_entry_points_reject_bad_arguments_without_gpu():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert lib.vlpet_version() >= 630
    A = 4096                  # a 16-byte aligned non-NULL value: every call below returns before it could be dereferenced

    def attn(q=A, kn=None, vn=None, pos=0, D=64, Lk=56, group=1, kr=None, ldkr=56, dt=1):
        return lib.vlpet_attn_decode_beam(q, 256, A, A, 256, 56 * 256, 256, 56 * 256, kn, vn, 256, pos, None, 0, None, 0, A, 256,
                                          6, 4, D, Lk, 0.125, group, kr, ldkr, dt, None)
    assert attn(q=None) == -5 and attn(kn=A) == -5
    assert attn(dt=5) == -6
    assert attn(group=0) == -1 and attn(D=32) == -1 and attn(Lk=2000) == -1
    assert attn(kn=A, vn=A, pos=3, group=3) == -1                                      # append needs one batch per row
    assert attn(kn=A, vn=A, pos=9, kr=A, ldkr=8) == -1                                 # key-row table shorter than pos + 1
    assert attn(q=A + 8) == -3 and attn(kr=A + 2) == -3

    def rows(lg=A, ids=A, V=500, ld=504, pos=0, ldi=20, K=4, S=1, eos=2, ngram=0, st=A, dt=1):
        return lib.vlpet_beam_rows(lg, ld, V, ids, ldi, pos, 8, K, S, eos, 0, ngram, 0, st, A, A, dt, None)
    assert rows(lg=None) == -5 and rows(st=None) == -5
    assert rows(dt=2) == -6
    assert rows(K=1) == -1 and rows(K=9) == -1 and rows(S=0) == -1 and rows(S=65) == -1
    assert rows(eos=-1) == -1 and rows(eos=500) == -1 and rows(ld=496) == -1 and rows(V=70000, ld=70000) == -1
    assert rows(pos=20) == -1 and rows(ngram=-1) == -1
    assert rows(lg=A + 4) == -3 and rows(ld=508) == -3 and rows(ids=A + 4) == -3 and rows(st=A + 4) == -3

    def adv(stats=A, ids_in=A, kri=None, kro=None, ldkr=20, K=4, S=1, V=500, pos=0, ldi=20, ldh=20, eos=2, ctr=A):
        return lib.vlpet_beam_advance(stats, A, A, S, V, 3, K, A, ids_in, A, ldi, kri, kro, ldkr, A, A, A, A, ldh, A, A, ctr, pos,
                                      eos, 1, 1.0, 0, None)
    assert adv(stats=None) == -5 and adv(ctr=None) == -5 and adv(kri=A) == -5
    assert adv(K=1) == -1 and adv(K=9) == -1 and adv(S=0) == -1 and adv(eos=500) == -1
    assert adv(pos=19) == -1 and adv(ldh=0) == -1 and adv(kri=A, kro=A, ldkr=1) == -1
    assert adv(ids_in=A + 4) == -3 and adv(ctr=A + 2) == -3 and adv(kri=A + 2, kro=A) == -3


# ---- generate() on the CPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BEAM_FIXTURES)
def test_generate_matches_reference_beam_search_cpu(name):
    from oracle.host_patch import cpu_reference_ops
    g = load_beam(name)
    model = build_beam_host(g)
    with cpu_reference_ops():
        out, scores = run_beam(model, g, "cpu")
    check_against_fixture(out, scores, g)
    assert model.training


def test_generate_without_num_beams_is_the_greedy_path():
    from oracle.host_patch import cpu_reference_ops
    import vlpet_amd.decode as D
    g = load_beam(BEAM_FIXTURES[0])
    model = build_beam_host(g)
    called = []
    bg = D.beam_generate
    D.beam_generate = lambda *a, **k: called.append(1) or bg(*a, **k)
    try:
        with cpu_reference_ops():
            a = model.generate(g["ids"], g["vis"], g["task"], max_length=g["max_length"], eos_token_id=g["eos"])
            b = model.generate(g["ids"], g["vis"], g["task"], max_length=g["max_length"], eos_token_id=g["eos"], num_beams=1)
    finally:
        D.beam_generate = bg
    assert not called and torch.equal(a, b)
