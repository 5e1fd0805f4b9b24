"""The autograd glue of K1, K2, K3 and the low-rank projector without a GPU: which C entry points a forward + backward calls, in which
order, with which ``phases`` word, which optional pointers NULL and which gradient slot in which of the eight gradient arguments, and
which timer names are recorded -- against literal tables.

A recording stand-in replaces the library (``_lib.load``): every ``vlpet_*`` call records its name and arguments and returns 0, size
queries return small multiples of 256, the shape queries return what the case sets.  ``functional._stream`` / ``_need_cuda`` are
patched, packs are ``PackedPair`` / ``LowRankPack`` objects over CPU buffers, and the public functions ``adapter_gate``,
``parallel_adapter``, ``lora_delta`` and ``lowrank_project`` run forward and backward on CPU tensors through real autograd.

The expected tables (``tests/golden/adapter_call_trace.json``: they are data, 2,592 K1 rows) were produced once by this same harness
(``python tests/test_adapter_call_trace.py --generate``) on the commit BEFORE the glue was folded (K1's ``phase()`` closure and its
five-way ladder, the slot assembly written out in ``functional`` and in ``lowrank``), which is why the harness uses only names that
commit had.  One normalisation, because the fold changes it by construction: a gated call with saved activations goes through
``vlpet_adapter_gate_bwd_saved_y`` with ``y`` and ``dx1_in`` possibly NULL, where the earlier glue picked ``_bwd_saved`` /
``_bwd_saved_acc`` for the same ``run_bwd`` call (csrc/api.hip: ``k1_bwd``); the harness writes all three in the ``_saved_y`` form.

The side-stream branch needs a real stream (tests/test_gpu_graph.py and tests/test_gpu_dp.py run it on the GPU): its rows are
transcribed from the earlier ladder's text and asserted on the pure function ``functional.k1_bwd_schedule`` only, which has its own
literal table over all of its inputs below."""
import itertools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "adapter_call_trace.json")

SIZES = {"vlpet_saved_bytes": 256, "vlpet_bwd_workspace_bytes": 512, "vlpet_lora_saved_bytes": 768,
         "vlpet_lowrank_bwd_workspace_bytes": 1024, "vlpet_lowrank_packed_bytes": 256, "vlpet_packed_bytes": 256,
         "vlpet_sublayer_tail_partials": 2}
QUERIES = ("vlpet_adapter_gate_bwd_form", "vlpet_adapter_gate_bwd_finalize_launch", "vlpet_lora_r8_applies")
STREAM = 4096        # what the patched functional._stream returns


class FakeLib:
    def __init__(self, answers, signatures):
        self.answers, self.signatures = answers, signatures
        self.calls, self.queries = [], []
        self.known = {STREAM: "stream"}       # address -> label
        self.in_forward = True

    def label(self, v):
        if v is None or v == 0:
            return "NULL"
        if v in self.known:
            return self.known[v]
        if self.in_forward:         # (alive until the backward: the output, the saved block, a mask)
            self.known[v] = f"f{sum(1 for k in self.known.values() if k[0] == 'f' and k[1:].isdigit())}"
            return self.known[v]
        return "ptr"

    def __getattr__(self, name):
        if not name.startswith("vlpet_"):
            raise AttributeError(name)

        def call(*args):
            if name in SIZES:
                return SIZES[name]
            if name == "vlpet_rank_tiles":
                return 1 if args[0] <= 32 else 3 if args[0] <= 96 else 6
            if name in QUERIES:
                self.queries.append(name)
                return self.answers[name]
            import ctypes
            types = self.signatures[name][1]
            assert len(types) == len(args), (name, len(types), len(args))
            row = [self.label(a) if t is ctypes.c_void_p else (round(a, 6) if isinstance(a, float) else a) for a, t in zip(args, types)]
            self.calls.append([name] + row)
            return 0
        return call


class Sink:
    """train.GradSink's three members, over a CPU buffer."""

    def __init__(self, shape, label, log):
        self.view, self.label, self.log = torch.zeros(*shape), label, log

    def take(self):
        return self.view

    def done(self):
        self.log.append(self.label)


class Harness:
    def __init__(self, monkeypatch, answers=None, timer=None):
        from vlpet_amd import _lib, functional as Fn, lowrank
        self.Fn, self.lowrank = Fn, lowrank
        self.lib = FakeLib(dict(answers or {}), _lib.SIGNATURES)
        self.codes, self.keep, self.done = {}, [], []
        monkeypatch.setattr(_lib, "load", lambda: self.lib)
        for mod in (Fn, lowrank):
            monkeypatch.setattr(mod, "_stream", lambda: STREAM, raising=False)
            monkeypatch.setattr(mod, "_need_cuda", lambda *ts: None, raising=False)
        orig = Fn.grad_slot

        def grad_slot(p, shape, block=False):
            s = orig(p, shape, block=block)
            code = self.codes[id(p)]
            if s.sunk:
                self.lib.known[s.ptr] = f"s{code}"
            else:
                s.t.fill_(code)
                self.lib.known[s.ptr] = f"g{code}"
                self.keep.append(s.t)
            return s
        for mod in (Fn, lowrank):
            monkeypatch.setattr(mod, "grad_slot", grad_slot, raising=False)

        class Timer(Fn.KernelTimer):
            def bracket(self, name, rows, fn):
                self.records.append(name)
                return fn()
        self.timer = None if timer is None else Timer(None if timer == "all" else timer)
        monkeypatch.setattr(Fn, "TIMER", self.timer)

    def name(self, t, label):
        self.lib.known[t.data_ptr()] = label
        self.keep.append(t)
        return t

    def params(self, ps, sunk=False, n_heads=1):
        for i, p in enumerate(ps):
            if p is None:
                continue
            self.codes[id(p)] = i + 1
            if sunk:
                p._vlpet_sink = Sink(p.shape, f"s{i + 1}", self.done)
        if sunk and n_heads:       # the sinks that span the stacked heads hang on the first head's weight / bias
            ps[0]._vlpet_block_sink = Sink((n_heads * ps[0].shape[0], ps[0].shape[1]), "s1", self.done)
            ps[n_heads]._vlpet_block_sink = Sink((n_heads * ps[n_heads].shape[0],), f"s{n_heads + 1}", self.done)

    def grads(self, ps):
        out = []
        for p in ps:
            if p is None or p.grad is None:
                out.append(None)
            else:
                v = int(p.grad.reshape(-1)[0])
                assert bool((p.grad == v).all())
                out.append(v)
        return out

    def result(self, **extra):
        calls = [normalise(c) for c in self.lib.calls]
        return dict(calls=calls, queries=self.lib.queries, timer=[] if self.timer is None else list(self.timer.records),
                    done=self.done, **extra)


def normalise(call):
    """``_bwd_saved`` (gated) / ``_bwd_saved_acc`` in the ``_bwd_saved_y`` form (see the module docstring)."""
    name, a = call[0], call[1:]
    if name == "vlpet_adapter_gate_bwd_saved" and a[-6] != 0:   # (gate_mode)  phases dy x1 x2 | saved pk_a pk_g | dx1 ...
        return ["vlpet_adapter_gate_bwd_saved_y"] + a[:4] + ["NULL"] + a[4:7] + ["NULL"] + a[7:]
    if name == "vlpet_adapter_gate_bwd_saved_acc":              # phases dy x1 x2 | saved pk_a pk_g dx1_in | dx1 ...
        return ["vlpet_adapter_gate_bwd_saved_y"] + a[:4] + ["NULL"] + a[4:]
    return call


D, NH, RH, RG, SHAPE = 64, 2, 4, 8, (2, 3)
TIMERS = (None, "all", ("k1_bwd_rows",))


def leaf(*shape):
    return torch.zeros(*shape, requires_grad=True)


def k1_cases():
    # gate mode, SAVE_ACTIVATIONS, K1_BWD_FROM_OUTPUT, link (0 none, 1 the tail parks d/dx1 for this op, 2 out_link armed upstream),
    # K1_BWD_PREVIOUS_SPLIT, K1_BWD_FINALIZE_LAUNCH, timer, form answer, finalize-launch answer
    return list(itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1)))


def run_k1(monkeypatch, case, sunk=False):
    gate_mode, save, from_out, link_mode, prev, fin_switch, timer, form, fin = case
    h = Harness(monkeypatch, {QUERIES[0]: form, QUERIES[1]: fin}, TIMERS[timer])
    Fn = h.Fn
    for k, v in dict(SAVE_ACTIVATIONS=bool(save), K1_BWD_FROM_OUTPUT=bool(from_out), K1_BWD_PREVIOUS_SPLIT=bool(prev),
                     K1_BWD_FINALIZE_LAUNCH=bool(fin_switch), WGRAD_STREAM=None).items():
        monkeypatch.setattr(Fn, k, v)
    x1, x2 = h.name(leaf(*SHAPE, D), "x1"), h.name(leaf(*SHAPE, D), "x2")
    r = NH * RH
    dw, db = [leaf(RH, D) for _ in range(NH)], [leaf(RH) for _ in range(NH)]
    ps = dw + db + [leaf(D, r), leaf(D)]
    gp = None
    if gate_mode:
        gp = [leaf(RG, D), leaf(RG), leaf(D, RG), leaf(D)]
        ps += gp
    h.params(ps, sunk, NH)
    pk_a = Fn.PackedPair(h.name(torch.zeros(256, dtype=torch.uint8), "pk_a"), 1, r, D, 0)
    pk_g = Fn.PackedPair(h.name(torch.zeros(256, dtype=torch.uint8), "pk_g"), 1, RG, D, 0) if gate_mode else None
    link = Fn.ResidualLink() if link_mode == 1 else None
    out_link = Fn.ResidualLink().arm() if link_mode == 2 else None
    out = Fn.adapter_gate(x1, x2, dw, db, ps[2 * NH], ps[2 * NH + 1], gp, pk_a, pk_g, gate_mode=gate_mode, delta_scale=0.5, x2_scale=0.25,
                          gate_scale=2.0, link=link, out_link=out_link)
    h.lib.in_forward = False
    armed = bool(link is not None and link.armed)
    if armed:
        link.park(h.name(torch.zeros(*SHAPE, D), "dx1_in"))
    out.backward(h.name(torch.zeros(*SHAPE, D), "dy"))
    return h.result(grads=h.grads(ps), x1_grad=x1.grad is not None, x2_grad=x2.grad is not None, armed=armed,
                    parked=bool(out_link is not None and out_link.holds))


def k2_cases():     # SAVE_ACTIVATIONS, bu None, link armed by the projection upstream, timer
    return list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1)))


def run_k2(monkeypatch, case, sunk=False):
    save, no_bu, linked, timer = case
    h = Harness(monkeypatch, {}, TIMERS[timer])
    Fn = h.Fn
    monkeypatch.setattr(Fn, "SAVE_ACTIVATIONS", bool(save))
    x, y = h.name(leaf(*SHAPE, D), "x"), h.name(leaf(*SHAPE, D), "y")
    ps = [leaf(RG, D), leaf(RG), leaf(D, RG), None if no_bu else leaf(D)]
    h.params(ps, sunk, 0)
    pk = Fn.PackedPair(h.name(torch.zeros(256, dtype=torch.uint8), "pk"), 1, RG, D, 0)
    link = Fn.ResidualLink().arm() if linked else None
    out = Fn.parallel_adapter(x, y, *ps, pk, scale=0.5, link=link)
    h.lib.in_forward = False
    out.backward(h.name(torch.zeros(*SHAPE, D), "dy"))
    return h.result(grads=h.grads(ps), x_grad=x.grad is not None, y_grad=y.grad is not None, parked=bool(link is not None and link.holds))


def k3_cases():     # rank-8 route applies, SAVE_ACTIVATIONS, dropout (0 none, 1 generator, 2 explicit mask), return_mask, link, timer
    return list(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1)))


def run_k3(monkeypatch, case, sunk=False):
    r8, save, drop, want_mask, linked, timer = case
    h = Harness(monkeypatch, {QUERIES[2]: r8}, TIMERS[timer])
    Fn = h.Fn
    monkeypatch.setattr(Fn, "SAVE_ACTIVATIONS", bool(save))
    monkeypatch.setattr(Fn, "LORA_R8_STREAMING", True)
    x, base = h.name(leaf(*SHAPE, D), "x"), h.name(leaf(*SHAPE, D), "base")
    ps = [leaf(RG, D), leaf(D, RG)]
    h.params(ps, sunk, 0)
    pk = Fn.PackedPair(h.name(torch.zeros(256, dtype=torch.uint8), "pk"), 1, RG, D, 0)
    keep = h.name(torch.ones(*SHAPE, D, dtype=torch.uint8), "keep") if drop == 2 else None
    link = Fn.ResidualLink().arm() if linked else None
    out = Fn.lora_delta(x, base, ps[0], ps[1], pk, 2.0, keep=keep, p=0.1 if drop else 0.0, seed=11, return_mask=bool(want_mask), link=link)
    if want_mask:
        out = out[0]
    h.lib.in_forward = False
    out.backward(h.name(torch.zeros(*SHAPE, D), "dy"))
    return h.result(grads=h.grads(ps), x_grad=x.grad is not None, base_grad=base.grad is not None,
                    parked=bool(link is not None and link.holds))


def proj_cases():   # gated, gate_residual, timer
    return list(itertools.product((0, 1), (0, 1), (0, 1)))


def run_proj(monkeypatch, case, sunk=False):
    gated, gate_residual, timer = case
    h = Harness(monkeypatch, {}, TIMERS[timer])
    lowrank = h.lowrank
    F_ = 128
    lin = torch.nn.Linear
    down, up, norm = [lin(F_, RH) for _ in range(NH)], lin(NH * RH, D), torch.nn.LayerNorm(D)
    gd, gu = (lin(F_, RG), lin(RG, D)) if gated else (None, None)
    ps = [m.weight for m in down] + [m.bias for m in down] + [up.weight, up.bias]
    if gated:
        ps += [gd.weight, gd.bias, gu.weight, gu.bias]
    h.params(ps, sunk, NH)

    class Cache:
        def __init__(self, label, r):
            self.label, self.r = label, r

        def get(self, dw, db, uw, ub, io, tiles):
            return lowrank.LowRankPack(h.name(torch.zeros(256, dtype=torch.uint8), self.label), tiles, self.r, F_, D, io)
    feats, R = h.name(torch.zeros(*SHAPE, F_), "feats"), h.name(leaf(*SHAPE, D), "R")
    out = lowrank.lowrank_project(feats, R, down, up, norm, gd, gu, bool(gate_residual), Cache("pk_a", NH * RH), Cache("pk_g", RG))
    h.lib.in_forward = False
    out.backward(h.name(torch.zeros(*SHAPE, D), "dy"))
    return h.result(grads=h.grads(ps), norm_grads=[norm.weight.grad is not None, norm.bias.grad is not None], R_grad=R.grad is not None)


# gradient sinks on every parameter (train.GradSink: the kernels write into the trainer's flat buffer, autograd gets None)
SUNK = {"k1": [(1, 1, 1, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0, 0, 0, 0), (2, 0, 1, 2, 1, 0, 1, 0, 0)], "k2": [(1, 0, 1, 0), (0, 1, 0, 1)],
        "k3": [(0, 1, 1, 0, 1, 0), (1, 0, 0, 0, 0, 1)], "proj": [(1, 0, 0), (0, 1, 1)]}
OPS = {"k1": (k1_cases, run_k1), "k2": (k2_cases, run_k2), "k3": (k3_cases, run_k3), "proj": (proj_cases, run_proj)}


def trace_all(monkeypatch_factory):
    """{op: rows in case order}, {op + "_sunk": rows}; each row an index into the list of distinct results."""
    distinct, table = [], {}
    for op, (cases, run) in OPS.items():
        for key, todo, sunk in ((op, cases(), False), (op + "_sunk", SUNK[op], True)):
            rows = []
            for case in todo:
                with monkeypatch_factory() as mp:
                    res = json.loads(json.dumps(run(mp, case, sunk)))
                if res not in distinct:
                    distinct.append(res)
                rows.append(distinct.index(res))
            table[key] = rows
    return dict(distinct=distinct, table=table)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("op", ["k1", "k2", "k3", "proj"])
@pytest.mark.parametrize("sunk", [False, True], ids=["fresh", "sunk"])
def test_call_trace(op, sunk, golden):
    cases, run = OPS[op]
    todo = SUNK[op] if sunk else cases()
    want = golden["table"][op + ("_sunk" if sunk else "")]
    assert len(want) == len(todo)
    for case, idx in zip(todo, want):
        with pytest.MonkeyPatch.context() as mp:
            got = json.loads(json.dumps(run(mp, case, sunk)))
        assert got == golden["distinct"][idx], (op, case)


def test_the_traces_tell_the_cases_apart(golden):
    """The table is not vacuous: the entry points, phase words and timer names the issue names all occur in it."""
    names = {c[0] for res in golden["distinct"] for c in res["calls"]}
    for n in ("vlpet_adapter_gate_fwd", "vlpet_adapter_gate_fwd_save", "vlpet_adapter_gate_bwd_phase", "vlpet_adapter_gate_bwd_saved",
              "vlpet_adapter_gate_bwd_saved_y", "vlpet_parallel_adapter_bwd", "vlpet_parallel_adapter_bwd_saved", "vlpet_lora_delta_fwd_r8",
              "vlpet_lora_delta_fwd_save", "vlpet_lora_delta_bwd_saved", "vlpet_lowrank_gate_bwd"):
        assert n in names, n
    phases = {c[1] for res in golden["distinct"] for c in res["calls"] if "gate_bwd_" in c[0] and "lowrank" not in c[0]}
    assert phases == {3, 35, 5, 6, 37, 38, 1, 33, 2, 34, 10, 42, 16, 48}
    timers = {tuple(res["timer"]) for res in golden["distinct"]}
    assert ("k1_fwd", "k1_bwd_rows", "k1_bwd_wgrad", "k1_bwd_fin") in timers and ("k1_bwd_rows", "k1_bwd_wgrad", "k1_bwd_fin") in timers
    assert ("k1_bwd_rows",) in timers and ("k1_fwd", "k1_bwd_rows") in timers


# ---- the K1 backward schedule as a pure function: (gate, saved, side, previous_split, bracketed, form, finalize_due) -> steps.
# Transcribed from the ladder in the earlier _AdapterGateFn.backward: precedence side stream > previous split > not bracketed > bracketed.
R_, W_, F_ = "k1_bwd_rows", "k1_bwd_wgrad", "k1_bwd_fin"
SCHEDULES = {
    "side": [(R_, 1 | 4, False), (W_, 2 | 4, True)],
    "prev": [(R_, 1 | 4, False), (W_, 2 | 4, False)],
    "plain": [(None, 3, False)],
    "whole": [(R_, 3, False)],                                          # bracketed, no gate: one call
    "rows+wgrad": [(R_, 1, False), (W_, 2, False)],                     # bracketed, gate, not the two-pass form
    "two-pass": [(R_, 1, False), (W_, 2 | 8, False), (F_, 16, False)],  # form 2 (saved activations only), finalize launch due
    "in-launch": [(R_, 1, False), (W_, 2 | 8, False)],                  # form 2, pass 2 reduces in the launch
}


def schedule_expected(gate, saved, side, prev, bracketed, form, fin):
    if side:
        return "side"
    if prev:
        return "prev"
    if not bracketed:
        return "plain"
    if not gate:
        return "whole"
    if not (saved and form == 2):
        return "rows+wgrad"
    return "two-pass" if fin else "in-launch"


# one letter per row of itertools.product(gate, saved, side, prev, bracketed, form 0/1/2, finalize_due): s side, p prev, . plain,
# w whole, r rows+wgrad, t two-pass, i in-launch
PURE = ("......wwwwwwpppppppppppp" "ssssssssssssssssssssssss" "......wwwwwwpppppppppppp" "ssssssssssssssssssssssss"
        "......rrrrrrpppppppppppp" "ssssssssssssssssssssssss" "......rrrritpppppppppppp" "ssssssssssssssssssssssss")
LETTER = {"s": "side", "p": "prev", ".": "plain", "w": "whole", "r": "rows+wgrad", "t": "two-pass", "i": "in-launch"}


def test_k1_bwd_schedule_table():
    from vlpet_amd.functional import k1_bwd_schedule
    rows = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)))
    assert len(rows) == len(PURE) == 192
    for row, letter in zip(rows, PURE):
        assert schedule_expected(*row) == LETTER[letter], row        # (the table and the transcription say the same)
        got = k1_bwd_schedule(*(bool(v) for v in row[:5]), row[5], bool(row[6]))
        assert [tuple(s) for s in got] == SCHEDULES[LETTER[letter]], row


if __name__ == "__main__" and "--generate" in sys.argv:
    sys.path.insert(0, os.path.dirname(HERE))
    out = trace_all(pytest.MonkeyPatch.context)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({k: len(v) for k, v in out["table"].items()}, len(out["distinct"]), "distinct results")
