"""The bracketed K1 backward through ``functional.adapter_gate`` (what bench.py's kernel timers run): the bits of the unbracketed one
and the expected timer names, at the smallest shape of each schedule of ``functional.k1_bwd_schedule`` -- the two-pass form with a
finalize launch, with the in-launch reduce (M >= 8,192), at six tiles, the fp32 form that is not two-pass, and the ungated op's one
bracket.  Each also under K1_BWD_FINALIZE_LAUNCH, and with a timer that names ``k1_bwd_rows`` only (the bracketed branch brackets
every step once that name is wanted).  tests/test_gpu_cols.py::test_kernel_brackets_and_previous_split_agree covers the same phases
at the C ABI."""
import pytest
import torch

import gpu_cases as C

pytestmark = pytest.mark.gpu
ROWS, WGRAD, FIN = "k1_bwd_rows", "k1_bwd_wgrad", "k1_bwd_fin"

CASES = {       # (dtype, M, d, r = r_g, gate mode) -> names by default, names under K1_BWD_FINALIZE_LAUNCH
    "two-pass": ((torch.bfloat16, 96, 128, 8, 1), [ROWS, WGRAD, FIN], [ROWS, WGRAD, FIN]),
    "in-launch": ((torch.bfloat16, 8224, 128, 8, 1), [ROWS, WGRAD], [ROWS, WGRAD, FIN]),
    "six-tiles": ((torch.bfloat16, 96, 128, 104, 1), [ROWS, WGRAD, FIN], [ROWS, WGRAD, FIN]),
    "fp32": ((torch.float32, 96, 64, 8, 1), [ROWS, WGRAD], [ROWS, WGRAD]),
    "no-gate": ((torch.bfloat16, 96, 128, 8, 0), [ROWS], [ROWS]),
}


@pytest.mark.parametrize("finalize_switch", [False, True], ids=["default", "finalize-launch"])
@pytest.mark.parametrize("case", list(CASES))
def test_bracketed_backward_is_the_unbracketed_one(case, finalize_switch):
    import vlpet_amd.functional as F
    (dtype, M, d, r, gate_mode), *names = CASES[case]
    want = names[int(finalize_switch)]
    nh, dev = 2, "cuda"
    t = C.make_k1(5, M, d, r, r, nh)
    gate = gate_mode != 0
    keys = ["wd", "bd", "wu", "bu"] + (["wgd", "bgd", "wgu", "bgu"] if gate else [])

    def run(timer):
        x1, x2 = (t[k].to(dtype).to(dev).requires_grad_(True) for k in ("x1", "x2"))
        P = {k: t[k].to(dev).requires_grad_(True) for k in keys}
        rh = r // nh
        dws = [P["wd"][i * rh:(i + 1) * rh].detach().clone().requires_grad_(True) for i in range(nh)]
        dbs = [P["bd"][i * rh:(i + 1) * rh].detach().clone().requires_grad_(True) for i in range(nh)]
        io, tiles = F._io_dtype(x2), F.rank_tiles(r)
        pk_a = F.pack_pair(dws, dbs, P["wu"], P["bu"], io, tiles)
        pk_g = F.pack_pair([P["wgd"]], [P["bgd"]], P["wgu"], P["bgu"], io, tiles) if gate else None
        gp = tuple(P[k] for k in keys[4:]) if gate else None
        F.TIMER = timer
        y = F.adapter_gate(x1, x2, dws, dbs, P["wu"], P["bu"], gp, pk_a, pk_g, gate_mode, 1.0, 1.0, 0.7)
        y.backward(t["dy"].to(dtype).to(dev))
        torch.cuda.synchronize()
        grads = [x2.grad] + ([x1.grad] if gate else []) + [w.grad for w in dws] + [b.grad for b in dbs] + [P[k].grad for k in keys[2:]]
        assert all(g is not None and torch.isfinite(g).all() for g in grads)
        return grads

    saved = F.TIMER, F.K1_BWD_FINALIZE_LAUNCH
    try:
        F.K1_BWD_FINALIZE_LAUNCH = finalize_switch
        ref = run(None)
        for timer, recorded in ((F.KernelTimer(), ["k1_fwd"] + want), (F.KernelTimer(names={ROWS}), want)):
            got = run(timer)
            assert [rec[0] for rec in timer.records] == recorded
            assert all(rec[1] == M for rec in timer.records)
            assert len(got) == len(ref) == (2 if gate else 1) + 2 * nh + (6 if gate else 2)
            for a, b in zip(got, ref):
                assert torch.equal(a, b)
    finally:
        F.TIMER, F.K1_BWD_FINALIZE_LAUNCH = saved
