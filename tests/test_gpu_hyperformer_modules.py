"""Hyperformer's controllers on the GPU (adapters/adapter_hypernetwork.py on csrc/hyper.hip): the reference's fixtures through the
kernel path, one generator launch per ``generate()``, a train step through generator + packs + K2 that reaches every parameter and
equals the plain-torch composition, bf16 parameters under the specification's budget, and the no_grad cache: hits launch nothing, every
task has buffers of its own, a parameter change is followed in place -- also by an already captured graph."""
import numpy as np
import pytest
import torch

import hyper_spec as S
import hyperformer_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_OUT = 1e-5      # fp32 generators: 9 terms of magnitude <= the result's scale (tests/hyper_spec.py: 9 * 2^-24 = 5e-7)
TOL_GRAD = 2e-4     # de sums 3,288 terms per element in fp32: N * 2^-24 = 2e-4 of the terms' magnitudes at worst; the MLP's gradients inherit it


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("form", C.FORMS)
def test_fixtures_through_the_kernel_path(form):
    import vlpet_amd.functional as VF
    z = C.fixture(form)
    ctl, te = C.controller(form, DEV)
    n0 = VF.HYPER_CALLS
    weights = ctl.generate(te, io_dtype=VF._io_dtype(torch.empty(1, device=DEV)))
    assert VF.HYPER_CALLS == n0 + 1                                # one launch for all layers, blocks and generators
    assert all(per[b].pack is not None and per[b].pack.r == 8 and per[b].pack.d == 64 for per in weights for b in C.BLOCKS)
    for key, t in C.each_output(weights):
        assert C.rel(_f64(t), z["out::" + key]) <= TOL_OUT, key
    C.fixture_loss(form, weights).backward()
    torch.cuda.synchronize()
    for n, p in ctl.named_parameters():
        assert C.rel(_f64(p.grad), z["d::" + n]) <= TOL_GRAD, n
    assert C.rel(_f64(te.grad), z["d_task_embedding"]) <= TOL_GRAD


@pytest.mark.parametrize("form", C.FORMS)
def test_bf16_parameters_within_the_specs_budget(form):
    ctl, te = C.controller(form, DEV, torch.bfloat16)
    with torch.no_grad():
        e = ctl.embedding_rows(te).float()
        weights = ctl.generate(te)
    ref = S.generate([(_f64(G), _f64(g)) for G, g in ctl.maps()], _f64(e))
    assert weights[0]["self_attention"].down_w.dtype == torch.bfloat16
    for layer, per in enumerate(weights):
        for block in C.BLOCKS:
            row, base = ctl.locate(layer, block)
            for k, (_, _, attr) in enumerate(C.PARTS):
                out, mag = ref[base + k]
                err = np.abs(_f64(getattr(per[block], attr)).reshape(-1) - out[row])
                assert (err <= S.budget(mag[row], 9, out[row], bf16=True)).all(), (layer, block, attr)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", C.FORMS)
def test_train_step_reaches_every_parameter_and_matches_the_eager_composition(form, dtype):
    """every adapter of every layer applied by K2 to its own activations (M = 40 rows); tolerances: K2's in tests/test_gpu_kernels.py
    (1e-3 fp32 IO, 1e-2 bf16 IO; gpu_cases.rel_err)"""
    import vlpet_amd.functional as VF
    from vlpet_amd.adapters import MetaLayersAdapterController
    from gpu_cases import rel_err
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    g = torch.Generator().manual_seed(3)
    keys = [(layer, b) for layer in range(2) for b in C.BLOCKS]
    xs = {k: torch.randn(40, 64, generator=g).to(dtype) for k in keys}
    dys = {k: torch.randn(40, 64, generator=g).to(dtype) for k in keys}
    meta = MetaLayersAdapterController(C.config())

    ref_ctl, ref_te = C.controller(form, "cpu", torch.float64)
    ref_x = {k: v.double().requires_grad_(True) for k, v in xs.items()}
    ref_w = ref_ctl.generate(ref_te)
    ref_out = {k: meta.fused(ref_x[k], ref_x[k], ref_w[k[0]][k[1]]) for k in keys}
    torch.autograd.backward([ref_out[k] for k in keys], [dys[k].double() for k in keys])

    ctl, te = C.controller(form, DEV)
    gx = {k: v.to(DEV).requires_grad_(True) for k, v in xs.items()}
    n0 = VF.HYPER_CALLS
    w = ctl.generate(te, io_dtype=VF._io_dtype(gx[keys[0]]))
    out = {k: meta.fused(gx[k], gx[k], w[k[0]][k[1]]) for k in keys}
    torch.autograd.backward([out[k] for k in keys], [dys[k].to(DEV) for k in keys])
    torch.cuda.synchronize()
    assert VF.HYPER_CALLS == n0 + 1
    errs = {"d_task_embedding": rel_err(te.grad, ref_te.grad)}
    for k in keys:
        errs[f"out{k}"], errs[f"dx{k}"] = rel_err(out[k], ref_out[k]), rel_err(gx[k].grad, ref_x[k].grad)
    for (n, p), (_, q) in zip(ctl.named_parameters(), ref_ctl.named_parameters()):
        assert p.grad is not None and bool(p.grad.abs().max() > 0), n
        errs["d::" + n] = rel_err(p.grad, q.grad)
    print(errs)
    assert max(errs.values()) <= tol, errs


@pytest.mark.parametrize("form", C.FORMS)
def test_no_grad_cache_hits_launch_nothing_and_every_task_has_its_own_buffers(form):
    import vlpet_amd.functional as VF
    from vlpet_amd.adapters import TaskEmbeddingController
    ctl, _ = C.controller(form, DEV)
    torch.manual_seed(1)
    tec = TaskEmbeddingController(C.config()).to(DEV)
    io = VF._io_dtype(torch.empty(1, device=DEV))
    ptrs, vals = {}, {}
    with torch.no_grad():
        for task in ("vqa", "gqa"):
            n0 = VF.HYPER_CALLS
            w = ctl.generate(tec(task), task=task, io_dtype=io)
            assert VF.HYPER_CALLS == n0 + 1
            ptrs[task] = [t.data_ptr() for _, t in C.each_output(w)] + [per[b].pack.buf.data_ptr() for per in w for b in C.BLOCKS]
            vals[task] = [t.clone() for _, t in C.each_output(w)]
        assert not set(ptrs["vqa"]) & set(ptrs["gqa"])
        assert max(float((a - b).abs().max()) for a, b in zip(vals["vqa"], vals["gqa"])) > 1e-3       # the tasks differ
        n0 = VF.HYPER_CALLS
        for task in ("vqa", "gqa", "vqa", "gqa"):                 # alternating tasks: hits, each task's own weights
            w = ctl.generate(tec(task), task=task, io_dtype=io)
            assert [t.data_ptr() for _, t in C.each_output(w)] + [per[b].pack.buf.data_ptr() for per in w for b in C.BLOCKS] == ptrs[task]
            assert all(torch.equal(t, v) for (_, t), v in zip(C.each_output(w), vals[task]))
        assert VF.HYPER_CALLS == n0
        # a parameter change (autograd's version counter sees it) is followed, in place
        ctl.block_nets("feed_forward")[1].weight_generator[0].bias.add_(0.5)          # (the up projection's weight generator)
        w = ctl.generate(tec("vqa"), task="vqa", io_dtype=io)
        assert VF.HYPER_CALLS == n0 + 1
        assert [t.data_ptr() for _, t in C.each_output(w)] + [per[b].pack.buf.data_ptr() for per in w for b in C.BLOCKS] == ptrs["vqa"]
        assert torch.allclose(w[1]["feed_forward"].up_w, vals["vqa"][[k for k, _ in C.each_output(w)].index("1::feed_forward::up::weight")] + 0.5)
        # a change the version counters do not see needs the epoch, as everywhere
        ctl.layer_id_embeddings.weight.data.mul_(1.5)
        VF.invalidate_caches()
        before = w[0]["self_attention"].down_w.clone()
        w = ctl.generate(tec("vqa"), task="vqa", io_dtype=io)
        assert VF.HYPER_CALLS == n0 + 2 and not torch.equal(w[0]["self_attention"].down_w, before)
        # and the result is what the plain-torch composition gives from the current parameters
        from vlpet_amd import eager
        rows = eager.hyper_generate(ctl.maps(), ctl.embedding_rows(tec("vqa")))
        for (key, t), (_, r) in zip(C.each_output(w), C.each_output(ctl._collect(rows, None))):
            assert C.rel(_f64(t), _f64(r)) <= TOL_OUT, key


@pytest.mark.parametrize("form", C.FORMS)
def test_captured_steps_of_two_tasks_follow_a_parameter_change(form):
    """one captured K2 step per task, replayed alternately: each reads its own task's weights and pack; after a parameter change and a
    ``generate()`` per task (refreshed in place, outside the graphs) the SAME graphs give the new results"""
    import vlpet_amd.functional as VF
    from vlpet_amd.adapters import MetaLayersAdapterController, TaskEmbeddingController
    ctl, _ = C.controller(form, DEV)
    meta = MetaLayersAdapterController(C.config())
    torch.manual_seed(2)
    tec = TaskEmbeddingController(C.config()).to(DEV)
    x = torch.randn(24, 64, device=DEV)
    io = VF._io_dtype(x)
    where = (1, "cross_attention")

    def eager_out(task):
        from vlpet_amd import eager
        w = ctl._collect(eager.hyper_generate(ctl.maps(), ctl.embedding_rows(tec(task))), None)
        return meta.fused(x, x, w[where[0]][where[1]])

    graphs, outs = {}, {}
    with torch.no_grad():
        for task in ("vqa", "caption"):
            w = ctl.generate(tec(task), task=task, io_dtype=io)[where[0]][where[1]]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                meta.fused(x, x, w)                              # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(side)
            graphs[task] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[task]):
                outs[task] = meta.fused(x, x, w)
        for rnd in range(2):
            for task in ("vqa", "caption", "vqa"):
                graphs[task].replay()
                torch.cuda.synchronize()
                assert float((outs[task] - eager_out(task)).abs().max()) <= 1e-3 * float(eager_out(task).abs().max()), (rnd, task)
            assert float((outs["vqa"] - outs["caption"]).abs().max()) > 1e-3
            if rnd == 0:
                old = {t: outs[t].clone() for t in outs}
                for _, g in ctl.maps():
                    g.add_(0.25)                                  # every generator's bias: every generated tensor moves
                for task in ("vqa", "caption"):
                    ctl.generate(tec(task), task=task, io_dtype=io)
        assert all(float((outs[t] - old[t]).abs().max()) > 1e-2 for t in outs)


@pytest.mark.parametrize("form", C.FORMS)
def test_captured_forward_and_backward_reproduce_the_eager_step(form):
    """generation, packs, K2 and the whole backward captured as one graph (autograd on: everything runs inside it and reads the
    parameters in place): a replay gives the eager step's gradients, and after the task embedding and a generator changed in place the
    SAME graph gives the new ones"""
    import vlpet_amd.functional as VF
    from vlpet_amd.adapters import MetaLayersAdapterController
    ctl, te = C.controller(form, DEV)
    meta = MetaLayersAdapterController(C.config())
    g = torch.Generator().manual_seed(7)
    keys = [(layer, b) for layer in range(2) for b in C.BLOCKS]
    x = {k: torch.randn(24, 64, generator=g).to(DEV) for k in keys}
    dy = {k: torch.randn(24, 64, generator=g).to(DEV) for k in keys}
    params = [te] + list(ctl.parameters())

    def step():
        w = ctl.generate(te, io_dtype=VF._io_dtype(x[keys[0]]))
        outs = [meta.fused(x[k], x[k], w[k[0]][k[1]]) for k in keys]
        return torch.autograd.grad(outs, params, [dy[k] for k in keys])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    n0 = VF.HYPER_CALLS
    with torch.cuda.graph(graph):
        static = step()
    assert VF.HYPER_CALLS == n0 + 1
    for rnd in range(2):
        n1 = VF.HYPER_CALLS
        graph.replay()
        torch.cuda.synchronize()
        assert VF.HYPER_CALLS == n1                              # a replay issues no call
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        for a, b, p in zip(got, want, ["task_embedding"] + [n for n, _ in ctl.named_parameters()]):
            assert torch.equal(a, b), (rnd, p)                   # the same kernels on the same values: the same bits
        if rnd == 0:
            first = got
            with torch.no_grad():
                te.mul_(-0.5)
                ctl.maps()[0][0].add_(0.01)
    assert max(float((a - b).abs().max()) for a, b in zip(first, got)) > 1e-3
