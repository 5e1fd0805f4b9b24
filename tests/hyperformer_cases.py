"""Shared by tests/test_hyperformer_modules.py, tests/test_hyper_spec.py and tests/test_gpu_hyperformer_modules.py: the controller
fixtures of tests/golden/make_hyperformer_goldens.py (the reference's AdapterLayersHyperNetController / AdapterLayersOneHyperNetController
alone: parameters, a task embedding, every layer's outputs, upstream gradients, every gradient) and the package's controllers loaded
from them."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORMS = ("unique", "one")
BLOCKS = ("self_attention", "feed_forward", "cross_attention")
PARTS = (("down", "weight", "down_w"), ("down", "bias", "down_b"), ("up", "weight", "up_w"), ("up", "bias", "up_b"))
TASKS = ["vqa", "gqa", "nlvr", "caption"]


@functools.lru_cache(maxsize=None)
def fixture(form):
    z = np.load(os.path.join(GOLDEN, f"hyper_ctl_{form}_d64_r8_p8.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def config(**over):
    from vlpet_amd.adapters import MetaAdapterConfig
    kw = dict(input_dim=64, d_model=64, reduction_factor=8, projected_task_embedding_dim=8, task_embedding_dim=64, tasks=list(TASKS))
    kw.update(over)
    return MetaAdapterConfig(**kw)


def controller(form, device="cpu", dtype=torch.float32, **over):
    """the package's controller of ``form`` with the fixture's parameters, and the fixture's task embedding as a leaf"""
    from vlpet_amd.adapters import AdapterLayersHyperNetController, AdapterLayersOneHyperNetController
    z = fixture(form)
    cls = AdapterLayersHyperNetController if form == "unique" else AdapterLayersOneHyperNetController
    ctl = cls(config(**over), int(z["layers"]), True)
    ctl.load_state_dict({k[3:]: torch.tensor(v) for k, v in z.items() if k.startswith("p::")})
    ctl = ctl.to(device=device, dtype=dtype)
    te = torch.tensor(z["task_embedding"]).to(device=device, dtype=dtype).requires_grad_(True)
    return ctl, te


def each_output(weights):
    """(fixture key suffix, tensor) of every generated tensor of ``weights`` (a controller's ``generate()`` result)"""
    for layer, per in enumerate(weights):
        for block in BLOCKS:
            for side, what, attr in PARTS:
                yield f"{layer}::{block}::{side}::{what}", getattr(per[block], attr)


def fixture_loss(form, weights):
    """sum(out * dout) over every output, as the fixture's gradients were made"""
    z = fixture(form)
    loss = 0
    for key, t in each_output(weights):
        loss = loss + (t.float() * torch.tensor(z["dout::" + key]).to(t.device)).sum()
    return loss


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
