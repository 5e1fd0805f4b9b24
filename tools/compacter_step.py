#!/usr/bin/env python3
"""One eager train step of BART-base with the Compacter adapters of scripts/image-text/single_compacter.sh (bf16 backbone, fp32
adapters, vqa batch): step time (HIP events, median of alternating rounds) and GPU kernel launches per step (torch.profiler), for the
model on the HIP expansion (csrc/phm.hip + K2) and for the same model with every adapter on the plain-torch composition
(vl-pet_amd/eager.py), one process.  profiles/r15_compacter.md keeps the output.
usage: compacter_step.py [batch] [rounds]      (default 64 5)"""
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vlpet_amd.host.bart as HB  # noqa: E402
import vlpet_amd.train as TR  # noqa: E402
from vlpet_amd.adapters import HyperComplexAdapter  # noqa: E402
from genbench import COMPACTER  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda"
torch.manual_seed(0)
cfg = HB.vlpet_config(**COMPACTER)
base = HB.VLBart(cfg)
TR.trainable_names(base, cfg)
legs = {}
for name in ("hip", "eager"):
    m = copy.deepcopy(base).to(dev)
    TR.cast_frozen(m, torch.bfloat16)
    n_ad = 0
    for mod in m.modules():
        if isinstance(mod, HyperComplexAdapter):
            mod.eager = name == "eager"
            n_ad += 1
    legs[name] = (m.train(), TR.Trainer(m, cfg, lr=1e-4, total_steps=1000, warmup_ratio=0.1))
gen = torch.Generator(device=dev).manual_seed(1)
batch = TR.synthetic_batch("vqa", B, cfg, dev, gen)


def step_ms(tr, k=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        tr.step(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def kernels(tr):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        tr.step(batch)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset"))]
    return len(ev)


for _, tr in legs.values():
    step_ms(tr, 2)
t = {k: [] for k in legs}
for _ in range(ROUNDS):
    for k, (_, tr) in legs.items():
        t[k].append(step_ms(tr))
print(f"BART-base + Compacter (division 2, r = 96, {n_ad} adapters), vqa batch {B}, bf16 backbone, eager trainer")
print("| adapters on | step ms (median, min..max) | GPU kernels per step |")
print("|---|---|---|")
for k, (_, tr) in legs.items():
    print(f"| {'csrc/phm.hip + K2' if k == 'hip' else 'eager.phm_adapter (plain torch)'} | {statistics.median(t[k]):.2f} ({min(t[k]):.2f}..{max(t[k]):.2f}) | {kernels(tr)} |")
