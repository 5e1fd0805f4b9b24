#!/usr/bin/env python3
"""Prompt tuning's encoder-input assembly, forward + backward, three ways in ONE process, the legs timed in ALTERNATING rounds (HIP
events), bf16, p = 0.1:
  (a) act.prefix_concat_dropout (csrc/prefix_cat.hip) on the [P, d] prompt rows;
  (b) the kernels this project had before: torch.cat of the expanded prompt and the text, act.concat_dropout, and autograd's sum(0)
      of the [B, P, d] gradient slice;
  (c) the reference-shaped chain: Embedding -> Linear(d, mid) -> Tanh -> Linear(mid, d) on B * P looked-up rows, torch.cat,
      F.dropout -- with the MLP inside the timed region, because running it on B * P rows is what the chain costs; (a) and (b) run
      the same MLP on P rows, also inside the timed region.
Shapes (B, P, La, Lv, d): (500, 40, 20, 36, 768) -- scripts/image-text/single_prompt.sh, one image -- and (416, 40, 20, 72, 768), the
two-image (nlvr) batch.  Warm (``ITERS`` back-to-back calls per round) and cold (a read-modify-write over 1 GiB before every timed call,
as tools/phm_bench.py).  Also printed: the kernels alone through the C ABI (forward, backward, backward without dpre), the chunk split of the backward's batch sum, and which task shapes pass 128 encoder tokens with
P = 40 and where the attention routing sends them.  profiles/r16_prompt.md keeps the output."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
import vlpet_amd.attention as A  # noqa: E402
import vlpet_amd.host.bart as HB  # noqa: E402
import vlpet_amd.train as TR  # noqa: E402
from vlpet_amd import _lib  # noqa: E402
from vlpet_amd.act import concat_dropout, prefix_concat_dropout  # noqa: E402
from vlpet_amd.prompt import EncoderPromptConfig, InputPrompts  # noqa: E402

lib = _lib.load()
dev, dtype, p, MID = "cuda", torch.bfloat16, 0.1, 800
SHAPES = [(500, 40, 20, 36, 768), (416, 40, 20, 72, 768)]
ROUNDS, ITERS, COLD_CALLS = 9, 50, 5
evict = torch.zeros(1 << 28, dtype=torch.float32, device=dev)


def warm(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) / ITERS * 1e3]


def cold(fn):
    out = []
    for _ in range(COLD_CALLS):
        evict.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def cell(t):
    return f"{statistics.median(t):.1f} ({min(t):.1f}..{max(t):.1f})"


lines, klines = [], []
for B, P, La, Lv, d in SHAPES:
    g = torch.Generator(device=dev).manual_seed(B)
    torch.manual_seed(B)
    mod = InputPrompts(EncoderPromptConfig(prompt_len=P, input_dim=d, mid_dim=MID)).to(dev, dtype)
    params = list(mod.parameters())
    a = torch.randn(B, La, d, device=dev, generator=g).to(dtype).requires_grad_(True)
    v = torch.randn(B, Lv, d, device=dev, generator=g).to(dtype).requires_grad_(True)
    dx = torch.randn(B, P + La + Lv, d, device=dev, generator=g).to(dtype)
    ids = mod.prefix_tokens.to(dev).unsqueeze(0).expand(B, -1)

    def leg_a():
        x = prefix_concat_dropout(mod.rows(), a, v, p, True, seed=7)
        return torch.autograd.grad(x, [a, v] + params, dx)

    def leg_b():
        x = concat_dropout(torch.cat([mod.rows().expand(B, -1, -1), a], 1), v, p, True, seed=7)
        return torch.autograd.grad(x, [a, v] + params, dx)

    def leg_c():
        x = TF.dropout(torch.cat([mod.prefix_embedding(ids), a, v], 1), p, True)
        return torch.autograd.grad(x, [a, v] + params, dx)

    # (a) and (b) apply the same mask: their gradients agree up to the order of the batch sum
    ga, gb = leg_a(), leg_b()
    err = max(float((x.float() - y.float()).abs().max() / (y.float().abs().max() + 1e-12)) for x, y in zip(ga, gb))
    legs = (leg_a, leg_b, leg_c)
    for mode, timer in (("warm", warm), ("cold", cold)):
        for fn in legs:
            for _ in range(5):
                fn()
        t = [[], [], []]
        for _ in range(ROUNDS):                             # alternating rounds
            for i, fn in enumerate(legs):
                t[i] += timer(fn)
        m = [statistics.median(x) for x in t]
        lines.append(f"| {B} | {P} | {La} | {Lv} | {mode} | {cell(t[0])} | {cell(t[1])} | {cell(t[2])} | {m[0] / m[1]:.2f} | {m[0] / m[2]:.2f} | {err:.2g} |")
    # the kernels alone, through the C ABI (no MLP, no autograd): forward; backward with all three outputs; backward without dpre
    # (what the batch sum adds: its partial blocks ride in the same launch, the chunk sum is a second one)
    st = torch.cuda.current_stream().cuda_stream
    pre = mod.rows().detach().contiguous()
    x = torch.empty(B, P + La + Lv, d, device=dev, dtype=dtype)
    dpre, da, dv = torch.empty_like(pre), torch.empty_like(a), torch.empty_like(v)
    ws = torch.empty(lib.vlpet_prefix_concat_ws_bytes(B, P, d) // 4, dtype=torch.float32, device=dev)

    def k_fwd():
        assert lib.vlpet_prefix_concat_dropout_fwd(pre.data_ptr(), a.data_ptr(), v.data_ptr(), x.data_ptr(), B, P, La, Lv, d, p, 7,
                                                   _lib.VLPET_BF16, st) == 0

    def k_bwd():
        assert lib.vlpet_prefix_concat_dropout_bwd(dx.data_ptr(), dpre.data_ptr(), da.data_ptr(), dv.data_ptr(), ws.data_ptr(), B, P, La, Lv,
                                                   d, p, 7, _lib.VLPET_BF16, st) == 0

    def k_bwd_no_dpre():
        assert lib.vlpet_prefix_concat_dropout_bwd(dx.data_ptr(), None, da.data_ptr(), dv.data_ptr(), None, B, P, La, Lv, d, p, 7,
                                                   _lib.VLPET_BF16, st) == 0
    for mode, timer in (("warm", warm), ("cold", cold)):
        t = [[], [], []]
        for _ in range(ROUNDS):
            for i, fn in enumerate((k_fwd, k_bwd, k_bwd_no_dpre)):
                t[i] += timer(fn)
        klines.append(f"| {B} | {P} | {La} | {Lv} | {mode} | {cell(t[0])} | {cell(t[1])} | {cell(t[2])} |")
    nc = lib.vlpet_prefix_concat_chunks(B)
    print(f"B = {B}: batch sum of dpre in {nc} chunks of {(B + nc - 1) // nc} items, workspace {lib.vlpet_prefix_concat_ws_bytes(B, P, d) / 1e6:.2f} MB "
          f"(two launches: partials, then the chunks added in order)")

print(f"\nforward + backward, bf16, d = 768, mid_dim = {MID}, p = {p}; us per call: median (min..max) over {ROUNDS} alternating rounds")
print("| B | P | La | Lv | calls | (a) prefix_concat_dropout | (b) cat + concat_dropout + sum(0) | (c) reference-shaped chain | a / b | a / c | max rel. difference a vs b |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(lines), flush=True)

print("\nthe kernels alone (C ABI), bf16, p = 0.1; us per call")
print("| B | P | La | Lv | calls | forward | backward (dpre, da, dv) | backward without dpre |")
print("|---|---|---|---|---|---|---|---|")
print("\n".join(klines), flush=True)

# ---- which task shapes leave the short-attention route with P = 40
print(f"\nencoder tokens with P = 40 (short attention kernels: up to {A.MAX_LEN}; long kernels: up to {A.MAX_LONG}); route = host.bart._route "
      "with the module's default switches")
print("| task | text | visual | tokens without prompt | with P = 40 | route, training (p = 0.1) | route, eval | with LONG_ATTENTION_TRAIN / LONG_ATTENTION on |")
print("|---|---|---|---|---|---|---|---|")
VIS = {"vqa": 36, "gqa": 36, "nlvr": 72, "caption": 36, "tvqa": 64, "how2qa": 64, "tvc": 64, "yc2c": 64}
for task, nv in VIS.items():
    L = TR.TEXT_LEN[task]
    n0, n1 = L + nv, L + nv + 40
    tr_ = HB._route(n1, n1, 0.1, True, grad=True)
    ev = HB._route(n1, n1, 0.1, False)
    on = [A.route(n1, n1, 0.1, t, t, eager=False, long_on=True, long_train_on=True) or "library (SDPA)" for t in (True, False)]
    print(f"| {task} | {L} | {nv} | {n0} | {n1} | {tr_ or 'library (SDPA)'} | {ev or 'library (SDPA)'} | {on[0]} / {on[1]} |")
