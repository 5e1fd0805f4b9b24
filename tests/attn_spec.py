"""Host statement of the short attention kernels (csrc/attn.hip): the eager chain of tests/test_gpu_attn_long_train.py::_eager with its
backward written out by hand, in two forms, plus the edge cases that tests/test_attn_spec.py (CPU) and
tests/test_gpu_attention_edges.py (GPU) share.  torch on the CPU only; nothing here runs a kernel.

``chain(..., dtype=torch.float64, rounded=False)`` is the reference.  ``chain(..., dtype=torch.float32, rounded=True)`` is the kernels'
documented arithmetic (the comments of csrc/attn.hip) and nothing else: the probabilities after dropout go into the second product as
bf16 (``acc_frag``), the output is stored as bf16, the backward takes ``delta = rowsum(dO * O)`` from that STORED output in fp32,
dS = P (keep dP / (1 - p) - delta) scale goes into both of its products as bf16, and dq, dk, dv are stored as bf16.  What it does not
restate: the order of the sums, exp2 against the saved log-sum-exp, and the hardware's exp2.

A row with no visible key (padding, the causal bound with Lq > Lk, a bias row of -inf) gives zeros and no gradient."""
from collections import namedtuple

import torch

TILE = 32             # rows of a work unit: a query block (out, dq) or a key tile (dk, dv)
TOL = 2e-2            # the project's tensor-wide bound
FLOOR = 2e-2 * 1e-2   # its absolute floor for a gradient whose reference is (nearly) zero


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def heads_first(t, heads):
    """[B, L, heads * 64] -> [B, heads, L, 64]"""
    B, L, _ = t.shape
    return t.reshape(B, L, heads, 64).transpose(1, 2)


def scores(q, k, key_mask, causal, bias, scale, heads, dtype):
    """scale q k^T + bias with -inf wherever a key is not visible: [B, heads, Lq, Lk]"""
    Lq, Lk = q.shape[1], k.shape[1]
    s = (heads_first(q.to(dtype), heads) @ heads_first(k.to(dtype), heads).transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(dtype)[None]
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :].bool(), float("-inf"))
    if causal:
        i = torch.arange(Lq)[:, None]; j = torch.arange(Lk)[None, :]
        s = s.masked_fill(j > i + (Lk - Lq), float("-inf"))
    return s


def dead_rows(q, k, key_mask, causal, bias, heads):
    """[B, heads, Lq] bool: the rows with no visible key (a property of the masks and of the bias's -inf entries, not of q and k)"""
    z = torch.zeros_like(q, dtype=torch.float32)
    return torch.isinf(scores(z, torch.zeros_like(k, dtype=torch.float32), key_mask, causal, bias, 1.0, heads, torch.float32)).all(-1)


def chain(q, k, v, do, key_mask, causal, keep, p, bias, scale, heads, dtype, rounded):
    """q, do [B, Lq, heads * 64], k, v [B, Lk, heads * 64]; key_mask [B, Lk] bool or None (True = attend); keep [B, heads, Lq, Lk] or None;
    bias [heads, Lq, Lk] or None.  Returns (out, dq, dk, dv), each [B, heads, L, 64] in ``dtype``."""
    r = bf16_round if rounded else (lambda x: x)
    Q, K, V, DO = (heads_first(t.to(dtype), heads) for t in (q, k, v, do))
    s = scores(q, k, key_mask, causal, bias, scale, heads, dtype)
    dead = torch.isinf(s).all(-1, keepdim=True)
    P = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1) * (~dead)
    kp = torch.ones_like(P) if keep is None else keep.to(dtype)
    inv_keep = 1.0 / (1.0 - p)
    Pd = r(P * kp * inv_keep)                              # the second product's operand
    O = r(Pd @ V)
    delta = (DO * O).sum(-1, keepdim=True)                 # from the output as stored
    dP = DO @ V.transpose(-1, -2)
    dS = r(P * (kp * dP * inv_keep - delta) * scale)       # the operand of both gradient products
    dV = r(Pd.transpose(-1, -2) @ DO)
    dK = r(dS.transpose(-1, -2) @ Q)
    dQ = r(dS @ K)
    return O, dQ, dK, dV


def eager(q, k, v, key_mask, causal, keep, p, bias, scale, heads):
    """tests/test_gpu_attn_long_train.py::_eager in the dtype of its inputs, for autograd: [B, Lq, heads * 64]"""
    B, Lq, _ = q.shape
    s = scores(q, k, key_mask, causal, bias, scale, heads, q.dtype)
    dead = torch.isinf(s).all(-1, keepdim=True)
    pr = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1) * (~dead)
    if keep is not None:
        pr = pr * keep.to(q.dtype) / (1.0 - p)
    return (pr @ heads_first(v, heads)).transpose(1, 2).reshape(B, Lq, heads * 64)


def tile_errors(a, r):
    """a, r [B, H, L, 64] -> (err, mag), each [B, H, ceil(L / 32)]: max|a - r| and max|r| over every 32-row tile -- a query block for out
    and dq, a key tile for dk and dv: the kernels' work units"""
    a, r = a.double(), r.double()
    B, H, L, D = r.shape
    nt = (L + TILE - 1) // TILE
    pad = nt * TILE - L
    d = torch.nn.functional.pad((a - r).abs(), (0, 0, 0, pad)).reshape(B, H, nt, TILE * D)
    m = torch.nn.functional.pad(r.abs(), (0, 0, 0, pad)).reshape(B, H, nt, TILE * D)
    return d.amax(-1), m.amax(-1)


def tile_budget(err_restated, mag):
    """what a tile of the kernel may be off by: three times the restatement's own error there (room for another summation order), two
    bf16 steps of the tile's largest value, the absolute floor"""
    return torch.maximum(torch.maximum(3.0 * err_restated, 2.0 ** -7 * mag), torch.full_like(mag, FLOOR))


def wide_error(name, a, r):
    """the project's tensor-wide measures: gpu_cases.rel_err for the output, max|a - r| / max(max|r|, 1e-2) for a gradient"""
    a, r = a.double(), r.double()
    if not torch.isfinite(a).all():
        return float("inf")
    e, m = float((a - r).abs().max()), float(r.abs().max())
    return e / (m + 1e-6) if name == "out" else e / max(m, 1e-2)


NAMES = ("out", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------------------------------------------- the cases
# mask: None | "random" (keep 75 %, key 0 always visible) | "suffix" (per-item lengths) | "dead1" (random, item 1 wholly masked when B = 3)
# bias: None | "plain" | "col7" (every 7th key column -inf for all rows) | "row5" (query row 5 all -inf) | "plus300" (plain + 300);
#       a bias means T5's form: scale 1, [H, Lq, Lk] of std 2, q and k at amplitude 0.35
# amp:  amplitude of q and k (None: 1.5, or 0.35 with a bias); zero_q: q = 0 (uniform rows)
# zero: gradients whose reference is identically zero and whose kernel value is the rounding of delta alone -- no tensor-wide bound
Case = namedtuple("Case", "name B H Lq Lk causal mask p bias amp zero_q zero")


def make_case(B, H, Lq, Lk, causal, mask, p, bias=None, amp=None, zero_q=False, zero=(), tag=""):
    name = f"{B}x{H}x{Lq}x{Lk}{'-causal' if causal else ''}{'-' + mask if mask else ''}-p{p}{'-bias_' + bias if bias else ''}{tag}"
    return Case(name, B, H, Lq, Lk, causal, mask, p, bias, amp, zero_q, tuple(zero))


CASES = [
    # tile edges on both axes, odd numbers of (batch, head) pairs
    make_case(1, 1, 31, 31, False, None, 0.1), make_case(3, 1, 32, 32, False, "random", 0.1), make_case(1, 3, 33, 33, True, None, 0.1),
    make_case(3, 5, 63, 65, False, "random", 0.1), make_case(1, 1, 64, 64, True, None, 0.0), make_case(3, 1, 65, 63, False, None, 0.1),
    make_case(1, 3, 95, 97, False, "random", 0.1), make_case(1, 1, 96, 96, False, None, 0.1), make_case(1, 1, 127, 127, True, None, 0.1),
    make_case(3, 3, 128, 128, True, "suffix", 0.1),
    # either side of the backward's occupancy switch (three workgroups per CU while Lqp + Lkp <= 128), unit counts 5 and 7
    make_case(3, 3, 97, 20, False, "random", 0.0), make_case(1, 5, 20, 97, False, None, 0.1), make_case(1, 3, 65, 100, False, "random", 0.1),
    make_case(3, 1, 64, 64, False, None, 0.1), make_case(3, 1, 65, 64, False, None, 0.1),
    # extreme aspect
    make_case(3, 1, 128, 1, False, None, 0.1, zero=("dq", "dk")), make_case(3, 1, 128, 1, False, None, 0.0), make_case(1, 1, 1, 128, False, "random", 0.9),
    make_case(3, 1, 1, 1, True, None, 0.1, zero=("dq", "dk")),
    # causal with Lq != Lk: the bound crosses tiles (Lq < Lk), the first Lq - Lk queries see nothing (Lq > Lk)
    make_case(3, 1, 20, 56, True, None, 0.1), make_case(3, 3, 56, 20, True, None, 0.1), make_case(1, 5, 33, 40, True, "suffix", 0.1),
    make_case(3, 1, 40, 33, True, None, 0.0),
    # dead rows: a dead item among live ones, also under the causal bound
    make_case(3, 3, 33, 33, False, "dead1", 0.1), make_case(3, 1, 56, 20, True, "dead1", 0.1),
    # bias forms
    make_case(3, 3, 33, 97, True, "random", 0.1, bias="col7"), make_case(1, 1, 32, 64, False, None, 0.0, bias="plain"),
    make_case(3, 1, 65, 33, False, "random", 0.1, bias="row5"), make_case(1, 3, 56, 56, False, None, 0.1, bias="plain"),
    make_case(1, 3, 56, 56, False, None, 0.1, bias="plus300"),
    # softmax extremes: nearly one-hot rows (scores in the tens), uniform rows
    make_case(1, 3, 56, 56, False, "random", 0.1, amp=4.0, tag="-amp4"), make_case(3, 1, 56, 56, False, None, 0.1, zero_q=True, tag="-q0"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def key_mask_of(kind, B, Lk, g):
    if kind is None:
        return None
    if kind == "suffix":
        lens = torch.randint(1, Lk + 1, (B,), generator=g)
        return torch.arange(Lk)[None, :] < lens[:, None]
    km = torch.rand(B, Lk, generator=g) > 0.25
    km[:, 0] = True
    if kind == "dead1" and B == 3:
        km[1] = False
    return km


def bias_of(kind, H, Lq, Lk, g):
    if kind is None:
        return None
    b = torch.randn(H, Lq, Lk, generator=g) * 2.0
    if kind == "col7":
        b[:, :, 6::7] = float("-inf")
    elif kind == "row5":
        b[:, 5, :] = float("-inf")
    elif kind == "plus300":
        b = b + 300.0
    return b


def inputs(case):
    """the case's tensors on the CPU: q, k, v, do (bf16, [B, L, H * 64]), key_mask, bias, scale.  "plain" and "plus300" draw the same
    numbers, so that the two runs differ by the constant alone."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    g = torch.Generator().manual_seed(Lq * 131 + Lk)
    amp = case.amp if case.amp is not None else (0.35 if case.bias else 1.5)
    mk = lambda L, a: (torch.randn(B, L, H * 64, generator=g) * a).bfloat16()
    q, k, v, do = mk(Lq, amp), mk(Lk, amp), mk(Lk, 1.5), mk(Lq, 1.0)
    if case.zero_q:
        q = torch.zeros_like(q)
    key_mask = key_mask_of(case.mask, B, Lk, g)
    bias = bias_of(case.bias, H, Lq, Lk, g)
    return q, k, v, do, key_mask, bias, (1.0 if case.bias else 64 ** -0.5)


def host_keep(case, seed=0):
    """a dropout mask for host-only tests (the GPU tests take the one the kernel exports)"""
    if case.p == 0.0:
        return None
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(case.B, case.H, case.Lq, case.Lk, generator=g) >= case.p
