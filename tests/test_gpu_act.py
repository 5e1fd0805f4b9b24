"""FFN activation + dropout pass (csrc/actdrop.hip, vlpet_amd.act) against the eager pair it replaces
(my_transformers/modeling_bart.py:1264-1265: activation_fn(fc1(x)) then F.dropout; T5DenseReluDense: relu then dropout),
with the mask the kernel applied exported so that forward and backward can be compared element for element."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_spec as DS
from oracle import vlpet_oracle as O
from gpu_cases import rel_err
from sentinel import pad_intact, padded_flat

pytestmark = pytest.mark.gpu

# ---- launch geometry (csrc/actdrop.hip) ---------------------------------------------------------------------------------------
ACT_CAP_GROUPS = 4096 * 256     # actdrop.hip:106 (cap = 256 * 16 workgroups) x actdrop.hip:109 (256 threads): 8-element groups per grid
                                # pass.  A thread takes groups g0 and g0 + stride per iteration (actdrop.hip:65-67); up to this
                                # count the second one never exists.

TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}
EAGER = {"gelu": F.gelu, "gelu_new": O.gelu_new, "relu": F.relu}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_act_dropout_matches_the_eager_pair(dtype, act, p):
    from vlpet_amd.act import act_dropout
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(7, 33, 3072, generator=g) * 2.0).to(dtype)
    dy = torch.randn(7, 33, 3072, generator=g).to(dtype)
    xg = x.cuda().requires_grad_(True)
    out, keep = act_dropout(xg, act, p, True, seed=1234, return_mask=True)
    out.backward(dy.cuda())
    keep = keep.cpu()
    assert keep.dtype == torch.uint8 and set(keep.unique().tolist()) <= {0, 1}
    if p == 0.0:
        assert int(keep.min()) == 1
    else:
        frac = float(keep.float().mean())
        assert abs(frac - (1.0 - p)) < 5e-3, frac                  # 710 k elements: 3 sigma is ~2e-3
    xr = x.float().requires_grad_(True)
    ref = EAGER[act](xr) * keep.float() / (1.0 - p)
    ref.backward(dy.float())
    assert rel_err(out.float().cpu(), ref.detach()) <= TOL[dtype]
    assert rel_err(xg.grad.float().cpu(), xr.grad) <= TOL[dtype]


def test_act_dropout_mask_is_a_function_of_the_seed_only():
    from vlpet_amd.act import act_dropout
    x = torch.randn(64, 3072, device="cuda", dtype=torch.bfloat16)
    _, k1 = act_dropout(x, "gelu", 0.1, True, seed=7, return_mask=True)
    _, k2 = act_dropout(x.float(), "relu", 0.1, True, seed=7, return_mask=True)     # other dtype, other activation: same mask
    _, k3 = act_dropout(x, "gelu", 0.1, True, seed=8, return_mask=True)
    assert torch.equal(k1, k2)
    assert not torch.equal(k1, k3)
    o_eval = act_dropout(x, "gelu", 0.1, False)                                      # eval: no dropout whatever p says
    assert rel_err(o_eval.float().cpu(), F.gelu(x.float()).cpu()) <= 1e-2


def test_act_dropout_argument_errors():
    from vlpet_amd import _lib
    from vlpet_amd.act import act_dropout
    with pytest.raises(RuntimeError):
        act_dropout(torch.randn(4, 16), "gelu", 0.0, False)                         # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        act_dropout(torch.randn(4, 12, device="cuda"), "gelu", 0.0, False)          # last dim not a multiple of 8
    with pytest.raises(RuntimeError):
        act_dropout(torch.randn(4, 16, device="cuda"), "swish", 0.0, False)
    lib = _lib.load()
    x = torch.randn(64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vlpet_act_dropout_fwd(x.data_ptr(), x.data_ptr(), None, 60, 0, 0.0, 0, _lib.VLPET_F32, st) == -1     # n % 8
    assert lib.vlpet_act_dropout_fwd(x.data_ptr(), x.data_ptr(), None, 64, 9, 0.0, 0, _lib.VLPET_F32, st) == -1     # act
    assert lib.vlpet_act_dropout_fwd(x.data_ptr(), x.data_ptr(), None, 64, 0, 1.0, 0, _lib.VLPET_F32, st) == -1     # p
    assert lib.vlpet_act_dropout_fwd(None, x.data_ptr(), None, 64, 0, 0.0, 0, _lib.VLPET_F32, st) == -5
    assert lib.vlpet_act_dropout_bwd(x.data_ptr(), x.data_ptr() + 4, x.data_ptr(), 8, 0, 0.0, 0, _lib.VLPET_F32, st) == -3


def test_host_encoder_layer_uses_the_fused_activation(monkeypatch):
    """The BART host layer goes through the HIP pass (not F.gelu + F.dropout) and agrees with the eager pair at p = 0."""
    import vlpet_amd.host.bart as HB
    calls = []
    real = HB.ffn_activation
    monkeypatch.setattr(HB, "ffn_activation", lambda x, act, p, tr: (calls.append((act, p, tr)), real(x, act, p, tr))[1])
    cfg = HB.vlpet_config(d_model=64, encoder_attention_heads=4, encoder_ffn_dim=128, adapter_down_dim=8, adapter_gating_down_dim=8,
                          dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    torch.manual_seed(0)
    layer = HB.BartEncoderLayer(cfg).cuda().eval()
    x = torch.randn(2, 8, 64, device="cuda")
    y = layer(x)
    assert calls == [("gelu", 0.0, False)]
    monkeypatch.setattr(HB, "ffn_activation", lambda x, act, p, tr: F.dropout(F.gelu(x), p=p, training=tr))
    y_ref = layer(x)
    assert rel_err(y, y_ref) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,La,Lv,d,p", [(5, 20, 36, 768, 0.1), (3, 7, 72, 64, 0.3), (4, 40, 36, 768, 0.0), (500, 20, 36, 768, 0.1)])
def test_concat_dropout_is_cat_then_dropout_with_the_regenerated_mask(B, La, Lv, d, p, dtype):
    """act.concat_dropout (src/modeling_bart.py:804-820): x = dropout(cat([a, v], 1)); every element is either 0 or its source / (1 - p),
    the kept fraction is 1 - p, and the backward applies the SAME mask to the two slices of the gradient."""
    from vlpet_amd.act import concat_dropout
    torch.manual_seed(0)
    a = (torch.randn(B, La, d) + 3.0).cuda().to(dtype).requires_grad_(True)       # (bounded away from 0: a zero output is a dropped element)
    v = (torch.randn(B, Lv, d) - 3.0).cuda().to(dtype).requires_grad_(True)
    x = concat_dropout(a, v, p, training=True, seed=11)
    ref = torch.cat([a, v], 1).detach().float()
    keep = x.detach().float() != 0
    if p == 0.0:
        assert torch.equal(x.detach(), torch.cat([a, v], 1).detach())
    else:
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) < 0.02, frac
        scaled = (ref / (1 - p)).to(dtype).float()
        assert float(((x.detach().float() - scaled) * keep).abs().max()) <= 2.0 ** -7 * float(scaled.abs().max())
    dx = torch.randn(B, La + Lv, d).cuda().to(dtype)
    x.backward(dx)
    want = (dx.float() * keep / (1 - p)).to(dtype).float()
    assert float((a.grad.float() - want[:, :La]).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    assert float((v.grad.float() - want[:, La:]).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    # the same seed gives the same mask; eval mode is the plain concatenation
    x2 = concat_dropout(a, v, p, training=True, seed=11)
    assert torch.equal(x2, x)
    assert torch.equal(concat_dropout(a, v, p, training=False), torch.cat([a, v], 1))
    # only one side wants a gradient
    v2 = v.detach()
    x3 = concat_dropout(a, v2, p, training=True, seed=11)
    a.grad = None
    x3.backward(dx)
    assert float((a.grad.float() - want[:, :La]).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


# ---- the two-group path: group counts at and past the grid cap, through the ABI ----------------------------------------------
_C = math.sqrt(2.0 / math.pi)


def _act64(act, x):
    """fp64 activation and derivative (F.gelu; HF NewGELUActivation; relu), in the forms that keep their relative accuracy in the
    negative tail: Phi(x) = erfc(-x / sqrt 2) / 2, and 0.5 (1 + tanh u) = sigmoid(2 u), 1 - tanh^2 u = 4 s (1 - s)."""
    if act == "relu":
        return x.clamp_min(0.0), (x > 0).double()
    if act == "gelu":
        cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
        return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    s = torch.sigmoid(2.0 * _C * (x + 0.044715 * x ** 3))
    return x * s, s + x * 2.0 * s * (1.0 - s) * _C * (1.0 + 3 * 0.044715 * x * x)


def _act_abi(act, p, seed, x, dy, want_mask=True):
    """vlpet_act_dropout_fwd / _bwd on flat tensors, outputs NaN-filled with sentinel elements behind.  -> out, dx, mask (CPU)"""
    from vlpet_amd import _lib
    from vlpet_amd.act import ACTS
    lib = _lib.load()
    lib.vlpet_set_seed_counter(None)
    n = x.numel()
    io = _lib.VLPET_F32 if x.dtype == torch.float32 else _lib.VLPET_BF16
    st = torch.cuda.current_stream().cuda_stream
    xg, dyg = x.cuda(), dy.cuda()
    obuf, out = padded_flat(n, x.dtype)
    dbuf, dx = padded_flat(n, x.dtype)
    mbuf, mask = padded_flat(n, torch.uint8) if want_mask else (None, None)
    assert lib.vlpet_act_dropout_fwd(xg.data_ptr(), out.data_ptr(), mask.data_ptr() if want_mask else None, n, ACTS[act], p, seed, io, st) == 0
    assert lib.vlpet_act_dropout_bwd(dyg.data_ptr(), xg.data_ptr(), dx.data_ptr(), n, ACTS[act], p, seed, io, st) == 0
    torch.cuda.synchronize()
    assert pad_intact(obuf, out) and pad_intact(dbuf, dx) and (not want_mask or pad_intact(mbuf, mask))
    return out.cpu(), dx.cpu(), mask.cpu() if want_mask else None


def _away_from_zero(n, gen, dtype):
    x = torch.randn(n, generator=gen)
    return (torch.where(x < 0, -1.0, 1.0) * (x.abs() + 0.25)).to(dtype)


G = ACT_CAP_GROUPS
TWO_GROUP_CASES = ([(torch.bfloat16, "gelu", 0.1, g) for g in (G, G + 1, 2 * G, 2 * G + 1, 3 * G + 5)]
                   + [(torch.bfloat16, "gelu_new", 0.1, 3 * G + 5), (torch.bfloat16, "relu", 0.1, 3 * G + 5)]
                   + [(torch.float32, "gelu", 0.0, 2 * G + 1), (torch.float32, "gelu", 0.5, 2 * G + 1)])


@pytest.mark.parametrize("dtype,act,p,groups", TWO_GROUP_CASES,
                         ids=[f"{str(c[0])[6:]}-{c[1]}-p{c[2]}-{c[3]}" for c in TWO_GROUP_CASES])
def test_act_dropout_at_and_past_the_grid_cap(dtype, act, p, groups):
    """Forward and backward against the fp64 activation / derivative times the exported mask; an element is exactly 0 where the
    mask drops; the whole exported mask is dropout_spec's (group g keyed by g, not by its partner group)."""
    assert 3 * G + 5 >= 3 * ACT_CAP_GROUPS
    n = 8 * groups
    seed = 0x0123456789ABCDEF + 7 * groups
    if groups == G + 1:             # the seed is one under which group G's mask differs from that of its partner, group 0: here it
        thr = DS.tail_thr(p)        # is the only second group, and a mask keyed by the partner must show in it
        assert int(DS.keep8(np.array([G]), seed, thr)[0]) != int(DS.keep8(np.array([0]), seed, thr)[0])
    gen = torch.Generator().manual_seed(groups % 1000 + int(p * 10))
    x = (torch.randn(n, generator=gen) * 2.0).to(dtype)
    dy = _away_from_zero(n, gen, dtype)
    out, dx, mask = _act_abi(act, p, seed, x, dy)
    want = torch.from_numpy(DS.keep_mask(groups, 8, seed, p).reshape(-1))
    assert set(mask.unique().tolist()) <= {0, 1}
    bad = mask.bool() != want
    assert not bool(bad.any()), f"{int(bad.sum())} mask elements differ from the spec, first at {int(bad.nonzero()[0])}"
    f, df = _act64(act, x.double())
    k = want.double() * float(DS.keep_scale(p) if DS.tail_thr(p) else 1.0)
    e_f, e_b = rel_err(out, f * k), rel_err(dx, dy.double() * df * k)
    print(f"ACT {act} {dtype} p={p} groups={groups}: fwd {e_f:.2e} bwd {e_b:.2e} (TOL {TOL[dtype]:.0e})")
    assert e_f <= TOL[dtype] and e_b <= TOL[dtype]
    assert bool((out[~want] == 0).all()) and bool((dx[~want] == 0).all())
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dx.float()).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_act_dropout_backward_past_the_cap_applies_the_spec(dtype):
    """The backward exports no mask: read it structurally, as test_gpu_dropout_masks.test_act_dropout_backward_applies_the_spec does
    (relu of positive inputs has derivative 1: dx = dy * keep_scale where the spec keeps, 0 where it drops), at 2 G + 1 groups."""
    groups, p, seed = 2 * G + 1, 0.1, 0x1F2E3D4C5B6A7988
    gen = torch.Generator().manual_seed(9)
    x = (torch.rand(8 * groups, generator=gen) + 0.5).to(dtype)
    dy = _away_from_zero(8 * groups, gen, dtype)
    _, dx, _ = _act_abi("relu", p, seed, x, dy, want_mask=False)
    keep = DS.keep_mask(groups, 8, seed, p).reshape(-1)
    got, want = dx.float().numpy(), (dy.float().numpy() * DS.keep_scale(p)).astype(np.float32)
    assert np.all(got[~keep] == 0), f"{int((got[~keep] != 0).sum())} nonzero where the spec drops"
    if dtype == torch.float32:
        assert np.array_equal(got[keep], want[keep])
    else:
        assert np.all(np.abs(got[keep] - want[keep]) <= np.abs(want[keep]) * 2.0 ** -8)


# ---- value sweep ---------------------------------------------------------------------------------------------------------------
SWEEP = [0.0, 1e-30, 1e-3, 0.5, 1.0, 3.0, 4.0, 5.5, 8.0, 12.0, 40.0, 1e4, 1e18]     # and their negatives; beyond 1e18 x^2 overflows
                                                                                    # in the reference formula too: out of scope


def _sweep(act):
    v = torch.tensor([s * a for a in SWEEP for s in (1.0, -1.0)], dtype=torch.float32)
    x = torch.cat([v, torch.ones(-len(v) % 8)])                   # padded to a multiple of 8
    out, dx, _ = _act_abi(act, 0.0, 0, x, torch.ones_like(x), want_mask=False)
    f, df = _act64(act, x.double())
    return x, out, dx, f, df


@pytest.mark.parametrize("act", ["gelu", "gelu_new", "relu"])
def test_activation_value_sweep(act):
    """Hand-picked values from +-0 to +-1e18, fp32 IO, p = 0, forward and derivative (dy = 1).
    relu is exact.  gelu (erf form): forward |err| <= 4e-7 |x| + 2^-22 |ref| -- Abramowitz & Stegun 7.1.26 bounds Phi by 7.5e-8, the
    rest is one ulp each of the hardware reciprocal and exponential on h <= 0.5.  The derivative Phi + x phi is held to the same
    bound and, as it carries the error of Phi once and not times x, to 4e-7 + 2^-22 |ref| as well:
    |err| <= min(4e-7 |x|, 4e-7) + 2^-22 |ref|.  gelu_new: per value at most 4 x the error of torch's own fp32
    F.gelu(approximate="tanh") (and its autograd) against the same fp64 reference, or 2^-22 relative, whichever is larger."""
    x, out, dx, f, df = _sweep(act)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
    o64, d64, x64 = out.double(), dx.double(), x.double()
    assert bool((out[x > 0] > 0).all()) and bool((out[x == 0] == 0).all())
    assert bool((out[x < 0] == 0).all()) if act == "relu" else bool((out[x < 0] <= 0).all())
    if act == "relu":
        assert torch.equal(o64, f) and torch.equal(d64, df)
        return
    e_f, e_d = (o64 - f).abs(), (d64 - df).abs()
    if act == "gelu":
        b_f, b_d = 4e-7 * x64.abs() + 2.0 ** -22 * f.abs(), 4e-7 * x64.abs().clamp_max(1.0) + 2.0 ** -22 * df.abs()
    else:
        xt = x.clone().requires_grad_(True)
        t = F.gelu(xt, approximate="tanh")
        t.backward(torch.ones_like(t))
        t_f = (t.detach().double() - f).abs().nan_to_num(nan=float("inf"))
        t_d = (xt.grad.double() - df).abs().nan_to_num(nan=float("inf"))
        b_f, b_d = torch.maximum(4 * t_f, 2.0 ** -22 * f.abs()), torch.maximum(4 * t_d, 2.0 ** -22 * df.abs())
        def r(e, te, ref):          # worst kernel error / torch error over the values where 4 x torch's error is the governing term
            m = (4 * te > 2.0 ** -22 * ref.abs()) & torch.isfinite(te)
            return float((e[m] / te[m]).max()) if bool(m.any()) else 0.0
        print(f"ACT gelu_new worst kernel error / torch fp32 error: fwd {r(e_f, t_f, f):.3f} derivative {r(e_d, t_d, df):.3f}")
    tiny = 1e-300
    print(f"ACT sweep {act}: worst err / bound fwd {float((e_f / (b_f + tiny)).max()):.3f} derivative {float((e_d / (b_d + tiny)).max()):.3f}")
    assert bool((e_f <= b_f).all()), [(float(a), float(e), float(b)) for a, e, b in zip(x, e_f, b_f) if e > b]
    assert bool((e_d <= b_d).all()), [(float(a), float(e), float(b)) for a, e, b in zip(x, e_d, b_d) if e > b]
