"""vlpet_attn_long_fwd_train / vlpet_attn_long_bwd (csrc/attn_long.hip, csrc/attn_long_bwd.hip, include/vlpet_hip.h) without a GPU: the
symbols and their ctypes signatures, the version bump, the argument checks that come back as negative codes before any launch, the
Python entry points' refusal of CPU tensors, and the hosts' switch."""
import pytest
import torch

E_SHAPE, E_ALIGN, E_NULL = -1, -3, -5


def _fwd(lib, q=16, k=16, v=16, km=None, bias=None, o=16, lse=16, keep=None, B=2, H=12, Lq=200, Lk=664, ld_q=768, ld_k=768, ld_v=768,
         causal=0, scale=0.125, p=0.1, seed=7):
    return lib.vlpet_attn_long_fwd_train(q, k, v, km, bias, o, lse, keep, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed, None)


def _bwd(lib, q=16, k=16, v=16, o=16, do=16, lse=16, km=None, bias=None, bias_t=None, dq=16, dk=16, dv=16, B=2, H=12, Lq=200, Lk=664,
         ld_q=768, ld_k=768, ld_v=768, causal=0, scale=0.125, p=0.1, seed=7, delta=16):
    return lib.vlpet_attn_long_bwd(q, k, v, o, do, lse, km, bias, bias_t, dq, dk, dv, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p,
                                   seed, delta, None)


def test_symbols_signatures_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name, n_args in (("vlpet_attn_long_fwd_train", 20), ("vlpet_attn_long_bwd", 25)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args
    # the arguments of vlpet_attn_long_fwd + keep_out, p, seed; those of vlpet_attn_bwd_kv + the scratch
    assert len(_lib.SIGNATURES["vlpet_attn_long_fwd"][1]) + 3 == 20
    assert len(_lib.SIGNATURES["vlpet_attn_bwd_kv"][1]) + 1 == 25
    assert lib.vlpet_version() >= 651


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_argument_errors_come_back_before_any_launch(call):
    from vlpet_amd import _lib
    lib = _lib.load()
    assert call(lib, Lk=1025) == E_SHAPE
    assert call(lib, Lq=1025) == E_SHAPE
    assert call(lib, Lq=0) == E_SHAPE
    assert call(lib, Lk=0) == E_SHAPE
    assert call(lib, B=0) == E_SHAPE
    assert call(lib, H=0) == E_SHAPE
    assert call(lib, o=None) == E_NULL
    assert call(lib, lse=None) == E_NULL
    assert call(lib, q=None) == E_NULL
    assert call(lib, q=8) == E_ALIGN                   # misaligned q
    assert call(lib, v=8) == E_ALIGN
    assert call(lib, bias=8) == E_ALIGN
    assert call(lib, scale=0.0) == E_SHAPE
    assert call(lib, ld_k=12 * 64 - 8) == E_SHAPE      # ld_k < H * 64
    assert call(lib, ld_v=12 * 64 + 4) == E_SHAPE      # not a multiple of 8
    assert call(lib, ld_q=760) == E_SHAPE
    assert call(lib, p=1.0) == E_SHAPE                 # p outside [0, 1)
    assert call(lib, p=-0.1) == E_SHAPE
    assert call(lib, p=float("nan")) == E_SHAPE


def test_backward_only_argument_errors():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert _bwd(lib, delta=None) == E_NULL             # the scratch is the caller's
    assert _bwd(lib, do=None) == E_NULL
    assert _bwd(lib, dq=None) == E_NULL
    assert _bwd(lib, dk=None) == E_NULL
    assert _bwd(lib, dv=None) == E_NULL
    assert _bwd(lib, do=8) == E_ALIGN
    assert _bwd(lib, dk=8) == E_ALIGN


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import vlpet_amd.attention as A
    assert isinstance(A.LONG_TRAIN_CALLS, int)
    q = torch.zeros(1, 200, 768, dtype=torch.bfloat16, requires_grad=True)
    n0 = A.LONG_TRAIN_CALLS
    with pytest.raises(RuntimeError):
        A.long_attention_train(q, q, q, 12)
    with pytest.raises(RuntimeError):
        A.long_attention_train(q, q, q, 12, p=0.1, training=True)
    with pytest.raises(RuntimeError):
        A.long_self_attention_train(torch.zeros(1, 200, 3 * 768, dtype=torch.bfloat16), 12)
    with pytest.raises(RuntimeError):
        A.long_attention_train(q, None, q, 12)
    assert A.LONG_TRAIN_CALLS == n0


def test_host_switches_exist_and_default_off():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    assert HB.LONG_ATTENTION_TRAIN is False and HT.LONG_ATTENTION_TRAIN is False
    assert HB.LONG_ATTENTION is False and HT.LONG_ATTENTION is False


def test_the_switch_applies_only_where_dropout_or_a_gradient_is_needed(monkeypatch):
    import os
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ab_switches.py")
    assert "VLPET_LONG_ATTENTION_TRAIN" in open(path).read()
    monkeypatch.setattr(HB, "LONG_ATTENTION_TRAIN", False)
    monkeypatch.setattr(HT, "LONG_ATTENTION_TRAIN", False)
    assert HB._long_train_applies(664, 664, 0.1, True) is False
    monkeypatch.setattr(HB, "LONG_ATTENTION_TRAIN", True)
    monkeypatch.setattr(HT, "LONG_ATTENTION_TRAIN", True)
    assert HB._long_train_applies(664, 664, 0.1, True) is True and HT._long_train_applies(20, 664, 0.1, True) is True
    assert HB._long_train_applies(128, 128, 0.1, True) is False          # the short kernels' lengths
    assert HB._long_train_applies(664, 1025, 0.1, True) is False
    assert HB._long_train_applies(664, 664, 0.1, False) is False         # neither dropout nor a gradient
    x = torch.zeros(1, requires_grad=True)
    assert HB._long_train_applies(664, 664, 0.0, False, x) is True
    with torch.no_grad():
        assert HT._long_train_applies(664, 664, 0.0, False, x) is False
    monkeypatch.setattr(HB, "EAGER_ATTENTION", True)
    assert HB._long_train_applies(664, 664, 0.1, True) is False
