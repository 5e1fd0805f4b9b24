"""vlpet_attn_long_fwd (csrc/attn_long.hip, include/vlpet_hip.h) without a GPU: the symbol and its ctypes signature, the version
bump, the argument checks that come back as negative codes before any launch, and the Python entry point's refusal of CPU tensors."""
import pytest
import torch


def _call(lib, q=16, k=16, v=16, km=None, bias=None, o=16, lse=16, B=2, H=12, Lq=200, Lk=664, ld_q=768, ld_k=768, ld_v=768, causal=0,
          scale=0.125):
    return lib.vlpet_attn_long_fwd(q, k, v, km, bias, o, lse, B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, None)


def test_symbol_signature_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert "vlpet_attn_long_fwd" in _lib.SIGNATURES
    assert hasattr(lib, "vlpet_attn_long_fwd")
    assert len(_lib.SIGNATURES["vlpet_attn_long_fwd"][1]) == 17
    assert lib.vlpet_version() >= 650


def test_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    E_SHAPE, E_ALIGN, E_NULL = -1, -3, -5
    assert _call(lib, Lk=1025) == E_SHAPE
    assert _call(lib, Lq=1025) == E_SHAPE
    assert _call(lib, Lq=0) == E_SHAPE
    assert _call(lib, B=0) == E_SHAPE
    assert _call(lib, o=None) == E_NULL
    assert _call(lib, lse=None) == E_NULL
    assert _call(lib, q=8) == E_ALIGN                   # misaligned q
    assert _call(lib, bias=8) == E_ALIGN
    assert _call(lib, scale=0.0) == E_SHAPE
    assert _call(lib, ld_k=12 * 64 - 8) == E_SHAPE      # ld_k < H * 64
    assert _call(lib, ld_v=12 * 64 + 4) == E_SHAPE      # not a multiple of 8
    assert _call(lib, ld_q=760) == E_SHAPE


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import vlpet_amd.attention as A
    assert A.MAX_LONG == 1024 and isinstance(A.LONG_CALLS, int)
    q = torch.zeros(1, 200, 768, dtype=torch.bfloat16)
    assert not A.supported_long(q, q, 12)
    n0 = A.LONG_CALLS
    with pytest.raises(RuntimeError):
        A.long_attention(q, q, q, 12)
    with pytest.raises(RuntimeError):
        A.long_self_attention(torch.zeros(1, 200, 3 * 768, dtype=torch.bfloat16), 12)
    assert A.LONG_CALLS == n0


def test_attn_bias_builds_its_transpose_on_demand():
    """The forward-only path never pays for the backward's transposed table; today's constructor behaviour is the default."""
    import vlpet_amd.attention as A
    rel = torch.randn(1, 2, 5, 7)
    eager, lazy = A.AttnBias(rel), A.AttnBias(rel, transposed=False)
    assert eager._bt is not None and lazy._bt is None
    assert torch.equal(lazy.b, eager.b) and lazy.b.shape == (2, 32, 32)
    assert torch.equal(lazy.bt, eager.bt) and lazy._bt is not None


def test_host_switches_exist_and_default_off():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.t5 as HT
    assert HB.LONG_ATTENTION is False and HT.LONG_ATTENTION is False
