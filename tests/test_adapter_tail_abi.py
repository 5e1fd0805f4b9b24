"""vlpet_adapter_tail_fwd / _applies / _rows (csrc/adapter_tail.hip, include/vlpet_hip.h) without a GPU: the symbols and their ctypes
signatures, the version bump, every argument error as a negative code before any launch, the Python entry point's refusal of CPU tensors
and the host switches."""
import pytest
import torch

A = 4096            # a 16-byte aligned non-NULL value: every call below returns before it could be dereferenced
E_SHAPE, E_RANK, E_ALIGN, E_NULL, E_DTYPE, E_ALIAS = -1, -2, -3, -5, -6, -7


def _call(lib, h=A, res=2 * A, wd=A, bd=A, wu=A, bu=A, gamma=A, beta=A, out=1 << 30, M=250, d=768, r=96, scale=1.0, eps=1e-5, norm=1,
          pdt=0, dt=1):
    return lib.vlpet_adapter_tail_fwd(h, res, wd, bd, wu, bu, gamma, beta, out, M, d, r, scale, eps, norm, pdt, dt, None)


def test_symbols_signatures_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name, n in (("vlpet_adapter_tail_fwd", 18), ("vlpet_adapter_tail_applies", 4), ("vlpet_adapter_tail_rows", 0)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n
    assert lib.vlpet_version() > 651                    # the parent's
    assert lib.vlpet_adapter_tail_rows() == 16
    assert b"overlap" in lib.vlpet_error_string(E_ALIAS)


def test_applies_names_the_two_geometries_in_both_dtypes():
    from vlpet_amd import _lib
    lib = _lib.load()
    for dt in (_lib.VLPET_BF16, _lib.VLPET_F32):
        assert lib.vlpet_adapter_tail_applies(1, 768, 96, dt) == 1 and lib.vlpet_adapter_tail_applies(28000, 64, 8, dt) == 1
        assert lib.vlpet_adapter_tail_applies(0, 768, 96, dt) == 0 and lib.vlpet_adapter_tail_applies(-3, 64, 8, dt) == 0
        for d, r in ((768, 8), (64, 96), (768, 192), (1024, 96), (64, 16), (0, 0)):
            assert lib.vlpet_adapter_tail_applies(250, d, r, dt) == 0
    assert lib.vlpet_adapter_tail_applies(250, 768, 96, 7) == 0


def test_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name in ("h", "res", "wd", "bd", "wu", "bu", "out"):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, gamma=None) == E_NULL
    assert _call(lib, gamma=None, beta=None, norm=0, out=A) == E_ALIAS          # the identity norm needs neither: the LAST check answers
    assert _call(lib, beta=None, out=A) == E_ALIAS                              # beta is optional
    assert _call(lib, M=0) == E_SHAPE and _call(lib, M=-5) == E_SHAPE
    assert _call(lib, d=768, r=8) == E_RANK and _call(lib, d=64, r=96) == E_RANK and _call(lib, d=512, r=64) == E_RANK
    assert _call(lib, d=0) == E_SHAPE and _call(lib, r=0) == E_SHAPE
    assert _call(lib, dt=7) == E_DTYPE and _call(lib, pdt=3) == E_DTYPE
    assert _call(lib, norm=2) == E_SHAPE and _call(lib, norm=-1) == E_SHAPE
    for name in ("h", "res", "wd", "bd", "wu", "bu", "gamma", "beta", "out"):
        kw = {name: (A if name != "out" else 1 << 30) + 8}
        assert _call(lib, **kw) == E_ALIGN, name
    # out overlapping h or res: equal, or shifted by less than M * d elements
    assert _call(lib, out=A) == E_ALIAS and _call(lib, out=2 * A) == E_ALIAS
    nbytes = 250 * 768 * 2
    assert _call(lib, h=1 << 20, out=(1 << 20) + nbytes - 16) == E_ALIAS
    assert _call(lib, res=(1 << 20), h=1 << 24, out=(1 << 20) - nbytes + 16) == E_ALIAS


def test_python_entry_point_refuses_cpu_tensors_and_counts_nothing():
    import vlpet_amd.adapter_tail as AT
    assert AT.row_tile() == 16 and isinstance(AT.ADAPTER_TAIL_MAX_ROWS, int) and AT.ADAPTER_TAIL_MAX_ROWS >= 0
    assert AT.applies(250, 768, 96, torch.bfloat16) and AT.applies(3, 64, 8, torch.float32)
    assert not AT.applies(250, 768, 96, torch.float16) and not AT.applies(250, 768, 64, torch.bfloat16)
    h = torch.zeros(4, 64)
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))
    (wd, bd), (wu, bu) = lin(8, 64), lin(64, 8)
    n0 = AT.CALLS
    with pytest.raises(RuntimeError):
        AT.adapter_tail(h, h.clone(), wd, bd, wu, bu, None)
    assert AT.CALLS == n0


def test_host_helpers_compose_without_a_gpu_and_the_switches_exist():
    import vlpet_amd.host.bart as HB
    import vlpet_amd.host.common as HC
    import vlpet_amd.host.t5 as HT
    from vlpet_amd.adapters import AdapterConfig, AdapterController
    assert HB.FUSE_ADAPTER_TAIL in (True, False) and HT.FUSE_ADAPTER_TAIL in (True, False)
    assert callable(HB._adapter_then_tail) and callable(HT._adapter_then_tail)
    ctl = AdapterController(AdapterConfig(tasks=["vqa"], input_dim=64, d_model=64, use_single_adapter=True, reduction_factor=8))
    h = torch.zeros(2, 1, 64)
    with torch.no_grad():
        assert HC.fused_adapter_tail(True, ctl, "vqa", h, h, None, 0.1, False) is None          # CPU tensors: the composition
