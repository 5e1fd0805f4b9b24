"""vlpet_phm_expand_pair_fwd / _bwd / vlpet_phm_workspace_bytes (csrc/phm.hip, include/vlpet_hip.h) without a GPU: the symbols and their
ctypes signatures, the version bump, every argument error as a negative code before any launch, the workspace size, and the Python
entry point's refusal of CPU tensors."""
import pytest
import torch

A = 1 << 20         # 16-byte aligned non-NULL values, far enough apart not to overlap: every call below returns before a dereference
E_SHAPE, E_RANK, E_ALIGN, E_WORKSPACE, E_NULL, E_DTYPE, E_ALIAS = -1, -2, -3, -4, -5, -6, -7
FWD = ("rule_d", "W_d", "rule_u", "W_u", "wt_d", "wt_u")
BWD = ("dwt_d", "dwt_u", "rule_d", "W_d", "rule_u", "W_u", "drule_d", "dW_d", "drule_u", "dW_u", "ws")


def _ptrs(names):
    return {n: (i + 1) * 16 * A for i, n in enumerate(names)}


def _fwd(lib, d=768, r=96, n=2, pdt=0, **over):
    p = {**_ptrs(FWD), **over}
    return lib.vlpet_phm_expand_pair_fwd(*[p[k] for k in FWD], d, r, n, pdt, None)


def _bwd(lib, d=768, r=96, n=2, pdt=0, ws_bytes=None, **over):
    p = {**_ptrs(BWD), **over}
    if ws_bytes is None:
        ws_bytes = lib.vlpet_phm_workspace_bytes(d, r, n) or 1 << 20
    return lib.vlpet_phm_expand_pair_bwd(*[p[k] for k in BWD], ws_bytes, d, r, n, pdt, None)


def test_symbols_signatures_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name, n in (("vlpet_phm_expand_pair_fwd", 11), ("vlpet_phm_expand_pair_bwd", 17), ("vlpet_phm_workspace_bytes", 3)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n
    assert lib.vlpet_version() > 660                    # the parent's


def test_workspace_is_positive_and_monotone_in_n():
    from vlpet_amd import _lib
    lib = _lib.load()
    for d, r, ns in ((768, 96, (1, 2, 3, 4, 6, 8)), (64, 8, (1, 2, 4, 8)), (840, 840, (1, 2, 3, 4, 5, 6, 7, 8))):
        sizes = [lib.vlpet_phm_workspace_bytes(d, r, n) for n in ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
        assert sizes == sorted(sizes), sizes
    assert lib.vlpet_phm_workspace_bytes(768, 96, 8) > lib.vlpet_phm_workspace_bytes(768, 96, 1)
    # at least one n^3 block of floats per 32 x 32 tile of W of either layer
    assert lib.vlpet_phm_workspace_bytes(768, 96, 2) >= (12 * 2 + 2 * 12) * 8 * 4
    for d, r, n in ((768, 96, 0), (768, 96, 9), (768, 96, 5), (770, 96, 4), (2, 96, 4), (0, 0, 1), (-8, 8, 2)):
        assert lib.vlpet_phm_workspace_bytes(d, r, n) == 0, (d, r, n)


def test_forward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name in FWD:
        assert _fwd(lib, **{name: None}) == E_NULL, name
    assert _fwd(lib, pdt=2) == E_DTYPE and _fwd(lib, pdt=-1) == E_DTYPE
    assert _fwd(lib, n=0) == E_RANK and _fwd(lib, n=9) == E_RANK and _fwd(lib, n=-2) == E_RANK
    assert _fwd(lib, d=770, n=4) == E_SHAPE                   # n does not divide d
    assert _fwd(lib, r=98, n=4) == E_SHAPE                    # n does not divide r
    assert _fwd(lib, d=0) == E_SHAPE and _fwd(lib, r=0, n=2) == E_SHAPE and _fwd(lib, d=4, r=96, n=8) == E_SHAPE
    for name in FWD:
        assert _fwd(lib, **{name: _ptrs(FWD)[name] + 8}) == E_ALIGN, name
    p = _ptrs(FWD)
    for out in ("wt_d", "wt_u"):
        for inp in ("rule_d", "W_d", "rule_u", "W_u"):
            assert _fwd(lib, **{out: p[inp]}) == E_ALIAS, (out, inp)
        # overlapping by its last 16 bytes only
        assert _fwd(lib, **{out: p["W_d"] - 768 * 96 * 4 + 16}) == E_ALIAS
    assert _fwd(lib, wt_u=p["wt_d"] + 768 * 96 * 4 - 16) == E_ALIAS            # the two outputs
    # a shared rule is the same memory passed twice: inputs may alias each other (the answer below comes from the NEXT check)
    assert _fwd(lib, rule_u=p["rule_d"], wt_u=p["W_u"]) == E_ALIAS


def test_backward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name in BWD:
        assert _bwd(lib, **{name: None}) == E_NULL, name
    assert _bwd(lib, pdt=5) == E_DTYPE
    assert _bwd(lib, n=0) == E_RANK and _bwd(lib, n=9) == E_RANK
    assert _bwd(lib, d=770, n=4) == E_SHAPE and _bwd(lib, r=98, n=4) == E_SHAPE
    for name in BWD:
        assert _bwd(lib, **{name: _ptrs(BWD)[name] + 4}) == E_ALIGN, name
    need = lib.vlpet_phm_workspace_bytes(768, 96, 2)
    assert _bwd(lib, ws_bytes=need - 1) == E_WORKSPACE and _bwd(lib, ws_bytes=0) == E_WORKSPACE
    p = _ptrs(BWD)
    for out in ("drule_d", "dW_d", "drule_u", "dW_u", "ws"):
        for inp in ("dwt_d", "dwt_u", "rule_d", "W_d", "rule_u", "W_u"):
            assert _bwd(lib, **{out: p[inp]}) == E_ALIAS, (out, inp)
    assert _bwd(lib, dW_u=p["dW_d"]) == E_ALIAS and _bwd(lib, drule_u=p["drule_d"]) == E_ALIAS and _bwd(lib, ws=p["dW_d"]) == E_ALIAS
    assert _bwd(lib, ws=p["drule_d"] - need + 16) == E_ALIAS
    # the error order of the header: a NULL wins over a bad dtype, the dtype over n, n over the shape, the shape over alignment, ..
    assert _bwd(lib, ws=None, pdt=9, n=0) == E_NULL and _bwd(lib, pdt=9, n=0) == E_DTYPE and _bwd(lib, n=0, d=7) == E_RANK
    assert _bwd(lib, d=770, n=4, ws=p["ws"] + 8) == E_SHAPE and _bwd(lib, ws=p["ws"] + 8, ws_bytes=0) == E_ALIGN
    assert _bwd(lib, ws_bytes=0, dW_u=p["dW_d"]) == E_WORKSPACE


def test_python_entry_point_refuses_cpu_tensors_and_counts_nothing():
    import vlpet_amd.functional as VF
    assert VF.PHM_MAX_DIVISION == 8 and isinstance(VF.PHM_CALLS, int)
    rule, Wd, Wu = torch.zeros(2, 2, 2), torch.zeros(2, 32, 4), torch.zeros(2, 4, 32)
    n0 = VF.PHM_CALLS
    with pytest.raises(RuntimeError):
        VF.phm_expand_pair(rule, Wd, rule, Wu, 2)
    with pytest.raises(RuntimeError):
        VF.phm_expand_pair_into(rule, Wd, rule, Wu, 2)
    assert VF.PHM_CALLS == n0
