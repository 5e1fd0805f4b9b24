"""vlpet_prefix_concat_dropout_fwd / _bwd, vlpet_prefix_concat_chunks, vlpet_prefix_concat_ws_bytes (csrc/prefix_cat.hip,
include/vlpet_hip.h) without a GPU: the symbols and their ctypes signatures, the version bump, the host helpers' arithmetic and every
argument error as a negative code before any launch."""
import prompt_spec as PS

A = 4096            # a 16-byte aligned non-NULL value: every call below returns before it could be dereferenced
E_SHAPE, E_ALIGN, E_NULL, E_DTYPE = -1, -3, -5, -6


def _fwd(lib, pre=A, a=2 * A, v=3 * A, x=1 << 30, B=4, P=5, La=7, Lv=3, d=64, p=0.1, dt=1):
    return lib.vlpet_prefix_concat_dropout_fwd(pre, a, v, x, B, P, La, Lv, d, p, 11, dt, None)


def _bwd(lib, dx=1 << 30, dpre=A, da=2 * A, dv=3 * A, ws=1 << 20, B=4, P=5, La=7, Lv=3, d=64, p=0.1, dt=1):
    return lib.vlpet_prefix_concat_dropout_bwd(dx, dpre, da, dv, ws, B, P, La, Lv, d, p, 11, dt, None)


def test_symbols_signatures_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name, n in (("vlpet_prefix_concat_dropout_fwd", 13), ("vlpet_prefix_concat_dropout_bwd", 14), ("vlpet_prefix_concat_chunks", 1),
                    ("vlpet_prefix_concat_ws_bytes", 3)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n
    assert lib.vlpet_version() > 670                    # the parent's


def test_chunk_count_depends_on_the_batch_alone_and_sizes_the_workspace():
    from vlpet_amd import _lib
    lib = _lib.load()
    for B in (1, 2, 31, 32, 33, 63, 64, 65, 67, 416, 500, 1000, 100000):
        cs, nc = PS.chunks(B)
        assert lib.vlpet_prefix_concat_chunks(B) == nc
        assert 1 <= nc <= PS.MAX_CHUNKS and (nc - 1) * cs < B <= nc * cs          # every chunk holds an item, all items are held
        assert lib.vlpet_prefix_concat_ws_bytes(B, 40, 768) == nc * 40 * 768 * 4
    assert (PS.chunks(33), PS.chunks(64), PS.chunks(500)) == ((2, 17), (2, 32), (16, 32))
    assert lib.vlpet_prefix_concat_chunks(0) == 0 and lib.vlpet_prefix_concat_chunks(-3) == 0
    assert lib.vlpet_prefix_concat_ws_bytes(0, 40, 768) == 0 and lib.vlpet_prefix_concat_ws_bytes(4, 0, 768) == 0
    assert lib.vlpet_prefix_concat_ws_bytes(4, 40, -8) == 0


def test_forward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name in ("pre", "a", "v", "x"):
        assert _fwd(lib, **{name: None}) == E_NULL, name
    for name in ("B", "P", "La", "Lv", "d"):
        assert _fwd(lib, **{name: 0}) == E_SHAPE and _fwd(lib, **{name: -2}) == E_SHAPE, name
    assert _fwd(lib, d=60) == E_SHAPE and _fwd(lib, d=4) == E_SHAPE
    assert _fwd(lib, p=1.0) == E_SHAPE and _fwd(lib, p=-0.1) == E_SHAPE and _fwd(lib, p=float("nan")) == E_SHAPE
    assert _fwd(lib, dt=7) == E_DTYPE and _fwd(lib, dt=-1) == E_DTYPE
    for name, base in (("pre", A), ("a", 2 * A), ("v", 3 * A), ("x", 1 << 30)):
        assert _fwd(lib, **{name: base + 8}) == E_ALIGN, name
    assert _fwd(lib, pre=None, d=60) == E_NULL           # the order of the neighbouring entry points: NULL, shape, dtype, alignment
    assert _fwd(lib, d=60, dt=7) == E_SHAPE and _fwd(lib, dt=7, x=(1 << 30) + 8) == E_DTYPE


def test_backward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert _bwd(lib, dx=None) == E_NULL
    assert _bwd(lib, dpre=None, da=None, dv=None, ws=None) == E_NULL          # nothing wanted
    assert _bwd(lib, dpre=None, da=None, dv=None) == E_NULL
    assert _bwd(lib, ws=None) == E_NULL                                       # dpre wanted, no workspace
    assert _bwd(lib, ws=None, da=None, dv=None) == E_NULL
    assert _bwd(lib, dpre=None) == E_SHAPE                                    # a workspace without the output it serves
    for name in ("B", "P", "La", "Lv", "d"):
        assert _bwd(lib, **{name: 0}) == E_SHAPE and _bwd(lib, **{name: -2}) == E_SHAPE, name
    assert _bwd(lib, d=60) == E_SHAPE
    assert _bwd(lib, p=1.0) == E_SHAPE and _bwd(lib, p=-0.1) == E_SHAPE
    assert _bwd(lib, dt=7) == E_DTYPE
    for name, base in (("dx", 1 << 30), ("dpre", A), ("da", 2 * A), ("dv", 3 * A), ("ws", 1 << 20)):
        assert _bwd(lib, **{name: base + 8}) == E_ALIGN, name
    # an output that is not wanted is not checked for alignment either: the remaining ones still are
    assert _bwd(lib, dpre=None, ws=None, da=2 * A + 8) == E_ALIGN and _bwd(lib, da=None, dv=3 * A + 4) == E_ALIGN


def test_python_entry_point_composes_on_cpu_tensors_and_the_switch_exists():
    import torch
    import vlpet_amd.act as ACT
    assert ACT.FUSE_PREFIX_CONCAT in (True, False) and ACT.FUSE_CONCAT_DROPOUT in (True, False)
    pre, a, v = torch.randn(3, 8), torch.randn(2, 4, 8), torch.randn(2, 1, 8)
    x = ACT.prefix_concat_dropout(pre, a, v, 0.5, training=False)
    assert torch.equal(x, torch.cat([pre.expand(2, -1, -1), a, v], 1))
