"""The C-ABI library loads on a CPU-only box and exports every symbol include/vlpet_hip.h declares;
argument errors come back as negative codes (no compute is launched without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "vlpet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vlpet_[a-z0-9_]+)\s*\(", txt)))


def test_exports_every_declared_symbol():
    from vlpet_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in vlpet_hip.h but not exported"
    assert set(syms) == set(_lib.SIGNATURES), "ctypes table and header disagree"


def test_no_process_wide_switches_in_the_header():
    """The in-launch reduce is chosen per call (`phases` bit 5) and finalize launches are not queued: the library's only state between
    calls is the dropout seed counter."""
    syms = declared_symbols()
    assert "vlpet_set_in_launch_reduce" not in syms
    assert not [s for s in syms if s.startswith("vlpet_finalize_")]


def test_diagnosis_build_is_not_stale():
    """The experiment-switch tests load vl-pet_amd/lib/libvlpet_hip_dbg.so (a DEBUG=1 build of the same sources) in child processes: if it
    exists it must export what the header declares -- a product rebuild that added an entry point without rebuilding it (__graft_entry__.build()
    does both) made those tests fail at load time on the GPU box, where nothing can be rebuilt."""
    dbg = os.path.join(ROOT, "vl-pet_amd", "lib", "libvlpet_hip_dbg.so")
    if not os.path.exists(dbg):
        pytest.skip("no diagnosis build")
    lib = ctypes.CDLL(dbg)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"stale diagnosis build (run __graft_entry__.build()): {missing}"


def test_error_codes_without_gpu():
    from vlpet_amd import _lib
    lib = _lib.load()
    assert lib.vlpet_version() >= 100
    assert [lib.vlpet_rank_tiles(r) for r in (1, 8, 32, 33, 96, 97, 192)] == [1, 1, 1, 3, 3, 6, 6]
    assert lib.vlpet_rank_tiles(193) == -2 and lib.vlpet_rank_tiles(0) == -1
    # bad shapes / NULL pointers are rejected before any launch
    assert lib.vlpet_adapter_gate_fwd(None, None, None, None, None, 0, 768, 3, 1, 1.0, 1.0, 1.0, 1, None) == -1
    assert lib.vlpet_adapter_gate_fwd(None, None, None, None, None, 16, 100, 3, 1, 1.0, 1.0, 1.0, 1, None) == -1
    assert lib.vlpet_adapter_gate_fwd(None, None, None, None, None, 16, 768, 2, 1, 1.0, 1.0, 1.0, 1, None) == -2
    assert lib.vlpet_adapter_gate_fwd(None, None, None, None, None, 16, 768, 3, 1, 1.0, 1.0, 1.0, 1, None) == -5
    assert lib.vlpet_adapter_gate_fwd(8, 24, 16, 16, 16, 16, 768, 3, 1, 1.0, 1.0, 1.0, 1, None) == -3   # misaligned
    assert lib.vlpet_adapter_gate_fwd(16, 16, 16, 16, 16, 16, 768, 3, 1, 1.0, 1.0, 1.0, 7, None) == -6  # dtype
    assert b"aligned" in lib.vlpet_error_string(-3)
    raw = 4 * (768 // 16 * 3) * 1024 + (96 + 768) * 4
    assert lib.vlpet_packed_bytes(3, 768, 1) == (raw + 255) // 256 * 256
    assert lib.vlpet_bwd_workspace_bytes(28000, 768, 3, 1, 1) > 2 * 28000 * 768 * 2
    # training forms: the saved-activation block is four [M, 32*tiles] IO tensors, each padded to 256 bytes
    assert lib.vlpet_saved_bytes(28000, 3, 1) == 4 * ((28000 * 96 * 2 + 255) // 256 * 256)
    assert lib.vlpet_saved_bytes(10, 3, 0) == 4 * ((10 * 96 * 4 + 255) // 256 * 256)
    assert lib.vlpet_saved_bytes(0, 3, 1) == 0 and lib.vlpet_saved_bytes(16, 2, 1) == 0
    assert lib.vlpet_adapter_gate_fwd_save(16, 16, 16, 16, 16, None, 16, 768, 3, 1, 1.0, 1.0, 1.0, 1, None) == -5   # no block
    assert lib.vlpet_adapter_gate_fwd_save(16, 16, 16, 16, 16, 8, 16, 768, 3, 1, 1.0, 1.0, 1.0, 1, None) == -3      # misaligned block
    assert lib.vlpet_parallel_adapter_fwd_save(16, 16, 16, 16, None, 16, 768, 3, 1.0, 1, None) == -5


def test_product_path_has_no_cpu_fallback():
    import torch
    import vlpet_amd.functional as F
    with pytest.raises(RuntimeError):
        F.pack_pair([torch.zeros(8, 64)], [torch.zeros(8)], torch.zeros(64, 8), torch.zeros(64), 1)
    from vlpet_amd.adapters import AdapterConfig, AdapterController
    ctl = AdapterController(AdapterConfig(tasks=["vqa"], d_model=64, input_dim=64, use_adapter_down_dim=True,
                                          adapter_down_dim=8, use_parallel_adapter=True))
    x = torch.zeros(2, 3, 64)
    with pytest.raises(RuntimeError):
        ctl(x, "vqa", y=x)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "vl-pet_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} mentions the oracle"


def test_lowrank_projector_argument_errors_without_gpu():
    """f4 entry points (include/vlpet_hip.h, LowRankVisualEmbedding): shapes, ranks, NULLs and alignment are rejected
    before any launch; the size queries are pure host arithmetic."""
    from vlpet_amd import _lib
    lib = _lib.load()
    assert lib.vlpet_version() >= 220
    n = lib.vlpet_lowrank_packed_bytes(3, 2048, 768, 1)
    assert n % 256 == 0 and n > (2048 // 16) * 3 * 1024          # at least the feat_dim-wide down fragments
    assert lib.vlpet_lowrank_packed_bytes(3, 2048, 768, 0) > n   # fp32 IO: hi/lo split, twice the fragments
    assert lib.vlpet_lowrank_packed_bytes(6, 2048, 768, 1) == 0 and lib.vlpet_lowrank_packed_bytes(3, 100, 768, 1) == 0
    assert lib.vlpet_lowrank_bwd_workspace_bytes(1024, 2048, 768, 3, 1) > 2 * 1024 * 768 * 2
    assert lib.vlpet_lowrank_bwd_workspace_bytes(0, 2048, 768, 3, 1) == 0
    fwd = lib.vlpet_lowrank_gate_fwd
    assert fwd(None, None, None, None, None, 0, 2048, 768, 3, 0, 1, None) == -1       # M
    assert fwd(None, None, None, None, None, 16, 2000, 768, 3, 0, 1, None) == -1      # feat_dim % 64
    assert fwd(None, None, None, None, None, 16, 2048, 768, 6, 0, 1, None) == -2      # r > 96 has no rows kernel
    assert fwd(None, None, None, None, None, 16, 2048, 768, 3, 0, 7, None) == -6
    assert fwd(None, None, None, None, None, 16, 2048, 768, 3, 0, 1, None) == -5
    assert fwd(16, 16, None, 24, None, 16, 2048, 768, 3, 0, 1, None) == -3            # misaligned output
    bwd = lib.vlpet_lowrank_gate_bwd
    assert bwd(*([None] * 13), 96, 96, None, 0, 16, 2048, 768, 3, 0, 1, None) == -5
    assert bwd(*([16] * 13), 97, 96, 16, 0, 16, 2048, 768, 3, 0, 1, None) == -2       # r beyond the padded rank
    assert bwd(*([16] * 13), 96, 96, 16, 0, 16, 2048, 768, 3, 0, 1, None) == -4       # workspace too small (VLPET_E_WORKSPACE)
    assert lib.vlpet_norm_residual_fwd(None, None, None, None, None, None, None, 16, 768, 1e-5, 1, None) == -5
    assert lib.vlpet_norm_residual_fwd(16, 16, 16, 16, 16, 16, 16, 16, 770, 1e-5, 1, None) == -1
