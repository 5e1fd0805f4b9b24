"""Return codes of the 16 entry points of K1, K2 and K3 (csrc/api.hip), one perturbed argument at a time, without a GPU.

Every row is rejected before a launch: the backward base rows have ``workspace_bytes`` 0 (VLPET_E_WORKSPACE is the last check in
front of the kernels), the forward base rows a misaligned ``out`` (VLPET_E_ALIGN is the last one there), and each perturbation only
makes an earlier check fire.  The expected codes were recorded (``python tests/test_abi_return_codes.py --generate``) from the
library of the commit BEFORE the 16 hand-written preambles were folded into one helper per operator: the fold must not change a code
for any input, the ORDER of the checks included (a NULL ``dbd`` together with ``M = 0`` is VLPET_E_NULL, not VLPET_E_SHAPE).  The test
skips itself where a GPU is present and refuses a table entry that is not an error code: a branch bug must never turn a fake pointer
into a launch."""
import os
import sys

import pytest

E_CODES = {-1: "SHAPE", -2: "RANK", -3: "ALIGN", -4: "WORKSPACE", -5: "NULL", -6: "DTYPE"}

K1_TAIL = "dwd dbd dwu dbu dwgd dbgd dwgu dbgu r rg workspace workspace_bytes M d tiles gate_mode delta_scale x2_scale gate_scale io_dtype stream"
K1_FWD_TAIL = "M d tiles gate_mode delta_scale x2_scale gate_scale io_dtype stream"
K2_TAIL = "dwd dbd dwu dbu r workspace workspace_bytes M d tiles scale io_dtype stream"
K3_TAIL = "da db r workspace workspace_bytes M d tiles scaling io_dtype stream"
ENTRIES = {
    "vlpet_adapter_gate_fwd": "x1 x2 packed_a packed_g out " + K1_FWD_TAIL,
    "vlpet_adapter_gate_fwd_save": "x1 x2 packed_a packed_g out saved " + K1_FWD_TAIL,
    "vlpet_adapter_gate_bwd": "dy x1 x2 packed_a packed_g dx1 dx2 " + K1_TAIL,
    "vlpet_adapter_gate_bwd_phase": "phases dy x1 x2 packed_a packed_g dx1 dx2 " + K1_TAIL,
    "vlpet_adapter_gate_bwd_saved": "phases dy x1 x2 saved packed_a packed_g dx1 dx2 " + K1_TAIL,
    "vlpet_adapter_gate_bwd_saved_acc": "phases dy x1 x2 saved packed_a packed_g dx1_in dx1 dx2 " + K1_TAIL,
    "vlpet_adapter_gate_bwd_saved_y": "phases dy x1 x2 y saved packed_a packed_g dx1_in dx1 dx2 " + K1_TAIL,
    "vlpet_parallel_adapter_fwd": "x y packed out M d tiles scale io_dtype stream",
    "vlpet_parallel_adapter_fwd_save": "x y packed out saved M d tiles scale io_dtype stream",
    "vlpet_parallel_adapter_bwd": "dy x packed dx " + K2_TAIL,
    "vlpet_parallel_adapter_bwd_saved": "dy x saved packed dx " + K2_TAIL,
    "vlpet_lora_delta_fwd": "x base packed keep_mask p seed keep_out out M d tiles scaling io_dtype stream",
    "vlpet_lora_delta_fwd_save": "x base packed keep_mask p seed keep_out out saved M d tiles scaling io_dtype stream",
    "vlpet_lora_delta_fwd_r8": "x base packed keep_mask p seed keep_out out saved M d r scaling io_dtype stream",
    "vlpet_lora_delta_bwd": "dy x packed keep_mask p seed dx " + K3_TAIL,
    "vlpet_lora_delta_bwd_saved": "dy x saved packed keep_mask p seed dx " + K3_TAIL,
}
NUMBERS = dict(phases=3, r=8, rg=8, workspace_bytes=0, M=16, d=256, tiles=1, gate_mode=1, delta_scale=1.0, x2_scale=1.0, gate_scale=1.0,
               scale=1.0, scaling=1.0, io_dtype=1, p=0.1, seed=1)


def base_row(entry):
    names = ENTRIES[entry].split()
    row = {n: NUMBERS.get(n, 16) for n in names}        # every pointer 16
    row["stream"] = None
    if "_fwd" in entry:
        row["out"] = 8                                  # (no workspace to fall back on: the alignment check is the last one)
    return names, row


def perturbations(entry):
    """[(what, {argument: value})] in a fixed order; the first is the base row itself."""
    names, row = base_row(entry)
    out = [("base", {})]
    for n in names:
        if n not in NUMBERS and n != "stream":
            out += [(f"{n}=NULL", {n: None}), (f"{n}=8", {n: 8})]
    out += [("M=0", {"M": 0}), ("d=100", {"d": 100}), ("dtype=7", {"io_dtype": 7})]
    if "tiles" in names:
        out.append(("tiles=2", {"tiles": 2}))
    if "gate_mode" in names:
        out += [(f"gate_mode={g}", {"gate_mode": g}) for g in (0, 2, 3)]
        opt = [n for n in ("y", "dx1_in") if n in names]
        if opt:     # ungated with y / dx1_in (as the base row has them), and without
            out += [("ungated, no " + n, {"gate_mode": 0, n: None}) for n in opt]
            out.append(("ungated, neither", {"gate_mode": 0, **{n: None for n in opt}}))
    if "phases" in names:
        out += [(f"phases={v}", {"phases": v}) for v in (0, 4, 8, 64)]
    for n in ("r", "rg"):
        if n in names:
            out += [(f"{n}=0", {n: 0}), (f"{n}=33", {n: 33})]       # 32 * tiles + 1
    if "p" in names:
        out.append(("p=1.0", {"p": 1.0}))
    if "dx1_in" in names:
        out.append(("dx1_in == dx1", {"dx1_in": 32, "dx1": 32}))
    if "dbd" in names:      # the order of the checks: a NULL bias slot wins over a bad shape, a bad gate mode over both
        out += [("dbd=NULL, M=0", {"dbd": None, "M": 0}), ("dbu=NULL, dtype=7", {"dbu": None, "io_dtype": 7})]
        if "gate_mode" in names:
            out.append(("dbd=NULL, gate_mode=3", {"dbd": None, "gate_mode": 3}))
    if "saved" in names:
        out += [("saved=NULL, M=0", {"saved": None, "M": 0}), ("saved=NULL, p=1.0", {"saved": None, "p": 1.0})] if "p" in names else \
               [("saved=NULL, M=0", {"saved": None, "M": 0})]
    return names, row, out


def codes_of(lib, entry):
    names, row, perts = perturbations(entry)
    fn = getattr(lib, entry)
    return [fn(*[{**row, **change}[n] for n in names]) for _, change in perts]


# entry -> the codes of perturbations(entry), in order
EXPECTED = {
    "vlpet_adapter_gate_fwd": [-3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -1, -1, -6, -2, -3, -3, -1],
    "vlpet_adapter_gate_fwd_save": [-3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -1, -1, -6, -2, -3, -3, -1, -5],
    "vlpet_adapter_gate_bwd": [-4, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -4, -4, -1, -2, -2, -2, -2, -5, -5, -1],
    "vlpet_adapter_gate_bwd_phase": [-4, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -4, -4, -1, -5, -5, -5, -5, -2, -2, -2, -2, -5, -5, -1],
    "vlpet_adapter_gate_bwd_saved": [-4, -5, -3, -5, -3, -5, -3, -5, -4, -5, -3, -5, -3, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -4, -4, -1, -5, -5, -5, -5, -2, -2, -2, -2, -5, -5, -1, -5],
    "vlpet_adapter_gate_bwd_saved_acc": [-4, -5, -3, -5, -3, -5, -3, -5, -4, -5, -3, -5, -3, -5, -4, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -5, -4, -1, -5, -5, -5, -5, -5, -5, -2, -2, -2, -2, -4, -5, -5, -1, -5],
    "vlpet_adapter_gate_bwd_saved_y": [-4, -5, -3, -5, -3, -5, -3, -4, -4, -5, -4, -5, -3, -5, -3, -4, -4, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -5, -4, -1, -5, -5, -5, -5, -5, -5, -5, -2, -2, -2, -2, -4, -5, -5, -1, -5],
    "vlpet_parallel_adapter_fwd": [-3, -5, -3, -5, -3, -5, -3, -5, -3, -1, -1, -6, -2],
    "vlpet_parallel_adapter_fwd_save": [-3, -5, -3, -5, -3, -5, -3, -5, -3, -5, -3, -1, -1, -6, -2, -5],
    "vlpet_parallel_adapter_bwd": [-4, -5, -3, -5, -3, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -2, -2, -5, -5],
    "vlpet_parallel_adapter_bwd_saved": [-4, -5, -3, -5, -3, -5, -4, -5, -3, -5, -3, -5, -4, -5, -4, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -2, -2, -5, -5, -5],
    "vlpet_lora_delta_fwd": [-3, -5, -3, -5, -3, -5, -3, -3, -3, -3, -3, -5, -3, -1, -1, -6, -2, -1],
    "vlpet_lora_delta_fwd_save": [-3, -5, -3, -5, -3, -5, -3, -3, -3, -3, -3, -5, -3, -5, -3, -1, -1, -6, -2, -1, -5, -5],
    "vlpet_lora_delta_fwd_r8": [-3, -5, -3, -5, -3, -5, -3, -3, -3, -3, -3, -5, -3, -3, -3, -1, -1, -6, -1, -1, -3, -1, -3],
    "vlpet_lora_delta_bwd": [-4, -5, -3, -5, -3, -5, -3, -4, -3, -5, -3, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -2, -2, -1],
    "vlpet_lora_delta_bwd_saved": [-4, -5, -3, -5, -3, -5, -4, -5, -3, -4, -3, -5, -3, -5, -4, -5, -4, -5, -3, -1, -1, -6, -2, -2, -2, -1, -5, -5],
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_return_codes(entry):
    import torch
    if torch.cuda.is_available():
        pytest.skip("fake pointers: CPU machines only")
    from vlpet_amd import _lib
    names, row, perts = perturbations(entry)
    want = EXPECTED[entry]
    assert len(want) == len(perts) and len(names) == len(_lib.SIGNATURES[entry][1])
    assert all(c in E_CODES for c in want), "every row must be rejected"
    fn = getattr(_lib.load(), entry)
    for (what, change), code in zip(perts, want):
        got = fn(*[{**row, **change}[n] for n in names])
        assert got == code, f"{entry}, {what}: {E_CODES.get(got, got)} (expected {E_CODES[code]})"


def test_every_check_is_reached():
    """The rows are not vacuous: every code occurs, and the base rows end at the last check."""
    assert {c for v in EXPECTED.values() for c in v} == set(E_CODES)
    for entry, v in EXPECTED.items():
        assert v[0] == (-3 if "_fwd" in entry else -4), entry


if __name__ == "__main__" and "--generate" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    assert not torch.cuda.is_available()
    from vlpet_amd import _lib
    for e in ENTRIES:
        got = codes_of(_lib.load(), e)
        assert all(c in E_CODES for c in got), (e, got)
        print(f'    "{e}": {got},')
