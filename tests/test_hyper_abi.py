"""vlpet_hyper_gen_fwd / _bwd / vlpet_hyper_gen_workspace_bytes (csrc/hyper.hip, include/vlpet_hip.h) without a GPU: the symbols and
their ctypes signatures, the version bump, the workspace size, every argument error as a negative code before any launch in the
header's order (NULL, DTYPE, SHAPE, ALIGN, WORKSPACE, ALIAS), and the Python entry points' refusal of CPU tensors."""
import ctypes

import pytest
import torch

A = 1 << 24         # 16-byte aligned non-NULL values, far enough apart not to overlap: every call below returns before a dereference
E_SHAPE, E_RANK, E_ALIGN, E_WORKSPACE, E_NULL, E_DTYPE, E_ALIAS = -1, -2, -3, -4, -5, -6, -7
N_BART = [73728, 96, 73728, 768] * 3            # one stack of BART-base with cross-attention: (down w, down b, up w, up b) x 3 blocks


def _tab(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


class Call:
    """one well-formed argument set; ``over`` replaces named scalars / tables, ``entry`` one entry of a table: {"G": (2, value)}"""

    def __init__(self, n=(512, 8, 64, 8), E=2, P=8, pdt=0):
        self.n, self.E, self.P, self.pdt = list(n), E, P, pdt
        S, k = len(self.n), [0]

        def nxt():
            k[0] += 1
            return k[0] * A
        self.G, self.g, self.out = [nxt() for _ in range(S)], [nxt() for _ in range(S)], [nxt() for _ in range(S)]
        self.dG, self.dg = [nxt() for _ in range(S)], [nxt() for _ in range(S)]
        self.dout = [nxt() for _ in range(S * E)]
        self.e, self.de, self.ws = nxt(), nxt(), nxt()

    def _args(self, over, entry):
        v = dict(S=len(self.n), n=list(self.n), E=self.E, P=self.P, pdt=self.pdt, e=self.e, de=self.de, ws=self.ws, ws_bytes=None,
                 G=list(self.G), g=list(self.g), out=list(self.out), dG=list(self.dG), dg=list(self.dg), dout=list(self.dout))
        v.update(over)
        for name, (i, val) in (entry or {}).items():
            v[name][i] = val
        for name in ("G", "g", "out", "dG", "dg", "dout"):
            v[name] = None if v[name] is None else _tab(v[name])
        v["n"] = None if v["n"] is None else _ints(v["n"])
        return v

    def fwd(self, lib, entry=None, **over):
        v = self._args(over, entry)
        return lib.vlpet_hyper_gen_fwd(v["S"], v["G"], v["g"], v["n"], v["e"], v["E"], v["P"], v["out"], v["pdt"], None)

    def bwd(self, lib, entry=None, **over):
        v = self._args(over, entry)
        if v["ws_bytes"] is None:
            v["ws_bytes"] = (lib.vlpet_hyper_gen_workspace_bytes(v["S"], v["n"], v["E"], v["P"]) if v["n"] is not None else 0) or 1 << 20
        return lib.vlpet_hyper_gen_bwd(v["S"], v["dout"], v["G"], v["n"], v["e"], v["E"], v["P"], v["dG"], v["dg"], v["de"], v["ws"],
                                       v["ws_bytes"], v["pdt"], None)


def _ws(lib, n, E, P):
    return lib.vlpet_hyper_gen_workspace_bytes(len(n), _ints(n), E, P)


def test_symbols_signatures_and_version():
    from vlpet_amd import _lib
    lib = _lib.load()
    for name, n in (("vlpet_hyper_gen_fwd", 10), ("vlpet_hyper_gen_bwd", 14), ("vlpet_hyper_gen_workspace_bytes", 4)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n
    assert lib.vlpet_version() > 680                    # the parent's


def test_header_declares_the_three_entry_points_and_their_error_order():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlpet_hip.h")).read()
    for name in ("vlpet_hyper_gen_fwd", "vlpet_hyper_gen_bwd", "vlpet_hyper_gen_workspace_bytes"):
        assert text.count(name + "(") >= 1 and text.count(name) >= 2, name              # the declaration and the description
    doc = text[text.index("Hyperformer:"):]
    order = [doc.index(k) for k in ("VLPET_E_NULL", "VLPET_E_DTYPE", "VLPET_E_SHAPE", "VLPET_E_ALIGN", "VLPET_E_WORKSPACE", "VLPET_E_ALIAS")]
    assert order == sorted(order)


def test_workspace_is_positive_and_monotone_in_rows_and_sizes():
    from vlpet_amd import _lib
    lib = _lib.load()
    for n, P in ((N_BART, 8), ([512, 8, 512, 64], 8), ([192, 3, 1], 5), ([73728, 96, 73728, 768], 64)):
        S = len(n)
        sizes = [_ws(lib, n, E, P) for E in range(1, min(64, 256 // S) + 1)]
        assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    grow = [_ws(lib, [k, 96, k, 768], 6, 8) for k in (1, 255, 256, 257, 4096, 73728, 1 << 20)]
    assert grow == sorted(grow) and grow[-1] > grow[0], grow
    more_maps = [_ws(lib, N_BART[:S], 6, 8) for S in range(1, 13)]
    assert more_maps == sorted(more_maps) and len(set(more_maps)) > 6
    # at least one [E, P] block of floats per 256 rows of every map
    assert _ws(lib, N_BART, 6, 8) >= 3 * (2 * 288 + 1 + 3) * 6 * 8 * 4
    for n, E, P in ((N_BART, 0, 8), (N_BART, 65, 8), (N_BART, 6, 0), (N_BART, 6, 65), ([], 6, 8), ([8] * 17, 6, 8), ([8, 0], 6, 8),
                    ([8, -4], 6, 8), ([8] * 16, 17, 8)):
        assert _ws(lib, n, E, P) == 0, (n, E, P)
    assert lib.vlpet_hyper_gen_workspace_bytes(4, None, 6, 8) == 0


def test_forward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    c = Call()
    for name in ("G", "g", "n", "e", "out"):
        assert c.fwd(lib, **{name: None}) == E_NULL, name
    for name in ("G", "g", "out"):
        for i in range(4):
            assert c.fwd(lib, entry={name: (i, None)}) == E_NULL, (name, i)
    assert c.fwd(lib, pdt=2) == E_DTYPE and c.fwd(lib, pdt=-1) == E_DTYPE
    for over in (dict(S=0), dict(S=17), dict(S=-1), dict(E=0), dict(E=65), dict(P=0), dict(P=65), dict(n=[512, 0, 64, 8]),
                 dict(n=[512, 8, -64, 8])):
        assert c.fwd(lib, **over) == E_SHAPE, over
    wide = Call(n=[8] * 16, E=17)                             # S * E = 272 row pointers: more than the kernel arguments carry
    assert wide.fwd(lib) == E_SHAPE and wide.bwd(lib) == E_SHAPE and Call(n=[8] * 16, E=16).fwd(lib, e=None) == E_NULL
    assert c.fwd(lib, e=c.e + 8) == E_ALIGN
    for name in ("G", "g", "out"):
        for i in range(4):
            assert c.fwd(lib, entry={name: (i, getattr(c, name)[i] + 8)}) == E_ALIGN, (name, i)
    for i in range(4):
        for inp in (c.G[0], c.g[3], c.e, c.G[i], c.g[i]):
            assert c.fwd(lib, entry={"out": (i, inp)}) == E_ALIAS, (i, inp)
    # overlapping by its last 16 bytes only; two outputs (out[0]: [2, 512] fp32 = 4,096 bytes)
    assert c.fwd(lib, entry={"out": (0, c.e - 4096 + 16)}) == E_ALIAS
    assert c.fwd(lib, entry={"out": (1, c.out[0] + 4096 - 16)}) == E_ALIAS
    # the order of the header: a NULL wins over a bad dtype, the dtype over the shape, the shape over alignment, alignment over aliasing
    assert c.fwd(lib, e=None, pdt=9, E=0) == E_NULL and c.fwd(lib, pdt=9, E=0) == E_DTYPE
    assert c.fwd(lib, E=0, e=c.e + 8) == E_SHAPE and c.fwd(lib, e=c.e + 8, entry={"out": (0, c.G[0])}) == E_ALIGN


def test_backward_argument_errors_come_back_before_any_launch():
    from vlpet_amd import _lib
    lib = _lib.load()
    c = Call()
    for name in ("dout", "G", "n", "e", "dG", "dg", "de", "ws"):
        assert c.bwd(lib, **{name: None}) == E_NULL, name
    for name in ("G", "dG", "dg"):
        for i in range(4):
            assert c.bwd(lib, entry={name: (i, None)}) == E_NULL, (name, i)
    assert c.bwd(lib, pdt=5) == E_DTYPE
    for over in (dict(S=0), dict(S=17), dict(E=0), dict(E=65), dict(P=0), dict(P=65), dict(n=[512, 8, 64, 0])):
        assert c.bwd(lib, **over) == E_SHAPE, over
    for name in ("e", "de", "ws"):
        assert c.bwd(lib, **{name: getattr(c, name) + 8}) == E_ALIGN, name
    for name in ("G", "dG", "dg"):
        for i in range(4):
            assert c.bwd(lib, entry={name: (i, getattr(c, name)[i] + 4)}) == E_ALIGN, (name, i)
    assert c.bwd(lib, entry={"dout": (5, c.dout[5] + 2)}) == E_ALIGN          # a row of dout: 4 bytes
    need = _ws(lib, c.n, c.E, c.P)
    assert need > 0 and c.bwd(lib, ws_bytes=need - 1) == E_WORKSPACE and c.bwd(lib, ws_bytes=0) == E_WORKSPACE
    for out in ("dG", "dg"):
        for i in range(4):
            for inp in (c.dout[0], c.dout[7], c.G[0], c.G[3], c.e):
                assert c.bwd(lib, entry={out: (i, inp)}) == E_ALIAS, (out, i, inp)
    for out in ("de", "ws"):
        for inp in (c.dout[0], c.dout[7], c.G[0], c.G[3], c.e, c.dG[2], c.dg[1]):
            assert c.bwd(lib, **{out: inp}) == E_ALIAS, (out, inp)
    assert c.bwd(lib, ws=c.de) == E_ALIAS and c.bwd(lib, entry={"dG": (1, c.dG[0])}) == E_ALIAS
    assert c.bwd(lib, entry={"dg": (2, c.dG[3])}) == E_ALIAS and c.bwd(lib, ws=c.de - need + 16) == E_ALIAS
    # the order of the header
    assert c.bwd(lib, ws=None, pdt=9, E=0) == E_NULL and c.bwd(lib, pdt=9, E=0) == E_DTYPE and c.bwd(lib, E=0, ws=c.ws + 8) == E_SHAPE
    assert c.bwd(lib, ws=c.ws + 8, ws_bytes=0) == E_ALIGN and c.bwd(lib, ws_bytes=0, de=c.e) == E_WORKSPACE


def test_null_rows_of_dout_are_not_an_error():
    """a NULL entry of dout means zeros: the checks pass it (the next check answers: the workspace is too small)"""
    from vlpet_amd import _lib
    lib = _lib.load()
    c = Call()
    assert c.bwd(lib, dout=[None] * 8, ws_bytes=16) == E_WORKSPACE
    assert c.bwd(lib, entry={"dout": (3, None)}, ws_bytes=16) == E_WORKSPACE


def test_python_entry_points_refuse_cpu_tensors_and_count_nothing():
    import vlpet_amd.functional as VF
    assert (VF.HYPER_MAX_MAPS, VF.HYPER_MAX_ROWS, VF.HYPER_MAX_DIM) == (16, 64, 64) and isinstance(VF.HYPER_CALLS, int)
    maps = [(torch.zeros(16, 8), torch.zeros(16)), (torch.zeros(4, 8), torch.zeros(4))]
    e = torch.zeros(2, 8)
    n0 = VF.HYPER_CALLS
    with pytest.raises(RuntimeError):
        VF.hyper_generate(maps, e)
    with pytest.raises(RuntimeError):
        VF.hyper_generate_into(maps, e)
    assert VF.HYPER_CALLS == n0
    assert VF.hyper_applies(12, 6, 8) and VF.hyper_applies(4, 36, 64, torch.bfloat16) and VF.hyper_applies(16, 16, 64)
    assert not VF.hyper_applies(17, 1, 8) and not VF.hyper_applies(1, 65, 8) and not VF.hyper_applies(1, 1, 65)
    assert not VF.hyper_applies(16, 17, 8) and not VF.hyper_applies(4, 6, 8, torch.float16)
