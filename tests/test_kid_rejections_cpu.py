"""The rejections of mogan_poly3_mmd_f64 (csrc/mogan_mmd.hip), as tests/test_fid_rejections_cpu.py does for the moments: every case is
answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that are never dereferenced.
-1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is shown by the answer changing to
MOGAN_ERR_LAUNCH: that case runs only where no GPU is present."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3
OK = dict(Nx=30000, Ny=30000, D=2048, S=100, s=1000, gamma=1.0 / 2048, coef0=1.0)
INF, NAN = float("inf"), float("nan")


def ws_bytes(S, s):
    return int(lib.load().mogan_poly3_mmd_ws_bytes(S, s))


def mmd(x=PTR, y=PTR, ix=PTR, iy=PTR, sums=PTR, ws=PTR, ws_size=None, **dims):
    d = dict(OK, **dims)
    if ws_size is None:
        ws_size = max(ws_bytes(d["S"], d["s"]), 1 << 20)
    return lib.load().mogan_poly3_mmd_f64(x, d["Nx"], y, d["Ny"], d["D"], ix, iy, d["S"], d["s"], d["gamma"], d["coef0"], sums, ws,
                                          ws_size, NULL)


SHAPE_CASES = [
    ("NULL x", dict(x=NULL)), ("NULL y", dict(y=NULL)), ("NULL ix", dict(ix=NULL)), ("NULL iy", dict(iy=NULL)),
    ("NULL sums", dict(sums=NULL)),
    ("S = 0", dict(S=0)), ("S < 0", dict(S=-1)), ("S = 65536", dict(S=65536)), ("S = 2^30", dict(S=1 << 30)),
    ("s = 1", dict(s=1)), ("s = 0", dict(s=0)), ("s < 0", dict(s=-1000)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("Nx = 0", dict(Nx=0)), ("Nx < 0", dict(Nx=-3)), ("Ny = 0", dict(Ny=0)), ("Ny < 0", dict(Ny=-3)),
    ("Nx = 2^31", dict(Nx=1 << 31)), ("Ny = 2^40", dict(Ny=1 << 40)),
    ("gamma = inf", dict(gamma=INF)), ("gamma = -inf", dict(gamma=-INF)), ("gamma = nan", dict(gamma=NAN)),
    ("coef0 = inf", dict(coef0=INF)), ("coef0 = nan", dict(coef0=NAN)),
    ("a bad shape with a NULL workspace is a shape error", dict(s=1, ws=NULL, ws_size=0)),
]
WS_CASES = [
    ("NULL ws", dict(ws=NULL)), ("NULL ws of size 0", dict(ws=NULL, ws_size=0)), ("size 0", dict(ws_size=0)),
    ("misaligned ws", dict(ws=ctypes.c_void_p(260))),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in SHAPE_CASES], ids=[c[0] for c in SHAPE_CASES])
def test_rejects_shapes_before_any_launch(kw):
    assert mmd(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in WS_CASES], ids=[c[0] for c in WS_CASES])
def test_rejects_a_missing_workspace_before_any_launch(kw):
    assert mmd(**kw) == WS


def test_rejects_a_short_workspace_before_any_launch():
    need = ws_bytes(OK["S"], OK["s"])
    assert need == 100 * 528 * 8                                    # T = 16: T (T + 1) + T^2 = 528 tiles per subset pair
    assert mmd(ws_size=need - 1) == WS and mmd(ws_size=8) == WS
    assert mmd(S=1, s=2, Nx=2, Ny=2, D=1, ws_size=ws_bytes(1, 2) - 1) == WS


def test_the_signatures_are_the_headers():
    assert lib.SIGNATURES["mogan_poly3_mmd_ws_bytes"] == [lib.I, lib.I]
    assert lib.SIGNATURES["mogan_poly3_mmd_f64"] == [lib.P, lib.L, lib.P, lib.L, lib.I, lib.P, lib.P, lib.I, lib.I,
                                                     ctypes.c_double, ctypes.c_double, lib.P, lib.P, lib.Z, lib.P]
    assert lib.load().mogan_poly3_mmd_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_is_positive_and_monotone():
    sizes = [2, 3, 63, 64, 65, 128, 129, 1000, 4096]
    counts = [1, 2, 3, 100, 65535]
    table = [[ws_bytes(S, s) for s in sizes] for S in counts]
    for row in table:
        assert all(v > 0 for v in row) and all(a <= b for a, b in zip(row, row[1:]))
        assert row[0] == row[1] == row[2] == row[3] < row[4]          # one tile row up to s = 64
    for lo, hi in zip(table, table[1:]):
        assert all(a < b for a, b in zip(lo, hi))
    assert ws_bytes(1, 2) == 3 * 8 and ws_bytes(1, 65) == 10 * 8 and ws_bytes(100, 1000) == 100 * 528 * 8


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_both_gates():
    """the limits themselves and the smallest legal problem: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the launch
    itself is what fails"""
    assert mmd() == LAUNCH
    assert mmd(S=65535) == LAUNCH and mmd(D=65536) == LAUNCH
    assert mmd(Nx=(1 << 31) - 1, Ny=(1 << 31) - 1) == LAUNCH
    assert mmd(S=1, s=2, D=1, Nx=1, Ny=1) == LAUNCH
    assert mmd(ws_size=ws_bytes(OK["S"], OK["s"])) == LAUNCH
    assert mmd(gamma=0.0, coef0=-1.0) == LAUNCH
