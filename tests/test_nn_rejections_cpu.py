"""The rejections of mogan_knn_cross_f64 (csrc/mogan_knn.hip), as tests/test_prdc_rejections_cpu.py does for its neighbours: every
case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that are never
dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is shown by the answer
changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  The size query is held to its closed form."""
import ctypes

import pytest
import torch

import nn_cases as C
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3
OK = dict(M=30000, N=80000, D=2048, K=5)
BIG = (1 << 31) - 1


def cross_ws(M, N, K):
    return int(lib.load().mogan_knn_cross_ws_bytes(M, N, K))


def cross(q=PTR, p=PTR, d2=PTR, idx=PTR, ws=PTR, ws_size=None, **dims):
    d = dict(OK, **dims)
    if ws_size is None:
        ws_size = max(cross_ws(d["M"], d["N"], d["K"]), 1 << 20)
    return lib.load().mogan_knn_cross_f64(q, d["M"], p, d["N"], d["D"], d["K"], d2, idx, ws, ws_size, NULL)


SHAPE_CASES = [
    ("NULL q", dict(q=NULL)), ("NULL p", dict(p=NULL)), ("NULL d2", dict(d2=NULL)), ("NULL idx", dict(idx=NULL)),
    ("K = 0", dict(K=0)), ("K < 0", dict(K=-3)), ("K = 9", dict(K=9)), ("K = 2^30", dict(K=1 << 30)),
    ("N = K - 1", dict(N=4)), ("N = 0", dict(N=0, K=1)), ("N < 0", dict(N=-7)),
    ("M = 0", dict(M=0)), ("M < 0", dict(M=-3)),
    ("M = 2^31", dict(M=1 << 31)), ("N = 2^31", dict(N=1 << 31)), ("M = 2^40", dict(M=1 << 40)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("a bad shape with a NULL workspace is a shape error", dict(K=0, ws=NULL, ws_size=0)),
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
    assert cross(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in WS_CASES], ids=[c[0] for c in WS_CASES])
def test_rejects_a_missing_workspace_before_any_launch(kw):
    assert cross(**kw) == WS


def test_rejects_a_short_workspace_before_any_launch():
    need = cross_ws(30000, 80000, 5)
    assert need == 8 * (30000 + 80000 + 2 * 30000 * 5) + 4 * 2 * 30000 * 5          # 469 stripes: two shares of the support tiles
    assert cross(ws_size=need - 1) == WS and cross(ws_size=8) == WS
    assert cross(M=1, N=1, D=1, K=1, ws_size=cross_ws(1, 1, 1) - 1) == WS
    assert cross(M=3, N=1100, D=8, K=8, ws_size=cross_ws(3, 1100, 8) - 1) == WS


def test_the_signatures_are_the_headers():
    assert lib.SIGNATURES["mogan_knn_cross_ws_bytes"] == [lib.L, lib.L, lib.I]
    assert lib.SIGNATURES["mogan_knn_cross_f64"] == [lib.P, lib.L, lib.P, lib.L, lib.I, lib.I, lib.P, lib.P, lib.P, lib.Z, lib.P]
    assert lib.load().mogan_knn_cross_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_follow_the_closed_form_and_are_0_for_illegal_arguments():
    for M, N in ((1, 1), (1, 8), (64, 64), (100, 67), (67, 100), (200, 130), (9, 200), (3, 1100), (30000, 80000), (12, 30000),
                 (30000, 12), (32768, 80000), (32769, 80000), (BIG, 8), (8, BIG), (BIG, BIG)):
        for K in (1, 3, 5, 8):
            if N >= K:
                lists = C.shares(M, N) * M * K
                assert cross_ws(M, N, K) == 8 * (M + N + lists) + (4 * lists + 7) // 8 * 8 == C.ws_bytes(M, N, K), (M, N, K)
            else:
                assert cross_ws(M, N, K) == 0
    assert cross_ws(1, 1, 1) == 32 and cross_ws(1, 3, 3) % 8 == 0 and cross_ws(1, 3, 3) == 8 * (1 + 3 + 3) + 16
    for M, N, K in ((0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, -1, 1), (5, 5, 0), (5, 5, 9), (5, 5, -2), (5, 4, 5), (1 << 31, 5, 1),
                    (5, 1 << 31, 1), (1 << 40, 5, 1)):
        assert cross_ws(M, N, K) == 0, (M, N, K)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_both_gates():
    """the limits themselves and the smallest legal problem: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the launch
    itself is what fails"""
    assert cross() == LAUNCH and cross(K=8) == LAUNCH and cross(K=1) == LAUNCH and cross(D=65536) == LAUNCH and cross(D=1) == LAUNCH
    assert cross(N=5) == LAUNCH and cross(M=1, N=1, D=1, K=1) == LAUNCH and cross(N=8, K=8) == LAUNCH
    assert cross(M=BIG, N=BIG, ws_size=cross_ws(BIG, BIG, 5)) == LAUNCH
    assert cross(ws_size=cross_ws(30000, 80000, 5)) == LAUNCH
