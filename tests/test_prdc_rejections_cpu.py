"""The rejections of mogan_knn_sqdist_f64 and mogan_ball_count_f64 (csrc/mogan_knn.hip), as tests/test_kid_rejections_cpu.py does for
the KID sums: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that
are never dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is shown by the
answer changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  The size queries are held to their closed forms."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3
KNN_OK = dict(N=30000, D=2048, K=5)
BALL_OK = dict(M=30000, N=30000, D=2048, R=2, side=0)
BIG = (1 << 31) - 1


def shares(rows, cols):
    """the closed form of the split of the column tiles: min(ceil(512 / Tr), Tc, 64)"""
    tr, tc = (rows + 63) // 64, (cols + 63) // 64
    return max(1, min(-(-512 // tr), tc, 64))


def knn_ws(N, K):
    return int(lib.load().mogan_knn_sqdist_ws_bytes(N, K))


def ball_ws(M, N, R):
    return int(lib.load().mogan_ball_count_ws_bytes(M, N, R))


def knn(x=PTR, out=PTR, ws=PTR, ws_size=None, **dims):
    d = dict(KNN_OK, **dims)
    if ws_size is None:
        ws_size = max(knn_ws(d["N"], d["K"]), 1 << 20)
    return lib.load().mogan_knn_sqdist_f64(x, d["N"], d["D"], d["K"], out, ws, ws_size, NULL)


def ball(q=PTR, p=PTR, r2=PTR, count=PTR, ws=PTR, ws_size=None, **dims):
    d = dict(BALL_OK, **dims)
    if ws_size is None:
        ws_size = max(ball_ws(d["M"], d["N"], d["R"]), 1 << 20)
    return lib.load().mogan_ball_count_f64(q, d["M"], p, d["N"], d["D"], r2, d["R"], d["side"], count, ws, ws_size, NULL)


KNN_SHAPE = [
    ("NULL x", dict(x=NULL)), ("NULL out", dict(out=NULL)),
    ("K = 0", dict(K=0)), ("K < 0", dict(K=-3)), ("K = 9", dict(K=9)), ("K = 2^30", dict(K=1 << 30)),
    ("N = K", dict(N=5)), ("N = 1", dict(N=1, K=1)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-7)),
    ("N = 2^31", dict(N=1 << 31)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("a bad shape with a NULL workspace is a shape error", dict(K=0, ws=NULL, ws_size=0)),
]
BALL_SHAPE = [
    ("NULL q", dict(q=NULL)), ("NULL p", dict(p=NULL)), ("NULL r2", dict(r2=NULL)), ("NULL count", dict(count=NULL)),
    ("R = 0", dict(R=0)), ("R < 0", dict(R=-1)), ("R = 5", dict(R=5)), ("R = 2^30", dict(R=1 << 30)),
    ("M = 0", dict(M=0)), ("M < 0", dict(M=-3)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-3)),
    ("M = 2^31", dict(M=1 << 31)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("side = 2", dict(side=2)), ("side = -1", dict(side=-1)), ("side = 256", dict(side=256)),
    ("a bad shape with a NULL workspace is a shape error", dict(side=2, ws=NULL, ws_size=0)),
]
WS_CASES = [
    ("NULL ws", dict(ws=NULL)), ("NULL ws of size 0", dict(ws=NULL, ws_size=0)), ("size 0", dict(ws_size=0)),
    ("misaligned ws", dict(ws=ctypes.c_void_p(260))),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in KNN_SHAPE], ids=[c[0] for c in KNN_SHAPE])
def test_knn_rejects_shapes_before_any_launch(kw):
    assert knn(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in BALL_SHAPE], ids=[c[0] for c in BALL_SHAPE])
def test_ball_rejects_shapes_before_any_launch(kw):
    assert ball(**kw) == SHAPE


@pytest.mark.parametrize("fn", [knn, ball], ids=["knn", "ball"])
@pytest.mark.parametrize("kw", [c[1] for c in WS_CASES], ids=[c[0] for c in WS_CASES])
def test_rejects_a_missing_workspace_before_any_launch(fn, kw):
    assert fn(**kw) == WS


def test_rejects_a_short_workspace_before_any_launch():
    need = knn_ws(30000, 5)
    assert need == 8 * (30000 + 2 * 30000 * 5)                      # 469 stripes: two shares of the column tiles
    assert knn(ws_size=need - 1) == WS and knn(ws_size=8) == WS
    assert knn(N=2, K=1, D=1, ws_size=knn_ws(2, 1) - 1) == WS
    need = ball_ws(30000, 30000, 2)
    assert need == 8 * 60000 + 4 * 2 * 30000 * 2
    assert ball(ws_size=need - 1) == WS and ball(ws_size=8) == WS
    assert ball(M=1, N=1, D=1, R=1, ws_size=ball_ws(1, 1, 1) - 1) == WS


def test_the_signatures_are_the_headers():
    assert lib.SIGNATURES["mogan_knn_sqdist_ws_bytes"] == [lib.L, lib.I]
    assert lib.SIGNATURES["mogan_knn_sqdist_f64"] == [lib.P, lib.L, lib.I, lib.I, lib.P, lib.P, lib.Z, lib.P]
    assert lib.SIGNATURES["mogan_ball_count_ws_bytes"] == [lib.L, lib.L, lib.I]
    assert lib.SIGNATURES["mogan_ball_count_f64"] == [lib.P, lib.L, lib.P, lib.L, lib.I, lib.P, lib.I, lib.I, lib.P, lib.P, lib.Z,
                                                      lib.P]
    assert lib.load().mogan_knn_sqdist_ws_bytes.restype is ctypes.c_size_t
    assert lib.load().mogan_ball_count_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_follow_their_closed_forms_and_are_0_for_illegal_arguments():
    for N in (2, 9, 64, 65, 67, 96, 130, 1000, 4096, 30000, 32768, 32769, 100000, BIG):
        for K in (1, 3, 5, 8):
            if N >= K + 1:
                assert knn_ws(N, K) == 8 * (N + shares(N, N) * N * K), (N, K)
            else:
                assert knn_ws(N, K) == 0
    for M, N in ((1, 1), (1, 2), (64, 64), (100, 67), (67, 100), (200, 130), (30000, 30000), (12, 30000), (30000, 12), (BIG, 3),
                 (3, BIG)):
        for R in (1, 2, 3, 4):
            part = 4 * shares(M, N) * M * R
            assert ball_ws(M, N, R) == 8 * (M + N) + (part + 7) // 8 * 8, (M, N, R)
    assert shares(30000, 30000) == 2 and shares(64, 64) == 1 and shares(130, 130) == 3 and shares(12, 30000) == 64
    for N, K in ((5, 0), (5, -1), (5, 9), (5, 5), (1, 1), (0, 1), (-4, 1), (1 << 31, 3), (1 << 40, 3)):
        assert knn_ws(N, K) == 0, (N, K)
    for M, N, R in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -1, 1), (5, 5, 0), (5, 5, 5), (5, 5, -2), (1 << 31, 5, 1), (5, 1 << 31, 1)):
        assert ball_ws(M, N, R) == 0, (M, N, R)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_both_gates():
    """the limits themselves and the smallest legal problems: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the
    launch itself is what fails"""
    assert knn() == LAUNCH and ball() == LAUNCH and ball(side=1) == LAUNCH
    assert knn(K=8) == LAUNCH and knn(K=1) == LAUNCH and knn(D=65536) == LAUNCH and knn(D=1) == LAUNCH
    assert knn(N=9, K=8) == LAUNCH and knn(N=2, K=1, D=1) == LAUNCH
    assert knn(N=BIG, ws_size=knn_ws(BIG, 5)) == LAUNCH
    assert knn(ws_size=knn_ws(30000, 5)) == LAUNCH
    assert ball(R=4) == LAUNCH and ball(R=1) == LAUNCH and ball(D=65536) == LAUNCH
    assert ball(M=1, N=1, D=1, R=1) == LAUNCH
    assert ball(M=BIG, N=BIG, ws_size=ball_ws(BIG, BIG, 2)) == LAUNCH
    assert ball(ws_size=ball_ws(30000, 30000, 2)) == LAUNCH
