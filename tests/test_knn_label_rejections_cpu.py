"""The rejections of mogan_knn_label_f64 (csrc/mogan_knn.hip), as tests/test_nn_rejections_cpu.py does for
mogan_knn_cross_f64: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are
dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is
shown by the answer changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  The size query is held to its
closed form: mogan_knn_cross_ws_bytes plus 24 bytes per share and query."""
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
OK = dict(M=30000, N=150000, D=256, K=5)
BIG = (1 << 31) - 1
POINTERS = ("q", "qlabel", "p", "plabel", "d2", "idx", "same_d2", "same_idx", "other_d2", "other_idx")


def label_ws(M, N, K):
    return int(lib.load().mogan_knn_label_ws_bytes(M, N, K))


def closed_form(M, N, K):
    return C.ws_bytes(M, N, K) + 24 * C.shares(M, N) * M


def label(ws=PTR, ws_size=None, **kw):
    d = dict(OK, **{k: v for k, v in kw.items() if k in OK})
    ptrs = {name: kw.get(name, PTR) for name in POINTERS}
    if ws_size is None:
        ws_size = max(label_ws(d["M"], d["N"], d["K"]), 1 << 20)
    return lib.load().mogan_knn_label_f64(ptrs["q"], ptrs["qlabel"], d["M"], ptrs["p"], ptrs["plabel"], d["N"], d["D"], d["K"],
                                          ptrs["d2"], ptrs["idx"], ptrs["same_d2"], ptrs["same_idx"], ptrs["other_d2"],
                                          ptrs["other_idx"], ws, ws_size, NULL)


SHAPE_CASES = [("NULL %s" % name, {name: NULL}) for name in POINTERS] + [
    ("K = 0", dict(K=0)), ("K < 0", dict(K=-3)), ("K = 9", dict(K=9)), ("K = 2^30", dict(K=1 << 30)),
    ("N = K - 1", dict(N=4)), ("N = 0", dict(N=0, K=1)), ("N < 0", dict(N=-7)),
    ("M = 0", dict(M=0)), ("M < 0", dict(M=-3)),
    ("M = 2^31", dict(M=1 << 31)), ("N = 2^31", dict(N=1 << 31)), ("M = 2^40", dict(M=1 << 40)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-256)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("a bad shape with a NULL workspace is a shape error", dict(K=0, ws=NULL, ws_size=0)),
    ("a NULL label with a NULL workspace is a shape error", dict(plabel=NULL, ws=NULL, ws_size=0)),
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
    assert label(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in WS_CASES], ids=[c[0] for c in WS_CASES])
def test_rejects_a_missing_workspace_before_any_launch(kw):
    assert label(**kw) == WS


def test_rejects_a_short_workspace_before_any_launch():
    need = label_ws(30000, 150000, 5)
    lists = 2 * 30000 * 5                                             # 469 stripes: two shares of the support tiles
    assert need == 8 * (30000 + 150000 + lists) + 4 * lists + 24 * 2 * 30000
    assert label(ws_size=need - 1) == WS and label(ws_size=8) == WS
    # the workspace of mogan_knn_cross_f64 for the same problem is too short: the label pairs come after it
    assert label(ws_size=int(lib.load().mogan_knn_cross_ws_bytes(30000, 150000, 5))) == WS
    assert label(M=1, N=1, D=1, K=1, ws_size=label_ws(1, 1, 1) - 1) == WS
    assert label(M=3, N=1100, D=8, K=8, ws_size=label_ws(3, 1100, 8) - 1) == WS


def test_the_signatures_are_the_headers():
    P, L, I, Z = lib.P, lib.L, lib.I, lib.Z
    assert lib.SIGNATURES["mogan_knn_label_ws_bytes"] == [L, L, I]
    assert lib.SIGNATURES["mogan_knn_label_f64"] == [P, P, L, P, P, L, I, I, P, P, P, P, P, P, P, Z, P]
    assert lib.load().mogan_knn_label_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_follow_the_closed_form_and_are_0_for_illegal_arguments():
    for M, N in ((1, 1), (1, 8), (64, 64), (70, 130), (70, 200), (1, 200), (3, 1100), (30000, 150000), (12, 30000), (30000, 12),
                 (32768, 80000), (32769, 80000), (BIG, 8), (8, BIG), (BIG, BIG)):
        for K in (1, 3, 5, 8):
            if N >= K:
                assert label_ws(M, N, K) == closed_form(M, N, K), (M, N, K)
                assert label_ws(M, N, K) % 8 == 0
                assert label_ws(M, N, K) - int(lib.load().mogan_knn_cross_ws_bytes(M, N, K)) == 24 * C.shares(M, N) * M
            else:
                assert label_ws(M, N, K) == 0
    assert label_ws(1, 1, 1) == 32 + 24 and label_ws(70, 200, 5) == closed_form(70, 200, 5) and C.shares(70, 200) == 4
    for M, N, K in ((0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, -1, 1), (5, 5, 0), (5, 5, 9), (5, 5, -2), (5, 4, 5), (1 << 31, 5, 1),
                    (5, 1 << 31, 1), (1 << 40, 5, 1)):
        assert label_ws(M, N, K) == 0, (M, N, K)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_both_gates():
    """the limits themselves and the smallest legal problem: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the launch
    itself is what fails"""
    assert label() == LAUNCH and label(K=8) == LAUNCH and label(K=1) == LAUNCH and label(D=65536) == LAUNCH and label(D=1) == LAUNCH
    assert label(N=5) == LAUNCH and label(M=1, N=1, D=1, K=1) == LAUNCH and label(N=8, K=8) == LAUNCH
    assert label(M=BIG, N=BIG, ws_size=label_ws(BIG, BIG, 5)) == LAUNCH
    assert label(ws_size=label_ws(30000, 150000, 5)) == LAUNCH
