"""The rejections of mogan_softmax_head_f64 (csrc/mogan_softmax_head.hip), as tests/test_kid_rejections_cpu.py does
for mogan_poly3_mmd_f64: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are
dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  The size query is held to its closed form,
8 S ceil(ceil(n / S) / 64) C, which does not shrink when n or C grows."""
import ctypes

import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, WS = -1, -3
OK = dict(n=30000, D=2048, C=1000, S=10)
BIG = (1 << 31) - 1
C_MAX = 1 << 20
POINTERS = ("x", "w", "bias", "row_lse", "row_h", "psum")


def head_ws(n, C, S):
    return int(lib.load().mogan_softmax_head_ws_bytes(n, C, S))


def closed_form(n, C, S):
    return 8 * S * (-(-(-(-n // S)) // 64)) * C


def head(ws=PTR, ws_size=None, **kw):
    d = dict(OK, **{k: v for k, v in kw.items() if k in OK})
    ptrs = {name: kw.get(name, PTR) for name in POINTERS}
    if ws_size is None:
        ws_size = max(head_ws(d["n"], d["C"], d["S"]), 1 << 20)
    return lib.load().mogan_softmax_head_f64(ptrs["x"], d["n"], d["D"], ptrs["w"], ptrs["bias"], d["C"], d["S"], ptrs["row_lse"],
                                             ptrs["row_h"], ptrs["psum"], ws, ws_size, NULL)


SHAPE_CASES = [("NULL %s" % name, {name: NULL}) for name in POINTERS if name != "row_lse"] + [
    ("misaligned x", dict(x=ctypes.c_void_p(258))), ("misaligned w", dict(w=ctypes.c_void_p(257))),
    ("misaligned bias", dict(bias=ctypes.c_void_p(259))), ("misaligned row_lse", dict(row_lse=ctypes.c_void_p(260))),
    ("misaligned row_h", dict(row_h=ctypes.c_void_p(260))), ("misaligned psum", dict(psum=ctypes.c_void_p(257))),
    ("n = 0", dict(n=0, S=1)), ("n < 0", dict(n=-5)), ("n = 2^31", dict(n=1 << 31)), ("n = 2^40", dict(n=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("C = 0", dict(C=0)), ("C < 0", dict(C=-1000)), ("C = 2^20 + 1", dict(C=C_MAX + 1)), ("C = 2^31 - 1", dict(C=BIG)),
    ("S = 0", dict(S=0)), ("S < 0", dict(S=-10)), ("S = n + 1", dict(n=9, S=10)), ("S = 65536", dict(n=100000, S=65536)),
    ("S = 2^30", dict(n=BIG, S=1 << 30)),
    ("a bad shape with a NULL workspace is a shape error", dict(S=0, ws=NULL, ws_size=0)),
    ("a NULL output with a NULL workspace is a shape error", dict(psum=NULL, ws=NULL, ws_size=0)),
]
WS_CASES = [
    ("NULL ws", dict(ws=NULL)), ("NULL ws of size 0", dict(ws=NULL, ws_size=0)), ("size 0", dict(ws_size=0)),
    ("misaligned ws", dict(ws=ctypes.c_void_p(260))), ("NULL ws and no row_lse", dict(ws=NULL, row_lse=NULL)),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in SHAPE_CASES], ids=[c[0] for c in SHAPE_CASES])
def test_rejects_shapes_before_any_launch(kw):
    assert head(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in WS_CASES], ids=[c[0] for c in WS_CASES])
def test_rejects_a_missing_workspace_before_any_launch(kw):
    assert head(**kw) == WS


def test_rejects_a_short_workspace_before_any_launch():
    need = head_ws(30000, 1000, 10)
    assert need == 8 * 10 * 47 * 1000                                  # 3000 rows per split: 47 stripes
    assert head(ws_size=need - 1) == WS and head(ws_size=8) == WS
    assert head(n=1, D=1, C=1, S=1, ws_size=head_ws(1, 1, 1) - 1) == WS
    assert head(n=130, D=3, C=65, S=130, ws_size=head_ws(130, 65, 130) - 1) == WS
    # a split more may need a larger workspace than the call before it had
    assert head_ws(130, 65, 2) > head_ws(130, 65, 1) and head(n=130, C=65, S=2, ws_size=head_ws(130, 65, 1)) == WS


def test_the_signatures_are_the_headers():
    P, L, I, Z = lib.P, lib.L, lib.I, lib.Z
    assert lib.SIGNATURES["mogan_softmax_head_ws_bytes"] == [L, I, I]
    assert lib.SIGNATURES["mogan_softmax_head_f64"] == [P, L, I, P, P, I, I, P, P, P, P, Z, P]
    assert lib.load().mogan_softmax_head_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_are_positive_monotone_in_n_and_c_and_0_for_illegal_arguments():
    sizes = (1, 2, 63, 64, 65, 128, 129, 130, 1000, 30000, 65535, 65536, BIG)
    for S in (1, 2, 3, 10, 64, 65535):
        for C in (1, 2, 64, 65, 1000, C_MAX):
            last = 0
            for n in sizes:
                if n < S:
                    assert head_ws(n, C, S) == 0
                    continue
                got = head_ws(n, C, S)
                assert got == closed_form(n, C, S) and got > 0 and got % 8 == 0 and got >= last, (n, C, S)
                last = got
        for n in (S, 70000, BIG):
            if n >= S:
                by_c = [head_ws(n, C, S) for C in (1, 2, 63, 64, 65, 130, 1000, C_MAX)]
                assert by_c == sorted(by_c) and by_c[0] > 0
    assert head_ws(1, 1, 1) == 8 and head_ws(130, 65, 130) == 8 * 130 * 65 and head_ws(130, 65, 2) == 8 * 2 * 2 * 65
    for n, C, S in ((0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, -1, 1), (5, 5, 0), (5, 5, 6), (5, 5, -2), (1 << 31, 5, 1), (1 << 40, 5, 1),
                    (5, C_MAX + 1, 1), (70000, 5, 65536)):
        assert head_ws(n, C, S) == 0, (n, C, S)
