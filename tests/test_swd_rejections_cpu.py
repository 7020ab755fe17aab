"""The rejections of the six sliced Wasserstein entries (csrc/mogan_swd.hip), as tests/test_prdc_rejections_cpu.py does for the PRDC
kernels: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that
are never dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is shown by the
answer changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  The size query is held to its closed form."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR, PTR2, PTR3 = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)     # non-null, aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3
BIG = (1 << 31) - 1


def L():
    return lib.load()


def down(x=PTR, out=PTR2, NC=6, H=16, W=16):
    return L().mogan_pyr_down(x, NC, H, W, out, NULL)


def resid(x=PTR, dn=PTR2, out=PTR3, NC=6, H=16, W=16):
    return L().mogan_lap_residual(x, dn, NC, H, W, out, NULL)


def gather(level=PTR, centres=PTR2, desc=PTR3, N=4, C=3, H=16, W=16, R=130, row0=5, rows_total=200):
    return L().mogan_swd_gather(level, N, C, H, W, centres, R, desc, row0, rows_total, NULL)


def mom_ws(rows, C):
    return int(L().mogan_swd_moments_ws_bytes(rows, C))


def mom(desc=PTR, out=PTR2, ws=PTR3, ws_size=None, rows=4099, C=3):
    if ws_size is None:
        ws_size = max(mom_ws(rows, C), 1 << 20)
    return L().mogan_swd_moments_f64(desc, rows, C, out, ws, ws_size, NULL)


def project(desc=PTR, moments=PTR2, dirs=PTR3, out=PTR, rows=130, C=3, D=128):
    return L().mogan_swd_project(desc, rows, C, moments, dirs, D, out, NULL)


def absdiff(a=PTR, b=PTR2, out=PTR3, rows=4097, D=3):
    return L().mogan_swd_absdiff_f64(a, b, rows, D, out, NULL)


PLANE = [("NC = 0", dict(NC=0)), ("NC < 0", dict(NC=-1)), ("odd H", dict(H=15)), ("odd W", dict(W=9)), ("H = 2", dict(H=2)),
         ("W = 2", dict(W=2)), ("H = 0", dict(H=0)), ("H < 0", dict(H=-16)), ("W < 0", dict(W=-16)),
         ("NC = 2^31", dict(NC=1 << 31)), ("NC = 2^40", dict(NC=1 << 40)), ("NC H W = 2^31", dict(NC=1 << 15, H=256, W=256)),
         ("NC H W above 2^31", dict(NC=BIG, H=4, W=4)), ("H W above 2^31", dict(NC=1, H=1 << 16, W=1 << 16))]
DOWN = [("NULL x", dict(x=NULL)), ("NULL out", dict(out=NULL))] + PLANE
RESID = [("NULL x", dict(x=NULL)), ("NULL down", dict(dn=NULL)), ("NULL out", dict(out=NULL)),
         ("out aliases x", dict(x=PTR, out=PTR)), ("out aliases down", dict(dn=PTR2, out=PTR2))] + PLANE
GATHER = [("NULL level", dict(level=NULL)), ("NULL centres", dict(centres=NULL)), ("NULL desc", dict(desc=NULL)),
          ("C = 0", dict(C=0)), ("C = 5", dict(C=5)), ("C < 0", dict(C=-3)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-1)),
          ("W = 6", dict(W=6)), ("H = 6", dict(H=6)), ("H = 0", dict(H=0)), ("R = 0", dict(R=0)), ("R < 0", dict(R=-5)),
          ("row0 < 0", dict(row0=-1)), ("row0 + R = rows_total + 1", dict(row0=71)), ("R > rows_total", dict(R=201, row0=0)),
          ("row0 + R overflows", dict(row0=(1 << 63) - 1, R=130)), ("rows_total = 0", dict(rows_total=0, R=1, row0=0)),
          ("rows_total = 2^31", dict(rows_total=1 << 31)), ("rows_total = 2^40", dict(rows_total=1 << 40)),
          ("N C H W = 2^31", dict(N=1 << 13, C=4, H=256, W=256)), ("N = 2^31 - 1", dict(N=BIG))]
MOM = [("NULL desc", dict(desc=NULL)), ("NULL moments", dict(out=NULL)), ("rows = 0", dict(rows=0)), ("rows < 0", dict(rows=-1)),
       ("rows = 2^31", dict(rows=1 << 31)), ("rows = 2^40", dict(rows=1 << 40)), ("C = 0", dict(C=0)), ("C = 5", dict(C=5)),
       ("a bad shape with a NULL workspace is a shape error", dict(C=0, ws=NULL, ws_size=0))]
PROJECT = [("NULL desc", dict(desc=NULL)), ("NULL moments", dict(moments=NULL)), ("NULL dirs", dict(dirs=NULL)),
           ("NULL out", dict(out=NULL)), ("rows = 0", dict(rows=0)), ("rows < 0", dict(rows=-3)), ("rows = 2^31", dict(rows=1 << 31)),
           ("C = 0", dict(C=0)), ("C = 5", dict(C=5)), ("D = 0", dict(D=0)), ("D < 0", dict(D=-128)), ("D = 1025", dict(D=1025)),
           ("D = 2^30", dict(D=1 << 30))]
ABSDIFF = [("NULL a", dict(a=NULL)), ("NULL b", dict(b=NULL)), ("NULL out", dict(out=NULL)), ("rows = 0", dict(rows=0)),
           ("rows < 0", dict(rows=-1)), ("rows = 2^31", dict(rows=1 << 31)), ("rows = 2^40", dict(rows=1 << 40)),
           ("D = 0", dict(D=0)), ("D = 1025", dict(D=1025)), ("D < 0", dict(D=-1))]
TABLE = [(fn, name, kw) for fn, cases in ((down, DOWN), (resid, RESID), (gather, GATHER), (mom, MOM), (project, PROJECT),
                                          (absdiff, ABSDIFF)) for name, kw in cases]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("fn,kw", [(t[0], t[2]) for t in TABLE], ids=["%s: %s" % (t[0].__name__, t[1]) for t in TABLE])
def test_rejects_shapes_before_any_launch(fn, kw):
    assert fn(**kw) == SHAPE


@pytest.mark.parametrize("kw", [dict(ws=NULL), dict(ws=NULL, ws_size=0), dict(ws_size=0), dict(ws=ctypes.c_void_p(260)),
                                dict(ws_size=8 * 3 * 65 - 1)],
                         ids=["NULL ws", "NULL ws of size 0", "size 0", "misaligned ws", "one byte short"])
def test_moments_reject_a_missing_workspace_before_any_launch(kw):
    assert mom(**kw) == WS


def test_the_signatures_are_the_headers():
    P, I, Lg, Z = lib.P, lib.I, lib.L, lib.Z
    assert lib.SIGNATURES["mogan_pyr_down"] == [P, Lg, I, I, P, P]
    assert lib.SIGNATURES["mogan_lap_residual"] == [P, P, Lg, I, I, P, P]
    assert lib.SIGNATURES["mogan_swd_gather"] == [P, I, I, I, I, P, Lg, P, Lg, Lg, P]
    assert lib.SIGNATURES["mogan_swd_moments_ws_bytes"] == [Lg, I]
    assert lib.SIGNATURES["mogan_swd_moments_f64"] == [P, Lg, I, P, P, Z, P]
    assert lib.SIGNATURES["mogan_swd_project"] == [P, Lg, I, P, P, I, P, P]
    assert lib.SIGNATURES["mogan_swd_absdiff_f64"] == [P, P, Lg, I, P, P]
    assert L().mogan_swd_moments_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_follow_their_closed_form_and_are_0_for_illegal_arguments():
    """8 C P bytes, P = min(ceil(rows / 64), 2048) shares of the rows"""
    for rows in (1, 63, 64, 65, 257, 4099, 131071, 131072, 131073, 2097152, BIG):
        for C in (1, 2, 3, 4):
            assert mom_ws(rows, C) == 8 * C * min(-(-rows // 64), 2048), (rows, C)
    assert mom_ws(4099, 3) == 8 * 3 * 65 and mom_ws(1, 1) == 8 and mom_ws(BIG, 4) == 8 * 4 * 2048
    for rows, C in ((0, 3), (-1, 3), (1 << 31, 3), (1 << 40, 3), (5, 0), (5, 5), (5, -1)):
        assert mom_ws(rows, C) == 0, (rows, C)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gates():
    """the limits themselves and the smallest legal problems: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the
    launch itself is what fails"""
    assert down() == LAUNCH and down(NC=1, H=4, W=4) == LAUNCH and down(H=8, W=32) == LAUNCH
    assert down(NC=(1 << 15) - 1, H=256, W=256) == LAUNCH and down(NC=BIG // 16, H=4, W=4) == LAUNCH
    assert resid() == LAUNCH and resid(NC=1, H=4, W=4) == LAUNCH and resid(NC=(1 << 15) - 1, H=256, W=256) == LAUNCH
    assert gather() == LAUNCH and gather(C=1) == LAUNCH and gather(C=4) == LAUNCH and gather(N=1, H=7, W=7, R=1) == LAUNCH
    assert gather(row0=70) == LAUNCH and gather(row0=0, R=200) == LAUNCH                     # row0 + R = rows_total
    assert gather(rows_total=BIG, row0=BIG - 130) == LAUNCH and gather(N=(1 << 13) - 1, C=4, H=256, W=256) == LAUNCH
    assert mom() == LAUNCH and mom(rows=1, C=1) == LAUNCH and mom(C=4) == LAUNCH
    assert mom(rows=BIG, ws_size=mom_ws(BIG, 3)) == LAUNCH and mom(ws_size=mom_ws(4099, 3)) == LAUNCH
    assert project() == LAUNCH and project(rows=1, C=1, D=1) == LAUNCH and project(D=1024, C=4) == LAUNCH
    assert project(rows=BIG) == LAUNCH
    assert absdiff() == LAUNCH and absdiff(rows=1, D=1) == LAUNCH and absdiff(rows=BIG, D=1024) == LAUNCH
