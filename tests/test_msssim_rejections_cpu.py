"""The rejections of the three MS-SSIM entries (csrc/mogan_ssim.hip), as tests/test_swd_rejections_cpu.py does for the SWD kernels:
every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that are never
dereferenced.  -1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  That the largest accepted sizes pass both gates is shown by the answer
changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  The size query is held to its closed form, and the two
ops refuse what they would have to convert."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

PTR, PTR2, PTR3, PTR4 = (ctypes.c_void_p(v) for v in (256, 512, 1024, 2048))     # non-null, aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3
BIG = (1 << 31) - 1
TILE = 32


def L():
    return lib.load()


def down(x=PTR, out=PTR2, NC=6, H=16, W=16):
    return L().mogan_avg_down2(x, NC, H, W, out, NULL)


def ws_bytes(P, C, S, n):
    return int(L().mogan_ssim_level_ws_bytes(P, C, S, n))


def level(a=PTR, b=PTR2, win=PTR3, terms=PTR4, ssim_map=NULL, cs_map=NULL, ws=PTR, ws_size=None, P=5, C=3, S=64, n=11):
    if ws_size is None:
        ws_size = max(ws_bytes(P, C, S, n), 1 << 20)
    return L().mogan_ssim_level_f64(a, b, P, C, S, win, n, terms, ssim_map, cs_map, ws, ws_size, NULL)


DOWN = [("NULL x", dict(x=NULL)), ("NULL out", dict(out=NULL)), ("NC = 0", dict(NC=0)), ("NC < 0", dict(NC=-1)),
        ("odd H", dict(H=15)), ("odd W", dict(W=9)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-16)),
        ("W < 0", dict(W=-16)), ("NC = 2^31", dict(NC=1 << 31)), ("NC = 2^40", dict(NC=1 << 40)),
        ("NC H W = 2^31", dict(NC=1 << 15, H=256, W=256)), ("H W above 2^31", dict(NC=1, H=1 << 16, W=1 << 16))]
LEVEL = [("NULL a", dict(a=NULL)), ("NULL b", dict(b=NULL)), ("NULL win", dict(win=NULL)), ("NULL terms", dict(terms=NULL)),
         ("C = 0", dict(C=0)), ("C = 5", dict(C=5)), ("C < 0", dict(C=-3)), ("P = 0", dict(P=0)), ("P < 0", dict(P=-1)),
         ("P = 2^31", dict(P=1 << 31)), ("S = 1", dict(S=1, n=1)), ("S = 0", dict(S=0, n=1)), ("S < 0", dict(S=-64)),
         ("n = 0", dict(n=0)), ("n < 0", dict(n=-11)), ("n = 12", dict(n=12)), ("n > S", dict(S=8, n=9)), ("n = 11 > S = 10", dict(S=10)),
         ("P C S S = 2^31", dict(P=1 << 13, C=4, S=256)), ("S S above 2^31", dict(P=1, C=1, S=1 << 16)),
         ("a bad shape with a NULL workspace is a shape error", dict(C=0, ws=NULL, ws_size=0))]
TABLE = [(fn, name, kw) for fn, cases in ((down, DOWN), (level, LEVEL)) for name, kw in cases]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("fn,kw", [(t[0], t[2]) for t in TABLE], ids=["%s: %s" % (t[0].__name__, t[1]) for t in TABLE])
def test_rejects_shapes_before_any_launch(fn, kw):
    assert fn(**kw) == SHAPE


@pytest.mark.parametrize("kw", [dict(ws=NULL), dict(ws=NULL, ws_size=0), dict(ws_size=0), dict(ws=ctypes.c_void_p(260)),
                                dict(ws_size=16 * 5 * 3 * 4 - 1)],
                         ids=["NULL ws", "NULL ws of size 0", "size 0", "misaligned ws", "one byte short"])
def test_a_level_rejects_a_missing_workspace_before_any_launch(kw):
    assert level(**kw) == WS


def test_the_signatures_are_the_headers():
    P, I, Lg, Z = lib.P, lib.I, lib.L, lib.Z
    assert lib.SIGNATURES["mogan_avg_down2"] == [P, Lg, I, I, P, P]
    assert lib.SIGNATURES["mogan_ssim_level_ws_bytes"] == [Lg, I, I, I]
    assert lib.SIGNATURES["mogan_ssim_level_f64"] == [P, P, Lg, I, I, P, I, P, P, P, P, Z, P]
    assert L().mogan_ssim_level_ws_bytes.restype is ctypes.c_size_t


def test_ws_bytes_follow_their_closed_form_and_are_0_for_illegal_arguments():
    """16 P C T T bytes, T = ceil((S - n + 1) / 32) tiles per axis"""
    for P in (1, 5, 64):
        for C in (1, 2, 3, 4):
            for S, n in ((2, 1), (2, 2), (4, 4), (11, 11), (12, 11), (16, 11), (41, 11), (42, 11), (43, 11), (77, 11), (256, 11),
                         (256, 1), (33, 1), (32, 1)):
                assert ws_bytes(P, C, S, n) == 16 * P * C * (-(-(S - n + 1) // TILE)) ** 2, (P, C, S, n)
    assert ws_bytes(5, 3, 64, 11) == 16 * 5 * 3 * 4 and ws_bytes(1, 1, 4, 4) == 16 and ws_bytes(64, 3, 256, 11) == 16 * 64 * 3 * 64
    for P, C, S, n in ((0, 3, 64, 11), (-1, 3, 64, 11), (1 << 31, 1, 2, 1), (5, 0, 64, 11), (5, 5, 64, 11), (5, 3, 1, 1),
                       (5, 3, 64, 0), (5, 3, 64, 12), (5, 3, 8, 9), (1 << 13, 4, 256, 11)):
        assert ws_bytes(P, C, S, n) == 0, (P, C, S, n)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gates():
    """the limits themselves and the smallest legal problems: neither MOGAN_ERR_SHAPE nor MOGAN_ERR_WS; without a device the
    launch itself is what fails"""
    assert down() == LAUNCH and down(NC=1, H=2, W=2) == LAUNCH and down(H=8, W=32) == LAUNCH
    assert down(NC=(1 << 15) - 1, H=256, W=256) == LAUNCH
    assert level() == LAUNCH and level(P=1, C=1, S=2, n=1) == LAUNCH and level(C=4) == LAUNCH and level(S=11) == LAUNCH
    assert level(S=4, n=4) == LAUNCH and level(ssim_map=PTR2, cs_map=PTR3) == LAUNCH and level(a=PTR, b=PTR) == LAUNCH
    assert level(P=(1 << 13) - 1, C=4, S=256) == LAUNCH and level(ws_size=ws_bytes(5, 3, 64, 11)) == LAUNCH


def test_the_ops_refuse_what_they_would_have_to_convert():
    x = torch.zeros(6, 8, 8)
    for bad in (x.double(), x[0], x[:, :, ::2], torch.zeros(6, 7, 8), torch.zeros(6, 8, 6)[:, :, :5], x.numpy()):
        with pytest.raises(ValueError):
            ops.avg_down2(bad)
    a, w = torch.zeros(2, 3, 16, 16), torch.full((11,), 1 / 11.0)
    for args in ((a.double(), a, w), (a, a.half(), w), (a, a, w.double()), (a[0], a[0], w), (a, a, w.view(1, 11)),
                 (a[:, :, :, ::2], a[:, :, :, ::2], w), (a, a, torch.zeros(22)[::2]), (a, torch.zeros(2, 3, 16, 8), w),
                 (a, torch.zeros(3, 3, 16, 16), w), (torch.zeros(2, 5, 16, 16), torch.zeros(2, 5, 16, 16), w),
                 (torch.zeros(2, 3, 16, 8), torch.zeros(2, 3, 16, 8), w), (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), w),
                 (a, a, torch.zeros(12)), (a, a.to("meta"), w), (a, a, w.to("meta")), (a.numpy(), a, w)):
        with pytest.raises(ValueError):
            ops.ssim_level(*args)
    # legal host tensors: nothing left to object to but the device -- there is no CPU path
    with pytest.raises(lib.MoganHipError, match="no CPU path"):
        ops.avg_down2(x)
    with pytest.raises(lib.MoganHipError, match="no CPU path"):
        ops.ssim_level(a, a, w)
