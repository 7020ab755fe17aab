"""The shape-error returns of the convolution entry points of libmogan_hip.so (csrc/mogan_gemm.hip).  Every case here is
answered by the host dispatch BEFORE any HIP call, so the table runs without a GPU: the pointers are dummies that are never
dereferenced and the workspace is null.  -1 = MOGAN_ERR_SHAPE; 1 = "not a geometry for this entry point" (mogan_conv2d_lrelu_fwd)."""
import ctypes

import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
WS = (NULL, 0, NULL)                # workspace, its size, stream


def _geom(B=2, Cin=8, Hs=8, Ws=8, Cout=8, KH=3, KW=3, stride=1, ph=1, pw=1):
    return dict(B=B, Cin=Cin, Hs=Hs, Ws=Ws, Cout=Cout, KH=KH, KW=KW, stride=stride, ph=ph, pw=pw)


def _ints(g):
    return [g[k] for k in ("B", "Cin", "Hs", "Ws", "Cout", "KH", "KW", "stride", "ph", "pw")]


def _out(g):
    return ((g["Hs"] + 2 * g["ph"] - g["KH"]) // g["stride"] + 1, (g["Ws"] + 2 * g["pw"] - g["KW"]) // g["stride"] + 1)


def _xd(g):
    return g["Cin"] * g["Hs"] * g["Ws"]


def _yd(g):
    oh, ow = _out(g)
    return g["Cout"] * oh * ow


def fwd(g, up=0):
    return lib.load().mogan_conv2d_fwd(PTR, PTR, PTR, *_ints(g), up, *WS)


def dgrad(g, up=0):
    return lib.load().mogan_conv2d_dgrad(PTR, PTR, PTR, *_ints(g), up, *WS)


def wgrad(g, up=0):
    return lib.load().mogan_conv2d_wgrad(PTR, PTR, PTR, *_ints(g), up, 0, *WS)


def lrelu(g, slope):
    return lib.load().mogan_conv2d_lrelu_fwd(PTR, PTR, PTR, *_ints(g), slope, *WS)


def affine_ex(g, scale=PTR, shift=PTR, x_bstride=None, y_bstride=-1):
    xbs = _xd(g) if x_bstride is None else x_bstride
    return lib.load().mogan_conv2d_affine_fwd_ex(PTR, xbs, PTR, scale, shift, PTR, y_bstride, NULL, 0, 0, *_ints(g), 1, *WS)


def fwd_ex(g, x_bstride=None, y_bstride=-1):
    xbs = _xd(g) if x_bstride is None else x_bstride
    return lib.load().mogan_conv2d_fwd_ex(PTR, xbs, PTR, PTR, y_bstride, NULL, 0, 0, *_ints(g), *WS)


def dgrad_ex(g, dy_bstride=None, dx_bstride=None, accumulate=0):
    dybs = _yd(g) if dy_bstride is None else dy_bstride
    dxbs = _xd(g) if dx_bstride is None else dx_bstride
    return lib.load().mogan_conv2d_dgrad_ex(PTR, dybs, PTR, PTR, dxbs, NULL, 0, accumulate, *_ints(g), *WS)


def fwd_member(g, **kw):
    a = lib.ConvFwdArgs()
    a.x = a.w = a.scale = a.shift = a.y = 256
    a.x_bstride, a.y_bstride, a.relu = _xd(g), -1, 1
    for k, v in list(g.items()) + list(kw.items()):
        setattr(a, k, v)
    return a


def dgrad_member(g, **kw):
    a = lib.ConvDgradArgs()
    a.dy = a.w = a.dx = 256
    a.dy_bstride, a.dx_bstride = _yd(g), _xd(g)
    for k, v in list(g.items()) + list(kw.items()):
        setattr(a, k, v)
    return a


def fwd_group(members, n=None):
    arr = (lib.ConvFwdArgs * max(1, len(members)))(*members)
    return lib.load().mogan_conv2d_affine_fwd_group(len(members) if n is None else n, arr, *WS)


def dgrad_group(members, n=None):
    arr = (lib.ConvDgradArgs * max(1, len(members)))(*members)
    return lib.load().mogan_conv2d_dgrad_group(len(members) if n is None else n, arr, *WS)


G = _geom()
S2K1 = _geom(KH=1, KW=1, stride=2, ph=0, pw=0)          # stride > kernel: a parity class without a tap

CASES = [
    ("fwd B=0", lambda: fwd(_geom(B=0)), -1),
    ("fwd OH<=0", lambda: fwd(_geom(Hs=2, Ws=2, KH=5, KW=5, ph=0, pw=0)), -1),
    ("fwd up=2", lambda: fwd(G, up=2), -1),
    ("fwd stride=0", lambda: fwd(_geom(stride=0)), -1),
    ("fwd 2^30 elements", lambda: fwd(_geom(B=1 << 14, Cin=1 << 10, Hs=8, Ws=8)), -1),
    ("dgrad Cout=0", lambda: dgrad(_geom(Cout=0)), -1),
    ("dgrad OW<=0", lambda: dgrad(_geom(Ws=1, KW=4, pw=0)), -1),
    ("wgrad up=2", lambda: wgrad(G, up=2), -1),
    ("wgrad Cin=0", lambda: wgrad(_geom(Cin=0)), -1),
    ("affine_ex null scale", lambda: affine_ex(G, scale=NULL), -1),
    ("affine_ex null shift", lambda: affine_ex(G, shift=NULL), -1),
    ("affine_ex x_bstride < dense", lambda: affine_ex(G, x_bstride=_xd(G) - 1), -1),
    ("affine_ex slice beyond 2^30", lambda: affine_ex(G, x_bstride=1 << 30), -1),
    ("affine_ex B=0", lambda: affine_ex(_geom(B=0)), -1),
    ("fwd_ex y_bstride < dense", lambda: fwd_ex(G, y_bstride=_yd(G) - 1), -1),
    ("fwd_ex x_bstride < dense", lambda: fwd_ex(G, x_bstride=_xd(G) - 1), -1),
    ("fwd_ex OH<=0", lambda: fwd_ex(_geom(Hs=2, Ws=2, KH=5, KW=5, ph=0, pw=0)), -1),
    ("dgrad_ex non-dense, stride > KH", lambda: dgrad_ex(S2K1, dy_bstride=_yd(S2K1) + 16), -1),
    ("dgrad_ex accumulate, stride > KH", lambda: dgrad_ex(S2K1, accumulate=1), -1),
    ("dgrad_ex dy_bstride < dense", lambda: dgrad_ex(G, dy_bstride=_yd(G) - 1), -1),
    ("dgrad_ex dx_bstride < dense", lambda: dgrad_ex(G, dx_bstride=_xd(G) - 1), -1),
    ("dgrad_ex B=0", lambda: dgrad_ex(_geom(B=0)), -1),
    ("lrelu slope=0", lambda: lrelu(_geom(Cin=3, KH=4, KW=4, stride=2), 0.0), -1),
    ("lrelu slope<0", lambda: lrelu(_geom(Cin=3, KH=4, KW=4, stride=2), -0.2), -1),
    ("lrelu Cin=32", lambda: lrelu(_geom(Cin=32, KH=4, KW=4, stride=2), 0.2), 1),
    ("lrelu Cout=4", lambda: lrelu(_geom(Cin=3, Cout=4, KH=4, KW=4, stride=2), 0.2), 1),
    ("lrelu Cin=32 and slope=0", lambda: lrelu(_geom(Cin=32, KH=4, KW=4, stride=2), 0.0), -1),
    ("lrelu B=0", lambda: lrelu(_geom(B=0, Cin=3), 0.2), -1),
    ("fwd_group n=5", lambda: fwd_group([fwd_member(G)] * 5), -1),
    ("fwd_group n=0", lambda: fwd_group([fwd_member(G)], n=0), -1),
    ("fwd_group null args", lambda: lib.load().mogan_conv2d_affine_fwd_group(2, NULL, *WS), -1),
    ("fwd_group n=1 zeroed member", lambda: fwd_group([lib.ConvFwdArgs()]), -1),
    ("fwd_group zeroed second member", lambda: fwd_group([fwd_member(G), lib.ConvFwdArgs()]), -1),
    ("fwd_group n=1 null scale", lambda: fwd_group([fwd_member(G, scale=None)]), -1),
    ("fwd_group second member null shift", lambda: fwd_group([fwd_member(G), fwd_member(G, shift=None)]), -1),
    ("fwd_group n=1 x_bstride < dense", lambda: fwd_group([fwd_member(G, x_bstride=_xd(G) - 1)]), -1),
    ("fwd_group second member x_bstride < dense", lambda: fwd_group([fwd_member(G), fwd_member(G, x_bstride=_xd(G) - 1)]), -1),
    ("dgrad_group n=5", lambda: dgrad_group([dgrad_member(G)] * 5), -1),
    ("dgrad_group n=0", lambda: dgrad_group([dgrad_member(G)], n=0), -1),
    ("dgrad_group null args", lambda: lib.load().mogan_conv2d_dgrad_group(2, NULL, *WS), -1),
    ("dgrad_group n=1 zeroed member", lambda: dgrad_group([lib.ConvDgradArgs()]), -1),
    ("dgrad_group zeroed second member", lambda: dgrad_group([dgrad_member(G), lib.ConvDgradArgs()]), -1),
    ("dgrad_group n=1 non-dense, stride > KH", lambda: dgrad_group([dgrad_member(S2K1, dy_bstride=_yd(S2K1) + 16)]), -1),
    # in a group of two or more the rejection does not depend on the addressing: a dense member is refused as well
    ("dgrad_group dense member, stride > KH", lambda: dgrad_group([dgrad_member(G), dgrad_member(S2K1)]), -1),
    ("dgrad_group n=1 dy_bstride < dense", lambda: dgrad_group([dgrad_member(G, dy_bstride=_yd(G) - 1)]), -1),
    ("dgrad_group second member dx_bstride < dense", lambda: dgrad_group([dgrad_member(G), dgrad_member(G, dx_bstride=_xd(G) - 1)]), -1),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_conv_entry_point_rejects_before_any_launch(call, expected):
    assert call() == expected
