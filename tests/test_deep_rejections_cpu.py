"""The rejections of the deep-block entry points (csrc/mogan_pgemm.hip: mogan_deep_conv_bn_act_fwd / _bwd, mogan_deep_block_eligible,
mogan_pk_panel_bytes) and of the grouped panel launches beside them (mogan_pk_group, mogan_panel_tail_group), as
tests/test_loss_rejections_cpu.py holds those of the losses: every case is answered by the host BEFORE any HIP call, so the
table runs without a GPU -- the data pointers are dummies that are never dereferenced (the argument tables of the grouped
launches are real host arrays: the host reads them).
-1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS.  A NULL in a nullable place (x with a panel given, rmean, rvar, zpanel; dgamma, dbeta, dx,
and the workspace of a backward without dx) is no rejection: tests/test_deep_entry_points_gpu.py runs those, and repeats the
rejections that can be stated with real buffers to see that a declined call has written nothing."""
import ctypes

import pytest

import deep_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, WS = -1, -3
BIG_WS = 1 << 30
GLU, TANH, SIGMOID = 3, 4, 5
GOOD = dict(B=4, Cin=64, Hs=8, Ws=8, Cout=64, KH=4, KW=4, stride=2, ph=1, pw=1, act=K.LRELU, groups=1)
FWD_PTRS = ("x", "xpanel", "wpk", "gamma", "beta", "rmean", "rvar", "y", "stats", "z", "zpanel")
BWD_PTRS = ("dz", "y", "stats", "gamma", "beta", "wpk_dgrad", "dy", "dgamma", "dbeta", "dx")


def L():
    return lib.load()


def _dims(d):
    return [d[k] for k in ("B", "Cin", "Hs", "Ws", "Cout", "KH", "KW", "stride", "ph", "pw")]


def fwd(null=(), ws=PTR, ws_bytes=BIG_WS, **kw):
    d = dict(GOOD, **kw)
    p = [NULL if n in null else PTR for n in FWD_PTRS]
    return L().mogan_deep_conv_bn_act_fwd(*p, *_dims(d), 1e-5, 0.1, d["act"], 0.2, d["groups"], ws, ws_bytes, NULL)


def bwd(null=(), ws=PTR, ws_bytes=BIG_WS, accumulate=1, **kw):
    d = dict(GOOD, **kw)
    p = [NULL if n in null else PTR for n in BWD_PTRS]
    return L().mogan_deep_conv_bn_act_bwd(*p[:9], accumulate, p[9], *_dims(d), d["act"], 0.2, d["groups"], ws, ws_bytes, NULL)


def eligible(**kw):
    d = dict(GOOD, **kw)
    return L().mogan_deep_block_eligible(*_dims(d), d["act"], d["groups"])


def fwd_panel_bytes(**kw):
    d = dict(GOOD, **kw)
    return K.up256(d["B"] * d["Hs"] * d["Ws"] * d["Cin"] * 6)


def bwd_panel_bytes(**kw):
    d = dict(GOOD, **kw)
    OH, OW = (d["Hs"] + 2 * d["ph"] - d["KH"]) // d["stride"] + 1, (d["Ws"] + 2 * d["pw"] - d["KW"]) // d["stride"] + 1
    return K.up256(d["B"] * OH * OW * d["Cout"] * 6)


# the shape rows both directions share: (name, changed arguments)
SHAPE_ROWS = [
    ("B = 0", dict(B=0)), ("B < 0", dict(B=-4)), ("groups = 0", dict(groups=0)), ("groups = 3", dict(B=6, groups=3)),
    ("B % groups", dict(B=5, groups=2)), ("Cin % 32", dict(Cin=48)), ("Cout % 32", dict(Cout=48)), ("Cout = 0", dict(Cout=0)),
    ("stride = 0", dict(stride=0)), ("stride < 0", dict(stride=-2)),
    ("OH <= 0", dict(Hs=2, Ws=2, ph=0, pw=0)), ("OW <= 0", dict(Ws=2, pw=0)),
    ("NE = 2064 > 2048", dict(B=129)), ("two groups, NE = 1040 > 1024", dict(B=130, groups=2)),
    ("act = GLU", dict(act=GLU)), ("act = TANH", dict(act=TANH)), ("act = SIGMOID", dict(act=SIGMOID)),
    ("KH * KW = 36 > 25", dict(KH=6, KW=6, ph=2, pw=2)),
]
# the data gradient's geometry, rejected where dx is wanted
DX_ROWS = [
    ("KH % stride", dict(KH=3)), ("KW % stride", dict(KW=3)),
    ("Hs % stride", dict(Hs=9)), ("Ws % stride", dict(Ws=9)), ("Cin = 0", dict(Cin=0)), ("Cin < 0", dict(Cin=-32)),
]

CASES = []
for name, kw in SHAPE_ROWS:
    CASES += [("fwd " + name, lambda kw=kw: fwd(**kw), SHAPE), ("fwd from a panel " + name, lambda kw=kw: fwd(null=("x",), **kw), SHAPE),
              ("bwd " + name, lambda kw=kw: bwd(**kw), SHAPE), ("bwd without dx " + name, lambda kw=kw: bwd(null=("dx",), ws=NULL, **kw), SHAPE),
              ("eligible " + name, lambda kw=kw: eligible(**kw), 0)]
CASES += [("fwd Cin = 0", lambda: fwd(Cin=0), SHAPE), ("fwd Hs = 0", lambda: fwd(Hs=0, ph=2), SHAPE)]
CASES += [("fwd NULL " + n, lambda n=n: fwd(null=(n,)), SHAPE) for n in ("gamma", "beta", "y", "stats", "z", "wpk")]
CASES += [("fwd from a panel NULL wpk", lambda: fwd(null=("x", "wpk")), SHAPE),
          ("fwd x and xpanel NULL", lambda: fwd(null=("x", "xpanel")), SHAPE),
          ("fwd x and xpanel NULL, no workspace either", lambda: fwd(null=("x", "xpanel"), ws=NULL, ws_bytes=0), SHAPE),
          ("fwd without xpanel: ws NULL", lambda: fwd(null=("xpanel",), ws=NULL), WS),
          ("fwd without xpanel: ws one byte short of the panel", lambda: fwd(null=("xpanel",), ws_bytes=fwd_panel_bytes() - 1), WS),
          ("fwd without xpanel: ws short, two groups", lambda: fwd(null=("xpanel",), B=8, groups=2, ws_bytes=fwd_panel_bytes(B=8) - 1), WS)]
CASES += [("bwd NULL " + n, lambda n=n: bwd(null=(n,)), SHAPE) for n in ("dz", "y", "stats", "gamma", "beta", "dy")]
CASES += [("bwd without dx NULL " + n, lambda n=n: bwd(null=(n, "dx")), SHAPE) for n in ("dz", "y", "stats", "gamma", "beta", "dy")]
CASES += [("bwd with dx: ws NULL", lambda: bwd(ws=NULL), WS),
          ("bwd with dx: ws one byte short of the panel", lambda: bwd(ws_bytes=bwd_panel_bytes() - 1), WS),
          ("bwd with dx: wpk_dgrad NULL", lambda: bwd(null=("wpk_dgrad",)), WS)]
CASES += [("bwd with dx " + name, lambda kw=kw: bwd(**kw), SHAPE) for name, kw in DX_ROWS]
CASES += [("bwd with dx, accumulate = 0, " + name, lambda kw=kw: bwd(accumulate=0, **kw), SHAPE) for name, kw in DX_ROWS[:4]]
CASES += [("eligible " + name, lambda kw=kw: eligible(**kw), 0) for name, kw in DX_ROWS]


# ------------------------------------------------------------------------------------- mogan_pk_group / _panel_tail_group
PK_GOOD = dict(B=2, M=64, Cp=64, CGp=2, cg0=0, PH=8, PW=8, outH=8, outW=8, KH=3, KW=3, stride=1, ph=1, pw=1, dgrad=0, nsplit=1)


def pk_group(n=1, args=True, null=(), **kw):
    arr = (lib.PkArgs * 9)()
    for a in arr:
        a.wpk, a.panel, a.raw = (None if k in null else 256 for k in ("wpk", "panel", "raw"))
        for k, v in dict(PK_GOOD, **kw).items():
            setattr(a, k, v)
    return L().mogan_pk_group(n, ctypes.cast(arr, ctypes.c_void_p) if args else NULL, NULL)


def tail_group(n=1, args=True):
    arr = (lib.TailArgs * 9)()
    return L().mogan_panel_tail_group(n, ctypes.cast(arr, ctypes.c_void_p) if args else NULL, NULL)


CASES += [("pk_group n = 0", lambda: pk_group(n=0), SHAPE), ("pk_group n = 9", lambda: pk_group(n=9), SHAPE),
          ("pk_group n < 0", lambda: pk_group(n=-1), SHAPE), ("pk_group args NULL", lambda: pk_group(args=False), SHAPE),
          ("pk_group Cp % 32", lambda: pk_group(Cp=48), SHAPE), ("pk_group Cp = 0", lambda: pk_group(Cp=0), SHAPE),
          ("pk_group cg0 + Cp / 32 > CGp", lambda: pk_group(cg0=1), SHAPE), ("pk_group cg0 < 0", lambda: pk_group(cg0=-1), SHAPE),
          ("pk_group dgrad with stride 2", lambda: pk_group(dgrad=1, stride=2), SHAPE),
          ("pk_group KH * KW = 35 > 25", lambda: pk_group(KH=5, KW=7), SHAPE), ("pk_group nsplit = 0", lambda: pk_group(nsplit=0), SHAPE),
          ("pk_group nsplit < 0", lambda: pk_group(nsplit=-2), SHAPE), ("pk_group stride = 0", lambda: pk_group(stride=0), SHAPE),
          ("pk_group B = 0", lambda: pk_group(B=0), SHAPE), ("pk_group M = 0", lambda: pk_group(M=0), SHAPE),
          ("pk_group outH = 0", lambda: pk_group(outH=0), SHAPE)]
CASES += [("pk_group NULL " + k, lambda k=k: pk_group(null=(k,)), SHAPE) for k in ("wpk", "panel", "raw")]
CASES += [("panel_tail_group n = 0", lambda: tail_group(n=0), SHAPE), ("panel_tail_group n = 9", lambda: tail_group(n=9), SHAPE),
          ("panel_tail_group n < 0", lambda: tail_group(n=-3), SHAPE), ("panel_tail_group args NULL", lambda: tail_group(args=False), SHAPE)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_the_good_arguments_are_eligible():
    """what every row above changes one thing of: a layer the deep block takes once the size heuristic is out of the way, also as two
    groups up to (B / 2) * OH * OW = 1024"""
    L().mogan_pk_debug_force(1, -1, 0)
    try:
        assert eligible() == 1 and eligible(B=8, groups=2) == 1
        assert eligible(B=128) == 1 and eligible(B=128, groups=2) == 1          # NE = 2048 in one group, 1024 each in two
        assert eligible(B=130) == 0 and eligible(B=130, groups=2) == 0          # NE * 2 = 2080 > 2048
        assert eligible(act=K.NONE) == 1 and eligible(act=K.RELU) == 1
    finally:
        L().mogan_pk_debug_force(0, -1, 0)
    assert eligible() == 0          # (K = 1024 but only 64 rows: the heuristic leaves this layer to the other kernels)


def test_panel_bytes():
    pb = L().mogan_pk_panel_bytes
    assert pb(4, 64, 16) == 6 * 4 * 64 * 16 and pb(32, 96, 64) == 6 * 32 * 96 * 64 and pb(1, 32, 1) == 192
    for bad in ((0, 64, 16), (4, 0, 16), (4, 64, 0), (-4, 64, 16), (4, -64, 16), (4, 64, -16)):
        assert pb(*bad) == 0, bad
    for row in K.ROWS:
        g = K.geom(row)
        assert K.up256(pb(g["B"], g["Cin"], g["Hs"] * g["Ws"])) == K.fwd_ws_bytes(row, 0)
        assert K.up256(pb(g["B"], g["Cout"], g["HW"])) == K.bwd_ws_bytes(row, 0)


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_deep_entry_point_rejects_before_any_launch(call, expected):
    L().mogan_pk_debug_force(1, -1, 0)          # (eligibility rows: the hard constraints alone)
    try:
        assert call() == expected
    finally:
        L().mogan_pk_debug_force(0, -1, 0)
