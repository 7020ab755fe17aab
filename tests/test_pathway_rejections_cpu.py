"""The rejections of the object-pathway and attention entry points of libmogan_hip.so (csrc/mogan_stn_attn.hip, the softmax
and concat of csrc/mogan_elem.hip), as tests/test_bn_rejections_cpu.py does for the batch-norm family: every case is answered by
the host BEFORE any HIP call, so the table runs without a GPU -- the data pointers are dummies that are never dereferenced (the
small host arrays of the concat -- C, rows, sb, sg, bcast and the pointer tables -- are real: the host reads them).
-1 = MOGAN_ERR_SHAPE.  A NULL in a nullable place (mask, dattn, lens, dsrc[i]) is no rejection: the GPU module runs those."""
import ctypes

import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE = -1
GOOD = (4, 3, 8, 8, 16, 16)         # B, C, Hin, Win, Hout, Wout
STN_PTRS = ("x / dy", "theta", "y / dx")


def L():
    return lib.load()


def _ptrs(n, null_at=None):
    return [NULL if i == null_at else PTR for i in range(n)]


def stn(fn, dims=GOOD, null_at=None, ac=0):
    return getattr(L(), "mogan_stn_" + fn)(*_ptrs(3, null_at), *dims, ac, NULL)


def stn_ex(fn, dims=GOOD, xB=None, plane=0, tG=0, null_at=None):
    return getattr(L(), "mogan_stn_%s_ex" % fn)(*_ptrs(3, null_at), *dims, 0, dims[0] if xB is None else xB, plane, tG, NULL)


def bbox(N=5, null_at=None):
    return L().mogan_bbox_to_theta(*_ptrs(3, null_at), N, NULL)


def attn_fwd(B=2, idf=8, Q=16, T=5, null_at=None):
    h, src, mask, wc, attn = _ptrs(5, null_at)
    return L().mogan_attn_fwd(h, src, mask, wc, attn, B, idf, Q, T, 0, NULL)


def attn_bwd(B=2, idf=8, Q=16, T=5, null_at=None):
    return L().mogan_attn_bwd(*_ptrs(6, null_at), B, idf, Q, T, NULL)


def sm_fwd(outer=3, L_=5, inner=4, null_at=None):
    x, y, lens = _ptrs(3, null_at)
    return L().mogan_softmax_fwd(x, y, lens, outer, L_, inner, 1.0, NULL)


def sm_bwd(outer=3, L_=5, inner=4, null_at=None):
    y, dy, dx, lens = _ptrs(4, null_at)
    return L().mogan_softmax_bwd(y, dy, dx, lens, outer, L_, inner, 1.0, NULL)


def cat(fn, C=(6, 5), rows=(6, 6), sb=(96, 5), sg=(0, 0), bcast=(0, 1), nsrc=None, N=6, HW=16, null_src=None, null_arg=None,
        other=PTR):
    """mogan_concat_fwd / _bwd with real host tables; null_src: which src[i] / dsrc[i] is NULL; null_arg: which of the table
    arguments (0 the pointer table, 1 C, 2 rows, 3 sb, 4 sg, 5 bcast) is NULL; other: dst / ddst"""
    n = len(C)
    tab = (ctypes.c_void_p * 4)(*[None if i == null_src or i >= n else 256 * (i + 1) for i in range(4)])
    pad = lambda v, fill: list(v) + [fill] * (4 - len(v))
    args = [tab, (ctypes.c_int * 4)(*pad(C, 1)), (ctypes.c_int * 4)(*pad(rows, 1)), (ctypes.c_longlong * 4)(*pad(sb, 1)),
            (ctypes.c_longlong * 4)(*pad(sg, 0)), (ctypes.c_int * 4)(*pad(bcast, 0))]
    args = [NULL if i == null_arg else ctypes.cast(a, ctypes.c_void_p) for i, a in enumerate(args)]
    nsrc = n if nsrc is None else nsrc
    if fn == "fwd":
        return L().mogan_concat_fwd(*args, nsrc, other, N, HW, NULL)
    return L().mogan_concat_bwd(other, *args, nsrc, N, HW, NULL)


def _with(i, v):
    d = list(GOOD)
    d[i] = v
    return tuple(d)


CASES = []
DIM_NAMES = ("B", "C", "Hin", "Win", "Hout", "Wout")
for i, name in enumerate(DIM_NAMES):
    for v in (0, -3):
        for fn in ("fwd", "bwd"):
            CASES += [("stn_%s %s = %d" % (fn, name, v), lambda fn=fn, d=_with(i, v): stn(fn, d), SHAPE),
                      ("stn_%s_ex %s = %d" % (fn, name, v), lambda fn=fn, d=_with(i, v): stn_ex(fn, d, xB=1), SHAPE)]
BIGP = 1 << 16                       # 65536 * 32768 = 2^31: one more than an int holds
for fn in ("fwd", "bwd"):
    CASES += [
        ("stn_%s B > 65535" % fn, lambda fn=fn: stn(fn, _with(0, 65536)), SHAPE),
        ("stn_%s_ex B > 65535" % fn, lambda fn=fn: stn_ex(fn, _with(0, 65536)), SHAPE),
        ("stn_%s_ex xB = 0" % fn, lambda fn=fn: stn_ex(fn, xB=0), SHAPE),
        ("stn_%s_ex xB = -2" % fn, lambda fn=fn: stn_ex(fn, xB=-2), SHAPE),
        ("stn_%s_ex B %% xB" % fn, lambda fn=fn: stn_ex(fn, xB=3), SHAPE),
        ("stn_%s_ex theta_G < 0" % fn, lambda fn=fn: stn_ex(fn, tG=-1), SHAPE),
        ("stn_%s_ex B %% theta_G" % fn, lambda fn=fn: stn_ex(fn, tG=3), SHAPE),
        ("stn_%s_ex x_plane, B %% xB" % fn, lambda fn=fn: stn_ex(fn, xB=3, plane=1), SHAPE),
        # a plane whose element count does not fit an int
        ("stn_%s Hin Win = 2^31" % fn, lambda fn=fn: stn(fn, (4, 3, BIGP, 1 << 15, 16, 16)), SHAPE),
        ("stn_%s Hout Wout = 2^31" % fn, lambda fn=fn: stn(fn, (4, 3, 8, 8, 1 << 15, BIGP)), SHAPE),
        ("stn_%s Hout Wout = 2^32 (0 as an int)" % fn, lambda fn=fn: stn(fn, (4, 3, 8, 8, BIGP, BIGP)), SHAPE),
        # ... or fits one, but not after the grid rounds it up to blocks of 256 (2^31 - 1 is prime: one row)
        ("stn_%s Hout Wout = 2^31 - 1" % fn, lambda fn=fn: stn(fn, (4, 3, 8, 8, 1, (1 << 31) - 1)), SHAPE),
        ("stn_%s Hin Win = 2^31 - 255" % fn, lambda fn=fn: stn(fn, (4, 3, (1 << 31) - 255, 1, 16, 16)), SHAPE),
        ("stn_%s_ex Hout Wout = 2^31 - 1" % fn, lambda fn=fn: stn_ex(fn, (4, 3, 8, 8, (1 << 31) - 1, 1)), SHAPE),
        ("stn_%s_ex x_plane, Hin Win = 2^31 - 255" % fn, lambda fn=fn: stn_ex(fn, (4, 3, 1, (1 << 31) - 255, 16, 16), plane=1), SHAPE),
        ("stn_%s_ex Hin Win = 2^31" % fn, lambda fn=fn: stn_ex(fn, (4, 3, BIGP, 1 << 15, 16, 16)), SHAPE),
        ("stn_%s_ex Hout Wout = 2^31" % fn, lambda fn=fn: stn_ex(fn, (4, 3, 8, 8, 1 << 15, BIGP)), SHAPE),
        ("stn_%s_ex x_plane, Hout Wout = 2^32" % fn, lambda fn=fn: stn_ex(fn, (4, 3, 8, 8, BIGP, BIGP), plane=1), SHAPE),
    ]
    for k, what in enumerate(STN_PTRS):
        CASES += [("stn_%s NULL %s" % (fn, what), lambda fn=fn, k=k: stn(fn, null_at=k), SHAPE),
                  ("stn_%s_ex NULL %s" % (fn, what), lambda fn=fn, k=k: stn_ex(fn, null_at=k), SHAPE),
                  ("stn_%s_ex x_plane, NULL %s" % (fn, what), lambda fn=fn, k=k: stn_ex(fn, plane=1, null_at=k), SHAPE)]
CASES += [
    # more channel groups of 8 than a grid extent holds, in the gather (the x_plane sum puts C in the grid's x extent)
    ("stn_bwd C > 8 * 65535", lambda: stn("bwd", _with(1, 8 * 65535 + 1)), SHAPE),
    ("stn_bwd_ex C > 8 * 65535", lambda: stn_ex("bwd", _with(1, 8 * 65535 + 1)), SHAPE),
    ("bbox_to_theta N = 0", lambda: bbox(0), SHAPE),
    ("bbox_to_theta N < 0", lambda: bbox(-4), SHAPE),
] + [("bbox_to_theta NULL %s" % w, lambda k=k: bbox(null_at=k), SHAPE) for k, w in enumerate(("bbox", "theta", "theta_inv"))]
for fn, call, names, nullable in (("attn_fwd", attn_fwd, ("h", "src", "mask", "wc", "attn"), {2}),
                                  ("attn_bwd", attn_bwd, ("src", "attn", "dwc", "dattn", "dh", "dscore"), {3})):
    CASES += [
        ("%s B = 0" % fn, lambda c=call: c(B=0), SHAPE), ("%s B < 0" % fn, lambda c=call: c(B=-1), SHAPE),
        ("%s B > 65535" % fn, lambda c=call: c(B=65536), SHAPE),
        ("%s idf = 0" % fn, lambda c=call: c(idf=0), SHAPE), ("%s idf < 0" % fn, lambda c=call: c(idf=-8), SHAPE),
        ("%s idf > 128" % fn, lambda c=call: c(idf=129), SHAPE),
        ("%s Q = 0" % fn, lambda c=call: c(Q=0), SHAPE), ("%s Q < 0" % fn, lambda c=call: c(Q=-16), SHAPE),
        ("%s T = 0" % fn, lambda c=call: c(T=0), SHAPE), ("%s T < 0" % fn, lambda c=call: c(T=-5), SHAPE),
        ("%s T > 32" % fn, lambda c=call: c(T=33), SHAPE),
    ] + [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names) if k not in nullable]
for fn, call, names in (("softmax_fwd", sm_fwd, ("x", "y")), ("softmax_bwd", sm_bwd, ("y", "dy", "dx"))):
    CASES += [
        ("%s outer = 0" % fn, lambda c=call: c(outer=0), SHAPE), ("%s outer < 0" % fn, lambda c=call: c(outer=-3), SHAPE),
        ("%s L = 0" % fn, lambda c=call: c(L_=0), SHAPE), ("%s L < 0" % fn, lambda c=call: c(L_=-5), SHAPE),
        ("%s inner = 0" % fn, lambda c=call: c(inner=0), SHAPE), ("%s inner < 0" % fn, lambda c=call: c(inner=-4), SHAPE),
    ] + [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names)]
TABLES = ("the pointer table", "C", "rows", "sb", "sg", "bcast")
OBJ = dict(C=(7,), rows=(2,), bcast=(1,))            # label[:, g] of a (2, 3, 7) tensor in a batch of 6: sb = 21, sg = 7
for fn in ("fwd", "bwd"):
    CASES += [
        ("concat_%s nsrc = 0" % fn, lambda fn=fn: cat(fn, nsrc=0), SHAPE),
        ("concat_%s nsrc < 0" % fn, lambda fn=fn: cat(fn, nsrc=-1), SHAPE),
        ("concat_%s nsrc = 5" % fn, lambda fn=fn: cat(fn, nsrc=5), SHAPE),
        ("concat_%s N = 0" % fn, lambda fn=fn: cat(fn, N=0), SHAPE),
        ("concat_%s N < 0" % fn, lambda fn=fn: cat(fn, N=-6), SHAPE),
        ("concat_%s HW = 0" % fn, lambda fn=fn: cat(fn, HW=0), SHAPE),
        ("concat_%s HW < 0" % fn, lambda fn=fn: cat(fn, HW=-16), SHAPE),
        ("concat_%s C[0] = 0" % fn, lambda fn=fn: cat(fn, C=(0, 5)), SHAPE),
        ("concat_%s C[1] < 0" % fn, lambda fn=fn: cat(fn, C=(6, -5)), SHAPE),
        ("concat_%s rows[0] = 0" % fn, lambda fn=fn: cat(fn, rows=(0, 6)), SHAPE),
        ("concat_%s rows[1] < 0" % fn, lambda fn=fn: cat(fn, rows=(6, -2)), SHAPE),
        ("concat_%s N %% rows[1]" % fn, lambda fn=fn: cat(fn, rows=(6, 4)), SHAPE),
        ("concat_%s NULL %s" % (fn, "dst" if fn == "fwd" else "ddst"), lambda fn=fn: cat(fn, other=NULL), SHAPE),
        # the per-object slice: sb a positive multiple of sg, and enough objects per row for the batch
        ("concat_%s sg > 0, sb = 0" % fn, lambda fn=fn: cat(fn, sb=(0,), sg=(7,), **OBJ), SHAPE),
        ("concat_%s sg > 0, sb < 0" % fn, lambda fn=fn: cat(fn, sb=(-21,), sg=(7,), **OBJ), SHAPE),
        ("concat_%s sg > 0, sb %% sg" % fn, lambda fn=fn: cat(fn, sb=(22,), sg=(7,), **OBJ), SHAPE),
        ("concat_%s sg > sb" % fn, lambda fn=fn: cat(fn, sb=(7,), sg=(21,), **OBJ), SHAPE),
        ("concat_%s N / rows > sb / sg" % fn, lambda fn=fn: cat(fn, sb=(14,), sg=(7,), **OBJ), SHAPE),
        ("concat_%s N / rows > sb / sg in the second source" % fn,
         lambda fn=fn: cat(fn, C=(6, 7), rows=(6, 2), sb=(96, 14), sg=(0, 7), bcast=(0, 1)), SHAPE),
    ] + [("concat_%s NULL %s" % (fn, w), lambda fn=fn, k=k: cat(fn, null_arg=k), SHAPE) for k, w in enumerate(TABLES)]
CASES += [
    ("concat_fwd NULL src[0]", lambda: cat("fwd", null_src=0), SHAPE),
    ("concat_fwd NULL src[1]", lambda: cat("fwd", null_src=1), SHAPE),
    # the backward writes a per-object gradient as the whole (rows, sb / sg, C) tensor: more objects than the batch reads
    ("concat_bwd N / rows < sb / sg with the gradient wanted", lambda: cat("bwd", sb=(28,), sg=(7,), **OBJ), SHAPE),
    ("concat_bwd N / rows < sb / sg, gradient not wanted, nothing else wanted: returns 0",
     lambda: cat("bwd", sb=(28,), sg=(7,), null_src=0, **OBJ), 0),
    # what is NOT refused and still launches nothing: no gradient wanted at all
    ("concat_bwd every dsrc[i] NULL returns 0", lambda: cat("bwd", C=(6,), rows=(6,), sb=(96,), sg=(0,), bcast=(0,), null_src=0), 0),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_pathway_entry_point_rejects_before_any_launch(call, expected):
    assert call() == expected
