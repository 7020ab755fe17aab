"""The rejections of the pooling, resize, sum and feeder entry points of libmogan_hip.so (csrc/mogan_elem.hip: mogan_add, mogan_scale,
mogan_group_sum, mogan_group_bcast, mogan_maxpool_*, mogan_avgpool_*, mogan_bilinear_*, and beside them mogan_relu_bwd,
mogan_copy_strided, mogan_down2_sum; csrc/mogan_feed.hip: mogan_feed_crop_flip, mogan_feed_resample), as
tests/test_bn_rejections_cpu.py holds those of the batch-norm family: every case is answered by the host BEFORE any HIP call, so
the table runs without a GPU -- the pointers are dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE.  Every row changes
one thing (or what its name says) of arguments the entry point takes; tests/test_pool_entry_points_gpu.py runs those arguments
and repeats some of the rows with real buffers to see that a declined call has written nothing.

The average pool's rows with s = 0 are answered before anything is divided: an integer division by zero on the host would end
the process, not fail a row.  The crop offsets of mogan_feed_crop_flip live on the device and are the caller's contract
(0 <= h1, w1 <= ori - size; attngan/feeder.draw_crop keeps it): no row here."""
import ctypes

import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE = -1

# entry point -> ((argument, a value the entry point takes), ...) in the order of the prototype, the stream left out;
# a value of PTR marks a pointer; NULLABLE: the pointers that may be NULL
GOOD = {
    "mogan_add": (("a", PTR), ("b", PTR), ("y", PTR), ("n", 1000)),
    "mogan_scale": (("a", PTR), ("alpha", 0.5), ("y", PTR), ("n", 1000)),
    "mogan_group_sum": (("x", PTR), ("y", PTR), ("n", 1000), ("G", 3)),
    "mogan_group_bcast": (("dy", PTR), ("dx", PTR), ("n", 1000), ("G", 3)),
    "mogan_maxpool_fwd": (("x", PTR), ("y", PTR), ("idx", PTR), ("planes", 5), ("H", 10), ("W", 9), ("k", 3), ("s", 2)),
    "mogan_maxpool_fwd_ex": (("x", PTR), ("y", PTR), ("y_bstride", -1), ("idx", PTR), ("B", 2), ("C", 5), ("H", 10), ("W", 9), ("k", 3),
                             ("s", 2)),
    "mogan_maxpool_bwd": (("idx", PTR), ("dy", PTR), ("dx", PTR), ("planes", 5), ("H", 10), ("W", 9), ("k", 3), ("s", 2)),
    "mogan_maxpool_bwd_ex": (("idx", PTR), ("dy", PTR), ("dy_bstride", -1), ("dx", PTR), ("relu_of", PTR), ("accumulate", 0), ("B", 2),
                             ("C", 5), ("H", 10), ("W", 9), ("k", 3), ("s", 2)),
    "mogan_avgpool_fwd": (("x", PTR), ("y", PTR), ("planes", 7), ("H", 11), ("W", 6), ("k", 3), ("s", 2), ("pad", 1)),
    "mogan_avgpool_bwd": (("dy", PTR), ("dx", PTR), ("planes", 7), ("H", 11), ("W", 6), ("k", 3), ("s", 2), ("pad", 1)),
    "mogan_avgpool_bwd_ex": (("dy", PTR), ("dx", PTR), ("relu_of", PTR), ("accumulate", 0), ("planes", 7), ("H", 11), ("W", 6), ("k", 3),
                             ("s", 2), ("pad", 1)),
    "mogan_bilinear_fwd": (("x", PTR), ("y", PTR), ("planes", 6), ("H", 6), ("W", 7), ("OH", 7), ("OW", 9)),
    "mogan_bilinear_bwd": (("dy", PTR), ("dx", PTR), ("planes", 6), ("H", 6), ("W", 7), ("OH", 7), ("OW", 9)),
    "mogan_relu_bwd": (("z", PTR), ("dz", PTR), ("dx", PTR), ("n", 1000), ("accumulate", 0)),
    "mogan_copy_strided": (("src", PTR), ("src_bstride", 64), ("dst", PTR), ("dst_bstride", 96), ("B", 3), ("n", 48)),
    "mogan_down2_sum": (("du", PTR), ("dx", PTR), ("planes", 4), ("H", 5), ("W", 6)),
    "mogan_feed_crop_flip": (("src", PTR), ("params", PTR), ("q", PTR), ("out", PTR), ("B", 3), ("ori", 11), ("size", 8)),
    "mogan_feed_resample": (("in", PTR), ("tmp", PTR), ("out", PTR), ("bounds", PTR), ("kk", PTR), ("ksize", 7), ("B", 5), ("S", 12),
                            ("OS", 5)),
}
NULLABLE = {"mogan_maxpool_fwd": ("idx",), "mogan_maxpool_fwd_ex": ("idx",), "mogan_maxpool_bwd_ex": ("relu_of",),
            "mogan_avgpool_bwd_ex": ("relu_of",)}
SUMS = ("mogan_add", "mogan_scale", "mogan_group_sum", "mogan_group_bcast")
MAXPOOLS = ("mogan_maxpool_fwd", "mogan_maxpool_fwd_ex", "mogan_maxpool_bwd", "mogan_maxpool_bwd_ex")
AVGPOOLS = ("mogan_avgpool_fwd", "mogan_avgpool_bwd", "mogan_avgpool_bwd_ex")


def L():
    return lib.load()


def run(name, **change):
    """the entry point with its good arguments, `change` applied (a pointer's name: None = NULL), on the NULL stream"""
    assert set(change) <= {k for k, _ in GOOD[name]}, (name, change)
    args = [(NULL if change[k] is None else change[k]) if k in change else v for k, v in GOOD[name]]
    return getattr(L(), name)(*args, NULL)


def pointers(name):
    return [k for k, v in GOOD[name] if v is PTR]


def short(name):
    return name[len("mogan_"):]


CASES = []


def row(name, what, expected=SHAPE, **change):
    CASES.append(("%s %s" % (short(name), what), lambda: run(name, **change), expected))


# every pointer that is not nullable
for name_ in GOOD:
    for p_ in pointers(name_):
        if p_ not in NULLABLE.get(name_, ()):
            row(name_, "NULL " + p_, **{p_: None})
# the sums: an empty tensor is answered first, with 0, whatever else is wrong with the call (its pointer is NULL)
for name_ in SUMS:
    row(name_, "n = 0 is 0", 0, n=0)
    row(name_, "n = 0 and NULL pointers is 0", 0, n=0, **{p_: None for p_ in pointers(name_)})
    row(name_, "n < 0", n=-4)
    row(name_, "n < 0 and NULL pointers", n=-1, **{p_: None for p_ in pointers(name_)})
for name_ in ("mogan_group_sum", "mogan_group_bcast"):
    row(name_, "G = 0", G=0)
    row(name_, "G < 0", G=-2)
    row(name_, "n = 0 and G = 0 is 0", 0, n=0, G=0)
    row(name_, "n < 0 and G = 0", n=-3, G=0)
# max pool: planes, window, stride, a map smaller than the window, offsets that do not fit a byte; backward: k <= 2 s
for name_ in MAXPOOLS:
    for dim_ in (("B", "C") if name_.endswith("_ex") else ("planes",)):
        row(name_, dim_ + " = 0", **{dim_: 0})
        row(name_, dim_ + " < 0", **{dim_: -3})
    row(name_, "k = 0", k=0)
    row(name_, "k < 0", k=-3)
    row(name_, "s = 0", s=0)
    row(name_, "s < 0", s=-2)
    row(name_, "H < k", H=2)
    row(name_, "W < k", W=2)
    row(name_, "H = 0", H=0)
    row(name_, "W < 0", W=-9)
    row(name_, "k * k = 256", H=40, W=40, k=16, s=8)
    row(name_, "k * k > 255 and k > 2 s", H=40, W=40, k=17, s=2)
for name_ in ("mogan_maxpool_bwd", "mogan_maxpool_bwd_ex"):
    row(name_, "k > 2 s", k=3, s=1)
    row(name_, "k = 5, s = 1 (the forward-only row)", H=9, W=9, k=5, s=1)
# average pool: window and stride before anything is divided, padding as torch accepts it, a padded map smaller than the window
for name_ in AVGPOOLS:
    row(name_, "planes = 0", planes=0)
    row(name_, "planes < 0", planes=-7)
    row(name_, "s = 0", s=0)
    row(name_, "s = 0 and k = 0", s=0, k=0)
    row(name_, "s < 0", s=-1)
    row(name_, "k = 0", k=0)
    row(name_, "k < 0", k=-3)
    row(name_, "pad < 0", pad=-1)
    row(name_, "2 pad > k", pad=2)
    row(name_, "2 pad > k, k = 1", k=1, s=1, pad=1)
    row(name_, "H = 0", H=0)
    row(name_, "H < 0", H=-11)
    row(name_, "W = 0", W=0)
    row(name_, "W < 0", W=-6)
    # C's truncating division gives (2 - 3) / 2 + 1 = 1 output row where the floor division of the callers gives 0
    row(name_, "H + 2 pad < k, s = 2 (truncating division)", H=2, W=8, k=3, s=2, pad=0)
    row(name_, "W + 2 pad < k, s = 2 (truncating division)", H=8, W=2, k=3, s=2, pad=0)
    row(name_, "H + 2 pad < k, s = 1", H=2, W=8, k=5, s=1, pad=1)
    row(name_, "W + 2 pad < k, s = 3", H=8, W=1, k=4, s=3, pad=1)
for name_ in ("mogan_bilinear_fwd", "mogan_bilinear_bwd"):
    for dim_ in ("planes", "H", "W", "OH", "OW"):
        row(name_, dim_ + " = 0", **{dim_: 0})
        row(name_, dim_ + " < 0", **{dim_: -5})
row("mogan_relu_bwd", "n = 0", n=0)
row("mogan_relu_bwd", "n < 0", n=-1)
for dim_ in ("B", "n"):
    row("mogan_copy_strided", dim_ + " = 0", **{dim_: 0})
    row("mogan_copy_strided", dim_ + " < 0", **{dim_: -2})
for dim_ in ("planes", "H", "W"):
    row("mogan_down2_sum", dim_ + " = 0", **{dim_: 0})
    row("mogan_down2_sum", dim_ + " < 0", **{dim_: -2})
for dim_ in ("B", "size"):
    row("mogan_feed_crop_flip", dim_ + " = 0", **{dim_: 0})
    row("mogan_feed_crop_flip", dim_ + " < 0", **{dim_: -8})
row("mogan_feed_crop_flip", "ori < size", ori=7)
for dim_ in ("B", "S", "OS", "ksize"):
    row("mogan_feed_resample", dim_ + " = 0", **{dim_: 0})
    row("mogan_feed_resample", dim_ + " < 0", **{dim_: -3})


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_the_prototypes():
    P, I, F, Lg = lib.P, lib.I, lib.F, lib.L
    want = {
        "mogan_add": [P, P, P, Lg, P], "mogan_scale": [P, F, P, Lg, P], "mogan_group_sum": [P, P, Lg, I, P],
        "mogan_group_bcast": [P, P, Lg, I, P],
        "mogan_maxpool_fwd": [P, P, P] + [I] * 5 + [P], "mogan_maxpool_bwd": [P, P, P] + [I] * 5 + [P],
        "mogan_maxpool_fwd_ex": [P, P, Lg, P] + [I] * 6 + [P], "mogan_maxpool_bwd_ex": [P, P, Lg, P, P] + [I] * 7 + [P],
        "mogan_avgpool_fwd": [P, P] + [I] * 6 + [P], "mogan_avgpool_bwd": [P, P] + [I] * 6 + [P],
        "mogan_avgpool_bwd_ex": [P, P, P] + [I] * 7 + [P],
        "mogan_bilinear_fwd": [P, P] + [I] * 5 + [P], "mogan_bilinear_bwd": [P, P] + [I] * 5 + [P],
        "mogan_relu_bwd": [P, P, P, Lg, I, P], "mogan_copy_strided": [P, Lg, P, Lg, I, Lg, P], "mogan_down2_sum": [P, P, I, I, I, P],
        "mogan_feed_crop_flip": [P, P, P, P, I, I, I, P], "mogan_feed_resample": [P] * 5 + [I] * 4 + [P],
    }
    assert set(want) == set(GOOD)
    for name, sig in want.items():
        assert lib.SIGNATURES[name] == sig, name
        kinds = [P if v is PTR else F if isinstance(v, float) else None for _, v in GOOD[name]] + [P]
        assert len(kinds) == len(sig) and all(k is None or k is s for k, s in zip(kinds, sig)), name


def test_the_good_arguments_are_rows_of_the_tables():
    """what every row above changes one thing of is a call the GPU module makes (tests/pool_cases.py)"""
    import pool_cases as K
    d = {k: dict(v) for k, v in GOOD.items()}
    assert tuple(d["mogan_maxpool_fwd"][k] for k in ("planes", "H", "W", "k", "s")) in K.MAX_ROWS
    assert tuple(d["mogan_maxpool_bwd"][k] for k in ("planes", "H", "W", "k", "s")) in K.MAX_ROWS
    for name in AVGPOOLS:
        assert tuple(d[name][k] for k in ("planes", "H", "W", "k", "s", "pad")) in K.AVG_ROWS
    for name in ("mogan_bilinear_fwd", "mogan_bilinear_bwd"):
        assert tuple(d[name][k] for k in ("planes", "H", "W", "OH", "OW")) in K.BIL_ROWS
    assert tuple(d["mogan_feed_crop_flip"][k] for k in ("B", "ori", "size")) in [r[0] for r in K.CROP_ROWS]
    assert tuple(d["mogan_feed_resample"][k] for k in ("B", "S", "OS")) in K.RESAMPLE_ROWS
    assert K.MAX_FWD_ONLY[3] > 2 * K.MAX_FWD_ONLY[4]


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_pool_entry_point_rejects_before_any_launch(call, expected):
    assert call() == expected
