"""The rejections of mogan_box_shift_sums_f64 (csrc/mogan_layout.hip), as tests/test_knn_label_rejections_cpu.py
does for mogan_knn_label_f64: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers
are dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE.  That the largest accepted sizes pass the gate is shown by the answer
changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  Then the ValueErrors of hip/ops.box_shift_sums, which
checks its host tensors before it touches the device."""
import ctypes
import re

import pytest
import torch

from helpers import ROOT, load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH = -1, -2
OK = dict(P=16, C=3, S=256, G=2)
POINTERS = ("a", "b", "edit", "others", "sums", "counts")


def shift(**kw):
    d = dict(OK, **{k: v for k, v in kw.items() if k in OK})
    ptrs = {name: kw.get(name, PTR) for name in POINTERS}
    return lib.load().mogan_box_shift_sums_f64(ptrs["a"], ptrs["b"], d["P"], d["C"], d["S"], ptrs["edit"], ptrs["others"], d["G"],
                                               ptrs["sums"], ptrs["counts"], NULL)


SHAPE_CASES = [("NULL %s" % name, {name: NULL}) for name in POINTERS] + [
    ("NULL others with G = 1", dict(others=NULL, G=1)), ("NULL others with G = 8", dict(others=NULL, G=8)),
    ("P = 0", dict(P=0)), ("P < 0", dict(P=-4)), ("P = 2^40", dict(P=1 << 40)),
    ("C = 0", dict(C=0)), ("C < 0", dict(C=-3)), ("C = 5", dict(C=5)), ("C = 2^30", dict(C=1 << 30)),
    ("S = 1", dict(S=1)), ("S = 0", dict(S=0)), ("S < 0", dict(S=-256)), ("S = 1025", dict(S=1025)), ("S = 2^30", dict(S=1 << 30)),
    ("G < 0", dict(G=-1)), ("G = 9", dict(G=9)), ("G = 2^30", dict(G=1 << 30)),
    ("P C S S = 2^31", dict(P=1 << 13, C=4, S=256)), ("P C S S = 2^31 at S = 1024", dict(P=512, C=4, S=1024)),
    ("P C S S = 3 * 2^30", dict(P=1 << 14, C=3, S=256)), ("P = 2^31 of the smallest pairs", dict(P=1 << 29, C=1, S=2)),
    ("P C S S wraps 64 bits' low half", dict(P=1 << 32, C=4, S=1024)),
    ("NULL others with G = 0 does not excuse a NULL a", dict(others=NULL, G=0, a=NULL)),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in SHAPE_CASES], ids=[c[0] for c in SHAPE_CASES])
def test_rejects_shapes_before_any_launch(kw):
    assert shift(**kw) == SHAPE


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gate():
    """the limits themselves and the smallest legal problem: not MOGAN_ERR_SHAPE; without a device the launch itself is what fails"""
    assert shift() == LAUNCH and shift(others=NULL, G=0) == LAUNCH and shift(G=8) == LAUNCH and shift(G=0) == LAUNCH
    assert shift(P=1, C=1, S=2, G=0, others=NULL) == LAUNCH and shift(C=4) == LAUNCH and shift(C=1) == LAUNCH
    assert shift(P=1, S=1024) == LAUNCH and shift(P=511, C=4, S=1024) == LAUNCH                  # 2^31 - 2^22 elements
    assert shift(P=(1 << 13) - 1, C=4, S=256) == LAUNCH and shift(P=(1 << 29) - 1, C=1, S=2) == LAUNCH


def test_the_signature_is_the_headers():
    P, L, I = lib.P, lib.L, lib.I
    assert lib.SIGNATURES["mogan_box_shift_sums_f64"] == [P, P, L, I, I, P, P, I, P, P, P]
    assert "mogan_box_shift_sums_f64" not in lib._RESTYPE
    text = open("%s/include/mogan_hip.h" % ROOT).read()
    decl = re.search(r"int mogan_box_shift_sums_f64\(([^)]*)\);", text).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(P if "*" in arg or arg.startswith("hipStream_t") else L if arg.startswith("long long") else I)
    assert kinds == lib.SIGNATURES["mogan_box_shift_sums_f64"]
    assert [" ".join(a.split()).split()[-1].lstrip("*") for a in decl.split(",")] == [
        "a", "b", "P", "C", "S", "edit", "others", "G", "sums", "counts", "stream"]


# ------------------------------------------------------------------------------------------------- the op's ValueErrors
def _args(P=2, C=3, S=16, G=1):
    a = torch.zeros((P, C, S, S))
    edit = torch.tensor([[2, 3, 6, 8, 4, -2]] * P, dtype=torch.int32)
    others = torch.zeros((P, G, 4), dtype=torch.int32)
    return a, a.clone(), edit, others


BAD_RECTANGLES = [("empty in x", [4, 3, 4, 8, 1, 1]), ("empty in y", [2, 8, 6, 8, 1, 1]), ("x1 < x0", [6, 3, 2, 8, 0, 1]),
                  ("x0 < 0", [-1, 3, 6, 8, 4, 0]), ("y0 < 0", [2, -2, 6, 8, 4, 2]), ("x1 > S", [2, 3, 17, 8, -2, 0]),
                  ("y1 > S", [2, 3, 6, 17, 0, -3]), ("moved past the left edge", [2, 3, 6, 8, -3, 0]),
                  ("moved past the top edge", [2, 3, 6, 8, 0, -4]), ("moved past the right edge", [2, 3, 6, 8, 11, 0]),
                  ("moved past the bottom edge", [2, 3, 6, 8, 0, 9]), ("an offset that wraps 32 bits", [2, 3, 6, 8, 2 ** 31 - 1, 0])]


@pytest.mark.parametrize("row", [c[1] for c in BAD_RECTANGLES], ids=[c[0] for c in BAD_RECTANGLES])
def test_the_op_refuses_a_bad_rectangle_on_the_host(row):
    a, b, edit, others = _args()
    edit[1] = torch.tensor(row, dtype=torch.int32)
    with pytest.raises(ValueError, match="edit row 1"):
        ops.box_shift_sums(a, b, edit, others)


def test_the_op_refuses_wrong_tensors_on_the_host():
    a, b, edit, others = _args()
    for args in ((a.double(), b, edit, others), (a, b.double(), edit, others), (a, b[:1], edit, others), (a[:, :, :, ::2], b, edit, others),
                 (a[0], b[0], edit, others), (a, b, edit.long(), others), (a, b, edit, others.long()), (a, b, edit.float(), others),
                 (a, b, edit[:1], others), (a, b, edit[:, :5].contiguous(), others), (a, b, edit, others[:1]), (a, b, edit, others[:, 0]),
                 (a, b, edit, torch.zeros((2, 9, 4), dtype=torch.int32)), (a, b, edit, torch.zeros((2, 1, 3), dtype=torch.int32)),
                 (a, b, edit.t().contiguous().t(), others), (a, b, edit.numpy(), others), (a.numpy(), b, edit, others),
                 (torch.zeros((2, 5, 16, 16)), torch.zeros((2, 5, 16, 16)), edit, others),
                 (torch.zeros((2, 3, 16, 8)), torch.zeros((2, 3, 16, 8)), edit, others),
                 (torch.zeros((2, 3, 1, 1)), torch.zeros((2, 3, 1, 1)), edit, others),
                 (torch.zeros((2, 3, 16, 16), device="meta"), torch.zeros((2, 3, 16, 16), device="meta"), edit, others)):
        with pytest.raises(ValueError):
            ops.box_shift_sums(*args)
    # legal host arguments reach the device gate: a host image is not the op's to upload
    with pytest.raises(lib.MoganHipError):
        ops.box_shift_sums(a, b, edit, others)
