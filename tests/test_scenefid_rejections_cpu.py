"""The rejections of mogan_roi_resize (csrc/mogan_roi.hip), as tests/test_msssim_rejections_cpu.py does for the MS-SSIM entries: every
case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that are never
dereferenced.  -1 = MOGAN_ERR_SHAPE.  That the largest accepted sizes pass the gate is shown by the answer changing to
MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  ops.roi_resize refuses what it would have to convert and what its
host-side look at the index and the boxes finds."""
import ctypes
import re

import pytest
import torch

from helpers import ROOT, load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

PTR, PTR2, PTR3, PTR4 = (ctypes.c_void_p(v) for v in (256, 512, 1024, 2048))     # non-null, aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH = -1, -2


def L():
    return lib.load()


def roi(x=PTR, boxes=PTR2, index=PTR3, y=PTR4, B=2, C=3, H=33, W=40, R=5, OH=19, OW=23):
    return L().mogan_roi_resize(x, B, C, H, W, boxes, index, R, y, OH, OW, NULL)


TABLE = [("NULL x", dict(x=NULL)), ("NULL boxes", dict(boxes=NULL)), ("NULL image_index", dict(index=NULL)), ("NULL y", dict(y=NULL)),
         ("NULL x with R = 0", dict(x=NULL, R=0)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-2)), ("H = 0", dict(H=0)),
         ("H < 0", dict(H=-33)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-40)), ("OH = 0", dict(OH=0)), ("OH < 0", dict(OH=-19)),
         ("OW = 0", dict(OW=0)), ("OW < 0", dict(OW=-23)), ("OH = 0 with R = 0", dict(OH=0, R=0)), ("C = 0", dict(C=0)),
         ("C = 5", dict(C=5)), ("C < 0", dict(C=-3)), ("R < 0", dict(R=-1)),
         ("B C H W = 2^31", dict(B=1 << 13, C=4, H=256, W=256)), ("H W = 2^31", dict(B=1, C=1, H=1 << 16, W=1 << 15)),
         ("H W above 2^32", dict(B=1, C=1, H=1 << 17, W=1 << 17)), ("B C H W above 2^64", dict(B=1 << 30, C=4, H=1 << 15, W=1 << 15)),
         ("R C OH OW = 2^31", dict(R=1 << 13, C=4, OH=256, OW=256)), ("OH OW = 2^31", dict(R=1, C=1, OH=1 << 16, OW=1 << 15)),
         ("R = 2^31", dict(R=1 << 31, C=1, OH=1, OW=1)), ("R = 2^62", dict(R=1 << 62, C=4, OH=2, OW=2))]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [t[1] for t in TABLE], ids=[t[0] for t in TABLE])
def test_rejects_shapes_before_any_launch(kw):
    assert roi(**kw) == SHAPE


def test_no_object_is_no_launch():
    assert roi(R=0) == 0 and roi(R=0, B=1, C=1, H=1, W=1, OH=1, OW=1) == 0
    assert roi(R=0, OH=1 << 16, OW=1 << 16) == 0                       # an empty y of any row size


def test_the_signature_is_the_headers():
    P, I, Lg = lib.P, lib.I, lib.L
    assert lib.SIGNATURES["mogan_roi_resize"] == [P, I, I, I, I, P, P, Lg, P, I, I, P]
    header = open("%s/include/mogan_hip.h" % ROOT).read()
    m = re.search(r"\nint mogan_roi_resize\(([^;]*)\);", header)
    assert m, "mogan_roi_resize is not declared in include/mogan_hip.h"
    kinds = {"const float*": P, "float*": P, "const int*": P, "int": I, "long long": Lg, "hipStream_t": P}
    args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
    assert [kinds[a] for a in args] == lib.SIGNATURES["mogan_roi_resize"]
    assert L().mogan_roi_resize.restype is ctypes.c_int


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gate():
    """the limits themselves and the smallest legal problem: not MOGAN_ERR_SHAPE; without a device the launch itself is what fails"""
    assert roi() == LAUNCH and roi(B=1, C=1, H=1, W=1, R=1, OH=1, OW=1) == LAUNCH and roi(C=4) == LAUNCH
    assert roi(B=(1 << 13) - 1, C=4, H=256, W=256) == LAUNCH and roi(B=1, C=1, H=(1 << 16) - 1, W=1 << 15) == LAUNCH
    assert roi(R=(1 << 13) - 1, C=4, OH=256, OW=256) == LAUNCH and roi(R=(1 << 31) - 1, C=1, OH=1, OW=1) == LAUNCH
    assert roi(x=PTR, y=PTR) == LAUNCH


def test_the_op_refuses_what_it_would_have_to_convert():
    x = torch.zeros(2, 3, 8, 8)
    boxes = torch.tensor([[0.1, 0.1, 0.5, 0.5], [-1, -1, -1, -1], [0.0, 0.0, 1.0, 1.0]])
    index = torch.tensor([0, 1, 1], dtype=torch.int32)
    out = torch.zeros(3, 3, 5, 4)
    nan, inf = boxes.clone(), boxes.clone()
    nan[1, 2], inf[0, 0] = float("nan"), float("inf")
    wide = torch.zeros(3, 8)
    for args, kw in (((x.double(), boxes, index), {}), ((x[0], boxes, index), {}), ((x[:, :, :, ::2], boxes, index), {}),
                     ((x.numpy(), boxes, index), {}), ((x.to("meta"), boxes, index), {}), ((torch.zeros(2, 5, 8, 8), boxes, index), {}),
                     ((x, boxes.double(), index), {}), ((x, boxes.numpy(), index), {}), ((x, boxes.to("meta"), index), {}),
                     ((x, boxes[:, :3], index), {}), ((x, wide[:, ::2], index), {}), ((x, boxes.view(-1), index), {}),
                     ((x, boxes[:2], index), {}), ((x, boxes.tolist(), index), {}),
                     ((x, boxes, index.float()), {}), ((x, boxes, index.to(torch.int16)), {}), ((x, boxes, index.numpy()), {}),
                     ((x, boxes, index.to("meta")), {}), ((x, boxes, index.view(3, 1)), {}), ((x, boxes, torch.zeros(6, dtype=torch.int32)[::2]), {}),
                     ((x, boxes, [0, 1, 1]), {}),
                     ((x, boxes, torch.tensor([0, 2, 1], dtype=torch.int32)), {}), ((x, boxes, torch.tensor([0, -1, 1])), {}),
                     ((x, nan, index), {}), ((x, inf, index), {}),
                     ((x, boxes, index), dict(out=out.double())), ((x, boxes, index), dict(out=torch.zeros(3, 3, 5, 5))),
                     ((x, boxes, index), dict(out=torch.zeros(3, 3, 5, 8)[:, :, :, ::2])), ((x, boxes, index), dict(out=out.numpy())),
                     ((x, boxes, index), dict(out=out.to("meta"))), ((x, boxes, index), dict(out=torch.zeros(4, 3, 5, 4)))):
        with pytest.raises(ValueError):
            ops.roi_resize(*args, 5, 4, **kw)
    for OH, OW in ((0, 4), (5, 0), (-5, 4)):
        with pytest.raises(ValueError):
            ops.roi_resize(x, boxes, index, OH, OW)
    # legal host tensors, int32 and int64 index, with and without out, no object at all: nothing left to object to but the
    # device -- there is no CPU path
    for idx, kw in ((index, {}), (index.long(), {}), (index, dict(out=out)), (index[:0], {}), (index, dict(out=torch.zeros(5, 3, 5, 4)[:3]))):
        with pytest.raises(lib.MoganHipError, match="no CPU path"):
            ops.roi_resize(x, boxes[:len(idx)], idx, 5, 4, **kw)
