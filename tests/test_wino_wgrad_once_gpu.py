"""-m gpu: the Winograd weight gradient (csrc/mogan_wino.hip: wino_wgrad_kernel + wino_wgrad_finish), whose blocks each own one
row of the 4 x 4 transform positions for 96 co x 96 ci, through ops.conv2d_wgrad on the smallest shapes at which its tiling can
go wrong.

Reference: the weight gradient of torch.nn.functional.conv2d in float64 on the CPU copies of the same tensors.
Tolerance: the one tests/test_kernels_gpu.py::test_conv2d_fwd_dgrad_wgrad applies to weight gradients (its _check): rel-L2 over
the whole tensor <= 2e-6; with accumulate the expected tensor is base + gradient, as test_upsample_conv3x3_both_formulations
checks its accumulation.
That the launch took the Winograd path is read from the measurement hook (mogan_prof_enable / mogan_prof_collect: a row with
mode 6 = weight gradient off the implicit GEMM, cfg 1 = Winograd), as tests/test_conv_entry_points_gpu.py does."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 2e-6          # tests/test_kernels_gpu.py::_check

# (Cin, Cout, B, H, W).  Input channels in multiples of 96 take the position-row block, the others (cases 3-5) the 96 x 32 block,
# where the "skipped" ci tile is a ci block that does not exist.
CASES = [
    (96, 96, 2, 16, 16),        # the step's tiling
    (96, 192, 2, 16, 16),       # the step's tiling, two co blocks
    (64, 96, 2, 4, 16),         # a skipped ci tile
    (128, 160, 1, 4, 32),       # second ci block and last co block partial
    (32, 64, 1, 2, 16),         # one chunk; an unpaired last chunk
    (96, 96, 3, 6, 48),         # chunk count (27) not a multiple of the chunks per split (9)
    (96, 160, 1, 4, 32),        # position-row block: last co block partial, with an empty 32-wide co tile
    (192, 96, 1, 2, 16),        # position-row block: second ci block
]


@pytest.fixture(scope="module", autouse=True)
def _launch_records():
    """the measurement hook is process-wide: on for this module only"""
    lib.load().mogan_prof_enable(1)
    yield
    lib.load().mogan_prof_enable(0)


def _rows():
    buf = (ctypes.c_double * (5 * 64))()
    n = lib.load().mogan_prof_collect(buf, 64)
    return {(int(buf[5 * i]), int(buf[5 * i + 1])) for i in range(n)}


def _seeded(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _ref_wgrad(dy, x, w_shape):
    w = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, 1, 1).backward(dy.double())
    return w.grad


@functools.lru_cache(maxsize=None)
def _case(case):
    Cin, Cout, B, H, W = case
    x, dy = _seeded(11, (B, Cin, H, W)), _seeded(12, (B, Cout, H, W))
    base = _seeded(13, (Cout, Cin, 3, 3))
    return x, dy, base, _ref_wgrad(dy, x, (Cout, Cin, 3, 3))


def _run(dy, x, w_shape, base=None):
    """ops.conv2d_wgrad into a fresh buffer (accumulate: pre-filled with base); asserts that the Winograd kernel ran"""
    out = base.to(DEV).clone() if base is not None else torch.full(w_shape, float("nan"), device=DEV)
    _rows()
    ops.conv2d_wgrad(dy.to(DEV), x.to(DEV), w_shape, 1, 1, 1, 0, out=out, accumulate=base is not None)
    torch.cuda.synchronize()
    rows = _rows()
    assert (6, 1) in rows, "not the Winograd weight gradient: launch records %s" % sorted(rows)
    return out.cpu()


def _check(got, ref, what):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), "%s: non-finite values" % what
    rel = (got - ref).norm().item() / (ref.norm().item() + 1e-30)
    mx = (got - ref).abs().max().item()
    print("%s: rel-L2 %.3e max-abs %.3e" % (what, rel, mx))
    assert rel <= RTOL, "%s: rel-L2 %.3e > %.1e (max-abs %.3e)" % (what, rel, RTOL, mx)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_wgrad_vs_fp64(case, accumulate):
    Cin, Cout, B, H, W = case
    x, dy, base, ref = _case(case)
    got = _run(dy, x, (Cout, Cin, 3, 3), base if accumulate else None)
    _check(got, ref + base.double() if accumulate else ref, "%s accumulate=%s" % (case, accumulate))


def test_same_bits_run_to_run():
    case = CASES[5]
    Cin, Cout, B, H, W = case
    x, dy, base, ref = _case(case)
    a = _run(dy, x, (Cout, Cin, 3, 3))
    b = _run(dy, x, (Cout, Cin, 3, 3))
    assert torch.equal(a, b)


@pytest.mark.parametrize("corner", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_single_element_at_an_image_corner(corner):
    """dY and x with one non-zero element each, at the same corner of the last image: only dW[co, ci, 1, 1] is non-zero; and
    with dY's element one pixel inwards on the diagonal, only the tap that points from it to the corner"""
    Cin, Cout, B, H, W = 96, 96, 2, 16, 32
    cy, cx = corner
    py, px = cy * (H - 1), cx * (W - 1)
    iy, ix = py + (1 - 2 * cy), px + (1 - 2 * cx)
    for qy, qx in ((py, px), (iy, ix)):
        x = torch.zeros(B, Cin, H, W)
        dy = torch.zeros(B, Cout, H, W)
        x[B - 1, 37, py, px] = 1.5
        dy[B - 1, 70, qy, qx] = -2.25
        ref = _ref_wgrad(dy, x, (Cout, Cin, 3, 3))
        kh, kw = py - qy + 1, px - qx + 1
        assert ref[70, 37, kh, kw].item() == -3.375 and int((ref != 0).sum()) == 1
        got = _run(dy, x, (Cout, Cin, 3, 3))
        _check(got, ref, "corner %s dY at %s" % (corner, (qy, qx)))
