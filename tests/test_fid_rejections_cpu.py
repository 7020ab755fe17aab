"""The rejections of mogan_col_mean_f64 and mogan_cov_f64 (csrc/mogan_stats.hip), as tests/test_retrieval_rejections_cpu.py does for
the ranking entry point: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are
dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE.  That the largest accepted sizes pass the shape gate is shown by the
answer changing from MOGAN_ERR_SHAPE to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH = -1, -2
OK = dict(N=30000, D=2048)


def mean(x=PTR, out=PTR, **dims):
    d = dict(OK, **dims)
    return lib.load().mogan_col_mean_f64(x, d["N"], d["D"], out, NULL)


def cov(x=PTR, mu=PTR, out=PTR, **dims):
    d = dict(OK, **dims)
    return lib.load().mogan_cov_f64(x, mu, d["N"], d["D"], out, NULL)


COV_CASES = [
    ("N = 1", dict(N=1)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-5)), ("N = 2^31", dict(N=1 << 31)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("NULL x", dict(x=NULL)), ("NULL mean", dict(mu=NULL)), ("NULL cov", dict(out=NULL)),
    ("N = 1 at the smallest width", dict(N=1, D=1)),
]
MEAN_CASES = [
    ("N = 0", dict(N=0)), ("N < 0", dict(N=-5)), ("N = 2^31", dict(N=1 << 31)), ("N = 2^40", dict(N=1 << 40)),
    ("D = 0", dict(D=0)), ("D < 0", dict(D=-2048)), ("D = 65537", dict(D=65537)), ("D = 2^30", dict(D=1 << 30)),
    ("NULL x", dict(x=NULL)), ("NULL mean", dict(out=NULL)),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in COV_CASES], ids=[c[0] for c in COV_CASES])
def test_cov_rejects_before_any_launch(kw):
    assert cov(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in MEAN_CASES], ids=[c[0] for c in MEAN_CASES])
def test_col_mean_rejects_before_any_launch(kw):
    assert mean(**kw) == SHAPE


def test_the_signatures_are_the_headers():
    assert lib.SIGNATURES["mogan_col_mean_f64"] == [lib.P, lib.L, lib.I, lib.P, lib.P]
    assert lib.SIGNATURES["mogan_cov_f64"] == [lib.P, lib.P, lib.L, lib.I, lib.P, lib.P]


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_shape_gate():
    """N = 2^31 - 1, D = 65536, the smallest shapes: not MOGAN_ERR_SHAPE; without a device the launch itself is what fails"""
    assert cov(N=(1 << 31) - 1) == LAUNCH and mean(N=(1 << 31) - 1) == LAUNCH
    assert cov(D=65536) == LAUNCH and mean(D=65536) == LAUNCH
    assert cov(N=2, D=1) == LAUNCH and mean(N=1, D=1) == LAUNCH
