"""The rejections of mogan_retrieval_rank (csrc/mogan_damsm.hip), as tests/test_bn_rejections_cpu.py does for the batch-norm entry
points: every case is answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that
are never dereferenced.  -1 = MOGAN_ERR_SHAPE.  That Rn = 1023 passes the shape gate is shown by the answer changing from
MOGAN_ERR_SHAPE to whatever the launch gives on this machine (0 with a GPU -- never tried here with dummy pointers -- or
MOGAN_ERR_LAUNCH without one): the case runs only where no GPU is present, the GPU module runs Rn = 1023 for real."""
import ctypes

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH = -1, -2
OK = dict(Q=4, Rn=99, C=256, N=1000)


def rank(code=PTR, pos=PTR, bank=PTR, idx=PTR, score=PTR, out=PTR, **dims):
    d = dict(OK, **dims)
    return lib.load().mogan_retrieval_rank(code, pos, bank, idx, d["Q"], d["Rn"], d["C"], d["N"], 1e-8, score, out, NULL)


CASES = [
    ("Q = 0", dict(Q=0)), ("Q < 0", dict(Q=-3)),
    ("Rn = 0", dict(Rn=0)), ("Rn < 0", dict(Rn=-1)), ("Rn = 1024", dict(Rn=1024)), ("Rn = 2^20", dict(Rn=1 << 20)),
    ("C = 0", dict(C=0)), ("C < 0", dict(C=-256)),
    ("N = 0", dict(N=0)), ("N < 0", dict(N=-1)), ("N = 2^31", dict(N=1 << 31)), ("N = 2^40", dict(N=1 << 40)),
    ("NULL code", dict(code=NULL)), ("NULL pos", dict(pos=NULL)), ("NULL bank", dict(bank=NULL)), ("NULL idx", dict(idx=NULL)),
    ("NULL rank", dict(out=NULL)),
    ("NULL rank and NULL score", dict(out=NULL, score=NULL)),
    ("Rn = 1024 at the smallest sizes", dict(Q=1, Rn=1024, C=1, N=1)),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_retrieval_rank_rejects_before_any_launch(kw):
    assert rank(**kw) == SHAPE


def test_the_signature_is_the_headers():
    assert lib.SIGNATURES["mogan_retrieval_rank"] == [lib.P, lib.P, lib.P, lib.P, lib.I, lib.I, lib.I, lib.L, lib.F, lib.P, lib.P,
                                                      lib.P]


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_shape_gate():
    """Rn = 1023, N = 2^31 - 1, a NULL score: not MOGAN_ERR_SHAPE; without a device the launch itself is what fails"""
    assert rank(Rn=1023) == LAUNCH
    assert rank(N=(1 << 31) - 1) == LAUNCH
    assert rank(score=NULL) == LAUNCH
    assert rank(Q=1, Rn=1, C=1, N=1) == LAUNCH
