"""The rejections of mogan_pk_adam_pack_both (csrc/mogan_pgemm.hip: the optimizer step of one deep convolution weight and both of its
packed copies in one pass) and of the two-part bucket step beside it (mogan_adam_prep, mogan_adam_apply; csrc/mogan_elem.hip), as
tests/test_deep_rejections_cpu.py holds those of the deep block: every case is answered by the host BEFORE any HIP call, so the
table runs without a GPU -- the data pointers are dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE.
tests/test_adam_pack_gpu.py repeats the ones that can be stated with real buffers to see that a declined call has written nothing."""
import ctypes

import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p(260)          # 4-byte aligned only
NULL = ctypes.c_void_p(None)
SHAPE = -1
GOOD = dict(Cout=64, Cin=32, KH=4, KW=4, stride=2, ph=1, pw=1)
PTRS = ("p", "g", "m", "v", "ema", "wpk_fwd", "wpk_dgrad")


def L():
    return lib.load()


def fused(null=(), odd=(), step=1, dev_state=NULL, zero_g=1, **kw):
    d = dict(GOOD, **kw)
    p = [NULL if n in null else ODD if n in odd else PTR for n in PTRS]
    return L().mogan_pk_adam_pack_both(*p, d["Cout"], d["Cin"], d["KH"], d["KW"], d["stride"], d["ph"], d["pw"], 2e-4, 0.5, 0.999,
                                       1e-8, step, dev_state, 0, 1.0, 0.999, zero_g, NULL)


def apply(null=(), odd=(), n=1000, dev_state=PTR):
    p = [NULL if k in null else ODD if k in odd else PTR for k in PTRS[:5]]
    return L().mogan_adam_apply(*p, n, 0.5, 0.999, 1e-8, dev_state, 0, 1.0, 0.999, NULL)


CASES = [("NULL " + n, lambda n=n: fused(null=(n,)), SHAPE) for n in PTRS if n != "ema"]
CASES += [("NULL " + n + ", dev_state given", lambda n=n: fused(null=(n,), dev_state=PTR), SHAPE) for n in PTRS if n != "ema"]
CASES += [("misaligned " + n, lambda n=n: fused(odd=(n,)), SHAPE) for n in PTRS]
CASES += [("step = 0 without dev_state", lambda: fused(step=0), SHAPE), ("step < 0 without dev_state", lambda: fused(step=-3), SHAPE),
          ("Cin % 32", lambda: fused(Cin=48), SHAPE), ("Cin = 16", lambda: fused(Cin=16), SHAPE), ("Cin = 0", lambda: fused(Cin=0), SHAPE),
          ("Cout % 32", lambda: fused(Cout=48), SHAPE), ("Cout = 16", lambda: fused(Cout=16), SHAPE), ("Cout = 0", lambda: fused(Cout=0), SHAPE),
          ("Cout < 0", lambda: fused(Cout=-64), SHAPE),
          ("5 x 5 taps", lambda: fused(KH=5, KW=5, stride=1, ph=2, pw=2), SHAPE),
          ("2 x 2 taps", lambda: fused(KH=2, KW=2, stride=2, ph=0, pw=0), SHAPE),
          ("6 x 6 taps", lambda: fused(KH=6, KW=6, stride=2, ph=2, pw=2), SHAPE),
          ("stride = 0", lambda: fused(stride=0), SHAPE), ("stride < 0", lambda: fused(stride=-2), SHAPE),
          ("KH % stride (3 x 3, stride 2)", lambda: fused(KH=3, KW=3, stride=2), SHAPE),
          ("zero_g = 0, Cin % 32", lambda: fused(Cin=48, zero_g=0), SHAPE),
          ("prep NULL dev_state", lambda: L().mogan_adam_prep(NULL, 2e-4, 0.5, 0.999, 0, NULL), SHAPE),
          ("apply NULL dev_state", lambda: apply(dev_state=NULL), SHAPE), ("apply n = 0", lambda: apply(n=0), SHAPE),
          ("apply n < 0", lambda: apply(n=-4), SHAPE)]
CASES += [("apply NULL " + n, lambda n=n: apply(null=(n,)), SHAPE) for n in PTRS[:4]]
CASES += [("apply misaligned " + n, lambda n=n: apply(odd=(n,)), SHAPE) for n in PTRS[:5]]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_the_prototypes():
    P, I, F, Lg = lib.P, lib.I, lib.F, lib.L
    assert lib.SIGNATURES["mogan_pk_adam_pack_both"] == [P] * 7 + [I] * 7 + [F] * 4 + [I, P, I, F, F, I, P]
    assert lib.SIGNATURES["mogan_adam_prep"] == [P, F, F, F, I, P]
    assert lib.SIGNATURES["mogan_adam_apply"] == [P] * 5 + [Lg, F, F, F, P, I, F, F, P]


def test_the_good_arguments_have_both_panels():
    """what every row above changes one thing of: a weight both panel formats take (the three test weights of
    tests/test_adam_pack_gpu.py among them)"""
    wb = L().mogan_pk_weight_bytes
    for Cout, Cin, KH, KW, s in ((64, 32, 4, 4, 2), (32, 64, 3, 3, 1), (64, 32, 1, 1, 1)):
        assert wb(Cout, Cin, KH, KW, s, 0) == Cout * Cin * KH * KW * 6 and wb(Cout, Cin, KH, KW, s, 1) == Cout * Cin * KH * KW * 6


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_adam_pack_rejects_before_any_launch(call, expected):
    assert call() == expected
