"""The rejections of the entry points at the end of the train step -- the logits head (csrc/mogan_smallc.hip), the BCE / KL /
reparametrisation losses and the Adam step (csrc/mogan_elem.hip), the DAMSM matching losses and the scalar sums
(csrc/mogan_damsm.hip) -- as tests/test_pathway_rejections_cpu.py does for the object pathway: every case is answered by the host
BEFORE any HIP call, so the table runs without a GPU -- the data pointers are dummies that are never dereferenced (the small host
arrays of mogan_scalar_sum / _scale are real: the host reads them).
-1 = MOGAN_ERR_SHAPE.  A NULL in a nullable place (bias, dx / dw / db, wt, mask, g0, g1, ema, dev_state) is no rejection: the GPU
module tests/test_loss_entry_points_gpu.py runs those, and the one rejection that used to reach a launch (a misaligned Adam
bucket WITH a device counter) lives there too, where the counter can be read back."""
import ctypes

import pytest

import loss_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
OFF = ctypes.c_void_p(260)          # one float off 16-byte alignment
NULL = ctypes.c_void_p(None)
SHAPE = -1
G = K.GAMMAS


def L():
    return lib.load()


def _ptrs(n, null_at=None, at=None, val=None):
    return [NULL if i == null_at else (val if i == at else PTR) for i in range(n)]


def head_fwd(B=2, Kd=8, Cout=1, null_at=None, off_at=None):
    x, w, bias, p = _ptrs(4, null_at, off_at, OFF)
    return L().mogan_logits_head_fwd(x, w, bias, p, B, Kd, Cout, NULL)


def head_bwd(B=2, Kd=8, Cout=1, null_at=None):
    return L().mogan_logits_head_bwd(*_ptrs(7, null_at), B, Kd, Cout, 0, NULL)


def elem(fn, n=16, null_at=None):
    """the BCE / BCE-with-logits / KL / reparametrisation entries by name"""
    f = getattr(L(), "mogan_" + fn)
    if fn in ("bce_fwd", "bce_logits_fwd"):
        a, b = _ptrs(2, null_at)
        return f(a, 1.0, 1.0, b, n, 0, NULL)
    if fn in ("bce_bwd", "bce_logits_bwd"):
        a, b, c = _ptrs(3, null_at)
        return f(a, 1.0, 1.0, b, c, n, NULL)
    return f(*_ptrs(ELEM_PTRS[fn], null_at), n, NULL)


ELEM_PTRS = {"bce_fwd": 2, "bce_bwd": 3, "bce_logits_fwd": 2, "bce_logits_bwd": 3, "kl_fwd": 3, "kl_bwd": 5, "reparam_fwd": 4,
             "reparam_bwd": 5}
ELEM_NAMES = {"bce_fwd": ("p", "loss"), "bce_bwd": ("p", "gout", "dp"), "bce_logits_fwd": ("x", "loss"),
              "bce_logits_bwd": ("x", "gout", "dx"), "kl_fwd": ("mu", "logvar", "loss"),
              "kl_bwd": ("mu", "logvar", "gout", "dmu", "dlogvar"), "reparam_fwd": ("mu", "logvar", "eps", "c"),
              "reparam_bwd": ("logvar", "eps", "dc", "dmu", "dlogvar")}
WORDS_GOOD = dict(B=2, Bc=3, C=10, S=36, T=7)


def words_fwd(null_at=None, **kw):
    d = dict(WORDS_GOOD, **kw)
    ctx, words, lens, sim, a1, a2, wc, wt = _ptrs(8, null_at)
    return L().mogan_damsm_words_fwd(ctx, words, lens, d["B"], d["Bc"], d["C"], d["S"], d["T"], *G, sim, a1, a2, wc, wt, NULL)


def words_bwd(null_at=None, **kw):
    d = dict(WORDS_GOOD, **kw)
    p = _ptrs(9, null_at)
    return L().mogan_damsm_words_bwd(*p[:7], d["B"], d["Bc"], d["C"], d["S"], d["T"], *G, p[7], p[8], NULL)


def ce_fwd(R=5, Q=5, null_at=None):
    sim, lab, mask, prow, pcol, nll, out2 = _ptrs(7, null_at)
    return L().mogan_damsm_ce_fwd(sim, lab, mask, R, Q, prow, pcol, nll, out2, NULL)


def ce_bwd(R=5, Q=5, null_at=None):
    prow, pcol, lab, g0, g1, dsim = _ptrs(6, null_at)
    return L().mogan_damsm_ce_bwd(prow, pcol, lab, g0, g1, R, Q, dsim, NULL)


def sent_fwd(B=3, Bc=5, C=10, null_at=None):
    cnn, rnn, sim = _ptrs(3, null_at)
    return L().mogan_damsm_sent_fwd(cnn, rnn, B, Bc, C, G[2], 1e-8, sim, NULL)


def sent_bwd(B=3, Bc=5, C=10, null_at=None):
    cnn, rnn, dsim, dcnn = _ptrs(4, null_at)
    return L().mogan_damsm_sent_bwd(cnn, rnn, dsim, B, Bc, C, G[2], 1e-8, dcnn, NULL)


def scalar(fn, n=3, null_arg=None, null_entry=None):
    """mogan_scalar_sum / _scale with real host tables; null_arg: 0 the pointer table, 1 weights, 2 the device scalar (out / g);
    null_entry: which in[k] / out[k] is NULL"""
    tab = (ctypes.c_void_p * 9)(*[None if k == null_entry else 256 * (k + 1) for k in range(9)])
    w = (ctypes.c_float * 9)(*([1.0] * 9))
    a = [NULL if i == null_arg else v for i, v in enumerate((ctypes.cast(tab, ctypes.c_void_p), ctypes.cast(w, ctypes.c_void_p), PTR))]
    if fn == "sum":
        return L().mogan_scalar_sum(a[0], a[1], n, a[2], NULL)
    return L().mogan_scalar_scale(a[2], a[1], n, a[0], NULL)


def adam(n=16, step=1, null_at=None, off_at=None, dev_state=NULL):
    p, g, m, v, ema = _ptrs(5, null_at, off_at, OFF)
    return L().mogan_adam_step(p, g, m, v, ema, n, 2e-4, 0.5, 0.999, 1e-8, step, dev_state, 0, 1.0, 0.999, NULL)


CASES = []
for fn, call, names, nullable in (("logits_head_fwd", head_fwd, ("x", "w", "bias", "p"), {2}),
                                  ("logits_head_bwd", head_bwd, ("dp", "p", "x", "w", "dx", "dw", "db"), {4, 5, 6})):
    CASES += [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names) if k not in nullable]
    CASES += [("%s B = 0" % fn, lambda c=call: c(B=0), SHAPE), ("%s B < 0" % fn, lambda c=call: c(B=-2), SHAPE),
              ("%s K = 0" % fn, lambda c=call: c(Kd=0), SHAPE), ("%s K < 0" % fn, lambda c=call: c(Kd=-8), SHAPE),
              ("%s Cout = 0" % fn, lambda c=call: c(Cout=0), SHAPE), ("%s Cout = 5" % fn, lambda c=call: c(Cout=5), SHAPE),
              ("%s Cout < 0" % fn, lambda c=call: c(Cout=-1), SHAPE)]
CASES += [("logits_head_fwd K %% 4 = %d" % (k % 4), lambda k=k: head_fwd(Kd=k), SHAPE) for k in (9, 10, 11)]
CASES += [("logits_head_fwd misaligned x", lambda: head_fwd(off_at=0), SHAPE), ("logits_head_fwd misaligned w", lambda: head_fwd(off_at=1), SHAPE),
          ("logits_head_bwd B K = 2^31", lambda: head_bwd(B=1 << 16, Kd=1 << 15), SHAPE),
          ("logits_head_bwd dx, dw and db NULL: returns 0", lambda: L().mogan_logits_head_bwd(PTR, PTR, PTR, PTR, NULL, NULL, NULL, 2, 8, 1, 0, NULL), 0)]
for fn, names in ELEM_NAMES.items():
    CASES += [("%s NULL %s" % (fn, w), lambda fn=fn, k=k: elem(fn, null_at=k), SHAPE) for k, w in enumerate(names)]
    CASES += [("%s n = 0" % fn, lambda fn=fn: elem(fn, n=0), SHAPE), ("%s n < 0" % fn, lambda fn=fn: elem(fn, n=-16), SHAPE)]
B_, Bc_, C_, S_, T_, _ = K.WORDS_LDS_EDGE
for fn, call, names, nullable in (("words_fwd", words_fwd, ("ctx", "words", "cap_lens", "sim", "a1", "a2", "wc", "wt"), {7}),
                                  ("words_bwd", words_bwd, ("ctx", "words", "cap_lens", "a1", "a2", "wc", "dsim", "dwc", "dscore_t"), set())):
    CASES += [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names) if k not in nullable]
    for dim in ("B", "Bc", "C", "S", "T"):
        CASES += [("%s %s = 0" % (fn, dim), lambda c=call, d=dim: c(**{d: 0}), SHAPE),
                  ("%s %s < 0" % (fn, dim), lambda c=call, d=dim: c(**{d: -3}), SHAPE)]
    CASES += [("%s T > 32" % fn, lambda c=call: c(T=33), SHAPE), ("%s B > 65535" % fn, lambda c=call: c(B=65536), SHAPE),
              # one channel past the LDS limit: (C T + T (S + 1) + 1088) * 4 bytes with C = 189, S = 289, T = 32 is 65664
              ("%s one channel past the LDS limit" % fn, lambda c=call: c(B=B_, Bc=Bc_, C=C_ + 1, S=S_, T=T_), SHAPE)]
CASES += [("words_bwd S = 641", lambda: words_bwd(S=641), SHAPE)]
for fn, call, names, nullable in (("ce_fwd", ce_fwd, ("sim", "labels", "mask", "prow", "pcol", "nll", "out2"), {2}),
                                  ("ce_bwd", ce_bwd, ("prow", "pcol", "labels", "g0", "g1", "dsim"), {3, 4})):
    CASES += [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names) if k not in nullable]
    CASES += [("%s R = Q = 0" % fn, lambda c=call: c(R=0, Q=0), SHAPE), ("%s R = Q < 0" % fn, lambda c=call: c(R=-5, Q=-5), SHAPE),
              ("%s R < Q" % fn, lambda c=call: c(R=4, Q=5), SHAPE), ("%s R > Q" % fn, lambda c=call: c(R=5, Q=4), SHAPE),
              ("%s Q = 0" % fn, lambda c=call: c(Q=0), SHAPE)]
for fn, call, names in (("sent_fwd", sent_fwd, ("cnn", "rnn", "sim")), ("sent_bwd", sent_bwd, ("cnn", "rnn", "dsim", "dcnn"))):
    CASES += [("%s NULL %s" % (fn, w), lambda c=call, k=k: c(null_at=k), SHAPE) for k, w in enumerate(names)]
    for dim in ("B", "Bc", "C"):
        CASES += [("%s %s = 0" % (fn, dim), lambda c=call, d=dim: c(**{d: 0}), SHAPE),
                  ("%s %s < 0" % (fn, dim), lambda c=call, d=dim: c(**{d: -3}), SHAPE)]
CASES += [("sent_bwd Bc > 8192 (LDS)", lambda: sent_bwd(Bc=8193), SHAPE)]
for fn, names in (("sum", ("in", "weights", "out")), ("scale", ("out", "weights", "g"))):
    CASES += [("scalar_%s n = 0" % fn, lambda fn=fn: scalar(fn, n=0), SHAPE), ("scalar_%s n = 9" % fn, lambda fn=fn: scalar(fn, n=9), SHAPE),
              ("scalar_%s n < 0" % fn, lambda fn=fn: scalar(fn, n=-1), SHAPE),
              ("scalar_%s NULL entry 0" % fn, lambda fn=fn: scalar(fn, null_entry=0), SHAPE),
              ("scalar_%s NULL entry n - 1" % fn, lambda fn=fn: scalar(fn, n=8, null_entry=7), SHAPE)]
    CASES += [("scalar_%s NULL %s" % (fn, w), lambda fn=fn, k=k: scalar(fn, null_arg=k), SHAPE) for k, w in enumerate(names)]
ADAM_PTRS = ("p", "g", "m", "v", "ema")
CASES += [("adam_step NULL %s" % w, lambda k=k: adam(null_at=k), SHAPE) for k, w in enumerate(ADAM_PTRS) if w != "ema"]
CASES += [("adam_step misaligned %s" % w, lambda k=k: adam(off_at=k), SHAPE) for k, w in enumerate(ADAM_PTRS)]
CASES += [("adam_step n = 0", lambda: adam(n=0), SHAPE), ("adam_step n < 0", lambda: adam(n=-4), SHAPE),
          ("adam_step n = 0 with a device counter", lambda: adam(n=0, dev_state=PTR), SHAPE),
          ("adam_step step = 0", lambda: adam(step=0), SHAPE), ("adam_step step < 0", lambda: adam(step=-1), SHAPE)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_the_lds_rows_sit_on_both_sides_of_the_limit():
    assert K.words_lds_bytes(C_, S_, T_) == 64 * 1024 and K.words_lds_bytes(C_ + 1, S_, T_) == 64 * 1024 + 4 * T_
    # by the figure the header had before (896 floats of scratch) 194 channels would still fit: the code never took them
    assert (194 * T_ + T_ * (S_ + 1) + 896) * 4 <= 64 * 1024 < K.words_lds_bytes(194, S_, T_)


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_loss_entry_point_rejects_before_any_launch(call, expected):
    assert call() == expected
