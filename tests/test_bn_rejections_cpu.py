"""The shape and workspace rejections of the batch-norm / affine / activation / bias entry points of libmogan_hip.so
(csrc/mogan_norm.hip, csrc/mogan_elem.hip), as tests/test_conv_rejections_cpu.py does for the convolutions: every case is
answered by the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies that are never dereferenced.
-1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS."""
import ctypes

import pytest

import bn_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, WS = -1, -3
BIG = 1 << 30                       # "enough workspace" for a call that must be refused for another reason

ONE = (4, 8, 64)                    # one launch
TWO = (17, 6, 256)                  # two launches
THREE = (20, 4, 225)                # three launches
BN1D = (16, 24, 1)


def L():
    return lib.load()


def need(B, C, HW):
    return int(L().mogan_bn_ws_bytes(B, C, HW))


def stats(B, C, HW, ws=PTR, n=BIG):
    return L().mogan_bn_stats(PTR, B, C, HW, 1e-5, 0.1, PTR, PTR, PTR, PTR, ws, n, NULL)


def fwd(B, C, HW, act):
    return L().mogan_bn_act_fwd(PTR, PTR, PTR, PTR, PTR, NULL, PTR, B, C, HW, act, 0.2, NULL)


def fused(B, C, HW, act, ws=PTR, n=BIG):
    return L().mogan_bn_act_fwd_fused(PTR, PTR, PTR, NULL, PTR, PTR, PTR, PTR, PTR, B, C, HW, act, 0.2, 1e-5, 0.1, ws, n, NULL)


def bwd(B, C, HW, act, ws=PTR, n=BIG):
    return L().mogan_bn_act_bwd(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, B, C, HW, act, 0.2, 0, ws, n, NULL)


def gfwd(G, B, C, HW, act):
    return L().mogan_bn_act_grouped_fwd(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, G, B, C, HW, act, 0.2, 1e-5, 0.1, NULL)


def gbwd(G, B, C, HW, act):
    return L().mogan_bn_act_grouped_bwd(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, G, B, C, HW, act, 0.2, 0, NULL)


def running(mean=PTR, invstd=PTR, C=8, n=64):
    return L().mogan_bn_running_update(mean, invstd, PTR, PTR, C, n, 1e-5, 0.1, NULL)


def affine_fwd(B, C, HW, act):
    return L().mogan_affine_act_fwd(PTR, PTR, PTR, PTR, B, C, HW, act, 0.2, NULL)


def affine_bwd(B, C, HW, act):
    return L().mogan_affine_act_bwd(PTR, PTR, PTR, PTR, PTR, B, C, HW, act, 0.2, NULL)


def relu_out(B, C, HW):
    return L().mogan_affine_relu_bwd_out(PTR, PTR, PTR, PTR, B, C, HW, NULL)


def act_fwd(B, C, HW, act):
    return L().mogan_act_fwd(PTR, PTR, B, C, HW, act, 0.2, NULL)


def act_bwd(B, C, HW, act):
    return L().mogan_act_bwd(PTR, PTR, PTR, B, C, HW, act, 0.2, NULL)


BAD_DIMS = [(0, 8, 64), (-1, 8, 64), (4, 0, 64), (4, -2, 64), (4, 8, 0), (4, 8, -5)]
BAD_ACTS = [-1, K.TANH, K.SIGMOID, 6, 99]          # no BatchNorm / affine kernel has them
CASES = []
for d in BAD_DIMS:
    CASES += [
        ("bn_ws_bytes %s is 0" % (d,), lambda d=d: need(*d), 0),
        ("bn_stats %s" % (d,), lambda d=d: stats(*d), SHAPE),
        ("bn_act_fwd %s" % (d,), lambda d=d: fwd(*d, K.RELU), SHAPE),
        ("bn_act_fwd_fused %s" % (d,), lambda d=d: fused(*d, K.RELU), SHAPE),
        ("bn_act_bwd %s" % (d,), lambda d=d: bwd(*d, K.RELU), SHAPE),
        ("bn_act_grouped_fwd %s" % (d,), lambda d=d: gfwd(2, *d, K.RELU), SHAPE),
        ("bn_act_grouped_bwd %s" % (d,), lambda d=d: gbwd(2, *d, K.RELU), SHAPE),
        ("affine_act_fwd %s" % (d,), lambda d=d: affine_fwd(*d, K.RELU), SHAPE),
        ("affine_act_bwd %s" % (d,), lambda d=d: affine_bwd(*d, K.RELU), SHAPE),
        ("affine_relu_bwd_out %s" % (d,), lambda d=d: relu_out(*d), SHAPE),
        ("act_fwd %s" % (d,), lambda d=d: act_fwd(*d, K.RELU), SHAPE),
        ("act_bwd %s" % (d,), lambda d=d: act_bwd(*d, K.RELU), SHAPE),
        ("bias_add %s" % (d,), lambda d=d: L().mogan_bias_add(PTR, PTR, *d, NULL), SHAPE),
        ("bias_grad %s" % (d,), lambda d=d: L().mogan_bias_grad(PTR, PTR, *d, 0, NULL), SHAPE),
    ]
# GLU halves the channels: odd C, on every path of every entry that takes an activation
for name, (B, C, HW) in (("one", ONE), ("two", TWO), ("three", THREE), ("1d", BN1D)):
    odd = (B, C | 1, HW)
    CASES += [
        ("bn_act_fwd GLU odd C, %s" % name, lambda o=odd: fwd(*o, K.GLU), SHAPE),
        ("bn_act_fwd_fused GLU odd C, %s" % name, lambda o=odd: fused(*o, K.GLU), SHAPE),
        ("bn_act_bwd GLU odd C, %s" % name, lambda o=odd: bwd(*o, K.GLU), SHAPE),
    ]
    for a in BAD_ACTS:
        CASES += [
            ("bn_act_fwd act %d, %s" % (a, name), lambda a=a, s=(B, C, HW): fwd(*s, a), SHAPE),
            # with a workspace that would do: the code is refused before the statistics are launched
            ("bn_act_fwd_fused act %d, %s" % (a, name), lambda a=a, s=(B, C, HW): fused(*s, a), SHAPE),
            ("bn_act_bwd act %d, %s" % (a, name), lambda a=a, s=(B, C, HW): bwd(*s, a), SHAPE),
        ]
CASES += [
    ("bn_act_grouped_fwd GLU odd C", lambda: gfwd(2, 4, 7, 16, K.GLU), SHAPE),
    ("bn_act_grouped_bwd GLU odd C", lambda: gbwd(2, 4, 7, 16, K.GLU), SHAPE),
    ("act_fwd GLU odd C", lambda: act_fwd(3, 7, 35, K.GLU), SHAPE),
    ("act_bwd GLU odd C", lambda: act_bwd(3, 7, 35, K.GLU), SHAPE),
    ("act_fwd act NONE", lambda: act_fwd(3, 8, 35, K.NONE), SHAPE),
    ("act_fwd act 6", lambda: act_fwd(3, 8, 35, 6), SHAPE),
    ("act_bwd act -1", lambda: act_bwd(3, 8, 35, -1), SHAPE),
    ("affine_act_fwd GLU", lambda: affine_fwd(3, 6, 35, K.GLU), SHAPE),
    ("affine_act_bwd GLU", lambda: affine_bwd(3, 6, 35, K.GLU), SHAPE),
    ("affine_act_fwd act TANH", lambda: affine_fwd(3, 6, 35, K.TANH), SHAPE),
    ("affine_act_bwd act 99", lambda: affine_bwd(3, 6, 35, 99), SHAPE),
    ("affine_act_fwd more channels than a grid extent", lambda: affine_fwd(2, 70000, 9, K.RELU), SHAPE),
    ("bn_act_grouped_fwd act 7", lambda: gfwd(2, 4, 8, 16, 7), SHAPE),
    ("bn_act_grouped_bwd act -1", lambda: gbwd(2, 4, 8, 16, -1), SHAPE),
    ("bn_running_update NULL mean", lambda: running(mean=NULL), SHAPE),
    ("bn_running_update NULL invstd", lambda: running(invstd=NULL), SHAPE),
    ("bn_running_update n = 0", lambda: running(n=0), SHAPE),
    ("bn_running_update n < 0", lambda: running(n=-3), SHAPE),
    ("bn_running_update C = 0", lambda: running(C=0), SHAPE),
    # more output channels than the apply grid's (image, channel) extent holds for one image, beyond the one-launch size:
    # refused before the statistics / partial sums are launched
    ("bn_act_fwd_fused Cy > 65535, two launches", lambda: fused(80, 70000, 64, K.RELU), SHAPE),
    ("bn_act_fwd_fused Cy > 65535, three launches", lambda: fused(2, 70000, 9, K.RELU), SHAPE),
    ("bn_act_bwd Cy > 65535, two launches", lambda: bwd(80, 70000, 64, K.RELU), SHAPE),
    ("bn_act_bwd Cy > 65535, three launches", lambda: bwd(2, 70000, 9, K.NONE), SHAPE),
    ("bn_act_fwd Cy > 65535", lambda: fwd(2, 70000, 9, K.LRELU), SHAPE),
]
G_, B_, C_ = K.GROUPED_INELIGIBLE[:3]
HW_ = K.GROUPED_INELIGIBLE[3] * K.GROUPED_INELIGIBLE[4]
CASES += [
    ("grouped_eligible %s" % (K.GROUPED_INELIGIBLE,), lambda: L().mogan_bn_act_grouped_eligible(G_, B_, C_, HW_), 0),
    ("grouped_eligible G = 0", lambda: L().mogan_bn_act_grouped_eligible(0, 2, 4, 16), 0),
    ("grouped_eligible 2^31 elements", lambda: L().mogan_bn_act_grouped_eligible(1 << 10, 16, 1 << 9, 256), 0),
    ("bn_act_grouped_fwd ineligible", lambda: gfwd(G_, B_, C_, HW_, K.RELU), SHAPE),
    ("bn_act_grouped_bwd ineligible", lambda: gbwd(G_, B_, C_, HW_, K.RELU), SHAPE),
    ("bn_act_grouped_fwd G = 0", lambda: gfwd(0, 2, 4, 16, K.RELU), SHAPE),
    ("bn_act_grouped_bwd G = -1", lambda: gbwd(-1, 2, 4, 16, K.RELU), SHAPE),
]
for g in K.GROUPED:
    CASES.append(("grouped_eligible %s" % (g,), lambda g=g: L().mogan_bn_act_grouped_eligible(g[0], *K.dims(g[1:])), 1))
# the workspace: NULL, or one byte short, wherever the path needs it (the one-launch forward does not: GPU module)
for name, s in (("two", TWO), ("three", THREE), ("1d", BN1D), ("one", ONE)):
    CASES += [
        ("bn_stats NULL ws, %s" % name, lambda s=s: stats(*s, ws=NULL, n=BIG), WS),
        ("bn_stats ws one byte short, %s" % name, lambda s=s: stats(*s, n=need(*s) - 1), WS),
        ("bn_act_bwd NULL ws, %s" % name, lambda s=s: bwd(*s, K.LRELU, ws=NULL, n=BIG), WS),
        ("bn_act_bwd ws one byte short, %s" % name, lambda s=s: bwd(*s, K.GLU, n=need(*s) - 1), WS),
    ]
    if name != "one":
        CASES += [
            ("bn_act_fwd_fused NULL ws, %s" % name, lambda s=s: fused(*s, K.RELU, ws=NULL, n=BIG), WS),
            ("bn_act_fwd_fused ws one byte short, %s" % name, lambda s=s: fused(*s, K.GLU, n=need(*s) - 1), WS),
            ("bn_act_fwd_fused no ws at all, %s" % name, lambda s=s: fused(*s, K.NONE, ws=NULL, n=0), WS),
        ]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_the_shapes_are_on_the_paths_their_names_say():
    for name, (B, C, HW) in (("one", ONE), ("two", TWO), ("three", THREE), ("three", BN1D)):
        assert K.path_of((B, C, HW)) == name
    assert all(need(*s) > 0 for s in (ONE, TWO, THREE, BN1D))


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bn_entry_point_rejects_before_any_launch(call, expected):
    assert call() == expected


def test_ws_bytes_pins_the_statistics_split_of_the_ragged_row():
    """(2, 4, 41, 100): HW = 4100 over three slabs of hper = 1368 (the last holds 1364) for each of the 2 images, so 6 partial
    entries of 4 doubles per channel, then mean / invstd (2 floats per channel) and 64 bytes: the size is the split"""
    B, C, HW = K.dims(K.TWO_LAUNCH[1])
    slabs, hper = B * 3, 1368
    assert 2 * hper < HW < 3 * hper and hper % 4 == 0
    assert need(B, C, HW) == C * slabs * 4 * 8 + C * 2 * 4 + 64
