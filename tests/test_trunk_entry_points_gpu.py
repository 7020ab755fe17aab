"""-m gpu: the channel-slice entry points of the frozen Inception trunk (include/mogan_hip.h; called by attngan/inception.py
only) through ctypes, against fp64 references, under the memory contract of tests/memguard.py: every output slice sits in a
sentinel-filled parent inside guard bands; in write mode it starts as NaN poison, in accumulate mode as a finite base; after
the call every slice element is written and right, nothing outside the slice changed, the inputs are bitwise unchanged.  The
workspace is NaN-poisoned before every call, and every convolution also runs with ws = NULL, ws_bytes = 0 (no split-K).

Tolerances: convolutions (products on the bf16 pipe from the exact three-piece split, fp32 accumulation) elementwise
|got - fp64| <= CONV_TOL * (the same sum over |terms|) + EPS32 * |base|; pooling gradients EPS32 * 4 * (sum over |terms| +
|base|); max-pool forward, its indices, ReLU backward and copies exactly.  Slice offsets are those of the trunk's kind
(whole channels, 16-byte aligned)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import memguard as mg
from helpers import load_pkg

load_pkg()
from oracle import inception_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu

CONV_TOL = 1e-5
EPS32 = 2.0 ** -24
DEV = "cuda"


def _lib():
    from mogan_amd.hip import lib
    return lib


class _WS:
    """the workspace: NaN-poisoned before every call; `null` = (NULL, 0)"""

    def __init__(self):
        self.buf = torch.empty(_lib().WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)

    def args(self, null):
        if null:
            return None, 0
        mg.poison_(self.buf.view(torch.float32))
        return self.buf.data_ptr(), self.buf.numel()


@pytest.fixture(scope="module")
def ws():
    return _WS()


def _slice(shape, c0, C):
    return (slice(None), slice(c0, c0 + C))


def _inp(shape, c0, C, relu=False, seed=0):
    """an input slice of a larger tensor (the rest random too): (parent, slice view)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    if relu:
        t = torch.relu(t)
    t = t.to(DEV)
    return t, t[:, c0:c0 + C]


def _stream():
    return _lib().stream_ptr()


# ---------------------------------------------------------------------------------------------------------------- forward
# (B, Cin, H, W, Cout, KH, KW, stride, ph, pw): the trunk's geometries and ragged ones
FWD_GEOMS = [
    (2, 192, 35, 35, 176, 1, 1, 1, 0, 0),      # Mixed_5b grouped 1x1
    (2, 48, 35, 35, 64, 5, 5, 1, 2, 2),        # branch5x5_2
    (2, 64, 35, 35, 96, 3, 3, 1, 1, 1),        # branch3x3dbl_2
    (2, 288, 35, 35, 384, 3, 3, 2, 0, 0),      # Mixed_6a branch3x3
    (2, 128, 17, 17, 128, 1, 7, 1, 0, 3),      # branch7x7_2
    (2, 160, 17, 17, 192, 7, 1, 1, 3, 0),      # branch7x7_3
    (2, 192, 17, 17, 320, 3, 3, 2, 0, 0),      # Mixed_7a branch3x3_2
    (2, 384, 8, 8, 384, 1, 3, 1, 0, 1),        # branch3x3_2a
    (2, 448, 8, 8, 384, 3, 3, 1, 1, 1),        # branch3x3dbl_2
    (3, 20, 13, 9, 37, 3, 3, 2, 1, 0),         # ragged, asymmetric pad
    (1, 7, 11, 6, 5, 3, 2, 1, 2, 1),           # ragged, pad wider than half the kernel
]


def _fwd_case(i, g, relu, two):
    B, Cin, H, W, Cout, KH, KW, s, ph, pw = g
    OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    cx0 = 16 * (i % 3)
    X, x = _inp((B, cx0 + Cin + 16, H, W), cx0, Cin, relu=True, seed=i)
    gen = torch.Generator().manual_seed(100 + i)
    w = (torch.randn((Cout, Cin, KH, KW), generator=gen) * (2.0 / (Cin * KH * KW)) ** 0.5).to(DEV)
    scale = (torch.rand(Cout, generator=gen) * 0.4 + 0.8).to(DEV)
    shift = (torch.randn(Cout, generator=gen) * 0.05).to(DEV)
    msplit = (Cout // 2 + 3) // 4 * 4 if two else Cout
    cy0 = 16 * ((i + 1) % 3)
    y = mg.Guarded((B, cy0 + msplit + 32, OH, OW), _slice(None, cy0, msplit), DEV)
    y2 = mg.Guarded((B, Cout - msplit + 48, OH, OW), _slice(None, 16, Cout - msplit), DEV) if two else None
    x64, w64 = x.cpu().double(), w.cpu().double()
    z = F.conv2d(x64, w64, None, s, (ph, pw))
    za = F.conv2d(x64.abs(), w64.abs(), None, s, (ph, pw))
    sc, sh = scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)
    ref = z * sc + sh
    if relu:
        ref = ref.clamp_min(0)
    tol = CONV_TOL * za * sc.abs() + 4 * EPS32 * sh.abs()
    return dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, KH=KH, KW=KW, s=s, ph=ph, pw=pw, X=X, x=x, w=w, scale=scale, shift=shift,
                msplit=msplit, y=y, y2=y2, ref=ref, tol=tol, relu=relu, frozen=[mg.Frozen(t) for t in (X, w, scale, shift)])


def _fwd_args(c):
    from mogan_amd.hip.lib import ConvFwdArgs
    y2 = c["y2"]
    return ConvFwdArgs(c["x"].data_ptr(), c["X"].stride(0), c["w"].data_ptr(), c["scale"].data_ptr(), c["shift"].data_ptr(),
                       c["y"].ptr, c["y"].bstride, y2.ptr if y2 else None, y2.bstride if y2 else 0,
                       c["msplit"] if y2 else c["Cout"], c["B"], c["Cin"], c["H"], c["W"], c["Cout"], c["KH"], c["KW"], c["s"],
                       c["ph"], c["pw"], c["relu"])


def _fwd_check(c, what):
    torch.cuda.synchronize()
    m = c["msplit"]
    c["y"].check(c["ref"][:, :m], c["tol"][:, :m], what=what + " y")
    if c["y2"] is not None:
        c["y2"].check(c["ref"][:, m:], c["tol"][:, m:], what=what + " y2")
    for f in c["frozen"]:
        f.check(what)


@pytest.mark.parametrize("null_ws", [False, True])
def test_conv2d_affine_fwd_ex_slices(null_ws, ws):
    call = _lib().call
    for i, g in enumerate(FWD_GEOMS):
        for relu, two in ((1, i % 2 == 0), (0, i % 2 == 1)):
            c = _fwd_case(i, g, relu, two)
            a = _fwd_args(c)
            wsp, wsn = ws.args(null_ws)
            call("mogan_conv2d_affine_fwd_ex", a.x, a.x_bstride, a.w, a.scale, a.shift, a.y, a.y_bstride, a.y2, a.y2_bstride,
                 a.msplit, a.B, a.Cin, a.Hs, a.Ws, a.Cout, a.KH, a.KW, a.stride, a.ph, a.pw, a.relu, wsp, wsn, _stream())
            _fwd_check(c, "affine_fwd_ex %s relu=%d y2=%d ws=%s" % (g, relu, two, not null_ws))


# groups as the Mixed blocks issue them: members write adjacent slices of ONE output tensor (or of two)
FWD_GROUPS = [[0, 5], [1, 2, 8], [4, 5, 6, 3], [9], [7, 8, 10]]


@pytest.mark.parametrize("grouped", [True, False])
def test_conv2d_affine_fwd_group_adjacent_slices(grouped, ws):
    """grouped: the group kernel itself (mogan_gemm_group_min_tiles(0)); else the default rule (small groups run member by
    member, with split-K)"""
    lib = _lib()
    L = lib.load()
    if grouped:
        L.mogan_gemm_group_min_tiles(0)
    try:
        for gi, members in enumerate(FWD_GROUPS):
            for null_ws in (False, True):
                cases = [_fwd_case(i, FWD_GEOMS[i], (i + gi) % 2, (i + gi) % 3 == 0) for i in members]
                # one shared output tensor per distinct output map: adjacent channel slices, written by the group
                _share_outputs(cases)
                arr = (lib.ConvFwdArgs * len(cases))(*[_fwd_args(c) for c in cases])
                wsp, wsn = ws.args(null_ws)
                lib.call("mogan_conv2d_affine_fwd_group", len(cases), ctypes.cast(arr, ctypes.c_void_p), wsp, wsn, _stream())
                for c in cases:
                    _fwd_check(c, "affine_fwd_group %s member %s ws=%s" % (members, (c["Cin"], c["Cout"]), not null_ws))
    finally:
        L.mogan_gemm_group_min_tiles(1600)


def _share_outputs(cases):
    """members with the same batch and output map write adjacent slices [c0, c0 + msplit) of one guarded parent"""
    by = {}
    for c in cases:
        OH = (c["H"] + 2 * c["ph"] - c["KH"]) // c["s"] + 1
        OW = (c["W"] + 2 * c["pw"] - c["KW"]) // c["s"] + 1
        by.setdefault((c["B"], OH, OW), []).append(c)
    for (B, OH, OW), cs in by.items():
        if len(cs) < 2:
            continue
        tot = sum(c["msplit"] for c in cs)
        parent = mg.Guarded((B, 16 + tot + 16, OH, OW), _slice(None, 16, tot), DEV)
        c0 = 16
        for c in cs:
            c["y"] = _SubSlice(parent, c0, c["msplit"])
            c0 += c["msplit"]


class _SubSlice:
    """channels [c0, c0 + n) of a Guarded parent (its check covers the whole guarded tensor: a neighbour's slice is written by
    its own member, so only bands, poison and this member's values are checked here)"""

    def __init__(self, g, c0, n):
        self.g, self.c0, self.n = g, c0, n
        self.view = g.parent[:, c0:c0 + n]

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def bstride(self):
        return self.g.bstride

    def check(self, expect, atol, what=""):
        p = [q for q in self.g.problems() if "expected" not in q]
        err = (self.view.cpu().double() - expect).abs()
        bad = ~(err <= atol)
        if bool(bad.any()):
            p.append("%d elements off (max err %.3e)" % (int(bad.sum()), float(err.max())))
        if bool(torch.isnan(self.view).any()):
            p.append("unwritten elements")
        assert not p, "%s: %s" % (what, "; ".join(p))


# ------------------------------------------------------------------------------------ data gradients (dgrad_ex, fwd_ex)
# (B, Cin, H, W, Cout, KH, KW, stride, ph, pw) of the forward convolution whose data gradient is taken
DGRAD_GEOMS = [
    (2, 192, 35, 35, 176, 1, 1, 1, 0, 0),      # Mixed_5b grouped 1x1 (K = concatenated output channels)
    (2, 288, 35, 35, 384, 3, 3, 2, 0, 0),      # Mixed_6a branch3x3
    (2, 96, 35, 35, 96, 3, 3, 2, 0, 0),        # Mixed_6a branch3x3dbl_3
    (2, 192, 17, 17, 320, 3, 3, 2, 0, 0),      # Mixed_7a branch3x3_2
    (2, 768, 17, 17, 192, 1, 1, 1, 0, 0),      # Mixed_6b 1x1
    (2, 160, 17, 17, 160, 1, 7, 1, 0, 3),      # 1x7 (dgrad_ex on a stride-1 geometry)
    (3, 20, 14, 11, 24, 3, 3, 2, 0, 0),        # ragged: the last row / column is in no window
    (2, 12, 9, 13, 8, 5, 5, 1, 2, 2),          # 5x5 p2, ragged map
]


def _dgrad_case(i, g, acc, mask):
    B, Cin, H, W, Cout, KH, KW, s, ph, pw = g
    OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    cy0 = 16 * (i % 2)
    DY, dy = _inp((B, cy0 + Cout + 16, OH, OW), cy0, Cout, seed=200 + i)
    gen = torch.Generator().manual_seed(300 + i)
    w = (torch.randn((Cout, Cin, KH, KW), generator=gen) * (1.0 / (Cin * KH * KW)) ** 0.5).to(DEV)
    cr0 = 16 * ((i + 1) % 3)
    R, r = _inp((B, cr0 + Cin + 32, H, W), cr0, Cin, relu=True, seed=400 + i)      # ReLU output: exact zeros
    r[:, :, 0, 0] = -1.0                                                             # and a negative value
    cx0 = 16 * (i % 3)
    base = torch.randn((B, Cin, H, W), generator=gen) if acc else None
    dx = mg.Guarded((B, cx0 + Cin + 16, H, W), _slice(None, cx0, Cin), DEV, base=None if base is None else base.to(DEV))
    dy64, w64 = dy.cpu().double(), w.cpu().double()
    ref = torch.nn.grad.conv2d_input((B, Cin, H, W), w64, dy64, s, (ph, pw))
    refa = torch.nn.grad.conv2d_input((B, Cin, H, W), w64.abs(), dy64.abs(), s, (ph, pw))
    if mask:
        ref = torch.where(r.cpu() > 0, ref, torch.zeros((), dtype=ref.dtype))
    tol = CONV_TOL * refa
    if acc:
        ref = ref + base.double()
        tol = tol + 2 * EPS32 * (base.double().abs() + refa)
    return dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, KH=KH, KW=KW, s=s, ph=ph, pw=pw, DY=DY, dy=dy, w=w, R=R, r=r if mask else None,
                acc=acc, dx=dx, ref=ref, tol=tol, frozen=[mg.Frozen(t) for t in (DY, w, R)])


def _dgrad_args(c):
    from mogan_amd.hip.lib import ConvDgradArgs
    r = c["r"]
    return ConvDgradArgs(c["dy"].data_ptr(), c["DY"].stride(0), c["w"].data_ptr(), c["dx"].ptr, c["dx"].bstride,
                         r.data_ptr() if r is not None else None, c["R"].stride(0) if r is not None else 0, c["acc"], c["B"],
                         c["Cin"], c["H"], c["W"], c["Cout"], c["KH"], c["KW"], c["s"], c["ph"], c["pw"])


def _dgrad_check(c, what):
    torch.cuda.synchronize()
    c["dx"].check(c["ref"], c["tol"], what=what)
    for f in c["frozen"]:
        f.check(what)


@pytest.mark.parametrize("null_ws", [False, True])
def test_conv2d_dgrad_ex_slices(null_ws, ws):
    call = _lib().call
    for i, g in enumerate(DGRAD_GEOMS):
        for acc, mask in ((0, 1), (1, 1), (1, 0), (0, 0)):
            c = _dgrad_case(i, g, acc, mask)
            a = _dgrad_args(c)
            wsp, wsn = ws.args(null_ws)
            call("mogan_conv2d_dgrad_ex", a.dy, a.dy_bstride, a.w, a.dx, a.dx_bstride, a.relu_of, a.relu_bstride, a.accumulate,
                 a.B, a.Cin, a.Hs, a.Ws, a.Cout, a.KH, a.KW, a.stride, a.ph, a.pw, wsp, wsn, _stream())
            _dgrad_check(c, "dgrad_ex %s acc=%d mask=%d ws=%s" % (g, acc, mask, not null_ws))


DGRAD_GROUPS = [[1, 2], [0, 6], [3, 4, 5, 7], [6]]


@pytest.mark.parametrize("grouped", [True, False])
def test_conv2d_dgrad_group(grouped, ws):
    lib = _lib()
    L = lib.load()
    if grouped:
        L.mogan_gemm_group_min_tiles(0)
    try:
        for gi, members in enumerate(DGRAD_GROUPS):
            for null_ws in (False, True):
                cases = [_dgrad_case(i, DGRAD_GEOMS[i], (i + gi) % 2, 1) for i in members]
                arr = (lib.ConvDgradArgs * len(cases))(*[_dgrad_args(c) for c in cases])
                wsp, wsn = ws.args(null_ws)
                lib.call("mogan_conv2d_dgrad_group", len(cases), ctypes.cast(arr, ctypes.c_void_p), wsp, wsn, _stream())
                for c in cases:
                    _dgrad_check(c, "dgrad_group %s member %s ws=%s" % (members, (c["Cin"], c["Cout"]), not null_ws))
    finally:
        L.mogan_gemm_group_min_tiles(1600)


# stride-1 data gradients as the trunk runs them: a forward convolution of dY with the flipped, (ci, co)-transposed filters
FLIP_GEOMS = [
    (2, 48, 35, 35, 64, 5, 5, 1, 2, 2),
    (2, 64, 35, 35, 96, 3, 3, 1, 1, 1),
    (2, 128, 17, 17, 128, 1, 7, 1, 0, 3),
    (2, 160, 17, 17, 192, 7, 1, 1, 3, 0),
    (2, 384, 8, 8, 384, 3, 1, 1, 1, 0),
    (3, 12, 13, 9, 20, 3, 3, 1, 1, 1),
]


@pytest.mark.parametrize("null_ws", [False, True])
def test_conv2d_fwd_ex_flipped_data_gradient(null_ws, ws):
    call = _lib().call
    for i, g in enumerate(FLIP_GEOMS):
        for acc, mask in ((0, 1), (1, 1), (1, 0)):
            c = _dgrad_case(50 + i, g, acc, mask)
            B, Cin, H, W, Cout, KH, KW, s, ph, pw = g
            wflip = c["w"].flip(2, 3).transpose(0, 1).contiguous()          # (Cin, Cout, KH, KW): the forward filters of dX
            c["frozen"].append(mg.Frozen(wflip))
            r = c["r"]
            wsp, wsn = ws.args(null_ws)
            call("mogan_conv2d_fwd_ex", c["dy"].data_ptr(), c["DY"].stride(0), wflip.data_ptr(), c["dx"].ptr, c["dx"].bstride,
                 r.data_ptr() if r is not None else None, c["R"].stride(0) if r is not None else 0, acc, B, Cout, H, W, Cin,
                 KH, KW, 1, KH - 1 - ph, KW - 1 - pw, wsp, wsn, _stream())
            _dgrad_check(c, "fwd_ex (flipped) %s acc=%d mask=%d ws=%s" % (g, acc, mask, not null_ws))


# ------------------------------------------------------------------------------------------------------------- pooling
POOL_GEOMS = [(2, 64, 147, 147), (2, 192, 71, 71), (2, 288, 35, 35), (2, 768, 17, 17), (3, 5, 10, 9)]


def test_maxpool_fwd_ex_into_a_slice_ties_first():
    call = _lib().call
    for i, (B, C, H, W) in enumerate(POOL_GEOMS):
        OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        gen = torch.Generator().manual_seed(500 + i)
        x = torch.relu(torch.randn((B, C, H, W), generator=gen))                  # post-ReLU: ties among zeros
        x[:, :, 0:3, 0:3] = 0.25                                                     # and a window of equal positive values
        x = x.to(DEV)
        fx = mg.Frozen(x)
        c0 = 16 * (1 + i % 2)
        y = mg.Guarded((B, c0 + C + 16, OH, OW), _slice(None, c0, C), DEV)
        idx = mg.Guarded((B, C, OH, OW), (Ellipsis,), DEV, dtype=torch.uint8)
        call("mogan_maxpool_fwd_ex", x.data_ptr(), y.ptr, y.bstride, idx.ptr, B, C, H, W, 3, 2, _stream())
        torch.cuda.synchronize()
        x64 = x.cpu()
        y.check(F.max_pool2d(x64, 3, 2), exact=True, what="maxpool_fwd_ex %s" % ((B, C, H, W),))
        want = IO.pool_offsets(x64)
        idx.check(want, exact=True, what="maxpool_fwd_ex idx %s" % ((B, C, H, W),))
        assert int(want[:, :, 0, 0].max()) == 0                                      # (the tie window: the first element)
        fx.check("maxpool_fwd_ex")


def test_maxpool_bwd_ex():
    call = _lib().call
    for i, (B, C, H, W) in enumerate(POOL_GEOMS):
        OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        gen = torch.Generator().manual_seed(600 + i)
        x = torch.relu(torch.randn((B, C, H, W), generator=gen))
        idx = IO.pool_offsets(x)
        c0 = 16 * (i % 3)
        DY = torch.randn((B, c0 + C + 16, OH, OW), generator=gen)
        dy = DY[:, c0:c0 + C]
        for acc, mask in ((0, 1), (1, 1), (0, 0), (1, 0)):
            base = torch.randn((B, C, H, W), generator=gen) if acc else None
            dx = mg.Guarded((B, C, H, W), (Ellipsis,), DEV, base=None if base is None else base.to(DEV))
            xg, idg, DYg = x.to(DEV), idx.to(DEV), DY.to(DEV)
            fr = [mg.Frozen(t) for t in (xg, idg, DYg)]
            call("mogan_maxpool_bwd_ex", idg.data_ptr(), DYg[:, c0:c0 + C].data_ptr(), DYg.stride(0), dx.ptr,
                 xg.data_ptr() if mask else None, acc, B, C, H, W, 3, 2, _stream())
            torch.cuda.synchronize()
            ref, refa = _pool_scatter(x, idx, dy)
            if mask:
                ref = torch.where(x > 0, ref, torch.zeros((), dtype=ref.dtype))
            tol = 4 * EPS32 * refa
            if acc:
                ref = ref + base.double()
                tol = tol + 2 * EPS32 * (base.double().abs() + refa)
            what = "maxpool_bwd_ex %s acc=%d mask=%d" % ((B, C, H, W), acc, mask)
            dx.check(ref, tol, what=what)
            for f in fr:
                f.check(what)


def _pool_scatter(x, idx, dy):
    """fp64 max-pool gradient routed through the given window offsets: (sum of dy, sum of |dy|) per input element"""
    IO.POOL_ARGMAX = {"t": idx}
    try:
        out = []
        for d in (dy, dy.abs()):
            x64 = x.double().requires_grad_(True)
            g, = torch.autograd.grad(IO._maxpool("t", x64), x64, d.double())
            out.append(g)
    finally:
        IO.POOL_ARGMAX = None
    return out


def test_avgpool_bwd_ex():
    """the 3x3 / stride 1 / pad 1 average pool of the pool branches (count_include_pad) and a ragged strided one"""
    call = _lib().call
    for i, (P, H, W, k, s, pad) in enumerate([(2 * 192, 35, 35, 3, 1, 1), (2 * 768, 17, 17, 3, 1, 1), (2 * 1280, 8, 8, 3, 1, 1),
                                              (7, 11, 6, 3, 2, 1), (5, 9, 10, 2, 2, 0)]):
        OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        gen = torch.Generator().manual_seed(700 + i)
        dy = torch.randn((P, OH, OW), generator=gen)
        r = torch.relu(torch.randn((P, H, W), generator=gen))
        for acc, mask in ((0, 1), (1, 1), (0, 0), (1, 0)):
            base = torch.randn((P, H, W), generator=gen) if acc else None
            dx = mg.Guarded((P, H, W), (Ellipsis,), DEV, base=None if base is None else base.to(DEV))
            dyg, rg = dy.to(DEV), r.to(DEV)
            fr = [mg.Frozen(t) for t in (dyg, rg)]
            call("mogan_avgpool_bwd_ex", dyg.data_ptr(), dx.ptr, rg.data_ptr() if mask else None, acc, P, H, W, k, s, pad,
                 _stream())
            torch.cuda.synchronize()
            outs = []
            for d in (dy, dy.abs()):
                x64 = torch.zeros((1, P, H, W), dtype=torch.float64, requires_grad=True)
                g, = torch.autograd.grad(F.avg_pool2d(x64, k, s, pad, count_include_pad=True), x64, d.double()[None])
                outs.append(g[0])
            ref, refa = outs
            if mask:
                ref = torch.where(r > 0, ref, torch.zeros((), dtype=ref.dtype))
            tol = 4 * EPS32 * refa
            if acc:
                ref = ref + base.double()
                tol = tol + 2 * EPS32 * (base.double().abs() + refa)
            what = "avgpool_bwd_ex %s acc=%d mask=%d" % ((P, H, W, k, s, pad), acc, mask)
            dx.check(ref, tol, what=what)
            for f in fr:
                f.check(what)


def test_relu_bwd_written_added_and_in_place():
    call = _lib().call
    for n in (2 * 2048 * 64, 1000003, 5):
        gen = torch.Generator().manual_seed(n)
        z = torch.relu(torch.randn(n, generator=gen))
        z[:3] = torch.tensor([0.0, -0.0, 1e-30])[:min(3, n)]
        dz = torch.randn(n, generator=gen)
        zg, dzg = z.to(DEV), dz.to(DEV)
        fr = [mg.Frozen(zg), mg.Frozen(dzg)]
        want = torch.where(z > 0, dz, torch.zeros(()))
        dx = mg.Guarded((1, n), (Ellipsis,), DEV)
        call("mogan_relu_bwd", zg.data_ptr(), dzg.data_ptr(), dx.ptr, n, 0, _stream())
        torch.cuda.synchronize()
        dx.check(want[None], exact=True, what="relu_bwd write %d" % n)
        base = torch.randn(n, generator=gen)
        dx = mg.Guarded((1, n), (Ellipsis,), DEV, base=base.to(DEV)[None])
        call("mogan_relu_bwd", zg.data_ptr(), dzg.data_ptr(), dx.ptr, n, 1, _stream())
        torch.cuda.synchronize()
        dx.check((base + want)[None], exact=True, what="relu_bwd accumulate %d" % n)
        # in place, as the trunk's stem does after a plain data gradient (inception.py: dx.ptr as both dz and dx)
        dx = mg.Guarded((1, n), (Ellipsis,), DEV, base=dzg[None])
        call("mogan_relu_bwd", zg.data_ptr(), dx.ptr, dx.ptr, n, 0, _stream())
        torch.cuda.synchronize()
        dx.check(want[None], exact=True, what="relu_bwd in place %d" % n)
        for f in fr:
            f.check("relu_bwd")


def test_copy_strided_between_channel_slices():
    """the grouped 1x1 data gradient's gather: a slice of the block-output gradient into the room in front of the scratch
    gradient (inception._Tape.scratch_for_group)"""
    call = _lib().call
    for i, (B, C, H, W, cs0, Cs, cd0, Cd) in enumerate([(2, 64, 35, 35, 0, 256, 0, 176), (2, 192, 17, 17, 0, 768, 0, 512),
                                                        (2, 320, 8, 8, 0, 2048, 0, 1152), (3, 5, 7, 9, 12, 20, 4, 11)]):
        gen = torch.Generator().manual_seed(800 + i)
        SRC = torch.randn((B, Cs, H, W), generator=gen).to(DEV)
        fs = mg.Frozen(SRC)
        dst = mg.Guarded((B, Cd, H, W), _slice(None, cd0, C), DEV)
        call("mogan_copy_strided", SRC[:, cs0:cs0 + C].data_ptr(), SRC.stride(0), dst.ptr, dst.bstride, B, C * H * W, _stream())
        torch.cuda.synchronize()
        dst.check(SRC[:, cs0:cs0 + C], exact=True, what="copy_strided %d" % i)
        fs.check("copy_strided")
