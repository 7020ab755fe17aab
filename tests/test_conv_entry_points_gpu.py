"""-m gpu: the convolution entry points of the GAN path (include/mogan_hip.h: mogan_conv2d_fwd / _dgrad / _wgrad, their *_wp forms
with prepared filter images, mogan_upconv3x3_*, mogan_conv2d_lrelu_fwd, the packed-weight kernels) through ctypes, per element
against fp64 and under the memory contract of tests/memguard.py -- what tests/test_trunk_entry_points_gpu.py does for the frozen
trunk, on the kernels a train step spends its time in.  Geometries, forced dispatches and inputs are those of
tests/test_kernels_gpu.py (tests/conv_cases.py).

Memory, every call:
  * the output is the payload of a guard-banded buffer: NaN poison in write mode, a finite base in accumulate mode; afterwards every
    element is written and nothing outside changed;
  * every input lives in a guard-banded buffer too, whose bands hold a NaN (an out-of-range read that reaches a sum shows in the
    values), and is bitwise unchanged afterwards, bands included;
  * the workspace is the payload of a guard-banded byte buffer, filled with 0xFF (NaN as fp32 and as bf16) before every call and
    passed with exactly its size; afterwards its bands are intact.  Three sizes, see WS_SIZES;
  * MOGAN_ERR_WS is accepted from a reduced workspace only, and then nothing may have been written; any other code fails;
  * the same call a second time, after poisoning workspace and output again, gives the same bits (include/mogan_hip.h: fixed
    summation order per split; no floating-point atomics in the convolution sources).

Values, every output, two assertions that catch different faults:
  * rel-L2 <= 2e-6 over the tensor, the project's figure (a uniformly lower precision -- a dropped third bf16 piece -- shows here);
  * per element |got - fp64| <= TOL * S (+ 2 * 2^-24 * (|base| + S) when accumulating), S = the same sum over the absolute values
    of both operands (a few wrong elements -- a ragged last tile, a slab edge, a border tap -- show here).  TOL comes from
    conv_cases.TOL (4 x torch's own fp32 CPU error) or, where the launch record says a Winograd kernel ran, conv_cases.TOL_WINO
    (4 x a plain fp32 emulation of the algorithm); tests/test_conv_reference_cpu.py derives both.

Which kernel ran is read from the measurement hook (mogan_prof_enable / mogan_prof_collect, rows {mode, cfg, ...}: modes 4 / 5 / 6
= forward / data gradient / weight gradient off the implicit GEMM with cfg 1 = Winograd 8-wave, 3 = Winograd 16-wave, 0 = direct,
2 = dconv2; modes 0 / 1 / 2 = implicit GEMM by tile configuration; 7 / 8 / 9 = packed; no row = a small-channel kernel or the
stem kernel, told apart by the geometry).  The last test of the module asserts the census of what was reached and what a reduced
workspace made decline."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as C
import memguard as mg
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_WS = -3
EPS32 = C.EPS32

# Workspace sizes.
#   full   lib.WORKSPACE_BYTES, what hip/ops.py hands every call: nothing may decline for lack of room, MOGAN_ERR_WS is a failure.
#   small  256 KiB, picked from the code so that the "does not fit" branches are taken:
#            - mogan_wino_try: below the smallest filter image of the tables (ceil(Kout / 96) * 8 * (Kin / 16) * 18 KiB + 18 KiB
#              = 306 KiB at Kin = 32), so every Winograd forward / data gradient declines (`u3bytes > ws_bytes`);
#            - mogan_wino_wgrad_try: above the smallest K-split slab (16 * Cout * Cin floats = 128 KiB at 64 x 32) and below two of
#              them, so the split is clamped (`nsplit * slab > ws_bytes`) for that case and the kernel declines for every larger one;
#            - the direct kernels: above the flipped filters of the smallest data gradient (64 * 64 * 9 floats = 144 KiB + 256), so
#              mogan_dconv_dgrad_try passes its first check and declines at the prepared filters (`ws_bytes < wpb + 256`), as the
#              forward does at once; dconv2's own check likewise;
#            - run_gemm / run_pk: `fit < 2` (no split-K) for outputs over 32 Ki floats, `min(nsplit, fit)` for smaller ones;
#            - sc_wgrad3x3: the per-block partials of the larger maps do not fit, the kernel declines;
#            - the packed entry points: under the pixel panels of the larger PK_CASES (MOGAN_ERR_WS); for the others the panel fits
#              and the slabs behind it do not.
#   null   (NULL, 0): no workspace at all; entry points that need one by contract (mogan_upconv3x3_*, the packed ones) answer
#          MOGAN_ERR_WS and write nothing.
SMALL_WS = 256 << 10
WS_SIZES = ("full", "small", "null")
# the reduced sizes run for the two default dispatches and one forced configuration with a split
REDUCED_FORCES = ((-1, 0), (-2, 0), (0, 3))
REDUCED_PK_FORCES = ((-1, 0), (1, 3))
REDUCED_PK_WGRAD_FORCES = ((-1, 0), (2, 3))

MODES = {0: ("gemm", "fwd"), 1: ("gemm", "dgrad"), 2: ("gemm", "wgrad"), 4: ("off", "fwd"), 5: ("off", "dgrad"), 6: ("off", "wgrad"),
         7: ("pk", "fwd"), 8: ("pk", "dgrad"), 9: ("pk", "wgrad")}
OFF_GEMM = {1: "wino8", 3: "wino16", 0: "direct", 2: "dconv2"}

REACHED = set()        # (family, direction of the kernel) with the full workspace
DECLINED = set()       # (family, direction of the kernel) taken with the full workspace and not with a reduced one
FIGURES = {}           # (family, direction of the entry point) -> [largest err / S, largest rel-L2]
LRELU = {"taken": 0, "declined": 0}
RAN = set()


def L():
    return lib.load()


class _WS:
    def __init__(self):
        self.bufs = {"full": mg.Banded((lib.WORKSPACE_BYTES,), torch.uint8, DEV), "small": mg.Banded((SMALL_WS,), torch.uint8, DEV)}

    def args(self, kind):
        if kind == "null":
            return None, 0
        b = self.bufs[kind]
        mg.poison_(b.t)
        return b.t.data_ptr(), b.t.numel()

    def intact(self):
        return all(b.intact() for b in self.bufs.values())


@pytest.fixture(scope="module")
def ws():
    return _WS()


@pytest.fixture(scope="module", autouse=True)
def _launch_records():
    """the measurement hook is process-wide: on for this module only"""
    L().mogan_prof_enable(1)
    yield
    L().mogan_prof_enable(0)


def _rows():
    buf = (ctypes.c_double * (5 * 64))()
    n = L().mogan_prof_collect(buf, 64)
    return {(int(buf[5 * i]), int(buf[5 * i + 1])) for i in range(n)}


def _families(rows, geom):
    """{(family, kernel direction)} of a call's launch records; no record: small-channel or stem kernel by the geometry"""
    out = set()
    for mode, cfg in rows:
        kind, d = MODES[mode]
        out.add((("gemm%d" % cfg) if kind == "gemm" else OFF_GEMM[cfg] if kind == "off" else "pk", d))
    if not out:
        entry, Cin, Cout, k, s = geom
        assert min(Cin, Cout) <= 4, "no launch record, and not a small-channel geometry: %s" % (geom,)
        out.add(("stem" if entry == "fwd" and Cin == 3 and k == (4, 4) and s == 2 and Cout > 4 else "smallc", entry))
    return out


def _group(fam):
    return "wino" if fam.startswith("wino") else "direct" if fam in ("direct", "dconv2") else fam


def _inp(t):
    """an input inside NaN guard bands, frozen (bands included)"""
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, base=t.to(DEV))
    g.frozen = mg.Frozen(g.buf)
    return g


@functools.lru_cache(maxsize=None)
def _case(kind, case):
    """inputs on the device and fp64 references of a table row, shared by the forces"""
    cc = C.as_conv_case(case, "conv" if kind == "conv" else "up" if kind == "up" else "pk")
    x, w, g = C.conv_inputs(case) if kind == "conv" else C.up_inputs(case) if kind == "up" else C.pk_inputs(case, kind == "pw")
    B, Cin, H, W, Cout, k, s, pad, up = cc
    ref, S = C.references(x, w, g, s, pad, up)
    return dict(cc=cc, x=_inp(x), w=_inp(w), g=_inp(g), w_cpu=w, ref=ref, S=S, dwbase=C.T("base%s%s" % (kind, case), tuple(w.shape)))


def _run(call, out_shape, ref, S, entry, geom, inputs, ws, wsk, what, base=None, allow_rc1=False, extra_tol=0.0, helper=None):
    """one entry point under the whole contract.  call(out_ptr, ws_ptr, ws_bytes) -> return code.  Returns (families, Guarded).
    helper = (name, tol): an elementwise kernel beside the convolutions (no launch record, its own rounding bound)."""
    out = mg.Guarded(tuple(out_shape), (Ellipsis,), DEV, base=None if base is None else base.to(DEV))
    wsp, wsn = ws.args(wsk)
    _rows()
    rc = call(out.ptr, wsp, wsn)
    torch.cuda.synchronize()
    rows = _rows()
    assert ws.intact(), "%s: the bands of the workspace changed" % what
    for t in inputs:
        t.frozen.check(what)
    if rc == ERR_WS or (allow_rc1 and rc == 1):
        assert rc == 1 or wsk != "full", "%s: MOGAN_ERR_WS with the full workspace" % what
        assert out.untouched(), "%s: return code %d, but the output was written" % (what, rc)
        assert not rows, "%s: return code %d after a launch %s" % (what, rc, rows)
        return {("errws" if rc == ERR_WS else "rc1", entry)}, out
    assert rc == 0, "%s: return code %d" % (what, rc)
    if helper:
        assert not rows, "%s: launch records %s" % (what, rows)
    fams = {(helper[0], entry)} if helper else _families(rows, geom)
    wino = any(f.startswith("wino") for f, _ in fams)
    tol = helper[1] if helper else (C.TOL_WINO if wino else C.TOL)[entry] + extra_tol
    ref, S = ref.double(), S.double()
    bound = tol * S
    if base is not None:
        b64 = base.double()
        ref, bound = ref + b64, bound + 2 * EPS32 * (b64.abs() + S)
    got = out.view.cpu().double()
    err = (got - ref).abs()
    frac = float(torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf")).max())       # the part of the bound that is used
    rel = float(err.norm() / (ref.norm() + 1e-30))
    for f, _ in fams:
        fig = FIGURES.setdefault((f, entry), [0.0, 0.0])
        fig[0], fig[1] = max(fig[0], frac * tol), max(fig[1], rel if rel == rel else float("inf"))
    tag = "%s [%s, ws %s]" % (what, "+".join(sorted(f for f, _ in fams)), wsk)
    out.check(ref, bound, what=tag + " (largest err / bound %.2f, rel-L2 %.2e)" % (frac, rel))
    assert rel <= C.REL_L2, "%s: rel-L2 %.3e > %.1e" % (tag, rel, C.REL_L2)
    # the same call again: same bits
    first = out.view.clone()
    out.reset()
    wsp, wsn = ws.args(wsk)
    rc2 = call(out.ptr, wsp, wsn)
    torch.cuda.synchronize()
    rows2 = _rows()
    assert rc2 == 0 and (helper or _families(rows2, geom) == fams), "%s: the second call took another path" % tag
    assert torch.equal(first.view(torch.int32), out.view.view(torch.int32)), "%s: the second call gave other bits" % tag
    assert ws.intact() and out.problems() == [], "%s: second call: %s" % (tag, out.problems())
    return fams, out


def _census(full, fams, wsk):
    """full: the families of the same call with the full workspace"""
    if wsk == "full":
        REACHED.update(fams)
        return
    for f, d in full:
        if _group(f) in ("wino", "direct", "pk") and (f, d) not in fams:
            DECLINED.add((_group(f), d))


def _sizes(force, reduced):
    return WS_SIZES if tuple(force) in reduced else ("full",)


# ------------------------------------------------------------------------------- mogan_conv2d_fwd / _dgrad / _wgrad, down2_sum
@pytest.mark.parametrize("case", C.CONV_CASES)
@pytest.mark.parametrize("force", C.FORCES)
def test_conv2d_fwd_dgrad_wgrad(case, force, ws):
    d = _case("conv", case)
    B, Cin, H, W, Cout, k, s, pad, up = case
    dims = (B, Cin, H, W, Cout, k[0], k[1], s, pad[0], pad[1], up)
    st = lib.stream_ptr()
    x, w, g, ref, S = d["x"], d["w"], d["g"], d["ref"], d["S"]
    what = "%s force %s" % (case, force)
    RAN.add(("conv", case, force))
    L().mogan_gemm_debug_force(*force)
    try:
        full = {}
        for wsk in _sizes(force, REDUCED_FORCES):
            runs = [
                ("fwd", "y", lambda o, p, n: L().mogan_conv2d_fwd(x.ptr, w.ptr, o, *dims, p, n, st), (x, w), None),
                ("dgrad", "dxu", lambda o, p, n: L().mogan_conv2d_dgrad(g.ptr, w.ptr, o, *dims, p, n, st), (g, w), None),
                ("wgrad", "dw", lambda o, p, n: L().mogan_conv2d_wgrad(g.ptr, x.ptr, o, *dims, 0, p, n, st), (g, x), None),
                ("wgrad", "dw", lambda o, p, n: L().mogan_conv2d_wgrad(g.ptr, x.ptr, o, *dims, 1, p, n, st), (g, x), d["dwbase"]),
            ]
            for i, (entry, key, call, inputs, base) in enumerate(runs):
                fams, out = _run(call, ref[key].shape, ref[key], S[key], entry, (entry, Cin, Cout, k, s), inputs, ws, wsk,
                                 "%s %s%s" % (what, entry, " accumulate" if base is not None else ""), base=base)
                if wsk == "full":
                    full[i] = fams
                _census(full[i], fams, wsk)
                if entry == "dgrad" and up and wsk == "full" and fams:
                    # the gradient at the resolution of x: sums of 2x2 blocks of what the kernel just wrote (three more roundings)
                    du = _inp(out.view)
                    _run(lambda o, p, n: L().mogan_down2_sum(du.ptr, o, B * Cin, H, W, st), ref["dx"].shape, ref["dx"], S["dx"], "dgrad",
                         None, (du,), ws, wsk, what + " down2_sum", helper=("down2", C.TOL["dgrad"] + 3 * EPS32))
    finally:
        L().mogan_gemm_debug_force(-1, 0)


def test_winograd_geometries_are_the_ones_the_dispatch_takes():
    """conv_cases.wino_geometry (which cases the CPU file measures the Winograd emulation on) against mogan_wino_prep_bytes"""
    if L().mogan_mfma_form() != 6:
        return
    for case in C.CONV_CASES:
        B, Cin, H, W, Cout, k, s, pad, up = case
        got = tuple(bool(L().mogan_wino_prep_bytes(B, Cin, H, W, Cout, k[0], k[1], s, pad[0], pad[1], up, dg)) for dg in (0, 1))
        assert got == C.wino_geometry(case)[:2], (case, got)


# ------------------------------------------------------------------------ prepared filter images: mogan_conv2d_fwd_wp / _dgrad_wp
@pytest.mark.parametrize("case", C.CONV_CASES)
def test_conv2d_with_prepared_filter_images(case, ws):
    """an image from mogan_conv_prep_group (3x3 s1: the Winograd kernels'; 4x4 s2: dconv2_fwd_kernel's), sized by
    mogan_conv_prep_bytes, in a guarded byte buffer; the convolution then runs with every workspace size -- with the image the
    Winograd kernels do not need one"""
    d = _case("conv", case)
    B, Cin, H, W, Cout, k, s, pad, up = case
    dims = (B, Cin, H, W, Cout, k[0], k[1], s, pad[0], pad[1], up)
    st = lib.stream_ptr()
    x, w, g, ref, S = d["x"], d["w"], d["g"], d["ref"], d["S"]
    RAN.add(("wp", case))
    for dg, entry, key, src in ((0, "fwd", "y", x), (1, "dgrad", "dxu", g)):
        nb = int(L().mogan_conv_prep_bytes(*dims, dg))
        if not nb:
            continue
        img = mg.Guarded((nb,), (Ellipsis,), DEV, dtype=torch.uint8)
        arrs = [(ty * 1)(v) for ty, v in ((ctypes.c_void_p, w.ptr), (ctypes.c_void_p, img.ptr), (ctypes.c_int, Cout), (ctypes.c_int, Cin),
                                          (ctypes.c_int, k[0]), (ctypes.c_int, dg))]
        rc = L().mogan_conv_prep_group(1, *[ctypes.cast(a, ctypes.c_void_p) for a in arrs], st)
        torch.cuda.synchronize()
        assert rc == 0
        img.check(what="%s image %d" % (case, dg), written=False)      # (bytes may equal the poison; the tail is padding)
        w.frozen.check("prep")
        img.frozen = mg.Frozen(img.buf)
        name = "mogan_conv2d_fwd_wp" if dg == 0 else "mogan_conv2d_dgrad_wp"
        full = None
        for wsk in WS_SIZES:
            fams, _ = _run(lambda o, p, n: getattr(L(), name)(src.ptr, w.ptr, img.ptr, o, *dims, p, n, st), ref[key].shape, ref[key],
                           S[key], entry, (entry, Cin, Cout, k, s), (src, w, img), ws, wsk, "%s %s" % (case, name))
            full = full or fams
            if wsk == "full":
                REACHED.update(fams)
            if k == (3, 3):
                assert fams == full and _group(next(iter(fams))[0]) == "wino", "%s: with an image the Winograd kernel needs no workspace: %s" % (case, fams)


# ------------------------------------------------------------------------------------------------------- mogan_upconv3x3_*
_TM = [[0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]]


@pytest.mark.parametrize("case", C.UP_CASES)
@pytest.mark.parametrize("force", [(-1, 0), (-2, 0), (0, 3)])
def test_upconv3x3_k4_fwd_dgrad_wgrad(case, force, ws):
    """nearest x2 + conv3x3 p1 as the transposed 4x4 s2 convolution with K = T w T^t: K itself (two roundings of sums of up to four
    filter taps), forward, data gradient at the source resolution, weight gradient written and accumulated.  The entry points
    need the workspace for K (include/mogan_hip.h): MOGAN_ERR_WS, nothing written, where it does not fit."""
    d = _case("up", case)
    B, Cin, H, W, Cout = case
    st = lib.stream_ptr()
    x, w, g, ref, S = d["x"], d["w"], d["g"], d["ref"], d["S"]
    what = "up %s force %s" % (case, force)
    RAN.add(("up", case, force))
    if force == (-1, 0):
        Tm = torch.tensor(_TM, dtype=torch.float64)
        w64 = d["w_cpu"].double()
        _run(lambda o, p, n: L().mogan_upconv3x3_k4(w.ptr, o, Cout, Cin, st), (Cin, Cout, 4, 4), torch.einsum("ai,ocij,bj->coab", Tm, w64, Tm),
             torch.einsum("ai,ocij,bj->coab", Tm, w64.abs(), Tm), "fwd", None, (w,), ws, "full", what + " k4", helper=("k4", 2 * EPS32))
    L().mogan_gemm_debug_force(*force)
    try:
        full = {}
        for wsk in WS_SIZES:
            runs = [
                ("fwd", "y", lambda o, p, n: L().mogan_upconv3x3_fwd(x.ptr, w.ptr, o, B, Cin, H, W, Cout, p, n, st), (x, w), None),
                ("dgrad", "dx", lambda o, p, n: L().mogan_upconv3x3_dgrad(g.ptr, w.ptr, o, B, Cin, H, W, Cout, p, n, st), (g, w), None),
                ("wgrad", "dw", lambda o, p, n: L().mogan_upconv3x3_wgrad(g.ptr, x.ptr, o, B, Cin, H, W, Cout, 0, p, n, st), (g, x), None),
                ("wgrad", "dw", lambda o, p, n: L().mogan_upconv3x3_wgrad(g.ptr, x.ptr, o, B, Cin, H, W, Cout, 1, p, n, st), (g, x),
                 d["dwbase"]),
            ]
            for i, (entry, key, call, inputs, base) in enumerate(runs):
                fams, _ = _run(call, ref[key].shape, ref[key], S[key], entry, (entry, Cin, Cout, (4, 4), 2), inputs, ws, wsk,
                               "%s %s%s" % (what, entry, " accumulate" if base is not None else ""), base=base)
                assert wsk != "null" or fams == {("errws", entry)}, "%s: no workspace for K, and no MOGAN_ERR_WS" % what
                if wsk == "full":
                    full[i] = fams
                _census(full[i], fams, wsk)
    finally:
        L().mogan_gemm_debug_force(-1, 0)


# ------------------------------------------------------------------------------------------------ mogan_conv2d_lrelu_fwd
@pytest.mark.parametrize("case", [c for c in C.CONV_CASES if c[8] == 0])
@pytest.mark.parametrize("force", [(-1, 0), (0, 3)])
def test_conv2d_lrelu_fwd_or_untouched(case, force, ws):
    """z = LeakyReLU_0.2(conv2d(x, w)); return code 1 = "not my geometry" leaves z untouched"""
    d = _case("conv", case)
    B, Cin, H, W, Cout, k, s, pad, up = case
    st = lib.stream_ptr()
    x, w = d["x"], d["w"]
    RAN.add(("lrelu", case, force))
    ref = F.leaky_relu(d["ref"]["y"], 0.2)
    L().mogan_gemm_debug_force(*force)
    try:
        for wsk in ("full", "null"):
            fams, _ = _run(lambda o, p, n: L().mogan_conv2d_lrelu_fwd(x.ptr, w.ptr, o, B, Cin, H, W, Cout, k[0], k[1], s, pad[0], pad[1],
                                                                       0.2, p, n, st),
                           ref.shape, ref, d["S"]["y"], "fwd", ("fwd", Cin, Cout, k, s), (x, w), ws, wsk,
                           "%s force %s lrelu" % (case, force), allow_rc1=True, extra_tol=EPS32)
            LRELU["declined" if fams == {("rc1", "fwd")} else "taken"] += 1
            if wsk == "full" and fams != {("rc1", "fwd")}:
                REACHED.update(fams)
    finally:
        L().mogan_gemm_debug_force(-1, 0)


# ----------------------------------------------------------------------------------------------------- packed-weight kernels
def _pack(w, Cout, Cin, k, s, pad, dg, fill):
    nb = int(L().mogan_pk_weight_bytes(Cout, Cin, k, k, s, dg))
    assert nb > 0
    p = mg.Guarded((nb,), (Ellipsis,), DEV, dtype=torch.uint8, base=torch.full((nb,), fill, dtype=torch.uint8))
    rc = L().mogan_pk_weight_pack(w.ptr, p.ptr, Cout, Cin, k, k, s, pad, pad, dg, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    p.check(what="pk_weight_pack dgrad=%d" % dg)
    w.frozen.check("pk_weight_pack")
    p.frozen = mg.Frozen(p.buf)
    return p


@functools.lru_cache(maxsize=None)
def _packs(case):
    """forward- and data-gradient-packed copies of a PK_CASES weight.  Every byte of a copy is written: two packs into buffers
    pre-filled with different bytes agree; mogan_pk_weight_pack_both gives the same two copies from one read of w."""
    d = _case("pk", case)
    B, Cin, H, W, Cout, k, s, pad = case
    out = []
    for dg in (0, 1):
        a, b = _pack(d["w"], Cout, Cin, k, s, pad, dg, 0x00), _pack(d["w"], Cout, Cin, k, s, pad, dg, 0xFF)
        assert torch.equal(a.view, b.view), "pk_weight_pack dgrad=%d of %s leaves bytes of the copy unwritten" % (dg, case)
        out.append(a)
    both = [mg.Guarded(tuple(p.view.shape), (Ellipsis,), DEV, dtype=torch.uint8, base=torch.full(tuple(p.view.shape), 0x5A, dtype=torch.uint8))
            for p in out]
    rc = L().mogan_pk_weight_pack_both(d["w"].ptr, both[0].ptr, both[1].ptr, Cout, Cin, k, k, s, pad, pad, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    for dg in (0, 1):
        both[dg].check(out[dg].view, exact=True, what="pk_weight_pack_both %s copy %d" % (case, dg))
    d["w"].frozen.check("pk_weight_pack_both")
    return out


@pytest.mark.parametrize("case", C.PK_CASES)
@pytest.mark.parametrize("force", C.PK_FORCES)
def test_packed_weight_fwd_dgrad(case, force, ws):
    d = _case("pk", case)
    B, Cin, H, W, Cout, k, s, pad = case
    dims = (B, Cin, H, W, Cout, k, k, s, pad, pad)
    st = lib.stream_ptr()
    x, g, ref, S = d["x"], d["g"], d["ref"], d["S"]
    wf, wd = _packs(case)
    RAN.add(("pk", case, force))
    L().mogan_pk_debug_force(1, *force)
    try:
        for entry, key, name, src, wp in (("fwd", "y", "mogan_conv2d_fwd_pk", x, wf), ("dgrad", "dx", "mogan_conv2d_dgrad_pk", g, wd)):
            full = None
            for wsk in _sizes(force, REDUCED_PK_FORCES):
                fams, _ = _run(lambda o, p, n: getattr(L(), name)(src.ptr, wp.ptr, o, *dims, p, n, st), ref[key].shape, ref[key], S[key],
                               entry, (entry, Cin, Cout, (k, k), s), (src, wp), ws, wsk, "%s force %s %s" % (case, force, name))
                full = full or fams
                assert wsk != "full" or fams == {("pk", entry)}, fams
                _census(full, fams, wsk)
    finally:
        L().mogan_pk_debug_force(0, -1, 0)


@pytest.mark.parametrize("case", C.PK_WGRAD_CASES)
@pytest.mark.parametrize("force", C.PK_WGRAD_FORCES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_packed_weight_gradient(case, force, accumulate, ws):
    d = _case("pw", case)
    B, Cin, H, W, Cout, k, s, pad = case
    st = lib.stream_ptr()
    x, g, ref, S = d["x"], d["g"], d["ref"], d["S"]
    RAN.add(("pw", case, force, accumulate))
    L().mogan_pk_debug_force(1, *force)
    try:
        full = None
        for wsk in _sizes(force, REDUCED_PK_WGRAD_FORCES):
            fams, _ = _run(lambda o, p, n: L().mogan_conv2d_wgrad_pk(g.ptr, x.ptr, o, B, Cin, H, W, Cout, k, k, s, pad, pad, accumulate, p, n, st),
                           ref["dw"].shape, ref["dw"], S["dw"], "wgrad", ("wgrad", Cin, Cout, (k, k), s), (g, x), ws, wsk,
                           "%s force %s wgrad_pk accumulate=%d" % (case, force, accumulate), base=d["dwbase"] if accumulate else None)
            full = full or fams
            assert wsk != "full" or fams == {("pk", "wgrad")}, fams
            _census(full, fams, wsk)
    finally:
        L().mogan_pk_debug_force(0, -1, 0)


# ------------------------------------------------------------------------------------------------------------------ census
def test_census_of_the_kernels_reached_and_declined():
    """Every kernel family of the dispatch was reached by at least one case with the full workspace, in every direction it has, and
    every family that needs workspace was seen to step aside for a reduced one.  Winograd 8-wave (wino3_fwd_kernel) and 16-wave
    (wino5_fwd_kernel) are told apart by the launch record (cfg 1 / 3).  The direct weight gradient is not in the declined set:
    it needs no workspace (a short one only shrinks its pixel-tile split, dconv.hip launch_wgrad)."""
    for key in sorted(FIGURES):
        print("%-8s %-5s largest err / S = %.3e   largest rel-L2 = %.3e" % (key + tuple(FIGURES[key])))
    print("reached: %s\ndeclined: %s\nlrelu: %s" % (sorted(REACHED), sorted(DECLINED), LRELU))
    want_ran = ({("conv", c, f) for c in C.CONV_CASES for f in C.FORCES} | {("wp", c) for c in C.CONV_CASES}
                | {("up", c, f) for c in C.UP_CASES for f in [(-1, 0), (-2, 0), (0, 3)]}
                | {("lrelu", c, f) for c in C.CONV_CASES if c[8] == 0 for f in [(-1, 0), (0, 3)]}
                | {("pk", c, f) for c in C.PK_CASES for f in C.PK_FORCES}
                | {("pw", c, f, a) for c in C.PK_WGRAD_CASES for f in C.PK_WGRAD_FORCES for a in (0, 1)})
    if RAN != want_ran:
        pytest.skip("the census needs every test of this module to have run (a selection was made)")
    gemms = ["gemm%d" % f[0] for f in C.FORCES if f[0] >= 0]
    want = {(f, "fwd") for f in ["smallc", "stem", "wino8", "wino16", "direct", "dconv2", "pk"] + gemms}
    want |= {(f, "dgrad") for f in ["smallc", "wino8", "wino16", "direct", "dconv2", "pk"] + gemms}
    want |= {(f, "wgrad") for f in ["smallc", "wino8", "direct", "pk"] + gemms}
    assert not want - REACHED, "never reached with the full workspace: %s" % sorted(want - REACHED)
    want_declined = {(f, d) for f in ("wino", "direct", "pk") for d in ("fwd", "dgrad", "wgrad")} - {("direct", "wgrad")}
    assert not want_declined - DECLINED, "never declined for a reduced workspace: %s" % sorted(want_declined - DECLINED)
    assert LRELU["taken"] > 0 and LRELU["declined"] > 0, LRELU
