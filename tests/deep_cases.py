"""Rows, inputs, staged fp64 references and per-element bounds of the deep-block entry points of include/mogan_hip.h --
mogan_deep_conv_bn_act_fwd / _bwd (csrc/mogan_pgemm.hip): the packed-weight GEMM followed by one tail kernel each way -- a plain
helper module, not a conftest, like tests/conv_cases.py and tests/bn_cases.py, whose inputs, references and tolerances it reuses.
tests/test_deep_entry_points_gpu.py runs the rows through the C ABI under tests/memguard.py; tests/test_deep_reference_cpu.py
keeps the references equal to torch in fp64, holds fp32 CPU evaluations to a quarter of the tolerances and asserts the coverage
and the band condition below; tests/test_deep_rejections_cpu.py holds what the host answers before a launch.  Nothing here needs
a GPU or the library (the three panel helpers at the end load it when they are called).

What decides the code a row runs, restated from the words of the header and the head of the tail kernels (not read from the library):
    class       NE = (B / groups) * OH * OW values per (channel, group) in the registers of half a wave: 8 per lane for NE <= 256,
                16 for NE <= 512, 32 for NE <= 1024, 64 up to 2048 (two groups: NE <= 1024, so at most 32)
    K-split     ntile = KH * KW * Cin / 32 K-tiles; a forced split asks for n = min(split, ntile) ranges; a range is whole trips of
                six tiles: kt_per = ceil(ceil(ntile / n) / 6) * 6; slabs = ceil(ntile / kt_per).  A workspace with room for fewer
                than two slabs behind the panel: one slab, stored straight into y; room for fewer than asked: that many.
    slab loop   the tail adds slabs 1 .. slabs-1 to slab 0 in trips of SB = 4 (class 8), 2 (class 16), 1 (classes 32, 64) and a
                remainder loop: (slabs - 1) // SB whole trips, (slabs - 1) % SB remainder passes.  One slab: the GEMM has stored
                into y itself and the tail does not write y again.
    LDS         with a panel to write, 8 channels x NE x groups fp32: two groups at NE = 1024 are 64 KB, the one size above the
                default limit (the launch raises the kernel's attribute first).

References are staged, so that one stage's error does not blur the next one's bound:
    y                      fp64 convolution of x                                  conv_cases.TOL["fwd"] * sum |x| |w|
    stats, z, running      bn_cases.bn_forward of the y THE KERNEL WROTE (fp64)   bn_cases.bound (groups: grouped_reference's form)
    dy, dgamma, dbeta      bn_cases.bn_backward of that y and the given dz        bn_cases.bound
    dx                     fp64 transposed convolution of the dy the kernel wrote TOL_DX * sum |dy| |w| (see MEASURED below)
and one end-to-end fp64 chain from x (chain), compared with the whole-tensor figures of test_deep_block_conv_bn_act only; its
gradients are taken on the kernel's side of the kink where the two disagree inside the band (chain_on_the_side_of).

The activation kink.  y is a convolution output and cannot be nudged off a kink as bn_cases._unkink nudges x.  For RELU / LRELU
an element is IN THE BAND when |fp64 pre-activation| < KINK * TOL["y"] * S_t.  Outside the band the sign of z must be the
reference's; inside, z gets its bound widened by the band's width, and the backward reference takes the derivative's side from
the sign of the z the kernel wrote (the backward recomputes the same fp32 expression from the same y and stats).  At most
BAND_SHARE of a row's elements may lie in the band: the CPU module checks that on every row with the fp32 CPU evaluation of y.

Special channels, every row: gamma[1] < 0, gamma[2] == 0.  The geometry CONST_GEOM has a constant channel of x and -- since a
constant input channel does not make a convolution output constant -- an all-zero filter ZERO_FILTER: that channel of y is 0
everywhere, its variance 0, invstd = 1 / sqrt(eps), its pre-activation beta = -0.25 exactly.
"""
import functools
import math

import torch
import torch.nn.functional as F

import bn_cases as BN
import conv_cases as CV

NONE, RELU, LRELU = BN.NONE, BN.RELU, BN.LRELU
BAND_SHARE = 0.01
ZERO_FILTER, NEG_GAMMA, ZERO_GAMMA = 3, 1, 2

# fp32 CPU evaluations of the staged formulas on these rows, largest (err - F) / S in units of 2^-24 (test_deep_reference_cpu
# measures and prints them and asserts them <= a quarter of the constant each output is held to):
#     y (torch fp32 conv2d) 2.74   z 3.12   dy 3.39   d gamma / d beta 0.31  (numpy restatement of csrc/mogan_bn.h)
#     dx (torch fp32 conv2d_input of the fp32 dy) 6.19
# y, z, dy and the parameter gradients stay within a quarter of conv_cases.TOL["fwd"] and bn_cases.TOL, which are reused as they
# are.  dx does not: a quarter of conv_cases.TOL["dgrad"] is 5.45 x 2^-24, and torch's fp32 data gradient of the 4x4 stride-2 rows
# needs up to 6.19 x 2^-24 = 3.69e-7 (five rows between 5.74 and 6.19: sums of 4 taps x 32 .. 96 channels per parity class, where a
# few elements out of 10^5 .. 10^6 land that far out).  That is a finding about the yardstick on these rows; dx is held to TOL_DX,
# 4 x the measured figure and far under the ceiling, instead.
MEASURED = {"y": 2.75 * BN.EPS32, "dx": 6.20 * BN.EPS32, "z": 3.13 * BN.EPS32, "dy": 3.40 * BN.EPS32, "dparam": 0.32 * BN.EPS32}
TOL_DX = 1.48e-6
assert CV.TOL["dgrad"] < TOL_DX <= BN.TOL_CEILING

ROWS = [
    # B, groups, Cin, Hs, Ws, Cout, k, stride, pad, act, forced split
    (3, 1, 64, 4, 4, 96, 3, 1, 1, RELU, 1),        # class 8, NE 48 (ragged half wave 32 + 16): one slab, the direct store
    (3, 1, 64, 4, 4, 96, 3, 1, 1, LRELU, 3),       #   3 slabs: remainder loop only
    (2, 1, 32, 6, 6, 32, 5, 1, 2, NONE, 5),        #   NE 72, ntile 25: 5 slabs, exactly one trip of four
    (4, 1, 64, 8, 8, 64, 4, 2, 1, LRELU, 6),       #   NE 64, ntile 32: 6 slabs, a trip and a remainder pass
    (10, 2, 64, 3, 3, 32, 3, 1, 1, RELU, 3),       #   two groups of NE 45 (odd HW = 9)
    (5, 1, 32, 16, 16, 32, 4, 2, 1, NONE, 2),      # class 16, NE 320, ntile 16: 2 slabs, remainder only
    (5, 1, 32, 16, 16, 32, 4, 2, 1, RELU, 3),      #   3 slabs: one trip of two
    (5, 1, 64, 16, 16, 32, 4, 2, 1, LRELU, 6),     #   ntile 32: 6 slabs, two trips and a remainder pass
    (10, 2, 32, 16, 16, 32, 4, 2, 1, LRELU, 3),    #   two groups
    (16, 1, 32, 16, 16, 96, 4, 2, 1, LRELU, 1),    # class 32, NE 1024
    (16, 1, 32, 16, 16, 96, 4, 2, 1, NONE, 3),
    (32, 2, 32, 16, 16, 96, 4, 2, 1, RELU, 1),     #   two groups: 64 KB of LDS
    (32, 2, 32, 16, 16, 96, 4, 2, 1, LRELU, 3),
    (32, 1, 32, 16, 16, 32, 4, 2, 1, RELU, 1),     # class 64, NE 2048
    (32, 1, 32, 16, 16, 32, 4, 2, 1, LRELU, 3),
    (32, 1, 32, 16, 16, 32, 4, 2, 1, NONE, 0),     #   the heuristic's own split: >= 1 slab is all that is asserted
]
TILE_ROW = ROWS[6]                 # also under the three forced tile shapes, mogan_pk_debug_force(1, 0..2, split)
VARIANT_ROWS = (ROWS[1], ROWS[4])  # one small row per group count for the nullable arguments
CONST_GEOM = ROWS[0][:9]


def row_id(row):
    return "B%d-G%d-%dx%dx%d-to%d-k%ds%dp%d-%s-split%d" % (row[:9] + (BN.ACT_NAMES[row[9]], row[10]))


def geom(row):
    """-> dict over B, G, Cin, Hs, Ws, Cout, k, s, pad, OH, OW, HW, NE, ntile, ntile_d (K-tiles per parity class of the data gradient)"""
    B, G, Cin, Hs, Ws, Cout, k, s, pad = row[:9]
    OH, OW = (Hs + 2 * pad - k) // s + 1, (Ws + 2 * pad - k) // s + 1
    return dict(B=B, G=G, Cin=Cin, Hs=Hs, Ws=Ws, Cout=Cout, k=k, s=s, pad=pad, OH=OH, OW=OW, HW=OH * OW, NE=B // G * OH * OW,
                ntile=k * k * Cin // 32, ntile_d=(k // s) * (k // s) * Cout // 32)


def ept_class(NE, G=1):
    e = 8 if NE <= 256 else 16 if NE <= 512 else 32 if NE <= 1024 else 64
    return min(e, 32) if G == 2 else e


def slabs_of(ntile, split, room=None):
    """slabs of a forced split (split >= 1); room: how many slabs the workspace holds behind the panel (None: enough)"""
    n = min(split, ntile)
    if room is not None and n > 1:
        n = 1 if room < 2 else min(n, room)
    kt_per = -(-(-(-ntile // n)) // 6) * 6
    return -(-ntile // kt_per)


def loop_shape(ept, slabs):
    """(whole trips, remainder passes) of the tail's slab loop"""
    sb = {8: 4, 16: 2, 32: 1, 64: 1}[ept]
    return (slabs - 1) // sb, (slabs - 1) % sb


def up256(v):
    return (v + 255) & ~255


def fwd_ws_bytes(row, slabs):
    g = geom(row)
    return up256(g["B"] * g["Hs"] * g["Ws"] * g["Cin"] * 6) + slabs * 4 * g["B"] * g["Cout"] * g["HW"]


def bwd_ws_bytes(row, slabs):
    g = geom(row)
    return up256(g["B"] * g["HW"] * g["Cout"] * 6) + slabs * 4 * g["B"] * g["Cin"] * g["Hs"] * g["Ws"]


# --------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(geometry):
    """x, w, gamma, beta, rm, rv, dz, the bases of the accumulating d gamma / d beta (fp32 tensors) of a row's first nine fields"""
    B, G, Cin, Hs, Ws, Cout, k, s, pad = geometry
    g = geom(geometry)
    tag = str(geometry)
    x, w = CV.T("dpx" + tag, (B, Cin, Hs, Ws)), CV.T("dpw" + tag, (Cout, Cin, k, k), 0.1)
    gamma, beta = CV.T("dpg" + tag, (Cout,), 0.3, 1.0), CV.T("dpb" + tag, (Cout,), 0.2)
    gamma[NEG_GAMMA] = -gamma[NEG_GAMMA].abs() - 0.5
    gamma[ZERO_GAMMA] = 0.0
    if geometry == CONST_GEOM:
        x[:, 0] = BN.CONST_VALUE
        w[ZERO_FILTER] = 0.0
        beta[ZERO_FILTER] = -0.25
    return dict(x=x, w=w, gamma=gamma, beta=beta, rm=CV.T("dprm" + tag, (Cout,), 0.1), rv=CV.T("dprv" + tag, (Cout,), 0.1).abs() + 1,
                dz=CV.T("dpdz" + tag, (B, Cout, g["OH"], g["OW"])), base_g=CV.T("dpbg" + tag, (Cout,)), base_b=CV.T("dpbb" + tag, (Cout,)))


# ------------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def conv_reference(geometry):
    """stage 1: y = conv(x, w) in fp64 and S_y = conv(|x|, |w|)"""
    g, inp = geom(geometry), inputs(geometry)
    ref, S = CV.references(inp["x"], inp["w"], inp["dz"], g["s"], (g["pad"], g["pad"]), 0)
    return ref["y"], S["y"]


def dgrad_reference(geometry, dy):
    """stage 4: dx = the transposed convolution of dy (what the kernel wrote, any dtype) in fp64, and S_dx"""
    g, inp = geom(geometry), inputs(geometry)
    ref, S = CV.references(inp["x"], inp["w"], dy, g["s"], (g["pad"], g["pad"]), 0)
    return ref["dxu"], S["dxu"]


def _kinked(act):
    return act in (RELU, LRELU)


def tail_reference(y, gamma, beta, act, rm, rv, dz, G, z_side=None, one_minus=BN.ONE_MINUS_MOM):
    """stages 2 and 3 on y (B, C, HW; the tensor the kernel wrote): G BatchNorm calls in sequence as bn_cases.grouped_reference makes
    them -- per-group statistics (G, C), running statistics carried from group to group, parameter gradients summed -- with what the
    kink needs beside: band (in the band or not, per element), bw (the band's width), t (the fp64 pre-activation), and, with z_side
    (the z the kernel wrote), the derivative's side inside the band taken from its sign.
    -> ref, S, F, bnd (dicts over mean, invstd, z, rm, rv, dy, dgamma, dbeta; bnd = TOL * S + F, z widened inside the band), extra"""
    per = y.shape[0] // G
    cat = {k: [] for k in ("mean", "invstd", "z", "dy", "band", "bw", "t")}
    Sc, Fc, bc = ({k: [] for k in ("mean", "invstd", "z", "dy")} for _ in range(3))
    ref, S, Fx, bnd = {}, {}, {}, {}
    for g in range(G):
        sl = slice(g * per, (g + 1) * per)
        r, Sf, Ff, ctx = BN.bn_forward(y[sl], gamma, beta, act, None, rm, rv, one_minus=one_minus)
        bw = BN.KINK * BN.TOL["y"] * ctx["S_t"]
        band = (ctx["t"].abs() < bw) if _kinked(act) else torch.zeros_like(bw, dtype=torch.bool)
        for k, src in (("mean", "mean"), ("invstd", "invstd"), ("z", "y")):
            cat[k].append(r[src])
            Sc[k].append(Sf.get(src, torch.zeros_like(r[src]))); Fc[k].append(Ff.get(src, torch.zeros_like(r[src])))
            bc[k].append(BN.bound(src, Sf, Ff) + (bw * band if k == "z" else 0.0))
        cat["band"].append(band); cat["bw"].append(bw); cat["t"].append(ctx["t"])
        for k in ("rm", "rv"):          # the running statistics carry the earlier groups' error on, scaled by 1 - momentum
            bnd[k] = BN.bound(k, Sf, Ff) + (BN.ONE_MINUS_MOM * bnd[k] if k in bnd else 0.0)
            ref[k] = r[k]
        rm, rv = r["rm"], r["rv"]
        if z_side is not None and bool(band.any()):
            side = torch.where(z_side[sl].double() > 0, torch.ones_like(bw), -torch.ones_like(bw))
            ctx = dict(ctx, t=torch.where(band, side, ctx["t"]))
        rb, Sb, Fb = BN.bn_backward(ctx, dz[sl], 1 if G == 1 else 2)
        cat["dy"].append(rb["dx"]); Sc["dy"].append(Sb["dx"]); Fc["dy"].append(torch.zeros_like(rb["dx"]))
        bc["dy"].append(BN.bound("dx", Sb, Fb))
        for k in ("dgamma", "dbeta"):
            ref[k], S[k], Fx[k] = ref.get(k, 0.0) + rb[k], S.get(k, 0.0) + Sb[k], Fx.get(k, 0.0) + Fb[k]
            bnd[k] = bnd.get(k, 0.0) + BN.bound(k, Sb, Fb)
    for k in ("mean", "invstd"):
        ref[k], S[k], Fx[k], bnd[k] = (torch.stack(v[k]) for v in (cat, Sc, Fc, bc))
    for k in ("z", "dy"):
        ref[k], S[k], Fx[k], bnd[k] = (torch.cat(v[k]) for v in (cat, Sc, Fc, bc))
    extra = {k: torch.cat(cat[k]) for k in ("band", "bw", "t")}
    return ref, S, Fx, bnd, extra


def accumulate_bound(key, S, Fx, bnd, base, G):
    """d gamma / d beta added into `base`: bn_cases.bound's accumulate form for one group, test_bn_act_grouped's for two"""
    if G == 1:
        return BN.bound(key, S, Fx, base)
    return bnd[key] + 2 * BN.EPS32 * (base.double().abs() + bnd[key] / BN.EPS32)


def act64(t, act):
    return F.relu(t) if act == RELU else F.leaky_relu(t, BN.SLOPE) if act == LRELU else t


def _chain(geometry, act, side=None):
    """side: per element, which side of the kink the derivative is taken on (None: the side of the chain's own pre-activation)"""
    g, inp = geom(geometry), inputs(geometry)
    x, w, gm, bt = (inp[k].double().clone().requires_grad_(True) for k in ("x", "w", "gamma", "beta"))
    rm, rv = inp["rm"].double().clone(), inp["rv"].double().clone()
    per = g["B"] // g["G"]
    t = torch.cat([F.batch_norm(F.conv2d(x[i * per:(i + 1) * per], w, None, g["s"], g["pad"]), rm, rv, gm, bt, True, BN.MOM, BN.EPS)
                   for i in range(g["G"])])
    z = act64(t, act)
    if side is None:
        z.backward(inp["dz"].double())
    else:
        slope = torch.full_like(t, 0.0 if act == RELU else BN.SLOPE)
        (t * torch.where(side, torch.ones_like(t), slope)).backward(inp["dz"].double())
    return dict(z=z.detach(), t=t.detach(), rm=rm, rv=rv, dx=x.grad, dgamma=gm.grad, dbeta=bt.grad, dw=w.grad)


@functools.lru_cache(maxsize=None)
def chain(geometry, act):
    """the whole block in fp64 from x by torch's own conv2d -> batch_norm(training) -> activation and autograd, groups as calls in
    sequence: z, t (the pre-activation), rm, rv, dx, dgamma, dbeta, dw -- for the whole-tensor figures"""
    return _chain(geometry, act)


def chain_on_the_side_of(geometry, act, z):
    """the chain's gradients with the derivative's side taken from the sign of z (the z the kernel wrote) where that differs from
    the chain's own -- allowed only inside the band, which for the chain is wider by what the convolution's error moves the
    pre-activation: KINK * TOL["y"] * S_t + |sc| * TOL["fwd"] * S_y.  One flipped element of a ReLU changes dx by about 1e-3 of its
    norm, so the whole-tensor figures hold only on the kernel's side of the kink.  -> chain dict, number of elements taken over"""
    c = chain(geometry, act)
    if not _kinked(act):
        return c, 0
    own, theirs = c["t"] > 0, z.double().reshape(c["t"].shape) > 0
    differ = own != theirs
    if not bool(differ.any()):
        return c, 0
    g, inp = geom(geometry), inputs(geometry)
    y, S_y = conv_reference(geometry)
    per = g["B"] // g["G"]
    width = []
    for i in range(g["G"]):
        sl = slice(i * per, (i + 1) * per)
        ctx = BN.bn_forward(y[sl].reshape(per, g["Cout"], g["HW"]), inp["gamma"], inp["beta"], NONE)[3]
        width.append(BN.KINK * BN.TOL["y"] * ctx["S_t"] + ctx["sc"].abs().view(1, -1, 1) * CV.TOL["fwd"] * S_y[sl].reshape(per, g["Cout"], g["HW"]))
    width = torch.cat(width).reshape(c["t"].shape)
    assert bool((c["t"].abs() < width)[differ].all()), "z and the fp64 chain disagree about a sign outside the kink band"
    return _chain(geometry, act, torch.where(differ, theirs, own)), int(differ.sum())


# --------------------------------------------------------------------------------- pixel panels (these load the library)
def _panel_decode(panel, Q, Cp):
    """pixel panel bytes -> (Q, Cp) fp32: the three bf16 pieces of every value add up to it exactly (csrc/mogan_mma.h)"""
    p = panel.view(torch.bfloat16).view(Q, Cp // 32, 3, 32).float()
    return (p[:, :, 0] + p[:, :, 1] + p[:, :, 2]).reshape(Q, Cp)


def _lib():
    from helpers import load_pkg
    load_pkg()
    from mogan_amd.hip import lib
    return lib


def _tail_member(B, n, H, W, srcs, dst=None, dst_bs=0, panel=None, Cp=0, c0=0, scale=None, shift=None, relu=0, box=0, add=None,
                 add_bs=0, mask=None, mask_bs=0):
    a = _lib().TailArgs()
    for j, (t, bs, slab, ns) in enumerate(srcs):
        a.src[j], a.src_bs[j], a.src_slab[j], a.src_nsplit[j] = t, bs, slab, ns
    a.nsrc, a.B, a.n, a.H, a.W, a.relu, a.box = len(srcs), B, n, H, W, relu, box
    if dst is not None:
        a.dst, a.dst_bs = dst, dst_bs
    if panel is not None:
        a.panel, a.CGp, a.cg0 = panel, Cp // 32, c0 // 32
    if scale is not None:
        a.scale, a.shift = scale, shift
    if add is not None:
        a.add, a.add_bs = add, add_bs
    if mask is not None:
        a.mask, a.mask_bs = mask, mask_bs
    return a


def _run_tail(members):
    import ctypes
    lib = _lib()
    arr = (lib.TailArgs * len(members))(*members)
    lib.call("mogan_panel_tail_group", len(members), ctypes.cast(arr, ctypes.c_void_p), lib.stream_ptr())
