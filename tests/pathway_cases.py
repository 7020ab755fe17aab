"""Tables, inputs, fp64 references and per-element bounds of the object-pathway and attention entry points of
include/mogan_hip.h -- mogan_stn_fwd / _bwd / _fwd_ex / _bwd_ex, mogan_bbox_to_theta, mogan_attn_fwd / _bwd, mogan_softmax_fwd /
_bwd, mogan_concat_fwd / _bwd (a plain helper module, not a conftest, like tests/bn_cases.py).
tests/test_pathway_entry_points_gpu.py runs the tables through the C ABI under tests/memguard.py;
tests/test_pathway_reference_cpu.py keeps the references equal to torch in fp64, derives the TOL constants below from fp32 CPU
evaluations and asserts the path coverage; tests/test_pathway_rejections_cpu.py holds what the host refuses before a launch.
Nothing here needs a GPU or the library.

Paths, restated from the words of include/mogan_hip.h and the heads of csrc/mogan_stn_attn.hip / csrc/mogan_elem.hip (not read
from the library):
    stn forward     one thread per output pixel, blocks of 256; the channels of a sample are split over csplit blocks so that
                    about 1024 blocks run: pb = ceil(Hout Wout / 256), csplit = ceil(1024 / (pb B)) clamped to [1, C], then
                    cchunk = ceil(C / csplit) channels per block and csplit = ceil(C / cchunk) (the last chunk may be ragged)
    stn backward    a gather: one thread per source pixel, blocks of 256, 8 channels per thread (one group = C of 8); the
                    output pixels searched are the preimage of the source cell, the WHOLE output when theta is singular
                    (|det| <= 1e-30) or, with align_corners, when a source axis has one pixel.  x_plane: one block per (image,
                    channel), thread t takes the output pixels t, t + 256, ..., then a tree over 256 partial sums
    attention       the words sit in 8, 16 or 32 slots (the smallest that holds T); the channel loops take 8 channels at a time
                    and the rest one by one; one thread per query, blocks of 256.  Limits idf <= 128, T <= 32
    softmax         one thread per (outer, inner) column, blocks of 256; lens is clamped to [0, L]
    concat forward  4 values per thread when HW % 4 == 0 and dst and every non-broadcast source are 16-byte aligned with sb and sg
                    multiples of 4; else one value per thread.  (Beyond 2^26 elements a thread takes several: a grid-stride
                    loop that no small test reaches -- it is not covered here.)
    concat backward non-broadcast sources: one thread per element of the source (a sum over the N / rows repeats when sg = 0);
                    broadcast sources: one wave per (row, channel), lane l sums hw = l, l + 64, ..., then 6 butterfly steps

Bounds.  |got - fp64| <= TOL[kind] * S + F per element, as in bn_cases: S is first order in what an fp32 evaluation can lose, in
units of one rounding; F is 0 everywhere here (no output is a rounded fp64 value).
  stn     y[o] = sum_s tent(ix - sx) tent(iy - sy) x[s] over the in-range source pixels, tent(d) = max(0, 1 - |d|), (ix, iy) the
          source coordinates of output pixel o by the two align_corners formulas of the header.  This dense form needs no floor.
              S_y[o] = sum_s |x[s]| (4 w[s] + Ty[s] Ix[s] S_ix + Tx[s] Iy[s] S_iy)
          w the tent weight (four roundings: the two factors, their product, the product with x; the additions are of at most
          four such terms); S_ix / S_iy the sums over the absolute terms of the coordinate formulas; the tent is 1-Lipschitz, so
          an error d of ix changes w[s] by at most d * tent(iy - sy) -- and only at the source columns within 1 of ix.  A
          coordinate that rounds across an integer moves weight onto a neighbouring pixel: Tx / Ty are the tents and Ix / Iy the
          column / row supports widened by MARGIN * 2^-24 * S_ix, which is more than the coordinate can be off, so that pixel is
          counted.  An absent object (theta_inv = [[-1, 0, -4], [0, -1, -4]]) has S = 0: exact zeros.
          dx[s] is the same matrix transposed (summed over the samples b = bx mod xB for a shared source, over the plane for
          x_plane) with |dy| for |x|, plus one rounding per addition of the chain: the number of (sample, output pixel) pairs
          whose weight on s is not 0; for x_plane ceil(Hout Wout / 256) * B / xB + 8 (tree) + 3 (the sum of four weights).
  attention   score = sum_c h src: S_score = sum_c |h| |src| (idf roundings of partial sums, each below that sum; the factor is
          left to TOL like conv_cases' S).  p = exp(score - m) / sum: the common shift m cancels; __expf is v_exp_f32 of the
          fp32-rounded product with log2(e) (bn_cases.sigmoid_parts): a perturbation of the argument by 2^-24 (2 + |arg|), the
          subtraction adds |arg|:   A_t = S_score_t + 2 + 2 |arg_t|,   S_p_t = p_t (A_t + sum_u p_u A_u + T + 2)
          (T additions of the sum, the reciprocal, the product).   S_wc = sum_t (|src| S_p + |src| p).
          backward, from the inputs src, attn (= p, an fp32 input), dwc, dattn:  dp = sum_c dwc src + dattn, S_dp = sum_c |dwc||src|
          + |dattn|;  dot = sum p dp, S_dot = sum_t p (S_dp + |dp|);  ds = p (dp - dot), S_ds = p (S_dp + S_dot + |dp| + |dot|) +
          |ds|;  dh = sum_t ds src, S_dh = sum_t |src| (S_ds + |ds|).  A masked word has p = 0: ds = 0 exactly.
          The scores stay within +-30 of each other (no probability below fp32's normal range, where a flush would be all the
          bound sees); every mask row keeps at least one word -- the all-masked row is NaN in the reference too and is not part
          of this table.
  softmax the same model; the argument is x * scale - m, which the compiler may or may not contract, so |x scale| + |m| count:
          A_l = |x scale| + |m| + 2 + |arg_l|, S_y = y (A_l + sum y A + n + 2).  dx = scale y (dy - dot): S_dot = sum |y dy|,
          S_dx = |scale| |y| (S_dot + |dy| + |dot|) + 2 |dx|.  Entries at l >= n are exact zeros in both directions (S = 0).
  concat  the forward moves values: bit for bit.  The backward is a sum in fp32: S = (additions of the longest chain) * sum |ddst|
          over what the element collects: N / rows - 1 additions for a non-broadcast source (none: a copy, S = 0, exact),
          (N / rows) * ceil(HW / 64) + 6 for a broadcast source.
"""
import functools
import math

import numpy as np
import torch

from helpers import det_array

EPS32 = 2.0 ** -24
TOL_CEILING = 1e-5            # conv_cases.TOL_CEILING
MARGIN = 16.0                 # the widening of the tents, in units of 2^-24 * S_ix (the coordinate is off by a few such units)
f32 = np.float32
LOG2E = f32(math.log2(math.e))

# Per-element tolerances: 4 x the largest err / S of the fp32 CPU evaluations over every row of the tables below
# (tests/test_pathway_reference_cpu.py measures them, asserts the factor 4 and the ceiling, and prints the figures).  Measured, in
# units of 2^-24 (restatement of the kernel's formula in numpy fp32, operand order kept / torch's own fp32 CPU evaluation):
#     stn_y 0.374 / 0.360   stn_dx 0.264 / 0.254   attn 1.021 / 1.001   wc 0.622 / 0.565   dscore 1.667   dh 1.063
#     sm_y 0.505 / 0.359   sm_dx 2.012 / 2.006   cat 0.761 / 0.761
# torch has no entry that takes attn as an input: dscore and dh are measured from the restatement alone (torch's softmax
# backward does take y: sm_dx has both).  Each kind takes the larger of its evaluations.
MEASURED = {"stn_y": 0.38 * EPS32, "stn_dx": 0.27 * EPS32, "attn": 1.03 * EPS32, "wc": 0.63 * EPS32, "dscore": 1.68 * EPS32,
            "dh": 1.07 * EPS32, "sm_y": 0.51 * EPS32, "sm_dx": 2.02 * EPS32, "cat": 0.77 * EPS32}
TOL = {k: 4 * v for k, v in MEASURED.items()}
# the whole-tensor rel-L2 figures tests/test_kernels_gpu.py holds, asserted beside the bounds
REL = {"stn_y": 1e-5, "stn_dx": 1e-5, "attn": 5e-6, "wc": 5e-6, "dscore": 2e-5, "dh": 2e-5, "sm_y": 2e-6, "sm_dx": 1e-5, "cat": 2e-6}


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def stn_rel_applies(Hin, Win, ac):
    """whether the whole-tensor rel-L2 figure REL["stn_*"] can be asked of a transformer call.  A source coordinate beyond 128 has
    an fp32 resolution of 2^-17 pixel, 7.6e-6 of a tap weight, and the det_array sources are white noise (neighbours differ by as
    much as they are).  Without align_corners the coordinates of the 257-pixel source axis lie between the pixels, and that
    resolution alone is the whole figure for ANY fp32 evaluation: torch's own fp32 grid_sample has 1.06e-5 (y) and 1.26e-5 (dx) on
    the (1, 257) row, the numpy restatement 1.18e-5 and 1.35e-5 (tests/test_pathway_reference_cpu.py asserts both: the exemption
    is needed, not convenient).  With align_corners several thetas of the table put the coordinates ON the pixels, the fp32
    evaluations have 3.9e-6 and 5.2e-6, and the figure is asked.  257 is prime, so "Hin * Win one past 256" has no other shape.
    The one exempted call is held to the per-element bound, which knows the coordinate's size through S_ix, and to the memory
    contract; every other call also to the figure."""
    return max(Hin, Win) <= 128 or bool(ac)


# ============================================================================================================ transformer
# boxes (x, y, w, h) in image fractions: the full image, 0.01- and 0.03-wide boxes, one hanging over the border, an absent object
BOXES = [(0.0, 0.0, 1.0, 1.0), (0.4, 0.3, 0.01, 0.2), (0.2, 0.6, 0.03, 0.03), (0.7, -0.1, 0.5, 0.45), (-1.0, -1.0, -1.0, -1.0)]
BOX_NAMES = ["full", "w0.01", "w0.03", "overhang", "absent"]


def bbox_to_theta_fp32(bbox):
    """numpy fp32 restatement of miscc/utils.py:16-49 in its operation order, one rounding per operation (no contraction):
    bbox (N, 4) fp32 -> theta, theta_inv (N, 6) fp32.  Division by 0 and inf - inf give what IEEE gives."""
    b = np.asarray(bbox, f32)
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    half, one, two, zero = f32(0.5), f32(1), f32(2), np.zeros_like(x)
    with np.errstate(all="ignore"):
        cx, cy = x + half * w, y + half * h
        th = np.stack([w, zero, two * (cx - half), zero, h, two * (cy - half)], 1)
        sx, sy = one / w, one / h
        thi = np.stack([sx, zero, (two * sx) * (half - cx), zero, sy, (two * sy) * (half - cy)], 1)
    assert th.dtype == f32 and thi.dtype == f32
    return th, thi


def bbox_table():
    """(N, 4) fp32 boxes for mogan_bbox_to_theta: the boxes above, boxes that divide by zero or carry inf / NaN / a denormal (the
    comparison is of bit patterns, non-finite ones included) and random ones up to one past a block of 256"""
    special = np.array([[0.1, 0.2, 0.0, 0.5], [0.1, 0.2, 0.5, -0.0], [np.inf, 0, 1, 1], [np.nan, 0, 1, 1], [0, 0, np.inf, 1],
                        [0.3, 0.3, 1e-30, 1e30], [0.5, 0.5, 1e-42, 3e38], [-1, -1, -1, -1]], f32)
    n = 257 - len(BOXES) - len(special)
    rnd = np.abs(det_array("bbox", (n, 4), 0.3, 0.1)) + f32(0.01)
    return np.concatenate([np.array(BOXES, f32), special, rnd]).astype(f32)


def _thetas():
    th, thi = bbox_to_theta_fp32(np.array(BOXES, f32))
    c, s = math.cos(0.6), math.sin(0.6)
    rows = [("identity", [1, 0, 0, 0, 1, 0])]
    rows += [("crop " + n, t) for n, t in zip(BOX_NAMES, th)] + [("place " + n, t) for n, t in zip(BOX_NAMES, thi)]
    rows += [("shear", [1.0, 0.4, 0.1, -0.3, 0.8, -0.05]), ("rotation", [c, -s, 0.05, s, c, -0.1]),
             ("reflection", [-0.9, 0.1, 0.05, 0.2, 0.8, 0.0]), ("minification", [3.0, 0, 0.2, 0, 3.0, -0.3]),
             ("singular zero", [0, 0, 0.3, 0, 0, -0.2]), ("singular rank one", [0.5, 0.25, 0.0, 1.0, 0.5, 0.1]),
             ("nearly singular", [1e-6, 0, 0.1, 0, 1e-6, -0.2])]
    return [n for n, _ in rows], np.array([t for _, t in rows], f32)


THETA_NAMES, THETAS = _thetas()          # 18 thetas: they ARE the batch of a transformer call (b -> THETAS[b % 18])
NT = len(THETA_NAMES)
THETA_KINDS = {"identity", "crop", "place", "shear", "rotation", "reflection", "minification", "singular", "nearly"}


def theta_kind(name):
    return name.split()[0]


def theta_det(th):
    th = np.asarray(th, np.float64)
    return th[0] * th[4] - th[1] * th[3]


# (B, C, Hin, Win, Hout, Wout); every row runs with align_corners 0 and 1
STN_SHAPES = [
    (NT, 13, 5, 7, 15, 17),        # Hout Wout = 255, both planes oblong, a ragged gather group (13 = 8 + 5); csplit == C
    (NT, 8, 8, 8, 16, 16),         # Hout Wout = 256; C exactly one gather group
    (NT, 1, 4, 3, 1, 257),         # an output axis of 1, Hout Wout = 257
    (NT, 3, 1, 257, 3, 5),         # a source axis of 1, Hin Win = 257
    (NT, 2, 6, 1, 5, 1),           # a source and an output axis of 1, the other way round
    (NT, 8, 17, 15, 4, 4),         # a large source on a small output
    (12, 50, 6, 5, 32, 32),        # the forward's ragged last channel chunk
    (256, 2, 4, 4, 32, 32),        # csplit == 1
]
STN_ROWS = [s + (ac,) for s in STN_SHAPES for ac in (0, 1)]
# (B, C, Hin, Win, Hout, Wout, xB, x_plane, theta_G); align_corners 0 and 1
STN_EX_SHAPES = [
    (NT, 5, 5, 7, 15, 17, 6, 0, 0),        # a shared source: three samples per image
    (NT, 5, 5, 7, 15, 17, NT, 0, 3),       # theta stored (image, object)
    (NT, 9, 4, 6, 9, 7, 6, 0, 3),          # both
    (NT, 13, 5, 7, 15, 17, 6, 1, 0),       # x_plane, Hout Wout < 256
    (NT, 4, 16, 16, 20, 20, NT, 1, 3),     # x_plane, Hout Wout > 256, theta_G
    (NT, 3, 3, 3, 16, 16, 2, 1, 0),        # x_plane, Hout Wout = 256, nine samples per image
]
STN_EX_ROWS = [s[:6] + (ac,) + s[6:] for s in STN_EX_SHAPES for ac in (0, 1)]


def stn_fwd_split(B, C, Hout, Wout):
    """(csplit, cchunk, channels of the last chunk) of the forward, from the words above"""
    pb = (Hout * Wout + 255) // 256
    csplit = min(max((1024 + pb * B - 1) // (pb * B), 1), C)
    cchunk = (C + csplit - 1) // csplit
    csplit = (C + cchunk - 1) // cchunk
    return csplit, cchunk, C - (csplit - 1) * cchunk


def stn_searches_everything(th, Hin, Win, ac):
    return (not abs(theta_det(th)) > 1e-30) or bool(ac and (Win < 2 or Hin < 2))


def theta_index(B, tG):
    """the theta row sample b uses: b, or with theta stored (B / tG, tG, 2, 3) and an object-major batch (b % nb) * tG + b // nb"""
    b = np.arange(B)
    if tG <= 0:
        return b
    nb = B // tG
    return (b % nb) * tG + b // nb


def stn_theta(B):
    return torch.from_numpy(THETAS[np.arange(B) % NT].copy())


def _axis(n_out, ac):
    """normalised coordinate of the output pixels of one axis and the sum of its absolute terms"""
    o = torch.arange(n_out, dtype=torch.float64)
    if ac:
        if n_out == 1:
            return torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        a = 2 * o / (n_out - 1)
    else:
        a = (2 * o + 1) / n_out
    return a - 1, a + 1 + (a - 1).abs()


def stn_coords(theta, Hin, Win, Hout, Wout, ac):
    """theta (B, 6) -> ix, iy, S_ix, S_iy (B, Hout * Wout) in fp64"""
    th = theta.double()
    xn, S_xn = _axis(Wout, ac)
    yn, S_yn = _axis(Hout, ac)
    XN, YN = xn.repeat(Hout)[None], yn.repeat_interleave(Wout)[None]
    SX, SY = S_xn.repeat(Hout)[None], S_yn.repeat_interleave(Wout)[None]
    out = []
    for k, n_in in ((0, Win), (3, Hin)):
        a, b, c = th[:, k:k + 1], th[:, k + 1:k + 2], th[:, k + 2:k + 3]
        g = a * XN + b * YN + c
        S_g = a.abs() * (SX + XN.abs()) + b.abs() * (SY + YN.abs()) + 2 * ((a * XN).abs() + (b * YN).abs()) + c.abs() + g.abs()
        if ac:
            i = (g + 1) * 0.5 * (n_in - 1)
            S_i = 0.5 * (n_in - 1) * (S_g + 2 * (g.abs() + 1)) + i.abs()
        else:
            i = ((g + 1) * n_in - 1) * 0.5
            S_i = 0.5 * (n_in * (S_g + 2 * (g.abs() + 1)) + ((g + 1) * n_in).abs() + 1) + i.abs()
        out.append((i, S_i))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _tents(i, S_i, n):
    """(B, P) coordinate -> tent weight, widened tent, widened support over the n source pixels of the axis: (B, P, n) each"""
    d = (i[:, :, None] - torch.arange(n, dtype=torch.float64)).abs()
    m = (MARGIN * EPS32 * S_i)[:, :, None]
    return (1 - d).clamp_min(0), (1 + m - d).clamp(0, 1), (d < 1 + m).double()


def stn_matrices(theta, Hin, Win, Hout, Wout, ac):
    """K_w (B, P, Hin, Win): the weight of source pixel s in output pixel o, and K_S, the first-order loss of it"""
    ix, iy, S_ix, S_iy = stn_coords(theta, Hin, Win, Hout, Wout, ac)
    wx, Tx, Ix = _tents(ix, S_ix, Win)
    wy, Ty, Iy = _tents(iy, S_iy, Hin)
    K_w = wy[:, :, :, None] * wx[:, :, None, :]
    K_S = 4 * K_w + S_ix[:, :, None, None] * (Ty[:, :, :, None] * Ix[:, :, None, :]) \
        + S_iy[:, :, None, None] * (Iy[:, :, :, None] * Tx[:, :, None, :])
    return K_w, K_S


def stn_reference(x, theta, dy, Hin, Win, Hout, Wout, ac, xB=None, plane=False, tG=0):
    """x (xB, C, Hin, Win), or (xB, C) with plane; theta (B, 6) as stored; dy (B, C, Hout * Wout) -> ref, S over y, dx (fp64)"""
    B = theta.shape[0]
    xB = B if xB is None else xB
    th = theta[torch.from_numpy(theta_index(B, tG))]
    K_w, K_S = stn_matrices(th, Hin, Win, Hout, Wout, ac)
    x = x.double()
    C = x.shape[1]
    xf = x[:, :, None, None].expand(xB, C, Hin, Win) if plane else x
    xs = xf[torch.arange(B) % xB]
    ref = {"y": torch.einsum("bphw,bchw->bcp", K_w, xs)}
    S = {"y": torch.einsum("bphw,bchw->bcp", K_S, xs.abs())}
    g = dy.double()
    per = lambda t: t.reshape(B // xB, xB, *t.shape[1:]).sum(0)          # over the samples b = j xB + bx
    dx = per(torch.einsum("bphw,bcp->bchw", K_w, g))
    S_a = per(torch.einsum("bphw,bcp->bchw", K_S, g.abs()))
    S_w = per(torch.einsum("bphw,bcp->bchw", K_w, g.abs()))
    if plane:
        chain = ((Hout * Wout + 255) // 256) * (B // xB) + 8 + 3
        ref["dx"], S["dx"] = dx.sum((2, 3)), S_a.sum((2, 3)) + chain * S_w.sum((2, 3))
    else:
        chain = per((K_w > 0).double().sum(1))[:, None]                   # (xB, 1, Hin, Win)
        ref["dx"], S["dx"] = dx, S_a + chain * S_w
    return ref, S


@functools.lru_cache(maxsize=None)
def stn_case(B, C, Hin, Win, Hout, Wout, ac, xB=None, plane=0, tG=0):
    """inputs, references and S of one transformer call, computed once and shared (read-only)"""
    xb = B if xB is None else xB
    tag = "%s" % ((B, C, Hin, Win, Hout, Wout, xb, plane),)
    x = T("stnx" + tag, (xb, C) if plane else (xb, C, Hin, Win))
    dy = T("stng" + tag, (B, C, Hout * Wout))
    theta = stn_theta(B)
    ref, S = stn_reference(x, theta, dy, Hin, Win, Hout, Wout, ac, xb, bool(plane), tG)
    return dict(x=x, theta=theta, dy=dy, ref=ref, S=S)


# ------------------------------------------------------------------ the fp32 restatement of stn_taps and the kernels (numpy)
def restate_taps(th, Hin, Win, Hout, Wout, ac):
    """stn_taps for every (b, output pixel): dict of (B, P) arrays x0, y0 (int), wx1, wy1 (fp32), vx0, vx1, vy0, vy1 (bool)"""
    one, two, half = f32(1), f32(2), f32(0.5)
    ox = np.tile(np.arange(Wout), Hout).astype(f32)[None]
    oy = np.repeat(np.arange(Hout), Wout).astype(f32)[None]
    if ac:
        xn = two * ox / f32(Wout - 1) - one if Wout > 1 else np.zeros_like(ox)
        yn = two * oy / f32(Hout - 1) - one if Hout > 1 else np.zeros_like(oy)
    else:
        xn = (two * ox + one) / f32(Wout) - one
        yn = (two * oy + one) / f32(Hout) - one
    t = [th[:, k:k + 1].astype(f32) for k in range(6)]
    gx = t[0] * xn + t[1] * yn + t[2]
    gy = t[3] * xn + t[4] * yn + t[5]
    if ac:
        ix, iy = (gx + one) * half * f32(Win - 1), (gy + one) * half * f32(Hin - 1)
    else:
        ix, iy = ((gx + one) * f32(Win) - one) * half, ((gy + one) * f32(Hin) - one) * half
    assert ix.dtype == f32 and iy.dtype == f32
    out = {}
    for n, i, N in (("x", ix, Win), ("y", iy, Hin)):
        fl = np.floor(i)
        i0 = np.minimum(np.maximum(fl, f32(-2)), f32(N) + one).astype(np.int64)
        inr = (fl >= -1) & (fl <= N)
        out[n + "0"], out["w" + n + "1"] = i0, i - fl
        out["v" + n + "0"], out["v" + n + "1"] = inr & (i0 >= 0) & (i0 < N), inr & (i0 + 1 >= 0) & (i0 + 1 < N)
    return out


def _tap_list(tp, Hin, Win):
    """the four taps in the kernels' order: (flat source index (clipped where invalid), valid, weight) each (B, P)"""
    one = f32(1)
    wx1, wy1 = tp["wx1"], tp["wy1"]
    w = [(one - wx1) * (one - wy1), wx1 * (one - wy1), (one - wx1) * wy1, wx1 * wy1]
    v = [tp["vx0"] & tp["vy0"], tp["vx1"] & tp["vy0"], tp["vx0"] & tp["vy1"], tp["vx1"] & tp["vy1"]]
    taps = []
    for k in range(4):
        sx, sy = tp["x0"] + (k & 1), tp["y0"] + (k >> 1)
        taps.append((np.clip(sy, 0, Hin - 1) * Win + np.clip(sx, 0, Win - 1), v[k], w[k]))
    return taps


def restate_stn_fp32(x, theta, dy, Hin, Win, Hout, Wout, ac, xB=None, plane=False, tG=0):
    """the forward and backward kernels in numpy fp32, operand and summation order kept, one rounding per operation: numpy fp32
    arrays as in stn_reference -> dict over y (B, C, P), dx"""
    B, C, P = theta.shape[0], x.shape[1], Hout * Wout
    xB = B if xB is None else xB
    taps = _tap_list(restate_taps(theta[theta_index(B, tG)], Hin, Win, Hout, Wout, ac), Hin, Win)
    bx = np.arange(B) % xB
    y = np.zeros((B, C, P), f32)
    xf = x.reshape(xB, C, -1)
    for idx, v, w in taps:
        val = np.broadcast_to(xf[bx], (B, C, P)) if plane else np.take_along_axis(xf[bx], np.broadcast_to(idx[:, None], (B, C, P)), 2)
        y = np.where(v[:, None], y + val * w[:, None], y)
    if plane:
        zero = f32(0)
        ws = [np.where(v, w, zero) for _, v, w in taps]
        wsum = ((ws[0] + ws[1]) + ws[2]) + ws[3]
        acc = np.zeros((xB, C, 256), f32)
        for b in range(B):
            for p0 in range(0, P, 256):
                n = min(256, P - p0)
                acc[b % xB, :, :n] += dy[b, :, p0:p0 + n] * wsum[b, None, p0:p0 + n]
        s = 128
        while s > 0:
            acc[:, :, :s] += acc[:, :, s:2 * s]
            s >>= 1
        dx = acc[:, :, 0].copy()
    else:
        # per source pixel: samples in batch order, output pixels row-major -- np.add.at adds in index order
        HW = Hin * Win
        idx = np.stack([t[0] for t in taps], 2) + (bx * HW)[:, None, None]          # (B, P, 4)
        val = np.stack([np.where(t[1], t[2], f32(0)) for t in taps], 2)            # (B, P, 4)
        vals = dy.transpose(0, 2, 1)[:, :, None, :] * val[:, :, :, None]           # (B, P, 4, C)
        keep = (val != 0).reshape(-1)
        dxf = np.zeros((xB * HW, C), f32)
        np.add.at(dxf, idx.reshape(-1)[keep], vals.reshape(-1, C)[keep])
        dx = dxf.reshape(xB, HW, C).transpose(0, 2, 1).reshape(xB, C, Hin, Win)
    assert y.dtype == f32 and dx.dtype == f32
    return {"y": y, "dx": dx}


# ================================================================================================================ attention
ATTN_ROWS = [(3, 6, 16, 5), (2, 13, 257, 8), (2, 8, 1, 9), (4, 48, 256, 16), (1, 20, 300, 17), (2, 128, 70, 32), (5, 24, 7, 12)]
MASKS = (None, 0, 1)          # no mask, mask_mode 0, mask_mode 1
SPREAD = 30.0


def attn_slots(T_):
    return 8 if T_ <= 8 else 16 if T_ <= 16 else 32


def attn_mask(B, T_):
    """uint8 (B, T): the tail from max(1, T - 1 - b) on and one word in the middle; word 0 always stays"""
    m = torch.zeros(B, T_, dtype=torch.uint8)
    for b in range(B):
        m[b, max(1, T_ - 1 - b):] = 1
        if (b + 1) % T_:
            m[b, (b + 1) % T_] = 1
    assert int(m[:, 0].sum()) == 0
    return m


def attn_mask_rows(B, Q, mode):
    """the mask row of (b, q): mode 0 the reference's (b Q + q) % B, mode 1 b"""
    r = torch.arange(B * Q).reshape(B, Q)
    return r % B if mode == 0 else r // Q


def attn_reference(h, src, mask, mode, dwc, dattn, attn_in=None):
    """h (B, idf, Q), src (B, idf, T), mask (B, T) uint8 or None -> ref, S over attn (B, T, Q), wc (B, idf, Q), and, from
    attn_in (the fp32 attn the backward receives; default: the reference's, rounded) dscore (B, T, Q), dh (B, idf, Q);
    dattn None: no term"""
    h, src = h.double(), src.double()
    B, idf, Q = h.shape
    T_ = src.shape[2]
    sc = torch.einsum("bcq,bct->btq", h, src)
    S_sc = torch.einsum("bcq,bct->btq", h.abs(), src.abs())
    off = torch.zeros(B, T_, Q, dtype=torch.bool)
    if mask is not None:
        off = mask.bool()[attn_mask_rows(B, Q, mode)].permute(0, 2, 1)            # (B, Q, T) -> (B, T, Q)
    sc = sc.masked_fill(off, -float("inf"))
    arg = sc - sc.max(1, keepdim=True).values
    p = torch.softmax(sc, 1)
    A = torch.where(off, torch.zeros_like(p), S_sc + 2 + 2 * arg.abs().masked_fill(off, 0.0))
    S_p = p * (A + (p * A).sum(1, keepdim=True) + T_ + 2)
    ref = {"attn": p, "wc": torch.einsum("bct,btq->bcq", src, p)}
    S = {"attn": S_p, "wc": torch.einsum("bct,btq->bcq", src.abs(), S_p + p)}
    pin = (p.float() if attn_in is None else attn_in).double()
    dwc = dwc.double()
    dp = torch.einsum("bcq,bct->btq", dwc, src)
    S_dp = torch.einsum("bcq,bct->btq", dwc.abs(), src.abs())
    if dattn is not None:
        dp, S_dp = dp + dattn.double(), S_dp + dattn.double().abs()
    dot = (pin * dp).sum(1, keepdim=True)
    S_dot = (pin * (S_dp + dp.abs())).sum(1, keepdim=True)
    ds = pin * (dp - dot)
    S_ds = pin * (S_dp + S_dot + dp.abs() + dot.abs()) + ds.abs()
    ref["dscore"], S["dscore"] = ds, S_ds
    ref["dh"], S["dh"] = torch.einsum("btq,bct->bcq", ds, src), torch.einsum("btq,bct->bcq", S_ds + ds.abs(), src.abs())
    ref["spread"] = float(arg.masked_fill(off, 0.0).abs().max())
    return ref, S


@functools.lru_cache(maxsize=None)
def attn_case(B, idf, Q, T_, mask_kind, with_dattn):
    tag = "%s" % ((B, idf, Q, T_),)
    h, src = T("ath" + tag, (B, idf, Q)), T("ats" + tag, (B, idf, T_), 0.3)
    mask = None if mask_kind is None else attn_mask(B, T_)
    dwc, dattn = T("atgw" + tag, (B, idf, Q)), T("atga" + tag, (B, T_, Q)) if with_dattn else None
    ref, S = attn_reference(h, src, mask, mask_kind, dwc, dattn)
    return dict(h=h, src=src, mask=mask, mode=mask_kind or 0, dwc=dwc, dattn=dattn, attn_in=ref["attn"].float(), ref=ref, S=S)


def _exp32(arg):
    """__expf: a correctly rounded exp2 of the fp32-rounded product with log2(e)"""
    with np.errstate(all="ignore"):
        return np.exp2((arg * LOG2E).astype(np.float64)).astype(f32)


def restate_attn_fp32(h, src, mask, mode, dwc, dattn, attn_in):
    """attn_fwd_kernel / attn_bwd_kernel in numpy fp32: the channel and word sums in the kernels' order, one rounding per
    multiply and per add (the kernels' fmaf rounds once: an equally valid evaluation)"""
    B, idf, Q = h.shape
    T_ = src.shape[2]
    s = np.zeros((B, T_, Q), f32)
    for c in range(idf):
        s = h[:, c, None, :] * src[:, c, :, None] + s
    if mask is not None:
        off = mask.astype(bool)[attn_mask_rows(B, Q, mode).numpy()].transpose(0, 2, 1)
        s = np.where(off, f32(-np.inf), s)
    m = s.max(1, keepdims=True)
    e = _exp32(s - m)
    tot = np.zeros((B, 1, Q), f32)
    for t in range(T_):
        tot = tot + e[:, t:t + 1]
    p = e * (f32(1) / tot)
    wc = np.zeros((B, idf, Q), f32)
    for t in range(T_):
        wc = src[:, :, t, None] * p[:, t, None, :] + wc
    pin = attn_in
    dp = np.zeros((B, T_, Q), f32) if dattn is None else dattn.copy()
    for c in range(idf):
        dp = dwc[:, c, None, :] * src[:, c, :, None] + dp
    dot = np.zeros((B, 1, Q), f32)
    for t in range(T_):
        dot = pin[:, t:t + 1] * dp[:, t:t + 1] + dot
    ds = pin * (dp - dot)
    dh = np.zeros((B, idf, Q), f32)
    for t in range(T_):
        dh = ds[:, t, None, :] * src[:, :, t, None] + dh
    out = {"attn": p, "wc": wc, "dscore": ds, "dh": dh}
    assert all(v.dtype == f32 for v in out.values())
    return out


# ================================================================================================================== softmax
SOFTMAX_ROWS = [(21, 5, 4), (1, 1, 1), (2, 33, 300), (300, 7, 1)]
SCALES = (1.0, 4.0, -2.5)
LENS = (False, True)


def softmax_lens(outer, L, inner):
    """int32 (outer * inner): 0, 1, L, L + 3, -2 in turn (a single column: L + 3)"""
    pat = np.array([0, 1, L, L + 3, -2], np.int32)
    n = outer * inner
    return torch.from_numpy(pat[(np.arange(n) + (3 if n == 1 else 0)) % 5].copy())


def lens_clamps(lens, L):
    l = lens.numpy()
    return {"zero": bool((l == 0).any()), "above": bool((l > L).any()), "negative": bool((l < 0).any())}


def softmax_reference(x, lens, scale, dy, y_in=None):
    """x (outer, L, inner), lens (outer * inner) int32 or None -> ref, S over y and, from y_in (the fp32 y the backward receives;
    default the reference's, rounded), dx"""
    x = x.double()
    outer, L, inner = x.shape
    n = torch.full((outer, 1, inner), L, dtype=torch.int64) if lens is None else lens.long().clamp(0, L).reshape(outer, 1, inner)
    off = torch.arange(L).reshape(1, L, 1) >= n
    xs = (x * scale).masked_fill(off, -float("inf"))
    m = xs.max(1, keepdim=True).values
    m = torch.where(n > 0, m, torch.zeros_like(m))
    arg = (xs - m).masked_fill(off, 0.0)
    y = torch.where(off, torch.zeros_like(x), torch.exp(arg))
    y = y / y.sum(1, keepdim=True).clamp_min(1e-300)
    A = torch.where(off, torch.zeros_like(x), (x * scale).abs() + m.abs() + 2 + arg.abs())
    ref = {"y": y}
    S = {"y": y * (A + (y * A).sum(1, keepdim=True) + n + 2)}
    yin = (y.float() if y_in is None else y_in).double()
    yin = torch.where(off, torch.zeros_like(yin), yin)
    g = dy.double()
    dot = (yin * g).sum(1, keepdim=True)
    S_dot = (yin * g).abs().sum(1, keepdim=True)
    ref["dx"] = scale * yin * (g - dot)
    S["dx"] = abs(scale) * yin.abs() * (S_dot + g.abs() + dot.abs()) + 2 * ref["dx"].abs()
    return ref, S


@functools.lru_cache(maxsize=None)
def softmax_case(outer, L, inner, with_lens, scale):
    tag = "%s" % ((outer, L, inner),)
    x, dy = T("smx" + tag, (outer, L, inner)), T("smg" + tag, (outer, L, inner))
    lens = softmax_lens(outer, L, inner) if with_lens else None
    ref, S = softmax_reference(x, lens, scale, dy)
    return dict(x=x, dy=dy, lens=lens, scale=scale, y_in=ref["y"].float(), ref=ref, S=S)


def restate_softmax_fp32(x, lens, scale, dy, y_in):
    """softmax_kernel in numpy fp32, the sums over l in order, x * scale rounded before the subtraction (no contraction)"""
    outer, L, inner = x.shape
    sc = f32(scale)
    n = np.full((outer, inner), L) if lens is None else np.clip(lens.astype(np.int64), 0, L).reshape(outer, inner)
    y, dx = np.zeros_like(x), np.zeros_like(x)
    live = lambda l: (l < n)
    m = np.full((outer, inner), -np.inf, f32)
    for l in range(L):
        m = np.where(live(l), np.maximum(m, x[:, l] * sc), m)
    s, dot = np.zeros((outer, inner), f32), np.zeros((outer, inner), f32)
    for l in range(L):
        s = np.where(live(l), s + _exp32(x[:, l] * sc - m), s)
        dot = np.where(live(l), dot + y_in[:, l] * dy[:, l], dot)
    with np.errstate(all="ignore"):
        inv = f32(1) / s
        for l in range(L):
            y[:, l] = np.where(live(l), _exp32(x[:, l] * sc - m) * inv, f32(0))
            dx[:, l] = np.where(live(l), sc * y_in[:, l] * (dy[:, l] - dot), f32(0))
    assert y.dtype == f32 and dx.dtype == f32
    return {"y": y, "dx": dx}


# =================================================================================================================== concat
CAT_B, CAT_G = 2, 3
CAT_N = CAT_B * CAT_G
# source kinds -> (rows, storage shape, sb, sg, bcast) for C channels on a plane of HW
CAT_KINDS = ("full", "plane", "rep", "rep_plane", "obj", "obj_plane")


def cat_layout(kind, C, HW):
    B, G, N = CAT_B, CAT_G, CAT_N
    return {"full": (N, (N, C, HW), C * HW, 0, 0), "plane": (N, (N, C), C, 0, 1), "rep": (B, (B, C, HW), C * HW, 0, 0),
            "rep_plane": (B, (B, C), C, 0, 1), "obj": (B, (B, G, C, HW), G * C * HW, C * HW, 0),
            "obj_plane": (B, (B, G, C), G * C, C, 1)}[kind]


BASE4 = (("full", 6), ("plane", 5), ("rep", 3), ("obj_plane", 7))
# (name, HW, sources (kind, C), which gradients are wanted)
CAT_CASES = [("base hw%d" % hw, hw, BASE4, (1, 1, 1, 1)) for hw in (1, 15, 16, 256)] + [
    ("reversed", 16, BASE4[::-1], (1, 1, 1, 1)),
    ("broadcast first", 15, (("plane", 4), ("full", 2), ("obj", 3)), (1, 1, 1)),
    ("broadcast in the middle", 16, (("full", 2), ("obj_plane", 4), ("rep", 5), ("full", 1)), (1, 1, 1, 1)),
    ("all broadcast", 16, (("plane", 4), ("obj_plane", 3), ("rep_plane", 2)), (1, 1, 1)),
    ("all plain", 16, (("rep", 2), ("full", 3), ("obj", 4)), (1, 1, 1)),
    ("one plain", 15, (("full", 3),), (1,)),
    ("one broadcast", 256, (("rep_plane", 3),), (1,)),
    ("two", 1, (("obj", 2), ("rep_plane", 3)), (1, 1)),
] + [("base without gradient %d" % i, 16, BASE4, tuple(int(j != i) for j in range(4))) for i in range(4)] + [
    ("base with one gradient", 15, BASE4, (0, 0, 1, 0)),
    ("no gradient at all", 16, BASE4, (0, 0, 0, 0)),
]


def cat_vector(HW, sources, misaligned=False):
    """whether the forward takes four values per thread (aligned test buffers; misaligned: a non-broadcast pointer off by 4 bytes)"""
    if HW % 4 or misaligned:
        return False
    return all(b or (sb % 4 == 0 and sg % 4 == 0) for _, _, sb, sg, b in (cat_layout(k, C, HW) for k, C in sources))


def cat_gather(kind, C, HW):
    """flat storage index of value(n, c, hw), (N, C, HW), by the header's addressing formula"""
    rows, shape, sb, sg, bc = cat_layout(kind, C, HW)
    n, c, hw = np.meshgrid(np.arange(CAT_N), np.arange(C), np.arange(HW), indexing="ij")
    return (n % rows) * sb + (n // rows) * sg + c * (1 if bc else HW) + (0 if bc else hw)


@functools.lru_cache(maxsize=None)
def cat_case(name):
    """sources (fp32 storage tensors), dst (exact), ddst, and per source the fp64 gradient with its S"""
    _, HW, sources, want = next(c for c in CAT_CASES if c[0] == name)
    srcs = [T("cat%s%d%s%d%d" % (name, i, k, C, HW), cat_layout(k, C, HW)[1]) for i, (k, C) in enumerate(sources)]
    idx = [cat_gather(k, C, HW) for k, C in sources]
    dst = torch.cat([s.reshape(-1)[torch.from_numpy(i)] for s, i in zip(srcs, idx)], 1)
    ddst = T("catg" + name, tuple(dst.shape))
    grads, Ss, c0 = [], [], 0
    for s, i, (k, C) in zip(srcs, idx, sources):
        rows, shape, sb, sg, bc = cat_layout(k, C, HW)
        g = ddst[:, c0:c0 + C].double().reshape(-1)
        fi = torch.from_numpy(i.reshape(-1))
        d = torch.zeros(s.numel(), dtype=torch.float64).index_add_(0, fi, g)
        a = torch.zeros(s.numel(), dtype=torch.float64).index_add_(0, fi, g.abs())
        reps = CAT_N // rows if sg == 0 else 1
        chain = reps * ((HW + 63) // 64) + 6 if bc else reps - 1
        grads.append(d.reshape(shape)); Ss.append((chain * a).reshape(shape))
        c0 += C
    return dict(HW=HW, sources=sources, want=want, srcs=srcs, dst=dst, ddst=ddst, grads=grads, S=Ss)


def restate_cat_bwd_fp32(ddst, kind, C, HW, c0):
    """concat_bwd_kernel for one source in numpy fp32, additions in the kernel's order -> the source's storage layout"""
    rows, shape, sb, sg, bc = cat_layout(kind, C, HW)
    g = ddst[:, c0:c0 + C]                                   # (N, C, HW)
    N = CAT_N
    if sg == 0:
        groups = [[n for n in range(r, N, rows)] for r in range(rows)]
    else:                                                    # storage row b G + g reads n = g rows + b
        groups = [[gi * rows + b] for b in range(rows) for gi in range(N // rows)]
    out = []
    for ns in groups:
        if not bc:
            t = np.zeros((C, HW), f32)
            for n in ns:
                t = t + g[n]
            out.append(t)
        else:
            lanes = np.zeros((C, 64), f32)
            for n in ns:
                for h0 in range(0, HW, 64):
                    k = min(64, HW - h0)
                    lanes[:, :k] = lanes[:, :k] + g[n][:, h0:h0 + k]
            o = 32
            while o > 0:
                lanes = lanes + lanes[:, np.arange(64) ^ o]
                o >>= 1
            out.append(lanes[:, 0])
    r = np.stack(out).reshape(shape)
    assert r.dtype == f32
    return r
