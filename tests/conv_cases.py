"""Geometries, inputs and CPU references of the GAN-path convolution family (a plain helper module, not a conftest):
the case tables that tests/test_kernels_gpu.py (through hip/ops.py, rel-L2) and tests/test_conv_entry_points_gpu.py (the C ABI
under tests/memguard.py, rel-L2 and a per-element bound) both run, the forced dispatches, the deterministic inputs, the fp64
references with the matching sums over absolute terms, a plain fp32 emulation of Winograd F(2x2,3x3) from the textbook matrices,
and the per-element tolerances.  Nothing here needs a GPU or the library; tests/test_conv_reference_cpu.py keeps the references
themselves within a quarter of the tolerances and records the figures they were derived from."""
import functools

import torch
import torch.nn.functional as F

from helpers import det_array

CONV_CASES = [
    # B, Cin, H, W, Cout, k (kh,kw), stride, pad (ph,pw), up
    (2, 8, 8, 8, 16, (3, 3), 1, (1, 1), 0),
    (2, 8, 8, 8, 16, (3, 3), 1, (1, 1), 1),        # upBlock: fused nearest x2
    (3, 5, 9, 7, 7, (3, 3), 1, (1, 1), 1),         # ragged everything
    (2, 6, 16, 16, 12, (4, 4), 2, (1, 1), 0),      # D down conv
    (2, 84, 16, 16, 24, (4, 4), 1, (1, 1), 0),     # D_NET64 local conv -> 15x15
    (3, 100, 16, 16, 50, (3, 3), 2, (1, 1), 0),    # BBOX_NET (3x3 s2)
    (2, 12, 4, 4, 1, (4, 4), 4, (0, 0), 0),        # logits conv 4x4 s4 (full-map dot kernels)
    (5, 70, 4, 4, 3, (4, 4), 4, (0, 0), 0),        # the same with 3 outputs, K = 1120 (not a multiple of 256)
    (4, 20, 5, 1, 6, (1, 1), 1, (0, 0), 0),        # conv_context (1x1 on (B,cdf,T,1))
    (2, 3, 32, 32, 96, (4, 4), 2, (1, 1), 0),      # first D conv (Cin=3)
    (2, 48, 16, 16, 3, (3, 3), 1, (1, 1), 0),      # img head (Cout=3)
    (3, 13, 37, 70, 3, (3, 3), 1, (1, 1), 0),      # img head, ragged sizes (direct small-channel kernels)
    (2, 20, 13, 128, 3, (3, 3), 1, (1, 1), 0),     # img head on 128-pixel rows: four pixels per thread (sc_fwd3x3_w4), ragged height / channels
    (1, 8, 16, 256, 4, (3, 3), 1, (1, 1), 0),      # the same with two tiles per row, four output channels, one channel chunk
    (2, 17, 9, 128, 1, (3, 3), 1, (1, 1), 0),      # one output channel, 17 input channels (a chunk of one)
    (2, 20, 64, 64, 1, (3, 3), 1, (1, 1), 0),      # multi-mnist img head (Cout=1)
    (2, 3, 64, 96, 40, (4, 4), 2, (1, 1), 0),      # first D conv, non-square (dgrad = 2x2-block kernel)
    (2, 1, 32, 32, 24, (4, 4), 2, (1, 1), 0),      # multi-mnist first D conv (Cin=1)
    (2, 3, 37, 45, 20, (3, 3), 2, (0, 0), 0),      # Inception Conv2d_1a (3 -> 32, 3x3 s2 valid, odd sizes): streaming dgrad
    (2, 10, 17, 17, 12, (1, 7), 1, (0, 3), 0),     # Inception 1x7
    (2, 10, 17, 17, 12, (7, 1), 1, (3, 0), 0),     # Inception 7x1
    (2, 6, 35, 35, 8, (3, 3), 2, (0, 0), 0),       # Inception 3x3 s2 valid (odd size)
    (2, 6, 12, 12, 8, (5, 5), 1, (2, 2), 0),       # Inception 5x5
    (1, 96, 32, 32, 96, (3, 3), 1, (1, 1), 0),     # 96-wide tile config
    (2, 160, 8, 8, 130, (3, 3), 1, (1, 1), 0),     # 128x128 tiles with ragged edges + long K
    # fused Winograd F(2x2,3x3) (3x3 s1 p1, Cin % 16 == 0, >= 64 output channels, H % 4 == 0, W % 32 == 0): fwd and dgrad
    (2, 32, 8, 32, 64, (3, 3), 1, (1, 1), 0),      # one tile column, two chunks
    (3, 48, 12, 64, 100, (3, 3), 1, (1, 1), 0),    # ragged M (100 = 96 + 4), odd chunk pairs, image borders everywhere
    (1, 96, 32, 32, 192, (3, 3), 1, (1, 1), 0),    # ResBlock widths
    (2, 64, 16, 96, 64, (3, 3), 1, (1, 1), 0),     # dgrad also Winograd (Cout % 16 == 0, Cin >= 64)
    (2, 32, 30, 61, 64, (3, 3), 1, (1, 1), 0),     # ragged grid (odd width: scalar stores), pad 1
    (2, 80, 29, 63, 96, (3, 3), 1, (0, 0), 0),     # valid convolution (Inception 4a): forward pad 0, data gradient pad 2
    # fused Winograd F(2x2,2x2) for 4x4 s2 p1 (Cin % 8 == 0, >= 64 in / 96 out channels, H, W % 4 == 0): forward
    (4, 72, 8, 8, 130, (4, 4), 2, (1, 1), 0),      # 4x4 outputs: a block spans 8 images; ragged M (130 = 128 + 2)
    (2, 64, 16, 24, 100, (4, 4), 2, (1, 1), 0),    # non-square, partly filled tile block, M < 128
    (1, 128, 64, 64, 128, (4, 4), 2, (1, 1), 0),   # several tile blocks of one image
    (16, 256, 8, 8, 192, (4, 4), 2, (1, 1), 0),    # few tiles, long K: the K range is split (partial slabs + reduce)
    (3, 104, 12, 20, 64, (4, 4), 2, (1, 1), 0),    # data gradient through it (Cout % 32 == 0, Cin >= 96): ragged M = 104, non-square
    # shapes that take the direct (halo-tile) kernel when no tile config is forced (>= 64 channels each side)
    (2, 64, 32, 32, 72, (3, 3), 1, (1, 1), 0),     # 3x3 s1, Cw=32, ragged M (forward: Winograd; dgrad: direct, 72 % 16 != 0)
    (2, 72, 32, 32, 64, (3, 3), 1, (1, 1), 0),     # Cin % 16 != 0: forward stays on the direct kernel (Cw=32, 16-byte halo loads)
    (2, 64, 16, 16, 64, (3, 3), 1, (1, 1), 1),     # upBlock: 16x16 -> 32x32
    (3, 64, 16, 16, 100, (3, 3), 1, (1, 1), 0),    # Cw=16, R=8; 96-wide M tile + ragged M
    (1, 64, 64, 128, 64, (3, 3), 1, (1, 1), 0),    # non-square
    (2, 256, 16, 16, 64, (3, 3), 1, (1, 1), 0),    # split over channel chunks
    (2, 64, 64, 64, 72, (4, 4), 2, (1, 1), 0),     # 4x4 s2 -> 32x32; dgrad = four 2x2 parity convs in one launch
    (2, 64, 32, 32, 256, (4, 4), 2, (1, 1), 0),    # 4x4 s2 -> 16x16; parity dgrad with channel split
    # round 5: the pre-split direct kernel (csrc/mogan_dconv2.hip; 3x3 s1 and the 2x2 parity classes of a 4x4 s2 data gradient on
    # grids of 8 x 32 tiles, channels % 16 == 0); 3x3 reaches it where Winograd declines or with force (-2, 0)
    (2, 96, 32, 64, 160, (3, 3), 1, (1, 1), 0),    # 96-row channel blocks, ragged M = 160 (guarded stores), dgrad: 160 -> 96
    (1, 32, 8, 32, 64, (3, 3), 1, (1, 1), 0),      # one tile, 64-row block; dgrad declined (32 output channels)
    (1, 16, 8, 32, 128, (3, 3), 1, (1, 1), 0),     # 128-row block, one 16-channel stage
    (1, 256, 8, 32, 64, (3, 3), 1, (1, 1), 0),     # one tile, 16 stages: K split over the stages + reduce
    (3, 48, 16, 32, 80, (3, 3), 1, (1, 1), 0),     # several tiles per persistent block across images
    (2, 96, 32, 64, 64, (4, 4), 2, (1, 1), 0),     # data gradient: four 2x2 parity classes, two 16-channel sub-chunks per stage
    (2, 128, 16, 64, 16, (4, 4), 2, (1, 1), 0),    # data gradient with 16 input channels of dY (one stage), 128-row blocks
    # 16 x 16 spatial tiles (maps with 16-pixel rows) and the 4x4 s2 FORWARD as a 2x2 filter over the space-to-depth image
    (2, 96, 64, 128, 192, (4, 4), 2, (1, 1), 0),   # forward: 8 x 32 tiles, 96-row blocks, 12 stages of 8 channels
    (2, 192, 32, 32, 96, (4, 4), 2, (1, 1), 0),    # forward and data gradient on 16 x 16 tiles, K split
    (3, 24, 32, 64, 100, (4, 4), 2, (1, 1), 0),    # forward: ragged M = 100, 24 channels (3 stages)
    (1, 8, 64, 32, 64, (4, 4), 2, (1, 1), 0),      # forward: one stage, two tiles of 16 x 16
    (2, 64, 16, 16, 128, (3, 3), 1, (1, 1), 0),    # 3x3 on one 16 x 16 tile per image
    # 32-pixel output rows from 3 input channels: the streaming first-layer kernel (csrc/mogan_stem.hip) inside the dispatch
    (2, 3, 16, 64, 40, (4, 4), 2, (1, 1), 0),
]


UP_CASES = [(2, 8, 8, 8, 16), (3, 5, 9, 7, 7), (2, 64, 16, 16, 64), (2, 96, 32, 32, 96), (1, 72, 64, 64, 100),
            (2, 128, 4, 4, 192)]


PK_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad      (forward needs Cin % 32 == 0, the data gradient Cout % 32 == 0)
    (4, 64, 8, 8, 96, 4, 2, 1),        # down-convolution 8x8 -> 4x4, four parity classes in the data gradient
    (3, 96, 16, 16, 160, 4, 2, 1),     # ragged: N = 3*64 = 192 columns, 160 rows (the last m-tile half empty)
    (16, 128, 4, 4, 64, 3, 1, 1),      # 3x3 s1 on a 4x4 map (jointConv / the last D_NET256 layers), one class
    (5, 32, 6, 10, 32, 4, 2, 1),       # non-square map, one K-tile per tap, N = 5*15 = 75
    (2, 64, 8, 8, 64, 1, 1, 0),        # 1x1
    (15, 64, 4, 4, 32, 3, 1, 1),       # the "wrong pair" batch (B - 1 images): N = 240
]


PK_WGRAD_CASES = PK_CASES + [
    (4, 20, 9, 7, 50, 3, 2, 1),        # nothing aligned: Cin, Cout, the map and K = 4*5*4 = 80 output pixels (padded to 96)
    (33, 16, 4, 4, 40, 4, 1, 0),       # 1x1 outputs: K = 33
]


# mogan_gemm_debug_force(cfg, split) of test_conv2d_fwd_dgrad_wgrad: (-1, 0) the default dispatch (small-channel / stem / Winograd /
# direct / implicit GEMM by shape), (-2, 0) the same without the Winograd kernels, the others an implicit-GEMM tile configuration
# and a split-K factor
FORCES = [(-1, 0), (-2, 0), (0, 3), (1, 1), (2, 2), (3, 1), (4, 5), (5, 2), (6, 3)]
# mogan_pk_debug_force(1, cfg, split) of test_packed_weight_convolution / test_packed_weight_gradient
PK_FORCES = [(-1, 0), (0, 1), (1, 3), (2, 2), (0, 5)]
PK_WGRAD_FORCES = [(-1, 0), (0, 2), (1, 1), (2, 3)]

EPS32 = 2.0 ** -24            # half an ulp of fp32: one rounding
REL_L2 = 2e-6                 # the project's whole-tensor figure (test_kernels_gpu._check)
TOL_CEILING = 1e-5            # what the project accepts per element for the trunk (test_trunk_entry_points_gpu.CONV_TOL)
# Per-element tolerances |got - fp64| <= TOL * S, S = the same sum over the absolute values of both operands: 4 x the largest
# err / S of the CPU reference named (torch's fp32 convolutions; the fp32 Winograd emulation below) over every case of the
# tables -- the figures and the cases they come from are in the docstring of tests/test_conv_reference_cpu.py, which also asserts
# that each reference stays within a quarter of its constant.
TOL = {"fwd": 1.1e-6, "dgrad": 1.3e-6, "wgrad": 1.9e-6}
TOL_WINO = {"fwd": 6.7e-7, "dgrad": 1.2e-6, "wgrad": 1.0e-6}


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def conv_inputs(case):
    """(x, w, g) of a CONV_CASES row, the tensors test_conv2d_fwd_dgrad_wgrad uses"""
    B, Cin, H, W, Cout, k, s, pad, up = case
    OH, OW = ((H << up) + 2 * pad[0] - k[0]) // s + 1, ((W << up) + 2 * pad[1] - k[1]) // s + 1
    return T("cx%s" % (case,), (B, Cin, H, W)), T("cw%s" % (case,), (Cout, Cin) + k, 0.2), T("cg%s" % (case,), (B, Cout, OH, OW))


def up_inputs(case):
    """(x, w, g) of an UP_CASES row (nearest x2 + conv3x3 p1), as test_upsample_conv3x3_both_formulations"""
    B, Cin, H, W, Cout = case
    return T("ux%s" % (case,), (B, Cin, H, W)), T("uw%s" % (case,), (Cout, Cin, 3, 3), 0.2), T("ug%s" % (case,), (B, Cout, 2 * H, 2 * W))


def pk_inputs(case, wgrad=False):
    """(x, w, g) of a PK_CASES / PK_WGRAD_CASES row, as test_packed_weight_convolution / test_packed_weight_gradient"""
    B, Cin, H, W, Cout, k, s, pad = case
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    p = "pw" if wgrad else "pk"
    return (T("%sx%s" % (p, case), (B, Cin, H, W)), T("%sw%s" % (p, case), (Cout, Cin, k, k), 0.2),
            T("%sg%s" % (p, case), (B, Cout, OH, OW)))


def as_conv_case(case, kind):
    """a row of any table in the layout of CONV_CASES"""
    if kind == "conv":
        return case
    if kind == "up":
        B, Cin, H, W, Cout = case
        return (B, Cin, H, W, Cout, (3, 3), 1, (1, 1), 1)
    B, Cin, H, W, Cout, k, s, pad = case
    return (B, Cin, H, W, Cout, (k, k), s, (pad, pad), 0)


def down2(t):
    """backward of the nearest x2 upsample: sums of 2x2 blocks"""
    B, C, H, W = t.shape
    return t.view(B, C, H // 2, 2, W // 2, 2).sum((3, 5))


def conv_all(x, w, g, s, pad, up):
    """forward, data gradient and weight gradient of conv2d(upsample?(x), w) in the dtype of the operands:
    y, dxu (gradient in the domain the convolution sees: the upsampled one for up = 1), dx (at the resolution of x), dw"""
    xu = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    y = F.conv2d(xu, w, None, s, pad)
    dxu = torch.nn.grad.conv2d_input(xu.shape, w, g, s, pad)
    dw = torch.nn.grad.conv2d_weight(xu, w.shape, g, s, pad)
    return {"y": y, "dxu": dxu, "dx": down2(dxu) if up else dxu, "dw": dw}


def references(x, w, g, s, pad, up):
    """(ref, S): conv_all in fp64 and the same sums over the absolute values of both operands"""
    x, w, g = x.double(), w.double(), g.double()
    return conv_all(x, w, g, s, pad, up), conv_all(x.abs(), w.abs(), g.abs(), s, pad, up)


# ------------------------------------------------------------------------------------------------------ Winograd F(2x2,3x3)
# Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", section 4.1: Y = A^t [(G g G^t) .* (B^t d B)] A on 4x4
# input tiles d that overlap by two, 2x2 output tiles Y
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def _mats(dtype):
    return torch.tensor(_BT, dtype=dtype), torch.tensor(_G, dtype=dtype), torch.tensor(_AT, dtype=dtype)


def _tiles(xp, ty, tx):
    """(B, C, ty, tx, 4, 4): the 4x4 tiles at stride 2 of the padded input, transformed: B^t d B"""
    BT = _mats(xp.dtype)[0]
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)[:, :, :ty, :tx]
    return torch.einsum("ai,bcyxij,dj->bcyxad", BT, d, BT)


def wino_fwd(x, w, pad):
    """conv3x3 stride 1, padding `pad` (0 or 1), by F(2x2,3x3) in the dtype of the operands (odd output sizes: one more row / column
    of zero padding, cropped)"""
    B, C, H, W = x.shape
    oH, oW = H + 2 * pad - 2, W + 2 * pad - 2
    ty, tx = (oH + 1) // 2, (oW + 1) // 2
    xp = F.pad(x, (pad, 2 * tx + 2 - W - pad, pad, 2 * ty + 2 - H - pad))
    _, G, AT = _mats(x.dtype)
    U = torch.einsum("ai,ocij,dj->adoc", G, w, G)                       # (4, 4, Cout, Cin)
    V = _tiles(xp, ty, tx).permute(4, 5, 1, 0, 2, 3).reshape(4, 4, C, B * ty * tx)
    M = torch.matmul(U, V).view(4, 4, w.shape[0], B, ty, tx)
    Y = torch.einsum("ia,adobyx,jd->boyixj", AT, M, AT).reshape(B, w.shape[0], 2 * ty, 2 * tx)
    return Y[:, :, :oH, :oW].contiguous()


def wino_dgrad(g, w, pad):
    """data gradient of the same convolution: F(2x2,3x3) over dY with the rotated, (ci, co)-transposed filters, padding 2 - pad"""
    return wino_fwd(g, w.flip(2, 3).transpose(0, 1).contiguous(), 2 - pad)


def wino_wgrad(x, g):
    """weight gradient of conv3x3 s1 p1 (even H, W): dW = G^t [sum over tiles and images (A dY A^t) .* (B^t d B)] G"""
    B, C, H, W = x.shape
    ty, tx = H // 2, W // 2
    _, G, AT = _mats(x.dtype)
    V = _tiles(F.pad(x, (1, 1, 1, 1)), ty, tx).permute(4, 5, 0, 2, 3, 1).reshape(4, 4, B * ty * tx, C)
    dY = g.view(B, g.shape[1], ty, 2, tx, 2)
    Q = torch.einsum("ia,boyaxd,jd->ijobyx", AT.t().contiguous(), dY, AT.t().contiguous()).reshape(4, 4, g.shape[1], B * ty * tx)
    M = torch.matmul(Q, V)                                              # (4, 4, Cout, Cin)
    return torch.einsum("ai,adoc,dj->ocij", G, M, G)


def wino_geometry(case):
    """(forward, data gradient, weight gradient): whether the default dispatch hands the geometry to the Winograd kernels
    (csrc/mogan_wino.hip, mogan_wino_try / mogan_wino_wgrad_try: 3x3 s1 without upsample, reduced channels % 16 == 0 and >= 32,
    produced channels >= 64, 4 x 32 output tiles filled to 70 %; the weight gradient pad 1, >= 32 / >= 64 channels, even H,
    W % 16 == 0).  The GPU file checks the first two against mogan_wino_prep_bytes."""
    B, Cin, H, W, Cout, k, s, pad, up = case
    if not (k == (3, 3) and s == 1 and up == 0 and pad in ((0, 0), (1, 1))):
        return False, False, False
    cH, cW = H + 2 * pad[0] - 2, W + 2 * pad[1] - 2

    def takes(Kin, Kout, oH, oW):
        filled = oH * oW >= 0.7 * (-(-oH // 4) * 4) * (-(-oW // 32) * 32)
        return cH >= 2 and cW >= 2 and Kin % 16 == 0 and Kin >= 32 and Kout >= 64 and filled

    wg = pad == (1, 1) and Cin >= 32 and Cout >= 64 and H % 2 == 0 and W % 16 == 0
    return takes(Cin, Cout, cH, cW), takes(Cout, Cin, H, W), wg
