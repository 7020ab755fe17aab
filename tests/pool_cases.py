"""Shapes, inputs, fp64 references and per-element bounds of the pooling, resize, sum and feeder entry points of
include/mogan_hip.h (csrc/mogan_elem.hip: mogan_avgpool_*, mogan_maxpool_* (the dense wrappers), mogan_bilinear_*, mogan_add,
mogan_scale, mogan_group_sum, mogan_group_bcast; csrc/mogan_feed.hip: mogan_feed_crop_flip, mogan_feed_resample).  A plain helper
module, not a conftest, like tests/bn_cases.py.  tests/test_pool_entry_points_gpu.py runs every row through the C ABI under
tests/memguard.py; tests/test_pool_reference_cpu.py keeps the references equal to torch's fp64 operators (and to Pillow), measures
TOL below, shows that the bounds reject the usual wrong variants and counts what the rows reach; tests/test_pool_rejections_cpu.py
holds what the host answers before a launch.  Nothing here needs a GPU or the library.

Average pool (count_include_pad=True, floor mode).  The reference is the explicit window sum over the zero-padded plane.
    forward   |got - ref| <= TOL["avg"] * S,  S = (terms + 2) * 2^-24 * (window sum of |x|) / k^2, terms = the in-bounds elements
              of the window (the kernel adds only those: terms - 1 additions, the rounded 1 / k^2 and the product)
    backward  |got - ref| <= 4 * 2^-24 * (sum of |dy| / k^2 over the windows that hold the element) -- the bound of
              test_trunk_entry_points_gpu.test_avgpool_bwd_ex; an element in no window has bound 0 and is exactly +0
Max pool (no padding).  y is exact against F.max_pool2d, idx exact against `pool_offsets` (oracle.inception_oracle.pool_offsets
    for any (k, s): the offset a * k + b of the first maximum in row-major order); the backward routes dy through idx in fp64,
    bound 4 * 2^-24 * (sum of |dy| routed to the element), elements that receive nothing are exactly +0.
    NaN inputs are out of scope: the kernel's `v > m` skips a NaN where torch propagates it.
Bilinear (align_corners=False).  Two 1-D weight matrices Wy (OH x H), Wx (OW x W) from the exact fp64 source coordinate
    src = max((o + 0.5) * in / out - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0:  y = Wy x Wx^T and
    dx = Wy^T dy Wx.  The kernel's coordinate is fp32 (possibly contracted into an FMA), so its src is off by a few ulps of
    src + 1, and the interpolant -- continuous, piecewise linear -- moves with it by at most that times the neighbouring values.
    With N the 0/1 band matrix with ones at the columns i0 - 1 .. i0 + 2 (clamped):
    forward   TOL["bil"] * 2^-24 * (A + ((src_y + 1) + (src_x + 1)) * R),  A = Wy |x| Wx^T, R = Ny |x| Nx^T
    backward  TOL["bil"] * 2^-24 * (Wy^T |dy| Wx + (diag(src_y + 1) Ny)^T |dy| Nx + Ny^T |dy| (diag(src_x + 1) Nx))
    Where the bound is 0 the comparison is exact.  The identity row is bitwise equal to its input both ways.
Sums.  IEEE-exact, compared bit for bit with the same fp32 operations of torch on the CPU (operands: +-0, +-inf, subnormals, pairs
    that cancel exactly; no NaN operand.  inf * 0 of mogan_scale is the one NaN result: a NaN for a NaN, whatever its payload).
Feeder.  Bytes and fp32 images bit for bit: the crop against slicing, the resampling against the two numpy passes of
    attngan/feeder.resample_u8_reference, restated below so that the intermediate image `tmp` is returned as well.

The `long long` instantiations behind POOL_LAUNCH need 2^31 elements and stay unrun.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import TOL_CEILING  # noqa: F401  (what the project accepts per element)

EPS32 = 2.0 ** -24
BIL_MAXC = 8                  # csrc/mogan_elem.hip: the candidates per axis the register path of bilinear_bwd_kernel holds
BLOCK = 256
GRID_CAP = 262144             # nblk() of csrc/mogan_elem.hip: beyond this many blocks a thread takes a second trip

# Per-element tolerances: 4 x the largest err / bound-with-TOL-1 of two fp32 CPU evaluations over every row
# (tests/test_pool_reference_cpu.py measures both, asserts the factor and the ceiling, and prints the figures).  Measured:
#     avg   torch's fp32 avg_pool2d 0.298                 the kernel's arithmetic in numpy fp32 (sequential sum, * fl32(1/k^2)) 0.298
#     bil   torch's fp32 interpolate + autograd 0.828     bil_src in numpy fp32, coordinate rounded twice and rounded once   0.806
# (in units of the bound with TOL = 1, which already carries 2^-24: TOL * 2^-24 is what compares with conv_cases.TOL)
MEASURED = {"avg": 0.30, "bil": 0.83}
TOL = {"avg": 1.2, "bil": 3.32}

AVG_ROWS = [(6, 35, 35, 3, 1, 1), (5, 8, 8, 8, 8, 0), (7, 11, 6, 3, 2, 1), (3, 9, 10, 2, 2, 0), (2, 7, 5, 5, 3, 2), (1, 3, 3, 3, 1, 0),
            (300, 4, 4, 2, 2, 0)]                                          # (planes, H, W, k, s, pad)
MAX_ROWS = [(5, 10, 9, 3, 2), (4, 8, 8, 2, 2), (3, 10, 7, 3, 3), (3, 9, 9, 4, 2), (2, 6, 6, 2, 1), (2, 5, 5, 1, 2), (2, 5, 5, 1, 1),
            (50, 7, 6, 3, 2)]                  # (the last: 300 outputs, the one row whose forward is more than one block)
MAX_FWD_ONLY = (2, 9, 9, 5, 1)                                             # (planes, H, W, k, s); k > 2 s: no backward
BIL_ROWS = [(3, 17, 17, 17, 17), (6, 6, 7, 7, 9), (2, 8, 8, 13, 13), (1, 30, 30, 7, 200), (2, 4, 5, 32, 33), (2, 40, 24, 13, 9),
            (1, 1, 9, 3, 4), (1, 9, 1, 1, 1), (40, 5, 5, 3, 4)]            # (planes, H, W, OH, OW)
BIL_IDENTITY = BIL_ROWS[0]
BIL_VARIANTS = ("align_corners", "no_half_pixel", "swapped", "unclamped")
SUM_N = (1, 255, 256, 257, 1000003)
SUM_G = (1, 3, 4)
ALPHAS = (0.5, -1.0, 1.0 / 3.0, 0.0)
ADD_LARGE_N = GRID_CAP * BLOCK + 257       # the smallest n at which a whole block (and one thread more) takes the second trip
CROP_ROWS = [((3, 11, 8), ((0, 0, 0), (3, 3, 1), (1, 2, 1))),
             ((2, 8, 8), ((0, 0, 0), (0, 0, 1))),
             ((5, 20, 17), ((0, 3, 0), (3, 0, 1), (3, 3, 0), (0, 0, 1), (1, 2, 1)))]     # (B, ori, size), (h1, w1, flip) per sample
RESAMPLE_ROWS = [(5, 12, 5), (2, 9, 4), (2, 6, 9), (2, 16, 8), (2, 13, 1), (2, 7, 7), (1, 20, 3)]      # (B, S, OS)
CHAIN = (CROP_ROWS[2], 9)                  # mogan_feed_resample on the q that mogan_feed_crop_flip wrote: 17 -> 9
PRECISION_BITS = 32 - 8 - 2                # attngan/feeder.PRECISION_BITS (the CPU module asserts the two agree)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def T(name, shape, scale=1.0):
    """deterministic N(0, 1) * scale fp32 tensor keyed by `name`"""
    return torch.randn(tuple(shape), generator=_gen(name)) * scale


def out_size(n, k, s, pad=0):
    return (n + 2 * pad - k) // s + 1


# ------------------------------------------------------------------------------------------------------------ average pool
def _windows(t, k, s, pad, OH, OW):
    """the k * k shifted views of the zero-padded planes: one (planes, OH, OW) tensor per window offset, row-major"""
    tp = F.pad(t, (pad, pad, pad, pad))
    return [tp[:, a:a + (OH - 1) * s + 1:s, b:b + (OW - 1) * s + 1:s] for a in range(k) for b in range(k)]


def _scatter(d, H, W, k, s, pad, scale):
    """sum over the windows that hold an element of d * scale: (planes, OH, OW) -> (planes, H, W)"""
    P, OH, OW = d.shape
    g = torch.zeros((P, H + 2 * pad + k, W + 2 * pad + k), dtype=torch.float64)
    for a in range(k):
        for b in range(k):
            g[:, a:a + (OH - 1) * s + 1:s, b:b + (OW - 1) * s + 1:s] += d * scale
    return g[:, pad:pad + H, pad:pad + W].contiguous()


@functools.lru_cache(maxsize=None)
def avg_case(row, divisor="k2"):
    """inputs, fp64 references and bounds (with TOL 1) of one average-pool row.  divisor: "k2" (count_include_pad=True, the kernel's),
    or the wrong one "clipped" (the size of the window clipped to the plane: count_include_pad=False) for the CPU module"""
    P, H, W, k, s, pad = row
    OH, OW = out_size(H, k, s, pad), out_size(W, k, s, pad)
    x, dy = T("avgx%s" % (row,), (P, H, W)), T("avgdy%s" % (row,), (P, OH, OW))
    x64, dy64 = x.double(), dy.double()
    terms = sum(_windows(torch.ones((1, H, W), dtype=torch.float64), k, s, pad, OH, OW))       # in-bounds elements per window
    div = torch.full_like(terms, float(k * k)) if divisor == "k2" else terms
    y =sum(_windows(x64, k, s, pad, OH, OW)) / div
    S = (terms + 2) * EPS32 * sum(_windows(x64.abs(), k, s, pad, OH, OW)) / (k * k)
    dx = _scatter(dy64 / div, H, W, k, s, pad, 1.0)
    dxa = _scatter(dy64.abs(), H, W, k, s, pad, 1.0 / (k * k))
    covered = _scatter(torch.ones((1, OH, OW), dtype=torch.float64), H, W, k, s, pad, 1.0)[0] > 0
    return dict(x=x, dy=dy, y=y, y_bound=S, dx=dx, dx_bound=4 * EPS32 * dxa, covered=covered, terms=terms[0], OH=OH, OW=OW)


def avg_restate_fp32(x, k, s, pad):
    """the kernel's forward in numpy fp32: the in-bounds elements of a window added in row-major order, times fl32(1 / k^2)"""
    P, H, W = x.shape
    OH, OW = out_size(H, k, s, pad), out_size(W, k, s, pad)
    xp = np.zeros((P, H + 2 * pad, W + 2 * pad), dtype=np.float32)
    xp[:, pad:pad + H, pad:pad + W] = x           # (x + 0 = x: adding the padding's zeros changes no bit of a sum of non-zero values)
    acc = np.zeros((P, OH, OW), dtype=np.float32)
    for a in range(k):
        for b in range(k):
            acc = acc + xp[:, a:a + (OH - 1) * s + 1:s, b:b + (OW - 1) * s + 1:s]
    return acc * (np.float32(1.0) / np.float32(k * k))


# ----------------------------------------------------------------------------------------------------------------- max pool
def pool_offsets(x, k, s):
    """oracle.inception_oracle.pool_offsets for any (k, s): the window offset a * k + b of the first maximum of every window"""
    H, W = x.shape[-2:]
    _, i = F.max_pool2d(x, k, s, return_indices=True)
    OH, OW = i.shape[-2:]
    a = i // W - torch.arange(OH).view(OH, 1) * s
    b = i % W - torch.arange(OW).view(1, OW) * s
    return (a * k + b).to(torch.uint8)


def max_route(idx, d, H, W, k, s):
    """fp64 max-pool gradient through the window offsets idx: dx[p, oy s + a, ox s + b] += d[p, oy, ox]; (dx, number of windows
    routed to each element)"""
    P, OH, OW = d.shape
    a, b = idx.long() // k, idx.long() % k
    pos = (torch.arange(OH).view(1, OH, 1) * s + a) * W + torch.arange(OW).view(1, 1, OW) * s + b
    out = torch.zeros((P, H * W), dtype=torch.float64).scatter_add_(1, pos.reshape(P, -1), d.double().reshape(P, -1))
    cnt = torch.zeros((P, H * W), dtype=torch.float64).scatter_add_(1, pos.reshape(P, -1), torch.ones((P, OH * OW), dtype=torch.float64))
    return out.view(P, H, W), cnt.view(P, H, W)


@functools.lru_cache(maxsize=None)
def max_case(row):
    """post-ReLU input (ties among zeros) with three planted windows: equal positive values (plane 0, the first window), +0.0 and
    -0.0 alternating from -0.0 (plane 1, the first window of the last row) and all -inf (plane 1, the last window)"""
    P, H, W, k, s = row
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    assert P >= 2 and OH >= 2 and OW >= 2
    x = torch.relu(T("maxx%s" % (row,), (P, H, W)))
    x[0, 0:k, 0:k] = 0.25
    y0 = (OH - 1) * s
    zeros = torch.zeros(k * k)
    zeros[0::2] = -0.0
    x[1, y0:y0 + k, 0:k] = zeros.view(k, k)
    x0 = (OW - 1) * s
    x[1, y0:y0 + k, x0:x0 + k] = float("-inf")
    dy = T("maxdy%s" % (row,), (P, OH, OW))
    y = F.max_pool2d(x, k, s)
    idx = pool_offsets(x, k, s)
    dx, cnt = max_route(idx, dy, H, W, k, s)
    dxa, _ = max_route(idx, dy.abs(), H, W, k, s)
    return dict(x=x, dy=dy, y=y, idx=idx, dx=dx, dx_bound=4 * EPS32 * dxa, routed=cnt, OH=OH, OW=OW,
                planted={"tie": (0, 0, 0), "zeros": (1, OH - 1, 0), "-inf": (1, OH - 1, OW - 1)})


# ------------------------------------------------------------------------------------------------------------------ bilinear
def bil_taps(n_in, n_out, variant=None):
    """(src, i0, i1, l1) per output index in fp64.  variant: None (the operator), or one of the wrong ones of BIL_VARIANTS"""
    o = np.arange(n_out, dtype=np.float64)
    if variant == "align_corners":
        src = o * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros(n_out)
    elif variant == "no_half_pixel":
        src = o * n_in / n_out
    else:
        src = np.maximum((o + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + 1 if variant == "unclamped" else np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    if variant == "swapped":
        l1 = 1.0 - l1
    return src, i0, i1, l1


def bil_matrices(n_in, n_out):
    """(W, N, src): the (n_out, n_in) weight matrix, the 0/1 band matrix with ones at i0 - 1 .. i0 + 2 (clamped), the coordinate"""
    src, i0, i1, l1 = bil_taps(n_in, n_out)
    Wm, N = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    r = np.arange(n_out)
    np.add.at(Wm, (r, i0), 1.0 - l1)
    np.add.at(Wm, (r, i1), l1)
    for d in (-1, 0, 1, 2):
        N[r, np.clip(i0 + d, 0, n_in - 1)] = 1.0
    return torch.from_numpy(Wm), torch.from_numpy(N), torch.from_numpy(src)


def bil_dense(row, variant=None):
    """the whole resize as one dense (planes * OH * OW, planes * H * W + W + 2) fp64 matrix over the flat tensor, so that the
    "unclamped" variant reads what a kernel without the clamp would: the next row's first pixel, the next plane's first row (zero
    columns stand for what lies past the end).  Forward M x, backward M^T dy."""
    P, H, W, OH, OW = row
    _, y0, y1, ly = bil_taps(H, OH, variant)
    _, x0, x1, lx = bil_taps(W, OW, variant)
    M = np.zeros((P * OH * OW, P * H * W + W + 2))
    rows = np.arange(P * OH * OW).reshape(P, OH, OW)
    base = (np.arange(P) * H * W).reshape(P, 1, 1)
    for yi, wy in ((y0, 1.0 - ly), (y1, ly)):
        for xi, wx in ((x0, 1.0 - lx), (x1, lx)):
            cols = base + yi.reshape(1, OH, 1) * W + xi.reshape(1, 1, OW)
            np.add.at(M, (rows.ravel(), cols.ravel()), np.broadcast_to(wy.reshape(1, OH, 1) * wx.reshape(1, 1, OW), (P, OH, OW)).ravel())
    return torch.from_numpy(M)


@functools.lru_cache(maxsize=None)
def bil_case(row):
    """inputs, fp64 references and bounds (with TOL 1) of one bilinear row; `unread`: the input elements no output reads"""
    P, H, W, OH, OW = row
    x, dy = T("bilx%s" % (row,), (P, H, W)), T("bildy%s" % (row,), (P, OH, OW))
    Wy, Ny, sy = bil_matrices(H, OH)
    Wx, Nx, sx = bil_matrices(W, OW)
    x64, dy64 = x.double(), dy.double()
    y = Wy @ x64 @ Wx.T
    A, R = Wy @ x64.abs() @ Wx.T, Ny @ x64.abs() @ Nx.T
    y_bound = EPS32 * (A + ((sy + 1).view(OH, 1) + (sx + 1).view(1, OW)) * R)
    dx = Wy.T @ dy64 @ Wx
    da = dy64.abs()
    dx_bound = EPS32 * (Wy.T @ da @ Wx + ((sy + 1).view(OH, 1) * Ny).T @ da @ Nx + Ny.T @ da @ ((sx + 1).view(OW, 1) * Nx))
    unread = ((Wy.sum(0) == 0).view(H, 1) | (Wx.sum(0) == 0).view(1, W)).expand(P, H, W)
    return dict(x=x, dy=dy, y=y, y_bound=y_bound, dx=dx, dx_bound=dx_bound, unread=unread)


def bil_src32(n_in, n_out, contracted):
    """bil_src of csrc/mogan_elem.hip in numpy fp32: (i0, i1, l1).  The coordinate with every operation rounded, or (contracted)
    with the product and the subtraction rounded once, as an FMA leaves it"""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out).astype(np.float32) + np.float32(0.5)
    if contracted:
        src = (o.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32)
    else:
        src = (o * scale).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0.0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def bil_restate_fp32(x, dy, OH, OW, contracted):
    """both bilinear kernels in numpy fp32, operand order kept: the forward's two lerps; the backward's sums over the outputs in
    ascending order with the weights bil_w forms ((i0 == i ? 1 - l1 : 0) + (i1 == i ? l1 : 0)).  A zero weight adds x * 0 = 0."""
    P, H, W = x.shape
    one = np.float32(1.0)
    y0, y1, ly = bil_src32(H, OH, contracted)
    x0, x1, lx = bil_src32(W, OW, contracted)
    ly_, lx_ = ly.reshape(1, OH, 1), lx.reshape(1, 1, OW)
    g = lambda yi, xi: x[:, yi][:, :, xi]
    y = (one - ly_) * ((one - lx_) * g(y0, x0) + lx_ * g(y0, x1)) + ly_ * ((one - lx_) * g(y1, x0) + lx_ * g(y1, x1))

    def w32(i0, i1, l1, n_in):
        cols = np.arange(n_in).reshape(1, n_in)
        return (np.where(i0.reshape(-1, 1) == cols, (one - l1).reshape(-1, 1), np.float32(0)) +
                np.where(i1.reshape(-1, 1) == cols, l1.reshape(-1, 1), np.float32(0))).astype(np.float32)
    wy, wx = w32(y0, y1, ly, H), w32(x0, x1, lx, W)
    r = np.zeros((P, OH, W), dtype=np.float32)
    for ox in range(OW):
        r = r + wx[ox].reshape(1, 1, W) * dy[:, :, ox:ox + 1]
    dx = np.zeros((P, H, W), dtype=np.float32)
    for oy in range(OH):
        dx = dx + wy[oy].reshape(1, H, 1) * r[:, oy:oy + 1, :]
    return y.astype(np.float32), dx


def bil_bwd_branches(row):
    """which branches of bilinear_bwd_kernel the row's threads take, by bil_cand restated in fp32: {"register", "loop"}"""
    P, H, W, OH, OW = row
    inv = np.float32(1.0) / (np.float32(W) / np.float32(OW))
    i = np.arange(W).astype(np.float32)
    lo = np.floor((i - np.float32(0.5)) * inv - np.float32(0.5)).astype(np.int64) - 1
    hi = np.ceil((i + np.float32(1.5)) * inv - np.float32(0.5)).astype(np.int64) + 1
    lo, hi = np.maximum(lo, 0), np.minimum(hi, OW - 1)
    return {"register" if d < BIL_MAXC else "loop" for d in (hi - lo).tolist()}


# ---------------------------------------------------------------------------------------------------------------------- sums
_SUB = 2.0 ** -149                         # the smallest subnormal
_MINN = 2.0 ** -126                        # the smallest normal
SPECIAL_PAIRS = [(0.0, -0.0), (-0.0, -0.0), (float("inf"), 1.0), (float("-inf"), float("-inf")), (_SUB, _SUB), (3 * _SUB, -3 * _SUB),
                 (1.5, -1.5), (_MINN, -_SUB), (3e38, 3e38), (-0.0, 0.0), (2.0 ** -130, 2.0 ** -140), (float("inf"), -3e38),
                 (-_MINN, _MINN), (1.0, 2.0 ** -24), (2.0 ** -127, 2.0 ** -127)]


def sum_operands(n, G=2, tag=""):
    """(G, n) fp32 operands: noise, with SPECIAL_PAIRS in the first places of groups 0 and 1 (as many as fit); no NaN, and no sum of
    the groups in order is one"""
    x = T("sum%s%d_%d" % (tag, n, G), (G, n))
    m = min(n, len(SPECIAL_PAIRS))
    sp = torch.tensor(SPECIAL_PAIRS[:m], dtype=torch.float64).float()
    x[0, :m] = sp[:, 0]
    if G > 1:
        x[1, :m] = sp[:, 1]
    return x


def group_sum_reference(x):
    """((x0 + x1) + x2) + ... in fp32"""
    t = x[0].clone()
    for g in range(1, x.shape[0]):
        t = t + x[g]
    return t


def same_ieee(got, want):
    """bit for bit, a NaN for a NaN (IEEE 754 does not fix the payload of inf * 0)"""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    return bool(((got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))).all())


# -------------------------------------------------------------------------------------------------------------------- feeder
def _images(name, B, S):
    """(B, S, S, 3) u8: noise, a 0 / 255 checkerboard (clip8 and the rounding bias) and a ramp, in turn"""
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    yy, xx = np.mgrid[0:S, 0:S]
    out = []
    for b in range(B):
        if b % 3 == 0:
            img = rng.randint(0, 256, (S, S, 3))
        elif b % 3 == 1:
            img = np.stack([((xx + yy) % 2) * 255, ((xx + yy + 1) % 2) * 255, ((xx // 2 + yy) % 2) * 255], -1)
        else:
            img = np.stack([(xx * 255) // max(S - 1, 1), 255 - (yy * 255) // max(S - 1, 1), ((xx + yy) * 37) % 256], -1)
        out.append(img.astype(np.uint8))
    return np.stack(out)


def normalise(u8):
    """((u8 / 255) - 0.5) / 0.5 in fp32, (B, n, n, 3) u8 -> (B, 3, n, n): ToTensor + Normalize as the kernels form them"""
    f = torch.from_numpy(np.ascontiguousarray(u8)).float() / 255.0
    return ((f - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def crop_case(row):
    (B, ori, size), params = row
    assert len(params) == B and all(0 <= h1 <= ori - size and 0 <= w1 <= ori - size for h1, w1, _ in params)
    src = _images("crop%s" % ((B, ori, size),), B, ori)
    q = np.stack([src[b, w1:w1 + size, h1:h1 + size][:, ::-1 if flip else 1] for b, (h1, w1, flip) in enumerate(params)])
    return dict(src=torch.from_numpy(src), params=torch.tensor(params, dtype=torch.int32), q=torch.from_numpy(np.ascontiguousarray(q)),
                out=normalise(q))


def resample_two_pass(img, bounds, kk):
    """the two passes of attngan/feeder.resample_u8_reference on (B, S, S, 3) u8 with the given tables: (tmp (B, S, OS, 3), out
    (B, OS, OS, 3)), both u8"""
    B, S = img.shape[:2]
    OS = bounds.shape[0]
    half = 1 << (PRECISION_BITS - 1)
    tmp = np.zeros((B, S, OS, 3), dtype=np.uint8)
    a = img.astype(np.int64)
    for ox in range(OS):
        x0, n = bounds[ox]
        acc = half + (a[:, :, x0:x0 + n, :] * kk[ox, :n].astype(np.int64)[None, None, :, None]).sum(2)
        tmp[:, :, ox, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    out = np.zeros((B, OS, OS, 3), dtype=np.uint8)
    t = tmp.astype(np.int64)
    for oy in range(OS):
        y0, n = bounds[oy]
        acc = half + (t[:, y0:y0 + n, :, :] * kk[oy, :n].astype(np.int64)[None, :, None, None]).sum(1)
        out[:, oy] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return tmp, out


def resample_expect(img, bounds, kk):
    """what mogan_feed_resample leaves for the u8 images `img` (a (B, S, S, 3) tensor): tmp and the fp32 out"""
    tmp, out = resample_two_pass(img.numpy(), bounds, kk)
    return dict(tmp=torch.from_numpy(tmp), out=normalise(out), out_u8=out)


@functools.lru_cache(maxsize=None)
def resample_case(row, tables):
    """tables: attngan.feeder.pil_bilinear_coeffs (handed in: this module does not import the package)"""
    B, S, OS = row
    bounds, kk = tables(S, OS)
    img = torch.from_numpy(_images("resample%s" % (row,), B, S))
    return dict(resample_expect(img, bounds, kk), img=img, bounds=torch.from_numpy(bounds.copy()), kk=torch.from_numpy(kk.copy()),
                ksize=kk.shape[1])


def launches():
    """threads of the largest launch of each kernel over the tables (one thread per output element; the census of the CPU module)"""
    n = {}
    n["avgpool_fwd"] = max(P * out_size(H, k, s, p) * out_size(W, k, s, p) for P, H, W, k, s, p in AVG_ROWS)
    n["avgpool_bwd"] = max(P * H * W for P, H, W, k, s, p in AVG_ROWS)
    n["maxpool_fwd"] = max(P * out_size(H, k, s) * out_size(W, k, s) for P, H, W, k, s in MAX_ROWS)
    n["maxpool_bwd"] = max(P * H * W for P, H, W, k, s in MAX_ROWS)
    n["bilinear_fwd"] = max(P * OH * OW for P, H, W, OH, OW in BIL_ROWS)
    n["bilinear_bwd"] = max(P * H * W for P, H, W, OH, OW in BIL_ROWS)
    n["add"] = n["scale"] = n["group_sum"] = n["group_bcast"] = max(SUM_N)
    n["feed_crop"] = max(B * size * size for (B, ori, size), _ in CROP_ROWS)
    rs = RESAMPLE_ROWS + [(CHAIN[0][0][0], CHAIN[0][0][2], CHAIN[1])]
    n["feed_resample_h"] = max(B * S * OS for B, S, OS in rs)
    n["feed_resample_v"] = max(B * OS * OS for B, S, OS in rs)
    return n
