"""The oracle, cases and bounds of the object-level Frechet distance's tests (tests/test_scenefid_reference_cpu.py,
test_scenefid_cpu.py, test_scenefid_rejections_cpu.py, test_scenefid_gpu.py): a plain helper module, no GPU.  The oracle restates the
definition of mogan_roi_resize (include/mogan_hip.h; attngan/scenefid.py) in numpy and shares nothing with the code under test: the
coordinates and weights in fp32, operation by operation -- every numpy fp32 operation rounds once, which is what the kernel's
__fmul_rn / __fdiv_rn / __fadd_rn / __fsub_rn do --, the blend in the dtype the caller asks for.

TOL_BLEND is derived, not measured: with the coordinates' bits shared, kernel and fp64 oracle differ by the blend alone, which is
seven fp32 roundings (1 - lx, two products and a sum per row -- the rows run side by side, so a path through the expression meets
three --, 1 - ly, a product and the last sum) of quantities bounded by max|x|, the weights lying in [0, 1]; contraction only removes
roundings.  MEASURED records what the fp32 blend of this oracle is off the fp64 one, in units of 2^-24 max|x|, over 400 random
cases (test_scenefid_reference_cpu.py measures it again and holds it under the bound), and how far the full box lies from
torch.nn.functional.interpolate on the CPU."""
import zlib

import numpy as np

EPS = 2.0 ** -24
TOL_BLEND_ULPS = 7
MEASURED = {"blend_ulps": 2.65, "interpolate": 3.7e-6}      # the latter at 256 -> 299: torch's build contracts the coordinate
ABSENT = (-1.0, -1.0, -1.0, -1.0)


def tol_blend(x):
    return TOL_BLEND_ULPS * EPS * float(np.abs(x).max())


def seed_of(what, case):
    return zlib.crc32(("%s %s" % (what, case)).encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- the definition
def axis_taps(b0, bl, n, on):
    """(i0, i1, l) of the `on` output positions of an axis of n source pixels for a box from b0, bl long (relative): fp32, one
    rounding per operation, in the definition's order"""
    f = np.float32
    p0 = f(b0) * f(n)
    pl = f(bl) * f(n)
    scale = pl / f(on)
    j = np.arange(on, dtype=np.float32)
    src = p0 + ((j + f(0.5)) * scale - f(0.5))
    assert src.dtype == np.float32 and type(scale) is np.float32
    src = np.minimum(np.maximum(src, f(0)), f(n - 1))
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    l = src - i0.astype(np.float32)
    assert l.dtype == np.float32
    return i0, i1, l


def roi_resize_oracle(x, boxes, index, OH, OW, blend=np.float64):
    """x (B, C, H, W) fp32, boxes (R, 4) fp32, index (R) -> (R, C, OH, OW) in `blend`: the definition, the blend in `blend`
    arithmetic.  An absent box (w <= 0 or h <= 0), a box value that is not finite and an index outside [0, B) give zeros."""
    x = np.asarray(x, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    B, C, H, W = x.shape
    out = np.zeros((len(boxes), C, OH, OW), dtype=blend)
    for r, (box, b) in enumerate(zip(boxes, index)):
        if not np.isfinite(box).all() or not box[2] > 0 or not box[3] > 0 or not 0 <= int(b) < B:
            continue
        x0, x1, lx = axis_taps(box[0], box[2], W, OW)
        y0, y1, ly = axis_taps(box[1], box[3], H, OH)
        lx, ly = lx.astype(blend)[None, None, :], ly.astype(blend)[None, :, None]
        hx, hy = blend(1) - lx, blend(1) - ly
        img = x[int(b)].astype(blend)
        top = hx * img[:, y0][:, :, x0] + lx * img[:, y0][:, :, x1]
        bot = hx * img[:, y1][:, :, x0] + lx * img[:, y1][:, :, x1]
        out[r] = hy * top + ly * bot
        assert out[r].dtype == blend and top.dtype == blend
    return out


# ------------------------------------------------------------------------------------------------- the kernel's cases
# the list every multi-image case shares: two boxes of image 0, an absent one in the middle of the list, none of image 1, and on
# image 2 a box that touches the right and bottom edges (x + w = y + h = 0.999), the full box, a box thinner than one pixel at every
# W used here, one that reaches past the image on the right and below and one that starts left of and above it
MIXED = ((0, (0.1, 0.2, 0.5, 0.4)), (0, (0.3, 0.1, 0.25, 0.6)), (0, ABSENT), (2, (0.5, 0.6, 0.499, 0.399)), (2, (0.0, 0.0, 1.0, 1.0)),
         (2, (0.4, 0.3, 0.01, 0.5)), (2, (0.7, 0.8, 0.6, 0.5)), (0, (-0.2, -0.1, 0.5, 0.5)), (2, (0.25, 0.125, 0.5, 0.005)))

# name -> (B, C, H, W, OH, OW, ((image, box), ...)).  One thread per output pixel in blocks of 256: "one block" stays inside one,
# the others end in a partly filled block (R OH OW is no multiple of 256 in any case); H W is a multiple of 64 only in "product".
KERNEL_CASES = {
    "mixed 3x33x40 to 19x23": (3, 3, 33, 40, 19, 23, MIXED),
    "one channel, one output row": (1, 1, 7, 5, 1, 9, ((0, (0.2, 0.1, 0.6, 0.7)), (0, (0.0, 0.0, 1.0, 1.0)), (0, ABSENT))),
    "four channels, one output column": (3, 4, 16, 12, 11, 1, MIXED),
    "one block": (1, 3, 5, 9, 6, 7, ((0, (0.0, 0.0, 1.0, 1.0)), (0, (0.5, 0.5, 0.499, 0.499)))),
    "one source pixel": (2, 3, 1, 1, 4, 5, ((1, (0.0, 0.0, 1.0, 1.0)), (0, (0.3, 0.3, 0.2, 0.2)), (1, ABSENT))),
    "upscale 3x17x13 to 40x37": (3, 3, 17, 13, 40, 37, MIXED),
    "product": (3, 3, 256, 256, 299, 299, ((0, (0.12, 0.3, 0.41, 0.37)), (2, (0.5, 0.6, 0.499, 0.399)), (0, ABSENT),
                                           (2, (0.0, 0.0, 1.0, 1.0)))),
}


def kernel_case(name):
    """(x, boxes (R, 4) fp32, index (R) int32, OH, OW, want (R, C, OH, OW) fp64) of a kernel case: x uniform in (-1, 1)"""
    B, C, H, W, OH, OW, rois = KERNEL_CASES[name]
    rng = np.random.RandomState(seed_of("kernel", name))
    x = rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    boxes = np.array([box for _, box in rois], dtype=np.float32)
    index = np.array([b for b, _ in rois], dtype=np.int32)
    return x, boxes, index, OH, OW, roi_resize_oracle(x, boxes, index, OH, OW)


# integer-valued images (|v| < 64) and boxes whose scale is a power of two at the case's size: coordinates, weights (multiples of
# 1/8 at the least) and every product and sum of the blend are exact in fp32 in any order and under any contraction
EXACT_CASES = {
    "8x8, a quarter, to 8x8": (2, 3, 8, 8, 8, 8, ((1, (0.25, 0.5, 0.5, 0.5)), (0, (0.0, 0.0, 0.5, 0.5)))),
    "16x16, all of it, to 32x32": (1, 3, 16, 16, 32, 32, ((0, (0.0, 0.0, 1.0, 1.0)),)),
    "8x16, half of it, to 16x16": (2, 4, 8, 16, 16, 16, ((0, (0.0, 0.0, 0.5, 1.0)), (1, ABSENT), (1, (0.5, 0.5, 0.5, 0.5)))),
    "16x16, an eighth, to 4x4": (1, 1, 16, 16, 4, 4, ((0, (0.125, 0.25, 0.5, 0.25)),)),
}


def exact_case(name):
    """as kernel_case, the image integer-valued in (-64, 64); `want` is fp64 and every value of it is a fp32 number"""
    B, C, H, W, OH, OW, rois = EXACT_CASES[name]
    x = np.random.RandomState(seed_of("exact", name)).randint(-63, 64, (B, C, H, W)).astype(np.float32)
    boxes = np.array([box for _, box in rois], dtype=np.float32)
    index = np.array([b for b, _ in rois], dtype=np.int32)
    return x, boxes, index, OH, OW, roi_resize_oracle(x, boxes, index, OH, OW)


def random_case(rng):
    """one of the 400 cases the fp32 blend is measured on: small random shapes, boxes inside, at the edge and past the image"""
    B, C = int(rng.randint(1, 4)), int(rng.randint(1, 5))
    H, W, OH, OW = (int(v) for v in rng.randint(1, 41, 4))
    R = int(rng.randint(1, 6))
    boxes = np.concatenate([rng.uniform(-0.2, 0.8, (R, 2)), rng.uniform(0.005, 0.9, (R, 2))], axis=1).astype(np.float32)
    x = (rng.uniform(-1, 1, (B, C, H, W)) * rng.choice([1.0, 3.0, 100.0])).astype(np.float32)
    return x, boxes, rng.randint(0, B, R).astype(np.int32), OH, OW


# ------------------------------------------------------------------------------------------------- the pass's boxes
def loader_boxes(length, seed, batch=4):
    """The (batches, batch, 3, 4) fp32 boxes of the data set's own samples in the order a pass of eval_setup.trainer(length, seed)
    sees them: the loader's batches in order, each sorted by caption length as prepare_data sorts it.  Call it after
    eval_setup.tiny_checkpoint (the data set takes its sizes from the config)."""
    import torch
    from mogan_amd.attngan.datasets import SyntheticTextDataset, prepare_data
    ds = SyntheticTextDataset(length=length, n_words=100, seed=seed, eval=True)
    dl = torch.utils.data.DataLoader(ds, batch_size=batch, drop_last=True, shuffle=False)
    return torch.stack([prepare_data(data, torch.device("cpu"), eval=True)[-1].float() for data in dl])
