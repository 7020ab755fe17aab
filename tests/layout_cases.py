"""The cases the tests of the layout-shift sums share (tests/test_layoutshift_gpu.py, test_layoutshift_cpu.py): images, edit tables,
the expected sums of the numpy oracle (attngan/layoutshift.sums_numpy) and the bound a device sum is held to.  A plain module.

CASES are (P, C, S, G): pairs, channels, side, rectangles of other objects per pair.
  (1, 1, 8, 0)      fewer pixels than threads, no other object (others = NULL on the device)
  (3, 3, 16, 2)     hand-made: rectangles touching each of the four edges, a 1 x 1 rectangle, a full-width rectangle moved along y only,
                    old and new rectangle overlapping and apart, another object overlapping the old rectangle, one reaching past the
                    image, an absent one
  (2, 3, 20, 1)     S not a power of two
  (5, 3, 64, 2)     more pairs
  (2, 3, 256, 3)    the product's size
  (2, 3, 7, 1)      S S no multiple of four: the kernel's 4-byte loads, and a last group of one pixel

The bound.  A sum of n non-negative fp64 terms t_i = (x_i - y_i)^2, x and y fp32 values, added in ANY order, is within
(n - 1) 2^-53 of the exact sum of the computed terms, relatively; a term is within 3 * 2^-53 of the exact square (the difference of
two fp32 values is exact in fp64 unless their exponents are more than 29 apart, one rounding then, doubled by the square, and the
square's own rounding).  The device's sum and the oracle's are therefore within 2 (n + 2) 2^-53 <= (n + 4) 2^-52 of each other,
relatively: bound = (n + 4) 2^-52 want, n the number of addends -- the pixels of the class (or of the old rectangle) times C.
Derived, not measured.  Counts are exact."""
import zlib

import numpy as np

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import layoutshift as LS  # noqa: E402

CASES = [(1, 1, 8, 0), (3, 3, 16, 2), (2, 3, 20, 1), (5, 3, 64, 2), (2, 3, 256, 3), (2, 3, 7, 1)]
EPS = 2.0 ** -52

HAND_EDIT = [[0, 0, 5, 4, 3, 2],          # touches the left and the top edge; old and new overlap
             [0, 10, 16, 14, 0, -10],     # full width (left and right edge), moved along y only to the top edge; old and new apart
             [15, 15, 16, 16, -7, -3]]    # 1 x 1 in the bottom right corner (right and bottom edge)
HAND_OTHERS = [[[2, 1, 9, 9], [12, 12, 16, 16]],       # the first overlaps the old rectangle and the new one
               [[-3, 8, 30, 12], [0, 0, 0, 0]],        # reaches past the image on both sides and into the old rectangle; absent
               [[5, 5, 5, 9], [14, 14, 16, 16]]]       # empty (x1 <= x0): absent; the second contains the old rectangle


def seed_of(what, key):
    return zlib.crc32(("%s %s" % (what, key)).encode()) & 0x7FFFFFFF


def images(key, what="a"):
    P, C, S, G = key
    rng = np.random.RandomState(seed_of("layout " + what, key))
    return np.clip(rng.standard_normal((P, C, S, S)) * 0.5, -1, 1).astype(np.float32)


def tables(key):
    """(edit (P, 6) int32, others (P, G, 4) int32)"""
    P, C, S, G = key
    if key == (3, 3, 16, 2):
        return np.array(HAND_EDIT, dtype=np.int32), np.array(HAND_OTHERS, dtype=np.int32)
    rng = np.random.RandomState(seed_of("layout tables", key))
    edit = np.zeros((P, 6), dtype=np.int32)
    others = np.zeros((P, G, 4), dtype=np.int32)
    for p in range(P):
        w, h = rng.randint(1, S // 2 + 1, 2)
        x0, y0 = rng.randint(0, S - w + 1), rng.randint(0, S - h + 1)
        rect = (x0, y0, x0 + w, y0 + h)
        offsets = LS.feasible_offsets(rect, S, 1)
        edit[p] = rect + offsets[rng.randint(len(offsets))]
        for g in range(G):
            ow, oh = rng.randint(1, S // 2 + 1, 2)
            ox, oy = rng.randint(-2, S - 1, 2)
            others[p, g] = (ox, oy, ox + ow, oy + oh) if (p + g) % 3 else (ox, oy, ox, oy + oh)       # every third one absent
    return edit, others


def case(key):
    """(a, b, edit, others) of a case, numpy"""
    edit, others = tables(key)
    return images(key, "a"), images(key, "b"), edit, others


_expected = {}


def expected(key):
    """(sums (P, 7), counts (P, 5), bound (P, 7)) of a case: computed once, handed out read-only"""
    if key not in _expected:
        a, b, edit, others = case(key)
        sums, counts = LS.sums_numpy(a, b, edit, others)
        bound = bound_of(sums, counts, edit, key[1])
        for t in (sums, counts, bound):
            t.setflags(write=False)
        _expected[key] = (sums, counts, bound)
    return _expected[key]


def addends(counts, edit, C):
    """(P, 7): the number of addends of every sum"""
    edit = np.asarray(edit, dtype=np.int64)
    area = (edit[:, 2] - edit[:, 0]) * (edit[:, 3] - edit[:, 1])
    return np.concatenate([np.asarray(counts, dtype=np.int64), area[:, None], area[:, None]], axis=1) * int(C)


def bound_of(sums, counts, edit, C):
    return (addends(counts, edit, C) + 4) * EPS * np.asarray(sums, dtype=np.float64)
