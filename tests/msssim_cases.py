"""The oracle, cases, seeds and bounds of the MS-SSIM tests (tests/test_msssim_reference_cpu.py, test_msssim_rejections_cpu.py,
test_msssim_gpu.py): a plain helper module.  The oracle is a numpy fp64 evaluation of the definition in attngan/msssim.py, written
here from the definition and sharing nothing with the code under test but the bits of the fp32 window, which the definition makes
an input.  No bound here comes from the code under test.

The bounds follow the project's rule: 4 x the larger error against fp64 of two fp32 CPU evaluations of the
same formula, taken over TOLERANCE_CASES x SEEDS x 8 pairs --
  * `level(..., np.float32)`: the numpy restatement in the centred form, every operation rounded to fp32;
  * `level_torch`: torch fp32 with conv2d (the window as a 1 x n and an n x 1 kernel) on the same formula.
MEASURED records what `measure()` gives (python tests/msssim_cases.py prints it); test_msssim_reference_cpu.py measures again on
the smaller cases and holds the record to it.  The level means are fp64 means of fp32 maps in all three."""
import functools
import zlib

import numpy as np

C1, C2 = 6.5025, 58.5225
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TILE = 32                                        # the kernel's tile of valid positions per axis (csrc/mogan_ssim.hip)

# (S, L, C) of the tolerance cases; 5 seeds x 8 pairs each
TOLERANCE_CASES = ((64, 5, 1), (64, 5, 3), (32, 4, 3), (16, 3, 3), (256, 5, 3))
SEEDS = (0, 1, 2, 3, 4)
PAIRS = 8
TERM_FLOOR = 0.25                                # every level term of every tolerance pair is at least this, in fp64

# (P, C, S) of the single-level kernel cases: one position (S = 4 with n = 4, S = 8 with n = 8, S = 11 with n = 11), 2 x 2 positions,
# sides around the tile (32 staged pixels; 32 valid positions are S = 42) and past two tiles, and one case at the product's size
KERNEL_CASES = ((1, 1, 4), (5, 3, 4), (1, 3, 8), (1, 3, 11), (5, 1, 11), (1, 4, 12), (5, 3, 12), (1, 3, 16), (5, 4, 16),
                (1, 1, TILE - 1), (5, 3, TILE), (1, 4, TILE + 1), (1, 3, TILE + 9), (5, 1, TILE + 10), (1, 3, TILE + 11),
                (1, 3, 2 * TILE + 3), (2, 4, 2 * TILE + 13), (2, 3, 256))
DOWN_SHAPES = ((1, 2, 2), (3, 4, 6), (5, 16, 16), (2, 34, 62), (6, 256, 256))    # (NC, H, W) of avg_down2

# measure(): the larger of the two fp32 evaluations' errors against fp64 over the tolerance
# cases.  The bounds are 4 x these.
MEASURED = {"map": 1.75e-6, "term": 2.12e-7, "score": 6.98e-8}
TOL_MAP, TOL_TERM, TOL_SCORE = (4 * MEASURED[k] for k in ("map", "term", "score"))

CLAMP_CASE = dict(S=32, L=4, C=3, seed=0)        # independent unsmoothed noise: find_clamp_pair() looks for its pair


def seed_of(what, case):
    return zlib.crc32(("%s %s" % (what, case)).encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- inputs
def smooth_noise(rng, shape):
    """tanh of Gaussian noise, averaged three times over each 2 x 2 cyclic neighbourhood: fp32 in (-1, 1)"""
    x = np.tanh(rng.standard_normal(shape))
    for _ in range(3):
        x = (x + np.roll(x, 1, -1) + np.roll(x, 1, -2) + np.roll(np.roll(x, 1, -1), 1, -2)) / 4
    return x.astype(np.float32)


def smooth_pairs(P, C, S, seed):
    """a = smooth noise, b = 0.5 a + 0.5 (an independent draw of it): two fp32 (P, C, S, S) arrays"""
    rng = np.random.RandomState(seed)
    a = smooth_noise(rng, (P, C, S, S))
    b = (0.5 * a.astype(np.float64) + 0.5 * smooth_noise(rng, (P, C, S, S))).astype(np.float32)
    return a, b


def rough_pairs(P, C, S, seed):
    """independent unsmoothed noise, tanh of a Gaussian: the clamp's input"""
    rng = np.random.RandomState(seed)
    return (np.tanh(rng.standard_normal((P, C, S, S))).astype(np.float32),
            np.tanh(rng.standard_normal((P, C, S, S))).astype(np.float32))


def integer_image(shape, seed, high=256):
    return np.random.RandomState(seed).randint(0, high, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------- the definition
def sides(size, scales):
    return [size >> j for j in range(scales)]


def window(side):
    """the definition's window, written out again: n = min(11, side), sigma = 1.5 n / 11, fp64, rounded once to fp32"""
    n = min(11, side)
    sigma = 1.5 * n / 11
    g = np.array([np.exp(-((k - (n - 1) / 2.0) ** 2) / (2 * sigma * sigma)) for k in range(n)], dtype=np.float64)
    return (g / g.sum()).astype(np.float32)


def avg_down2(x, dtype=np.float64):
    x = x.astype(dtype)
    return (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * dtype(0.25)).astype(dtype)


def _filter(x, g, axis):
    """valid positions along `axis`, the taps added from zero in index order, in x's dtype"""
    m = x.shape[axis] - len(g) + 1
    out = None
    for k in range(len(g)):
        index = [slice(None)] * x.ndim
        index[axis] = slice(k, k + m)
        tap = g[k] * x[tuple(index)]
        out = tap if out is None else out + tap
    assert out.dtype == x.dtype
    return out


def level(a, b, win, dtype=np.float64):
    """One level of the definition for (P, C, S, S) pairs in `dtype` arithmetic: (ssim_map, cs_map) of shape (P, C, M, M) in
    `dtype` and terms (P, 2) fp64 = (mean ssim, mean cs), the means in fp64"""
    g = win.astype(dtype)
    da, db = dtype(127.5) * a.astype(dtype), dtype(127.5) * b.astype(dtype)

    def G(x):
        return _filter(_filter(x, g, -1), g, -2)
    ma, mb = G(da), G(db)
    saa, sbb, sab = G(da * da) - ma * ma, G(db * db) - mb * mb, G(da * db) - ma * mb
    mua, mub = dtype(127.5) + ma, dtype(127.5) + mb
    cs = (dtype(2) * sab + dtype(C2)) / ((saa + sbb) + dtype(C2))
    lum = (dtype(2) * (mua * mub) + dtype(C1)) / ((mua * mua + mub * mub) + dtype(C1))
    ssim = lum * cs
    assert ssim.dtype == dtype and cs.dtype == dtype
    terms = np.stack([ssim.astype(np.float64).mean(axis=(1, 2, 3)), cs.astype(np.float64).mean(axis=(1, 2, 3))], axis=1)
    return ssim, cs, terms


def level_torch(a, b, win):
    """the same formula in torch fp32 with conv2d: (ssim_map, cs_map, terms) as `level` gives them"""
    import torch
    import torch.nn.functional as F
    P, C, S, _ = a.shape
    g = torch.from_numpy(np.array(win))
    kx, ky = g.view(1, 1, 1, -1), g.view(1, 1, -1, 1)

    def G(x):
        return F.conv2d(F.conv2d(x, kx), ky)
    da = 127.5 * torch.from_numpy(np.array(a)).view(P * C, 1, S, S)
    db = 127.5 * torch.from_numpy(np.array(b)).view(P * C, 1, S, S)
    ma, mb = G(da), G(db)
    saa, sbb, sab = G(da * da) - ma * ma, G(db * db) - mb * mb, G(da * db) - ma * mb
    mua, mub = 127.5 + ma, 127.5 + mb
    cs = (2 * sab + C2) / ((saa + sbb) + C2)
    ssim = (2 * (mua * mub) + C1) / ((mua * mua + mub * mub) + C1) * cs
    M = S - len(win) + 1
    ssim, cs = ssim.view(P, C, M, M).numpy(), cs.view(P, C, M, M).numpy()
    assert ssim.dtype == np.float32
    terms = np.stack([ssim.astype(np.float64).mean(axis=(1, 2, 3)), cs.astype(np.float64).mean(axis=(1, 2, 3))], axis=1)
    return ssim, cs, terms


def all_levels(a, b, scales, dtype=np.float64, one_level=level):
    """terms (P, L, 2) fp64 of (P, C, S, S) pairs over `scales` levels, the 2 x 2 mean between them in `dtype`"""
    out = []
    for j, side in enumerate(sides(a.shape[-1], scales)):
        out.append((one_level(a, b, window(side), dtype) if one_level is level else one_level(a, b, window(side)))[2])
        if j + 1 < scales:
            a, b = avg_down2(a, dtype), avg_down2(b, dtype)
    return np.stack(out, axis=1)


def score(terms):
    """the score of terms (..., L, 2), the definition written out per pair: (score, clamped)"""
    t = np.asarray(terms, dtype=np.float64)
    L = t.shape[-2]
    w = np.array(WEIGHTS[:L], dtype=np.float64)
    if L < 5:
        w = w / w.sum()
    flat = t.reshape(-1, L, 2)
    scores, clamped = [], []
    for pair in flat:
        used = [pair[j, 1] for j in range(L - 1)] + [pair[L - 1, 0]]
        clamped.append(any(u < 0 for u in used))
        s = 1.0
        for u, wj in zip(used, w):
            s *= max(u, 0.0) ** wj
        scores.append(s)
    return np.array(scores).reshape(t.shape[:-2]), np.array(clamped).reshape(t.shape[:-2])


# ------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def kernel_case(case):
    """(a, b, win, ssim_map, cs_map, terms) of a single-level case: inputs fp32, the maps and terms of the fp64 oracle; read only"""
    P, C, S = case
    a, b = smooth_pairs(P, C, S, seed_of("kernel", case))
    win = window(S)
    ssim, cs, terms = level(a, b, win)
    for arr in (a, b, win, ssim, cs, terms):
        arr.setflags(write=False)
    return a, b, win, ssim, cs, terms


@functools.lru_cache(maxsize=None)
def tolerance_case(case, seed):
    """(a, b, terms (P, L, 2) fp64, score (P,)) of a tolerance case under one seed; read only"""
    S, L, C = case
    a, b = smooth_pairs(PAIRS, C, S, seed_of("tolerance", case) + seed)
    terms = all_levels(a, b, L)
    sc, clamped = score(terms)
    assert not clamped.any()
    for arr in (a, b, terms, sc):
        arr.setflags(write=False)
    return a, b, terms, sc


def measure(cases=TOLERANCE_CASES, seeds=SEEDS):
    """{"map", "term", "score"}: the larger error against the fp64 oracle of the two fp32 CPU evaluations over the cases, and
    "floor", the smallest fp64 level term met"""
    worst = {"map": 0.0, "term": 0.0, "score": 0.0, "floor": np.inf}
    for case in cases:
        S, L, C = case
        for seed in seeds:
            a, b, terms, sc = tolerance_case(case, seed)
            worst["floor"] = min(worst["floor"], float(terms.min()))
            for one_level, dtype in ((level, np.float32), (level_torch, np.float32)):
                t32 = all_levels(a, b, L, dtype, one_level)
                worst["term"] = max(worst["term"], float(np.abs(t32 - terms).max()))
                worst["score"] = max(worst["score"], float(np.abs(score(t32)[0] - sc).max()))
            # the maps of the finest level (the coarser levels' inputs differ between the evaluations by the 2 x 2 mean's rounding)
            win = window(S)
            ssim, cs, _ = level(a, b, win)
            for got in (level(a, b, win, np.float32), level_torch(a, b, win)):
                worst["map"] = max(worst["map"], float(np.abs(got[0] - ssim).max()), float(np.abs(got[1] - cs).max()))
    return worst


@functools.lru_cache(maxsize=None)
def find_clamp_pair():
    """(a, b, terms (L, 2) fp64) of the first pair of CLAMP_CASE's rough noise with a level mean that enters the score below -0.01"""
    k = CLAMP_CASE
    a, b = rough_pairs(64, k["C"], k["S"], k["seed"])
    terms = all_levels(a, b, k["L"])
    used = np.concatenate([terms[:, :-1, 1], terms[:, -1:, 0]], axis=1)
    j = int(np.argmin(used.min(axis=1)))
    return np.ascontiguousarray(a[j:j + 1]), np.ascontiguousarray(b[j:j + 1]), terms[j]


if __name__ == "__main__":
    print(measure())
    print(find_clamp_pair()[2])
