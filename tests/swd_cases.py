"""The cases, seeds, oracle and bounds of the sliced Wasserstein tests (tests/test_swd_reference_cpu.py, test_swd_gpu.py; DESIGN.md
section 9g).  The oracle is plain numpy -- the index rules of attngan/swd.py's docstring written out a second time, directly, one
tap at a time -- and knows nothing of the code under test.  No bound here comes from the code under test:

  pyramid      per element 25 * 2^-24 * sum |w_i x_i| over that element's taps (25 taps, fewer than 25 roundings touch any one of
               them in a separable or a direct fp32 evaluation), plus one rounding of the subtraction for the residual;
  exact cases  integer images 0..255: one pyr_down step and one lap_residual step from the oracle's own `down` are exact in fp32 in
               any summation order (every weight is k / 256, every partial sum a multiple of 2^-8 below 2^8, resp. 2^-14 below
               2^9); a two-deep chain is exact for images of 0 / 1 only.  The CPU module shows it: fp32 and fp64 oracle agree
               bit for bit;
  moments      fp64 sums of n = rows * 49 terms in any order: n * 2^-53 relative to the sum of the terms' magnitudes, carried
               through to mean and standard deviation (moments_bounds);
  projections  the largest deviation of numpy's fp32 matmul from the fp64 oracle on the case, times 4 (projection_bound);
  absdiff      fp64 sum of `rows` exact terms: rows * 2^-53 * sum |a - b|; dyadic inputs are exact;
  whole score  2 * the case's projection bound * 1000 per level (the figure is a mean of absolute differences of projections).
"""
import numpy as np

LD = np.longdouble
W5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
U32, U64 = 2.0 ** -24, 2.0 ** -53
TAPS = 25

PYRAMID_SHAPES = [(1, 4, 4), (3, 16, 8), (2, 8, 32), (6, 16, 16)]           # (N C, H, W)
GATHER_CASES = [(1, 7, 1), (3, 7, 1), (1, 16, 130), (3, 16, 130), (3, 16, 1), (1, 7, 130)]      # (C, size, R)
MOMENT_CASES = [(rows, C) for rows in (1, 257, 4099) for C in (1, 3)]
PROJECT_CASES = [(1, 1, 1), (63, 3, 5), (65, 1, 128), (130, 3, 130)]        # (rows, C, D)
ABSDIFF_CASES = [(rows, D) for rows in (1, 255, 4097) for D in (1, 3)]
SCORE_CASES = [1, 3]                                                        # channels; 16 images of 32 x 32, levels 32 and 16
SCORE = dict(images=16, size=32, patches=8, dirs=16, repeats=2, min_res=16, seed=1234)
CHANNEL_MEANS = (-40.0, 3.0, 55.0)           # far apart: a standardisation that is off by one channel cannot pass


def seed_of(*key):
    import zlib
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def mirror(i, n):
    """the index rule: the edge sample is not repeated"""
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


# ------------------------------------------------------------------------------------------------------------ pyramid
def pyr_down(x, dtype=np.float64):
    """x (N C, H, W) -> (N C, H / 2, W / 2), one tap at a time, all arithmetic in `dtype`"""
    x = np.asarray(x).astype(dtype)
    NC, H, W = x.shape
    w = W5.astype(dtype)
    out = np.zeros((NC, H // 2, W // 2), dtype=dtype)
    for oy in range(H // 2):
        for ox in range(W // 2):
            s = np.zeros(NC, dtype=dtype)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    s = s + (w[dy + 2] * w[dx + 2]) * x[:, mirror(2 * oy + dy, H), mirror(2 * ox + dx, W)]
            out[:, oy, ox] = s
    return out


def pyr_up(d, dtype=np.float64):
    """d (N C, h, w) -> (N C, 2h, 2w): the same filter times 4 over the zero-inserted image, which IS formed here"""
    d = np.asarray(d).astype(dtype)
    NC, h, w_ = d.shape
    H, W = 2 * h, 2 * w_
    z = np.zeros((NC, H, W), dtype=dtype)
    z[:, ::2, ::2] = d
    w = W5.astype(dtype)
    out = np.zeros((NC, H, W), dtype=dtype)
    for y in range(H):
        for x in range(W):
            s = np.zeros(NC, dtype=dtype)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    s = s + (w[dy + 2] * w[dx + 2]) * z[:, mirror(y + dy, H), mirror(x + dx, W)]
            out[:, y, x] = dtype(4.0) * s
    return out


def lap_residual(x, down, dtype=np.float64):
    return np.asarray(x).astype(dtype) - pyr_up(down, dtype)


def down_bound(x):
    """per output element: 25 * 2^-24 * sum |w_i x_i|"""
    return TAPS * U32 * pyr_down(np.abs(np.asarray(x, dtype=np.float64)))


def residual_bound(x, down):
    """per element: the filter's bound on pyr_up plus one rounding of the subtraction"""
    up = TAPS * U32 * pyr_up(np.abs(np.asarray(down, dtype=np.float64)))
    return up + U32 * (np.abs(lap_residual(x, down)) + up)


def laplacian_levels(img, sizes, dtype=np.float64):
    """(B, C, S, S) -> the levels of `sizes`, finest first, each (B, C, s, s)"""
    B, C = img.shape[:2]
    g = np.asarray(img).astype(dtype).reshape(B * C, sizes[0], sizes[0])
    out = []
    for s in sizes[:-1]:
        d = pyr_down(g, dtype)
        out.append(lap_residual(g, d, dtype).reshape(B, C, s, s))
        g = d
    out.append(g.reshape(B, C, sizes[-1], sizes[-1]))
    return out


def integer_image(shape, seed, high=256):
    return np.random.RandomState(seed).randint(0, high, size=shape).astype(np.float32)


def gaussian_image(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


# -------------------------------------------------------------------------------------------------------- descriptors
def descriptors(level, centres):
    """level (N, C, H, W), centres (R, 3) = (image, cy, cx) -> (R, C 49) in (channel, y, x) order"""
    level = np.asarray(level)
    out = np.empty((len(centres), level.shape[1] * 49), dtype=level.dtype)
    for r, (n, cy, cx) in enumerate(np.asarray(centres)):
        out[r] = level[n, :, cy - 3:cy + 4, cx - 3:cx + 4].reshape(-1)
    return out


def gather_centres(N, size, R, seed):
    """R triples that include the four corners of the legal range (where there is more than one legal centre)"""
    rng = np.random.RandomState(seed)
    lo, hi = 3, size - 4
    c = np.stack([rng.randint(0, N, R), rng.randint(lo, hi + 1, R), rng.randint(lo, hi + 1, R)], axis=1).astype(np.int32)
    corners = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    for i, (cy, cx) in enumerate(corners[:R]):
        c[(i * 37) % R, 1:] = (cy, cx)
    if R >= 4:
        rows = {(i * 37) % R for i in range(4)}
        assert len(rows) == 4
    return c


# ------------------------------------------------------------------------------------------------------------ moments
def moment_inputs(rows, C, seed):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((rows, C, 49))
    x = x * np.array([0.5, 3.0, 20.0, 1.0])[:C, None] + np.array(CHANNEL_MEANS + (0.0,))[:C, None]
    return np.ascontiguousarray(x.reshape(rows, C * 49).astype(np.float32))


def moments(desc, C):
    """(C, 2) longdouble: mean and population standard deviation per channel"""
    x = np.asarray(desc).astype(LD).reshape(desc.shape[0], C, 49)
    mean = x.sum(axis=(0, 2)) / LD(desc.shape[0] * 49)
    var = ((x - mean[None, :, None]) ** 2).sum(axis=(0, 2)) / LD(desc.shape[0] * 49)
    return np.stack([mean, np.sqrt(var)], axis=1)


def moments_bounds(desc, C):
    """(C, 2) float64 bounds on |mean - oracle| and |std - oracle| for fp64 sums of n terms in any order, each sum within
    n 2^-53 of the sum of its terms' magnitudes:
      mean:  dm = (n + 1) u sum|x| / n                                        (the sum, one division)
      std:   S' = sum (x - m')^2 = S + n dm'^2 for the computed mean m' (exactly), every term carries 3 roundings (the difference, the
             square, its entry into the sum) and the sum n more: |S_computed - S| <= n dm^2 + (n + 3) u (S + n dm^2); the
             variance adds one division, the root one rounding, and d sqrt(v) = dv / (2 sqrt(v)) -- for S > 0; a constant channel has
             S = 0 and dm = 0 where its value is exactly representable in the partial sums, which the test chooses."""
    n = desc.shape[0] * 49
    x = np.asarray(desc).astype(LD).reshape(desc.shape[0], C, 49)
    ref = moments(desc, C)
    out = np.zeros((C, 2))
    for c in range(C):
        dm = (n + 1) * U64 * float(np.abs(x[:, c]).sum()) / n
        S = float(((x[:, c] - ref[c, 0]) ** 2).sum())
        dS = n * dm * dm + (n + 3) * U64 * (S + n * dm * dm)
        std = float(ref[c, 1])
        dvar = dS / n + U64 * (S + dS) / n
        out[c, 0] = dm
        out[c, 1] = (dvar / (2 * std) + 2 * U64 * std) if std > 0 else 0.0
    return out


# -------------------------------------------------------------------------------------------------------- projections
def standardise(desc, mom):
    """the once-rounded fp32 values the projection multiplies: float32((float64(v) - mean) / std), mom (C, 2) fp64"""
    C = mom.shape[0]
    x = np.asarray(desc, dtype=np.float64).reshape(desc.shape[0], C, 49)
    z = (x - mom[None, :, 0, None]) / mom[None, :, 1, None]
    return np.ascontiguousarray(z.reshape(desc.shape[0], C * 49).astype(np.float32))


def projections(desc, mom, dirs):
    """(D, rows) fp64 from the once-rounded fp32 standardised values"""
    return np.ascontiguousarray((standardise(desc, mom).astype(np.float64) @ np.asarray(dirs, dtype=np.float64)).T)


def numpy_fp32_deviation(desc, mom, dirs):
    """the largest deviation of numpy's fp32 matmul from the fp64 oracle: the reference arithmetic's own error on the case"""
    z = standardise(desc, mom)
    got = (z @ np.asarray(dirs, dtype=np.float32)).T.astype(np.float64)
    return float(np.abs(got - projections(desc, mom, dirs)).max())


def projection_bound(desc, mom, dirs):
    """4 x numpy's own deviation: the factor allows for another summation order and for the split product dropping its lowest cross
    terms (csrc/mogan_mma.h)"""
    return 4.0 * numpy_fp32_deviation(desc, mom, dirs)


def unit_directions(K, D, seed):
    d = np.random.RandomState(seed).randn(K, D)
    d = d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    return np.ascontiguousarray(d.astype(np.float32))


def project_inputs(case):
    """(desc, moments fp64, dirs) of a PROJECT_CASES entry; the moments are the oracle's own, rounded to fp64"""
    rows, C, D = case
    desc = moment_inputs(rows, C, seed_of("project", case))
    if rows == 1:                                            # one row: 49 values per channel still have a spread
        assert (moments(desc, C)[:, 1] > 0).all()
    mom = moments(desc, C).astype(np.float64)
    return desc, np.ascontiguousarray(mom), unit_directions(49 * C, D, seed_of("dirs", case))


# ------------------------------------------------------------------------------------------------------------ absdiff
def absdiff_inputs(rows, D, seed, dyadic):
    rng = np.random.RandomState(seed)
    if dyadic:                                               # multiples of 1/8 below 64: every |a - b| and every partial sum is exact
        return (rng.randint(-512, 512, (D, rows)) / 8.0).astype(np.float32), (rng.randint(-512, 512, (D, rows)) / 8.0).astype(np.float32)
    return rng.standard_normal((D, rows)).astype(np.float32), (rng.standard_normal((D, rows)) * 3 + 1).astype(np.float32)


def absdiff(a, b):
    return np.abs(np.asarray(a).astype(LD) - np.asarray(b).astype(LD)).sum(axis=1)


def absdiff_bound(a, b):
    return a.shape[1] * U64 * absdiff(a, b).astype(np.float64)


# -------------------------------------------------------------------------------------------------------- the whole score
def score_images(C, seed):
    """16 integer images 0..255 of 32 x 32 per side (so that both pyramid levels are exact in fp32 and the oracle's descriptors are
    the device's bit for bit); the generated side is drawn from another distribution"""
    n, s = SCORE["images"], SCORE["size"]
    rng = np.random.RandomState(seed)
    real = rng.randint(0, 256, (n, C, s, s)).astype(np.float32)
    fake = np.clip(np.round(rng.standard_normal((n, C, s, s)) * 40 + 128), 0, 255).astype(np.float32)
    return real, fake


def score_oracle(real, fake, centres, directions, sizes):
    """per level: the figure in fp64 and the level's projection bound (the largest over sides and repeats).
    centres: {"real": [per level (R, 3)], "fake": [...]}; directions: [per level [per repeat (K, D) fp32]]"""
    C = real.shape[1]
    lv = {"real": laplacian_levels(real, sizes), "fake": laplacian_levels(fake, sizes)}
    figures, bounds = [], []
    for li in range(len(sizes)):
        desc, mom = {}, {}
        for side in ("real", "fake"):
            desc[side] = descriptors(lv[side][li], centres[side][li]).astype(np.float32)
            assert (desc[side] == descriptors(lv[side][li], centres[side][li])).all()        # the levels are fp32-exact
            mom[side] = np.ascontiguousarray(moments(desc[side], C).astype(np.float64))
        per_repeat, bound = [], 0.0
        for d in directions[li]:
            pr = np.sort(projections(desc["real"], mom["real"], d), axis=1)
            pf = np.sort(projections(desc["fake"], mom["fake"], d), axis=1)
            per_repeat.append(float(np.abs(pr - pf).mean()))
            bound = max(bound, projection_bound(desc["real"], mom["real"], d), projection_bound(desc["fake"], mom["fake"], d))
        figures.append(float(np.mean(per_repeat)) * 1000.0)
        bounds.append(2.0 * bound * 1000.0)
    return figures, bounds
