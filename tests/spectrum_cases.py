"""The oracle, cases, seeds and bounds of the radial-power-spectrum tests (tests/test_spectrum_cpu.py, test_spectrum_reference_cpu.py,
test_spectrum_rejections_cpu.py, test_spectrum_gpu.py): a plain helper module.  It shares nothing with the code under test but what
the definition makes an INPUT of the kernel: the fp32 weights and window, and the table of bins (which test_spectrum_cpu.py holds to
a brute-force table written here).

The oracle (`sums`) is the definition of attngan/spectrum.py in numpy fp64 on numpy.fft.fft2 over the FULL plane: a half-plane
table is unfolded by (u, v) -> (-u, -v) and every frequency is added once.  It is not the kernel's formulation (half plane with
multiplicities, radix-2 in two passes).

The bound does not come from the code under test.  Every case's sums are formed a second time on the CPU by a direct DFT, the
matrix product with exp(-2 pi i u k / S) in numpy.longdouble (`sums_direct`).  Per bin the bound is
    MULTIPLE x max(|sums - sums_direct|, eps_fp64 log2(S^2) total),   total = sum over the plane of |F|^2
-- the second term is the error scale of a power-of-two transform of N = S^2 points in fp64 (relative error of a coefficient
~ eps log2 N against the rms coefficient, see e.g. Van Loan, "Computational Frameworks for the FFT", 1992, section 1.4; |F|^2 then
moves by twice that, and a bin's members add up to no more than the total).  MEASURED_SPREAD is the largest |sums - sums_direct| over
all cases and bins in units of eps log2(S^2) total, as `measure()` gives it on the CPU these tests were written on (python
tests/spectrum_cases.py prints it); test_spectrum_reference_cpu.py measures again and holds the record to it.  The two references
differ by well under one unit, so the second term decides nearly every bound; MULTIPLE = 4 leaves the usual factor (DESIGN.md
section 9c: 4 x the reference's own error) for a transform that adds in another order."""
import functools
import zlib

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MULTIPLE = 4.0
MEASURED_SPREAD = 0.149                       # max |sums - sums_direct| / (eps log2(S^2) total) over CASES: measure() gave 0.1481

LUMA = (0.299, 0.587, 0.114)
WINDOWS = ("hann", "none")
# (S, B): 8 and 32 have an odd number of radix-2 stages, 8 is the smallest side; 16 and 64 an even number; one case at the product's
# size; B = 1, 3 and 5 images (several workgroups in every launch).  Each runs at C = 1 and C = 3, with and without the window.
SHAPES = ((8, 1), (8, 5), (16, 3), (32, 5), (64, 3), (256, 2))
CASES = tuple((S, B, C, w) for S, B in SHAPES for C in (1, 3) for w in WINDOWS)
KINDS = ("normal", "checker_on_ramp", "cosine", "impulse", "constant")          # image b of a case is KINDS[b]
CHECKER = 1e-3                                # amplitude of the period-2 checkerboard of the dynamic-range image: its bin holds
                                              # (CHECKER / mean)^2 = 2.6e-6 of bin 0's power, and 1e-8 of it is the bound there
GAINS = (1.0, 0.5, -0.25)                     # how a pattern enters the three channels


def seed_of(what, case):
    return zlib.crc32(("%s %s" % (what, case)).encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- the definition, written again
def weights(C):
    return np.asarray(LUMA if C == 3 else (1.0,) * C, dtype=np.float32)


def hann(S):
    i = np.arange(S, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / S)).astype(np.float32)


def window(name, S):
    return hann(S) if name == "hann" else None


def signed(S):
    u = np.arange(S)
    return np.where(u <= S // 2, u, u - S)


def full_table(S):
    """bin(u, v) over the full plane by brute force: floor(sqrt(fu^2 + fv^2) + 1 / 2) in float64.  sqrt(n) is never a half-integer
    for an integer n, and for n <= 2 128^2 it stays 7e-4 away from one: the rounding cannot go wrong."""
    f = signed(S).astype(np.float64)
    return np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(np.int64)


def unfold(half, S):
    """the full-plane (S, S) table of a half-plane (S, S / 2 + 1) one: entry (u, v) for v > S / 2 is the half plane's (-u, -v)"""
    half = np.asarray(half, dtype=np.int64)
    full = np.empty((S, S), dtype=np.int64)
    full[:, :S // 2 + 1] = half
    u = (-np.arange(S)) % S
    for v in range(S // 2 + 1, S):
        full[:, v] = half[u, S - v]
    return full


def plane(x, weight, win):
    """(B, S, S) fp64: the weighted sum over the channels (ascending), times the window"""
    x = np.asarray(x)
    y = np.zeros((x.shape[0],) + x.shape[2:], dtype=np.float64)
    for c in range(x.shape[1]):
        y += np.float64(weight[c]) * x[:, c].astype(np.float64)
    if win is not None:
        w = np.asarray(win, dtype=np.float64)
        y = y * (w[:, None] * w[None, :])
    return y


def bin_sums(power, full, n_bins):
    """(B, n_bins): the full plane's |F|^2 added per bin; entries outside [0, n_bins) are left out"""
    keep = (full >= 0) & (full < n_bins)
    return np.stack([np.bincount(full[keep], weights=p[keep], minlength=n_bins) for p in power])


def sums(x, weight, win, half=None, n_bins=None):
    """The oracle: (B, n_bins) fp64 sums of |F|^2 per bin over the full plane, numpy.fft.fft2"""
    S = x.shape[-1]
    full = full_table(S) if half is None else unfold(half, S)
    n_bins = int(full.max()) + 1 if n_bins is None else n_bins
    F = np.fft.fft2(plane(x, weight, win))
    return bin_sums(F.real ** 2 + F.imag ** 2, full, n_bins)


@functools.lru_cache(maxsize=None)
def dft_matrix(S):
    """(cos, -sin)(2 pi (u k mod S) / S) in longdouble"""
    pi = 4 * np.arctan(np.longdouble(1))
    m = (np.arange(S)[:, None] * np.arange(S)[None, :]) % S
    ang = 2 * pi * m.astype(np.longdouble) / np.longdouble(S)
    return np.cos(ang), -np.sin(ang)


def sums_direct(x, weight, win, half=None, n_bins=None):
    """The second reference: the same sums from F = M y M^T in longdouble, M the DFT matrix; returned in fp64"""
    S = x.shape[-1]
    full = full_table(S) if half is None else unfold(half, S)
    n_bins = int(full.max()) + 1 if n_bins is None else n_bins
    mr, mi = dft_matrix(S)
    out = []
    for y in plane(x, weight, win).astype(np.longdouble):
        ar, ai = mr @ y, mi @ y                                             # rows: (Mr + i Mi) y
        fr, fi = ar @ mr.T - ai @ mi.T, ar @ mi.T + ai @ mr.T               # ... (Mr + i Mi)^T
        p = fr * fr + fi * fi
        keep = (full >= 0) & (full < n_bins)
        s = np.zeros(n_bins, dtype=np.longdouble)
        np.add.at(s, full[keep], p[keep])
        out.append(s.astype(np.float64))
    return np.stack(out)


def total_power(x, weight, win):
    """sum over the plane of |F|^2 = S^2 sum (w y)^2 per image (Parseval)"""
    y = plane(x, weight, win)
    return float(x.shape[-1]) ** 2 * (y * y).sum(axis=(1, 2))


def unit(x, weight, win):
    """eps log2(S^2) total per image: what the spread and the bound are counted in"""
    return EPS * np.log2(float(x.shape[-1]) ** 2) * total_power(x, weight, win)


def bound(want, direct, x, weight, win):
    """(B, n_bins): MULTIPLE x max(|want - direct|, eps log2(S^2) total)"""
    return MULTIPLE * np.maximum(np.abs(want - direct), unit(x, weight, win)[:, None])


def count_of(S):
    full = full_table(S)
    return np.bincount(full.ravel(), minlength=int(full.max()) + 1)


def energy(win, S):
    if win is None:
        return float(S) ** 2
    w = np.asarray(win, dtype=np.float64)
    return float((w * w).sum() ** 2)


def profile(x, weight, win):
    """p (B, n_bins): the definition's per-image profile"""
    S = x.shape[-1]
    return sums(x, weight, win) / (count_of(S) * energy(win, S))


def figures(P_real, P_fake, count, S):
    """the figures of the definition, written again on plain numpy (None where no bin holds power)"""
    pr, pf = np.asarray(P_real, np.float64), np.asarray(P_fake, np.float64)
    ok = (pr > 0) & (pf > 0)
    k = np.arange(len(pr))
    use = ok & (k >= 1)
    with np.errstate(divide="ignore"):
        db_r, db_f = 10 * np.log10(pr), 10 * np.log10(pf)
    d = db_f - db_r
    hi = use & (k > S // 4)
    lo = use & (k <= S // 2)
    at = int(k[use][np.argmax(np.abs(d[use]))])
    return {"lsd_db": float(np.sqrt(np.mean(d[use] ** 2))),
            "hf_db": float(10 * np.log10((count[hi] * pf[hi]).sum() / (count[hi] * pr[hi]).sum())),
            "slope_real": float(np.polyfit(np.log10(k[lo]), db_r[lo], 1)[0]),
            "slope_fake": float(np.polyfit(np.log10(k[lo]), db_f[lo], 1)[0]),
            "peak": {"bin": at, "excess_db": float(d[at]), "period": float(S) / at},
            "empty_bins": [int(i) for i in k[~ok]]}


# ------------------------------------------------------------------------------------------------- inputs
def cosine(S, a, b):
    i = np.arange(S)
    return np.cos(2.0 * np.pi * ((a * i[:, None] + b * i[None, :]) % S) / S)


def pattern(kind, S, rng):
    """one (S, S) fp64 pattern in [-1, 1]"""
    i = np.arange(S)
    if kind == "normal":
        return np.clip(rng.standard_normal((S, S)) * 0.4, -1, 1)
    if kind == "checker_on_ramp":        # eight decades between bin 0 and the last bin, where the checkerboard lives
        ramp = 0.4 + 0.3 * (i[:, None] + 0.5 * i[None, :]) / S
        return ramp + CHECKER * (1 - 2 * ((i[:, None] + i[None, :]) % 2))
    if kind == "cosine":
        return 0.75 * cosine(S, int(rng.randint(1, S // 2)), int(rng.randint(0, S)))
    if kind == "impulse":
        x = np.zeros((S, S))
        x[int(rng.randint(1, S)), int(rng.randint(1, S))] = 1.0           # (not where the Hann window is zero)
        return x
    if kind == "constant":
        return np.full((S, S), 0.625)
    raise KeyError(kind)


def images(patterns, C, rng=None):
    """(B, C, S, S) fp32 from B patterns: channel c holds GAINS[c] times the pattern"""
    p = np.asarray(patterns, dtype=np.float64)
    return np.ascontiguousarray(np.stack([GAINS[c] * p for c in range(C)], axis=1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(key):
    """(x, weight, window) of a case (S, B, C, window name): image b is KINDS[b]"""
    S, B, C, w = key
    rng = np.random.RandomState(seed_of("case", key))
    x = images([pattern(KINDS[b], S, rng) for b in range(B)], C)
    if C == 3:                           # the normal image: three independent channels
        x[0] = np.clip(rng.standard_normal((3, S, S)) * 0.4, -1, 1).astype(np.float32)
    x.setflags(write=False)
    return x, weights(C), window(w, S)


@functools.lru_cache(maxsize=None)
def references(key):
    """(sums, sums_direct) of a case: computed once per process and shared"""
    x, weight, win = case(key)
    pair = sums(x, weight, win), sums_direct(x, weight, win)
    for a in pair:
        a.setflags(write=False)
    return pair


def expected(key):
    """(want, bound) of a case, both (B, n_bins)"""
    x, weight, win = case(key)
    want, direct = references(key)
    return want, bound(want, direct, x, weight, win)


def spread(key):
    """max over bins and images of |sums - sums_direct| in units of eps log2(S^2) total"""
    x, weight, win = case(key)
    want, direct = references(key)
    return float((np.abs(want - direct) / unit(x, weight, win)[:, None]).max())


def measure(cases=CASES):
    return max(spread(k) for k in cases)


# the analytic images, no window: (name, pattern builder, the one populated bin and its value as functions of S)
def analytic(S, C):
    """x (N, C, S, S), and per image (name, bin or None for 'every bin equal', value): without a window
      impulse       |F|^2 = 1 everywhere: p equal in every bin, sums[k] = count[k] g^2
      constant c    bin 0 alone, (c g S^2)^2
      cosine (a, b) bin(a, b) alone, S^4 / 2 times g^2 -- S^4 g^2 where (a, b) is its own mirror image, (S/2, 0), (0, S/2) and
                    (S/2, S/2): there cos^2 = 1 everywhere and the single member carries the whole S^2 sum y^2 = S^4
    g = the plane's gain, sum_c weight[c] GAINS[c].  The last entry of a row says whether the fp32 image IS the pattern (values 0,
    0.5, +-1 times the gains): then the analytic value holds to the fp64 bound alone.  A general cosine is rounded to fp32 on its
    way in, every sample by at most 2^-24 of itself: F at the line moves by at most 2^-24 sum |y| <= 2^-24 S^2 against S^2 / 2, the
    power there by at most 2^-22 of itself (ANALYTIC_REL = 2^-21 leaves a factor two), and what the rounding spreads over the
    other bins is at most S^2 sum (2^-24 y)^2 <= 2^-48 S^4 g'^2 in all, g' = sum_c |weight[c] GAINS[c]| (ANALYTIC_LEAK)."""
    h = S // 2
    freqs = ((1, 2), (3, S - 1), (h - 1, h), (h, 0), (0, h), (h, h), (0, 1))
    x0 = np.zeros((S, S))
    x0[3, 5] = 1.0
    pats = [x0, np.full((S, S), 0.5)] + [cosine(S, a, b) for a, b in freqs]
    full = full_table(S)
    g = float(sum(np.float64(w) * np.float64(np.float32(GAINS[c])) for c, w in enumerate(weights(C))))
    rows = [("impulse", None, g * g, True), ("constant", 0, (0.5 * g * S * S) ** 2, True)]
    for a, b in freqs:
        own_mirror = (2 * a) % S == 0 and (2 * b) % S == 0
        rows.append(("cosine %s" % ((a, b),), int(full[a, b]), g * g * float(S) ** 4 * (1.0 if own_mirror else 0.5), own_mirror))
    return images(pats, C), rows


ANALYTIC_REL = 2.0 ** -21


def analytic_leak(S, C):
    gp = float(sum(abs(np.float64(w) * GAINS[c]) for c, w in enumerate(weights(C))))
    return 2.0 ** -48 * float(S) ** 4 * gp * gp


def analytic_check(got, S, C):
    """holds (N, n_bins) sums of analytic(S, C)'s images, no window, to their analytic values; returns the worst miss in units of
    its tolerance for the record"""
    x, rows = analytic(S, C)
    count = count_of(S)
    fp64 = MULTIPLE * unit(x, weights(C), None)
    worst = 0.0
    for b, (name, at, value, exact) in enumerate(rows):
        want = value * count if at is None else np.where(np.arange(len(count)) == at, value, 0.0)
        tol = np.full(len(count), fp64[b]) + (0.0 if exact else analytic_leak(S, C))
        if at is not None and not exact:
            tol[at] = fp64[b] + ANALYTIC_REL * value
        miss = np.abs(got[b] - want) / tol
        assert (miss <= 1.0).all(), "%s at S = %d, C = %d: bin %d off by %.3e, allowed %.3e" % (
            name, S, C, int(miss.argmax()), np.abs(got[b] - want)[miss.argmax()], tol[miss.argmax()])
        worst = max(worst, float(miss.max()))
    return worst


def custom_table(S):
    """a half-plane table that is NOT the radial one: the radial bins with a -1 region (fv above S / 4) and, used with a smaller
    n_bins, entries at or above it: (table int32 (S, S / 2 + 1), n_bins)"""
    half = full_table(S)[:, :S // 2 + 1].astype(np.int32)
    half[:, S // 4 + 1:] = -1
    return np.ascontiguousarray(half), S // 4 + 2


if __name__ == "__main__":
    for k in CASES:
        print(k, "%.4f" % spread(k))
    print("MEASURED_SPREAD", measure())
