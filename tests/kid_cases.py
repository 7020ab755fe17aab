"""Shapes, seeded inputs, oracle and measured bounds of the kernel-Inception-distance path (csrc/mogan_mmd.hip, attngan/kid.py),
shared by tests/test_kid_reference_cpu.py (which measures the bounds), tests/test_kid_cpu.py and tests/test_kid_gpu.py (which
apply them).

The three sums of a subset pair, under k(a, b) = (gamma <a, b> + coef0)^3:
    sums[k, 0] = sum_{i != j} k(x_ix[k,i], x_ix[k,j]),  sums[k, 1] = the same of y through iy,  sums[k, 2] = sum_{i,j} k(x_ix[k,i], y_iy[k,j])
(i != j by POSITION in the subset).

Oracle.  The defining formula in numpy.longdouble (64-bit mantissa on x86) from the fp32 inputs widened exactly, with the fp64
gamma and coef0 the entry point is given, widened exactly too.

Error measure.  err = |got - oracle| / A per sum, A the same sum taken over |k| (a sum with cancellation is not judged against
itself); the largest of a subset pair's three, the largest over the subset pairs.

Bound.  SUM_TOL is 4 x the largest err over CASES of two fp64 CPU evaluations (the margin is fid_cases.MOMENT_TOL's): `numpy_fp64`,
the formula in plain numpy, and `restatement`, which follows the kernel's order -- the Gram matrices as rank-4 updates along the
feature axis in index order (one K step of the fp64 MFMA each), t = acc * gamma + coef0, (t * t) * t, 64 x 64 tiles, of xx and yy
only those on and above the diagonal (a diagonal tile keeps i < j) and doubled, the tile sums added in tile order.  MEASURED holds
the figures the CPU module printed; that module holds SUM_TOL to them and to the ceiling 1e-13 (fid_cases.MOMENT_TOL_CEILING).  One
dropped pair at s = 130 weighs about 6e-5 of a sum, eight orders above the ceiling: the bound cannot hide one.

Exact cases.  Integer-valued fp32 inputs in [-4, 4] and gamma a power of two passed explicitly, coef0 = 1: every <a, b> is an
integer of magnitude 16 D at most, gamma <a, b> + 1 is exact and at most 17 in magnitude, its cube is a multiple of 2^-21 below
2^13, and a sum of fewer than 2^15 of them needs 49 bits: every partial sum is exact in fp64 in ANY summation order.  The kernel
must give `exact_expected` (numpy fp64) bit for bit.  A wrong lane map, a dropped tail, a diagonal counted, a tile not doubled or
a lost K step all fail it.

End to end.  KID_E2E_TOL bounds, relative to |sums0| / (s (s - 1)) + |sums1| / (s (s - 1)) + 2 |sums2| / s^2, how far the reported
mean and spread may be from the figure formed in numpy fp64 from the returned codes: 4 x the largest disagreement of a subset
pair's mmd2 between the two fp64 CPU evaluations above at the end-to-end test's size (4 subset pairs of 8 out of 12 codes of 2048
features, four seeds).
"""
import numpy as np

import fid_cases
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import kid as KIDMOD  # noqa: E402

LD = np.longdouble
SUM_TOL_CEILING = fid_cases.MOMENT_TOL_CEILING
CT = 64

# (S, s, D, Nx, Ny) -> seed
CASES = {
    (1, 2, 1, 2, 2): 0,             # the smallest legal problem
    (1, 3, 16, 5, 4): 0,            # Nx != Ny, gather through a permuted (hand-written, unsorted) index
    (2, 5, 17, 9, 9): 0,            # a D tail of 1; two subsets that overlap
    (1, 64, 48, 64, 64): 0,         # exactly one full tile; D not a multiple of 64
    (3, 67, 80, 100, 90): 0,        # an s tail of 3 inside the second tile; off-diagonal tiles of the triangle; three subsets
    (2, 130, 100, 130, 200): 0,     # three tile rows; D not a multiple of 16
    (1, 96, 2048, 96, 96): 0,       # the workload's D, many K steps
}
HAND_INDEX = {(1, 3, 16, 5, 4): (np.array([[4, 0, 2]], dtype=np.int32), np.array([[3, 1, 0]], dtype=np.int32))}
INDEPENDENCE_CASE = (3, 67, 80, 100, 90)
# (S, s, D, Nx, Ny, gamma) -> seed
EXACT_CASES = {(2, 67, 48, 70, 75, 2.0 ** -6): 1, (1, 130, 128, 140, 130, 2.0 ** -7): 1}
# the end-to-end test's size: 4 subset pairs of 8 out of 12 codes in 2048 features
E2E = (4, 8, 2048, 12, 12)
E2E_SEEDS = (0, 1, 2, 3)

# ---- recorded by tests/test_kid_reference_cpu.py (it fails when a figure is exceeded or stale) ----
MEASURED = {"numpy fp64": 2.9e-16, "restatement": 4.4e-16}
SUM_TOL = 1.8e-15
KID_MEASURED = {"e2e": 7.0e-16}
KID_E2E_TOL = 2.8e-15


def make_inputs(case, seed):
    """(x (Nx, D), y (Ny, D)) fp32 as fid_cases.fd_pair draws them: normal draws times a per-column scale in [1/e, e], a shared
    mixing, a per-column offset of up to twice the scale"""
    S, s, D, Nx, Ny = case
    return fid_cases.fd_pair((D, Nx, Ny), seed)


def make_indices(case, seed):
    """(ix, iy) int32 (S, s): the hand-written table of the case that has one, else kid.draw_subsets under the case's seed"""
    if case in HAND_INDEX:
        return HAND_INDEX[case]
    S, s, D, Nx, Ny = case
    return KIDMOD.draw_subsets(Nx, Ny, S, s, seed)


def make_exact_inputs(case, seed):
    """(x, y, ix, iy, gamma): integer-valued fp32 codes in [-4, 4], subsets from kid.draw_subsets"""
    S, s, D, Nx, Ny, gamma = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-4, 5, (Nx, D)).astype(np.float32)
    y = rng.randint(-4, 5, (Ny, D)).astype(np.float32)
    ix, iy = KIDMOD.draw_subsets(Nx, Ny, S, s, seed)
    return x, y, ix, iy, gamma


def _sums_of(kxx, kyy, kxy):
    """the three sums of one subset pair from its three kernel matrices: the diagonals of xx and yy by position left out"""
    off = ~np.eye(kxx.shape[0], dtype=bool)
    return [kxx[off].sum(), kyy[off].sum(), kxy.sum()]


def _formula(x, y, ix, iy, gamma, coef0, dtype):
    """(sums (S, 3), the same sums over |k|) by the defining formula in `dtype`"""
    g, c = dtype(gamma), dtype(coef0)
    sums, mags = [], []
    for rx, ry in zip(ix, iy):
        a, b = x[rx].astype(dtype), y[ry].astype(dtype)
        ks = []
        for p, q in ((a, a), (b, b), (a, b)):
            t = (p @ q.T) * g + c
            ks.append((t * t) * t)
        sums.append(_sums_of(*ks))
        mags.append(_sums_of(*[np.abs(k) for k in ks]))
    return np.array(sums, dtype=dtype), np.array(mags, dtype=dtype)


def oracle(x, y, ix, iy, gamma, coef0=1.0):
    """(sums (S, 3), A (S, 3)) in numpy.longdouble"""
    return _formula(x, y, ix, iy, gamma, coef0, LD)


def numpy_fp64(x, y, ix, iy, gamma, coef0=1.0):
    """sums (S, 3): the defining formula in plain numpy fp64"""
    return _formula(x, y, ix, iy, gamma, coef0, np.float64)[0]


exact_expected = numpy_fp64


def restatement(x, y, ix, iy, gamma, coef0=1.0, kstep=4, tile=CT):
    """sums (S, 3) fp64 in the kernel's order (see the module docstring)"""
    g, c = np.float64(gamma), np.float64(coef0)
    out = []
    for rx, ry in zip(ix, iy):
        a, b = x[rx].astype(np.float64), y[ry].astype(np.float64)
        s, D = a.shape
        T = (s + tile - 1) // tile
        row = []
        for p, q, sym in ((a, a, True), (b, b, True), (a, b, False)):
            acc = np.zeros((s, s))
            for k in range(0, D, kstep):
                acc = acc + p[:, k:k + kstep] @ q[:, k:k + kstep].T
            t = acc * g + c
            v = (t * t) * t
            if sym:
                v = np.triu(v, 1)                                 # i < j only; whole tiles below the diagonal are skipped below
            total = np.float64(0.0)
            for bi in range(T):
                for bj in range(bi if sym else 0, T):
                    part = v[bi * tile:(bi + 1) * tile, bj * tile:(bj + 1) * tile].sum()
                    total = total + (part + part if sym else part)
            row.append(total)
        out.append(row)
    return np.array(out, dtype=np.float64)


def sum_error(got, ref, mag):
    """the largest |got - oracle| / A over the three sums of every subset pair"""
    return float((np.abs(np.asarray(got, LD) - ref) / mag).max())


def mmd2_scale(sums, s):
    """|sums0| / (s (s - 1)) + |sums1| / (s (s - 1)) + 2 |sums2| / s^2 per subset pair: what KID_E2E_TOL is relative to"""
    a = np.abs(np.asarray(sums, dtype=np.float64))
    return a[:, 0] / (s * (s - 1.0)) + a[:, 1] / (s * (s - 1.0)) + 2.0 * a[:, 2] / (float(s) * s)


def gamma_of(case):
    return 1.0 / case[2]


_REF = {}


def reference(case):
    """inputs, index tables and longdouble oracle of a case, computed once and shared: {"x", "y", "ix", "iy", "gamma", "sums", "mag"}"""
    if case not in _REF:
        x, y = make_inputs(case, CASES[case])
        ix, iy = make_indices(case, CASES[case])
        gamma = gamma_of(case)
        sums, mag = oracle(x, y, ix, iy, gamma)
        for a in (x, y, ix, iy):
            a.setflags(write=False)
        _REF[case] = {"x": x, "y": y, "ix": ix, "iy": iy, "gamma": gamma, "sums": sums, "mag": mag}
    return _REF[case]
