"""Shapes, seeded inputs, oracles and measured bounds of the Frechet-distance path (csrc/mogan_stats.hip, attngan/fid.py), shared by
tests/test_fid_reference_cpu.py (which measures the bounds), tests/test_fid_cpu.py and tests/test_fid_gpu.py (which apply them).

Oracle of the moments.  numpy.mean / numpy.cov(rowvar=False) on the fp32 inputs widened to numpy.longdouble (64-bit mantissa on
x86): every fp32 input is exact there and the result carries about 11 bits more than fp64.

Bound of the moments.  err = max |got - oracle| / max |oracle|, for the mean and for the covariance separately, the larger of the
two.  MOMENT_TOL is 4 x the largest err over CASES of two fp64 CPU evaluations (the margin is conv_cases.TOL's and
retrieval_cases.TOL's): numpy.mean / numpy.cov in fp64, and `restatement`, which follows the kernels' order -- the mean as 16 strided
row groups added in group order, the Gram matrix as rank-4 updates in index order (one K step of the fp64 MFMA each), a true division
at the end.  MEASURED holds the figures the CPU module printed; that module holds MOMENT_TOL to them and to the ceiling 1e-13.

Exact cases.  Integer-valued fp32 inputs in [-8, 8] with ONE row adjusted (it may leave [-8, 8], it stays an integer) so that every
column sum is a multiple of N: the mean is an integer, the centred values are integers, every partial sum of the Gram matrix is an
integer far below 2^53 -- exact in fp64 in ANY summation order -- and the division by N - 1 is the one rounding.  The kernels must
give `exact_expected` bit for bit: the defining formula G / (N - 1) in numpy fp64.  (numpy.cov itself ends with a multiplication by
the rounded reciprocal 1 / (N - 1), two roundings, and is off that by one unit in the last place on part of the elements; the CPU
module shows it.  The entry point is specified with the division.)  A wrong lane map, a dropped tail row, a lost K step or a
reciprocal all fail it.

Bound of the distance.  FD_TOL: relative disagreement of fid.frechet_distance with the textbook route
Tr scipy.linalg.sqrtm(S1 S2) on full-rank pairs (both sets N > D), 4 x the largest measured, ceiling 1e-10.  FD_SELF_TOL: the
self-distance of a full-rank set relative to 2 Tr S (it is not 0: Tr S and Tr (S S)^(1/2) are computed differently).  Both figures
are a few roundings of threaded eigen-solvers and differ from run to run (1.3e-15 ... 1.5e-15 and 1.6e-15 ... 1.9e-15 over two
dozen runs, three seeds per case, thread counts 1 ... 32): FD_MEASURED records the largest seen.  A
rank-deficient pair is NOT judged against sqrtm (the error is sqrtm's: FD_RANK_DEFICIENT_VS_SQRTM records it); for the end-to-end test
FD_E2E_TOL bounds, relative to Tr S1 + Tr S2, how far the distance moves when rank-deficient covariances of that test's size are
exchanged for another valid fp64 evaluation of the same covariances (numpy.cov against the rounded oracle and the kernels'
restatement).  That figure is ill-conditioned by construction -- noise eigenvalues of the order 1e-16 Tr S enter through a square
root -- and moved between 3.4e-10 and 5.8e-10 with the BLAS thread count; FD_MEASURED["e2e"] records twice the largest seen.
"""
import numpy as np

LD = np.longdouble
MOMENT_TOL_CEILING = 1e-13
FD_TOL_CEILING = 1e-10

# (N, D) -> seed
CASES = {
    (2, 1): 0,            # the smallest legal shape
    (3, 16): 0,           # an N tail of 3
    (5, 17): 0,           # an N tail and a D tail of 1
    (64, 48): 0,          # D not a multiple of 64
    (67, 80): 0,          # an N tail and a D tail inside a 64-tile
    (130, 100): 0,        # D not a multiple of 16
    (1031, 64): 0,        # many K steps, N prime
    (96, 2048): 0,        # the workload's D, enough K for every tile of the triangle
}
EXACT_CASES = {(67, 80): 1, (1031, 64): 1}

# full-rank pairs of the distance bound: (D, N1, N2) -> seed
FD_CASES = {(16, 40, 50): 0, (64, 200, 300): 0, (100, 150, 130): 0, (256, 2000, 1500): 0}
FD_RANK_DEFICIENT = (64, 20, 30)
# the end-to-end test's size: 12 images in 2048 features, both sets
FD_E2E = (2048, 12, 12)

# ---- recorded by tests/test_fid_reference_cpu.py (it fails when a figure is exceeded or stale) ----
MEASURED = {"numpy fp64": 6.3e-16, "restatement": 4.9e-16}
MOMENT_TOL = 2.6e-15
FD_MEASURED = {"vs sqrtm": 1.6e-15, "self": 1.9e-15, "e2e": 1.2e-9}
FD_TOL = 6.4e-15
FD_SELF_TOL = 7.6e-15
FD_E2E_TOL = 4.8e-9
FD_RANK_DEFICIENT_VS_SQRTM = 2.7e-9      # a record, not a bound


def make_inputs(shape, seed):
    """(N, D) fp32: normal draws times a per-column scale in [1/e, e] plus a per-column offset of up to twice the scale"""
    N, D = shape
    rng = np.random.RandomState(seed)
    scale = np.exp(rng.uniform(-1.0, 1.0, D))
    offset = scale * rng.uniform(-2.0, 2.0, D)
    return (rng.standard_normal((N, D)) * scale + offset).astype(np.float32)


def make_exact_inputs(shape, seed):
    """(N, D) fp32, integer-valued, every column sum a multiple of N (the last row carries the adjustment)"""
    N, D = shape
    rng = np.random.RandomState(seed)
    x = rng.randint(-8, 9, (N, D)).astype(np.int64)
    r = x.sum(0) % N
    x[-1] -= np.where(r <= N // 2, r, r - N)
    assert not (x.sum(0) % N).any() and np.abs(x).max() <= 8 + N // 2 + 1
    return x.astype(np.float32)


def oracle(x):
    """(mean, cov) in numpy.longdouble"""
    xl = x.astype(LD)
    return np.mean(xl, axis=0), np.atleast_2d(np.cov(xl, rowvar=False))


def exact_expected(x):
    """(mean, cov) fp64 of an exact case: the defining formulas in numpy fp64, the covariance ending in a true division"""
    x64 = x.astype(np.float64)
    N = x.shape[0]
    mean = x64.sum(0) / N
    assert (mean == np.round(mean)).all()
    xc = x64 - mean
    return mean, (xc.T @ xc) / (N - 1)


def numpy_fp64(x):
    x64 = x.astype(np.float64)
    return np.mean(x64, axis=0), np.atleast_2d(np.cov(x64, rowvar=False))


def restatement(x, groups=16, kstep=4):
    """(mean, cov) fp64 in the kernels' order: the mean from `groups` strided row groups, each added in index order, then added in
    group order; the Gram matrix of the centred rows as rank-`kstep` updates in index order; a true division by N - 1"""
    x64 = x.astype(np.float64)
    N, D = x64.shape
    total = np.zeros(D)
    for g in range(groups):
        part = np.zeros(D)
        for row in x64[g::groups]:
            part = part + row
        total = total + part
    mean = total / N
    xc = x64 - mean
    acc = np.zeros((D, D))
    for k in range(0, N, kstep):
        blk = xc[k:k + kstep]
        acc = acc + blk.T @ blk
    return mean, acc / (N - 1)


def moment_error(got, ref):
    """the larger of max |d mean| / max |mean| and max |d cov| / max |cov| against a longdouble oracle"""
    (m, c), (mr, cr) = got, ref
    em = float(np.abs(np.asarray(m, LD) - mr).max() / max(np.abs(mr).max(), LD(np.finfo(np.float64).tiny)))
    ec = float(np.abs(np.asarray(c, LD) - cr).max() / np.abs(cr).max())
    return max(em, ec)


_REF = {}


def reference(shape):
    """inputs and longdouble oracle of a case, computed once and shared: {"x", "mean", "cov"}"""
    if shape not in _REF:
        x = make_inputs(shape, CASES[shape])
        mean, cov = oracle(x)
        x.setflags(write=False)
        _REF[shape] = {"x": x, "mean": mean, "cov": cov}
    return _REF[shape]


def fd_pair(case, seed):
    """two sets of D-dimensional codes with different column scales, offsets and a shared mixing, as make_inputs draws them:
    (x1 (N1, D), x2 (N2, D)) fp32"""
    D, n1, n2 = case
    rng = np.random.RandomState(seed)
    mix = np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D)
    out = []
    for n in (n1, n2):
        scale = np.exp(rng.uniform(-1.0, 1.0, D))
        offset = scale * rng.uniform(-2.0, 2.0, D)
        out.append(((rng.standard_normal((n, D)) * scale) @ mix + offset).astype(np.float32))
    return out


def stats64(x):
    """numpy fp64 (mean, cov) as torch-ready arrays"""
    m, c = numpy_fp64(x)
    return np.ascontiguousarray(m), np.ascontiguousarray(c)
