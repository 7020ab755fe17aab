"""Shapes, seeded inputs, oracle and measured bounds of the precision / recall / density / coverage path (csrc/mogan_knn.hip,
attngan/prdc.py), shared by tests/test_prdc_reference_cpu.py (which measures the bounds and checks the cases), tests/test_prdc_cpu.py
and tests/test_prdc_gpu.py (which apply them).

A case (N, M, D, K) is a set x of N codes, a set y of M codes, D features, and K neighbours for the radii of x (min(K, M - 1) for
those of y; none where M < 2).  Four ball problems hang on it, `problems(case)`: queries y against the balls of x and queries x
against the balls of y, each with the radius taken from the support point (side "support") and from the query (side "query"), under
the radii of the neighbours `ks(K)` (up to 4 columns).

Inputs.  fid_cases.fd_pair's two sets are offset from each other, every count between them is 0 and a kernel that writes zeros
would pass.  Here both sets are cut from ONE pool, fd_pair((D, N + M, 2), seed)[0]: x the first N rows, y the rest, and every odd
row of y pushed outward from x's column mean by the factor 1.6 (in fp32).  The decisions are then mixed: test_prdc_reference_cpu.py
asserts the shares.

Oracle.  d2(a, b) = sum_k (a_k - b_k)^2 in numpy.longdouble from the fp32 inputs widened exactly: direct differences, no Gram form.
The radii are its K smallest per row over j != i by position; the counts compare it with the radii the entry point is GIVEN (the
oracle's radii rounded to fp64, widened again), d2 <= r2.

Radii bound.  err = |got - oracle| / A, A = |a|^2 + |b|^2 + 2 sum_k |a_k b_k| of the pair the oracle's k-th neighbour is -- the
magnitude that enters the cancellation of the Gram form, so a small distance is not judged against itself.  RADII_TOL is 4 x the
largest err over CASES of two fp64 CPU evaluations: `numpy_fp64`, the Gram form in plain numpy, and `restatement`, which follows the
kernel's order -- the Gram matrix as rank-4 updates along the feature axis in index order (one K step of the fp64 MFMA each), the
norms as the diagonal of the same updates of a set against itself, (na + nb) - 2 g, clamped at 0.  MEASURED holds the figures the
CPU module printed; that module holds RADII_TOL to them and to the ceiling 1e-13 (fid_cases.MOMENT_TOL_CEILING).

Counts.  Equality with the oracle, every query, every column.  That is legitimate because the CPU module asserts
|d2 - r2| >= MARGIN * A = 1e-9 A in longdouble for every (query, support, column) of every problem of every case: four orders above
the ceiling of the radii bound, so no fp64 evaluation within the bound can decide differently.

Exact cases.  Integer-valued fp32 inputs in [-4, 4]: every product, norm and distance is an integer of magnitude 64 D <= 2^13 at
most, exact in fp64 in ANY order.  The radii must equal `numpy_fp64`'s bit for bit and the counts integer arithmetic, ties (d2 = r2,
which the CPU module asserts to occur) included.  In the first case row DUP_ROW of x occurs K + 1 times (DUP_AT) and row DUP_QUERY of
y is one more bit copy: the copies' radii are 0, they are each other's neighbours, and the query is counted by each of them.
"""
import numpy as np

import fid_cases
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import prdc as PRDCMOD  # noqa: E402

LD = np.longdouble
RADII_TOL_CEILING = fid_cases.MOMENT_TOL_CEILING
MARGIN = 1e-9
PUSH = np.float32(1.6)

# (N, M, D, K) -> seed
CASES = {
    (2, 1, 1, 1): 0,              # the smallest legal problem
    (5, 4, 16, 3): 0,
    (9, 9, 17, 5): 0,             # a D tail of 1
    (64, 64, 48, 8): 0,           # exactly one tile, K max
    (67, 100, 80, 5): 0,          # a tail of 3 in the second tile, M != N
    (130, 200, 100, 3): 0,        # three tile rows
    (96, 96, 2048, 5): 0,         # the workload's D
}
EXACT_CASES = {(67, 70, 48, 5): 1, (130, 140, 128, 8): 1}
DUP_CASE, DUP_ROW, DUP_AT, DUP_QUERY = (67, 70, 48, 5), 3, (3, 10, 20, 40, 64, 66), 7

# ---- recorded by tests/test_prdc_reference_cpu.py (it fails when a figure is exceeded or stale) ----
MEASURED = {"numpy fp64": 4.1e-16, "restatement": 1.1e-15}
RADII_TOL = 4.4e-15


def ks(K):
    """the neighbours whose radii make the columns of a case's radius tables: up to 4 of 1 .. K, 1 and K among them"""
    return sorted({1, min(2, K), (K + 1) // 2, K})


def make_inputs(case, seed):
    """(x (N, D), y (M, D)) fp32 from one pool, every odd row of y pushed outward from x's column mean (module docstring)"""
    N, M, D, K = case
    pool = fid_cases.fd_pair((D, N + M, 2), seed)[0]
    x, y = pool[:N].copy(), pool[N:].copy()
    centre = x.mean(axis=0, dtype=np.float32)
    y[1::2] = centre + PUSH * (y[1::2] - centre)
    assert x.dtype == y.dtype == np.float32
    return x, y


def make_exact_inputs(case, seed):
    """(x, y): integer-valued fp32 codes in [-4, 4]; the duplicates of DUP_CASE"""
    N, M, D, K = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-4, 5, (N, D)).astype(np.float32)
    y = rng.randint(-4, 5, (M, D)).astype(np.float32)
    if case == DUP_CASE:
        assert len(DUP_AT) == K + 1
        for i in DUP_AT:
            x[i] = x[DUP_ROW]
        y[DUP_QUERY] = x[DUP_ROW]
    return x, y


# ------------------------------------------------------------------------------------------------- distances
def oracle_d2(a, b):
    """(d2 (Na, Nb), A (Na, Nb)) in longdouble: direct differences; A = |a|^2 + |b|^2 + 2 sum |a_k b_k|"""
    a, b = a.astype(LD), b.astype(LD)
    d2 = np.empty((a.shape[0], b.shape[0]), dtype=LD)
    for i in range(a.shape[0]):
        diff = b - a[i]
        d2[i] = (diff * diff).sum(axis=1)
    mag = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] + 2 * (np.abs(a) @ np.abs(b).T)
    return d2, mag


def numpy_fp64_d2(a, b):
    """d2 (Na, Nb): the Gram form in plain numpy fp64"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    return np.maximum((na[:, None] + nb[None, :]) - 2.0 * (a @ b.T), 0.0)


def _gram4(a, b, kstep):
    acc = np.zeros((a.shape[0], b.shape[0]))
    for k in range(0, a.shape[1], kstep):
        acc = acc + a[:, k:k + kstep] @ b[:, k:k + kstep].T
    return acc


def restatement_d2(a, b, kstep=4):
    """d2 (Na, Nb) fp64 in the kernel's order (module docstring)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    na, nb = np.diag(_gram4(a, a, kstep)), np.diag(_gram4(b, b, kstep))
    return np.maximum((na[:, None] + nb[None, :]) - 2.0 * _gram4(a, b, kstep), 0.0)


# ------------------------------------------------------------------------------------------------- radii and counts
def knn_of(d2_self, K):
    """(the K smallest of every row of a set's own (n, n) distance matrix over j != i by position, ascending (n, K); their j)"""
    d = np.array(d2_self)
    n = d.shape[0]
    d[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :K]
    return np.take_along_axis(d, order, axis=1), order


def counts_of(d2, r2, side):
    """count (M, R) int64: #{ i : d2[j, i] <= r2[., c] }; d2 (M, N) queries x support; side "support": r2 (N, R), "query": (M, R)"""
    r2 = np.asarray(r2)
    if r2.ndim == 1:
        r2 = r2[:, None]
    r = r2.astype(d2.dtype)
    inside = d2[:, :, None] <= (r[None, :, :] if side == "support" else r[:, None, :])
    return inside.sum(axis=1).astype(np.int64)


def margin_of(d2, mag, r2, side):
    """the smallest |d2 - r2| / A over every (query, support, column)"""
    r2 = np.asarray(r2)
    if r2.ndim == 1:
        r2 = r2[:, None]
    r = r2.astype(d2.dtype)
    gap = np.abs(d2[:, :, None] - (r[None, :, :] if side == "support" else r[:, None, :])) / mag[:, :, None]
    return float(gap.min())


def radii_error(got, ref, mag_self, order):
    """the largest |got - oracle| / A over (row, k), A of the pair the oracle's k-th neighbour is"""
    a = np.take_along_axis(mag_self, order, axis=1)
    return float((np.abs(np.asarray(got, LD) - ref) / a).max())


def problems(case):
    """the ball problems of a case: (name, queries, support, whose radii, side) with "x" / "y" naming the sets; side "support"
    takes the radii of the support set, "query" those of the queries; y has radii where M >= 2"""
    out = [("y in the balls of x", "y", "x", "x", "support"), ("the balls of x over y", "x", "y", "x", "query")]
    if case[1] >= 2:
        out += [("x in the balls of y", "x", "y", "y", "support"), ("the balls of y over x", "y", "x", "y", "query")]
    return out


_REF = {}


def _reference(key, x, y, K):
    """everything the tests share about a pair of sets, computed once and frozen"""
    if key not in _REF:
        N, M = x.shape[0], y.shape[0]
        ref = {"x": x, "y": y, "K": {"x": K, "y": min(K, M - 1)}}
        d_xx, a_xx = oracle_d2(x, x)
        d_yx, a_yx = oracle_d2(y, x)
        ref["d2"] = {("x", "x"): d_xx, ("y", "x"): d_yx, ("x", "y"): d_yx.T}
        ref["mag"] = {("x", "x"): a_xx, ("y", "x"): a_yx, ("x", "y"): a_yx.T}
        ref["radii"], ref["order"], ref["given"] = {}, {}, {}
        ref["radii"]["x"], ref["order"]["x"] = knn_of(d_xx, K)
        if M >= 2:
            d_yy, a_yy = oracle_d2(y, y)
            ref["d2"][("y", "y")], ref["mag"][("y", "y")] = d_yy, a_yy
            ref["radii"]["y"], ref["order"]["y"] = knn_of(d_yy, ref["K"]["y"])
        for s in ref["radii"]:
            cols = [k - 1 for k in ks(ref["K"][s])]
            ref["given"][s] = np.ascontiguousarray(ref["radii"][s][:, cols].astype(np.float64))     # what the entry point is given
        ref["counts"] = {}
        for name, q, p, of, side in problems(key[0]):
            if of in ref["given"]:
                ref["counts"][name] = counts_of(ref["d2"][(q, p)], ref["given"][of], side)
        for a in [x, y] + [a for k in ("d2", "mag", "radii", "order", "given", "counts") for a in ref[k].values()]:
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def reference(case):
    """{"x", "y", "K", "d2", "mag", "radii", "order", "given", "counts"} of a case of CASES under its seed"""
    key = (case, "c")
    if key not in _REF:
        _reference(key, *make_inputs(case, CASES[case]), case[3])
    return _REF[key]


def exact_reference(case):
    """the same of a case of EXACT_CASES; every figure is an integer, so longdouble and fp64 agree to the bit"""
    key = (case, "e")
    if key not in _REF:
        _reference(key, *make_exact_inputs(case, EXACT_CASES[case]), case[3])
    return _REF[key]


# ------------------------------------------------------------------------------------------------- the four figures
def prdc_counts(real, fake, k_pr, k_dc, d2=numpy_fp64_d2):
    """(fake_in_real (n, 2), real_in_fake (n,), real_own (n,)) int64 by `d2` (plain numpy fp64 unless told otherwise): the counts
    condGANTrainer.prdc reads back, from the same five steps"""
    real_r2, _ = knn_of(d2(real, real), max(k_pr, k_dc))
    fake_r2, _ = knn_of(d2(fake, fake), k_pr)
    d_fr = d2(fake, real)
    fake_in_real = counts_of(d_fr, real_r2[:, [k_pr - 1, k_dc - 1]], "support")
    real_in_fake = counts_of(d_fr.T, fake_r2[:, k_pr - 1], "support")[:, 0]
    real_own = counts_of(d_fr.T, real_r2[:, k_dc - 1], "query")[:, 0]
    return fake_in_real, real_in_fake, real_own


def prdc_numpy(real, fake, k_pr, k_dc):
    """the four figures in numpy fp64 on a pair of code matrices"""
    return PRDCMOD.scores_from_counts(*prdc_counts(real, fake, k_pr, k_dc), k_dc=k_dc)


def prdc_margin(real, fake, k_pr, k_dc):
    """the smallest |d2 - r2| / A in longdouble over every decision behind prdc_counts"""
    d_rr, _ = oracle_d2(real, real)
    d_ff, _ = oracle_d2(fake, fake)
    d_fr, a_fr = oracle_d2(fake, real)
    real_r2, _ = knn_of(d_rr, max(k_pr, k_dc))
    fake_r2, _ = knn_of(d_ff, k_pr)
    return min(margin_of(d_fr, a_fr, real_r2[:, [k_pr - 1, k_dc - 1]], "support"),
               margin_of(d_fr.T, a_fr.T, fake_r2[:, k_pr - 1], "support"),
               margin_of(d_fr.T, a_fr.T, real_r2[:, k_dc - 1], "query"))
